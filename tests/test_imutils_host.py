"""CPU: tuch_amd.utils.imutils, tuch_amd.augment and the crop records of tuch_amd.ops against values recorded from the
reference's own functions (tests/golden/imutils.npz, written by tests/golden/make_golden_imutils.py) and against the
closed form of the resampling rule (tests/image_cases.py)."""
import functools
import sys
import types

import numpy as np
import pytest

import golden_io as gio
import image_cases as ic

J24 = [5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 15, 16, 17, 18, 19, 21, 20, 23, 22]
J49 = [0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21] + [25 + i for i in J24]


@functools.lru_cache(maxsize=None)
def golden():
    data = gio.load('imutils.npz')
    return {k: data[k] for k in data.files}


def handed_arrays(g):
    """Per kept crop draw: the array the reference handed to resize (rot = 0) or rotate, [h, w, C] uint8."""
    sizes = g['crop_handed_shape'].prod(1)
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [g['crop_handed'][off[k]:off[k + 1]].reshape(g['crop_handed_shape'][k]) for k in range(len(sizes))]


def table_for(images):
    """IMAGE_TABLE + packed bytes without a device (ops.pack_images needs one only for the copy)."""
    from tuch_amd import ops
    buf, table = ops.pack_images(images, device='cpu')
    return buf.numpy(), table


# ------------------------------------------------------------------------------------------------ transforms
def test_transform_integers_and_matrix_equal_the_reference():
    from tuch_amd.utils import imutils
    g = golden()
    for k, (cx, cy, s, rot, res) in enumerate(g['gt_params']):
        res = [int(res), int(res)]
        t = imutils.get_transform([cx, cy], s, res, rot=rot)
        assert np.abs(t - g['gt_matrix'][k]).max() <= 1e-12 * max(1.0, np.abs(g['gt_matrix'][k]).max()), k
        pts = g['gt_points'][k]
        assert np.array_equal(imutils.transform_points(pts, [cx, cy], s, res, rot=rot), g['gt_forward'][k]), k
        assert np.array_equal(imutils.transform_points(pts, [cx, cy], s, res, invert=1, rot=rot), g['gt_inverse'][k]), k
        for p in (0, len(pts) - 1):
            assert np.array_equal(imutils.transform(pts[p], [cx, cy], s, res, rot=rot), g['gt_forward'][k, p])
            assert np.array_equal(imutils.transform(pts[p], [cx, cy], s, res, invert=1, rot=rot), g['gt_inverse'][k, p])


def test_crop_records_carry_the_reference_box_and_pad():
    from tuch_amd import ops
    g = golden()
    assert len(g['crop_draws']) >= 100 and int(g['crop_skipped'][0]) >= 1
    images = [g['image_%d' % k] for k in range(5)]
    _, table = table_for(images)
    for k, (img, cx, cy, s, rot, res) in enumerate(g['crop_draws']):
        rec = ops.crop_records(table[int(img)], [[cx, cy]], [s], [rot], [0], None, int(res))[0]
        ulx, uly, brx, bry, pad = g['crop_boxes'][k]
        p = int(pad) if rot != 0 else 0
        assert (rec['ox'], rec['oy']) == (ulx - p, uly - p), k
        assert (rec['pw'], rec['ph']) == (brx - ulx + 2 * p, bry - uly + 2 * p), k
        # the array the reference built has exactly that shape
        assert tuple(g['crop_handed_shape'][k][:2]) == (rec['ph'], rec['pw']), k
        assert rec['K'] == min(max(-(-max(brx - ulx, bry - uly) // int(res)), 1), 16)
    ragged = ops.crop_records(table[2], [[3.2, 28.7]], [0.2], [0], [0], None, 16)[0]
    assert (ragged['pw'], ragged['ph'], ragged['K']) == (39, 40, 3)


def test_a_box_without_area_raises():
    from tuch_amd import ops
    _, table = table_for([np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(ValueError):
        ops.crop_records(table, [[2.5, 2.5]], [1e-4], [0], [0], None, 8)


# ------------------------------------------------------------------------------------------------ flips, processing
def test_flip_functions_equal_the_reference():
    from tuch_amd.utils import imutils
    g = golden()
    assert np.array_equal(imutils.flip_kp(g['flip_kp24_in'].copy()), g['flip_kp24_out'])
    assert np.array_equal(imutils.flip_kp(g['flip_kp49_in'].copy()), g['flip_kp49_out'])
    assert np.array_equal(imutils.flip_pose(g['flip_pose_in'].copy()), g['flip_pose_out'])
    img = np.arange(24).reshape(2, 4, 3)
    assert np.array_equal(imutils.flip_img(img), img[:, ::-1])


def test_derived_permutations_equal_the_tables_and_are_involutions():
    from tuch_amd.utils import imutils
    j24, j49 = imutils.derived_flip_perms()
    assert j24 == J24 and j49 == J49
    for perm in (j24, j49):
        assert [perm[i] for i in perm] == list(range(len(perm)))
    # the data folder's constants win when they are importable
    mods = {k: sys.modules.get(k) for k in ('data', 'data.essentials', 'data.essentials.constants')}
    try:
        for name in mods:
            sys.modules[name] = types.ModuleType(name)
            sys.modules[name].__path__ = []
        sys.modules['data.essentials.constants'].J24_FLIP_PERM = list(reversed(range(24)))
        sys.modules['data.essentials.constants'].J49_FLIP_PERM = list(reversed(range(49)))
        assert imutils.flip_perms() == (list(reversed(range(24))), list(reversed(range(49))))
    finally:
        for name, mod in mods.items():
            if mod is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = mod
    assert imutils.flip_perms() == (J24, J49)


def test_processing_functions_equal_the_reference():
    from tuch_amd.augment import RegressorInput
    g = golden()
    ri = RegressorInput(img_res=224)
    c, s, r, f = g['proc_center'], g['proc_scale'], g['proc_rot'], g['proc_flip']
    assert (r == 0).any() and (r != 0).any() and f.min() == 0 and f.max() == 1
    for key in ('proc_kp', 'proc_kp32'):
        got = ri.j2d_processing(g[key], c, s, r, f)
        assert got.dtype == np.float32 and np.array_equal(got, g[key + '_out']), key
    # the reference never applies its rotation to the 3D joints (base_dataset.py:223-233): kept
    got = ri.j3d_processing(g['proc_S'], r, f)
    assert got.dtype == np.float32 and np.array_equal(got, g['proc_S_out'])
    assert np.array_equal(ri.j3d_processing(g['proc_S'][:, :, :3], r, f), g['proc_S3_out'])
    unflipped = np.nonzero((f == 0) & (r != 0))[0]
    assert len(unflipped) and np.array_equal(got[unflipped], g['proc_S'][unflipped].astype(np.float32))
    # poses: 1e-6 away from rotation angle pi (there the two conventions pick opposite axes)
    got = ri.pose_processing(g['proc_pose'], r, f)
    want = g['proc_pose_out']
    away = np.abs(np.linalg.norm(want[:, :3], axis=1) - np.pi) > 1e-3
    assert away.sum() >= len(want) - 2
    assert got.dtype == np.float32 and np.abs(got[away] - want[away]).max() <= 1e-6


def test_rot_aa_equals_the_reference_away_from_pi():
    from tuch_amd.utils import imutils
    g = golden()
    want = g['rot_aa_out']
    got = np.stack([imutils.rot_aa(a.copy(), r) for a, r in zip(g['rot_aa_in'], g['rot_aa_rot'])])
    away = np.abs(np.linalg.norm(want, axis=1) - np.pi) > 1e-3
    assert away.sum() >= len(want) - 2
    assert np.abs(got[away] - want[away]).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ augmentation parameters
def test_augm_params_bounds_order_and_no_augmentation():
    from tuch_amd.augment import RegressorInput
    opt = types.SimpleNamespace(noise_factor=0.4, rot_factor=30, scale_factor=0.25)
    ri = RegressorInput(opt, is_train=True)
    flip, pn, rot, sc = ri.augm_params(2000, np.random.default_rng(3))
    assert set(np.unique(flip)) == {0, 1} and 0.4 < flip.mean() < 0.6
    assert pn.shape == (2000, 3) and pn.min() >= 0.6 and pn.max() <= 1.4
    assert np.abs(rot).max() <= 60 and 0.5 < (rot == 0).mean() < 0.7
    assert sc.min() >= 0.75 and sc.max() <= 1.25 and (sc == 1.25).any()
    # the reference's order of draws, restated on the same generator
    g = np.random.default_rng(11)
    want_flip = int(g.uniform() <= 0.5)
    want_pn = g.uniform(0.6, 1.4, 3)
    want_rot = min(60, max(-60, g.standard_normal() * 30))
    want_sc = min(1.25, max(0.75, g.standard_normal() * 0.25 + 1))
    if g.uniform() <= 0.6:
        want_rot = 0
    flip, pn, rot, sc = ri.augm_params(1, np.random.default_rng(11))
    assert (flip[0], rot[0], sc[0]) == (want_flip, want_rot, want_sc) and np.array_equal(pn[0], want_pn)
    for kw in (dict(is_train=False), dict(use_augmentation=False)):
        flip, pn, rot, sc = RegressorInput(opt, **kw).augm_params(5, np.random.default_rng(3))
        assert not flip.any() and np.all(pn == 1) and not rot.any() and np.all(sc == 1)


# ------------------------------------------------------------------------------------------------ the integer records
def _record_cases():
    rng = np.random.default_rng(5)
    cases = [((3.2, 28.7), 0.2, 0.0, 0, 16), ((3.2, 28.7), 0.2, 30.0, 1, 16), ((400.0, 1.5), 0.68, 0.0, 0, 8),
             ((375.5, 550.0), 4.48, 30.0, 1, 224), ((375.5, 550.0), 4.48, -77.5, 0, 224), ((20.0, 15.0), 0.04, 90.0, 0, 8),
             ((-250.0, 2000.0), 17.0, 59.0, 1, 224)]
    for _ in range(40):
        res = int(rng.choice([8, 16, 224]))
        cases.append((tuple(rng.uniform(-200, 1200, 2)), float(rng.uniform(0.03, 8.0)),
                      float(rng.choice([0.0, rng.uniform(-60, 60)])), int(rng.integers(0, 2)), res))
    return cases


def test_records_stay_within_2_to_the_minus_12_px_of_the_closed_form():
    from tuch_amd import ops
    _, table = table_for([np.zeros((750, 1101, 3), np.uint8)])
    worst = 0.0
    for center, scale, rot, flip, res in _record_cases():
        rec = ops.crop_records(table, [center], [scale], [rot], [flip], None, res)[0]
        ul, br, _ = ops.crop_box(center, scale, rot, res)
        pixels = None if res <= 16 else [(i, j) for i in (0, 1, 111, 222, 223) for j in (0, 1, 112, 223)]
        x, y = ic.closed_form(ul, br, rot, flip, res, int(rec['K']), pixels)
        rx, ry = ic.record_positions(rec, res, pixels)
        worst = max(worst, np.abs(rx - x).max(), np.abs(ry - y).max())
    assert worst <= 2.0 ** -12, worst
    assert worst >= 2.0 ** -40           # (positions are snapped to 2^-16 px: a zero would mean nothing was compared)


def test_records_outside_the_packed_buffer_are_rejected():
    from tuch_amd import ops
    buf, table = table_for([np.zeros((10, 12, 3), np.uint8), np.zeros((6, 5, 1), np.float32)])
    good = ops.crop_records(table, [[5, 5], [2, 2]], [0.05, 0.05], [0, 0], [0, 0], None, 8)
    ops.check_crop_records(good, buf.size, 3)
    for field, index, value in (('offset', 1, buf.size - 8), ('offset', 0, -1), ('height', 0, 11 + buf.size // 36),
                                ('stride', 0, 35), ('stride', 1, 22), ('width', 0, 13), ('channels', 0, 2), ('type', 0, 2),
                                ('K', 0, 0), ('K', 0, 17), ('offset', 1, int(table['offset'][1]) + 2), ('pw', 0, 0),
                                ('ox', 0, 1 << 30)):
        bad = good.copy()
        bad[field][index] = value
        with pytest.raises(ValueError):
            ops.check_crop_records(bad, buf.size, 3)
    with pytest.raises(ValueError):                 # a 3-channel source into a 1-channel output
        ops.check_crop_records(good, buf.size, 1)
    with pytest.raises(ValueError):                 # the buffer is shorter than the table says
        ops.check_crop_records(good, buf.size - 1, 3)


def test_pack_images_places_every_image_where_the_table_says():
    from tuch_amd import ops
    rng = np.random.default_rng(2)
    images = [rng.integers(0, 256, (3, 5, 3)).astype(np.uint8), rng.normal(size=(4, 3)).astype(np.float32),
              rng.integers(0, 256, (1, 1, 1)).astype(np.uint8)]
    buf, table = table_for(images)
    assert table.dtype == ops.IMAGE_TABLE and list(table['channels']) == [3, 1, 1] and list(table['type']) == [0, 1, 0]
    assert all(o % 16 == 0 for o in table['offset']) and table['stride'][0] == 16 and table['stride'][1] == 12
    for img, t in zip(images, table):
        a = img.reshape(img.shape[0], -1)
        rows = buf[t['offset']:t['offset'] + t['height'] * t['stride']].reshape(t['height'], t['stride'])
        assert np.array_equal(rows[:, :a.shape[1] * a.itemsize].copy().view(a.dtype), a)


def test_the_float64_restatement_reproduces_the_reference_geometry():
    """tests/image_cases.py on the records = the array the reference handed to resize, at the identity scale (no device)."""
    from tuch_amd import ops
    g = golden()
    images = [g['image_%d' % k] for k in range(5)]
    buf, table = table_for(images)
    arrays = handed_arrays(g)
    seen = 0
    for k, (img, cx, cy, s, rot, res) in enumerate(g['crop_draws']):
        res = int(res)
        if rot != 0 or s != res / 200.0:
            continue
        want = arrays[k].astype(np.float64)
        if want.shape[:2] != (res, res):            # truncation toward zero left a side of R - 1: not the identity
            continue
        rec = ops.crop_records(table[int(img)], [[cx, cy]], [s], [0], [0], None, res)[0]
        raw, _ = ic.crop_from_records(buf, rec, res, [0.0] * 3, [1.0] * 3)
        ch = want.shape[2]
        assert np.array_equal(np.round(raw.reshape(3, res, res)[:ch] * 255.0, 9), want.transpose(2, 0, 1)), k
        seen += 1
    assert seen >= 22


# ------------------------------------------------------------------------------------------------ compat
def test_install_imutils_is_opt_in():
    from tuch_amd import compat
    import tuch_amd.utils.imutils as ours
    before = list(sys.meta_path), {k: v for k, v in sys.modules.items() if k == 'tuch' or k.startswith('tuch.')}
    try:
        compat.uninstall()
        compat.install()
        assert sys.modules.get('tuch.utils.imutils') is not ours
        assert compat._finder.find_spec('tuch.utils.imutils') is None          # left to the checkout
        assert compat.install_imutils() == ['tuch.utils.imutils']
        import importlib
        assert importlib.import_module('tuch.utils.imutils') is ours
        from tuch.utils.imutils import crop, flip_kp, transform                 # noqa: F401
        assert 'tuch.utils.renderer' not in compat._enabled
        compat.uninstall()
        assert 'tuch.utils.imutils' not in sys.modules and compat._finder.find_spec('tuch.utils.imutils') is None
    finally:
        compat.uninstall()
        sys.meta_path[:] = before[0]
        sys.modules.update(before[1])


def test_binding_declares_the_entry_point():
    from tuch_amd import _C, ops
    assert 'tuch_crop_batch' in _C.exported_symbols()
    assert ops.CROP_RECORD.itemsize == 120
    assert _C.lib().tuch_abi_version() == _C.ABI_VERSION == 3
