"""GPU: the batched crop (csrc/image_crop.hip, tuch_amd.ops.crop_batch, tuch_amd.augment, tuch_amd.utils.imutils.crop) against
the float64 restatement of its rule (tests/image_cases.py) on the same integer records, against the arrays the reference's
own crop() built (tests/golden/imutils.npz) and against the reference's keypoint transform.

Tolerance against the oracle, in ``raw`` (values in [0,1]): (K^2 + 16) 2^-24.  The texels are integers up to 255 and the
weights frac / 65536 are exact, every term is non-negative, so only the float32 products and the fixed-order sums round,
each by at most 2^-24 of a value that is at most 255 (1 after the division): 6 roundings in a bilinear sample, K^2 - 1 adds
whose partial sums average half the total (K^2 / 2), the division by K^2, the product with pn (<= 1.4 before the clamp)
and the division by 255 -- about 0.7 K^2 + 10 in units of 2^-24.  ``out`` divides by std: the bound divided by min(std).
float32 sources: the same bound times max|value| / 255.  Observed maxima are logged with helpers.report_value; on the
device the largest error was 0.152 of the bound (the full-size case), and a bright texel landed within 0.87 px of the
reference's keypoint (bound 1.75 px).
"""
import functools

import numpy as np
import pytest
import torch

import golden_io as gio
import image_cases as ic
from helpers import report_value

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


@functools.lru_cache(maxsize=None)
def golden():
    data = gio.load('imutils.npz')
    return {k: data[k] for k in data.files}


def golden_images():
    g = golden()
    return [g['image_%d' % k] for k in range(5)]


def handed_arrays(g):
    sizes = g['crop_handed_shape'].prod(1)
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [g['crop_handed'][off[k]:off[k + 1]].reshape(g['crop_handed_shape'][k]) for k in range(len(sizes))]


def run(buf, rec, res, mean=MEAN, std=STD):
    """-> (out, raw) numpy [B,C,R,R] float32."""
    from tuch_amd import ops
    out, raw = ops.crop_batch(buf, rec, res, mean, std, raw=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), raw.cpu().numpy()


def crop_samples(images, samples, res, mean=MEAN, std=STD, row_align=4, narrow=()):
    """samples: (image index, center, scale, rot, flip, pn).  narrow: sample indices whose image is declared 3 texels
    narrower than it was packed (rows then lie `stride` apart with unused bytes between).  -> out, raw, bytes, records."""
    from tuch_amd import ops
    buf, table = ops.pack_images(images, device=DEV, row_align=row_align)
    tab = table[[s[0] for s in samples]].copy()
    for k in narrow:
        tab['width'][k] -= 3
    rec = ops.crop_records(tab, [s[1] for s in samples], [s[2] for s in samples], [s[3] for s in samples],
                           [s[4] for s in samples], [s[5] for s in samples], res)
    out, raw = run(buf, rec, res, mean, std)
    return out, raw, buf.cpu().numpy(), rec


def check_against_oracle(what, out, raw, host, rec, res, mean=MEAN, std=STD, pixels=None, scale_of=None):
    worst = 0.0
    for b in range(len(rec)):
        want_raw, want_out = ic.crop_from_records(host, rec[b], res, mean, std, pixels)
        k = int(rec[b]['K'])
        bound = (k * k + 16) * 2.0 ** -24 * (1.0 if scale_of is None else scale_of[b])
        got_raw, got_out = raw[b].reshape(len(mean), -1), out[b].reshape(len(mean), -1)
        if pixels is not None:
            flat = np.asarray(pixels)[:, 0] * res + np.asarray(pixels)[:, 1]
            got_raw, got_out = got_raw[:, flat], got_out[:, flat]
        e_raw, e_out = np.abs(got_raw - want_raw).max(), np.abs(got_out - want_out).max()
        worst = max(worst, e_raw / bound, e_out / (bound / min(std)))
        assert e_raw <= bound, (what, b, k, e_raw, bound)
        assert e_out <= bound / min(std), (what, b, k, e_out, bound / min(std))
    report_value('crop %s: max error / bound (raw and out)' % what, worst)


# ------------------------------------------------------------------------------------------------ 1. identity, quarter turns
def _golden_batches(select):
    """The golden crop draws picked by select(draw, handed array), grouped by R -> {R: [(k, draw)]}."""
    g = golden()
    arrays = handed_arrays(g)
    groups = {}
    for k, d in enumerate(g['crop_draws']):
        if select(d, arrays[k]):
            groups.setdefault(int(d[5]), []).append((k, d))
    return groups, arrays


def test_identity_scale_returns_the_reference_copy_bit_for_bit():
    groups, arrays = _golden_batches(lambda d, a: d[4] == 0 and d[3] == d[5] / 200.0 and a.shape[:2] == (int(d[5]),) * 2)
    seen = 0
    for res, items in groups.items():
        samples = [(int(d[0]), (d[1], d[2]), d[3], 0.0, 0, (1, 1, 1)) for _, d in items]
        _, raw, _, _ = crop_samples(golden_images(), samples, res)
        for n, (k, _) in enumerate(items):
            want = arrays[k].astype(np.float32).transpose(2, 0, 1)
            got = raw[n] * np.float32(255.0)
            assert got.dtype == np.float32 and np.array_equal(got[:want.shape[0]], want), k
            assert np.array_equal(got[0], got[2]) or want.shape[0] == 3
            seen += 1
    assert seen >= 22


def test_quarter_turns_are_exact_permutations_of_the_source_texels():
    groups, arrays = _golden_batches(lambda d, a: d[4] in (90.0, 180.0, 270.0))
    seen = 0
    for res, items in groups.items():
        samples = [(int(d[0]), (d[1], d[2]), d[3], d[4], 0, (1, 1, 1)) for _, d in items]
        _, raw, _, _ = crop_samples(golden_images(), samples, res)
        g = golden()
        for n, (k, d) in enumerate(items):
            pad = int(g['crop_boxes'][k][4])
            padded = arrays[k]                                   # the zero-padded copy the reference handed to rotate
            assert padded.shape[0] == padded.shape[1] == res + 2 * pad and pad > 0
            # the picture turns counter-clockwise by the angle (skimage.transform.rotate), then the pad is cut off
            want = np.rot90(padded, int(d[4]) // 90)[pad:-pad, pad:-pad].astype(np.float32).transpose(2, 0, 1)
            assert np.array_equal(raw[n] * np.float32(255.0), want), (k, d[4])
            seen += 1
    assert seen >= 12


# ------------------------------------------------------------------------------------------------ 2. the oracle, same records
def _sources():
    rng = np.random.default_rng(7)
    return [rng.integers(0, 256, (30, 40, 3)).astype(np.uint8),                    # 0
            rng.integers(0, 256, (23, 17, 1)).astype(np.uint8),                    # 1
            rng.uniform(0, 255, (12, 31, 3)).astype(np.float32),                   # 2
            rng.uniform(0, 255, (7, 5, 1)).astype(np.float32),                     # 3
            rng.integers(0, 256, (1, 1, 3)).astype(np.uint8),                      # 4
            rng.integers(0, 256, (3, 800, 3)).astype(np.uint8),                    # 5: the strip
            np.full((9, 11, 3), 250, np.uint8)]                                    # 6: bright, for the saturating noise


ONE = (1.0, 1.0, 1.0)
PN = (0.7, 1.0, 1.35)
ORACLE_CASES = {
    # one batch of 5: sizes, strides, types, channel counts
    'mixed': (16, 16, (0, 2), [(0, (20.0, 15.0), 0.12, 0.0, 0, PN), (1, (8.0, 11.0), 0.1, 30.0, 1, ONE),
                               (2, (15.5, 6.0), 0.07, -77.5, 0, PN), (3, (2.0, 3.0), 0.04, 0.0, 1, ONE),
                               (0, (5.0, 25.0), 0.2, 30.0, 1, PN)]),
    # K = 1, 2, 3 and the cap: box sides 8, 16, 24 and >= 136 at R = 8
    'K': (8, 4, (), [(0, (20.0, 15.0), 0.04, 0.0, 0, ONE), (0, (20.0, 15.0), 0.08, 0.0, 0, PN),
                     (0, (20.0, 15.0), 0.12, 30.0, 1, PN), (5, (400.0, 1.5), 0.68, 0.0, 0, ONE),
                     (5, (300.0, 1.0), 0.75, -77.5, 1, PN), (0, (20.0, 15.0), 0.03, 0.0, 0, ONE)]),
    'rot': (16, 4, (), [(0, (20.0, 15.0), 0.1, r, f, PN) for r in (0.0, 30.0, -77.5) for f in (0, 1)]
            + [(2, (15.0, 6.0), 0.05, r, 1, ONE) for r in (30.0, -77.5)]),
    # half outside, the ragged 39 x 40 box, a box that misses the image, the 1 x 1 image, noise that saturates
    'placement': (16, 4, (), [(0, (0.0, 15.0), 0.1, 0.0, 0, ONE), (0, (40.0, 30.0), 0.1, 30.0, 1, ONE),
                              (0, (3.2, 28.7), 0.2, 0.0, 0, PN), (0, (3.2, 28.7), 0.2, 30.0, 1, PN),
                              (0, (200.0, 200.0), 0.1, 0.0, 0, ONE), (0, (-90.0, 15.0), 0.2, 30.0, 0, ONE),
                              (4, (0.5, 0.5), 0.02, 0.0, 0, PN), (4, (0.0, 1.0), 0.05, 30.0, 1, ONE),
                              (6, (5.0, 4.0), 0.05, 0.0, 0, (1.4, 1.02, 0.6)), (6, (5.0, 4.0), 0.08, 30.0, 1, (1.4, 1.4, 1.4))]),
}


@pytest.mark.parametrize('name', sorted(ORACLE_CASES))
def test_against_the_float64_oracle_on_the_same_records(name):
    res, align, narrow, samples = ORACLE_CASES[name]
    images = _sources()
    out, raw, host, rec = crop_samples(images, samples, res, row_align=align, narrow=narrow)
    scale_of = [max(float(np.abs(images[s[0]]).max()) / 255.0, 2.0 ** -10) if images[s[0]].dtype == np.float32 else 1.0
                for s in samples]
    check_against_oracle(name, out, raw, host, rec, res, scale_of=scale_of)
    if name == 'K':
        assert list(rec['K']) == [1, 2, 3, 16, 16, 1]
        assert rec['pw'][3] >= 136
    if name == 'mixed':
        assert sorted(set(rec['type'])) == [0, 1] and sorted(set(rec['channels'])) == [1, 3]
        assert rec['stride'][0] > rec['width'][0] * 3 and len(set(rec['stride'])) >= 3
        assert np.array_equal(raw[1][0], raw[1][1]) and np.array_equal(raw[1][0], raw[1][2])      # grey fills every channel
    if name == 'placement':
        assert (rec['pw'][2], rec['ph'][2]) == (39, 40)
        for b in (4, 5):                                         # the box misses the image: zeros, not an error
            assert not raw[b].any()
            assert np.allclose(out[b], (-np.array(MEAN) / np.array(STD))[:, None, None], rtol=0, atol=1e-6)
        assert raw[8][0].max() == 1.0 and raw[9].max() == 1.0    # 250 x 1.4 saturates at 255
        assert raw[8][2].max() < 0.6
    assert raw.min() >= 0.0 and raw.max() <= 1.0


def test_one_output_channel_and_an_empty_batch():
    from tuch_amd import ops
    images = _sources()
    samples = [(1, (8.0, 11.0), 0.1, 30.0, 1, ONE), (3, (2.0, 3.0), 0.04, 0.0, 0, PN)]
    out, raw, host, rec = crop_samples(images, samples, 8, mean=[0.45], std=[0.225])
    assert out.shape == (2, 1, 8, 8)
    check_against_oracle('one channel', out, raw, host, rec, 8, mean=[0.45], std=[0.225],
                         scale_of=[1.0, float(images[3].max()) / 255.0])
    buf, table = ops.pack_images(images, device=DEV)
    empty = ops.crop_batch(buf, np.zeros(0, ops.CROP_RECORD), 8, MEAN, STD)
    assert empty.shape == (0, 3, 8, 8)
    with pytest.raises(ValueError):                              # a 3-channel source cannot go into one channel
        ops.crop_batch(buf, ops.crop_records(table[:1], [[5, 5]], [0.1], [0], [0], None, 8), 8, [0.45], [0.225])
    bad = ops.crop_records(table[:1], [[5, 5]], [0.1], [0], [0], None, 8)
    bad['offset'] = buf.numel() - 10                             # would address past the buffer: refused on the host
    with pytest.raises(ValueError):
        ops.crop_batch(buf, bad, 8, MEAN, STD)


# ------------------------------------------------------------------------------------------------ 3. sense of rotation, flip
@pytest.mark.parametrize('rot', [30.0, -45.0, 60.0, 0.0])
def test_sense_of_rotation_and_flip_follow_the_reference_keypoint_map(rot):
    from tuch_amd.utils import imutils
    res, scale, center = 16, 0.16, (20.0, 15.0)
    kps = [(30, 15), (20, 5), (12, 22), (27, 8)]                  # texels 4 or more source pixels from the centre
    samples, images = [], []
    for kp in kps:
        for flip in (0, 1):
            img = np.zeros((30, 40, 1), np.uint8)
            img[kp[1], kp[0]] = 255
            images.append(img)
            samples.append((len(images) - 1, center, scale, rot, flip, ONE))
    _, raw, _, _ = crop_samples(images, samples, res)
    bound = 1.5 * res / (200 * scale) + 1
    worst = 0.0
    for n, (_, _, _, _, flip, _) in enumerate(samples):
        kp = np.array(kps[n // 2], np.float64)
        assert np.linalg.norm(kp - center) >= 4
        want = imutils.transform(kp + 1, center, scale, [res, res], rot=rot).astype(np.float64)     # as j2d_processing calls it
        if flip:
            want[0] = res - want[0]
        assert raw[n][0].sum() > 0, n
        got = np.array(ic.centroid(raw[n][0]))
        worst = max(worst, np.linalg.norm(got - want))
        assert np.linalg.norm(got - want) <= bound, (n, got, want)
    report_value('crop rot %g: centroid to keypoint distance, worst (bound %.2f px)' % (rot, bound), worst)


# ------------------------------------------------------------------------------------------------ 4. batches, graphs
def test_batch_independence_repeatability_graph_replay_and_no_synchronisation():
    from tuch_amd import ops
    images = _sources()
    res = 16
    samples = ORACLE_CASES['mixed'][3] + ORACLE_CASES['placement'][3][:4]
    buf, table = ops.pack_images(images, device=DEV)
    tab = table[[s[0] for s in samples]]
    args = ([s[1] for s in samples], [s[2] for s in samples], [s[3] for s in samples], [s[4] for s in samples],
            [s[5] for s in samples])
    rec = ops.crop_records(tab, *args, res)
    first = [t.clone() for t in ops.crop_batch(buf, rec, res, MEAN, STD, raw=True)]
    again = ops.crop_batch(buf, rec, res, MEAN, STD, raw=True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    only_out = ops.crop_batch(buf, rec, res, MEAN, STD)
    assert torch.equal(only_out, first[0])
    for b in range(len(samples)):                                 # alone, and at another position of another batch
        alone = ops.crop_batch(buf, rec[b:b + 1], res, MEAN, STD, raw=True)
        assert torch.equal(alone[0][0], first[0][b]) and torch.equal(alone[1][0], first[1][b]), b
    order = np.arange(len(samples))[::-1].copy()
    turned = ops.crop_batch(buf, rec[order], res, MEAN, STD, raw=True)
    assert torch.equal(turned[0], first[0][torch.as_tensor(order, device=DEV)])
    # uploaded records: one launch, no host synchronisation
    dev_rec = ops.upload_crop_records(buf, rec)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        quiet = ops.crop_batch(buf, dev_rec, res, MEAN, STD, raw=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(quiet[0], first[0]) and torch.equal(quiet[1], first[1])
    # graph replay on other pixels and other records
    static_buf, static_rec = buf.clone(), ops.upload_crop_records(buf, rec)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.crop_batch(static_buf, static_rec, res, MEAN, STD, raw=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.crop_batch(static_buf, static_rec, res, MEAN, STD, raw=True)
    other_images = [255 - im if im.dtype == np.uint8 else (255.0 - im) for im in images]
    other_buf, other_table = ops.pack_images(other_images, device=DEV)
    assert np.array_equal(other_table, table)
    other_rec = ops.upload_crop_records(other_buf, rec[order])
    want = [t.clone() for t in ops.crop_batch(other_buf, other_rec, res, MEAN, STD, raw=True)]
    static_buf.copy_(other_buf)
    static_rec.tensor.copy_(other_rec.tensor)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    assert not torch.equal(want[1], first[1])


# ------------------------------------------------------------------------------------------------ 5. full size
def test_full_size_batch_against_the_oracle_on_a_strided_subset():
    rng = np.random.default_rng(3)
    shapes = [(448, 600), (750, 1101), (600, 448), (500, 800)]
    images = []
    for h, w in shapes:                                           # smooth + noise: neighbouring texels differ, no flat areas
        ys, xs = np.mgrid[0:h, 0:w]
        base = 127 + 80 * np.sin(xs / 37.0)[..., None] * np.cos(ys[..., None] / 23.0 + np.arange(3))
        images.append(np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8))
    samples = [(0, (300.0, 224.0), 2.1, 0.0, 0, PN), (1, (550.5, 375.0), 3.6, 30.0, 1, ONE),
               (2, (100.0, 500.0), 1.12, -77.5, 0, PN), (3, (700.0, 40.0), 4.3, 12.5, 1, PN)]
    out, raw, host, rec = crop_samples(images, samples, 224)
    assert list(rec['K']) == [2, 4, 1, 4]
    pixels = [(i, j) for i in list(range(0, 224, 9)) + [223] for j in list(range(0, 224, 7)) + [223]]
    check_against_oracle('full size', out, raw, host, rec, 224, pixels=pixels)
    assert raw.std() > 0.05


# ------------------------------------------------------------------------------------------------ 6. the product level
def test_regressor_input_and_imutils_crop():
    import types
    from tuch_amd import ops
    from tuch_amd.augment import RegressorInput
    from tuch_amd.utils import imutils
    rng = np.random.default_rng(9)
    res = 16
    images = [rng.integers(0, 256, (30, 40, 3)).astype(np.uint8), rng.integers(0, 256, (23, 17, 3)).astype(np.uint8),
              rng.uniform(0, 255, (12, 31, 3)).astype(np.float32)]
    center = np.array([[20.0, 15.0], [8.0, 12.0], [15.0, 6.0]])
    scale = np.array([0.15, 0.1, 0.06])
    opt = types.SimpleNamespace(noise_factor=0.4, rot_factor=30, scale_factor=0.25)
    ri = RegressorInput(opt, img_res=res, is_train=True, device=DEV)
    flip, pn, rot, sc = ri.augm_params(3, np.random.default_rng(4))
    flip[:], rot[:] = [1, 0, 1], [rot[0] if rot[0] else 25.0, 0.0, -40.0]
    img, raw = ri.rgb_processing(images, center, sc * scale, rot, flip, pn, raw=True)
    torch.cuda.synchronize()
    assert img.shape == (3, 3, res, res) and img.dtype == torch.float32 and img.device.type == 'cuda'
    buf, table = ops.pack_images(images, device=DEV)
    rec = ops.crop_records(table, center, sc * scale, rot, flip, pn, res)
    check_against_oracle('RegressorInput', img.cpu().numpy(), raw.cpu().numpy(), buf.cpu().numpy(), rec, res,
                         scale_of=[1.0, 1.0, float(images[2].max()) / 255.0])
    # annotations: the batch functions equal the per-sample functions of the host tests
    kp = np.concatenate([rng.uniform(0, 40, (3, 49, 2)), rng.uniform(0, 1, (3, 49, 1))], 2)
    S = np.concatenate([rng.normal(0, 0.5, (3, 24, 3)), np.ones((3, 24, 1))], 2)
    pose = rng.normal(0, 0.5, (3, 72))
    got_kp, got_S, got_pose = ri.j2d_processing(kp, center, sc * scale, rot, flip), ri.j3d_processing(S, rot, flip), \
        ri.pose_processing(pose, rot, flip)
    for b in range(3):
        one = kp[b].copy()
        for i in range(49):
            one[i, 0:2] = imutils.transform(one[i, 0:2] + 1, center[b], sc[b] * scale[b], [res, res], rot=rot[b])
        one[:, :-1] = 2. * one[:, :-1] / res - 1.
        one = imutils.flip_kp(one) if flip[b] else one
        assert np.array_equal(got_kp[b], one.astype('float32'))
        assert np.array_equal(got_S[b], (imutils.flip_kp(S[b].copy()) if flip[b] else S[b]).astype('float32'))
        p = pose[b].copy()
        p[:3] = imutils.rot_aa(p[:3], rot[b])
        assert np.array_equal(got_pose[b], (imutils.flip_pose(p) if flip[b] else p).astype('float32'))
    # demo: (img in [0,1], normalised [1,3,R,R]); imutils.crop on uint8 gives [0,1], HWC float64
    shown, norm = RegressorInput(img_res=res, device=DEV).process_image(images[0], bbox=[4, 3, 30, 24])
    assert shown.shape == (3, res, res) and norm.shape == (1, 3, res, res)
    assert float(shown.min()) >= 0 and float(shown.max()) <= 1 and float(shown.max()) > 0.5
    back = norm[0] * torch.tensor(STD, device=DEV)[:, None, None] + torch.tensor(MEAN, device=DEV)[:, None, None]
    assert torch.allclose(back, shown, atol=1e-6)
    c = imutils.crop(images[0], [20.0, 15.0], 0.15, [res, res], rot=20)
    assert c.shape == (res, res, 3) and c.dtype == np.float64 and c.min() >= 0 and 0.5 < c.max() <= 1
    cf = imutils.crop(images[2], [15.0, 6.0], 0.04, [8, 8])
    assert cf.shape == (8, 8, 3) and cf.max() > 1.5              # float input keeps its range
