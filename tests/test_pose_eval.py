"""CPU: the pose-evaluation interface (tuch_amd.utils.pose_utils, tuch_amd.eval): the reference's signatures, the compat
mapping, the subset logic of the summary, argument errors raised before any launch, and the C ABI entries.
The device results are checked in tests/test_gpu_pose_eval.py."""
import inspect
import sys

import numpy as np
import pytest
import torch


def test_signatures_match_the_reference():
    from tuch_amd.utils import pose_utils
    # tuch/utils/pose_utils.py:28, 73, 80
    assert list(inspect.signature(pose_utils.compute_similarity_transform).parameters) == ['S1', 'S2']
    assert list(inspect.signature(pose_utils.compute_similarity_transform_batch).parameters) == ['S1', 'S2']
    sig = inspect.signature(pose_utils.reconstruction_error)
    assert list(sig.parameters) == ['S1', 'S2', 'reduction']
    assert sig.parameters['reduction'].default == 'mean'
    from tuch_amd import eval as ev
    assert list(inspect.signature(ev.pose_errors).parameters) == [
        'pred_vertices', 'J_regressor', 'joint_map', 'gt_vertices', 'gt_joints', 'pelvis_index', 'return_joints']
    assert list(inspect.signature(ev.validation_metrics).parameters) == [
        'gt_vertices', 'pred_vertices', 'J_regressor', 'joint_mapper']
    assert list(inspect.signature(ev.Evaluator.summary).parameters)[1:] == ['cnc', 'euclthres_lower']


def test_compat_maps_pose_utils():
    import tuch_amd.compat as compat
    saved = {k: v for k, v in sys.modules.items() if k == 'tuch' or k.startswith('tuch.')}
    try:
        names = compat.install()
        assert 'tuch.utils.pose_utils' in names
        from tuch.utils.pose_utils import reconstruction_error, compute_similarity_transform_batch
        import tuch_amd.utils.pose_utils as ours
        assert reconstruction_error is ours.reconstruction_error
        assert compute_similarity_transform_batch is ours.compute_similarity_transform_batch
        assert 'tuch.utils.error_measures' not in compat._MAP
    finally:
        for k in [k for k in sys.modules if k == 'tuch' or k.startswith('tuch.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def print_final_result_numbers(mpjpe, recon_err, cnc, euclthres_lower=0.01):
    """eval.py:75-89, restated: the values it prints, in order."""
    out = [1000 * mpjpe.mean(), 1000 * recon_err.mean()]
    contact, no_contact = (cnc < euclthres_lower), (cnc == np.inf)
    unclear = ~(no_contact + contact)
    out += [contact.sum(), no_contact.sum(), unclear.sum()]
    with np.errstate(invalid='ignore', divide='ignore'), _quiet():          # mean of an empty subset: NaN
        out += [1000 * mpjpe[contact].mean(), 1000 * mpjpe[no_contact].mean(), 1000 * mpjpe[unclear].mean(),
                1000 * recon_err[contact].mean(), 1000 * recon_err[no_contact].mean(), 1000 * recon_err[unclear].mean()]
    return out


class _quiet:
    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter('ignore', RuntimeWarning)

    def __exit__(self, *a):
        return self._w.__exit__(*a)


KEYS = ['mpjpe', 'recon_err', 'n_contact', 'n_no_contact', 'n_unclear', 'mpjpe_contact', 'mpjpe_no_contact',
        'mpjpe_unclear', 'recon_err_contact', 'recon_err_no_contact', 'recon_err_unclear']


@pytest.mark.parametrize('kind', ['mixed', 'no_unclear', 'all_contact'])
def test_summary_matches_print_final_result(kind):
    from tuch_amd.eval import pose_summary
    rng = np.random.default_rng(3)
    n = 40
    mpjpe = rng.uniform(0.03, 0.2, n).astype(np.float32)
    recon = rng.uniform(0.02, 0.1, n).astype(np.float32)
    cnc = rng.uniform(0.0, 0.05, n)
    if kind == 'mixed':
        cnc[::3] = np.inf
        cnc[1] = 0.01                     # on the threshold: unclear
        cnc[2] = np.nan                   # neither: unclear
    elif kind == 'no_unclear':
        cnc[cnc >= 0.01] = np.inf
    else:
        cnc[:] = 0.001
    got = pose_summary(mpjpe, recon, cnc)
    assert sorted(got) == sorted(KEYS)
    want = print_final_result_numbers(mpjpe.astype(np.float64), recon.astype(np.float64), cnc)
    for k, w in zip(KEYS, want):
        if np.isnan(w):
            assert np.isnan(got[k]), k
        else:
            assert got[k] == pytest.approx(float(w), rel=1e-12), k
    assert got['n_contact'] + got['n_no_contact'] + got['n_unclear'] == n
    if kind != 'mixed':
        assert got['n_unclear'] == 0 and np.isnan(got['mpjpe_unclear']) and np.isnan(got['recon_err_unclear'])
    assert set(pose_summary(mpjpe, recon)) == {'mpjpe', 'recon_err'}


def test_argument_errors_raise_before_any_launch():
    from tuch_amd.utils import pose_utils as pu
    from tuch_amd import eval as ev
    a = np.zeros((4, 14, 3), np.float32)
    with pytest.raises(ValueError):
        pu.reconstruction_error(a, np.zeros((4, 13, 3), np.float32))
    with pytest.raises(TypeError):
        pu.reconstruction_error(a, a.astype(np.float64))
    with pytest.raises(ValueError):                       # D = 4 (first axis 14 -> points x coordinates)
        pu.reconstruction_error(np.zeros((4, 14, 4)), np.zeros((4, 14, 4)))
    with pytest.raises(ValueError):
        pu.compute_similarity_transform_batch(np.zeros((14, 3)), np.zeros((14, 3)))
    with pytest.raises(TypeError):
        pu.reconstruction_error(torch.zeros(4, 14, 3, dtype=torch.float16), torch.zeros(4, 14, 3, dtype=torch.float16))
    with pytest.raises(TypeError):
        pu.reconstruction_error(a, torch.zeros(4, 14, 3))
    reg = np.full((17, 100), 0.01, np.float32)
    pred = torch.zeros(2, 100, 3)
    jmap = list(range(14))
    with pytest.raises(ValueError):                       # joint_map out of range
        ev.pose_errors(pred, reg, [0, 17], gt_vertices=pred)
    with pytest.raises(ValueError):
        ev.pose_errors(pred, reg, [-1, 2], gt_vertices=pred)
    with pytest.raises(ValueError):                       # vertex count mismatch
        ev.pose_errors(torch.zeros(2, 99, 3), reg, jmap, gt_vertices=torch.zeros(2, 99, 3))
    with pytest.raises(ValueError):                       # gt shape
        ev.pose_errors(pred, reg, jmap, gt_vertices=torch.zeros(3, 100, 3))
    with pytest.raises(ValueError):                       # gt_joints must have len(joint_map) joints
        ev.pose_errors(pred, reg, jmap, gt_joints=torch.zeros(2, 17, 3))
    with pytest.raises(ValueError):                       # both ground truths / none
        ev.pose_errors(pred, reg, jmap, gt_vertices=pred, gt_joints=torch.zeros(2, 14, 3))
    with pytest.raises(ValueError):
        ev.pose_errors(pred, reg, jmap)
    with pytest.raises(TypeError):                        # dtype mismatch
        ev.pose_errors(pred, reg, jmap, gt_vertices=pred.double())
    with pytest.raises(TypeError):
        ev.pose_errors(pred.double(), reg, jmap, gt_vertices=pred)
    with pytest.raises(ValueError):                       # too many regressed joints
        ev.pose_errors(pred, np.zeros((25, 100), np.float32), jmap, gt_vertices=pred)
    with pytest.raises(ValueError):
        ev.pose_errors(pred, reg, jmap, gt_vertices=pred, pelvis_index=17)


def test_no_host_fallback():
    from tuch_amd.utils import pose_utils as pu
    from tuch_amd import eval as ev
    t = torch.zeros(2, 14, 3, dtype=torch.float64)          # host tensors: never computed on the host
    with pytest.raises(RuntimeError, match='no host fallback'):
        pu.reconstruction_error(t, t)
    with pytest.raises(RuntimeError, match='no host fallback'):
        ev.pose_errors(torch.zeros(2, 100, 3), np.full((17, 100), 0.01, np.float32), list(range(14)),
                       gt_vertices=torch.zeros(2, 100, 3))
    if not torch.cuda.is_available():                      # numpy inputs go to the device, when there is one
        with pytest.raises(RuntimeError, match='no host fallback'):
            pu.reconstruction_error(t.numpy(), t.numpy())


def test_abi_entries_resolve_and_validate():
    from tuch_amd import _C, _build
    _build.build()
    L = _C.lib()
    assert 'tuch_procrustes' in _C.exported_symbols() and 'tuch_pose_metrics' in _C.exported_symbols()
    assert L.tuch_procrustes(None, None, 1, 14, 3, 0, 0, None, None, None) != 0
    assert b'null pointer' in L.tuch_last_error()
    p = _C.c_void_p(16)
    assert L.tuch_procrustes(p, p, 1, 14, 4, 0, 0, None, p, None) != 0
    assert b'bad sizes' in L.tuch_last_error()
    assert L.tuch_pose_metrics(p, p, p, p, p, 1, 100, 17, 14, 0, p, p, None, None, None) != 0
    assert b'exactly one' in L.tuch_last_error()
    assert L.tuch_pose_metrics(p, p, None, p, p, 1, 100, 25, 14, 0, p, p, None, None, None) != 0
    assert b'bad sizes' in L.tuch_last_error()
    assert L.tuch_pose_metrics(p, p, None, p, p, 1, 100, 17, 14, 17, p, p, None, None, None) != 0
    assert b'pelvis_index' in L.tuch_last_error()
