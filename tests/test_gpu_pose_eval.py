"""GPU: pose evaluation on the device (csrc/pose_eval.hip) against the reference's own results
(tests/golden/make_golden_pose_eval.py: tuch/utils/pose_utils.py on synthetic joint sets, eval.py's numbers on seeded
meshes that tests/pose_eval_cases.py regenerates), plus determinism across batch compositions, graph replay and the
Evaluator's chunked accumulation.

Tolerances, set from the observed maxima (logged through helpers.report_value): float64 joint sets 1e-9 absolute; float32
ones 1e-5 relative + 1e-6 m (the reference solves those in float32, we in float64); mesh metrics 1e-5 relative + 2e-6 m
(float32 regression of 6890 vertices)."""
import os

import numpy as np
import pytest
import torch

import pose_eval_cases as pc
from helpers import report_value

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'pose_eval.npz'))
CASES = [str(c) for c in G['joint_cases']]
DEV = torch.device('cuda:0')


def close(got, want, f32, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    d = np.abs(got[~nan] - want[~nan])
    bound = (1e-5 * np.abs(want[~nan]) + 1e-6) if f32 else np.full(d.shape, 1e-9)
    report_value('pose_eval %-40s max |d|' % what, float(d.max()) if d.size else 0.0)
    assert np.all(d <= bound), (what, float(d.max()))


@pytest.mark.parametrize('case', CASES)
def test_joint_sets_match_the_reference(case):
    from tuch_amd.utils.pose_utils import compute_similarity_transform_batch, reconstruction_error
    S1, S2 = G[case + '_S1'], G[case + '_S2']
    f32 = S1.dtype == np.float32
    hat = compute_similarity_transform_batch(S1, S2)
    assert isinstance(hat, np.ndarray) and hat.dtype == G[case + '_hat'].dtype and hat.shape == S1.shape
    close(hat, G[case + '_hat'], f32, case + ' S1_hat')
    re = reconstruction_error(S1, S2, reduction=None)
    assert isinstance(re, np.ndarray) and re.dtype == G[case + '_re'].dtype and re.shape == (S1.shape[0],)
    close(re, G[case + '_re'], f32, case + ' per body')
    for red in ('mean', 'sum'):
        r = reconstruction_error(S1, S2, reduction=red)
        assert np.ndim(r) == 0 and np.asarray(r).dtype == G['%s_re_%s' % (case, red)].dtype
        close(r, G['%s_re_%s' % (case, red)], f32, '%s %s' % (case, red))
    assert reconstruction_error(S1, S2).dtype == G[case + '_re_mean'].dtype          # default: 'mean'


def test_single_body_matches_the_reference():
    from tuch_amd.utils.pose_utils import compute_similarity_transform
    got = compute_similarity_transform(G['j14_f32_S1'][0], G['j14_f32_S2'][0])
    assert got.dtype == np.float64 and got.shape == (14, 3)           # the reference's R is float64
    close(got, G['single_hat'], True, 'single body (float32 in)')
    got = compute_similarity_transform(G['t3x14_S1'][0], G['t3x14_S2'][0])
    assert got.shape == (3, 14)
    close(got, G['single_t_hat'], False, 'single body [3, 14]')


@pytest.mark.parametrize('case', ['j14_f64', 'j14_f32', 'd2t', 'nan'])
def test_tensors_stay_on_the_device(case):
    from tuch_amd.utils.pose_utils import compute_similarity_transform_batch, reconstruction_error
    S1, S2 = G[case + '_S1'], G[case + '_S2']
    a, b = torch.tensor(S1, device=DEV), torch.tensor(S2, device=DEV)
    hat = compute_similarity_transform_batch(a, b)
    re = reconstruction_error(a, b, reduction=None)
    m = reconstruction_error(a, b)
    assert hat.device == a.device and re.device == a.device and m.device == a.device and m.dim() == 0
    assert hat.dtype == a.dtype and re.dtype == a.dtype
    # the same kernel as the numpy path: the same bits
    np.testing.assert_array_equal(hat.cpu().numpy(), compute_similarity_transform_batch(S1, S2))
    np.testing.assert_array_equal(re.cpu().numpy(), reconstruction_error(S1, S2, reduction=None))


def mesh_inputs(name):
    _, seed, B, V, R, jmap, kind = next(c for c in pc.MESH_CASES if c[0] == name)
    pred, gt, reg, gt_joints = pc.mesh_case(seed, B, V, R, len(jmap))
    t = lambda x: torch.tensor(x, device=DEV)                                            # noqa: E731
    gt_kw = {'gt_vertices': t(gt)} if kind == 'vertices' else {'gt_joints': t(gt_joints)}
    return t(pred), gt_kw, t(reg), torch.tensor(jmap, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize('name', [c[0] for c in pc.MESH_CASES])
def test_mesh_metrics_match_the_reference(name):
    from tuch_amd.eval import pose_errors
    pred, gt_kw, reg, jmap = mesh_inputs(name)
    out = pose_errors(pred, reg, jmap.tolist(), return_joints=True, **gt_kw)
    want_keys = {'mpjpe', 'pa_mpjpe', 'joints'} | ({'v2v'} if 'gt_vertices' in gt_kw else set())
    assert set(out) == want_keys
    for k in want_keys:
        assert out[k].device == pred.device and out[k].dtype == torch.float32
        g = G['mesh_%s_%s' % (name, k)]
        got = out[k].cpu().numpy()
        d = np.abs(got - g)
        report_value('pose_eval mesh %-30s %-8s max |d|' % (name, k), float(d.max()))
        assert np.all(d <= 1e-5 * np.abs(g) + 2e-6), (name, k, float(d.max()))


def test_same_body_same_bits_in_any_batch():
    from tuch_amd.eval import pose_errors
    from tuch_amd.utils.pose_utils import reconstruction_error
    pred, gt_kw, reg, jmap = mesh_inputs('h36m_j14_v6890')
    gt = gt_kw['gt_vertices']
    ref = {k: v.cpu().numpy() for k, v in pose_errors(pred, reg, jmap, gt_vertices=gt, return_joints=True).items()}
    rng = np.random.default_rng(0)
    for B in (1, 7, 64, 300):
        idx = torch.tensor(rng.integers(0, pred.shape[0], B), device=DEV)
        out = pose_errors(pred[idx].contiguous(), reg, jmap, gt_vertices=gt[idx].contiguous(), return_joints=True)
        for k, v in out.items():
            np.testing.assert_array_equal(v.cpu().numpy(), ref[k][idx.cpu().numpy()], err_msg='%s at batch %d' % (k, B))
    S1 = np.random.default_rng(1).standard_normal((300, 14, 3))
    S2 = S1[:, ::-1] * 1.3 + np.random.default_rng(2).standard_normal((300, 14, 3)) * 0.05
    full = reconstruction_error(S1, S2, reduction=None)
    for B in (1, 7, 64):
        p = rng.permutation(300)[:B]
        np.testing.assert_array_equal(reconstruction_error(S1[p], S2[p], reduction=None), full[p])


def test_graph_replay_bit_identical_to_eager():
    from tuch_amd.eval import pose_errors
    pred, gt_kw, reg, jmap = mesh_inputs('h36m_j14_v6890')
    gt = gt_kw['gt_vertices']
    eager = {k: v.clone() for k, v in pose_errors(pred, reg, jmap, gt_vertices=gt, return_joints=True).items()}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                          # warm-up off the capture
        pose_errors(pred, reg, jmap, gt_vertices=gt, return_joints=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = pose_errors(pred, reg, jmap, gt_vertices=gt, return_joints=True)
    for v in out.values():
        v.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(out[k], eager[k]), k
    # replays see new inputs in place
    pred.mul_(1.01)
    g.replay()
    fresh = pose_errors(pred, reg, jmap, gt_vertices=gt)
    torch.cuda.synchronize()
    assert torch.equal(out['mpjpe'], fresh['mpjpe']) and torch.equal(out['pa_mpjpe'], fresh['pa_mpjpe'])


def test_evaluator_chunks_equal_one_call():
    from tuch_amd.eval import Evaluator, pose_errors, validation_metrics
    pred, gt_kw, reg, jmap = mesh_inputs('h36m_j14_v6890')
    gt = gt_kw['gt_vertices']
    one = pose_errors(pred, reg, jmap, gt_vertices=gt, return_joints=True)
    ev = Evaluator(reg.cpu().numpy(), jmap.tolist(), capacity=100, return_joints=True)
    cuts = [0, 1, 8, 9, 40, 64]
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert ev.add(pred[a:b], gt_vertices=gt[a:b]) == (a, b)
    r = ev.results()
    assert set(r) == {'mpjpe', 'pa_mpjpe', 'v2v', 'joints'} and ev.count == 64
    for k in r:
        np.testing.assert_array_equal(r[k], one[k].cpu().numpy(), err_msg=k)
    cnc = np.where(np.arange(64) % 3 == 0, np.inf, np.linspace(0, 0.03, 64))
    s = ev.summary(cnc=cnc)
    assert s['n_contact'] + s['n_no_contact'] + s['n_unclear'] == 64
    assert s['recon_err'] == pytest.approx(1000 * r['pa_mpjpe'].astype(np.float64).mean(), rel=1e-12)
    name = 'h36m_j14_v6890'
    assert s['mpjpe'] == pytest.approx(1000 * G['mesh_%s_mpjpe' % name].mean(), rel=1e-5)
    vm = validation_metrics([gt[:10], gt[10:]], [pred[:10], pred[10:]], reg, jmap.tolist())
    assert set(vm) == {'mpjpe', 'v2v'}
    assert vm == validation_metrics(gt, pred, reg, jmap.tolist())
    assert vm['v2v'] == pytest.approx(1000 * G['mesh_%s_v2v' % name].mean(), rel=1e-5)
    with pytest.raises(ValueError):
        ev.add(pred, gt_vertices=gt)                                    # 64 + 64 > capacity
