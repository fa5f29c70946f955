"""GPU: fitting SMPL to target meshes -- the data term (csrc/mesh_fit.hip: vertex_fit_kernel) and the sparse transfer
(mesh_transfer_kernel) against float64, the term's conventions and reproducibility, fit.MeshFitter's trajectory against
the float64 loop of tests/mesh_fit_cases.py, convergence, the captured loop, and the conversion script."""
import os
import pickle

import numpy as np
import pytest
import torch

import helpers
import lbs_cases
import mesh_fit_cases as mc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TRAJECTORY_ATOL = 1e-4      # a wrongly signed gradient moves a parameter by lr = 1e-2 in one step: 100 x this


def _dev(a, **kw):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV, **kw)


def _term(case, weights='case'):
    """ops.vertex_fit on a case + one backward pass: (per_body, total, g_verts, g_transl) as numpy."""
    from tuch_amd import ops
    v, tr = _dev(case['verts'], requires_grad=True), _dev(case['transl'], requires_grad=True)
    total, per = ops.vertex_fit(v, tr, _dev(case['target']), _dev(case['weights']) if weights == 'case' else weights)
    assert not per.requires_grad and total.dim() == 0 and per.shape == (v.shape[0],)
    ops.backward_scalar(total)
    return per.cpu().numpy(), total.item(), v.grad.cpu().numpy(), tr.grad.cpu().numpy()


def _check_term(case, got, what):
    per, total, gv, gt = got
    rper, rtotal, rgv, rgt = case['ref']
    err = max(mc.rel_err(per, rper), mc.rel_err(total, rtotal))
    helpers.report_value('vertex_fit %s: loss rel. error (bound %.2e)' % (what, case['bound']), err)
    helpers.grad_close(gv, rgv, lbs_cases.GRAD_FLOOR, 'vertex_fit %s g_verts' % what)
    helpers.grad_close(gt, rgt, lbs_cases.GRAD_FLOOR, 'vertex_fit %s g_transl' % what)
    assert err <= case['bound'], (what, err, case['bound'])


# one lane, one wavefront, a ragged second workgroup (kChunk = 1024 > 362: the chunk boundary is in the V = 6890 case),
# more bodies than one wavefront of them
@pytest.mark.parametrize('batch', [1, 3, 65])
@pytest.mark.parametrize('num_verts', [1, 64, 257, 362])
def test_term_matches_float64(batch, num_verts):
    case = mc.term_case(batch, num_verts)
    _check_term(case, _term(case), 'B=%d V=%d' % (batch, num_verts))


def test_term_matches_float64_at_smpl_size():
    case = mc.term_case(2, 6890)
    _check_term(case, _term(case), 'B=2 V=6890')


def test_term_weighted_matches_float64():
    for batch, num_verts in ((3, 362), (2, 1500)):
        case = mc.term_case(batch, num_verts, weighted=True)
        _check_term(case, _term(case), 'weighted B=%d V=%d' % (batch, num_verts))


def test_term_non_unit_upstream_gradient_and_target_gradient():
    from tuch_amd import ops
    case = mc.term_case(3, 257)
    v, tr, tg = _dev(case['verts'], requires_grad=True), _dev(case['transl'], requires_grad=True), _dev(case['target'], requires_grad=True)
    total, _ = ops.vertex_fit(v, tr, tg)
    (2.5 * total).backward()
    helpers.grad_close(v.grad.cpu().numpy(), 2.5 * case['ref'][2], lbs_cases.GRAD_FLOOR, 'vertex_fit scaled g_verts')
    helpers.grad_close(tr.grad.cpu().numpy(), 2.5 * case['ref'][3], lbs_cases.GRAD_FLOOR, 'vertex_fit scaled g_transl')
    assert torch.equal(tg.grad, -v.grad)


def test_target_on_the_vertex_gives_a_zero_row():
    from tuch_amd import ops
    case = mc.term_case(3, 362)
    v, tr = _dev(case['verts']), _dev(case['transl'])
    hit = np.zeros((3, 362), bool)
    hit[:, ::7] = True
    hit[1] = True                                               # a whole body on its target: loss 0, every gradient 0
    tg = torch.where(_dev(hit)[:, :, None], v + tr[:, None], _dev(case['target']))      # the kernel's own sum: d = 0 exactly
    vr, trr = v.clone().requires_grad_(True), tr.clone().requires_grad_(True)
    total, per = ops.vertex_fit(vr, trr, tg)
    ops.backward_scalar(total)
    for x in (total, per, vr.grad, trr.grad):
        assert torch.isfinite(x).all()
    assert torch.equal(vr.grad[_dev(hit)], torch.zeros(int(hit.sum()), 3, device=DEV))
    assert per[1].item() == 0.0 and torch.equal(trr.grad[1], torch.zeros(3, device=DEV))
    rows = ~hit[0]
    ref = mc.term_statement(case['verts'][:1, rows], case['transl'][:1], case['target'][:1, rows], None, torch.float64)
    assert abs(per[0].item() * 362 / rows.sum() - ref[0][0]) <= case['bound'] * ref[0][0]
    assert (vr.grad[0][_dev(rows)].abs().sum(1) > 0).all()


def test_zero_weight_vertices_are_skipped_entirely():
    from tuch_amd import ops
    case = mc.term_case(3, 362, weighted=True)
    w = case['weights']
    keep = np.nonzero(w != 0)[0]
    assert 0 < len(keep) < 362
    target = case['target'].copy()
    target[:, w == 0] = np.nan
    target[0, np.nonzero(w == 0)[0][0]] = np.inf
    per, total, gv, gt = _term(dict(case, target=target))
    # the same call with those vertices removed: the same numbers (up to the order of the sums)
    v2, tr2 = _dev(case['verts'][:, keep], requires_grad=True), _dev(case['transl'], requires_grad=True)
    total2, per2 = ops.vertex_fit(v2, tr2, _dev(case['target'][:, keep]), _dev(w[keep]))
    ops.backward_scalar(total2)
    assert np.isfinite(per).all() and np.isfinite(gv).all() and np.isfinite(gt).all() and np.isfinite(total)
    assert np.array_equal(gv[:, w == 0], np.zeros((3, 362 - len(keep), 3), np.float32))
    assert np.array_equal(gv[:, keep], v2.grad.cpu().numpy())
    # (both calls are within the bound of float64, in sums of different shapes)
    np.testing.assert_allclose(per, per2.cpu().numpy(), rtol=2 * case['bound'], atol=0)
    np.testing.assert_allclose(total, total2.item(), rtol=2 * case['bound'], atol=0)
    helpers.grad_close(gt, tr2.grad.cpu().numpy(), lbs_cases.GRAD_FLOOR, 'vertex_fit g_transl, zero-weight vertices removed')
    _check_term(case, (per, total, gv, gt), 'weighted, NaN targets at weight 0')


def test_term_is_bit_reproducible_in_both_modes():
    from tuch_amd import ops
    from tuch_amd.ops._base import _ticket
    case = mc.term_case(65, 257)
    big = mc.term_case(2, 6890)
    for mode in (True, False):
        with ops.deterministic_mode(mode):
            for c in (case, big):
                first, second, third = _term(c), _term(c), _term(c)       # the third call finds the ticket the second left
                for a, b, d in zip(first, second, third):
                    assert np.array_equal(a, b) and np.array_equal(a, d)
    assert int(_ticket(torch.device(DEV)).item()) == 0


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('num_rows', [1, 65, 362])
def test_transfer_matches_float64(num_rows, batch):
    from tuch_amd import ops
    c = mc.transfer_case(num_rows, batch)
    table = ops.transfer_table((c['indptr'], c['indices'], c['data']), num_src=mc.TRANSFER_SRC)
    out = ops.mesh_transfer(table, _dev(c['src']))
    assert out.shape == (batch, num_rows, 3) and out.dtype == torch.float32
    err = mc.scaled_err(out.cpu().numpy(), c['ref'])
    helpers.report_value('mesh_transfer R=%d B=%d: error / largest entry (bound %.2e)' % (num_rows, batch, c['bound']), err)
    assert err <= c['bound']
    lengths = np.diff(c['indptr'])
    assert torch.equal(out[:, _dev(lengths == 0)], torch.zeros(batch, int((lengths == 0).sum()), 3, device=DEV))
    assert torch.equal(out, ops.mesh_transfer(table, _dev(c['src'])))
    assert torch.equal(ops.mesh_transfer(table, _dev(c['src'][0])), out[0])               # [N,3] -> [R,3]


# ---- the fit
@pytest.fixture(scope='module')
def smpl():
    from tuch_amd.models.smpl import SMPL
    return SMPL(model_data=mc.fit_inputs()['body'], batch_size=mc.FIT_BATCH).to(DEV)


def _fit(smpl, num_iters, **kw):
    from tuch_amd.fit import MeshFitter
    c = mc.fit_inputs()
    go = kw.pop('global_orient', c['global_orient'])
    fitter = MeshFitter(smpl, num_iters=num_iters, **kw)
    return fitter, fitter(_dev(c['target']), _dev(go))


def test_trajectory_follows_the_float64_loop(smpl):
    ref = mc.fit_reference(50)
    fitter, fit = _fit(smpl, 50, record_history=True)
    history = fitter.history['fit']
    assert len(history) == 50
    worst = 0.0
    for it, (got, want) in enumerate(zip(history, ref['params'])):
        for g, w in zip(got['params'], want):
            worst = max(worst, float(np.abs(g.cpu().numpy().astype(np.float64) - w).max()))
    helpers.report_value('MeshFitter: parameters before every update vs float64, 50 iterations (bound %.0e)' % TRAJECTORY_ATOL, worst)
    assert worst <= TRAJECTORY_ATOL
    # the objective before the first update is the float64 loop's
    np.testing.assert_allclose(history[0]['loss'].item(), ref['loss'][0].sum(), rtol=1e-5)
    for got, want in zip((fit.body_pose, fit.betas, fit.transl), ref['final']):
        assert np.abs(got.cpu().numpy() - want).max() <= TRAJECTORY_ATOL


def test_fit_converges(smpl):
    c = mc.fit_inputs()
    _, start = _fit(smpl, 0)
    fitter, fit = _fit(smpl, 300)
    ratio = (fit.loss / start.loss).cpu().numpy()
    helpers.report_value('MeshFitter: largest final / initial loss after 300 iterations (bound %.2f)' % mc.CONVERGED, ratio.max())
    assert fitter.graph_replayed == {'fit': 297}
    assert np.all(ratio <= mc.CONVERGED), ratio
    # what is returned belongs together: vertices = the body model at the returned parameters + the translation
    verts = smpl(global_orient=fit.global_orient, body_pose=fit.body_pose, betas=fit.betas).vertices + fit.transl[:, None]
    assert torch.equal(verts, fit.vertices)
    per = torch.norm(_dev(c['target']) - fit.vertices, dim=2).mean(1)
    np.testing.assert_allclose(fit.loss.cpu().numpy(), per.cpu().numpy(), rtol=1e-4)
    assert torch.equal(fit.global_orient, _dev(c['global_orient']))             # held fixed


def test_captured_loop_equals_eager_loop(smpl, monkeypatch):
    monkeypatch.setenv('TUCH_GRAPH_STRICT', '1')
    c = mc.fit_inputs()
    target, go = _dev(c['target']), _dev(c['global_orient'])
    kept = (target.clone(), go.clone())
    _, eager = _fit(smpl, 20, use_graph=False)
    from tuch_amd.fit import MeshFitter
    fitter = MeshFitter(smpl, num_iters=20, use_graph=True)
    assert fitter.graph_strict
    first = fitter(target, go)
    assert fitter.graph_replayed == {'fit': 17}
    for name, a, b in zip(first._fields, first, eager):
        assert torch.equal(a, b), name
    assert len(fitter._sessions) == 1
    second = fitter(target, go)                                  # the kept session: replays only
    assert fitter.graph_replayed == {'fit': 20} and len(fitter._sessions) == 1
    for name, a, b in zip(first._fields, first, second):
        assert torch.equal(a, b), name
    assert torch.equal(target, kept[0]) and torch.equal(go, kept[1])            # inputs are never modified


def test_at_most_four_captured_sessions_are_kept(smpl, monkeypatch):
    """Five batch sizes are five sessions: the first one's goes when the fifth is stored.  A kept session only replays; an
    evicted one is captured again (three eager iterations, two replays) and gives a fresh fitter's bits."""
    monkeypatch.setenv('TUCH_GRAPH_STRICT', '1')
    from tuch_amd.fit import MeshFitter
    c = mc.fit_inputs()
    target, go = _dev(c['target']), _dev(c['global_orient'])
    assert target.shape[0] == mc.FIT_BATCH == 5
    fitter = MeshFitter(smpl, num_iters=5)
    assert fitter.graph_strict and fitter.keep_sessions
    for k in range(1, 6):
        fitter(target[:k], go[:k])
        assert fitter.graph_replayed == {'fit': 2} and len(fitter._sessions) == min(k, 4)
    assert [key[0] for key in fitter._sessions] == [2, 3, 4, 5]
    fitter(target, go)
    assert fitter.graph_replayed == {'fit': 5} and len(fitter._sessions) == 4              # kept: replays only
    again = fitter(target[:1], go[:1])
    assert fitter.graph_replayed == {'fit': 2}                                              # evicted: captured again
    assert [key[0] for key in fitter._sessions] == [3, 4, 5, 1]
    fresh = MeshFitter(smpl, num_iters=5)(target[:1], go[:1])
    for name, a, b in zip(again._fields, again, fresh):
        assert torch.equal(a, b), name


def test_fit_global_orient(smpl):
    go = mc.perturbed_orient()
    _, start = _fit(smpl, 0, global_orient=go, fit_global_orient=True)
    _, fit = _fit(smpl, 300, global_orient=go, fit_global_orient=True)
    ratio = (fit.loss / start.loss).cpu().numpy()
    helpers.report_value('MeshFitter(fit_global_orient): largest final / initial loss after 300 iterations', ratio.max())
    assert np.all(ratio <= mc.CONVERGED), ratio
    assert not torch.equal(fit.global_orient, _dev(go))


def test_conversion_script(smpl, tmp_path):
    from oracle import lbs as ol
    from synthetic import random_poses
    from tuch_amd.utils.smplxtosmpl_mtp import SMPLXtoSMPL
    body = mc.fit_inputs()['body']
    nv = body.num_verts
    rng = np.random.default_rng(4)
    # the 'SMPL-X' mesh: the ico-6 body's vertices permuted, 40 of them twice; the matrix averages the copies of a vertex
    source_of = rng.permutation(np.concatenate([np.arange(nv), rng.choice(nv, 40, replace=False)]))
    matrix = np.zeros((nv, len(source_of)), np.float32)
    matrix[source_of, np.arange(len(source_of))] = 1.0
    matrix /= matrix.sum(1, keepdims=True)
    bp, go, be = random_poses(3, 21)
    bp[:, 63:] = 0.0                                            # SMPL-X has no SMPL hand joints
    m = ol.model_tensors(body, torch.float64)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    verts = ol.smpl_forward(m, t64(be), t64(bp), t64(go))[0].numpy()
    folder = tmp_path / 'mtp' / 'smplx' / 'subject'
    folder.mkdir(parents=True)
    for i in range(3):
        with open(folder / ('%04d.pkl' % i), 'wb') as f:
            pickle.dump({'vertices': verts[i][source_of].astype(np.float32), 'body_pose': bp[i:i + 1, :63],
                         'global_orient': go[i:i + 1]}, f)
    written = SMPLXtoSMPL(str(tmp_path / 'mtp'), smpl=smpl, smplx_to_smpl={'matrix': matrix}, batch_size=2, max_iterations=30)
    assert len(written) == 3
    for i in range(3):
        twin = tmp_path / 'mtp' / 'smpl' / 'subject' / ('%04d.pkl' % i)
        assert str(twin) in written and twin.exists()
        with open(twin, 'rb') as f:
            out = pickle.load(f)
        assert sorted(out) == ['betas', 'pose']
        assert out['pose'].dtype == np.float64 and out['pose'].shape == (72,)
        assert out['betas'].dtype == np.float64 and out['betas'].shape == (10,)
        assert np.array_equal(out['pose'][:3], go[i].astype(np.float64))
        assert np.all(np.isfinite(out['pose'])) and np.all(np.isfinite(out['betas']))
        # 30 iterations from the SMPL-X pose (an Adam step is about lr = 1e-2): the pose has stayed near it, the shape has moved
        assert np.abs(out['pose'][3:] - bp[i]).max() < 0.45 and np.abs(out['betas']).max() > 0
    stamps = {p: os.stat(p).st_mtime_ns for p in written}
    assert SMPLXtoSMPL(str(tmp_path / 'mtp'), smpl=smpl, smplx_to_smpl={'matrix': matrix}, batch_size=2, max_iterations=30) == []
    assert {p: os.stat(p).st_mtime_ns for p in written} == stamps
