"""GPU: fitting SMPL to unregistered points.  The hinted closest-point search (csrc/closest_point.hip:
tuch_closest_point with a hint) against the unhinted one, bit for bit, for every kind of hint; the data term (csrc/scan_fit.hip)
against the float64 statements of tests/scan_fit_cases.py; fit.ScanFitter against the float64 loop there.

Observed on an MI355X (2026-10-19): term error / bound at most 0.022 ('squared'), 7.6e-5 ('distance'), 4.8e-4 ('gmof');
gradients at most 0.15 of the bound; the fitter's parameters over the first 20 updates 0.03 - 0.25 of the bound, its loss ratios
at most 1.009 x the float64 loop's.  DESIGN.md section 3, "Fit to unregistered points"."""
import functools

import numpy as np
import pytest
import torch

import closest_point_cases as cc
import helpers
import scan_fit_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MESHES = ('triangle', 'strip', 'tetrahedron', 'icosphere', 'degenerate', 'body122')


def _dev(a, **kw):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV, **kw)


@functools.lru_cache(maxsize=None)
def model(name):
    from tuch_amd.ops import ContactModel
    return ContactModel(cc.mesh(name)[1], device=DEV)


def _same(a, b, what):
    for field, x, y in zip(a._fields, a, b):
        assert torch.equal(x, y), (what, field)


# ---------------------------------------------------------------------------------------------------------- the search
def _check_all_hints(name, c, counts=None):
    m = model(name)
    verts, points = _dev(c['verts']), _dev(c['points'])
    dcounts = None if counts is None else _dev(np.asarray(counts, np.int32))
    plain = m.closest_point(verts, points, dcounts)
    answer = plain.face.cpu().numpy()
    for kind in sc.HINT_KINDS:
        hint = sc.hints(kind, c['points'], c['verts'], c['faces'], answer)
        _same(plain, m.closest_point(verts, points, dcounts, hint=_dev(hint)), (name, kind))
    return plain


@pytest.mark.parametrize('count', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('name', MESHES)
def test_hinted_search_equals_unhinted_for_every_hint(name, batch, count):
    c = cc.case(name, batch, count)
    plain = _check_all_hints(name, c)
    # (and the unhinted call is still the statement's: the face it names attains the float64 minimum within the bound)
    face = plain.face.cpu().numpy()
    for b in range(batch):
        via_face = cc.face_d2(c['points'][b], c['verts'][b], c['faces'], face[b])
        assert np.all(np.abs(via_face - c['ref']['d2'][b]) <= c['ref']['bound'][b])


@pytest.mark.parametrize('name', ['strip', 'icosphere', 'body122'])
def test_hinted_search_with_ragged_counts(name):
    c = cc.case(name, 3, 257)
    for counts in ([257, 0, 65], [1000, -5, 64], [130, 63, 1]):
        plain = _check_all_hints(name, c, counts)
        n = np.clip(counts, 0, 257)
        face = plain.face.cpu().numpy()
        for b in range(3):
            assert np.all(face[b, n[b]:] == -1) and np.all(face[b, :n[b]] >= 0)


@pytest.mark.parametrize('name', ['strip', 'icosphere', 'body122'])
def test_hint_may_alias_the_face_output(name):
    """The C call with face == hint: every lane reads its hint before it writes its face."""
    from tuch_amd import _C, ops
    c = cc.case(name, 3, 257)
    m = model(name)
    verts, points, counts = _dev(c['verts']), _dev(c['points']), _dev(np.array([257, 40, 130], np.int32))
    plain = m.closest_point(verts, points, counts)
    L = _C.lib()
    nbytes = L.tuch_closest_point_workspace_bytes(m._handle, 3, 257, 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for kind in sc.HINT_KINDS:
        both = _dev(sc.hints(kind, c['points'], c['verts'], c['faces'], plain.face.cpu().numpy()))
        d2, bary = torch.empty_like(plain.d2), torch.empty_like(plain.bary)
        _C.check(L.tuch_closest_point(m._handle, _C.ptr(verts), _C.ptr(points), None, 0.0, _C.ptr(counts), _C.ptr(both), 3, 257,
                                      _C.ptr(d2), _C.ptr(both), _C.ptr(bary), _C.ptr(ws), nbytes, _C.stream()))
        _same(plain, ops.ClosestPoint(d2, both, bary), (name, kind))
        # and once more from what it left: the loop's own use
        _C.check(L.tuch_closest_point(m._handle, _C.ptr(verts), _C.ptr(points), None, 0.0, _C.ptr(counts), _C.ptr(both), 3, 257,
                                      _C.ptr(d2), _C.ptr(both), _C.ptr(bary), _C.ptr(ws), nbytes, _C.stream()))
        _same(plain, ops.ClosestPoint(d2, both, bary), (name, kind, 'again'))


@pytest.mark.parametrize('name', ['strip', 'body122'])
def test_nan_body_with_valid_hints_leaves_the_others_alone(name):
    c = cc.case(name, 3, 257)
    m = model(name)
    clean = m.closest_point(_dev(c['verts']), _dev(c['points']))
    hint = _dev(clean.face.cpu().numpy())
    for rows in (slice(None, None, 5), slice(None)):                # some vertices, then nothing finite at all
        verts = c['verts'].copy()
        verts[1, rows] = np.nan
        plain = m.closest_point(_dev(verts), _dev(c['points']))
        got = m.closest_point(_dev(verts), _dev(c['points']), hint=hint)
        for b in (0, 2):
            for field, x, y in zip(clean._fields, clean, got):
                assert torch.equal(x[b], y[b]), (name, field, b)
        face = got.face.cpu().numpy()
        assert np.all((face >= -1) & (face < len(c['faces'])))
        # a hinted lane of that body has fallen back, not admitted nothing: wherever the unhinted call finds a face for a
        # query of the NaN body, the hinted call finds one too
        assert np.all(face[1][plain.face.cpu().numpy()[1] >= 0] >= 0)


def test_hinted_search_at_smpl_size_from_the_answer_of_a_moved_mesh():
    c = cc.case('smpl', 2, 1024)
    m = model('smpl')
    rng = np.random.default_rng(2)
    moved = (c['verts'] + 2e-3 * rng.standard_normal(c['verts'].shape)).astype(np.float32)
    before = m.closest_point(_dev(moved), _dev(c['points']))
    plain = m.closest_point(_dev(c['verts']), _dev(c['points']))
    changed = (before.face != plain.face).float().mean().item()
    helpers.report_value('closest_point hinted, smpl B=2 Q=1024: share of hints that are not the answer', changed)
    # two thirds of cc.case's queries are vertices and edge midpoints of the mesh itself, where several faces tie: any
    # movement hands those to another face.  Both kinds of hint, the right face and a near wrong one, are well represented.
    assert 0.05 < changed < 0.95
    _same(plain, m.closest_point(_dev(c['verts']), _dev(c['points']), hint=before.face), 'smpl')


def test_hint_shape_and_device_are_checked():
    from tuch_amd._C import TuchError
    c = cc.case('strip', 3, 65)
    m = model('strip')
    with pytest.raises(TuchError, match='hint'):
        m.closest_point(_dev(c['verts']), _dev(c['points']), hint=torch.zeros(3, 64, dtype=torch.int32, device=DEV))
    with pytest.raises(TuchError, match='hint'):
        m.closest_point(_dev(c['verts']), _dev(c['points']), hint=torch.zeros(3, 65, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------- the term
def _term(m, c, points=None, weights='case', counts='case', hint=None, grad_points=True, scale=None, verts=None):
    """ops.scan_fit on a case + one backward pass: dict of numpy (per, total, gv, gt, gp) and the ClosestPoint."""
    from tuch_amd import ops
    v = _dev(c['verts'] if verts is None else verts, requires_grad=True)
    tr = _dev(c['transl'], requires_grad=True)
    p = _dev(c['points'] if points is None else points, requires_grad=grad_points)
    w = _dev(c['weights']) if isinstance(weights, str) else weights
    n = _dev(c['counts']) if isinstance(counts, str) else counts
    total, per, near = ops.scan_fit(m, v, tr, p, n, w, hint, c['rho'], c['sigma'])
    assert total.dim() == 0 and per.shape == (v.shape[0],) and not per.requires_grad and not near.d2.requires_grad
    if scale is None:
        ops.backward_scalar(total)
    else:
        (scale * total).backward()
    out = dict(per=per.cpu().numpy(), total=total.item(), gv=v.grad.cpu().numpy(), gt=tr.grad.cpu().numpy(),
               gp=p.grad.cpu().numpy() if grad_points else None)
    return out, near


@pytest.mark.parametrize('rho', sc.RHOS)
@pytest.mark.parametrize('count', [64, 65, 257])
@pytest.mark.parametrize('name', ['icosphere', 'body122'])
def test_term_matches_float64(name, count, rho):
    """per_body and total within 4 x the error of the float32 numpy restatement (floored: cc.bounds' floor carried through
    rho); the ClosestPoint is closest_point's on the shifted points, bit for bit."""
    c = sc.term_case(name, 3, count, rho)
    m = model(name)
    got, near = _term(m, c)
    err = np.abs(got['per'].astype(np.float64) - c['ref'][0])
    helpers.report_value('scan_fit %s Q=%d %s: largest per-body error / bound' % (name, count, rho), (err / c['bound']).max())
    print('scan_fit', name, count, rho, 'per_body error', err, 'bound', c['bound'])
    assert np.all(err <= c['bound']), (err, c['bound'])
    assert abs(got['total'] - c['ref'][1]) <= c['bound'].sum()
    shifted = _dev(c['points']) - _dev(c['transl'])[:, None]
    _same(m.closest_point(_dev(c['verts']), shifted, _dev(c['counts'])), near, (name, count, rho))
    # a hint changes nothing, and face_out may be the hint tensor
    from tuch_amd import ops
    both = near.face.clone()
    total, per, again = ops.scan_fit(m, _dev(c['verts']), _dev(c['transl']), _dev(c['points']), _dev(c['counts']), None, both,
                                     c['rho'], c['sigma'], face_out=both)
    assert again.face is both
    _same(near, again, 'hinted')
    assert total.item() == got['total'] and np.array_equal(per.cpu().numpy(), got['per'])


def test_term_at_batch_65_with_two_chunks_matches_float64():
    """65 bodies x 257 points: two workgroups per body, and 4 x 65 = 260 (body, component) sums for the 256 threads of the
    workgroup that arrives last -- the second trip of its loop, which a batch of 3 never takes.  per_body and total by the
    rule of test_term_matches_float64; the last body's sums, the ones of the second trip, have the bits of that body alone."""
    c = sc.term_case('icosphere', 65, 257, 'distance')
    m = model('icosphere')
    got, _ = _term(m, c)
    err = np.abs(got['per'].astype(np.float64) - c['ref'][0])
    print('scan_fit batch 65: largest per-body error / bound', (err / c['bound']).max())
    assert np.all(err <= c['bound']), (err, c['bound'])
    assert abs(got['total'] - c['ref'][1]) <= c['bound'].sum()
    last = dict(c, **{k: c[k][64:] for k in ('verts', 'points', 'transl', 'counts')})
    alone, _ = _term(m, last)
    for key in ('per', 'gt', 'gv', 'gp'):
        assert np.array_equal(got[key][64:], alone[key]), key


@pytest.mark.parametrize('rho', sc.RHOS)
def test_term_weighted_matches_float64(rho):
    c = sc.term_case('icosphere', 3, 257, rho, weighted=True)
    got, _ = _term(model('icosphere'), c)
    err = np.abs(got['per'].astype(np.float64) - c['ref'][0])
    print('scan_fit weighted', rho, 'per_body error', err, 'bound', c['bound'])
    assert np.all(err <= c['bound']), (err, c['bound'])
    assert abs(got['total'] - c['ref'][1]) <= c['bound'].sum()


@pytest.mark.parametrize('rho', sc.RHOS)
@pytest.mark.parametrize('name', ['icosphere', 'body122'])
def test_gradients_against_central_differences(name, rho):
    from tuch_amd import ops
    c = sc.grad_case(name, rho)
    sc.assert_interior_with_margin(c['points'], c['transl'], c['verts'], c['faces'])
    m = model(name)
    for mode in (True, False):
        with ops.deterministic_mode(mode):
            got, _ = _term(m, c)
        for key, what in (('gp', 'points'), ('gt', 'transl'), ('gv', 'verts')):
            ok, ratio = sc.grad_within(got[key], c[key])
            helpers.report_value('scan_fit %s %s grad_%s, deterministic=%d: error / bound' % (name, rho, what, mode), ratio)
            assert ok, (name, rho, what, mode, ratio)
        # the translation moves every query the other way
        ok, ratio = sc.grad_within(got['gt'], -got['gp'].astype(np.float64).sum(1))
        assert ok, (name, rho, mode, ratio)
    with ops.deterministic_mode(True):
        scaled, _ = _term(m, c, scale=2.5)                          # a non-unit upstream gradient scales all three
    for key in ('gp', 'gt', 'gv'):
        ok, ratio = sc.grad_within(scaled[key], 2.5 * c[key])
        assert ok, (name, rho, key, ratio)


def test_zero_weight_points_with_nan_coordinates_change_nothing():
    from tuch_amd import ops
    c = sc.term_case('icosphere', 3, 257, 'distance', weighted=True)
    m = model('icosphere')
    off = c['weights'] == 0
    assert off.any() and not off.all(1).any()
    points = c['points'].copy()
    points[off] = np.nan
    points[0, np.nonzero(off[0])[0][0]] = np.inf
    with ops.deterministic_mode(True):
        clean, _ = _term(m, c)
        dirty, _ = _term(m, c, points=points)
    for key in ('per', 'total', 'gv', 'gt'):
        assert np.array_equal(clean[key], dirty[key]), key
    assert np.all(np.isfinite(dirty['gp'])) and not dirty['gp'][off].any()
    assert np.array_equal(clean['gp'][~off], dirty['gp'][~off])


def test_bodies_without_weight_or_points_give_zero():
    c = sc.term_case('icosphere', 3, 257, 'gmof', weighted=True)
    m = model('icosphere')
    weights = c['weights'].copy()
    weights[2] = 0.0
    counts = np.array([257, 0, 100], np.int32)
    points = c['points'].copy()
    points[1] = np.nan                                              # a body without points: nothing of it is read
    got, near = _term(m, c, points=points, weights=_dev(weights), counts=_dev(counts))
    assert got['per'][0] > 0 and got['per'][1] == 0.0 and got['per'][2] == 0.0 and got['total'] == got['per'][0]
    for key in ('gv', 'gt', 'gp'):
        assert np.all(np.isfinite(got[key])), key
        assert not got[key][1].any() and not got[key][2].any() and got[key][0].any(), key
    assert np.all(near.face.cpu().numpy()[1] == -1)
    # above Q and below 0 are clamped
    full, _ = _term(m, c, counts=_dev(np.array([1000, -3, 257], np.int32)))
    assert full['per'][1] == 0.0 and full['per'][0] == got['per'][0]


def test_deterministic_mode_gives_equal_bits_twice_and_alone():
    from tuch_amd import ops
    from tuch_amd.ops._base import _ticket
    for rho in ('distance', 'gmof'):
        c = sc.term_case('body122', 3, 257, rho, weighted=True)
        m = model('body122')
        with ops.deterministic_mode(True):
            first, second, third = _term(m, c)[0], _term(m, c)[0], _term(m, c)[0]      # the third finds the second's ticket
            for key in first:
                assert np.array_equal(first[key], second[key]) and np.array_equal(first[key], third[key]), key
            for b in range(3):                                      # a body alone
                one = dict(c, verts=c['verts'][b:b + 1], transl=c['transl'][b:b + 1], points=c['points'][b:b + 1],
                           weights=c['weights'][b:b + 1], counts=c['counts'][b:b + 1])
                alone, _ = _term(m, one)
                assert alone['per'][0] == first['per'][b] and alone['total'] == first['per'][b]
                assert np.array_equal(alone['gv'][0], first['gv'][b]) and np.array_equal(alone['gt'][0], first['gt'][b])
                assert np.array_equal(alone['gp'][0], first['gp'][b])
    assert int(_ticket(torch.device(DEV)).item()) == 0


def test_term_workspace_guards_and_capture():
    from tuch_amd import ops
    from tuch_amd.ops import ContactModel
    c = sc.term_case('body122', 3, 257, 'distance')
    guarded = ContactModel(c['faces'], device=DEV)
    guarded.set_option('canary', 1)
    assert guarded.canary_selftest() == 1
    guarded.canary_hits()
    with ops.deterministic_mode(True):
        want, near = _term(model('body122'), c)
        got, _ = _term(guarded, c)
        assert guarded.canary_hits() == 0
        for key in want:
            assert np.array_equal(want[key], got[key]), key
        # captured and replayed: the same bits
        v, tr, p, n = _dev(c['verts']), _dev(c['transl']), _dev(c['points']), _dev(c['counts'])
        hint = torch.full((3, 257), -1, dtype=torch.int32, device=DEV)
        m = model('body122')
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.scan_fit(m, v, tr, p, n, None, hint, 'distance', face_out=hint)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            total, per, out = ops.scan_fit(m, v, tr, p, n, None, hint, 'distance', face_out=hint)
        hint.fill_(-1)
        for _ in range(2):                                          # the second replay starts from the first's faces
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(per.cpu().numpy(), want['per']) and total.item() == want['total']
            _same(near, out, 'replay')


def test_term_argument_errors():
    from tuch_amd import ops
    c = sc.term_case('icosphere', 3, 64, 'distance')
    m = model('icosphere')
    v, tr, p = _dev(c['verts']), _dev(c['transl']), _dev(c['points'])
    with pytest.raises(ValueError, match='rho'):
        ops.scan_fit(m, v, tr, p, rho='huber')
    with pytest.raises(ValueError, match='sigma'):
        ops.scan_fit(m, v, tr, p, rho='gmof')
    with pytest.raises(ValueError, match='transl'):
        ops.scan_fit(m, v, tr[:2], p)
    with pytest.raises(ValueError, match='verts'):
        ops.scan_fit(m, v[:, :-1], tr, p)
    with pytest.raises(ValueError, match='weights'):
        ops.scan_fit(m, v, tr, p, weights=torch.ones(3, 63, device=DEV))
    with pytest.raises(RuntimeError, match='HIP device'):
        ops.scan_fit(m, v.cpu(), tr, p)


# ---------------------------------------------------------------------------------------------------------- the fitter
@pytest.fixture(scope='module')
def smpl():
    from tuch_amd.models.smpl import SMPL
    return SMPL(model_data=sc.fit_inputs()['body'], batch_size=sc.FIT_BATCH).to(DEV)


@functools.lru_cache(maxsize=None)
def body_model():
    from tuch_amd.ops import ContactModel
    return ContactModel(sc.fit_inputs()['faces'], device=DEV)           # no geodesic mask


def _fit(smpl, num_iters, points=None, fit_global_orient=False, **kw):
    from tuch_amd.fit import ScanFitter
    c = sc.fit_inputs()
    go = sc.perturbed_orient() if fit_global_orient else c['global_orient']
    fitter = ScanFitter(smpl, body_model(), num_iters=num_iters, fit_global_orient=fit_global_orient, **kw)
    return fitter, fitter(_dev(c['points'] if points is None else points), _dev(go), counts=_dev(c['counts']))


@pytest.mark.parametrize('rho, fit_global_orient', [('distance', False), ('squared', False), ('distance', True)])
def test_trajectory_follows_the_float64_loop(smpl, rho, fit_global_orient):
    """(a) the parameters before each of the first updates against the float64 loop, within 4 x the float32 CPU loop's own
    deviation, floored at 1e-4."""
    prefix, bound = sc.trajectory_bound(rho, fit_global_orient)
    assert prefix >= 5, prefix
    ref = sc.fit_reference(sc.FIT_PREFIX, rho, fit_global_orient)
    fitter, _ = _fit(smpl, sc.FIT_PREFIX, fit_global_orient=fit_global_orient, rho=rho, record_history=True)
    history = fitter.history['fit']
    assert len(history) == sc.FIT_PREFIX
    worst = 0.0
    for it in range(prefix):
        dev = max(float(np.abs(g.cpu().numpy().astype(np.float64) - w).max())
                  for g, w in zip(history[it]['params'], ref['params'][it]))
        worst = max(worst, dev / bound[it])
        assert dev <= bound[it], (it, dev, bound[it])
    helpers.report_value('ScanFitter %s orient=%d: parameters vs float64 over %d iterations, error / bound'
                         % (rho, fit_global_orient, prefix), worst)
    np.testing.assert_allclose(history[0]['loss'].item(), ref['loss'][0].sum(), rtol=1e-4)


@pytest.mark.parametrize('rho, fit_global_orient', [('distance', False), ('squared', False), ('gmof', False), ('distance', True)])
def test_fit_reduces_the_loss_like_the_float64_loop(smpl, rho, fit_global_orient):
    """(b) final / initial loss of every body after 60 iterations at most 1.25 x the float64 loop's."""
    ref = sc.fit_reference(sc.FIT_ITERS, rho, fit_global_orient)
    want = ref['final_loss'] / ref['loss'][0]
    sigma = sc.SIGMA if rho == 'gmof' else None
    _, start = _fit(smpl, 0, fit_global_orient=fit_global_orient, rho=rho, sigma=sigma)
    fitter, fit = _fit(smpl, sc.FIT_ITERS, fit_global_orient=fit_global_orient, rho=rho, sigma=sigma)
    assert fitter.graph_replayed == {'fit': sc.FIT_ITERS - 3}
    np.testing.assert_allclose(start.loss.cpu().numpy(), ref['loss'][0], rtol=1e-4)
    ratio = (fit.loss / start.loss).cpu().numpy()
    print('ScanFitter', rho, fit_global_orient, 'ratio', ratio, 'float64', want)
    helpers.report_value('ScanFitter %s orient=%d: largest ratio / float64 ratio (bound %.2f)'
                         % (rho, fit_global_orient, sc.RATIO_MARGIN), (ratio / want).max())
    assert np.all(ratio <= sc.RATIO_MARGIN * want), (ratio, want)
    # what is returned belongs together
    c = sc.fit_inputs()
    verts = smpl(global_orient=fit.global_orient, body_pose=fit.body_pose, betas=fit.betas).vertices
    assert torch.equal(verts + fit.transl[:, None], fit.vertices)
    near = body_model().closest_point(verts, _dev(c['points']) - fit.transl[:, None], _dev(c['counts']))
    assert torch.equal(near.face, fit.face) and torch.equal(near.bary, fit.bary)
    assert fit.face.shape == (3, sc.FIT_POINTS) and fit.bary.shape == (3, sc.FIT_POINTS, 3)
    assert torch.equal(fit.global_orient, _dev(c['global_orient'])) != fit_global_orient


def test_hint_graph_and_sessions_change_no_bit(smpl, monkeypatch):
    """(c) use_hint on and off, (d) replayed and eager, (e) a kept session on other points and a fresh fitter: equal bits
    in deterministic mode."""
    from tuch_amd import ops
    from tuch_amd.fit import ScanFitter
    monkeypatch.setenv('TUCH_GRAPH_STRICT', '1')
    c = sc.fit_inputs()
    points, go, counts = _dev(c['points']), _dev(c['global_orient']), _dev(c['counts'])
    kept = (points.clone(), go.clone(), counts.clone())
    rng = np.random.default_rng(3)
    moved = (c['points'] + 0.01 * rng.standard_normal(c['points'].shape)).astype(np.float32)
    for b, n in enumerate(c['counts']):                                 # the real points in the opposite order
        moved[b, :n] = moved[b, :n][::-1]
    other, other_counts = _dev(moved), _dev(np.array([200, 64, 100], np.int32))
    with ops.deterministic_mode(True):
        make = lambda **kw: ScanFitter(smpl, body_model(), num_iters=20, fit_global_orient=False, **kw)
        hinted = make(use_hint=True)
        assert hinted.graph_strict
        first = hinted(points, go, counts=counts)
        assert hinted.graph_replayed == {'fit': 17} and len(hinted._sessions) == 1
        for name, fit in (('use_hint=False', make(use_hint=False)(points, go, counts=counts)),
                          ('eager', make(use_hint=True, use_graph=False)(points, go, counts=counts)),
                          ('eager, use_hint=False', make(use_hint=False, use_graph=False)(points, go, counts=counts))):
            for field, a, b in zip(first._fields, first, fit):
                assert torch.equal(a, b), (name, field)
        second = hinted(other, go, counts=other_counts)                 # the kept session: replays only, hint reset
        assert hinted.graph_replayed == {'fit': 20} and len(hinted._sessions) == 1
        fresh = make(use_hint=True)(other, go, counts=other_counts)
        for field, a, b in zip(second._fields, second, fresh):
            assert torch.equal(a, b), ('kept session', field)
        assert not torch.equal(first.body_pose, second.body_pose)
    # inputs are never modified (compared as bits: the padding is NaN)
    assert torch.equal(points.view(torch.int32), kept[0].view(torch.int32)) and torch.equal(go, kept[1]) and torch.equal(counts, kept[2])


def test_fitter_shape_and_device_errors(smpl):
    from tuch_amd.fit import ScanFitter
    c = sc.fit_inputs()
    fitter = ScanFitter(smpl, body_model(), num_iters=5)
    points, go = _dev(c['points']), _dev(c['global_orient'])
    with pytest.raises(ValueError, match='points'):
        fitter(points[:, :, :2], go)
    with pytest.raises(ValueError, match='global_orient'):
        fitter(points, go[:2])
    with pytest.raises(ValueError, match='body_pose'):
        fitter(points, go, body_pose=torch.zeros(3, 72, device=DEV))
    with pytest.raises(ValueError, match='counts'):
        fitter(points, go, counts=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='weights'):
        fitter(points, go, weights=torch.ones(3, 5, device=DEV))
    with pytest.raises(RuntimeError, match='HIP device'):
        fitter(points.cpu(), go.cpu())
    with pytest.raises(ValueError, match='rho'):
        ScanFitter(smpl, body_model(), rho='huber')
    with pytest.raises(ValueError, match='sigma'):
        ScanFitter(smpl, body_model(), rho='gmof')
