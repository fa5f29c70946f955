"""GPU: the nearest point of a cloud (csrc/point_cloud.hip) against the brute-force statement of tests/cloud_fit_cases.py,
bit for bit -- np.array_equal on d2's bits and on the index, no tolerance, no allowed mismatch --, the model -> scan term
against its float64 statement, and fit.ScanFitter with model_to_scan against the float64 loop of the two-sided objective.

Observed on an MI355X (2026-10-20): every search case equal to brute force in all bits; term error / bound at most 2.3e-3
(the floor on d2 carried through rho is the bound); gradients at most 0.22 of the bound; the fitter's parameters over the
first 20 updates 0.045 of the bound, its loss ratios at most 1.001 x the float64 loop's; the stray-arm case 5.76 mm one-sided
against 2.87 mm two-sided.  DESIGN.md section 3, "Nearest point of a cloud; two-sided fit"."""
import functools

import numpy as np
import pytest
import torch

import cloud_fit_cases as cf
import helpers
import scan_fit_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
RESOLUTIONS = (1, 4, 64)


def _dev(a, **kw):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV, **kw)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cloud(points, counts=None, weights=None, resolution=64):
    from tuch_amd.ops import PointCloud
    return PointCloud(_dev(points), _dev(counts), _dev(weights), resolution)


def _nearest(cloud, queries, shift=None, counts=None, hint=None, tau=None):
    out = cloud.nearest(_dev(queries), _dev(shift), _dev(counts), None if hint is None else _dev(hint), tau)
    return out.d2.cpu().numpy(), out.index.cpu().numpy()


def _check(points, queries, shift=None, counts=None, weights=None, tau=None, query_counts=None, resolutions=RESOLUTIONS,
           what=''):
    """Every resolution against brute force; returns the brute-force (d2, index)."""
    want = cf.brute_force_batch(queries, points, counts, weights, shift, tau, query_counts)
    for res in resolutions:
        d2, index = _nearest(_cloud(points, counts, weights, res), queries, shift, query_counts, None, tau)
        assert np.array_equal(index, want[1]), (what, res, np.nonzero(index != want[1]))
        assert np.array_equal(_bits(d2), _bits(want[0])), (what, res)
    return want


# ---------------------------------------------------------------------------------------------------------- the search
@pytest.mark.parametrize('num_queries', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('num_points', [1, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize('batch', [1, 3])
def test_search_equals_brute_force(batch, num_points, num_queries):
    name = 'icosphere' if (num_points + num_queries) % 2 else 'body122'
    c = cf.cloud_case(name, batch, num_points, num_queries)
    d2, index = _check(c['points'], c['queries'], c['shift'], what=(name, batch, num_points, num_queries))
    assert np.all(index >= 0) and np.all(np.isfinite(d2))
    _check(c['points'], c['queries'], None, what='no shift', resolutions=(64,))


def _grid_points(g, b, steps):
    """origin + k cell per axis in float32, as the header has them: points exactly on walls and corners of body b's grid."""
    o, cell = g.origin[b].astype(F32), F32(g.cell[b])
    axes = [(o[k] + np.asarray(steps[k], F32) * cell).astype(F32) for k in range(3)]
    return np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 3).astype(F32)


@pytest.mark.parametrize('resolution', [4, 64])
def test_points_and_queries_on_cell_walls_and_corners(resolution):
    rng = np.random.default_rng(5)
    lo, hi = np.array([-0.3, 0.1, -1.0], F32), np.array([0.5, 0.9, 1.0], F32)
    anchors = np.stack([lo, hi])
    g = _cloud(anchors[None], resolution=resolution).grid()
    dims = g.dims[0]
    assert dims.max() == resolution and g.cell[0] > 0 and np.array_equal(g.origin[0], lo)
    steps = [np.unique(np.clip([0, 1, 2, d // 2, d - 1, d], 0, d)) for d in dims]
    walls = _grid_points(g, 0, steps)
    walls = np.minimum(np.maximum(walls, lo), hi)                           # (the box, hence the grid, must not change)
    mixed = walls.copy()                                                    # on a wall along one axis only
    mixed[:, 1:] = (lo + (hi - lo) * rng.random((len(walls), 3)).astype(F32))[:, 1:]
    points = np.concatenate([anchors, walls, mixed]).astype(F32)[None]
    again = _cloud(points, resolution=resolution).grid()
    assert np.array_equal(again.origin, g.origin) and np.array_equal(again.cell, g.cell) and np.array_equal(again.dims, g.dims)
    on_walls = _grid_points(g, 0, [np.arange(0, d + 1, max(d // 4, 1)) for d in dims])
    step = np.nextafter(on_walls, np.inf).astype(F32)
    queries = np.concatenate([on_walls, step, np.nextafter(on_walls, -np.inf).astype(F32), walls[::3],
                              (lo + (hi - lo) * rng.random((64, 3))).astype(F32)])[None]
    _check(points, queries, what='walls', resolutions=(resolution,))


def test_degenerate_boxes():
    rng = np.random.default_rng(6)
    queries = rng.standard_normal((2, 65, 3)).astype(F32)
    same = np.tile(np.array([0.25, -0.5, 1.5], F32), (2, 64, 1))            # a box without extent: all d2 tie, index 0 wins
    d2, index = _check(same, queries, what='coincident')
    assert np.all(index == 0)
    plane = rng.standard_normal((2, 257, 3)).astype(F32)
    plane[:, :, 2] = 0.125
    _check(plane, queries, what='plane')
    line = plane.copy()
    line[:, :, 1] = -3.0
    _check(line, queries, what='line')
    one = rng.standard_normal((2, 1, 3)).astype(F32)                        # Q = 1
    d2, index = _check(one, queries, what='one point')
    assert np.all(index == 0)


def test_scene_far_from_the_origin():
    c = cf.cloud_case('icosphere', 2, 257, 257)
    move = np.array([100.0, -100.0, 100.0], F32)
    points, queries = (c['points'] + move).astype(F32), (c['queries'] + move).astype(F32)
    d2, index = _check(points, queries, c['shift'], what='far scene')
    # coordinates of 100 m have a spacing of 7.6e-6 m: many queries see several points at the same bits
    assert len(np.unique(index)) > 100


def test_queries_a_kilometre_away_tie_in_the_bits_and_take_the_lowest_index():
    rng = np.random.default_rng(8)
    points = (0.05 * rng.standard_normal((2, 257, 3))).astype(F32)
    points[:, :, 0] = 0.0                                                   # a disc across the line of sight
    queries = np.zeros((2, 64, 3), F32)
    queries[:, :, 0] = 1000.0
    queries[:, :, 1:] = (0.01 * rng.standard_normal((2, 64, 2))).astype(F32)
    want = cf.brute_force_batch(queries, points)
    d = (queries[0, 0][None] - points[0]).astype(F32)
    sq = (d * d).astype(F32)
    e = ((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)
    assert (e == e.min()).sum() > 10                                        # the ties are there
    _check(points, queries, what='1 km')
    assert np.all(want[1] < 64)                                             # ... and low indices win them
    out = (1000.0 * rng.standard_normal((2, 64, 3))).astype(F32)            # outside the grid in every direction
    _check(points, out, what='outside')


def test_queries_in_an_empty_region_inside_the_box():
    rng = np.random.default_rng(9)
    shell = rng.standard_normal((2, 1024, 3))
    shell = (shell / np.linalg.norm(shell, axis=2, keepdims=True) * (1.0 + 0.01 * rng.standard_normal((2, 1024, 1)))).astype(F32)
    queries = (0.2 * rng.standard_normal((2, 130, 3))).astype(F32)          # ~25 cells of 1/32 m from the nearest point
    _check(shell, queries, what='hollow')


# ---------------------------------------------------------------------------------------------------------- validity
def _validity_inputs():
    c = cf.cloud_case('body122', 3, 257, 130)
    rng = np.random.default_rng(11)
    points = c['points'].copy()
    counts = np.array([257, 64, 130], np.int32)
    for b in range(3):
        points[b, counts[b]:] = np.nan
    weights = (rng.random((3, 257)) + 0.5).astype(F32)
    off = rng.random((3, 257)) < 0.25
    weights[off] = 0.0
    points[off] = np.nan
    keep = np.nonzero(~off[0])[0]
    points[0, keep[3]] = np.inf                                             # an Inf point of weight 1
    points[0, keep[4], 1] = -np.inf
    weights[0, keep[3]] = 1.0
    return c, points, counts, weights


def test_ragged_counts_zero_weights_and_non_finite_points():
    c, points, counts, weights = _validity_inputs()
    d2, index = _check(points, c['queries'], c['shift'], counts, weights, what='validity')
    for b in range(3):
        ids = cf.valid_points(points[b], counts[b], weights[b])
        assert np.all(np.isin(index[b], ids))
    _check(points, c['queries'], c['shift'], counts, None, what='counts only', resolutions=(64,))
    _check(points, c['queries'], c['shift'], np.array([1000, -5, 1], np.int32), weights, what='counts clamped', resolutions=(4,))
    # query counts: entries beyond them get -1 / +inf
    qc = np.array([130, 0, 65], np.int32)
    d2, index = _check(points, c['queries'], c['shift'], counts, weights, query_counts=qc, what='query counts', resolutions=(64,))
    assert np.all(index[1] == -1) and np.all(np.isposinf(d2[1])) and np.all(index[2, 65:] == -1) and np.all(index[2, :65] >= 0)


def test_empty_cloud_and_nan_body_leave_the_others_alone():
    c = cf.cloud_case('body122', 3, 257, 130)
    clean = _cloud(c['points']).nearest(_dev(c['queries']), _dev(c['shift']))
    counts = np.array([257, 0, 257], np.int32)
    got = _cloud(c['points'], counts).nearest(_dev(c['queries']), _dev(c['shift']))
    assert torch.all(got.index[1] == -1) and torch.all(torch.isposinf(got.d2[1]))
    for b in (0, 2):
        assert torch.equal(got.d2[b], clean.d2[b]) and torch.equal(got.index[b], clean.index[b])
    for what in ('points', 'queries', 'both'):
        points, queries = c['points'].copy(), c['queries'].copy()
        if what != 'queries':
            points[1, ::3] = np.nan
            points[1, 1::3] = np.inf
        if what != 'points':
            queries[1, ::2] = np.nan
            queries[1, 1] = np.inf
        got = _cloud(points).nearest(_dev(queries), _dev(c['shift']))
        for b in (0, 2):
            assert torch.equal(got.d2[b], clean.d2[b]) and torch.equal(got.index[b], clean.index[b]), (what, b)
        want = cf.brute_force_batch(queries, points, shift=c['shift'])
        assert np.array_equal(got.index.cpu().numpy(), want[1]) and np.array_equal(_bits(got.d2.cpu().numpy()), _bits(want[0]))
    all_nan = np.full_like(c['points'], np.nan)
    all_nan[0] = c['points'][0]
    got = _cloud(all_nan).nearest(_dev(c['queries']), _dev(c['shift']))
    assert torch.equal(got.index[0], clean.index[0]) and torch.all(got.index[1:] == -1)


def test_max_distance():
    c = cf.cloud_case('icosphere', 3, 257, 257)
    for tau in (0.004, 0.02, 0.5):
        d2, index = _check(c['points'], c['queries'], c['shift'], tau=tau, what=('tau', tau))
        assert np.all(d2[index >= 0] <= F32(tau) * F32(tau))
    d2, index = _check(c['points'], c['queries'], c['shift'], tau=0.004, what='tau small', resolutions=(64,))
    assert (index < 0).any() and (index >= 0).any()
    # a hand-made point at exactly tau, one a float32 step beyond, and queries with nothing within tau
    tau = F32(0.3)
    t2 = tau * tau
    x = np.sqrt(np.float64(t2)).astype(F32)
    for cand in (np.nextafter(x, F32(0)), np.nextafter(x, F32(1)), x):
        if F32(cand * cand) == t2:
            x = cand
    assert F32(x * x) == t2
    y = x
    while F32(y * y) <= t2:
        y = np.nextafter(y, F32(1))
    points = np.array([[[y, 0, 0], [x, 0, 0], [5, 5, 5]], [[y, 0, 0], [0, y, 0], [5, 5, 5]]], F32)
    queries = np.zeros((2, 64, 3), F32)
    queries[:, 1:] = np.array([-3, -3, -3], F32)
    d2, index = _check(points, queries, tau=float(tau), what='exactly tau')
    assert index[0, 0] == 1 and d2[0, 0] == t2 and index[1, 0] == -1 and np.all(index[:, 1:] == -1)


# ---------------------------------------------------------------------------------------------------------- hints
def test_every_hint_gives_the_unhinted_bits():
    c, points, counts, weights = _validity_inputs()
    for tau in (None, 0.01):
        for res in (4, 64):
            cloud = _cloud(points, counts, weights, res)
            plain = cloud.nearest(_dev(c['queries']), _dev(c['shift']), max_distance=tau)
            answer = plain.index.cpu().numpy()
            for kind in cf.HINT_KINDS:
                hint = cf.hints(kind, c['queries'], c['shift'], points, counts, weights, answer)
                got = cloud.nearest(_dev(c['queries']), _dev(c['shift']), hint=_dev(hint), max_distance=tau)
                assert torch.equal(got.d2, plain.d2) and torch.equal(got.index, plain.index), (tau, res, kind)
                both = _dev(hint)                                           # hint may alias index
                got = cloud.nearest(_dev(c['queries']), _dev(c['shift']), hint=both, max_distance=tau, index_out=both)
                assert got.index is both
                assert torch.equal(got.d2, plain.d2) and torch.equal(both, plain.index), (tau, res, kind, 'alias')
                got = cloud.nearest(_dev(c['queries']), _dev(c['shift']), hint=both, max_distance=tau, index_out=both)
                assert torch.equal(got.d2, plain.d2) and torch.equal(both, plain.index), (tau, res, kind, 'again')
    mix = cf.hints('mix', c['queries'], c['shift'], points, counts, weights, answer)
    for value in (-1, 257, cf.INT32_MAX, cf.INT32_MIN):
        assert (mix[0, :64] == value).any()                                 # within one wavefront
    assert (weights[0][cf.hints('zero_weight', c['queries'], c['shift'], points, counts, weights, answer)[0]] == 0).all()


# ---------------------------------------------------------------------------------------------------------- invariance
def test_invariance_of_the_bits():
    from tuch_amd.ops import PointCloud
    c = cf.cloud_case('body122', 3, 4099, 257)
    points, queries, shift = _dev(c['points']), _dev(c['queries']), _dev(c['shift'])
    cloud = PointCloud(points, resolution=64)
    base = cloud.nearest(queries, shift)
    rng = np.random.default_rng(12)
    perm = torch.as_tensor(rng.permutation(257), device=DEV)                 # the queries permuted
    got = cloud.nearest(queries[:, perm].contiguous(), shift)
    assert torch.equal(got.d2, base.d2[:, perm]) and torch.equal(got.index, base.index[:, perm])
    for b in range(3):                                                      # a body alone
        got = PointCloud(points[b:b + 1].contiguous(), resolution=64).nearest(queries[b:b + 1].contiguous(), shift[b:b + 1].contiguous())
        assert torch.equal(got.d2[0], base.d2[b]) and torch.equal(got.index[0], base.index[b])
    pperm = rng.permutation(4099)                                           # the points permuted, indices mapped back
    got = PointCloud(points[:, torch.as_tensor(pperm, device=DEV)].contiguous(), resolution=64).nearest(queries, shift)
    # (points are distinct here: equal d2 bits between different points would let the smaller NEW index win)
    back = torch.as_tensor(pperm, device=DEV)[got.index.long()]
    d2_ties = cf.brute_force_batch(c['queries'], c['points'], shift=c['shift'])
    assert torch.equal(got.d2, base.d2)
    same = (back == base.index.long())
    if not bool(same.all()):                                                # only an exact tie in the bits may differ
        for b, n in torch.nonzero(~same).cpu().numpy():
            q = (c['queries'][b, n] + c['shift'][b]).astype(F32)
            for idx in (int(back[b, n]), int(base.index[b, n])):
                d = (q - c['points'][b, idx]).astype(F32)
                sq = (d * d).astype(F32)
                assert F32(F32(sq[0] + sq[1]) + sq[2]) == d2_ties[0][b, n]
    for res in (1, 7, 16, 200):                                             # other resolutions
        got = PointCloud(points, resolution=res).nearest(queries, shift)
        assert torch.equal(got.d2, base.d2) and torch.equal(got.index, base.index), res
    # eager against captured and replayed (the build inside the graph too)
    hint = torch.full((3, 257), -1, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cloud.rebuild(points)
        cloud.nearest(queries, shift, hint=hint, index_out=hint)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cloud.rebuild(points)
        out = cloud.nearest(queries, shift, hint=hint, index_out=hint)
    hint.fill_(-1)
    for _ in range(2):                                                      # the second replay starts from the first's answers
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.d2, base.d2) and torch.equal(out.index, base.index)


def test_smpl_size_hinted_from_a_moved_mesh():
    import closest_point_cases as cc
    verts, faces = cf.mesh_verts('smpl', 2)
    assert verts.shape[1] == 6890
    points = np.stack([cf.surface_samples(verts[b], faces, 8192, 50 + b) for b in range(2)])
    rng = np.random.default_rng(14)
    moved = (verts + 2e-3 * rng.standard_normal(verts.shape)).astype(F32)
    cloud = _cloud(points, resolution=64)
    before = cloud.nearest(_dev(moved))
    got = cloud.nearest(_dev(verts), hint=before.index)
    plain = cloud.nearest(_dev(verts))
    changed = (before.index != plain.index).float().mean().item()
    helpers.report_value('point cloud hinted, smpl B=2 N=6890 Q=8192: share of hints that are not the answer', changed)
    assert 0.01 < changed < 0.99
    want = cf.brute_force_batch(verts, points)
    for out in (got, plain):
        assert np.array_equal(out.index.cpu().numpy(), want[1]) and np.array_equal(_bits(out.d2.cpu().numpy()), _bits(want[0]))


# ---------------------------------------------------------------------------------------------------------- the term
def _term(c, cloud=None, verts=None, vw='case', hint=None, scale=None, tau='case', index_out=None):
    """ops.cloud_fit on a case + one backward pass: dict of numpy (per, total, gv, gt) and the NearestPoint."""
    from tuch_amd import ops
    if cloud is None:
        cloud = _cloud(c['points'], c['counts'], c['weights'])
    v = _dev(c['verts'] if verts is None else verts, requires_grad=True)
    tr = _dev(c['transl'], requires_grad=True)
    w = _dev(c['vw']) if isinstance(vw, str) else vw
    t = c['tau'] if isinstance(tau, str) else tau
    total, per, near = ops.cloud_fit(cloud, v, tr, w, hint, c['rho'], c['sigma'], t, c['scale'], index_out=index_out)
    assert total.dim() == 0 and per.shape == (v.shape[0],) and not per.requires_grad and not near.d2.requires_grad
    if scale is None:
        ops.backward_scalar(total)
    else:
        (scale * total).backward()
    return dict(per=per.cpu().numpy(), total=total.item(), gv=v.grad.cpu().numpy(), gt=tr.grad.cpu().numpy()), near


@pytest.mark.parametrize('tau', [False, True])
@pytest.mark.parametrize('weighted', ['none', 'V', 'BV'])
@pytest.mark.parametrize('rho', sc.RHOS)
def test_term_matches_float64(rho, weighted, tau):
    """per_body and total within 4 x the error of the float32 numpy restatement (floored as sc.term_case floors its bound);
    the NearestPoint is PointCloud.nearest's, bit for bit."""
    c = cf.term_case('body122', rho, weighted, tau)
    cloud = _cloud(c['points'], c['counts'])
    got, near = _term(c, cloud)
    err = np.abs(got['per'].astype(np.float64) - c['ref'][0])
    helpers.report_value('cloud_fit body122 %s weights=%s tau=%d: largest per-body error / bound' % (rho, weighted, tau),
                         (err / c['bound']).max())
    print('cloud_fit', rho, weighted, tau, 'per_body error', err, 'bound', c['bound'])
    assert np.all(c['ref'][0] > 0)
    assert np.all(err <= c['bound']), (err, c['bound'])
    assert abs(got['total'] - c['ref'][1]) <= c['bound'].sum()
    plain = cloud.nearest(_dev(c['verts']), _dev(c['transl']), max_distance=c['tau'])
    live = torch.ones_like(plain.index, dtype=torch.bool) if c['vw'] is None else \
        (_dev(c['vw']) != 0).expand(plain.index.shape)
    assert torch.equal(near.index[live], plain.index[live]) and torch.equal(near.d2[live], plain.d2[live])
    assert torch.all(near.index[~live] == -1) and torch.all(torch.isposinf(near.d2[~live]))
    if tau:
        assert (near.index[live] < 0).any() and (near.index[live] >= 0).any()
    # a hint changes nothing, and index_out may be the hint tensor
    both = near.index.clone()
    again, out = _term(c, cloud, hint=both, index_out=both)
    assert out.index is both and torch.equal(both, near.index) and torch.equal(out.d2, near.d2)
    for key in got:
        assert np.array_equal(got[key], again[key]), key


@pytest.mark.parametrize('name', ['icosphere', 'body122'])
def test_term_without_an_angle_has_the_plain_querys_bits(name):
    """ops.cloud_fit without max_angle: the NearestPoint of PointCloud.nearest without query_normals, bit for bit -- on a
    plain cloud, and on one that has been given normals, which neither call then reads."""
    from tuch_amd import ops
    c = cf.cloud_case(name, 3, 257, 257)
    cloud = _cloud(c['points'])
    verts, transl = _dev(c['queries']), _dev(c['shift'])
    plain = cloud.nearest(verts, transl)
    assert (plain.index >= 0).all()
    normals = np.random.default_rng(7).standard_normal(c['points'].shape).astype(F32)
    for oriented in (False, True):
        if oriented:
            cloud.orient(_dev(normals))
            again = cloud.nearest(verts, transl)
            assert torch.equal(again.index, plain.index) and torch.equal(again.d2, plain.d2)
        _, _, near = ops.cloud_fit(cloud, verts, transl)
        assert torch.equal(near.index, plain.index) and torch.equal(near.d2, plain.d2), oriented


def test_term_at_batch_65_with_two_chunks_matches_float64():
    """65 bodies x 257 weighted vertices against clouds of 65 points: two workgroups per body (and two strides of the
    normaliser's sum), and 4 x 65 = 260 (body, component) sums for the 256 threads of the workgroup that arrives last --
    the second trip of its loop, which a batch of 3 never takes.  per_body and total by the rule of
    test_term_matches_float64; the last body's sums, the ones of the second trip, have the bits of that body alone."""
    c = cf.term_case('body122', 'distance', 'BV', False, batch=65, num_points=65, num_verts=257)
    got, _ = _term(c)
    err = np.abs(got['per'].astype(np.float64) - c['ref'][0])
    print('cloud_fit batch 65: largest per-body error / bound', (err / c['bound']).max())
    assert np.all(c['ref'][0] > 0)
    assert np.all(err <= c['bound']), (err, c['bound'])
    assert abs(got['total'] - c['ref'][1]) <= c['bound'].sum()
    last = dict(c, **{k: c[k][64:] for k in ('verts', 'transl', 'points', 'counts', 'vw')})
    alone, _ = _term(last)
    for key in ('per', 'gt', 'gv'):
        assert np.array_equal(got[key][64:], alone[key]), key


@pytest.mark.parametrize('rho', sc.RHOS)
def test_gradients_against_central_differences(rho):
    from tuch_amd import ops
    c = cf.grad_case(rho)
    cf.assert_gap(c['verts'], c['transl'], c['points'])
    for mode in (True, False):
        with ops.deterministic_mode(mode):
            got, _ = _term(c)
        for key, what in (('gv', 'verts'), ('gt', 'transl')):
            ok, ratio = sc.grad_within(got[key], c[key])
            helpers.report_value('cloud_fit %s grad_%s, deterministic=%d: error / bound' % (rho, what, mode), ratio)
            assert ok, (rho, what, mode, ratio)
        ok, ratio = sc.grad_within(got['gt'], got['gv'].astype(np.float64).sum(1))
        assert ok, (rho, mode, ratio)
    scaled, _ = _term(c, scale=2.5)                                          # a non-unit upstream gradient scales both
    for key in ('gv', 'gt'):
        ok, ratio = sc.grad_within(scaled[key], 2.5 * c[key])
        assert ok, (rho, key, ratio)


def test_equal_bits_twice_alone_and_in_both_modes():
    from tuch_amd import ops
    from tuch_amd.ops._base import _ticket
    results = []
    for rho in ('distance', 'gmof'):
        c = cf.term_case('body122', rho, 'BV', True)
        for mode in (True, False):
            with ops.deterministic_mode(mode):
                first, second, third = _term(c)[0], _term(c)[0], _term(c)[0]   # the third finds the second's ticket
                for key in first:
                    assert np.array_equal(first[key], second[key]) and np.array_equal(first[key], third[key]), key
                for b in range(3):                                          # a body alone
                    one = dict(c, verts=c['verts'][b:b + 1], transl=c['transl'][b:b + 1], points=c['points'][b:b + 1],
                               vw=c['vw'][b:b + 1], counts=c['counts'][b:b + 1])
                    alone, _ = _term(one)
                    assert alone['per'][0] == first['per'][b] and alone['total'] == first['per'][b]
                    assert np.array_equal(alone['gv'][0], first['gv'][b]) and np.array_equal(alone['gt'][0], first['gt'][b])
            results.append(first)
        for key in results[-1]:                                             # the two modes
            assert np.array_equal(results[-1][key], results[-2][key]), key
    assert int(_ticket(torch.device(DEV)).item()) == 0


def test_zero_weight_vertices_and_bodies_without_weight_or_points():
    c = cf.term_case('body122', 'distance', 'BV', True)
    clean, near = _term(c)
    off = c['vw'] == 0
    assert off.any() and not off.all(1).any()
    verts = c['verts'].copy()
    verts[off] = np.nan
    verts[0, np.nonzero(off[0])[0][0]] = np.inf
    dirty, _ = _term(c, verts=verts)
    for key in clean:
        assert np.array_equal(clean[key], dirty[key]), key
    assert np.all(np.isfinite(dirty['gv'])) and not dirty['gv'][off].any()
    vw = c['vw'].copy()
    vw[2] = 0.0
    empty = dict(c, counts=np.array([257, 0, 130], np.int32))
    got, near = _term(empty, vw=_dev(vw))
    assert got['per'][0] > 0 and got['per'][1] == 0.0 and got['per'][2] == 0.0 and got['total'] == got['per'][0]
    for key in ('gv', 'gt'):
        assert np.all(np.isfinite(got[key])) and not got[key][1].any() and not got[key][2].any() and got[key][0].any(), key
    assert torch.all(near.index[1:] == -1)
    # without tau a vertex without winner (a non-finite one of weight 1) contributes nothing and has a zero row
    verts = c['verts'].copy()
    verts[0, 5] = np.nan
    got, near = _term(dict(c, vw=None), verts=verts, vw=None, tau=None)
    assert np.all(np.isfinite(got['gv'])) and not got['gv'][0, 5].any() and near.index[0, 5].item() == -1 and np.isfinite(got['total'])


def test_term_workspace_guards_and_capture():
    from tuch_amd import ops
    c = cf.term_case('body122', 'distance', 'V', True)
    want, near = _term(c)
    was = ops.set_cloud_canary(True)
    try:
        guarded = _cloud(c['points'], c['counts'], resolution=64)
        assert guarded._nbytes > _cloud(c['points'], c['counts'], resolution=1)._nbytes
        got, _ = _term(c, guarded)
        guarded.nearest(_dev(c['verts']), _dev(c['transl']))
        guarded.rebuild(_dev(c['points']), _dev(c['counts']))
        assert guarded.canary_hits() == 0
        for key in want:
            assert np.array_equal(want[key], got[key]), key
    finally:
        ops.set_cloud_canary(was)
    # captured and replayed: the same bits
    cloud = _cloud(c['points'], c['counts'])
    v, tr, vw = _dev(c['verts']), _dev(c['transl']), _dev(c['vw'])
    hint = torch.full(tuple(v.shape[:2]), -1, dtype=torch.int32, device=DEV)
    call = lambda: ops.cloud_fit(cloud, v, tr, vw, hint, c['rho'], c['sigma'], c['tau'], c['scale'], index_out=hint)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        total, per, out = call()
    hint.fill_(-1)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(per.cpu().numpy(), want['per']) and total.item() == want['total']
        assert torch.equal(out.d2, near.d2) and torch.equal(out.index, near.index)


def test_argument_errors():
    from tuch_amd import ops
    from tuch_amd.ops import PointCloud
    c = cf.term_case('body122', 'distance')
    points, v, tr = _dev(c['points']), _dev(c['verts']), _dev(c['transl'])
    with pytest.raises(ValueError, match='points'):
        PointCloud(points[:, :, :2])
    with pytest.raises(ValueError, match='counts'):
        PointCloud(points, counts=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='weights'):
        PointCloud(points, weights=torch.ones(3, 5, device=DEV))
    with pytest.raises(ValueError, match='resolution'):
        PointCloud(points, resolution=0)
    with pytest.raises(RuntimeError, match='HIP device'):
        PointCloud(points.cpu())
    cloud = PointCloud(points)
    with pytest.raises(ValueError, match='queries'):
        cloud.nearest(v[:2])
    with pytest.raises(ValueError, match='shift'):
        cloud.nearest(v, tr[:2])
    with pytest.raises(ValueError, match='hint'):
        cloud.nearest(v, hint=torch.zeros(3, 5, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='max_distance'):
        cloud.nearest(v, max_distance=0.0)
    with pytest.raises(RuntimeError, match='HIP device'):
        cloud.nearest(v.cpu())
    with pytest.raises(ValueError, match='rho'):
        ops.cloud_fit(cloud, v, tr, rho='huber')
    with pytest.raises(ValueError, match='sigma'):
        ops.cloud_fit(cloud, v, tr, rho='gmof')
    with pytest.raises(ValueError, match='transl'):
        ops.cloud_fit(cloud, v, tr[:2])
    with pytest.raises(ValueError, match='vertex_weights'):
        ops.cloud_fit(cloud, v, tr, vertex_weights=torch.ones(5, device=DEV))
    with pytest.raises(ValueError, match='PointCloud'):
        ops.cloud_fit(None, v, tr)


def test_nearest_is_differentiable_with_the_index_held_fixed():
    c = cf.grad_case('squared')
    cloud = _cloud(c['points'])
    v, tr = _dev(c['verts'], requires_grad=True), _dev(c['transl'], requires_grad=True)
    out = cloud.nearest(v, tr)
    up = torch.linspace(0.5, 1.5, v.shape[1], device=DEV)[None].expand(2, -1)
    (out.d2 * up).sum().backward()
    q = (c['verts'].astype(np.float64) + c['transl'].astype(np.float64)[:, None])
    s = np.stack([c['points'][b][out.index[b].cpu().numpy()] for b in range(2)]).astype(np.float64)
    want = 2.0 * up.cpu().numpy()[:, :, None] * (q - s)
    ok, ratio = sc.grad_within(v.grad.cpu().numpy(), want)
    assert ok, ratio
    ok, ratio = sc.grad_within(tr.grad.cpu().numpy(), want.sum(1))
    assert ok, ratio


# ---------------------------------------------------------------------------------------------------------- the fitter
@pytest.fixture(scope='module')
def smpl():
    from tuch_amd.models.smpl import SMPL
    return SMPL(model_data=sc.fit_inputs()['body'], batch_size=sc.FIT_BATCH).to(DEV)


@functools.lru_cache(maxsize=None)
def body_model():
    from tuch_amd.ops import ContactModel
    return ContactModel(sc.fit_inputs()['faces'], device=DEV)


def _fit(smpl, num_iters, **kw):
    from tuch_amd.fit import ScanFitter
    c = sc.fit_inputs()
    kw.setdefault('fit_global_orient', False)
    fitter = ScanFitter(smpl, body_model(), num_iters=num_iters, **kw)
    return fitter, fitter(_dev(c['points']), _dev(c['global_orient']), counts=_dev(c['counts']))


def test_two_sided_trajectory_follows_the_float64_loop(smpl):
    """The parameters before each of the first 20 updates against the float64 loop of the two-sided objective, within 4 x
    the float32 CPU loop's own deviation, floored at 1e-4 (the float32 loop holds the floor over all 20 iterations for
    this seed: tests/test_cloud_fit_host.py)."""
    holds, bound = cf.trajectory_bound('distance')
    assert holds
    ref = cf.fit_reference(sc.FIT_PREFIX)
    fitter, _ = _fit(smpl, sc.FIT_PREFIX, model_to_scan=cf.FIT_LAMBDA, record_history=True)
    history = fitter.history['fit']
    assert len(history) == sc.FIT_PREFIX
    worst = 0.0
    for it in range(sc.FIT_PREFIX):
        dev = max(float(np.abs(g.cpu().numpy().astype(np.float64) - w).max())
                  for g, w in zip(history[it]['params'], ref['params'][it]))
        worst = max(worst, dev / bound[it])
        assert dev <= bound[it], (it, dev, bound[it])
    helpers.report_value('ScanFitter two-sided: parameters vs float64 over %d iterations, error / bound' % sc.FIT_PREFIX, worst)
    np.testing.assert_allclose(history[0]['loss'].item(), ref['loss'][0].sum(), rtol=1e-4)


def test_two_sided_fit_reduces_the_loss_like_the_float64_loop(smpl):
    """final / initial two-sided loss of every body after 60 iterations at most sc.RATIO_MARGIN x the float64 loop's."""
    ref = cf.fit_reference(sc.FIT_ITERS)
    want = ref['final_loss'].sum(1) / ref['loss'][0].sum(1)
    two = lambda fitter, fit: (fit.loss + fitter.model_to_scan_result.loss).cpu().numpy()
    start = two(*_fit(smpl, 0, model_to_scan=cf.FIT_LAMBDA))
    fitter, fit = _fit(smpl, sc.FIT_ITERS, model_to_scan=cf.FIT_LAMBDA)
    assert fitter.graph_replayed == {'fit': sc.FIT_ITERS - 3}
    np.testing.assert_allclose(start, ref['loss'][0].sum(1), rtol=1e-4)
    ratio = two(fitter, fit) / start
    print('ScanFitter two-sided ratio', ratio, 'float64', want)
    helpers.report_value('ScanFitter two-sided: largest ratio / float64 ratio (bound %.2f)' % sc.RATIO_MARGIN, (ratio / want).max())
    assert np.all(ratio <= sc.RATIO_MARGIN * want), (ratio, want)
    # what is returned belongs together
    from tuch_amd import ops
    c = sc.fit_inputs()
    result = fitter.model_to_scan_result
    assert result.d2.shape == (3, 362) and result.index.dtype == torch.int32 and result.loss.shape == (3,)
    verts = smpl(global_orient=fit.global_orient, body_pose=fit.body_pose, betas=fit.betas).vertices
    near = ops.PointCloud(_dev(c['points']), _dev(c['counts'])).nearest(verts, fit.transl)
    assert torch.equal(near.d2, result.d2) and torch.equal(near.index, result.index)
    for b in range(3):
        assert torch.all(result.index[b] < int(c['counts'][b])) and torch.all(result.index[b] >= 0)


def test_two_sided_hint_graph_and_sessions_change_no_bit(smpl, monkeypatch):
    from tuch_amd import ops
    from tuch_amd.fit import ScanFitter
    monkeypatch.setenv('TUCH_GRAPH_STRICT', '1')
    c = sc.fit_inputs()
    points, go, counts = _dev(c['points']), _dev(c['global_orient']), _dev(c['counts'])
    rng = np.random.default_rng(3)
    moved = (c['points'] + 0.01 * rng.standard_normal(c['points'].shape)).astype(F32)
    other, other_counts = _dev(moved), _dev(np.array([200, 64, 100], np.int32))

    def same(a, fa, b, fb, what):
        for field, x, y in zip(a._fields, a, b):
            assert torch.equal(x, y), (what, field)
        for field, x, y in zip(fa.model_to_scan_result._fields, fa.model_to_scan_result, fb.model_to_scan_result):
            assert torch.equal(x, y), (what, 'model_to_scan_result', field)
    with ops.deterministic_mode(True):
        make = lambda **kw: ScanFitter(smpl, body_model(), num_iters=20, fit_global_orient=False, model_to_scan=0.5,
                                       max_distance=0.5, **kw)
        hinted = make(use_hint=True)
        first = hinted(points, go, counts=counts)
        first_result = hinted.model_to_scan_result
        assert hinted.graph_replayed == {'fit': 17} and len(hinted._sessions) == 1
        for name, kw in (('use_hint=False', dict(use_hint=False)), ('eager', dict(use_hint=True, use_graph=False)),
                         ('resolution', dict(resolution=16))):
            f = make(**kw)
            fit = f(points, go, counts=counts)
            for field, x, y in zip(first._fields, first, fit):
                assert torch.equal(x, y), (name, field)
            for field, x, y in zip(first_result._fields, first_result, f.model_to_scan_result):
                assert torch.equal(x, y), (name, 'model_to_scan_result', field)
        second = hinted(other, go, counts=other_counts)                     # the kept session: replays only, cloud rebuilt
        assert hinted.graph_replayed == {'fit': 20} and len(hinted._sessions) == 1
        fresh_fitter = make(use_hint=True)
        fresh = fresh_fitter(other, go, counts=other_counts)
        same(second, hinted, fresh, fresh_fitter, 'kept session')
        assert not torch.equal(first.body_pose, second.body_pose)


def test_model_to_scan_off_is_the_one_sided_fit(smpl):
    from tuch_amd import ops
    with ops.deterministic_mode(True):
        plain_fitter, plain = _fit(smpl, 20)
        off_fitter, off = _fit(smpl, 20, model_to_scan=0.0, max_distance=0.1, resolution=8)
        on_fitter, on = _fit(smpl, 20, model_to_scan=1.0)
    for field, a, b in zip(plain._fields, plain, off):
        assert torch.equal(a, b), field
    assert plain_fitter.model_to_scan_result is None and off_fitter.model_to_scan_result is None
    assert len(off_fitter._sessions) == 1 and next(iter(off_fitter._sessions.values()))['cloud'] is None
    assert on_fitter.model_to_scan_result is not None and not torch.equal(on.body_pose, plain.body_pose)
    assert plain._fields == ('global_orient', 'body_pose', 'betas', 'transl', 'vertices', 'loss', 'face', 'bary')


def test_two_sided_fitter_argument_errors(smpl):
    from tuch_amd.fit import ScanFitter
    c = sc.fit_inputs()
    points, go = _dev(c['points']), _dev(c['global_orient'])
    with pytest.raises(ValueError, match='model_to_scan'):
        ScanFitter(smpl, body_model(), model_to_scan=-1.0)
    with pytest.raises(ValueError, match='max_distance'):
        ScanFitter(smpl, body_model(), model_to_scan=1.0, max_distance=0.0)
    with pytest.raises(ValueError, match='resolution'):
        ScanFitter(smpl, body_model(), model_to_scan=1.0, resolution=0)
    with pytest.raises(ValueError, match='vertex_weights'):
        ScanFitter(smpl, body_model(), model_to_scan=1.0, vertex_weights=torch.ones(5))
    with pytest.raises(ValueError, match='vertex_weights'):
        ScanFitter(smpl, body_model(), num_iters=2, model_to_scan=1.0, vertex_weights=torch.ones(2, 362))(points, go)
    with pytest.raises(RuntimeError, match='HIP device'):
        ScanFitter(smpl, body_model(), model_to_scan=1.0)(points.cpu(), go.cpu())
    # vertex weights are taken: a fit with half the vertices switched off differs, and its result says so
    vw = torch.ones(362)
    vw[::2] = 0.0
    fitter = ScanFitter(smpl, body_model(), num_iters=6, fit_global_orient=False, model_to_scan=1.0, vertex_weights=vw)
    fitter(points, go, counts=_dev(c['counts']))
    assert torch.all(fitter.model_to_scan_result.index[:, ::2] == -1) and torch.all(fitter.model_to_scan_result.index[:, 1::2] >= 0)


def test_the_two_sided_fit_brings_a_stray_arm_back_sooner():
    """What the feature is for: the scan is the true body, the fit starts with one arm rotated 0.6 rad away at the shoulder.
    Scan points near the arm's true place pull on whatever surface is nearest; only the second direction pulls the arm's
    own vertices to the scan.  After the same number of iterations the two-sided fit is closer to the true vertices (the
    float64 CPU loops: 5.75 mm against 2.86 mm, tests/test_cloud_fit_host.py; only the ordering is asserted)."""
    from tuch_amd.fit import ScanFitter
    from tuch_amd.models.smpl import SMPL
    from tuch_amd.ops import ContactModel
    c = cf.feature_case()
    assert c['one_sided'] >= 1.5 * c['two_sided']
    smpl = SMPL(model_data=c['body'], batch_size=1).to(DEV)
    model = ContactModel(np.asarray(c['body'].faces, np.int64), device=DEV)
    true = _dev(c['true'].astype(F32))
    dist = {}
    for name, lam in (('one_sided', 0.0), ('two_sided', 1.0)):
        fitter = ScanFitter(smpl, model, num_iters=cf.FEATURE_ITERS, fit_global_orient=False, model_to_scan=lam)
        fit = fitter(_dev(c['points']), _dev(c['global_orient']), body_pose=_dev(c['body_pose0']))
        dist[name] = (fit.vertices[0] - true).norm(dim=1).mean().item()
        helpers.report_value('stray arm, %s: mean vertex-to-true-vertex distance / float64 loop' % name, dist[name] / c[name])
    print('stray arm', dist, 'float64', c['one_sided'], c['two_sided'])
    assert dist['two_sided'] < dist['one_sided'], dist
