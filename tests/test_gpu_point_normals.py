"""GPU: the k nearest points of a cloud and the PCA normals over them (csrc/point_cloud.hip: pc_knn_kernel,
pc_normals_kernel) against the statements of tests/point_normal_cases.py.  The k-nearest lists and the scatter matrices
are compared bit for bit -- np.array_equal on the index, on d2's bits and on cov's bits, no tolerance, no allowed mismatch --,
the normals and the variation against float64 within the bound the source file derives (E = (n + 256) u sum_j |d_j|^2;
angle <= 2 E / (lambda1 - lambda0), variation within 2 E / trace + 2 u), and ScanFitter(estimate_normals=) against the same
fitter given the normals PointCloud.normals computes.

Observed on an MI355X (2026-10-20): every k-nearest case and every scatter matrix equal to the statement in all bits;
angle error / bound at most 1.9e-3 and variation error / bound at most 1.8e-3 over k in {3, 8, 16, 32} and both clouds
(the bound is a worst-case one: 15 rotations and n roundings per sum all taken against one side), no zero row there;
the fitter's composition equal in every field.  DESIGN.md section 3, "k nearest points and normals of a cloud"."""
import functools
import gc

import numpy as np
import pytest
import torch

import cloud_fit_cases as cf
import helpers
import point_normal_cases as pn
import scan_fit_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
RESOLUTIONS = (1, 4, 64)
KS = (1, 3, 8, 16, 32)


def _dev(a, **kw):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV, **kw)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cloud(points, counts=None, weights=None, resolution=64):
    from tuch_amd.ops import PointCloud
    return PointCloud(_dev(points), _dev(counts), _dev(weights), resolution)


def _knn(cloud, queries, k, shift=None, counts=None, tau=None):
    out = cloud.knn(_dev(queries), k, _dev(shift), _dev(counts), tau)
    assert out.d2.shape == out.index.shape == (cloud.batch, cloud.num_points if queries is None else queries.shape[1], k)
    assert out.index.dtype == torch.int32 and out.d2.dtype == torch.float32
    return out.d2.cpu().numpy(), out.index.cpu().numpy()


def _check(points, queries, ks=KS, shift=None, counts=None, weights=None, tau=None, query_counts=None,
           resolutions=RESOLUTIONS, what=''):
    """Every resolution and every k against brute force (the list for k is the first k columns of the list for max k);
    returns the brute-force (d2, index) for the largest k."""
    want = pn.knn_brute_force_batch(queries, points, max(ks), counts, weights, shift, tau, query_counts)
    for res in resolutions:
        cloud = _cloud(points, counts, weights, res)
        for k in ks:
            d2, index = _knn(cloud, queries, k, shift, query_counts, tau)
            assert np.array_equal(index, want[1][:, :, :k]), (what, res, k, np.argwhere(index != want[1][:, :, :k])[:5])
            assert np.array_equal(_bits(d2), _bits(want[0][:, :, :k])), (what, res, k)
    return want


# ---------------------------------------------------------------------------------------------------------- the search
@pytest.mark.parametrize('num_points', [1, 2, 3, 63, 64, 65, 257, 4099])
@pytest.mark.parametrize('batch', [1, 3])
def test_knn_equals_brute_force(batch, num_points):
    """points x queries {1, 64, 65, 257} x k {1, 3, 8, 16, 32} x resolutions {1, 4, 64}, k > number of points included."""
    name = 'icosphere' if num_points % 2 else 'body122'
    for num_queries in (1, 64, 65, 257):
        c = cf.cloud_case(name, batch, num_points, num_queries)
        d2, index = _check(c['points'], c['queries'], shift=c['shift'], what=(name, batch, num_points, num_queries))
        full = min(num_points, 32)
        assert np.all(index[:, :, :full] >= 0) and np.all(index[:, :, full:] == -1) and np.all(np.isposinf(d2[:, :, full:]))
    _check(c['points'], c['queries'], ks=(8,), what='no shift', resolutions=(64,))


def test_max_distance_gives_partial_lists():
    c = cf.cloud_case('icosphere', 3, 257, 257)
    partial = 0
    for tau in (0.004, 0.05, 0.5):
        d2, index = _check(c['points'], c['queries'], ks=(3, 16), shift=c['shift'], tau=tau, what=('tau', tau))
        assert np.all(d2[index >= 0] <= F32(tau) * F32(tau))
        found = (index >= 0).sum(2)
        partial += int(((found > 0) & (found < 16)).sum())
    assert partial > 0                                                      # partial lists are there


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
    points[0, keep[3]] = np.inf
    points[0, keep[4], 1] = -np.inf
    weights[0, keep[3]] = 1.0
    queries = c['queries'].copy()
    queries[0, 5] = np.nan
    queries[1, 7, 2] = np.inf
    queries[2, 64] = -np.inf
    return c, points, counts, weights, queries


def test_counts_zero_weights_and_non_finite_points_and_queries():
    c, points, counts, weights, queries = _validity_inputs()
    d2, index = _check(points, queries, ks=(1, 8, 32), shift=c['shift'], counts=counts, weights=weights, what='validity')
    for b in range(3):
        ids = cf.valid_points(points[b], counts[b], weights[b])
        assert np.all(np.isin(index[b][index[b] >= 0], ids))
    assert np.all(index[0, 5] == -1) and np.all(index[1, 7] == -1) and np.all(index[2, 64] == -1)
    _check(points, queries, ks=(8,), shift=c['shift'], counts=np.array([1000, -5, 1], np.int32), weights=weights,
           what='counts clamped', resolutions=(4,))
    qc = np.array([130, 0, 65], np.int32)
    d2, index = _check(points, queries, ks=(8,), shift=c['shift'], counts=counts, weights=weights, query_counts=qc,
                       what='query counts', resolutions=(64,))
    assert np.all(index[1] == -1) and np.all(np.isposinf(d2[1])) and np.all(index[2, 65:] == -1) and np.all(index[2, :64, 0] >= 0)
    # an empty cloud, and a body of NaN beside clean ones
    empty = np.array([257, 0, 257], np.int32)
    d2, index = _check(c['points'], c['queries'], ks=(8,), counts=empty, what='empty', resolutions=(64,))
    assert np.all(index[1] == -1)


def test_degenerate_boxes():
    rng = np.random.default_rng(6)
    queries = rng.standard_normal((2, 65, 3)).astype(F32)
    same = np.tile(np.array([0.25, -0.5, 1.5], F32), (2, 64, 1))            # all keys tie in d2: indices 0 .. k - 1 win
    d2, index = _check(same, queries, what='coincident')
    assert np.array_equal(index, np.broadcast_to(np.arange(32), index.shape))
    plane = rng.standard_normal((2, 257, 3)).astype(F32)
    plane[:, :, 2] = 0.125
    _check(plane, queries, what='plane')
    line = plane.copy()
    line[:, :, 1] = -3.0
    _check(line, queries, what='line')
    one = rng.standard_normal((2, 1, 3)).astype(F32)                        # Q = 1
    d2, index = _check(one, queries, what='one point')
    assert np.all(index[:, :, 0] == 0) and np.all(index[:, :, 1:] == -1)


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
    steps = [np.unique(np.clip([0, 1, 2, d // 2, d - 1, d], 0, d)) for d in dims]
    walls = np.minimum(np.maximum(_grid_points(g, 0, steps), lo), hi)       # (the box, hence the grid, must not change)
    mixed = walls.copy()                                                    # on a wall along one axis only
    mixed[:, 1:] = (lo + (hi - lo) * rng.random((len(walls), 3)).astype(F32))[:, 1:]
    points = np.concatenate([anchors, walls, mixed]).astype(F32)[None]
    again = _cloud(points, resolution=resolution).grid()
    assert np.array_equal(again.origin, g.origin) and np.array_equal(again.cell, g.cell) and np.array_equal(again.dims, g.dims)
    on_walls = _grid_points(g, 0, [np.arange(0, d + 1, max(d // 4, 1)) for d in dims])
    queries = np.concatenate([on_walls, np.nextafter(on_walls, np.inf).astype(F32), np.nextafter(on_walls, -np.inf).astype(F32),
                              walls[::3], (lo + (hi - lo) * rng.random((64, 3))).astype(F32)])[None]
    _check(points, queries, ks=(1, 8, 32), what='walls', resolutions=(resolution,))


def test_far_scene_and_queries_outside_the_grid():
    c = cf.cloud_case('icosphere', 2, 257, 257)
    move = np.array([100.0, -100.0, 100.0], F32)
    _check((c['points'] + move).astype(F32), (c['queries'] + move).astype(F32), ks=(8, 32), shift=c['shift'], what='far scene')
    rng = np.random.default_rng(8)
    out = (1000.0 * rng.standard_normal((2, 64, 3))).astype(F32)            # outside the grid in every direction: bits tie
    _check(c['points'], out, ks=(8, 32), what='outside')


def test_self_query():
    """queries=None: the cloud's own points in the caller's order; every valid point finds itself first, or the
    smallest index among its duplicates; an invalid point gets -1 / +inf."""
    c, points, counts, weights, _ = _validity_inputs()
    points, weights = points.copy(), weights.copy()
    points[0, 12] = points[0, 40] = c['points'][0, 12]                      # duplicates: the smaller index comes first
    weights[0, 12] = weights[0, 40] = 1.0
    for res in (4, 64):
        cloud = _cloud(points, counts, weights, res)
        d2, index = _knn(cloud, None, 8)
        # the statement: the points as queries, the invalid ones made non-finite
        queries = points.copy()
        for b in range(3):
            bad = np.setdiff1d(np.arange(257), cf.valid_points(points[b], counts[b], weights[b]))
            queries[b, bad] = np.nan
        want = pn.knn_brute_force_batch(queries, points, 8, counts, weights)
        assert np.array_equal(index, want[1]) and np.array_equal(_bits(d2), _bits(want[0]))
        for b in range(3):
            ids = cf.valid_points(points[b], counts[b], weights[b])
            bad = np.setdiff1d(np.arange(257), ids)
            assert np.all(index[b, bad] == -1) and np.all(np.isposinf(d2[b, bad]))
            assert np.all(d2[b, ids, 0] == 0)
            own = index[b, ids, 0] == ids
            assert own.sum() >= len(ids) - 1
        assert index[0, 40, 0] == 12 and index[0, 40, 1] == 40 and index[0, 12, 0] == 12 and index[0, 12, 1] == 40


# ---------------------------------------------------------------------------------------------------------- invariance
def _all_outputs(cloud, queries, k, shift=None, viewpoint=None):
    near = cloud.knn(queries, k, shift)
    out = cloud.normals(queries, k, viewpoint, shift, with_cov=True)
    return dict(d2=near.d2, index=near.index, normal=out.normal, variation=out.variation, count=out.count, cov=out.cov)


def _equal_bits(a, b):
    """torch.equal on the bit patterns (NaN-free here, but -0.0 must not pass for 0.0)."""
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def test_invariance_of_the_bits():
    from tuch_amd.ops import PointCloud
    c = cf.cloud_case('body122', 3, 4099, 257)
    points, queries, shift = _dev(c['points']), _dev(c['queries']), _dev(c['shift'])
    view = _dev(np.array([[0, 0, 3], [1, 2, 3], [-2, 0.5, 0]], F32))
    k = 16
    cloud = PointCloud(points, resolution=64)
    base = _all_outputs(cloud, queries, k, shift, view)
    assert bool((base['normal'].abs().sum(2) > 0).all())
    rng = np.random.default_rng(12)
    perm = torch.as_tensor(rng.permutation(257), device=DEV)                 # the queries permuted
    got = _all_outputs(cloud, queries[:, perm].contiguous(), k, shift, view)
    for key in base:
        assert _equal_bits(got[key], base[key][:, perm].contiguous()), ('queries permuted', key)
    for b in range(3):                                                      # a body alone
        got = _all_outputs(PointCloud(points[b:b + 1].contiguous(), resolution=64), queries[b:b + 1].contiguous(), k,
                           shift[b:b + 1].contiguous(), view[b:b + 1].contiguous())
        for key in base:
            assert _equal_bits(got[key][0], base[key][b]), ('alone', b, key)
    pperm = torch.as_tensor(rng.permutation(4099), device=DEV)              # the points permuted, indices mapped back
    got = _all_outputs(PointCloud(points[:, pperm].contiguous(), resolution=64), queries, k, shift, view)
    back = pperm[got['index'].long()].to(torch.int32)
    ties = (base['d2'][:, :, 1:] == base['d2'][:, :, :-1]).any(2)             # (equal d2 bits let the smaller NEW index lead)
    free = ~ties
    assert float(free.float().mean()) > 0.95                                # nearly every row is compared
    assert _equal_bits(got['d2'], base['d2'])
    assert torch.equal(back[free], base['index'][free])
    for key in ('normal', 'variation', 'count', 'cov'):
        assert _equal_bits(got[key][free], base[key][free]), ('points permuted', key)
    for res in (1, 7, 16, 200):                                             # other resolutions
        got = _all_outputs(PointCloud(points, resolution=res), queries, k, shift, view)
        for key in base:
            assert _equal_bits(got[key], base[key]), (res, key)
    # the per-query viewpoint layout with the same positions: the same bits
    got = cloud.normals(queries, k, view[:, None].expand(-1, 257, -1).contiguous(), shift)
    assert _equal_bits(got.normal, base['normal'])
    # eager against captured and replayed (the build inside the graph too)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cloud.rebuild(points)
        _all_outputs(cloud, queries, k, shift, view)
    torch.cuda.current_stream().wait_stream(s)
    gc.collect()                                            # (dead fitters of earlier tests own graphs: not inside a capture)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cloud.rebuild(points)
        out = _all_outputs(cloud, queries, k, shift, view)
    for _ in range(2):
        for t in out.values():
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for key in base:
            assert _equal_bits(out[key], base[key]), ('replay', key)


def test_guarded_workspace_gives_the_same_bits():
    """set_cloud_canary: the cloud's regions are laid out with guard words between them; knn and normals address them
    there, return the bits of the unguarded cloud and change no guard word."""
    from tuch_amd import ops
    c, points, counts, weights, queries = _validity_inputs()
    q, shift = _dev(queries), _dev(c['shift'])
    view = _dev(np.array([[0, 0, 3], [1, 2, 3], [-2, 0.5, 0]], F32))

    def outputs(cloud):
        out = []
        for k in (3, 16, 32):
            near, own = cloud.knn(q, k, shift, max_distance=0.2), cloud.knn(None, k)
            normal = cloud.normals(q, k, view, shift, with_cov=True)
            out += [near.d2, near.index, own.d2, own.index, normal.normal, normal.variation, normal.count, normal.cov]
        return out
    want = outputs(_cloud(points, counts, weights, 16))
    assert bool((want[1] >= 0).any()) and bool((want[4] != 0).any())
    was = ops.set_cloud_canary(True)
    try:
        guarded = _cloud(points, counts, weights, 16)
        got = outputs(guarded)
        assert guarded.canary_hits() == 0
    finally:
        ops.set_cloud_canary(was)
    assert guarded._nbytes > _cloud(points, counts, weights, 16)._nbytes     # the guards were there
    for at, (a, b) in enumerate(zip(want, got)):
        assert _equal_bits(a, b), at


# ---------------------------------------------------------------------------------------------------------- statistics
def _neighbourhoods(c, k, tau=None, body=0, queries=None):
    """(q [N,3] float32, index [N,k]) of one body of a cloud case by brute force."""
    x = c['queries'][body] if queries is None else queries
    _, index = pn.knn_brute_force(x, c['points'][body], k, shift=c['shift'][body], tau=tau)
    return pn.shifted(x, c['shift'][body]), index


@pytest.mark.parametrize('k', [3, 16, 32])
def test_covariance_and_count_equal_the_float32_statement(k):
    """cov == cov_f32 of the brute-force neighbour list in all bits, count == n; with tau some lists are partial."""
    c = cf.cloud_case('body122', 2, 257, 130)
    cloud = _cloud(c['points'])
    for tau in (None, 0.08):
        out = cloud.normals(_dev(c['queries']), k, shift=_dev(c['shift']), max_distance=tau, with_cov=True)
        cov, count = out.cov.cpu().numpy(), out.count.cpu().numpy()
        partial = 0
        for b in range(2):
            q, index = _neighbourhoods(c, k, tau, b)
            n = (index >= 0).sum(1)
            assert np.array_equal(count[b], n)
            partial += int(((n > 0) & (n < k)).sum())
            for i in range(130):
                want, _ = pn.cov_f32(q[i], c['points'][b][index[i, :n[i]]])
                assert np.array_equal(_bits(cov[b, i]), _bits(want)), (tau, b, i, cov[b, i], want)
        assert tau is None or partial > 0


def _compare_normals(c, k, out, body=0, view=None):
    """Per query of one body: (ratio angle / bound, ratio variation error / bound, zero?) against pca_f64 of the brute-force
    neighbours; asserts count and the orientation."""
    normal, variation, count = (t[body].cpu().numpy() for t in (out.normal, out.variation, out.count))
    q, index = _neighbourhoods(c, k, None, body)
    ratios, var_ratios, zero = [], [], []
    for i in range(len(q)):
        n = int((index[i] >= 0).sum())
        assert count[i] == n
        if not normal[i].any():
            zero.append(i)
            assert variation[i] == 0.0
            continue
        ref = pn.pca_f64(q[i], c['points'][body][index[i, :n]])
        bound = pn.error_bound(n, ref['total'])
        gap = ref['lam'][1] - ref['lam'][0]
        assert abs(float(np.linalg.norm(normal[i].astype(np.float64))) - 1.0) <= 4 * pn.U
        ratios.append(pn.angle(normal[i], ref['normal']) / (2 * bound / gap))
        want = ref['lam'][0] / ref['trace']
        var_ratios.append(abs(float(variation[i]) - want) / (2 * bound / ref['trace'] + 2 * pn.U))
        if view is None:
            assert pn.canonical(normal[i]), (i, normal[i])
        else:
            t = (np.asarray(view, F32) - q[i]).astype(F32)
            p = (normal[i] * t).astype(F32)
            assert F32(F32(p[0] + p[1]) + p[2]) >= 0, (i, normal[i], t)
    return np.asarray(ratios), np.asarray(var_ratios), zero


@pytest.mark.parametrize('num_points', [257, 4099])
@pytest.mark.parametrize('k', [3, 8, 16, 32])
def test_normals_and_variation_within_the_derived_bound(k, num_points):
    """Against pca_f64 of the same neighbours: the angle (sign removed) at most 2 E / (lambda1 - lambda0) with lambda from
    float64 -- the theorem bounds the sine; the angle itself is asserted, which asks more --, the variation within
    2 E / trace + 2 u.  For k in {8, 16, 32} the bound is not vacuous on these clouds (tests/test_point_normals_host.py:
    2 E / gap <= 0.014), so EVERY query must get a non-zero normal and none is left out; k = 3: the bound only, on the
    rows that are not zero.  Observed on an MI355X (2026-10-20), largest angle error / bound (variation error / bound), Q = 257 |
    4099: k = 3: 1.21e-3 (1.81e-3) | 1.43e-3 (1.00e-3); k = 8: 1.27e-3 (1.34e-3) | 1.55e-3 (1.45e-3); k = 16: 1.56e-3 (1.22e-3) |
    1.50e-3 (1.51e-3); k = 32: 1.34e-3 (1.53e-3) | 1.92e-3 (1.68e-3); zero rows: none, k = 3 included."""
    c = cf.cloud_case('body122', 1, num_points, 257)
    view = np.array([0.3, -0.2, 4.0], F32)
    cloud = _cloud(c['points'])
    worst = 0.0
    for v in (None, view):
        out = cloud.normals(_dev(c['queries']), k, None if v is None else _dev(v[None]), _dev(c['shift']))
        ratios, var_ratios, zero = _compare_normals(c, k, out, 0, v)
        if k >= 8:
            assert not zero, zero
        assert len(ratios) + len(zero) == 257 and len(ratios) > 128
        print('normals k=%d Q=%d: angle / bound %.3g, variation error / bound %.3g, zero rows %d'
              % (k, num_points, ratios.max(), var_ratios.max(), len(zero)))
        assert ratios.max() <= 1.0, ratios.max()
        assert var_ratios.max() <= 1.0, var_ratios.max()
        worst = max(worst, ratios.max())
    helpers.report_value('point normals k=%d Q=%d: largest angle error / bound' % (k, num_points), worst)


def test_zero_normals_exactly_where_the_rule_says():
    rng = np.random.default_rng(21)
    queries = (0.1 * rng.standard_normal((1, 65, 3))).astype(F32)
    line = np.zeros((1, 64, 3), F32)
    line[0, :, 0] = np.arange(64) * F32(0.125)                              # collinear along an axis, exact floats
    diagonal = np.repeat(np.arange(64, dtype=F32)[None, :, None] * F32(0.125), 3, 2)        # ... and along (1, 1, 1)
    same = np.tile(np.array([0.25, -0.5, 1.5], F32), (1, 64, 1))            # coincident
    for what, points in (('line', line), ('diagonal', diagonal), ('coincident', same)):
        out = _cloud(points).normals(_dev(queries), 8, with_cov=True)
        assert not out.normal.any().item() and not out.variation.any().item(), what
        assert torch.all(out.count == 8), what
    two = (rng.standard_normal((1, 2, 3))).astype(F32)                      # n < 3: two points; tau leaving fewer than 3
    out = _cloud(two).normals(_dev(queries), 8)
    assert not out.normal.any().item() and torch.all(out.count == 2)
    c = cf.cloud_case('body122', 1, 257, 130)
    out = _cloud(c['points']).normals(_dev(c['queries']), 8, shift=_dev(c['shift']), max_distance=0.1)
    count, normal = out.count.cpu().numpy()[0], out.normal.cpu().numpy()[0]
    assert (count < 3).any() and (count >= 3).any()
    assert not normal[count < 3].any()
    # a non-finite query and an entry beyond counts: nothing found, a zero row
    queries = c['queries'].copy()
    queries[0, 3] = np.nan
    out = _cloud(c['points']).normals(_dev(queries), 8, shift=_dev(c['shift']), counts=_dev(np.array([100], np.int32)),
                                      with_cov=True)
    for t in (out.normal, out.variation, out.count, out.cov):
        assert not t[0, 3].any().item() and not t[0, 100:].any().item()
    assert torch.all(out.count[0, :3] == 8)


def test_orientation():
    """s >= 0 against the viewpoint for every non-zero normal in both layouts (inside _compare_normals: the float32
    sequence of the rule); without one the canonical sign; an exact-float plane z = 0.125 seen from above."""
    c = cf.cloud_case('body122', 2, 257, 130)
    cloud = _cloud(c['points'])
    q, s = _dev(c['queries']), _dev(c['shift'])
    plain = cloud.normals(q, 16, shift=s)
    view = np.array([[0.5, 0.25, 3.0], [-4.0, 0.0, 0.5]], F32)
    per_body = cloud.normals(q, 16, _dev(view), s)
    rng = np.random.default_rng(22)
    each = (np.repeat(view[:, None], 130, 1) + rng.standard_normal((2, 130, 3))).astype(F32)
    per_query = cloud.normals(q, 16, _dev(each), s)
    flipped = 0
    for b in range(2):
        _compare_normals(c, 16, plain, b)
        _compare_normals(c, 16, per_body, b, view[b])
        normal = per_query.normal[b].cpu().numpy()
        qq = pn.shifted(c['queries'][b], c['shift'][b])
        t = (each[b] - qq).astype(F32)
        p = (normal * t).astype(F32)
        assert np.all(((p[:, 0] + p[:, 1]).astype(F32) + p[:, 2]).astype(F32) >= 0)
        for got in (per_body, per_query):                                   # the viewpoint changes the sign only
            a, w = got.normal[b], plain.normal[b]
            assert bool(((a == w).all(1) | (a == -w).all(1)).all())
        flipped += int((per_body.normal[b] != plain.normal[b]).any(1).sum())
    assert flipped > 0
    # the plane: the cloud's own points as queries, the sensor above
    pts = rng.standard_normal((1, 257, 3)).astype(F32)
    pts[:, :, 2] = 0.125
    out = _cloud(pts).normals(None, 16, _dev(np.array([[0.0, 0.0, 5.0]], F32)))
    normal = out.normal[0].cpu().numpy()
    _, index = pn.knn_brute_force(pts[0], pts[0], 16)
    for i in range(257):
        ref = pn.pca_f64(pts[0, i], pts[0][index[i]])
        bound = 2 * pn.error_bound(16, ref['total']) / (ref['lam'][1] - ref['lam'][0])
        assert normal[i, 2] > 0 and pn.angle(normal[i], [0, 0, 1]) <= bound, (i, normal[i], bound)
    below = _cloud(pts).normals(None, 16, _dev(np.array([[0.0, 0.0, -5.0]], F32)))
    assert torch.all(below.normal[0, :, 2] < 0)


# ---------------------------------------------------------------------------------------------------------- the fitter
@pytest.fixture(scope='module')
def smpl():
    from tuch_amd.models.smpl import SMPL
    return SMPL(model_data=sc.fit_inputs()['body'], batch_size=2).to(DEV)


@functools.lru_cache(maxsize=None)
def body_model():
    from tuch_amd.ops import ContactModel
    return ContactModel(sc.fit_inputs()['faces'], device=DEV)


def _scan():
    c = cf.cloud_case('body122', 2, 257, 1)
    go = np.zeros((2, 3), F32)
    view = np.array([[0.0, 0.0, 3.0], [1.0, 0.5, 3.0]], F32)
    return _dev(c['points']), _dev(go), _dev(view)


@pytest.mark.parametrize('model_to_scan', [0.0, 0.5])
def test_fitter_estimating_normals_is_the_fit_given_them(smpl, model_to_scan, monkeypatch):
    """ScanFitter(max_normal_angle, estimate_normals=16)(points, go, viewpoint=c) returns the bits, in every field, of the
    same fitter without the option called with normals=PointCloud(points).normals(k=16, viewpoint=c).normal."""
    from tuch_amd import ops
    from tuch_amd.fit import ScanFitter
    monkeypatch.setenv('TUCH_GRAPH_STRICT', '1')
    points, go, view = _scan()
    kw = dict(num_iters=20, fit_global_orient=False, max_normal_angle=60.0, model_to_scan=model_to_scan)
    with ops.deterministic_mode(True):
        normals = ops.PointCloud(points).normals(k=16, viewpoint=view).normal
        assert bool((normals.abs().sum(2) > 0).any())
        given_fitter = ScanFitter(smpl, body_model(), **kw)
        given = given_fitter(points, go, normals=normals)
        fitter = ScanFitter(smpl, body_model(), estimate_normals=16, **kw)
        got = fitter(points, go, viewpoint=view)
        assert fitter.graph_replayed == given_fitter.graph_replayed == {'fit': 17}
        assert list(fitter._sessions) == list(given_fitter._sessions)          # the session is that of a fit given normals
        for field, a, b in zip(given._fields, given, got):
            assert torch.equal(a, b), field
        if model_to_scan > 0:
            for field, a, b in zip(fitter.model_to_scan_result._fields, fitter.model_to_scan_result,
                                   given_fitter.model_to_scan_result):
                assert torch.equal(a, b), field
        again = fitter(points, go, viewpoint=view)                          # the kept session: replays only
        assert fitter.graph_replayed == {'fit': 20} and len(fitter._sessions) == 1
        for field, a, b in zip(given._fields, given, again):
            assert torch.equal(a, b), ('kept session', field)
        held = next(iter(fitter._sessions.values()))['t']['normals']         # what the loop read
        assert torch.equal(held.view(torch.int32), normals.view(torch.int32))


def test_fitter_without_the_option_is_unchanged(smpl):
    """Without estimate_normals nothing of it exists: the session key is the one a fit without the option has always had
    (17 entries, none about the estimate), no cloud is built, and the loop is replayed as before."""
    from tuch_amd import ops
    from tuch_amd.fit import ScanFitter
    points, go, _ = _scan()
    with ops.deterministic_mode(True):
        fitter = ScanFitter(smpl, body_model(), num_iters=20, fit_global_orient=False, max_normal_angle=60.0)
        assert fitter.estimate_normals is None
        first = fitter(points, go)
        assert fitter.graph_replayed == {'fit': 17} and len(fitter._sessions) == 1
        key, sess = next(iter(fitter._sessions.items()))
        assert key == (2, 257, False, False, 0, 0.01, False, 'distance', None, True, False, 0.0, None, None, 64, False, None)
        assert sess['cloud'] is None and sess['normals_cloud'] is None and sess['t']['normals'] is None
        second = ScanFitter(smpl, body_model(), num_iters=20, fit_global_orient=False)(points, go)
        for field, a, b in zip(first._fields, first, second):
            assert torch.equal(a, b), field
        with pytest.raises(ValueError, match='viewpoint needs estimate_normals'):
            fitter(points, go, viewpoint=torch.zeros(2, 3, device=DEV))
