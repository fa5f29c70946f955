"""Posed vertex normals, the normal-compatible nearest point of a cloud, its term and ScanFitter(model_to_scan_normals=True)
on the device, against the restatements of tests/oriented_cloud_cases.py (checked against float64 in
tests/test_oriented_cloud_host.py)."""
import functools

import numpy as np
import pytest
import torch

import closest_point_cases as cc
import cloud_fit_cases as cf
import helpers
import oriented_cloud_cases as oc
import scan_fit_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
RESOLUTIONS = (1, 4, 64)


def _dev(a, **kw):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV, **kw)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _equal_bits(got, want):
    """The same bits; where the rule gives NaN (a NaN body's raw rows) a NaN of any payload."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _same(got, want, what=''):
    assert np.array_equal(got[1], want[1]), (what, np.nonzero(np.asarray(got[1]) != np.asarray(want[1])))
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what


def _cloud(points, normals, counts=None, weights=None, resolution=64, cones=True):
    from tuch_amd.ops import PointCloud
    return PointCloud(_dev(points), _dev(counts), _dev(weights), resolution).orient(_dev(normals), cones=cones)


def _nearest(cloud, queries, query_normals, angle, shift=None, counts=None, hint=None, tau=None):
    out = cloud.nearest(_dev(queries), _dev(shift), _dev(counts), None if hint is None else _dev(hint), tau,
                        query_normals=_dev(query_normals), max_angle=angle)
    return out.d2.cpu().numpy(), out.index.cpu().numpy()


def _check(c, angle, counts=None, weights=None, tau=None, query_counts=None, resolutions=RESOLUTIONS, shift='case', what=''):
    """Every resolution, with cones and without, against the oriented brute force; returns the brute-force (d2, index)."""
    shift = c['shift'] if isinstance(shift, str) else shift
    want = oc.brute_force_batch(c['queries'], c['query_normals'], c['points'], c['normals'], oc.cos32(angle), counts, weights,
                                shift, tau, query_counts)
    for res in resolutions:
        for cones in (True, False):
            cloud = _cloud(c['points'], c['normals'], counts, weights, res, cones)
            assert (cloud._cones is not None) == cones
            _same(_nearest(cloud, c['queries'], c['query_normals'], angle, shift, query_counts, None, tau), want,
                  (what, res, cones))
    return want


# ---------------------------------------------------------------------------------------------------------- vertex normals
@functools.lru_cache(maxsize=None)
def _ico6_posed():
    import torch as t
    from oracle import lbs as ol
    c = sc.fit_inputs()
    m = ol.model_tensors(c['body'], t.float64)
    f = lambda a: t.as_tensor(a, dtype=t.float64)
    return ol.smpl_forward(m, f(c['true_betas']), f(c['true_body_pose']), f(c['global_orient']))[0].numpy().astype(F32), c['faces']


def _normal_meshes():
    for name in ('tetrahedron', 'icosphere', 'strip', 'degenerate'):
        verts, faces = cc.mesh(name)
        yield name, verts[0], faces
    v, faces = _ico6_posed()
    yield 'ico6', v[0], faces
    # V = 63, 64, 65: strips of 61, 62, 63 faces
    for num_faces in (61, 62, 63):
        verts, faces = cc.open_strip(num_faces)
        yield 'strip%d' % len(verts), verts, faces


def test_vertex_normals_equal_the_restatement_bit_for_bit():
    from tuch_amd import ops
    sizes = set()
    for name, verts, faces in _normal_meshes():
        num_verts = len(verts)
        sizes.add(num_verts)
        off, ids = oc.vertex_table(faces, num_verts)
        table = ops.vertex_normal_table(faces, num_verts, DEV)
        assert torch.equal(table.off.cpu(), torch.as_tensor(off)) and torch.equal(table.ids.cpu(), torch.as_tensor(ids))
        batch = cc.body_batch(verts, 3, 5)
        batch[1, ::3] = np.nan                                   # a NaN body between two clean ones
        for normalize in (False, True):
            want = np.stack([oc.vertex_normals32(b, faces, off, ids, normalize) for b in batch])
            got = ops.vertex_normals(_dev(batch), table, normalize).cpu().numpy()
            assert _equal_bits(got, want), (name, normalize)
            for b in (0, 2):                                     # a body alone: the same bits, the NaN body changed nothing
                alone = ops.vertex_normals(_dev(batch[b:b + 1]), table, normalize).cpu().numpy()
                assert np.array_equal(_bits(alone[0]), _bits(want[b])) and not np.isnan(want[b]).any(), (name, normalize, b)
            if normalize:
                assert np.all(np.isfinite(got)) and not got[1, ::3].any()
                if name == 'degenerate':
                    assert (~got[0].any(1)).any()               # the vertices of faces without area: zero rows
        # captured and replayed
        v = _dev(batch)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.vertex_normals(v, table, True)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = ops.vertex_normals(v, table, True)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), name
    assert {63, 64, 65} <= sizes
    with pytest.raises(ValueError, match='table'):
        ops.vertex_normals(_dev(batch[:, :5]), table)
    with pytest.raises(ValueError, match='VertexNormalTable'):
        ops.vertex_normals(_dev(batch), None)


# ---------------------------------------------------------------------------------------------------------- the query
@pytest.mark.parametrize('num_queries', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('num_points', [1, 64, 65, 257, 4099])
@pytest.mark.parametrize('batch', [1, 3])
def test_oriented_search_equals_brute_force(batch, num_points, num_queries):
    name = 'icosphere' if (num_points + num_queries) % 2 else 'body122'
    c = oc.cloud_case(name, batch, num_points, num_queries)
    angle = oc.ANGLES[(num_points + num_queries + batch) % 3]
    d2, index = _check(c, angle, what=(name, batch, num_points, num_queries, angle))
    tau = 0.03
    _, within = _check(c, angle, tau=tau, what=('tau', name, batch, num_points, num_queries, angle))
    if num_points >= 257 and num_queries >= 64:                  # the case exercises the rule and the limit
        plain = cf.brute_force_batch(c['queries'], c['points'], shift=c['shift'])
        assert (index != plain[1]).any() and (index >= 0).all() and (within < 0).any() and (within >= 0).any()


@pytest.mark.parametrize('angle', oc.ANGLES)
@pytest.mark.parametrize('kinds', [('true',), ('true', 'flipped'), ('true', 'random'), ('true', 'zero'), oc.KINDS])
def test_every_kind_of_normal_and_every_angle(angle, kinds):
    for query_kinds in (('true',), oc.KINDS):
        c = oc.cloud_case('body122', 2, 257, 130, kinds, query_kinds)
        _check(c, angle, what=(angle, kinds, query_kinds))
    _check(c, angle, shift=None, resolutions=(64,), what='no shift')


def test_ragged_counts_zero_weights_and_non_finite_points():
    c = dict(oc.cloud_case('body122', 3, 257, 130))
    rng = np.random.default_rng(5)
    points, normals = c['points'].copy(), c['normals'].copy()
    weights = (rng.random(points.shape[:2]) + 0.1).astype(F32)
    weights[rng.random(points.shape[:2]) < 0.3] = 0.0
    points[weights == 0] = np.nan                                # never to be read
    points[0, 5] = np.inf
    points[1, 7, 1] = np.nan
    normals[2, ::9] = np.nan                                     # a non-finite normal: unconstrained
    normals[0, 1::9] = np.inf
    counts = np.array([257, 64, 130], np.int32)
    query_counts = np.array([130, 1, 65], np.int32)
    c.update(points=points, normals=normals)
    d2, index = _check(c, 60.0, counts, weights, what='ragged')
    for b in range(3):
        assert np.all(index[b] < counts[b])
        assert np.all(weights[b][index[b][index[b] >= 0]] != 0)
    d2, index = _check(c, 60.0, counts, weights, tau=0.05, query_counts=query_counts, what='ragged + query counts')
    for b in range(3):
        assert np.all(index[b, query_counts[b]:] == -1) and np.all(np.isposinf(d2[b, query_counts[b]:]))
    queries = c['queries'].copy()
    queries[0, 3] = np.nan
    c.update(queries=queries)
    d2, index = _check(c, 60.0, counts, weights, what='non-finite query', resolutions=(4,))
    assert index[0, 3] == -1


@pytest.mark.parametrize('angle', oc.ANGLES)
def test_threshold_pairs_are_decided_by_the_rule(angle):
    t = oc.threshold_case(angle)
    own = np.repeat(np.arange(64), 4)
    adm = oc.pair_rule32(t['query_normals'][0], t['normals'][0][own], oc.cos32(angle), diagonal=True)
    t = dict(t, shift=None)
    d2, index = _check(t, angle, shift=None, what=('threshold', angle))
    # 1 mm above its own point, decimetres from the next: an admissible own point is the answer
    assert np.array_equal(index[0][adm], own[adm]) and np.all(index[0][~adm] != own[~adm])
    assert adm.reshape(64, 4)[:, 2].all() and not adm.reshape(64, 4)[:, 3].any()


def test_every_hint_gives_the_unhinted_bits():
    c = oc.cloud_case('body122', 3, 257, 130)
    rng = np.random.default_rng(9)
    counts = np.array([257, 64, 130], np.int32)
    weights = np.where(rng.random(c['points'].shape[:2]) < 0.2, 0.0, 1.0).astype(F32)
    want = oc.brute_force_batch(c['queries'], c['query_normals'], c['points'], c['normals'], oc.cos32(60.0), counts, weights,
                                c['shift'], 0.05)
    plain = cf.brute_force_batch(c['queries'], c['points'], counts, weights, c['shift'], 0.05)
    assert (plain[1] != want[1]).any()                           # 'unoriented': an inadmissible hint for those queries
    for cones in (True, False):
        cloud = _cloud(c['points'], c['normals'], counts, weights, 64, cones)
        for kind in cf.HINT_KINDS + ('unoriented',):
            hint = plain[1] if kind == 'unoriented' else cf.hints(kind, c['queries'], c['shift'], c['points'], counts, weights,
                                                                    np.maximum(want[1], 0))
            _same(_nearest(cloud, c['queries'], c['query_normals'], 60.0, c['shift'], None, hint, 0.05), want, (kind, cones))
        # the hint tensor may be the output
        both = _dev(plain[1])
        out = cloud.nearest(_dev(c['queries']), _dev(c['shift']), hint=both, max_distance=0.05, index_out=both,
                            query_normals=_dev(c['query_normals']), max_angle=60.0)
        assert out.index is both
        _same((out.d2.cpu().numpy(), both.cpu().numpy()), want, 'aliased')


def test_invariance_of_the_bits():
    c = oc.cloud_case('icosphere', 3, 257, 130)
    want = oc.brute_force_batch(c['queries'], c['query_normals'], c['points'], c['normals'], oc.cos32(60.0), shift=c['shift'])
    rng = np.random.default_rng(2)
    pp, qp = rng.permutation(257), rng.permutation(130)
    moved = dict(c, points=c['points'][:, pp], normals=c['normals'][:, pp], queries=c['queries'][:, qp],
                 query_normals=c['query_normals'][:, qp])
    for cones in (True, False):
        d2, index = _nearest(_cloud(moved['points'], moved['normals'], cones=cones), moved['queries'], moved['query_normals'],
                             60.0, c['shift'])
        assert np.array_equal(_bits(d2), _bits(want[0][:, qp]))
        # (equal distances may name another of the permuted points only where two points tie in the bits: none here)
        assert np.array_equal(np.where(index >= 0, pp[np.maximum(index, 0)], -1), want[1][:, qp])
        for b in range(3):                                       # a body alone
            one = _nearest(_cloud(c['points'][b:b + 1], c['normals'][b:b + 1], cones=cones), c['queries'][b:b + 1],
                           c['query_normals'][b:b + 1], 60.0, c['shift'][b:b + 1])
            _same((one[0][0], one[1][0]), (want[0][b], want[1][b]), ('alone', b))
    # captured and replayed
    cloud = _cloud(c['points'], c['normals'])
    q, u, sh = _dev(c['queries']), _dev(c['query_normals']), _dev(c['shift'])
    call = lambda: cloud.nearest(q, sh, query_normals=u, max_angle=60.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        _same((out.d2.cpu().numpy(), out.index.cpu().numpy()), want, 'replayed')


def test_a_cloud_whose_normals_all_face_away():
    """Every point carries -u0, every query u0 or no normal (a zero or a NaN row): the constrained queries get -1 / +inf
    -- with the cones every block is passed by --, the others tuch_point_cloud_nearest's bits."""
    c = oc.cloud_case('icosphere', 2, 257, 130)
    u0 = np.array([0.3, -0.5, 0.8], F32)
    normals = np.broadcast_to(-u0, c['points'].shape).copy()
    qn = np.broadcast_to(u0, c['queries'].shape).copy()
    qn[:, ::4] = 0.0
    qn[:, 1::8] = np.nan
    free = ~(np.isfinite(qn).all(2) & (qn != 0).any(2))
    plain = cf.brute_force_batch(c['queries'], c['points'], shift=c['shift'])
    for cones in (True, False):
        for res in (4, 64):
            got = _nearest(_cloud(c['points'], normals, resolution=res, cones=cones), c['queries'], qn, 60.0, c['shift'])
            assert np.all(got[1][~free] == -1) and np.all(np.isposinf(got[0][~free]))
            assert np.array_equal(got[1][free], plain[1][free]) and np.array_equal(_bits(got[0][free]), _bits(plain[0][free]))


def test_nearest_oriented_is_differentiable_with_the_index_held_fixed():
    c = oc.cloud_case('icosphere', 2, 257, 65)
    cloud = _cloud(c['points'], c['normals'])
    q, sh = _dev(c['queries'], requires_grad=True), _dev(c['shift'], requires_grad=True)
    out = cloud.nearest(q, sh, query_normals=_dev(c['query_normals']), max_angle=60.0)
    won = out.index >= 0
    torch.where(won, out.d2, torch.zeros_like(out.d2)).sum().backward()
    idx = out.index.cpu().numpy()
    x = (c['queries'] + c['shift'][:, None]).astype(np.float64)
    s = np.stack([c['points'][b][np.maximum(idx[b], 0)] for b in range(2)]).astype(np.float64)
    want = np.where((idx >= 0)[:, :, None], 2.0 * (x - s), 0.0)
    ok, ratio = sc.grad_within(q.grad.cpu().numpy(), want)
    assert ok, ratio
    ok, ratio = sc.grad_within(sh.grad.cpu().numpy(), want.sum(1))
    assert ok, ratio


# ---------------------------------------------------------------------------------------------------------- the term
def _term(c, cloud=None, hint=None, scale=None, index_out=None, cones=True, verts=None):
    from tuch_amd import ops
    if cloud is None:
        cloud = _cloud(c['points'], c['normals'], c['counts'], c['weights'], cones=cones)
    v = _dev(c['verts'] if verts is None else verts, requires_grad=True)
    tr = _dev(c['transl'], requires_grad=True)
    table = ops.vertex_normal_table(c['faces'], v.shape[1], DEV)
    total, per, near = ops.cloud_fit(cloud, v, tr, _dev(c['vw']), hint, c['rho'], c['sigma'], c['tau'], c['scale'],
                                     index_out=index_out, max_angle=c['angle'], normal_table=table)
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
    """per_body and total against the float64 statement over the float32 admissible set, within the bound of the
    unoriented term's test; index / d2 are the oriented query's on vertex_normals' raw rows, bit for bit."""
    from tuch_amd import ops
    c = oc.term_case('body122', rho, weighted, tau)
    cloud = _cloud(c['points'], c['normals'], c['counts'])
    got, near = _term(c, cloud)
    err = np.abs(got['per'].astype(np.float64) - c['ref'][0])
    helpers.report_value('oriented cloud_fit body122 %s weights=%s tau=%d: largest per-body error / bound' % (rho, weighted, tau),
                         (err / c['bound']).max())
    print('oriented cloud_fit', rho, weighted, tau, 'per_body error', err, 'bound', c['bound'])
    assert np.all(c['ref'][0] > 0)
    assert np.all(err <= c['bound']), (err, c['bound'])
    assert abs(got['total'] - c['ref'][1]) <= c['bound'].sum()
    table =ops.vertex_normal_table(c['faces'], c['verts'].shape[1], DEV)
    rows = ops.vertex_normals(_dev(c['verts']), table)
    query = cloud.nearest(_dev(c['verts']), _dev(c['transl']), max_distance=c['tau'], query_normals=rows, max_angle=c['angle'])
    live = torch.ones_like(query.index, dtype=torch.bool) if c['vw'] is None else \
        (_dev(c['vw']) != 0).expand(query.index.shape)
    assert torch.equal(near.index[live], query.index[live]) and torch.equal(near.d2[live], query.d2[live])
    assert torch.all(near.index[~live] == -1) and torch.all(torch.isposinf(near.d2[~live]))
    index32 = np.stack(c['index32'])
    assert np.array_equal(near.index.cpu().numpy(), index32)
    plain = cloud.nearest(_dev(c['verts']), _dev(c['transl']), max_distance=c['tau'])
    assert (near.index[live] != plain.index[live]).any() and (near.index[live] >= 0).any()
    # a hint changes nothing, index_out may be the hint tensor, and the cones change nothing
    both = plain.index.clone()
    again, out = _term(c, cloud, hint=both, index_out=both)
    assert out.index is both and torch.equal(both, near.index) and torch.equal(out.d2, near.d2)
    bare, _ = _term(c, cones=False)
    for key in got:
        assert np.array_equal(got[key], again[key]) and np.array_equal(got[key], bare[key]), key


@pytest.mark.parametrize('rho', sc.RHOS)
def test_gradients_against_central_differences(rho):
    """At the vertices whose best and second-best ADMISSIBLE points differ by >= 1 mm in distance (and which have a
    match): central differences of the float64 statement with the match held by the gap."""
    from tuch_amd import ops
    c = oc.term_case('body122', rho)
    cos, step = oc.cos32(c['angle']), 1e-6
    off, ids = oc.vertex_table(c['faces'], c['verts'].shape[1])
    for mode in (True, False):
        with ops.deterministic_mode(mode):
            got, near = _term(c)
        worst, used = 0.0, 0
        for b in range(len(c['verts'])):
            n = int(c['counts'][b])
            pts, nrm = c['points'][b, :n], c['normals'][b, :n]
            q = (c['verts'][b] + c['transl'][b][None]).astype(np.float64)
            adm = oc.pair_rule32(oc.vertex_normals32(c['verts'][b], c['faces'], off, ids), nrm, cos)
            dist = np.where(adm, np.sqrt(((q[:, None] - pts.astype(np.float64)[None]) ** 2).sum(-1)), np.inf)
            two = np.sort(dist, 1)[:, :2]
            clear = np.isfinite(two[:, 0]) & (two[:, 1] - two[:, 0] >= cf.GRAD_GAP) & (two[:, 0] >= 1e-3)
            assert clear.sum() >= 20
            idx = dist.argmin(1)
            # the match is fixed by the gap (a 1e-6 step moves no distance by 1 mm, and a vertex's own normal only through
            # its neighbours' steps, which the per-vertex differences below do not take)
            s = pts.astype(np.float64)[idx]
            w = 1.0 / len(q)
            for k in range(3):
                d = np.zeros(3)
                d[k] = step
                f = lambda x: c['scale'] * w * sc.rho_numpy(((x - s) ** 2).sum(1), rho, c['sigma'])
                want = (f(q + d) - f(q - d)) / (2 * step)
                ok, ratio = sc.grad_within(got['gv'][b][clear, k], want[clear])
                worst = max(worst, ratio)
                assert ok, (rho, mode, b, k, ratio)
            used += int(clear.sum())
        helpers.report_value('oriented cloud_fit %s grad_verts, deterministic=%d, %d vertices: error / bound' % (rho, mode, used),
                             worst)
        ok, ratio = sc.grad_within(got['gt'], got['gv'].astype(np.float64).sum(1))
        assert ok, ratio


def test_equal_bits_twice_alone_and_in_both_modes():
    from tuch_amd import ops
    from tuch_amd.ops._base import _ticket
    results = []
    c = oc.term_case('body122', 'gmof', 'BV', True)
    for mode in (True, False):
        with ops.deterministic_mode(mode):
            first, second, third = _term(c)[0], _term(c)[0], _term(c)[0]
            for key in first:
                assert np.array_equal(first[key], second[key]) and np.array_equal(first[key], third[key]), key
            for b in range(3):
                one = dict(c, verts=c['verts'][b:b + 1], transl=c['transl'][b:b + 1], points=c['points'][b:b + 1],
                           normals=c['normals'][b:b + 1], vw=c['vw'][b:b + 1], counts=c['counts'][b:b + 1])
                alone, _ = _term(one)
                assert alone['per'][0] == first['per'][b] and alone['total'] == first['per'][b]
                assert np.array_equal(alone['gv'][0], first['gv'][b]) and np.array_equal(alone['gt'][0], first['gt'][b])
        results.append(first)
    for key in results[-1]:
        assert np.array_equal(results[-1][key], results[-2][key]), key
    assert int(_ticket(torch.device(DEV)).item()) == 0


def test_unconstrained_oriented_calls_have_the_plain_calls_bits():
    """There is one query path: with all-zero query normals (nearest) or all-zero point normals (the term) every pair is
    unconstrained and the oriented entry points return the plain ones' tensors, torch.equal.  Batch 2, 257 points with
    ragged counts, 257 queries, resolution 8: several 4^3 blocks, a partial last workgroup, a wavefront boundary.  (That
    the reference agrees is tests/test_oriented_cloud_host.py's.)"""
    from tuch_amd import ops
    c = oc.cloud_case('body122', 2, 257, 257, ('true',))
    counts = np.array([257, 130], np.int32)
    queries, shift, zeros = _dev(c['queries']), _dev(c['shift']), torch.zeros(2, 257, 3, device=DEV)
    for cones in (True, False):
        cloud = _cloud(c['points'], c['normals'], counts, None, 8, cones)
        assert (cloud._cones is not None) == cones
        answers = cloud.nearest(queries, shift).index
        assert (answers >= 0).all()
        for hint in (None, answers):
            for tau in (None, 0.03):
                plain = cloud.nearest(queries, shift, hint=hint, max_distance=tau)
                got = cloud.nearest(queries, shift, hint=hint, max_distance=tau, query_normals=zeros, max_angle=60.0)
                assert torch.equal(got.d2, plain.d2) and torch.equal(got.index, plain.index), (cones, hint is None, tau)
                if tau is not None:                              # the limit is exercised
                    assert (plain.index < 0).any() and (plain.index >= 0).any()
    t = oc.term_case('body122', 'gmof', 'BV', True)
    cloud = _cloud(t['points'], np.zeros_like(t['normals']), t['counts'], t['weights'])
    table = ops.vertex_normal_table(t['faces'], t['verts'].shape[1], DEV)
    for mode in (True, False):
        for tau in (None, t['tau']):
            with ops.deterministic_mode(mode):
                out = []
                for extra in ({}, dict(max_angle=60.0, normal_table=table)):
                    v, tr = _dev(t['verts'], requires_grad=True), _dev(t['transl'], requires_grad=True)
                    total, per, near = ops.cloud_fit(cloud, v, tr, _dev(t['vw']), None, t['rho'], t['sigma'], tau, t['scale'],
                                                     **extra)
                    ops.backward_scalar(total)
                    out.append(dict(total=total.detach(), per_body=per, d2=near.d2, index=near.index, grad_verts=v.grad,
                                    grad_transl=tr.grad))
            for key in out[0]:
                assert torch.equal(out[0][key], out[1][key]), (key, mode, tau)
            assert (out[0]['index'] >= 0).any() and out[0]['grad_verts'].abs().sum() > 0
            if tau is not None:
                assert (out[0]['index'] < 0).any()


def test_term_workspace_guards_and_capture():
    from tuch_amd import ops
    c = oc.term_case('body122', 'distance', 'V', True)
    want, near = _term(c)
    was = ops.set_cloud_canary(True)
    try:
        guarded = _cloud(c['points'], c['normals'], c['counts'], resolution=64)
        got, _ = _term(c, guarded)
        guarded.nearest(_dev(c['verts']), _dev(c['transl']), query_normals=_dev(c['verts']), max_angle=30.0)
        guarded.rebuild(_dev(c['points']), _dev(c['counts']))
        assert guarded.point_normals is None and guarded._cones is None
        guarded.orient(_dev(c['normals']))
        assert guarded.canary_hits() == 0
        for key in want:
            assert np.array_equal(want[key], got[key]), key
    finally:
        ops.set_cloud_canary(was)
    cloud = _cloud(c['points'], c['normals'], c['counts'])
    v, tr, vw = _dev(c['verts']), _dev(c['transl']), _dev(c['vw'])
    table = ops.vertex_normal_table(c['faces'], v.shape[1], DEV)
    hint = torch.full(tuple(v.shape[:2]), -1, dtype=torch.int32, device=DEV)
    call = lambda: ops.cloud_fit(cloud, v, tr, vw, hint, c['rho'], c['sigma'], c['tau'], c['scale'], index_out=hint,
                                 max_angle=c['angle'], normal_table=table)
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
    c = oc.term_case('body122', 'distance')
    points, v, tr, nrm = _dev(c['points']), _dev(c['verts']), _dev(c['transl']), _dev(c['normals'])
    table = ops.vertex_normal_table(c['faces'], v.shape[1], DEV)
    cloud = PointCloud(points)
    with pytest.raises(ValueError, match='oriented cloud'):
        cloud.nearest(v, query_normals=v, max_angle=60.0)
    with pytest.raises(ValueError, match='oriented cloud'):
        ops.cloud_fit(cloud, v, tr, max_angle=60.0, normal_table=table)
    with pytest.raises(ValueError, match='normals'):
        cloud.orient(nrm[:, :5])
    with pytest.raises(RuntimeError, match='HIP device'):
        cloud.orient(nrm.cpu())
    cloud.orient(nrm)
    with pytest.raises(ValueError, match='go together'):
        cloud.nearest(v, query_normals=v)
    with pytest.raises(ValueError, match='go together'):
        cloud.nearest(v, max_angle=60.0)
    with pytest.raises(ValueError, match='query_normals'):
        cloud.nearest(v, query_normals=v[:, :5], max_angle=60.0)
    with pytest.raises(ValueError, match='max_angle'):
        cloud.nearest(v, query_normals=v, max_angle=120.0)
    with pytest.raises(ValueError, match='go together'):
        ops.cloud_fit(cloud, v, tr, max_angle=60.0)
    with pytest.raises(ValueError, match='table'):
        ops.cloud_fit(cloud, v[:, :50], tr, max_angle=60.0, normal_table=table)
    cloud.rebuild(points)
    with pytest.raises(ValueError, match='oriented cloud'):
        cloud.nearest(v, query_normals=v, max_angle=60.0)
    assert cloud.nearest(v).index.shape == (3, v.shape[1])          # the plain query is untouched


# ---------------------------------------------------------------------------------------------------------- the fitter
@functools.lru_cache(maxsize=None)
def _front():
    from tuch_amd.models.smpl import SMPL
    from tuch_amd.ops import ContactModel
    s = oc.front_scan()
    return s, SMPL(model_data=s['body'], batch_size=1).to(DEV), ContactModel(s['faces'], device=DEV)


def _front_fit(num_iters, flag, **kw):
    from tuch_amd.fit import ScanFitter
    s, smpl, model = _front()
    kw.setdefault('max_normal_angle', oc.FEATURE_ANGLE)
    extra = dict(model_to_scan_normals=flag) if flag is not None else {}
    fitter = ScanFitter(smpl, model, num_iters=num_iters, fit_global_orient=False, model_to_scan=1.0, **extra, **kw)
    call = {} if kw.get('estimate_normals') else dict(normals=_dev(s['normals']))
    if kw.get('estimate_normals'):
        call['viewpoint'] = _dev(np.asarray([oc.FEATURE_VIEWPOINT], F32))
    return fitter, fitter(_dev(s['points']), _dev(s['global_orient']), **call)


def test_flag_off_is_the_fitter_without_the_argument():
    from tuch_amd import ops
    with ops.deterministic_mode(True):
        plain_fitter, plain = _front_fit(20, None)
        off_fitter, off = _front_fit(20, False)
        on_fitter, on = _front_fit(20, True)
    for field, a, b in zip(plain._fields, plain, off):
        assert torch.equal(a, b), field
    for field, a, b in zip(plain_fitter.model_to_scan_result._fields, plain_fitter.model_to_scan_result,
                           off_fitter.model_to_scan_result):
        assert torch.equal(a, b), field
    assert plain_fitter.graph_replayed == off_fitter.graph_replayed == on_fitter.graph_replayed == {'fit': 17}
    sess = next(iter(off_fitter._sessions.values()))
    assert sess['oriented'] == {} and sess['cloud'].point_normals is None
    assert not torch.equal(on.body_pose, plain.body_pose)
    assert (on_fitter.model_to_scan_result.index == -1).any() and torch.all(off_fitter.model_to_scan_result.index >= 0)


def test_hint_graph_resolution_and_sessions_change_no_bit(monkeypatch):
    from tuch_amd import ops
    monkeypatch.setenv('TUCH_GRAPH_STRICT', '1')
    s, _, _ = _front()
    rng = np.random.default_rng(3)
    moved = _dev((s['points'] + 0.01 * rng.standard_normal(s['points'].shape)).astype(F32))

    def same(a, fa, b, fb, what):
        for field, x, y in zip(a._fields, a, b):
            assert torch.equal(x, y), (what, field)
        for field, x, y in zip(fa.model_to_scan_result._fields, fa.model_to_scan_result, fb.model_to_scan_result):
            assert torch.equal(x, y), (what, 'model_to_scan_result', field)
    with ops.deterministic_mode(True):
        hinted, first = _front_fit(20, True, use_hint=True, max_distance=0.5)
        assert hinted.graph_replayed == {'fit': 17} and len(hinted._sessions) == 1
        for name, kw in (('use_hint=False', dict(use_hint=False)), ('eager', dict(use_hint=True, use_graph=False)),
                         ('resolution', dict(resolution=16))):
            f, fit = _front_fit(20, True, max_distance=0.5, **kw)
            same(first, hinted, fit, f, name)
        go, nrm = _dev(s['global_orient']), _dev(s['normals'])
        second = hinted(moved, go, normals=nrm)                  # the kept session: replays only, cloud rebuilt and oriented
        assert hinted.graph_replayed == {'fit': 20} and len(hinted._sessions) == 1
        from tuch_amd.fit import ScanFitter
        _, smpl, model = _front()
        fresh_fitter = ScanFitter(smpl, model, num_iters=20, fit_global_orient=False, model_to_scan=1.0, max_distance=0.5,
                                  max_normal_angle=oc.FEATURE_ANGLE, model_to_scan_normals=True)
        fresh = fresh_fitter(moved, go, normals=nrm)
        same(second, hinted, fresh, fresh_fitter, 'kept session')
        assert not torch.equal(first.body_pose, second.body_pose)


def test_trajectory_follows_the_float64_loop():
    """The parameters before each of the first 10 updates against the float64 CPU loop, within 4 x the float32 CPU loop's
    own deviation, floored at sc.TRAJECTORY_FLOOR (the float32 loop holds the floor: tests/test_oriented_cloud_host.py)."""
    holds, bound = oc.trajectory_bound()
    assert holds
    ref = oc.trajectory()
    fitter, _ = _front_fit(oc.TRAJECTORY_PREFIX, True, record_history=True)
    history = fitter.history['fit']
    assert len(history) == oc.TRAJECTORY_PREFIX
    worst = 0.0
    for it in range(oc.TRAJECTORY_PREFIX):
        dev = max(float(np.abs(g.cpu().numpy().astype(np.float64) - w).max()) for g, w in zip(history[it]['params'], ref['params'][it]))
        print('iteration', it, 'deviation', dev, 'bound', bound[it])
        worst = max(worst, dev / bound[it])
        assert dev <= bound[it], (it, dev, bound[it])
    helpers.report_value('ScanFitter model_to_scan_normals: parameters vs float64 over %d iterations, error / bound'
                         % oc.TRAJECTORY_PREFIX, worst)
    np.testing.assert_allclose(history[0]['loss'].item(), ref['loss'][0].sum(), rtol=1e-4)


def test_fitter_argument_errors():
    from tuch_amd.fit import ScanFitter
    s, smpl, model = _front()
    with pytest.raises(ValueError, match='model_to_scan_normals'):
        ScanFitter(smpl, model, model_to_scan_normals=True, max_normal_angle=60.0)
    with pytest.raises(ValueError, match='model_to_scan_normals'):
        ScanFitter(smpl, model, model_to_scan_normals=True, model_to_scan=1.0)
    fitter = ScanFitter(smpl, model, num_iters=2, model_to_scan_normals=True, model_to_scan=1.0, max_normal_angle=60.0)
    with pytest.raises(ValueError, match='normals at the call'):
        fitter(_dev(s['points']), _dev(s['global_orient']))


@pytest.mark.parametrize('estimated', [False, True])
def test_a_front_only_scan_no_longer_flattens_the_body(estimated):
    """What the feature is for: a scan that sees one side of the body (the ico-6 body's front vertices, a sensor on +z),
    the fit started at the true pose.  The plain two-sided fit pulls the back vertices to the front points; with
    model_to_scan_normals they have no match and stay.  The float64 CPU loops: 15.6 mm against 5.6 mm after 40
    iterations (tests/test_oriented_cloud_host.py); only the ordering is asserted here.  estimated: the normals come from
    the points (estimate_normals=16, viewpoint=)."""
    s, _, _ = _front()
    true = _dev(s['true'].astype(F32))
    kw = dict(estimate_normals=16) if estimated else {}
    dist = {}
    for name, flag in (('two_sided', False), ('oriented', True)):
        fitter, fit = _front_fit(oc.FEATURE_ITERS, flag, **kw)
        dist[name] = (fit.vertices[0] - true).norm(dim=1).mean().item()
        if flag:
            share = (fitter.model_to_scan_result.index >= 0).float().mean().item()
    print('front-only scan, estimated=%d' % estimated, dist, 'matched share', share)
    helpers.report_value('front-only scan, estimated=%d: oriented / plain two-sided distance' % estimated,
                         dist['oriented'] / dist['two_sided'])
    assert dist['oriented'] < dist['two_sided'], dist
    assert 0.5 < share < 1.0, share
