"""The restatements of tests/oriented_cloud_cases.py against float64, and the case the feature is for, on the CPU."""
import numpy as np
import pytest

import closest_point_cases as cc
import cloud_fit_cases as cf
import oriented_cloud_cases as oc
import scan_fit_cases as sc

F32 = np.float32
MESHES = ('tetrahedron', 'icosphere', 'strip', 'degenerate')


def _posed_body():
    c = sc.fit_inputs()
    from oracle import lbs as ol
    import torch
    m = ol.model_tensors(c['body'], torch.float64)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    verts = ol.smpl_forward(m, t(c['true_betas']), t(c['true_body_pose']), t(c['global_orient']))[0].numpy()
    return verts.astype(F32), c['faces']


def test_the_table_is_the_package_s():
    from tuch_amd import ops
    for name in MESHES:
        verts, faces = cc.mesh(name)
        off, ids = ops.vertex_face_table(faces, verts.shape[1])
        o2, i2 = oc.vertex_table(faces, verts.shape[1])
        assert np.array_equal(off, o2) and np.array_equal(ids, i2), name


@pytest.mark.parametrize('name', MESHES + ('ico6',))
def test_float32_vertex_normals_are_the_float64_ones(name):
    if name == 'ico6':
        verts, faces = _posed_body()
    else:
        verts, faces = cc.mesh(name)
    off, ids = oc.vertex_table(faces, verts.shape[1])
    for v in verts:
        u32 = oc.vertex_normals32(v, faces, off, ids)
        u64 = oc.vertex_normals64(v, faces, off, ids)
        # every face normal carries at most 5 u of its corners' products; the sum of k <= 12 of them k more roundings
        scale = np.abs(np.cross(*(v.astype(np.float64)[faces][:, k] - v.astype(np.float64)[faces][:, 0] for k in (1, 2)))).max()
        assert np.abs(u32 - u64).max() <= 64 * cc.EPS32 * max(scale, np.abs(v).max() ** 2)
        long = np.linalg.norm(u64, axis=1) > 1e-3 * np.linalg.norm(u64, axis=1).max()
        cosine = (u32[long].astype(np.float64) * u64[long]).sum(1) / (
            np.linalg.norm(u32[long].astype(np.float64), axis=1) * np.linalg.norm(u64[long], axis=1))
        assert np.degrees(np.arccos(np.clip(cosine, -1, 1))).max() < 0.05
        unit = oc.vertex_normals32(v, faces, off, ids, normalize=True)
        length = np.linalg.norm(unit.astype(np.float64), axis=1)
        zero = oc.sq32(u32) == 0
        assert np.all(unit[zero] == 0) and np.all(np.abs(length[~zero] - 1) < 4 * cc.EPS32)
    if name == 'degenerate':
        assert zero.any()                      # the vertices of the faces without area


@pytest.mark.parametrize('angle', oc.ANGLES)
def test_the_float32_rule_is_the_float64_rule_away_from_the_threshold(angle):
    rng = np.random.default_rng(int(angle))
    u = rng.standard_normal((300, 3)) * 10.0 ** rng.uniform(-4, 2, (300, 1))
    n = rng.standard_normal((400, 3)) * 10.0 ** rng.uniform(-4, 2, (400, 1))
    u32, n32 = u.astype(F32), n.astype(F32)
    assert (oc.sq32(u32)[:, None] * oc.sq32(n32)[None]).min() >= 1e-30
    c = oc.cos32(angle)
    got = oc.pair_rule32(u32, n32, c)
    cos = oc.pair_cos64(u32, n32)
    clear = np.abs(cos - float(c)) > 2.0 ** -20 * max(float(c), 2.0 ** -4)
    assert np.array_equal(got[clear], (cos >= float(c))[clear] & (cos > 0)[clear])
    assert clear.mean() > 0.999
    # a missing normal on either side: unconstrained
    n32[::7] = 0
    u32[::5] = np.nan
    got = oc.pair_rule32(u32, n32, c)
    assert got[::5].all() and got[:, ::7].all()
    assert np.array_equal(oc.pair_rule32(u32[:300], n32[:300], c, diagonal=True), np.diag(got[:300, :300]))


def test_threshold_pairs_fall_on_both_sides():
    for angle in oc.ANGLES:
        t = oc.threshold_case(angle)
        own = np.repeat(np.arange(64), 4)
        adm = oc.pair_rule32(t['query_normals'][0], t['normals'][0][own], oc.cos32(angle), diagonal=True).reshape(64, 4)
        assert adm[:, 2].all()                                  # 1 degree inside
        assert not adm[:, 3].any()                              # 1 degree outside
        assert (oc.sq32(t['query_normals'][0]) * oc.sq32(t['normals'][0][own])).min() >= 1e-30


def test_brute_force_without_normals_is_the_unoriented_sweep():
    c = oc.cloud_case('icosphere', 2, 257, 65)
    zero = np.zeros_like(c['normals'])
    got = oc.brute_force_batch(c['queries'], c['query_normals'], c['points'], zero, oc.cos32(30.0), shift=c['shift'])
    want = cf.brute_force_batch(c['queries'], c['points'], shift=c['shift'])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    away = oc.brute_force_batch(c['queries'], c['query_normals'], c['points'], c['normals'], oc.cos32(60.0), shift=c['shift'])
    assert (away[1] != want[1]).any() and (away[0] >= want[0]).all()
    # the case of the device's one-path test (tests/test_gpu_oriented_cloud.py): an unconstrained oriented call, by zero
    # query normals or by zero point normals, is the plain call in the reference alone
    c = oc.cloud_case('body122', 2, 257, 257, ('true',))
    counts = np.array([257, 130], np.int32)
    for tau in (None, 0.03):
        want = cf.brute_force_batch(c['queries'], c['points'], counts, shift=c['shift'], tau=tau)
        for qn, pn in ((np.zeros_like(c['query_normals']), c['normals']), (c['query_normals'], np.zeros_like(c['normals']))):
            got = oc.brute_force_batch(c['queries'], qn, c['points'], pn, oc.cos32(60.0), counts, shift=c['shift'], tau=tau)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
        assert (want[1] >= 0).any() and ((want[1] < 0).any() if tau else (want[1] >= 0).all())


def test_what_it_is_for_on_the_cpu():
    """The front-only scan: the plain two-sided fit drags the body towards the sensor, the oriented one does not."""
    r = oc.feature_loops()
    print('mean vertex-to-true distance after %d iterations: %s' % (oc.FEATURE_ITERS, r))
    assert r['two_sided'] >= 1.5 * r['oriented']
    assert r['oriented'] < 2.5 * r['one_sided']
    assert 0.5 < r['matched'] < 1.0


def test_the_float32_loop_holds_the_trajectory_floor():
    holds, bound = oc.trajectory_bound()
    assert oc.TRAJECTORY_PREFIX >= 10 and holds, bound
