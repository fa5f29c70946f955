"""CPU: the statements of tests/point_normal_cases.py against float64, the argument errors of PointCloud.knn / .normals /
ScanFitter(estimate_normals=) that are raised before any device is touched, and the ABI names."""
import ctypes

import numpy as np
import pytest
import torch

import cloud_fit_cases as cf
import point_normal_cases as pn

F32 = np.float32


def test_knn_brute_force_is_the_sorted_sweep():
    c = cf.cloud_case('body122', 2, 257, 65)
    for b in range(2):
        d2, index = pn.knn_brute_force(c['queries'][b], c['points'][b], 8, shift=c['shift'][b])
        one = cf.brute_force(c['queries'][b], c['points'][b], shift=c['shift'][b])
        assert np.array_equal(d2[:, 0], one[0]) and np.array_equal(index[:, 0], one[1])          # k = 1 is the nearest
        assert np.all(np.diff(d2.astype(np.float64), axis=1) >= 0)
        q = pn.shifted(c['queries'][b], c['shift'][b]).astype(np.float64)
        e = ((q[:, None] - c['points'][b].astype(np.float64)[None]) ** 2).sum(-1)
        want = np.sort(e, 1)[:, :8]
        np.testing.assert_allclose(d2, want, rtol=1e-5)
        rows = np.arange(65)[:, None]
        np.testing.assert_allclose(e[rows, index], want, rtol=1e-5)
    # ties: the smaller index first; fewer valid points than k: the tail
    same = np.tile(np.array([0.25, -0.5, 1.5], F32), (5, 1))
    d2, index = pn.knn_brute_force(np.zeros((2, 3), F32), same, 8)
    assert np.array_equal(index[:, :5], np.tile(np.arange(5), (2, 1))) and np.all(index[:, 5:] == -1)
    assert np.all(np.isposinf(d2[:, 5:])) and np.all(d2[:, :5] == d2[0, 0])
    # tau, weights, counts, a non-finite query, query_count
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [np.nan, 0, 0]], F32)
    w = np.array([1, 0, 1, 1, 1], F32)
    qs = np.array([[0.1, 0, 0], [np.inf, 0, 0], [0.1, 0, 0]], F32)
    d2, index = pn.knn_brute_force(qs, pts, 3, count=5, weights=w, tau=2.5, query_count=2)
    assert index.tolist() == [[0, 2, -1], [-1, -1, -1], [-1, -1, -1]]


def test_cov_f32_against_float64_and_the_bound_is_not_vacuous():
    """The float32 sequence's scatter matrix against float64 on the noisy clouds the device tests use, every query of
    them, k in {8, 16, 32}.  Each error is within the derived (n + 4.01) u T.  Asserted as the figures the feature was
    specified with: covariance error <= 2.6 u trace, gap (lambda1 - lambda0) / trace >= 2.4e-3; and the angle bound
    2 E / gap <= 0.02, far from vacuous.  Observed: 2.12 u trace, 5.9e-3, 0.0139."""
    worst_err, least_gap, worst_bound = 0.0, np.inf, 0.0
    for num_points in (257, 4099):
        c = cf.cloud_case('body122', 1, num_points, 257)
        q = pn.shifted(c['queries'][0], c['shift'][0])
        _, index = pn.knn_brute_force(c['queries'][0], c['points'][0], 32, shift=c['shift'][0])
        for k in (8, 16, 32):
            for i in range(257):
                s = c['points'][0][index[i, :k]]
                got, _ = pn.cov_f32(q[i], s)
                ref = pn.pca_f64(q[i], s)
                err = np.linalg.norm(pn.full(got) - ref['cov'])
                assert err <= (k + 4.01) * pn.U * ref['total']
                worst_err = max(worst_err, err / (pn.U * ref['trace']))
                gap = ref['lam'][1] - ref['lam'][0]
                least_gap = min(least_gap, gap / ref['trace'])
                worst_bound = max(worst_bound, 2 * pn.error_bound(k, ref['total']) / gap)
    print('cov_f32 error / (u trace)', worst_err, 'least gap / trace', least_gap, 'largest 2E / gap', worst_bound)
    assert worst_err <= 2.6 and least_gap >= 2.4e-3 and worst_bound <= 0.02


def test_cov_f32_edges():
    cov, m = pn.cov_f32(np.zeros(3, F32), np.zeros((0, 3), F32))
    assert not cov.any() and not m.any()
    same = np.tile(np.array([0.25, -0.5, 1.5], F32), (7, 1))
    cov, m = pn.cov_f32(np.array([1, 2, 3], F32), same)
    assert not cov.any() and np.array_equal(m, (same[0] - np.array([1, 2, 3], F32)).astype(F32))
    line = np.zeros((9, 3), F32)
    line[:, 0] = np.arange(9)
    ref = pn.pca_f64(np.zeros(3), line)
    assert ref['lam'][1] - ref['lam'][0] <= 2 * pn.error_bound(9, ref['total'])     # collinear: the bound says nothing
    assert pn.canonical([0.1, -0.2, 0.9]) and not pn.canonical([0.1, -0.9, 0.2]) and pn.canonical([0.5, -0.5, 0.5])
    assert abs(pn.angle([0, 0, 1], [0, 1e-9, -1]) - 1e-9) < 1e-15


class _Cloud:
    """A PointCloud that never saw a device: what the argument checks read."""

    def __new__(cls, batch=2, num_points=5):
        from tuch_amd.ops import PointCloud
        cloud = object.__new__(PointCloud)
        cloud.batch, cloud.num_points, cloud.resolution = batch, num_points, 64
        cloud.points = torch.zeros(batch, num_points, 3)
        cloud.counts = cloud.weights = None
        return cloud


def test_argument_errors_before_any_device():
    cloud = _Cloud()
    q = torch.zeros(2, 7, 3)
    for k in (0, 33, -1, 2.0, None, True):
        with pytest.raises(ValueError, match='k must be'):
            cloud.knn(q, k=k)
        with pytest.raises(ValueError, match='k must be'):
            cloud.normals(q, k=k)
    with pytest.raises(ValueError, match='queries'):
        cloud.knn(q[:1], k=3)
    with pytest.raises(ValueError, match='queries'):
        cloud.normals(q[:, :, :2], k=3)
    with pytest.raises(ValueError, match='shift'):
        cloud.knn(q, k=3, shift=torch.zeros(3, 3))
    with pytest.raises(ValueError, match='viewpoint'):
        cloud.normals(q, k=3, viewpoint=torch.zeros(2, 6, 3))
    with pytest.raises(ValueError, match='viewpoint'):
        cloud.normals(None, k=3, viewpoint=torch.zeros(2, 7, 3))                # own points: N is 5
    with pytest.raises(RuntimeError, match='HIP device'):                       # no host fallback
        cloud.knn(q, k=3)
    with pytest.raises(RuntimeError, match='HIP device'):
        cloud.normals(None, k=3, viewpoint=torch.zeros(2, 3))


class _Smpl:
    v_template = torch.zeros(10, 3)


def test_scan_fitter_argument_errors_before_any_device():
    from tuch_amd.fit import ScanFitter
    with pytest.raises(ValueError, match='max_normal_angle'):
        ScanFitter(_Smpl(), None, estimate_normals=16)
    for k in (0, 33, 1.5):
        with pytest.raises(ValueError, match='estimate_normals'):
            ScanFitter(_Smpl(), None, max_normal_angle=60.0, estimate_normals=k)
    fitter = ScanFitter(_Smpl(), None, max_normal_angle=60.0, estimate_normals=16)
    points, go = torch.zeros(2, 5, 3), torch.zeros(2, 3)
    with pytest.raises(ValueError, match='normals were passed'):
        fitter(points, go, normals=torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match='viewpoint'):
        fitter(points, go, viewpoint=torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match='viewpoint needs estimate_normals'):
        ScanFitter(_Smpl(), None, max_normal_angle=60.0)(points, go, viewpoint=torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match='HIP device'):
        fitter(points, go, viewpoint=torch.zeros(2, 3))


def test_abi_names_and_k_range():
    from tuch_amd import _C
    assert {'tuch_point_cloud_knn', 'tuch_point_cloud_normals'} <= set(_C.exported_symbols())
    L = _C.lib()
    one = ctypes.c_void_p(16)                                                   # never dereferenced: k is checked first
    for k in (0, 33):
        assert L.tuch_point_cloud_knn(one, 0, one, None, None, one, None, None, 0.0, 1, 1, 1, k, one, one, None) != 0
        assert b'k = %d' % k in L.tuch_last_error()
        assert L.tuch_point_cloud_normals(one, 0, one, None, None, one, None, None, 0.0, 1, 1, 1, k, None, 0, one, one, one, None,
                                          None) != 0
        assert b'k = %d' % k in L.tuch_last_error()
    assert L.tuch_point_cloud_normals(one, 0, one, None, None, one, None, None, 0.0, 1, 1, 1, 8, None, 1, one, one, one, None,
                                      None) != 0
    assert b'viewpoint' in L.tuch_last_error()
