"""CPU: the statements of the point-cloud tests (tests/cloud_fit_cases.py) -- the brute-force rule on hand cases, float32
against float64, the float64 term's gradients against central differences --, the float32 yardstick of the two-sided fit,
and the C ABI of the new entry points as far as it goes without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cloud_fit_cases as cf
import scan_fit_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.mark.parametrize('rho', sc.RHOS)
def test_statement_gradients_against_central_differences(rho):
    c = cf.grad_case(rho)
    cf.assert_gap(c['verts'], c['transl'], c['points'])
    per, total, gv, gt = cf.term_statement(c['verts'], c['transl'], c['points'], None, None, c['vw'], rho, c['sigma'],
                                           None, c['scale'])
    assert np.isfinite(total) and per.shape == (2,) and abs(per.sum() - total) <= 1e-12 * abs(total)
    for name, got, want in (('verts', gv, c['gv']), ('transl', gt, c['gt'])):
        ok, ratio = sc.grad_within(got, want)
        assert ok, (rho, name, ratio)
        assert np.abs(want).max() > 0
    np.testing.assert_allclose(gt, gv.sum(1), rtol=1e-9, atol=1e-12)     # the translation moves every query the same way


def test_float32_and_float64_sweeps_agree_where_the_runner_up_is_clear():
    c = cf.cloud_case('icosphere', 3, 257, 257)
    for b in range(3):
        d2, index = cf.brute_force(c['queries'][b], c['points'][b], shift=c['shift'][b])
        q = (c['queries'][b] + c['shift'][b][None]).astype(F32)
        i64, d64, second = cf.nearest_f64(q, c['points'][b])
        # the float32 rounding of d2: 6 u relative (the source file's derivation), taken as 8 u on both candidates
        clear = second - d64 > 16 * cf.EPS32 * second
        assert clear.mean() > 0.9
        assert np.array_equal(index[clear], i64[clear])
        assert np.all(np.abs(d2.astype(np.float64) - d64)[clear] <= 8 * cf.EPS32 * d64[clear])


def test_hand_cases_of_the_rule():
    origin = np.zeros((1, 3), F32)
    two = np.array([[1, 0, 0], [-1, 0, 0]], F32)
    d2, index = cf.brute_force(origin, two)
    assert index[0] == 0 and d2[0] == 1.0                               # equal bits: the lower index
    d2, index = cf.brute_force(origin, two[::-1])
    assert index[0] == 0
    dup = np.array([[3, 0, 0], [0.5, 0.5, 0], [0.5, 0.5, 0], [0.5, 0.5, 0]], F32)
    d2, index = cf.brute_force(origin, dup)
    assert index[0] == 1 and d2[0] == 0.5
    # weights and counts drop points before the sweep; NaN / Inf points are never neighbours
    d2, index = cf.brute_force(origin, dup, weights=np.array([1, 0, 1, 1], F32))
    assert index[0] == 2
    d2, index = cf.brute_force(origin, dup, count=1)
    assert index[0] == 0 and d2[0] == 9.0
    bad = dup.copy()
    bad[1] = np.nan
    bad[2, 0] = np.inf
    assert cf.brute_force(origin, bad)[1][0] == 3
    # tau: a point at exactly tau is kept, one a float32 step beyond is dropped
    tau = F32(0.3)
    t2 = tau * tau
    x = np.sqrt(np.float64(t2)).astype(F32)
    for cand in (x, np.nextafter(x, F32(0)), np.nextafter(x, F32(1))):
        if F32(cand * cand) == t2:
            x = cand
    assert F32(x * x) == t2
    at = np.array([[x, 0, 0]], F32)
    d2, index = cf.brute_force(origin, at, tau=tau)
    assert index[0] == 0 and d2[0] == t2
    y = x
    while F32(y * y) <= t2:
        y = np.nextafter(y, F32(1))
    d2, index = cf.brute_force(origin, np.array([[y, 0, 0]], F32), tau=tau)
    assert index[0] == -1 and np.isposinf(d2[0])
    # no winner: empty cloud, non-finite query, beyond the real queries
    assert cf.brute_force(origin, dup, count=0)[1][0] == -1
    assert cf.brute_force(np.array([[np.nan, 0, 0]], F32), dup)[1][0] == -1
    assert cf.brute_force(np.zeros((2, 3), F32), dup, query_count=1)[1].tolist() == [1, -1]
    # the shift is one float32 add
    d2, index = cf.brute_force(np.array([[1e8, 0, 0]], F32), np.array([[1e8, 0, 0], [1e8 + 8, 0, 0]], F32),
                               shift=np.array([3, 0, 0], F32))
    assert index[0] == (0 if F32(F32(1e8) + F32(3)) == F32(1e8) else 1)


def test_term_statement_edge_rules():
    c = cf.term_case('icosphere', 'distance', 'BV', tau=True)
    verts = c['verts'].copy()
    verts[0, c['vw'][0] == 0] = np.nan                                  # weight 0: never computed from
    counts = np.array([257, 0, 130], np.int32)
    vw = c['vw'].copy()
    vw[2] = 0.0
    per, total, gv, gt = cf.term_statement(verts, c['transl'], c['points'], counts, None, vw, 'distance', None, c['tau'],
                                           c['scale'])
    assert per[0] > 0 and per[1] == 0.0 and per[2] == 0.0 and total == per[0]
    assert np.all(np.isfinite(gv)) and not gv[1].any() and not gv[2].any() and not gv[0][c['vw'][0] == 0].any()
    # a vertex without winner contributes rho(tau^2) and no gradient
    far = c['verts'].copy()
    far[0, 0] += 10.0
    per2, _, gv2, _ = cf.term_statement(far, c['transl'], c['points'], c['counts'], None, None, 'distance', None, c['tau'], 1.0)
    assert not gv2[0, 0].any() and per2[0] > 0


def test_float32_loop_holds_the_floor_on_the_committed_seed():
    """The yardstick of the fitter test: over all compared iterations the float32 CPU loop of the two-sided objective stays
    within sc.TRAJECTORY_FLOOR of the float64 loop."""
    holds, bound = cf.trajectory_bound('distance')
    assert holds and len(bound) == sc.FIT_PREFIX and np.all(bound >= sc.TRAJECTORY_FLOOR)
    ref = cf.fit_reference(sc.FIT_PREFIX)
    assert np.all(ref['loss'][:, :, 1] > 0)                             # the second direction is there


def test_the_feature_case_separates_the_two_fits_in_float64():
    """The case tests/test_gpu_cloud_fit.py runs on the product: committed because the float64 two-sided loop beats the
    one-sided one by at least a factor 1.5 (observed: 5.75 mm against 2.86 mm)."""
    c = cf.feature_case()
    assert c['one_sided'] >= 1.5 * c['two_sided'] > 0, (c['one_sided'], c['two_sided'])


def test_abi_symbols_and_argument_checks():
    from tuch_amd import _C
    L = _C.lib()
    header = open(os.path.join(ROOT, 'include', 'tuch_amd.h')).read()
    names = ('tuch_point_cloud_workspace_bytes', 'tuch_point_cloud_build', 'tuch_point_cloud_nearest',
             'tuch_point_cloud_fit_terms', 'tuch_point_cloud_fit_scratch_bytes', 'tuch_point_cloud_grid',
             'tuch_point_cloud_set_canary', 'tuch_point_cloud_canary_hits')
    for name in names:
        assert name in _C.exported_symbols() and hasattr(L, name) and name + '(' in header
    assert L.tuch_abi_version() == 3
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(256)     # a non-null pointer that is never followed
    assert L.tuch_point_cloud_build(null, null, null, 1, 1, 1, null, 0, null) != 0
    assert b'tuch_point_cloud_build: null pointer' in L.tuch_last_error()

    def nearest(normals, query_normals, cos):
        return L.tuch_point_cloud_nearest(null, 0, null, null, null, normals, null, query_normals, null, null, null, 0.0, cos,
                                          null, 0, 1, 1, 1, null, null, null)

    def fit_terms(normals, cos, mesh, faces):
        return L.tuch_point_cloud_fit_terms(null, 0, null, null, null, normals, cos, mesh, mesh, mesh, faces, null, 0, null,
                                            null, null, 0.0, 1, 1, 1, null, 0, 1, 0.0, 1.0, *([null] * 8), 0, null)

    # the one function reports under its own name with and without normals; without them the cosine is not read
    for normals, cos in ((null, 0.0), (null, float('nan')), (null, 2.0), (some, 0.5)):
        assert nearest(normals, normals, cos) != 0
        assert b'tuch_point_cloud_nearest: null pointer' in L.tuch_last_error(), cos
        assert fit_terms(normals, cos, normals, 1) != 0
        assert b'tuch_point_cloud_fit_terms: null pointer' in L.tuch_last_error(), cos
    # normals and query_normals go together
    for normals, query_normals in ((some, null), (null, some)):
        assert nearest(normals, query_normals, 0.5) == -1               # TUCH_ERR_ARG
        message = L.tuch_last_error()
        assert b'tuch_point_cloud_nearest: ' in message and b'normals' in message and b'query_normals' in message
    # with normals: the cosine, the mesh and its size are asked for
    for bad in (1.0, -0.1, float('nan')):
        assert nearest(some, some, bad) != 0
        assert b'tuch_point_cloud_nearest: max_angle_cos' in L.tuch_last_error(), bad
        assert fit_terms(some, bad, some, 1) != 0
        assert b'tuch_point_cloud_fit_terms: max_angle_cos' in L.tuch_last_error(), bad
    assert fit_terms(some, 0.5, null, 1) != 0
    assert b'tuch_point_cloud_fit_terms: null pointer' in L.tuch_last_error()
    assert fit_terms(some, 0.5, some, 0) != 0
    assert b'tuch_point_cloud_fit_terms: bad sizes' in L.tuch_last_error()
    assert L.tuch_point_cloud_grid(null, 1, 1, null, null, null) != 0
    assert b'tuch_point_cloud_grid: null pointer' in L.tuch_last_error()
    assert L.tuch_point_cloud_canary_hits(null, None, 0) != 0
    assert b'tuch_point_cloud_canary_hits: null pointer' in L.tuch_last_error()
    # bad sizes name the entry point too
    assert L.tuch_point_cloud_build(some, null, null, 0, 5, 4, some, 1 << 20, null) != 0
    assert b'tuch_point_cloud_build: bad sizes' in L.tuch_last_error()
    assert L.tuch_point_cloud_build(some, null, null, 1, 5, 4, some, 16, null) != 0
    assert b'tuch_point_cloud_build: workspace' in L.tuch_last_error()
    size = L.tuch_point_cloud_workspace_bytes
    for args in ((0, 5, 4), (5, 0, 4), (5, 5, 0), (-1, 5, 4), (5, -2, 4), (5, 5, -3)):
        assert size(*args) == 0
    assert L.tuch_point_cloud_fit_scratch_bytes(0, 5) == 0 and L.tuch_point_cloud_fit_scratch_bytes(2, 6890) > 0
    base = size(2, 100, 8)
    assert base > 0
    for more in ((3, 100, 8), (2, 1000, 8), (2, 100, 16), (64, 41328, 64)):
        assert size(*more) >= base
    seq = [size(b, q, r) for b, q, r in ((1, 1, 1), (1, 1, 2), (1, 2, 2), (2, 2, 2), (2, 2, 64), (2, 6890, 64), (64, 6890, 64))]
    assert seq == sorted(seq)
    # the guards only add bytes, and the option goes back
    was = L.tuch_point_cloud_set_canary(1)
    try:
        assert size(2, 100, 8) > base
    finally:
        L.tuch_point_cloud_set_canary(was)
    assert size(2, 100, 8) == base
