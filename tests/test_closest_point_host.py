"""CPU: the float64 statement of the closest-point query (tests/closest_point_cases.py) against sampled surface points and
hand-made cases, and the C ABI of tuch_closest_point as far as it goes without a device."""
import ctypes

import numpy as np
import pytest

import closest_point_cases as cc

A, B, C = (np.array(x, np.float64) for x in ([0, 0, 0], [1, 0, 0], [0, 1, 0]))


def test_statement_against_sampled_surface_points():
    rng = np.random.default_rng(5)
    n = 60                                              # 1891 sampled points per triangle
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    keep = i + j <= n
    w = np.stack([i[keep], j[keep], n - i[keep] - j[keep]], 1) / n
    assert len(w) > 1800
    worst = 0.0
    for _ in range(200):
        tri = rng.standard_normal((3, 3)) * rng.choice([0.05, 1.0, 3.0])
        p = rng.standard_normal(3) * rng.choice([0.1, 1.0, 10.0])
        d = np.sqrt(cc.tri_d2(p, tri[0], tri[1], tri[2]))
        samples = np.linalg.norm(w @ tri - p, axis=1)
        pitch = max(np.linalg.norm(tri[k] - tri[(k + 1) % 3]) for k in range(3)) / n
        assert d <= samples.min() + 1e-12               # no sampled point is nearer than the statement's distance
        assert samples.min() - d <= pitch               # and the nearest one is within the sampling pitch of it
        worst = max(worst, (samples.min() - d) / pitch)
    assert worst > 0.0                                  # (the samples are not the answer themselves)


@pytest.mark.parametrize('p, d2', [
    ([-1, -1, 1], 3.0),             # corner a
    ([2, -0.5, 0], 1.25),           # corner b
    ([-0.5, 2, 0], 1.25),           # corner c
    ([0.5, -1, 2], 5.0),            # edge ab
    ([-1, 0.5, 2], 5.0),            # edge ca
    ([1, 1, 1], 1.5),               # edge bc
    ([0.25, 0.25, 3], 9.0),         # interior
    ([1, 0, 0], 0.0),               # on a corner
    ([0.5, 0.5, 0], 0.0),           # on an edge
    ([0.25, 0.25, 0], 0.0),         # in the interior
])
def test_statement_exact_values(p, d2):
    assert cc.tri_d2(np.array(p, np.float64), A, B, C) == d2
    assert cc.tri_d2(np.array(p, np.float32), *(x.astype(np.float32) for x in (A, B, C))) == np.float32(d2)
    # the same for every naming of the corners
    for a, b, c in ((B, C, A), (C, A, B), (A, C, B)):
        assert cc.tri_d2(np.array(p, np.float64), a, b, c) == d2


def test_statement_degenerate_triangles_are_their_edges():
    p = np.array([0.5, 2.0, 0.0])
    assert cc.tri_d2(p, A, B, B) == 4.0                             # two equal corners: the segment ab
    assert cc.tri_d2(p, A, 0.25 * B, B) == 4.0                      # collinear corners: the segment ab
    assert cc.tri_d2(p, B, B, B) == 4.25                            # a point
    d2, face = cc.statement(np.array([[0.25, 0.25, 3.0], [5.0, 0.0, 0.0]]), np.stack([A, B, C]), np.array([[0, 1, 1], [0, 1, 2]]))
    assert np.array_equal(d2, [9.0, 16.0]) and np.array_equal(face, [1, 0])       # ties go to the first face


def test_bound_is_the_restatements_error_with_a_floor():
    c = cc.case('icosphere', 1, 65)
    p, v = c['points'][0], c['verts'][0]
    d64, _ = cc.statement(p, v, c['faces'])
    d32, _ = cc.statement(p, v, c['faces'], np.float32)
    assert d32.dtype == np.float32 and d64.dtype == np.float64
    near = np.abs(p).max(1) < 100
    assert (~near).sum() == 1
    err = np.abs(d32[near] - d64[near]).max()
    assert 0 < err < 1e-5                                           # float32 noise at unit scale, not an error of the statement
    b = c['ref']['bound'][0]
    assert np.all(b[near] >= 4 * err) and np.all(b >= cc.FLOOR_ULPS * cc.EPS32 * np.abs(v).max() ** 2)
    assert b[near].max() < 1e-4 and np.array_equal(c['ref']['d2'][0], d64)


def test_abi_symbols_and_argument_checks():
    from tuch_amd import _C
    L = _C.lib()
    for name in ('tuch_closest_point_workspace_bytes', 'tuch_closest_point', 'tuch_closest_point_bwd'):
        assert name in _C.exported_symbols() and hasattr(L, name)
    assert L.tuch_abi_version() == 3
    null = ctypes.c_void_p(0)
    assert L.tuch_closest_point(null, null, null, null, 0.0, null, null, 1, 1, null, null, null, null, 0, null) != 0
    assert b'tuch_closest_point: null pointer' in L.tuch_last_error()
    assert L.tuch_closest_point_bwd(null, null, null, null, null, null, 1, 1, null, null, null, null) != 0
    assert b'tuch_closest_point_bwd: null pointer' in L.tuch_last_error()
    for oriented in (0, 1):
        assert L.tuch_closest_point_workspace_bytes(null, 0, 5, oriented) == 0
        assert L.tuch_closest_point_workspace_bytes(null, 4, 5, oriented) == 0    # no model: nothing to size

