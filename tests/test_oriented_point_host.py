"""CPU: the admissibility rule of the normal-compatible closest point as tests/oriented_point_cases.py restates it in
float32 -- against the float64 angle away from the threshold, for missing normals and faces without area --, and the
argument checks of the new C entry points and Python wrappers as far as they go without a device."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import closest_point_cases as cc
import oriented_point_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = ('triangle', 'strip', 'tetrahedron', 'icosphere', 'degenerate', 'body122')


@pytest.mark.parametrize('angle', oc.ANGLES)
def test_float32_rule_equals_the_float64_angle_away_from_the_threshold(angle):
    """Wherever |cos(m, n) - cos(max_angle)| > 1e-4 the float32 decision is the float64 one; the pairs within 1e-4 are
    under 1 % of all pairs (a property of these inputs: random unit normals, seed 5)."""
    rng = np.random.default_rng(5)
    c = oc.cos32(angle)
    total = near = 0
    for name in MESHES:
        verts, faces = cc.mesh(name)
        n = rng.standard_normal((200, 3))
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        got = oc.rule32(verts[0], faces, n, c)
        cos = oc.cos64(verts[0], faces, n)
        has_area = np.isfinite(cos)
        # (a face without area is inadmissible: checked on its own below)
        assert not got[~has_area].any()
        clear = has_area & (np.abs(cos - float(c)) > 1e-4)
        assert np.array_equal(got[clear], (cos > float(c))[clear]), name
        total += int(has_area.sum())
        near += int((has_area & ~clear).sum())
    assert near < 0.01 * total, (near, total)


def test_zero_nan_and_inf_normals_are_unconstrained():
    verts, faces = cc.mesh('degenerate')
    n = np.array([[0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0], [-np.inf, 1, 1], [3e19, 3e19, 0], [0, 0, 1e-30], [0, 0, 1]],
                 np.float32)
    free = oc.unconstrained32(n)
    # zero, NaN, Inf, a length whose square overflows, one whose square underflows to 0; the last one is a normal
    assert free.tolist() == [True, True, True, True, True, True, False]
    adm = oc.rule32(verts[0], faces, n, oc.cos32(60))
    assert adm[:6].all() and not adm[6].all()


def test_a_face_without_area_is_never_admissible_for_a_constrained_query():
    verts, faces = cc.mesh('degenerate')
    m, mm = oc.face_normals32(verts[0], faces)
    flat = np.nonzero(mm == 0)[0]
    assert len(flat) == 3                                           # collinear, (a, a, c), a point
    rng = np.random.default_rng(1)
    n = rng.standard_normal((50, 3)).astype(np.float32)
    for angle in oc.ANGLES:
        assert not oc.rule32(verts[0], faces, n, oc.cos32(angle))[:, flat].any()
    nan_verts = verts[0].copy()
    nan_verts[faces[5]] = np.nan                                    # NaN corners: every comparison is false
    assert not oc.rule32(nan_verts, faces, n, oc.cos32(90))[:, 5].any()


def test_reference_reduces_to_the_plain_statement_for_zero_normals_and_is_empty_for_flipped_ones():
    c = oc.case('icosphere', 1, 65, 60.0)
    zero = np.zeros_like(c['normals'])
    ref = oc.reference(c['points'], zero, c['verts'], c['faces'], 60.0)
    assert np.array_equal(ref['d2'], c['plain']['d2']) and np.array_equal(ref['face'], c['plain']['face'])
    # the cases hold both matched and unmatched queries, and the filter changes answers
    kinds = np.arange(65) % 4
    assert np.array_equal(c['ref']['face'][0][kinds == 3], c['plain']['face'][0][kinds == 3])
    assert (c['ref']['face'][0][kinds == 1] != c['plain']['face'][0][kinds == 1]).any()
    one = oc.case('triangle', 1, 65, 60.0)
    assert (one['ref']['face'] == -1).any() and (one['ref']['face'] == 0).any()
    assert np.all(np.isposinf(one['ref']['d2'][one['ref']['face'] == -1]))


def test_threshold_queries_straddle_the_rule():
    verts, faces = cc.mesh('icosphere')
    for angle in oc.ANGLES:
        p, n, f = oc.threshold_queries(verts[0], faces, angle)
        assert len(p) == 256
        adm = oc.rule32(verts[0], faces, n, oc.cos32(angle), pairs=(np.arange(len(f)), f))
        assert adm[2::4].all() and not adm[3::4].any()              # a degree inside, a degree outside
        d2, near = cc.statement(p, verts[0], faces)
        assert np.array_equal(near, f) and np.all(np.abs(np.sqrt(d2) - 1e-4) < 1e-6)


def test_abi_symbols_and_argument_checks():
    from tuch_amd import _C
    L = _C.lib()
    header = open(os.path.join(ROOT, 'include', 'tuch_amd.h')).read()
    for name in ('tuch_closest_point', 'tuch_closest_point_workspace_bytes', 'tuch_scan_fit_terms',
                 'tuch_scan_fit_workspace_bytes'):
        assert name in _C.exported_symbols() and hasattr(L, name) and name + '(' in header
    assert L.tuch_abi_version() == 3
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(64)      # normals that are not NULL and never read: the model is NULL

    def closest_point(normals, cos):
        return L.tuch_closest_point(null, null, null, normals, cos, null, null, 1, 1, null, null, null, null, 0, null)

    def scan_fit_terms(normals, cos):
        return L.tuch_scan_fit_terms(*([null] * 4), normals, cos, *([null] * 3), 1, 1, 1, 0.0, *([null] * 10), 0, null)

    assert closest_point(some, 0.5) != 0
    assert b'tuch_closest_point: null pointer' in L.tuch_last_error()
    assert scan_fit_terms(some, 0.5) != 0
    assert b'tuch_scan_fit_terms: null pointer' in L.tuch_last_error()
    for bad in (1.0, 1.5, -0.1, float('nan'), float('inf')):
        assert closest_point(some, bad) != 0
        assert b'tuch_closest_point: max_angle_cos' in L.tuch_last_error(), bad
        assert scan_fit_terms(some, bad) != 0
        assert b'tuch_scan_fit_terms: max_angle_cos' in L.tuch_last_error(), bad
    # without normals the cosine is not read: garbage in it is no error of its own
    for garbage in (float('nan'), 2.0):
        assert closest_point(null, garbage) != 0
        assert b'tuch_closest_point: null pointer' in L.tuch_last_error(), garbage
        assert scan_fit_terms(null, garbage) != 0
        assert b'tuch_scan_fit_terms: null pointer' in L.tuch_last_error(), garbage
    assert L.tuch_closest_point_workspace_bytes(null, 4, 5, 1) == 0      # no model: nothing to size
    assert L.tuch_scan_fit_workspace_bytes(null, 4, 5, 1) == 0


def test_wrapper_argument_checks():
    from tuch_amd import ops
    from tuch_amd.fit import ScanFitter
    verts, points, normals = torch.zeros(2, 12, 3), torch.zeros(2, 7, 3), torch.ones(2, 7, 3)
    fake = types.SimpleNamespace(num_verts=12)
    for call in (lambda **kw: ops.ContactModel.closest_point(fake, verts, points, **kw),
                 lambda **kw: ops.scan_fit(fake, verts, torch.zeros(2, 3), points, **kw)):
        with pytest.raises(ValueError, match='go together'):
            call(normals=normals)
        with pytest.raises(ValueError, match='go together'):
            call(max_angle=60.0)
        for bad in (0.0, -5.0, 90.5, 180.0, float('nan')):
            with pytest.raises(ValueError, match='max_angle'):
                call(normals=normals, max_angle=bad)
        with pytest.raises(ValueError, match='normals'):
            call(normals=normals[:, :6], max_angle=60.0)
        with pytest.raises(ValueError, match='normals'):
            call(normals=normals[:, :, :2], max_angle=60.0)
    assert ops.args.max_angle_cos(None, None, points, 'x') is None
    assert ops.args.max_angle_cos(normals, 60.0, points, 'x') == float(oc.cos32(60.0))
    assert 0.0 <= ops.args.max_angle_cos(normals, 90.0, points, 'x') < 1e-7
    assert ops.args.max_angle_cos(normals, 1e-3, points, 'x') < 1.0
    for bad in (0.0, 91.0, -1.0):
        with pytest.raises(ValueError, match='max_normal_angle'):
            ScanFitter(None, None, max_normal_angle=bad)
    smpl = types.SimpleNamespace(v_template=torch.zeros(12, 3))
    go = torch.zeros(2, 3)
    with pytest.raises(ValueError, match='max_normal_angle'):
        ScanFitter(smpl, fake)(points, go, normals=normals)
    with pytest.raises(ValueError, match='normals'):
        ScanFitter(smpl, fake, max_normal_angle=60.0)(points, go, normals=normals[:, :6])
