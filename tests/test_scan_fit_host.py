"""CPU: the float64 statements of the scan-fit data term (tests/scan_fit_cases.py) -- each rho and its fixed-face
gradients against central differences of the full statement --, the C ABI of the new entry points as far as it goes
without a device, and the face -> group table of a model whose tables stay in host memory."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import closest_point_cases as cc
import scan_fit_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('rho', sc.RHOS)
def test_statement_gradients_against_central_differences(rho):
    c = sc.grad_case('icosphere', rho)
    sc.assert_interior_with_margin(c['points'], c['transl'], c['verts'], c['faces'])
    per, total, gv, gt, gp = sc.term_statement(c['points'], c['verts'], c['faces'], c['transl'], None, c['weights'], rho,
                                               c['sigma'])
    assert np.isfinite(total) and per.shape == (2,) and abs(per.sum() - total) <= 1e-12 * abs(total)
    for name, got, want in (('points', gp, c['gp']), ('transl', gt, c['gt']), ('verts', gv, c['gv'])):
        ok, ratio = sc.grad_within(got, want)
        assert ok, (rho, name, ratio)
        assert np.abs(want).max() > 0
    # the translation moves every query the other way
    np.testing.assert_allclose(gt, -gp.sum(1), rtol=1e-9, atol=1e-12)


def test_rho_values_and_the_gradient_at_zero():
    d2 = np.array([0.0, 0.25, 4.0])
    assert np.array_equal(sc.rho_numpy(d2, 'squared', None), d2)
    assert np.array_equal(sc.rho_numpy(d2, 'distance', None), [0.0, 0.5, 2.0])
    np.testing.assert_allclose(sc.rho_numpy(d2, 'gmof', 0.5), [0.0, 0.125, 0.25 * 4.0 / 4.25], rtol=1e-15)
    for rho in sc.RHOS:
        x = torch.tensor(d2, requires_grad=True)
        y = sc.rho_torch(x, rho, 0.5)
        np.testing.assert_allclose(y.detach().numpy(), sc.rho_numpy(d2, rho, 0.5), rtol=1e-15)
        y.sum().backward()
        assert torch.isfinite(x.grad).all()
    x = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    sc.rho_torch(x, 'distance', None).sum().backward()
    assert x.grad.item() == 0.0                                     # vertex_fit's convention


def test_torch_statement_equals_the_numpy_statement():
    c = cc.case('icosphere', 1, 65)
    p, v, faces = c['points'][0].astype(np.float64), c['verts'][0].astype(np.float64), c['faces']
    d2, face = cc.statement(p, v, faces)
    tri = torch.tensor(v[faces[face]])
    got = sc.tri_d2_torch(torch.tensor(p), tri[:, 0], tri[:, 1], tri[:, 2]).numpy()
    np.testing.assert_allclose(got, d2, rtol=1e-12, atol=1e-18)


def test_empty_bodies_and_zero_weights_in_the_statement():
    c = sc.term_case('icosphere', 3, 65, 'distance', weighted=True)
    counts = np.array([65, 0, 20], np.int32)
    weights = c['weights'].copy()
    weights[2] = 0.0
    points = c['points'].copy()
    points[0, c['weights'][0] == 0] = np.nan                        # never computed from
    per, total, gv, gt, gp = sc.term_statement(points, c['verts'], c['faces'], c['transl'], counts, weights, 'distance', None)
    assert per[1] == 0.0 and per[2] == 0.0 and per[0] > 0 and total == per[0]
    for g in (gv, gt, gp):
        assert np.all(np.isfinite(g)) and not g[1].any() and not g[2].any()


def test_hint_kinds():
    c = cc.case('strip', 3, 65)
    answer = c['ref']['face']
    num_faces = len(c['faces'])
    wrong = sc.hints('wrong', c['points'], c['verts'], c['faces'], answer)
    assert wrong.dtype == np.int32 and np.all(wrong != answer) and np.all((wrong >= 0) & (wrong < num_faces))
    mix = sc.hints('mix', c['points'], c['verts'], c['faces'], answer)
    for value in (-1, num_faces, sc.INT32_MAX, sc.INT32_MIN):
        assert (mix[0, :64] == value).any()                         # within one wavefront
    assert np.array_equal(sc.hints('answer', c['points'], c['verts'], c['faces'], answer), answer)
    one = cc.case('triangle', 1, 5)
    assert np.all(sc.hints('wrong', one['points'], one['verts'], one['faces'], one['ref']['face']) == 0)


def test_abi_symbols_and_argument_checks():
    from tuch_amd import _C
    L = _C.lib()
    header = open(os.path.join(ROOT, 'include', 'tuch_amd.h')).read()
    for name in ('tuch_closest_point', 'tuch_contact_model_face_groups', 'tuch_scan_fit_workspace_bytes',
                 'tuch_scan_fit_terms'):
        assert name in _C.exported_symbols() and hasattr(L, name) and name + '(' in header
    assert L.tuch_abi_version() == 3
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(64)      # not NULL, never read: the model is NULL, which every call reports first
    # the one function reports under its own name for the plain, the hinted and the oriented argument set
    for normals, cos, hint in ((null, 0.0, null), (null, 0.0, some), (some, 0.5, some)):
        assert L.tuch_closest_point(null, null, null, normals, cos, null, hint, 1, 1, null, null, null, null, 0, null) != 0
        assert b'tuch_closest_point: null pointer' in L.tuch_last_error()
        assert L.tuch_scan_fit_terms(null, null, null, null, normals, cos, null, null, hint, 1, 1, 1, 0.0, *([null] * 10), 0,
                                     null) != 0
        assert b'tuch_scan_fit_terms: null pointer' in L.tuch_last_error()
    assert L.tuch_contact_model_face_groups(null, None, null, null, null) != 0
    assert b'tuch_contact_model_face_groups: null model' in L.tuch_last_error()
    for oriented in (0, 1):
        assert L.tuch_scan_fit_workspace_bytes(null, 4, 5, oriented) == 0         # no model: nothing to size
        assert L.tuch_scan_fit_workspace_bytes(null, 0, 5, oriented) == 0


_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + '/tests')
import closest_point_cases as cc
from tuch_amd.ops import ContactModel
for name in ('triangle', 'strip', 'icosphere', 'body122'):
    faces = cc.mesh(name)[1]
    off, lst, grp = ContactModel(faces, device='cpu').face_groups()
    F, G = len(faces), len(off) - 1
    assert off[0] == 0 and off[-1] == F and np.all(np.diff(off) >= 1) and np.all(np.diff(off) <= 64), name
    assert np.array_equal(np.sort(lst), np.arange(F)), name
    assert grp.min() == 0 and grp.max() == G - 1, name
    for g in range(G):
        assert np.all(grp[lst[off[g]:off[g + 1]]] == g), (name, g)
    # the inverse: face f is in the run of its group
    pos = np.empty(F, np.int64)
    pos[lst] = np.arange(F)
    assert np.all((off[grp] <= pos) & (pos < off[grp + 1])), name
print('face groups ok')
'''


def test_face_group_table_is_the_inverse_of_the_face_list():
    """A model built with its tables in host memory (TUCH_HOST_TABLES=1, read when the library is loaded: a process of its
    own): face_group[f] = g exactly for the faces of face_list[group_off[g] .. group_off[g + 1])."""
    env = dict(os.environ, TUCH_HOST_TABLES='1')
    out = subprocess.run([sys.executable, '-c', _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'face groups ok' in out.stdout, out.stdout + out.stderr
