"""tests/hd_branch_cases.py without a GPU: (1) its float64 restatement of the HD branch agrees with the project's oracle
(oracle.contact.train_contact_body, itself checked against the reference's recorded results by test_oracle_golden.py) on
the golden HD regressor; (2) the synthetic fixture satisfies, by the restatement alone, every condition that
tests/test_gpu_hd_branch.py relies on."""
import numpy as np
import pytest

import hd_branch_cases as hc
from helpers import TANH_QUANTUM, assert_close, golden, golden_mask, oracle_segments, point_touches_surface
from oracle import contact as oc


# ------------------------------------------------------------------------------------------ (1) anchored to the oracle
@pytest.mark.parametrize('b', [0, 1, 2])
def test_restatement_matches_the_oracle_on_the_golden_hd_regressor(b):
    """Fed the oracle's own vertex-level results, `reference` selects the same HD points and gives the same inside /
    outside flags; its partner differs from the oracle's only between rows whose float64 squared distances tie within the
    noise of the oracle's float32 |x|^2 + |y|^2 - 2 x.y matrix (2e-6, helpers.hd_picks_vs_oracle); `evaluate` with the
    ORACLE's partners and flags gives its loss and gradient to the tolerances test_oracle_golden.py holds the oracle to
    against the reference (1e-5 on the loss; 1e-4 + 2e-6 of the largest entry + the tanh quantum on the gradient)."""
    g, gm = golden(hc.TAG), golden_mask(hc.TAG)
    euclthres = float(g['euclthres'])
    r = oc.train_contact_body(g['verts'][b], g['faces'], gm, euclthres, oracle_segments(g), True,
                              hd_idx=g['hd_idx'], hd_w=g['hd_w'], hd_face=g['hd_face'])
    ref = hc.reference(g['verts'][b], g['faces'], gm, g['hd_idx'], g['hd_w'], g['hd_face'],
                       (r['exterior_verts']).astype(np.uint8), r['min_d2'], 1, euclthres)
    assert ref['n'] > 300
    assert np.array_equal(ref['sel'], np.where(r['hd_sel'])[0])
    assert np.abs(ref['winding'] - hc.THRESH).min() > 1e-3
    assert np.array_equal(ref['exterior'], r['hd_exterior'])
    assert (~ref['exterior']).any() and ref['exterior'].any()
    assert (ref['admissible'] > 0).all()
    differ = np.where(ref['argmin'] != r['hd_argmin'])[0]
    assert len(differ) <= max(3, ref['n'] // 500)
    d2, ok = hc.pair_d2(ref, r['hd_argmin'][differ], differ)
    assert ok.all() and (np.abs(d2 - ref['min_d2'][differ]) < 2e-6).all()
    assert np.array_equal(hc.geomask_of(ref, np.arange(ref['n'])[:, None], np.arange(ref['n'])[None, :]), r['hd_mask'])
    terms, grad = hc.evaluate(ref, r['hd_argmin'], r['hd_exterior'], (1.0, 1.0), g['hd_idx'], g['hd_w'], g['verts'].shape[1])
    assert_close(terms[0], r['push'], 1e-5, 0, 'interior sum, body %d' % b)
    assert_close(terms[1], r['pull'], 1e-5, 0, 'exterior sum, body %d' % b)
    assert_close(terms.sum(), r['loss'], 1e-5, 0, 'loss, body %d' % b)
    assert_close(grad, r['grad'], 1e-4, 2e-6 * np.abs(r['grad']).max() + TANH_QUANTUM, 'gradient, body %d' % b)


def test_winding_numbers_of_a_tetrahedron():
    """The restated solid-angle sum: 1 inside a closed, outward-oriented surface, 0 outside."""
    v = np.array([[0., 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    tris = v[np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])]
    w = hc.winding_numbers(np.array([[0.1, 0.1, 0.1], [1.0, 1.0, 1.0], [-0.1, 0.2, 0.2]]), tris)
    np.testing.assert_allclose(w, [1.0, 0.0, 0.0], atol=1e-12)


# --------------------------------------------------------------------------------------------- (2) the fixture's conditions
def test_fans_and_layout():
    faces, gm, verts, _ = hc.mesh()
    fans = hc.fans()
    hd_face, fan, _ = hc.layout()
    n = hc.num_points()
    assert len(fans) == 10 and hc.PREFIX_COUNTS == (1, 32, 33, 64, 65, 1023, 1024, 1025, 2048, 2049)
    every = np.concatenate(fans)
    assert len(np.unique(every)) == len(every)                                    # pairwise disjoint in faces
    assert not (faces[every] == hc.EQUAL_VERTEX).any()
    for i, fs in enumerate(fans):
        assert (faces[fs] == hc.FAN_CENTRES[i]).any(1).all() and len(fs) == (faces == hc.FAN_CENTRES[i]).any(1).sum()
        assert (fan == i).sum() == hc.FAN_POINTS[i] and np.isin(hd_face[fan == i], fs).all()
    outside = np.setdiff1d(np.arange(len(faces)), every)
    assert np.array_equal(np.sort(hd_face[fan < 0]), outside)                     # exactly one point each
    assert n == 2049 + len(outside) and n % 32 != 0 and n > 2 * 2048
    first = [np.unique(faces[fs, 0]) for fs in fans]
    assert not gm[np.ix_(first[0], first[1])].any() and not gm[np.ix_(first[1], first[0])].any()
    for i in range(10):
        assert not gm[np.ix_(first[i], first[i])].any()                           # no partner inside a fan
        for j in range(i + 1, 10):
            if (i, j) != (0, 1):
                assert gm[np.ix_(first[i], first[j])].all() and gm[np.ix_(first[j], first[i])].all()
    assert not np.array_equal(hd_face, np.sort(hd_face))                          # a shuffle, the same for every K
    for K in hc.KS:
        idx, w, face = hc.regressor(K)
        assert idx.shape == (n, K) and w.shape == (n, K) and w.dtype == np.float32 and np.array_equal(face, hd_face)
        assert idx.min() >= 0 and idx.max() < verts.shape[1] and (w >= 0).all()
        np.testing.assert_allclose(w.sum(1), 1.0, atol=1e-6)                      # convex
        if K == 1:
            assert (faces[face] == idx).any(1).all()                              # a corner of its own face
        if K == 3:
            assert np.array_equal(idx, faces[face])
        if K == 8:
            assert np.array_equal(idx[:, :3], faces[face])
            nnz = (w != 0).sum(1)
            assert set(nnz.tolist()) == set(range(3, 9)) and (w[:, :3] > 0).all()
            pad = w == 0
            assert pad.any() and (np.cumsum(pad, 1)[~pad] == 0).all()             # zeros only behind the non-zeros


def test_inputs_flag_what_they_should():
    _, _, verts, euclthres = hc.mesh()
    exterior, min_d2, valid = hc.inputs()
    e2 = hc.eucl2(euclthres)
    assert e2.dtype == np.float32 and min_d2.dtype == np.float32 and exterior.dtype == np.uint8
    flagged = (min_d2 < e2) | (exterior == 0)
    centres = np.asarray(hc.FAN_CENTRES)
    for b in range(10):
        assert np.array_equal(np.where(flagged[b])[0], np.sort(centres[:b + 1]))
        if b >= 1:
            assert (exterior[b, centres[:b + 1]] == 0).any() and (min_d2[b, centres[:b + 1]] < e2).any()   # both ways
            assert np.nextafter(min_d2[b, centres[1]], np.float32(1)) == e2
    for b in range(11):
        equal = (min_d2[b] == e2) & (exterior[b] != 0)
        assert equal.any() and not (equal & flagged[b]).any()                     # equality does not select
    assert valid.tolist() == [1] * 11 + [0, 1]
    assert not flagged[hc.EMPTY_VALID].any() and flagged[hc.INVALID].all() and flagged[hc.EVERYTHING].all()
    assert (exterior[hc.EVERYTHING] == 0).any() and (exterior[hc.EVERYTHING] != 0).any()
    gt = hc.GRAD_TERMS
    assert gt.shape == (hc.BATCH, 2) and len(np.unique(gt)) > 4 and (gt[3] < 0).all() and gt[hc.NO_INTERIOR_GRAD, 0] == 0
    assert gt[hc.NO_INTERIOR_GRAD, 1] != 0


@pytest.mark.parametrize('K', hc.KS)
def test_reference_is_inside_the_conditions_of_the_gpu_test(K):
    faces, gm, verts, _ = hc.mesh()
    hd_idx, hd_w, hd_face = hc.regressor(K)
    _, fan, _ = hc.layout()
    refs = hc.fixture_reference(K)
    n_all = hc.num_points()
    assert [r['n'] for r in refs] == list(hc.PREFIX_COUNTS) + [0, 0, n_all]
    for b in range(10):
        assert np.array_equal(refs[b]['sel'], np.where((fan >= 0) & (fan <= b))[0])
    # bodies 0 and 1: no admissible pair at all; everywhere else every column has a candidate
    for b in (0, 1):
        assert (refs[b]['admissible'] == 0).all() and (refs[b]['argmin'] == -1).all() and np.isinf(refs[b]['min_d2']).all()
    for b in list(range(2, 10)) + [hc.EVERYTHING]:
        assert (refs[b]['admissible'] > 0).all() and (refs[b]['argmin'] >= 0).all(), b
    for b, r in enumerate(refs):
        if r['n'] == 0:
            continue
        # no borderline inside / outside decision
        assert np.abs(r['winding'] - hc.THRESH).min() > 1e-3, (b, np.abs(r['winding'] - hc.THRESH).min())
        np.testing.assert_allclose(np.linalg.norm(r['offs'] - r['pts'], axis=1), 0.001, rtol=1e-9)   # 1 mm off the point
    for b in (5, 6, 7, 8, 9, hc.EVERYTHING):
        assert refs[b]['exterior'].any() and (~refs[b]['exterior']).any(), b
    r = refs[hc.NO_INTERIOR_GRAD]
    assert hc.GRAD_TERMS[hc.NO_INTERIOR_GRAD, 0] == 0 and (~r['exterior']).sum() > 10
    if K == 1:
        # ... and some vertex carries only interior points that are no exterior point's partner: with no upstream gradient
        # for the interior sum it must get exactly nothing
        involved = r['exterior'].copy()
        involved[r['argmin'][r['exterior']]] = True
        assert (hc.supported_vertices(K, r) & ~hc.supported_vertices(K, dict(r, sel=r['sel'][involved]))).any()
    # the first selected point in the caller's order is not the only candidate for "slot 0": the body has other points
    assert refs[1]['sel'][0] == refs[1]['sel'].min() and refs[1]['n'] == 32
    # CSR lists: a vertex with more than 64 non-zero entries beside selected vertices with fewer than 5
    entries = np.bincount(hd_idx[hd_w != 0], minlength=verts.shape[1])
    assert entries.max() > 64
    for b in (5, hc.EVERYTHING):
        sup = hc.supported_vertices(K, refs[b])
        assert (entries[sup] > 64).any() and (entries[sup] < 5).any(), b
    # partners across slot 1024, for any slot order that keeps the points of a fan together: in body 8 (2048 points) every
    # point of fan 8 (1023 points) has its partner in fan 5 (958 points), and at least two different ones.  If fan 8 lies
    # on both sides of the boundary, fan 5 does not (two runs of consecutive slots cannot both contain slots 1023 and 1024),
    # and the points of fan 8 on the other side reach across; if fan 8 lies on one side it leaves one slot free there, so
    # all but at most one point of fan 5 lie on the other side
    r = refs[8]
    f = fan[r['sel']]
    of8 = np.where(f == 8)[0]
    assert len(of8) == 1023 and (f == 5).sum() == 958
    assert (f[r['argmin'][of8]] == 5).all() and len(np.unique(r['argmin'][of8])) >= 2


@pytest.mark.parametrize('K', hc.KS)
def test_no_offset_point_touches_the_surface(K):
    """The offset point of every HD point, in every pose that some body selects it in, lies clear of every triangle: its
    inside / outside flag does not depend on the precision it is computed in."""
    faces, _, verts, _ = hc.mesh()
    refs = hc.fixture_reference(K)
    seen = set()
    for b, r in enumerate(refs):
        for i, s in enumerate(r['sel']):
            key = (hc.BODY_POSE[b], int(s))
            if key in seen:
                continue
            seen.add(key)
            assert not point_touches_surface(r['offs'][i], verts[b], faces), (b, int(s))
