"""Every stage of the HD branch of RegressorLoss.contact_loss (csrc/hd_contact.hip: face flags, count / scatter, points,
terms, point adjoint, vertex gather; the searches of csrc/hd_search.hip and csrc/v2v.hip under it) against the float64
restatement of tests/hd_branch_cases.py, on a batch of 13 bodies whose selections are CONSTRUCTED to sit on the
structural edges of those kernels (see that file; tests/test_hd_branch_host.py proves the fixture's conditions without a
GPU).  Run with `-m gpu` on MI355X.

Bounds, all taken from the tests that already hold the same code to them:
  * a partner is admissible and its float64 squared distance exceeds the float64 masked minimum d2 by at most
    2e-6 d2 + 1e-9 (exact search, test_v2v_min_indexed_matches_brute_force) or 2e-6 d2 + 4e-6 (matrix-core search with
    points in any order, test_v2v_min_indexed_mfma_vs_exact); the observed worst excess is logged;
  * selection and inside / outside flags are exact (no offset point of the fixture is borderline);
  * the two sums per body against the restatement evaluated with the DEVICE's partners and flags (a tie in the search is
    then no issue): 1e-4 relative, the tolerance of the HD loss tests; the vertex gradient with
    grad_close(5e-6, quantum=True), the HD tolerance of test_gpu_train_step.py / test_gpu_properties.py."""
import contextlib

import numpy as np
import pytest
import torch

import hd_branch_cases as hc
from helpers import assert_close, grad_close, report_value

pytestmark = pytest.mark.gpu

# (hd_search, hd_search_waves, K, deterministic): every wave count with every row format, both modes with each
CASES = [(1, 4, 3, True), (1, 4, 1, False), (1, 4, 8, True),
         (1, 2, 3, False), (1, 2, 1, True), (1, 2, 8, False),
         (1, 1, 3, True), (1, 1, 1, False), (1, 1, 8, True),
         (0, 4, 3, False), (0, 4, 1, True), (0, 4, 8, False)]
OPTIONS = ('hd_search', 'hd_search_waves', 'hd_overlap', 'canary')


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def models():
    """The contact model of the golden mesh and one HD model per row format, built once."""
    from tuch_amd.ops import ContactModel, HDModel
    faces, gm, _, _ = hc.mesh()
    cm = ContactModel(faces, gm, None, device=dev())
    return cm, {K: HDModel(cm, *hc.regressor(K)) for K in hc.KS}


@contextlib.contextmanager
def options(cm, **values):
    before = {name: cm.get_option(name) for name in OPTIONS}
    try:
        for name, value in values.items():
            cm.set_option(name, value)
        yield
    finally:
        for name, value in before.items():
            cm.set_option(name, value)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def run(hd, bodies=None):
    """One forward and one backward of the fixture's batch (or of the bodies given) -> everything the device decided."""
    _, _, verts, euclthres = hc.mesh()
    exterior, min_d2, valid = hc.inputs()
    pick = np.arange(hc.BATCH) if bodies is None else np.asarray(bodies)
    batch = len(pick)
    v = torch.tensor(verts[pick], device=dev(), requires_grad=True)
    terms = hd.contact_terms(v, torch.tensor(exterior[pick], device=dev()), torch.tensor(min_d2[pick], device=dev()),
                             torch.zeros(batch, verts.shape[1], dtype=torch.int32, device=dev()),
                             torch.tensor(valid[pick], device=dev()), euclthres, hc.THRESH)
    saved = hd.last_saved
    terms.backward(torch.tensor(hc.GRAD_TERMS[pick], device=dev()))
    torch.cuda.synchronize()
    counts, sel = hd.selection(saved, batch)
    part, ext = hd.details(saved, batch)
    for b in range(batch):
        ext[b, counts[b]:] = False                        # (behind the count: never written)
    return dict(terms=terms.detach().cpu().numpy(), grad=v.grad.cpu().numpy(), counts=counts, sel=sel, part=part, ext=ext)


def same_decisions(a, b, what, rows_a=None):
    """terms, selection, partners and flags of two runs: the same bits (rows_a: the bodies of `a` that `b` holds)."""
    rows = slice(None) if rows_a is None else rows_a
    assert np.array_equal(bits(a['terms'][rows]), bits(b['terms'])), what
    for key in ('counts', 'sel', 'part', 'ext'):
        assert np.array_equal(a[key][rows], b[key]), (what, key)


def in_reference_order(ref, out, b):
    """The device's picks of body b as `evaluate` wants them: per position of ref['sel'] the partner's position and the
    flag; plus the position of every slot's point."""
    n = ref['n']
    ids = out['sel'][b, :n].astype(np.int64)
    slot_of = np.argsort(ids)                             # position i of the reference lives in slot slot_of[i]
    partner = np.searchsorted(ref['sel'], out['part'][b, :n][slot_of].astype(np.int64))
    return partner, out['ext'][b, :n][slot_of], np.searchsorted(ref['sel'], ids)


def check_against_reference(out, K, search, what):
    faces, _, verts, _ = hc.mesh()
    hd_idx, hd_w, hd_face = hc.regressor(K)
    refs = hc.fixture_reference(K)
    num_verts = verts.shape[1]
    assert out['terms'].dtype == np.float32 and out['grad'].dtype == np.float32
    assert np.isfinite(out['terms']).all() and np.isfinite(out['grad']).all()
    worst = 0.0
    for b, ref in enumerate(refs):
        n = ref['n']
        # 1. selection
        assert out['counts'][b] == n, (what, b, out['counts'][b], n)
        assert np.array_equal(np.sort(out['sel'][b, :n]), ref['sel']), (what, b)
        assert (out['sel'][b, n:] == -1).all() and (out['part'][b, n:] == -1).all(), (what, b)
        if n == 0:
            assert (out['terms'][b] == 0).all() and (out['grad'][b] == 0).all(), (what, b)
            continue
        partner, ext, pos = in_reference_order(ref, out, b)
        # 2. flags
        assert np.array_equal(ext, ref['exterior']), (what, b, int((ext != ref['exterior']).sum()))
        # 3. partners
        ids = out['part'][b, :n]
        assert np.isin(ids, ref['sel']).all(), (what, b)
        none = ref['admissible'] == 0
        assert (ref['sel'][partner[none]] == ref['sel'].min()).all(), (what, b)      # first selected in the caller's order
        some = np.where(~none)[0]
        if len(some):
            d2, ok = hc.pair_d2(ref, partner[some], some)
            assert ok.all(), (what, b, int((~ok).sum()))
            excess = d2 - ref['min_d2'][some]
            assert (excess >= -1e-18).all()
            bound = 2e-6 * ref['min_d2'][some] + (4e-6 if search else 1e-9)
            assert (excess <= bound).all(), (what, b, float(excess.max()), int((excess > bound).sum()))
            worst = max(worst, float(excess.max()))
        # 4. terms, 5. gradient: with the device's own partners and flags
        terms, grad = hc.evaluate(ref, partner, ext, hc.GRAD_TERMS[b], hd_idx, hd_w, num_verts)
        assert_close(out['terms'][b], terms, 1e-4, 0, '%s: terms of body %d' % (what, b))
        got = out['grad'][b]
        assert (got[~hc.supported_vertices(K, ref)] == 0).all(), (what, b)
        if b == 0:
            # one point, its own partner: d = 0
            assert (out['terms'][b] == 0).all() and (got == 0).all() and not terms.any() and not grad.any(), what
            continue
        grad_close(got, grad, 5e-6, '%s: vertex gradient of body %d' % (what, b), quantum=True)
        if b == hc.NO_INTERIOR_GRAD:
            # no upstream gradient for the interior sum: the gradient is that of the exterior points alone, and the vertices
            # that only interior points (and nobody's exterior partner) rest on get exactly nothing
            assert (~ext).sum() > 10 and ext.any()
            _, only = hc.evaluate(ref, partner, ext, hc.GRAD_TERMS[b], hd_idx, hd_w, num_verts, keep=ext)
            grad_close(got, only, 5e-6, '%s: exterior-only gradient of body %d' % (what, b), quantum=True)
            involved = np.zeros(n, bool)
            involved[ext] = True
            involved[partner[ext]] = True
            rest = dict(ref, sel=ref['sel'][involved])
            # (such vertices exist for K = 1: test_hd_branch_host.py; with K = 3 and 8 every point of a fan rests on its centre)
            assert (got[~hc.supported_vertices(K, rest)] == 0).all(), what
    report_value('hd branch %s: worst partner excess over the float64 minimum' % what, worst)


def check_edges_reached(out):
    """7. the batch really sits on the edges: tiles of 9..16 and of more than 16 mask vertices, partners across slot 1024,
    a body of more than 2048 points, and a first point in the caller's order that is not slot 0."""
    faces = hc.mesh()[0]
    hd_face = hc.layout()[0]
    tiles_mid = tiles_high = straddle = 0
    for b in list(range(10)) + [hc.EVERYTHING]:
        n = int(out['counts'][b])
        ids = out['sel'][b, :n].astype(np.int64)
        runs, distinct = hc.tile_runs(faces[hd_face[ids], 0])
        tiles_mid += int(((runs >= 9) & (runs <= 16) & (distinct >= 9)).sum())
        tiles_high += int((distinct > 16).sum())
        if n > 1024:
            slot_of_id = np.full(len(hd_face), -1, np.int64)
            slot_of_id[ids] = np.arange(n)
            partner_slot = slot_of_id[out['part'][b, :n].astype(np.int64)]
            assert (partner_slot >= 0).all()
            straddle += int(((np.arange(n) < 1024) != (partner_slot < 1024)).sum())
    assert tiles_mid > 0 and tiles_high > 0 and straddle > 0, (tiles_mid, tiles_high, straddle)
    assert out['counts'].max() > 2048 and out['counts'][hc.EVERYTHING] % 32 != 0
    assert out['sel'][1, 0] != out['sel'][1, :32].min()


@pytest.mark.parametrize('search,waves,K,deterministic', CASES)
def test_hd_branch_against_float64(models, search, waves, K, deterministic):
    """Checks 1-7 of the module's head for one combination of search form, wave count, row format and mode; then
    6. two calls agree bit for bit (the gradient too in deterministic mode), hd_overlap = 0 gives the bits of hd_overlap = 1,
    and every body sent alone gives the bits it has in the batch."""
    from tuch_amd import ops
    cm, hds = models
    hd = hds[K]
    what = 'search=%d waves=%d K=%d %s' % (search, waves, K, 'fixed' if deterministic else 'float')
    mode_before = ops.deterministic()
    with options(cm, hd_search=search, hd_search_waves=waves, hd_overlap=1), ops.deterministic_mode(deterministic):
        assert ops.deterministic() == deterministic and cm.get_option('hd_search_waves') == waves
        out = run(hd)
        check_against_reference(out, K, search, what)
        check_edges_reached(out)
        again = run(hd)
        same_decisions(out, again, what + ': second call')
        if deterministic:
            assert np.array_equal(bits(out['grad']), bits(again['grad'])), what
        cm.set_option('hd_overlap', 0)
        assert cm.get_option('hd_overlap') == 0
        serial = run(hd)
        same_decisions(out, serial, what + ': hd_overlap=0')
        if deterministic:
            assert np.array_equal(bits(out['grad']), bits(serial['grad'])), what
        else:
            assert np.allclose(out['grad'], serial['grad'], rtol=1e-4, atol=1e-6 * np.abs(out['grad']).max())
        cm.set_option('hd_overlap', 1)
        for b in range(hc.BATCH):
            alone = run(hd, [b])
            same_decisions(out, alone, '%s: body %d alone' % (what, b), rows_a=slice(b, b + 1))
            if deterministic:
                assert np.array_equal(bits(out['grad'][b]), bits(alone['grad'][0])), (what, b)
    assert ops.deterministic() == mode_before              # restored


def test_hd_branch_keeps_inside_its_workspace_regions(models):
    """8. option canary: guard words behind every region of the branch's workspace and saved state (forward, adjoint and
    both searches) are intact after a run of the edge batch."""
    cm, hds = models
    for search, K in ((1, 8), (0, 1)):
        with options(cm, hd_search=search, canary=1):
            cm.canary_hits(reset=True)
            out = run(hds[K])
            assert cm.canary_hits() == 0
            assert out['counts'].tolist() == [r['n'] for r in hc.fixture_reference(K)]
