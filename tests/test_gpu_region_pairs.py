"""The region-pair kernels of csrc/region_min.hip (all pairs / few selected pairs, plain / inverted keys, finalize,
backward) and the key decode of stage2_fused_kernel (csrc/contact_terms.hip) against the float64 references of
tests/region_pair_cases.py, at region sizes on both sides of every size branch of the kernels (see that file and
tests/test_region_pair_cases.py).  Run with `-m gpu` on MI355X.

Bounds (u = 2^-24, half an ulp of 1 in float32):
  * 'grid' vertices: every float32 operation of the search is exact, so minima, index pairs, keys, the stage-2 total and
    both gradients equal the float64 reference bit for bit, ties included (first flat index);
  * 'raw' vertices: |out - min| <= 8 u min (three rounded differences, one product, two FMAs of non-negative terms); the
    returned pair is admissible and its float64 d2 is <= min (1 + 16 u) (a near-tie may pick another pair, never a farther
    one); a gradient component is within (n + 3) u S of the float64 sum of its n contributions, S the sum of their
    magnitudes (a rounded difference and product per contribution, n - 1 rounded additions, the conversion from fixed point);
  * the stage-2 total is within P B u total of the float64 sum of the float32 minima (a float32 sum of P B non-negative
    terms in any order) -- that alternative of the two is the one used; on 'grid' the sum is exact and equality is asserted."""
import functools

import numpy as np
import pytest
import torch

import region_pair_cases as rc
from helpers import golden, report_value

pytestmark = pytest.mark.gpu
U = rc.U
SETS = ['grid', 'raw']


def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def model():
    from tuch_amd.ops import ContactModel
    m = ContactModel(golden(rc.TAG)['faces'], rc.mask(), None, list(rc.regions()[1]), rc.pairs(), device=dev())
    _searched.cache_clear()
    _searched.model = m
    yield m
    _searched.cache_clear()
    _searched.model = None


@functools.lru_cache(maxsize=None)
def _searched(which, masked, selected):
    """(out [B,P] float32, ij [B,P,2]) of tuch_region_pair_min as numpy, once per module (read-only)."""
    verts = torch.tensor(rc.vertices(which), device=dev())
    sel = torch.tensor(rc.select(), device=dev()) if selected else None
    out, ij = _searched.model.region_pair_min(verts, select=sel, masked=masked)
    out, ij = out.cpu().numpy(), ij.cpu().numpy().astype(np.int64)
    out.setflags(write=False)
    ij.setflags(write=False)
    return out, ij


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_search(out, ij, which, masked, entries, what):
    """out / ij of the entries [B,P] bool against the float64 reference (the module's head comment)."""
    ref = rc.reference(which, masked)
    lists, gm = rc.regions()[1], rc.mask()
    v = rc.vertices(which).astype(np.float64)
    assert out.dtype == np.float32 and entries.any()
    none = entries & (ref['flat'] < 0)
    assert none.any() == masked                           # the fully inadmissible pairs
    assert (out[none] == 0).all() and (ij[none] == -1).all()
    some = entries & (ref['flat'] >= 0)
    if which == 'grid':
        assert np.array_equal(out[some].astype(np.float64), ref['min'][some]), what
        assert np.array_equal(ij[some], ref['ij'][some]), what
        assert np.array_equal(rc.flat_of(ij)[some], ref['flat'][some]), what
        return
    worst_value = worst_pick = 0.0
    for b, p in zip(*np.nonzero(some)):
        mn, (i, j) = ref['min'][b, p], ij[b, p]
        r1, r2 = (lists[r] for r in rc.pairs()[p])
        assert i in r1 and j in r2 and (not masked or gm[i, j]), (what, b, p, i, j)
        err, d2 = abs(float(out[b, p]) - mn), ((v[b, i] - v[b, j]) ** 2).sum()
        assert err <= 8 * U * mn, (what, b, rc.PAIR_NAMES[p], float(out[b, p]), mn)
        assert d2 <= mn * (1 + 16 * U), (what, b, rc.PAIR_NAMES[p], d2, mn)
        if mn > 0:
            worst_value, worst_pick = max(worst_value, err / mn / U), max(worst_pick, (d2 / mn - 1) / U)
    report_value('region pairs %s: max |out - min| / (u min), bound 8' % what, worst_value)
    report_value('region pairs %s: max (d2(i, j) / min - 1) / u, bound 16' % what, worst_pick)


@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('which', SETS)
def test_all_pairs_form_vs_float64(model, which, masked):
    out, ij = _searched(which, masked, False)
    check_search(out, ij, which, masked, np.ones(out.shape, bool), '%s %s all pairs' % (which, 'masked' if masked else 'plain'))


@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('which', SETS)
def test_selected_pairs_form_vs_float64_and_the_all_pairs_form(model, which, masked):
    sel = rc.select()
    out, ij = _searched(which, masked, True)
    check_search(out, ij, which, masked, sel, '%s %s selected pairs' % (which, 'masked' if masked else 'plain'))
    out_all, ij_all = _searched(which, masked, False)
    assert np.array_equal(bits(out[sel]), bits(out_all[sel])) and np.array_equal(ij[sel], ij_all[sel])
    assert (bits(out[~sel]) == 0).all() and (ij[~sel] == -1).all()


def _keys(model, which, masked, selected):
    """~keys of tuch_region_pair_keys as uint64 [B,P] (0 stays 0: no candidate)."""
    from tuch_amd import _C
    verts = torch.tensor(rc.vertices(which), device=dev())
    sel = torch.tensor(rc.select().astype(np.uint8), device=dev()) if selected else None
    keys = torch.zeros(verts.shape[0], model.num_pairs, dtype=torch.int64, device=dev())
    _C.check(_C.lib().tuch_region_pair_keys(model._handle, _C.ptr(verts), verts.shape[0], _C.ptr(sel), int(masked), _C.ptr(keys),
                                            _C.stream()))
    raw = keys.cpu().numpy().view(np.uint64)
    return keys, np.where(raw == 0, np.uint64(0), ~raw)


@pytest.mark.parametrize('selected', [True, False])
@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('which', SETS)
def test_inverted_keys(model, which, masked, selected):
    """The complement of a key is bits(min d2) << 32 | flat index of the plain forms' answer (checked against float64 by
    the tests above; on 'grid' the reference's own flat index as well); 0: unselected, or no admissible column."""
    keys, plain = _keys(model, which, masked, selected)
    out, ij = _searched(which, masked, selected)
    flat = rc.flat_of(ij)
    want = np.where(flat >= 0, (bits(out).astype(np.uint64) << np.uint64(32)) | flat.astype(np.uint64), np.uint64(0))
    raw = keys.cpu().numpy().view(np.uint64)
    assert np.array_equal(raw == 0, flat < 0)
    assert np.array_equal(plain, want)
    entries = rc.select() if selected else np.ones(flat.shape, bool)
    assert np.array_equal(flat < 0, ~entries | (rc.reference(which, masked)['flat'] < 0))
    if which == 'grid':
        ref = rc.reference(which, masked)
        some = entries & (ref['flat'] >= 0)
        assert np.array_equal((plain & np.uint64(0xffffffff)).astype(np.int64)[some], ref['flat'][some])
        assert np.array_equal((plain >> np.uint64(32)).astype(np.uint32)[some], bits(ref['min'].astype(np.float32))[some])


def check_gradient(grad, verts, ij, g, which, what):
    """grad [B,V,3] against grad_reference: exact on 'grid', (n + 3) u S on 'raw'."""
    want, s, n = rc.grad_reference(verts, ij, g)
    assert (n > 1).any() and np.abs(want).max() > 0
    grad = np.asarray(grad, np.float64)
    if which == 'grid':
        assert np.array_equal(grad, want), what
        return
    err, bound = np.abs(grad - want), (n + 3) * U * s
    report_value('region pairs %s: max gradient error / ((n + 3) u S), bound 1' % what,
                 float((err[s > 0] / bound[s > 0]).max()))
    assert (err <= bound).all(), (what, float((err - bound).max()))


@pytest.mark.parametrize('selected', [True, False])
@pytest.mark.parametrize('which', SETS)
def test_stage2_fused_decodes_the_keys(model, which, selected):
    """tuch_smplify_stage2_fused with no valid body and zero small terms: the total is r2r_scale * sum of the minima in
    the keys, the gradient the region term's alone.  The keys (masked with the select patterns, unmasked for all pairs)
    are decoded HERE with the region lists -- that they are right is test_inverted_keys' business."""
    from tuch_amd import _C, ops
    masked = selected
    keys, plain = _keys(model, which, masked, selected)
    lists, sizes = rc.regions()[1], rc.pair_sizes()
    B, P = plain.shape
    d2 = (plain >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    ij = np.full((B, P, 2), -1, np.int64)
    for b, p in zip(*np.nonzero(plain)):
        idx = int(plain[b, p] & np.uint64(0xffffffff))
        ij[b, p] = lists[rc.pairs()[p][0]][idx // sizes[p][1]], lists[rc.pairs()[p][1]][idx % sizes[p][1]]
    d2[plain == 0] = 0.0
    contact_scale, r2r_scale = 10.0, 2.0
    total_want = r2r_scale * d2.sum()
    if which == 'grid':                       # multiples of 2^-12 with a sum below 2^12: exact in float32 in any order
        assert np.array_equal(d2 * 4096, np.round(d2 * 4096)) and d2.sum() < 4096

    verts_np = rc.vertices(which)
    N = verts_np.shape[1]
    L = _C.lib()
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev())
    verts, partner, exterior, valid, small = (torch.tensor(verts_np, device=dev()), z(B, N, dtype=torch.int32),
                                              z(B, N, dtype=torch.uint8), z(B, dtype=torch.uint8), z(B, 2))
    share = torch.empty(L.tuch_smplify_stage2_fused_scratch_floats(B), dtype=torch.float32, device=dev())
    ticket = z(1, dtype=torch.int32)

    def run(grad=None, fixed=None):
        out = z(1)
        _C.check(L.tuch_smplify_stage2_fused(_C.ptr(verts), _C.ptr(partner), _C.ptr(exterior), _C.ptr(valid), B, N,
                                             ops.MODE_SMPLIFY, 0.0, _C.ptr(small), P, contact_scale, r2r_scale, _C.ptr(share),
                                             _C.ptr(ticket), _C.ptr(out), _C.ptr(grad), model._handle, _C.ptr(keys), _C.ptr(fixed),
                                             _C.stream()))
        assert int(ticket.item()) == 0
        return out

    def fixed_to_float(fixed):
        out = torch.empty(B, N, 3, dtype=torch.float32, device=dev())
        _C.check(L.tuch_fixed_to_float(_C.ptr(fixed), fixed.numel(), _C.ptr(out), _C.stream()))
        return out.cpu().numpy()

    what = '%s stage-2 decode, %s' % (which, 'selected, masked' if selected else 'all pairs, plain')
    grad, fixed = z(B, N, 3), z(B, N, 3, dtype=torch.int64)
    totals = [run(), run(grad=grad), run(fixed=fixed)]
    assert torch.equal(totals[0], totals[1]) and torch.equal(totals[0], totals[2])
    total = float(totals[0].item())
    report_value('region pairs %s: |total - float64| / (P B u total), bound 1' % what,
                 abs(total - total_want) / max(P * B * U * total_want, 1e-300))
    assert abs(total - total_want) <= P * B * U * total_want and total_want > 0
    if which == 'grid':
        assert total == total_want
    g = np.where(plain != 0, r2r_scale, 0.0)
    check_gradient(grad.cpu().numpy(), verts_np, ij, g, which, what + ' (float atomics)')
    first = fixed.clone()
    check_gradient(fixed_to_float(fixed), verts_np, ij, g, which, what + ' (fixed point)')
    # the same buffers again: the ticket was left zero, the fixed-point sums do not depend on the order of arrival
    fixed.zero_()
    again = run(fixed=fixed)
    assert torch.equal(again, totals[0]) and torch.equal(fixed, first) and bool((first != 0).any())


@pytest.mark.parametrize('selected', [False, True])
@pytest.mark.parametrize('which', SETS)
def test_backward_vs_float64(model, which, selected):
    """region_pair_min_bwd_kernel through autograd, masked (so (-1, -1) entries are among them), with a non-uniform
    upstream gradient that has zeros; (1, 1602) and (1602, 1) share their arg-min vertices."""
    verts_np, g = rc.vertices(which), rc.upstream(which)
    verts = torch.tensor(verts_np, device=dev(), requires_grad=True)
    sel = torch.tensor(rc.select(), device=dev()) if selected else None
    out, ij = model.region_pair_min(verts, select=sel, masked=True)
    out.backward(torch.tensor(g, device=dev()))
    ij = ij.cpu().numpy().astype(np.int64)
    assert np.array_equal(ij, _searched(which, True, selected)[1]) and (ij < 0).any() and (g == 0).any()
    if not selected:
        a, b = rc.PAIR_NAMES.index((1, 1602)), rc.PAIR_NAMES.index((1602, 1))
        assert np.array_equal(ij[:, a], ij[:, b, ::-1]) and (g[:2, a] != 0).all() and (g[:2, b] != 0).all()
    check_gradient(verts.grad.cpu().numpy(), verts_np, ij, g, which,
                   '%s backward, %s' % (which, 'selected' if selected else 'all pairs'))
