"""Regions, pairs, select patterns and float64 references shared by the region-pair tests (tests/test_region_pair_cases.py
on the CPU, tests/test_gpu_region_pairs.py on the device).  numpy only, no GPU here.

The kernels of csrc/region_min.hip change form with the SIZES of the two regions of a pair (LDS tile, preloaded mask words,
column quarters of the few-pairs form, rounds of row blocks, float4 reads with a scalar tail): the regions here are
cut from one seeded permutation of the `medium` golden's 1602 vertices at sizes on both sides of every such edge.  They
are in shuffled order, so a flat index a * n2 + k in region-list order cannot be mistaken for one in vertex order, and
they overlap (ContactModel accepts that), so the unmasked minimum of many pairs is an exact tie at d2 = 0.

Two vertex sets: 'raw', the golden's float32 vertices, and 'grid', the same rounded to multiples of 2^-6: with
|coordinate| < 1 every difference (a multiple of 2^-6 below 2), square (a multiple of 2^-12 below 4) and three-term
sum (below 12) is exact in float32, so a float32 d2 in any operation order equals the float64 value bit for bit and
ties are exact."""
from __future__ import annotations

import functools

import numpy as np

import helpers

TAG = 'medium'
SIZES = (1, 31, 33, 64, 65, 255, 257, 513, 520, 1025, 1100, 1602)
REGION_SEED, SELECT_SEED = 11, 12
GRID = 2.0 ** -6
U = 2.0 ** -24            # float32: half an ulp of 1

# (first, second) by region name: a size, or 'N0' = every vertex the mask rules out for the one vertex of region 1
PAIR_NAMES = (
    (1100, 1602), (1602, 1100), (1025, 1025), (1602, 1602), (513, 520), (520, 513), (257, 255), (255, 257),
    (64, 65), (65, 64), (31, 33), (33, 31), (33, 1100), (1100, 33), (1, 1), (1, 'N0'), ('N0', 1), (1, 1602), (1602, 1),
    (257, 1025), (1025, 257), (513, 513), (520, 1100), (1100, 520))
SUBSET_MUST = ((1602, 1100), (1, 'N0'))


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def mask() -> np.ndarray:
    return helpers.golden_mask(TAG)


@functools.lru_cache(maxsize=None)
def vertices(which: str) -> np.ndarray:
    """[3,1602,3] float32: 'raw' or 'grid' (read-only)."""
    v = np.array(helpers.golden(TAG)['verts'], np.float32)
    if which == 'grid':
        v = (np.round(v.astype(np.float64) / GRID) * GRID).astype(np.float32)
    else:
        assert which == 'raw'
    assert np.abs(v).max() < 1.0
    _readonly(v)
    return v


@functools.lru_cache(maxsize=None)
def regions():
    """(names, lists): every region is a window of one seeded permutation of the vertices, rotated by a seeded offset of
    its own (no vertex twice within a region; regions overlap); 'N0' keeps the permutation's order too.
    The whole-body region starts at the first vertex of the permutation that shares its 'grid' position in body 1 (the
    body with every pair selected) with a vertex less than 256 places behind it: row 0 of (1602, 1602) then attains the
    unmasked minimum d2 = 0 twice, in columns 0 and k < 256 -- one lane, one column quarter, one LDS tile of either
    kernel: a tie that only the strict '<' of the column loop resolves to the first index."""
    num_verts = mask().shape[0]
    rng = np.random.default_rng(REGION_SEED)
    perm = rng.permutation(num_verts)
    names, lists = [], []
    for size in SIZES:
        names.append(size)
        offset = int(rng.integers(num_verts))
        if size == num_verts:
            at = vertices('grid')[1][perm]
            offset = next(o for o in range(num_verts)
                          if (at[(o + 1 + np.arange(255)) % num_verts] == at[o]).all(1).any())
        lists.append(np.roll(perm, -offset)[:size].astype(np.int64))
    single = int(lists[names.index(1)][0])
    names.append('N0')
    lists.append(perm[~mask()[single, perm]].astype(np.int64))
    _readonly(*lists)
    return tuple(names), tuple(lists)


@functools.lru_cache(maxsize=None)
def pairs() -> np.ndarray:
    """[P,2] region indices."""
    names = regions()[0]
    p = np.asarray([[names.index(a), names.index(b)] for a, b in PAIR_NAMES], np.int64)
    _readonly(p)
    return p


def pair_sizes():
    """[(n1, n2)] of every pair."""
    lists = regions()[1]
    return [(len(lists[a]), len(lists[b])) for a, b in pairs()]


@functools.lru_cache(maxsize=None)
def select() -> np.ndarray:
    """[3,P] bool: body 0 nothing, body 1 every pair, body 2 a seeded subset of five with SUBSET_MUST in it."""
    num_pairs = len(PAIR_NAMES)
    sel = np.zeros((3, num_pairs), bool)
    sel[1] = True
    must = [PAIR_NAMES.index(p) for p in SUBSET_MUST]
    rest = [k for k in range(num_pairs) if k not in must]
    sel[2, must] = True
    sel[2, np.random.default_rng(SELECT_SEED).choice(rest, 5 - len(must), replace=False)] = True
    _readonly(sel)
    return sel


def pair_d2(verts_b, r1, r2, mask_block=None) -> np.ndarray:
    """[n1,n2] float64 squared distances of one body's float32 vertices (cast first), +inf where the mask block is False."""
    v = np.asarray(verts_b).astype(np.float64)
    d2 = ((v[r1][:, None, :] - v[r2][None, :, :]) ** 2).sum(-1)
    if mask_block is not None:
        d2 = np.where(mask_block, d2, np.inf)
    return d2


@functools.lru_cache(maxsize=None)
def reference(which: str, masked: bool):
    """The float64 minimum of every (body, pair): dict of
         min [B,P] float64 (0 where no column is admissible), ij [B,P,2] vertex ids ((-1, -1) there), flat [B,P] the FIRST
         flat index a * n2 + k attaining it (-1 there), last [B,P] the last one, count [B,P] how many attain it,
         row_last [B,P] the last one in the row of the first (a * n2 + k with the same a)."""
    verts, (_, lists), gm = vertices(which), regions(), mask()
    num_bodies, num_pairs = verts.shape[0], len(PAIR_NAMES)
    out = dict(min=np.zeros((num_bodies, num_pairs)), ij=np.full((num_bodies, num_pairs, 2), -1, np.int64),
               flat=np.full((num_bodies, num_pairs), -1, np.int64), last=np.full((num_bodies, num_pairs), -1, np.int64),
               count=np.zeros((num_bodies, num_pairs), np.int64), row_last=np.full((num_bodies, num_pairs), -1, np.int64))
    for p, (ra, rb) in enumerate(pairs()):
        r1, r2 = lists[ra], lists[rb]
        block = gm[np.ix_(r1, r2)] if masked else None
        for b in range(num_bodies):
            d2 = pair_d2(verts[b], r1, r2, block)
            flat = int(np.argmin(d2.reshape(-1)))                 # the first flat index
            mn = d2.reshape(-1)[flat]
            if not np.isfinite(mn):
                continue
            hits = np.flatnonzero(d2.reshape(-1) == mn)
            out['min'][b, p], out['flat'][b, p], out['last'][b, p], out['count'][b, p] = mn, flat, hits[-1], len(hits)
            out['ij'][b, p] = r1[flat // len(r2)], r2[flat % len(r2)]
            out['row_last'][b, p] = hits[hits // len(r2) == flat // len(r2)][-1]
    _readonly(*out.values())
    return out


def flat_of(ij) -> np.ndarray:
    """[B,P] flat index a * n2 + k of vertex-id pairs ij [B,P,2] in region-list order (-1 for (-1, -1)): a region holds no
    vertex twice, so the position of a vertex in it is unique."""
    lists = regions()[1]
    ij = np.asarray(ij, np.int64)
    flat = np.full(ij.shape[:2], -1, np.int64)
    for p, (ra, rb) in enumerate(pairs()):
        pos1 = {int(v): k for k, v in enumerate(lists[ra])}
        pos2 = {int(v): k for k, v in enumerate(lists[rb])}
        for b in range(ij.shape[0]):
            i, j = int(ij[b, p, 0]), int(ij[b, p, 1])
            if i >= 0:
                flat[b, p] = pos1[i] * len(lists[rb]) + pos2[j]
    return flat


def grad_reference(verts, ij, g):
    """d sum(g * min d2) / d verts for given arg-min pairs: +2 g (v_i - v_j) to i, the negative to j, summed in float64.
    Returns (grad [B,V,3], S [B,V,3] the sum of the |contributions| per component, n [B,V,3] how many there were);
    entries with (-1, -1) or g == 0 contribute nothing."""
    v = np.asarray(verts).astype(np.float64)
    ij, g = np.asarray(ij, np.int64), np.asarray(g).astype(np.float64)
    grad, s, n = np.zeros_like(v), np.zeros_like(v), np.zeros(v.shape, np.int64)
    for b in range(v.shape[0]):
        for p in range(ij.shape[1]):
            i, j = ij[b, p]
            if i < 0 or j < 0 or g[b, p] == 0.0:
                continue
            c = 2.0 * g[b, p] * (v[b, i] - v[b, j])
            grad[b, i] += c
            grad[b, j] -= c
            s[b, i] += np.abs(c)
            s[b, j] += np.abs(c)
            n[b, i] += 1
            n[b, j] += 1
    return grad, s, n


def upstream(which: str) -> np.ndarray:
    """[3,P] float32 upstream gradient of region_pair_min: powers of two on 'grid' (every product stays dyadic), seeded
    uniform values on 'raw'; zeros in both."""
    num_pairs = len(PAIR_NAMES)
    rng = np.random.default_rng(SELECT_SEED + 1)
    if which == 'grid':
        g = 2.0 ** rng.integers(-3, 4, (3, num_pairs))
    else:
        g = rng.uniform(0.25, 4.0, (3, num_pairs))
    g[0, 3] = g[1, 0] = g[2, PAIR_NAMES.index((1, 1602))] = 0.0
    return g.astype(np.float32)
