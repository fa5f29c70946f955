"""GPU: the near lists of the ray-crossing inside test (csrc/ray_winding.hip: ray_leaf_bounds_kernel, ray_near_kernel)
through tuch_ray_near_debug.  The lists may hold more (ray, leaf) pairs than can cross -- the walk filters and tests
exactly -- but never fewer:

  * every (query, leaf) pair with lo[k] <= r[k] <= hi[k] for all 13 slabs, evaluated in float64 from the returned
    single-precision bounds and ray values, is listed;
  * every decoded 16-bit record bound lies on the outward side of its single-precision bound (or is the saturated code
    that never rejects);
  * padding slots are listed nowhere; a block's list names each leaf once, and in the one-wavefront form in ascending
    order (the order of stage 1's queue);
  * the flags are reproducible and equal the fixture's wherever the fixture's winding number is clear of the threshold.

Inputs are the smallest that can go wrong: the two small bodies (every vertex lies exactly ON a bound of the leaves that
hold its faces), the full body (430 leaves: seven rounds of stage 1, the last partial), the small body far from the origin
(the records are relative to a reference point), scaled past the fixed-point range (saturation), with a NaN vertex, and
the points form with ragged counts (0, 1, 65).  Vertices and points, one and four wavefronts per query block."""
import functools

import numpy as np
import pytest
import torch

from helpers import golden

pytestmark = pytest.mark.gpu

SCALE = 8192.0
LOWER = [0, 1, 3, 4, 6, 8]          # the ray value each of the record's 13 halves meets: six lower bounds ...
UPPER = [0, 1, 2, 3, 4, 5, 7]       # ... and seven upper bounds


def dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def model_of(tag):
    from tuch_amd.ops import ContactModel
    return ContactModel(golden(tag)['faces'], None, None, None, None, device=dev())


def body_case(name):
    """(tag, verts [B,V,3] float32) of a named input."""
    tag = {'small': 'small', 'ico_small': 'ico_small', 'full': 'full'}.get(name, 'small')
    v = golden(tag)['verts'].astype(np.float32).copy()
    v = v[:1] if tag == 'full' else v[:2]
    if name == 'far':
        v = v + np.array([30.0, -20.0, 25.0], np.float32)
    elif name == 'very_far':
        v = v + np.array([0.0, 0.0, 1.0e4], np.float32)
    elif name == 'scaled':
        v = v * np.float32(8.0)
    elif name == 'nan':
        v[0, 57] = np.nan
    elif name == 'many':             # the small body often enough that the step takes the one-wavefront form by itself:
        v = np.concatenate([v] * 513)    # 2 query blocks x 1026 bodies > 2048 workgroups
    return tag, v


def decode(records):
    """[B][L][8] int32 -> levels [B][13][L] (int), leaf numbers [B][L]."""
    r = records.view(np.uint32).astype(np.int64)
    halves = np.stack([r[..., 0] & 0xffff, r[..., 0] >> 16, r[..., 1] & 0xffff, r[..., 1] >> 16, r[..., 2] & 0xffff,
                       r[..., 2] >> 16, r[..., 3] & 0xffff, r[..., 3] >> 16, r[..., 4] & 0xffff, r[..., 4] >> 16,
                       r[..., 5] & 0xffff, r[..., 5] >> 16, r[..., 6] & 0xffff], 1)
    halves = np.where(halves >= 32768, halves - 65536, halves)
    return halves, r[..., 6] >> 16


def check_lists(d, real_counts, waves, what, expect_pairs=True):
    bounds, rays = d['bounds'].astype(np.float64), d['rays'].astype(np.float64)
    B, _, L = bounds.shape
    slots = rays.shape[1]
    levels, leaf_no = decode(d['records'])
    assert np.array_equal(leaf_no, np.broadcast_to(np.arange(L), (B, L))), what
    # records: outward of the single-precision bounds, or the code that never rejects (also for a NaN bound)
    for j in range(13):
        lv, bd = levels[:, j], bounds[:, j]
        if j < 6:
            ok = (lv == -32768) | (lv / SCALE <= bd)
        else:
            ok = (lv == 32767) | (lv / SCALE >= bd)
        assert ok.all(), (what, j, lv[~ok][:4], bd[~ok][:4])
    listed = np.unpackbits(d['bitmap'], axis=2, bitorder='little').astype(bool)        # [B][L][slots]
    assert listed.shape == (B, L, slots)
    required_total = 0
    for b in range(B):
        n = int(real_counts[b])
        real = np.arange(slots) < n
        inside = np.ones((L, slots), bool)
        with np.errstate(invalid='ignore'):
            for j, k in enumerate(LOWER):
                inside &= bounds[b, j][:, None] <= rays[b, :, k][None, :]
            for j, k in enumerate(UPPER):
                inside &= rays[b, :, k][None, :] <= bounds[b, 6 + j][:, None]
        inside &= real[None, :]
        missing = inside & ~listed[b]
        assert not missing.any(), (what, b, np.argwhere(missing)[:5])
        assert not listed[b][:, ~real].any(), (what, b, 'a padding slot is listed')
        required_total += int(inside.sum())
        # the lists themselves: each leaf once per block, the leaves with a bit set, ascending in the one-wavefront form
        for qb in range(slots // 64):
            m = int(d['lengths'][b, qb])
            got = d['leaves'][b, qb, :m]
            want = np.nonzero(listed[b][:, qb * 64:(qb + 1) * 64].any(1))[0]
            assert (d['leaves'][b, qb, m:] == -1).all(), (what, b, qb)
            assert np.array_equal(np.sort(got), want), (what, b, qb, got, want)
            if waves == 1:
                assert np.array_equal(got, want), (what, b, qb, 'not in ascending leaf order', got)
    if expect_pairs:
        assert required_total > 0, what
    return required_total, int(listed.sum())


@pytest.mark.parametrize('waves', [1, 4])
@pytest.mark.parametrize('name', ['small', 'ico_small', 'full', 'far', 'very_far', 'scaled', 'nan'])
def test_no_pair_is_dropped_vertices(name, waves):
    tag, v = body_case(name)
    model = model_of(tag)
    verts = torch.tensor(v, device=dev())
    d = model.ray_near_debug(verts, waves=waves)
    V = v.shape[1]
    required, listed = check_lists(d, [V] * v.shape[0], waves, '%s, %d waves' % (name, waves))
    if name == 'full':
        # the test can fail: far from every (leaf, vertex) pair is listed (a ray meets a handful of the 430 leaves), and
        # the list is close to what is required: rounding apart widens a slab by at most two steps of 2^-13 m (0.25 mm)
        # against leaves a few centimetres across -- about 1 % more pairs per slab direction, a few slabs decide a pair
        assert listed < 0.1 * d['bounds'].shape[2] * V, listed
        assert listed <= 1.05 * required, (listed, required)
    if name == 'nan':
        assert np.isnan(d['rays'][0]).any() and not np.isnan(d['rays'][1, :V]).any()
        return                                          # (the walk is not part of this test)
    # flags: reproducible, and the fixture's wherever its winding number is clear of the threshold
    e1 = model.exterior_flags(verts, apply_segments=False).cpu().numpy()
    e2 = model.exterior_flags(verts, apply_segments=False).cpu().numpy()
    assert np.array_equal(e1, e2)
    if name in ('small', 'ico_small', 'full'):
        w = golden(tag)['winding'][:v.shape[0]]
        clear = np.abs(w - 0.99) > 1e-4
        assert np.array_equal(e1.astype(bool)[clear], (w <= 0.99)[clear])


def test_the_step_takes_the_form_its_sizes_ask_for():
    """waves = 0: four wavefronts per block at B = 2, one at B = 1026 of the small body (more than 2048 query blocks);
    either lists the same pairs and gives the same flags."""
    tag, v2 = body_case('small')
    _, many = body_case('many')
    model = model_of(tag)
    a = model.ray_near_debug(torch.tensor(v2, device=dev()), waves=0)
    c = model.ray_near_debug(torch.tensor(many, device=dev()), waves=0)
    V = v2.shape[1]
    check_lists(a, [V] * 2, 4, 'small, B = 2')
    ends = {k: np.concatenate([x[:2], x[-2:]]) for k, x in c.items()}
    check_lists(ends, [V] * 4, 1, 'small, B = 1026')      # ascending order: the one-wavefront form
    assert np.array_equal(c['bitmap'], np.concatenate([a['bitmap']] * 513))
    assert np.array_equal(np.sort(c['leaves'], axis=2), np.concatenate([np.sort(a['leaves'], axis=2)] * 513))
    e2 = model.exterior_flags(torch.tensor(v2, device=dev()), apply_segments=False).cpu().numpy()
    em = model.exterior_flags(torch.tensor(many, device=dev()), apply_segments=False).cpu().numpy()
    assert np.array_equal(em, np.concatenate([e2] * 513))


@pytest.mark.parametrize('waves', [1, 4])
def test_no_pair_is_dropped_points_with_ragged_counts(waves):
    tag, v = body_case('small')
    model = model_of(tag)
    verts = torch.tensor(np.concatenate([v, v[:1]]), device=dev())             # three bodies
    rng = np.random.default_rng(11)
    q = 70
    base = verts.cpu().numpy()[:, rng.integers(0, v.shape[1], q)]
    pts = torch.tensor((base + 0.002 * rng.standard_normal(base.shape)).astype(np.float32), device=dev())
    counts = torch.tensor([0, 1, 65], dtype=torch.int32, device=dev())
    d = model.ray_near_debug(verts, pts, counts, waves=waves)
    assert d['rays'].shape[1] == 128
    check_lists(d, [0, 1, 65], waves, 'points, %d waves' % waves)
    assert (d['lengths'][0] == 0).all() and d['lengths'][1, 1] == 0 and d['lengths'][2, 1] > 0
    _, e1 = model.winding_points(verts, pts, counts, flags_only=True)
    _, e2 = model.winding_points(verts, pts, counts, flags_only=True)
    assert torch.equal(e1, e2)
