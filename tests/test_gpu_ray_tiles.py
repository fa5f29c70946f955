"""The crossing walk's tiles (csrc/ray_winding.hip: ray_tiles_fill_kernel, ray_leaf_kernel): a leaf with c >= 64 rays has
c / 64 tiles and the last one carries the c % 64 left over as a second ray set of the same pass (set B); a leaf with fewer
than 64 rays has one tile.  Which pass a ray rides in must never change an answer, so every assertion here is EXACT, on
integers and flags: against float64 solid-angle sums computed here, against the reference's own flags in the golden files,
and against the block-major walk (option ray_pair_cap = 1), which has one ray set per pass.  The rays per (leaf, body) that
an input must have for a test to mean anything are asserted first, from tuch_ray_near_debug's bitmap."""
import numpy as np
import pytest
import torch

from helpers import golden, oracle_segments

pytestmark = pytest.mark.gpu

K_SHEAR = (np.float32(0.3217), np.float32(0.4331))     # csrc/ray_winding.hip: kShearX, kShearY (the ray is (kx, ky, 1))
K_BOX_RANGE = 16.0                                      # csrc/ray_winding.hip: kBoxRange


def dev():
    return torch.device('cuda:0')


def make_model(faces, segments=None):
    from tuch_amd.ops import ContactModel
    return ContactModel(np.asarray(faces), None, segments, None, None, device=dev())


def golden_model(g, with_segments=True):
    import golden_io as gio
    segs = gio.unpack_segments(g)
    return make_model(g['faces'], [(s['vidx'], list(s['bands'].values())) for s in segs.values()] if with_segments else None)


def winding_f64(points, verts, faces):
    """Winding numbers by float64 solid angles (van Oosterom & Strackee) of the float32 coordinates."""
    p = np.asarray(points, np.float64)[:, None, :]
    tri = np.asarray(verts, np.float64)[np.asarray(faces)]
    a, b, c = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
    na, nb, nc = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1), np.linalg.norm(c, axis=-1)
    num = np.einsum('qfi,qfi->qf', a, np.cross(b, c))
    den = na * nb * nc + (a * b).sum(-1) * nc + (a * c).sum(-1) * nb + (b * c).sum(-1) * na
    return (2.0 * np.arctan2(num, den)).sum(-1) / (4.0 * np.pi)


def integers(w):
    """Off the surface the winding number is an integer: a test input that leaves doubt about it is a broken test."""
    n = np.rint(w)
    assert np.abs(w - n).max() < 1e-3, np.abs(w - n).max()
    return n.astype(np.int64)


def exterior_of(n):
    return n.astype(np.float64) <= 0.99


def rays_per_leaf(d):
    """[B][L]: how many rays the near lists hold for every (body, leaf) -- the c of the tiling rule."""
    return np.unpackbits(d['bitmap'], axis=2, bitorder='little').sum(2).astype(np.int64)


def passes_of(c):
    """The tiling rule: c / 64 passes for a leaf with at least 64 rays, one for a leaf with fewer, none for none."""
    return np.where(c > 0, np.maximum(1, c // 64), 0)


PAIR_CAP = 16                                           # csrc/model.h: the default of option ray_pair_cap


def assert_both_walks_run(c, rays):
    """ray_tiles_fill_kernel walks a body block-major iff its listed pairs exceed ray_pair_cap x rays (the tiles then fit
    as well: at most pairs / 64 + one per leaf).  With the default every body of the input must fit, with ray_pair_cap = 1
    none may: otherwise a comparison of the two walks compares one walk with itself."""
    pairs = c.sum(1)
    assert (pairs <= PAIR_CAP * rays).all() and (pairs > rays).all(), (pairs, rays)


def leaf_strip_lengths(faces, num_verts):
    """Strip elements of every leaf, in the order the near lists number the leaves (preorder)."""
    from tuch_amd.ops import cluster_tree
    f = np.asarray(faces)
    t = cluster_tree(f, num_verts, leaf_faces=max(len(f) // 850, 32))     # csrc/model.hip: the model's leaf size
    nodes = t['nodes']
    return nodes[nodes[:, 5] < 0, 3].astype(np.int64), t


# ---- points on one ray ---------------------------------------------------------------------------------------------------
def point_triangle_distance(p, tri):
    """Distances [Q] of points [Q,3] to the nearest of the triangles [F,3,3] (Ericson, Real-Time Collision Detection 5.1.5)."""
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    p = p[:, None, :]
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide='ignore', invalid='ignore'):
        denom = va + vb + vc
        v, w = vb / denom, vc / denom
        near = a + ab * v[..., None] + ac * w[..., None]                       # the face's interior
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        near = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + (c - b) * t_bc[..., None], near)
        near = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + ac * t_ac[..., None], near)
        near = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + ab * t_ab[..., None], near)
    near = np.where(((d6 >= 0) & (d5 <= d6))[..., None], c, near)
    near = np.where(((d3 >= 0) & (d4 <= d3))[..., None], b, near)
    near = np.where(((d1 <= 0) & (d2 <= 0))[..., None], a, near)
    return np.linalg.norm(p - near, axis=-1).min(1)


def line_crossings(origin, d, tri):
    """Parameters t (sorted) at which the line origin + t d passes through the triangles [F,3,3] (Moeller & Trumbore)."""
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    h = np.cross(d[None], e2)
    det = (e1 * h).sum(-1)
    ok = np.abs(det) > 1e-12
    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    s = origin[None] - tri[:, 0]
    u = (s * h).sum(-1) * inv
    qv = np.cross(s, e1)
    v = (qv * d[None]).sum(-1) * inv
    t = (e2 * qv).sum(-1) * inv
    return np.sort(t[ok & (u >= 0) & (v >= 0) & (u + v <= 1)])


def points_on_one_ray(verts, faces, q):
    """q points on ONE line along the ray direction through the body, at least 1 mm apart and 1 mm off every face, spread from
    half a metre in front of the body to just before the line leaves it for good: every one of their rays still has the
    line's last crossing ahead, so the leaf of the face crossed there lists all q of them."""
    v = np.asarray(verts, np.float64)
    tri = v[np.asarray(faces)]
    d = np.array([K_SHEAR[0], K_SHEAR[1], 1.0], np.float64)
    origin = v.mean(0) + 0.013
    t_cross = line_crossings(origin, d, tri)
    assert len(t_cross) >= 2 and len(t_cross) % 2 == 0, t_cross           # the line goes through the closed body
    t = np.arange(t_cross[0] - 0.5, t_cross[-1] - 0.005, 0.001)           # |d| > 1: 1 mm in t is more than 1 mm apart
    pts = (origin[None] + t[:, None] * d[None]).astype(np.float32)
    t = t[point_triangle_distance(pts.astype(np.float64), tri) >= 1.0e-3]
    assert len(t) >= q, (len(t), q)
    t = t[np.unique(np.round(np.linspace(0, len(t) - 1, q)).astype(np.int64))]
    assert len(t) == q
    pts = (origin[None] + t[:, None] * d[None]).astype(np.float32)
    assert np.linalg.norm(np.diff(pts.astype(np.float64), axis=0), axis=-1).min() >= 1.0e-3
    return pts


@pytest.fixture(scope='module')
def small():
    return golden('small')


def points_results(model, verts, tp, tc):
    w, _ = model.winding_points(verts, tp, tc, flags_only=False)
    _, ext = model.winding_points(verts, tp, tc, flags_only=True)           # the flags of the crossing walk
    return w.cpu().numpy(), ext.cpu().numpy().astype(bool)


# ---- 1. set boundaries, points form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('q', [63, 64, 65, 127, 128, 129, 191, 192, 193])
def test_points_at_the_set_boundaries_equal_the_rounded_solid_angle_sums(small, q):
    """A leaf with exactly q rays: q = 63 one short tile; 64 one full; 65, 127 one pass with a set B of 1 / 63; 128 two full;
    129 a full tile and a pass with a set B of 1; 191, 192, 193 the same one tile further.  Body 1: q - 3 rays."""
    g = small
    v0, faces = g['verts'][0], g['faces']
    pts = points_on_one_ray(v0, faces, q)
    counts = np.array([q, q - 3], np.int32)
    verts = torch.tensor(np.stack([v0, v0]), device=dev())                  # the same body twice: the line is laid through it
    tp, tc = torch.tensor(np.stack([pts, pts]), device=dev()), torch.tensor(counts, device=dev())
    model = make_model(faces)
    c = rays_per_leaf(model.ray_near_debug(verts, tp, tc))
    assert (c[0] == q).any() and (c[1] == q - 3).any(), (q, c.max(1))       # an input that does not give that is a broken test
    assert c.max() <= q
    assert_both_walks_run(c, q)
    want = points_results(model, verts, tp, tc)
    ns = []
    for b in range(2):
        n = integers(want[0][b][:counts[b]].astype(np.float64))
        assert np.array_equal(n, integers(winding_f64(pts[:counts[b]], v0, faces)))
        assert np.array_equal(want[1][b][:counts[b]], exterior_of(n))
        ns.append(n)
    assert (ns[0] != 0).any() and (ns[0] == 0).any()                        # points on both sides of the surface
    model.set_option('ray_pair_cap', 1)                                     # the block-major walk: one ray set per pass
    _, got = model.winding_points(verts, tp, tc, flags_only=True)           # (w is the solid-angle path: not this kernel)
    got = got.cpu().numpy().astype(bool)
    for b in range(2):
        assert np.array_equal(got[b][:counts[b]], want[1][b][:counts[b]])


# ---- 2. vertex form with segments -------------------------------------------------------------------------------------------
def vertex_results(model, verts):
    plain = model.exterior_flags(verts, apply_segments=False)
    ext, w, _, seg_e = model.exterior_flags(verts, apply_segments=True, return_details=True)
    return plain, ext, w, seg_e


@pytest.mark.parametrize('tag', ['medium', 'full'])
def test_vertex_flags_and_segment_flags_equal_the_reference_and_the_block_major_walk(tag):
    """Three bodies whose leaves hold passes of every kind: a set B beside a single full tile (65 <= c <= 127) and beside the
    last of several (c >= 129).  Every vertex is asserted: no vertex of these fixtures has |w - 0.99| <= 1e-4."""
    g = golden(tag)
    assert (np.abs(g['winding'] - 0.99) <= 1e-4).sum() == 0
    idx = np.arange(3) % g['verts'].shape[0]
    verts = torch.tensor(g['verts'][idx], device=dev())
    model = golden_model(g)
    c = rays_per_leaf(model.ray_near_debug(verts))
    assert ((c >= 65) & (c <= 127)).any() and (c >= 129).any(), np.sort(c.reshape(-1))[-8:]
    assert_both_walks_run(c, verts.shape[1])
    leaf_major = model.ray_work(verts)['elements']
    want = vertex_results(model, verts)
    plain, ext, w, seg_e = (x.cpu().numpy() for x in want)
    plain, ext, seg_e = plain.astype(bool), ext.astype(bool), seg_e.astype(bool)
    assert np.array_equal(plain, ~(g['winding'][idx] > 0.99))
    assert np.array_equal(plain, w <= np.float32(0.99))
    assert np.array_equal(seg_e, g['segment_exterior'][idx].astype(bool))
    segs = oracle_segments(g)
    for b in range(3):
        expect, off = plain[b].copy(), 0
        for s in segs:
            expect[s.vidx[~seg_e[b][off:off + len(s.vidx)]]] = True
            off += len(s.vidx)
        assert np.array_equal(ext[b], expect)
    bare = golden_model(g, with_segments=False)                              # the walk without the per-segment counters
    bare_flags = bare.exterior_flags(verts, apply_segments=False)
    assert np.array_equal(bare_flags.cpu().numpy().astype(bool), plain)
    model.set_option('ray_pair_cap', 1)
    bare.set_option('ray_pair_cap', 1)
    assert model.ray_work(verts)['elements'] > leaf_major                    # block-major order walks more elements: it ran
    for a, b in zip(want, vertex_results(model, verts)):
        assert torch.equal(a, b)
    assert torch.equal(bare.exterior_flags(verts, apply_segments=False), bare_flags)


# ---- 3. tile accounting -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,nb', [('small', 9), ('full', 2)])
def test_passes_and_elements_follow_the_tiling_rule(tag, nb):
    """tuch_ray_work counts the passes and the strip elements they step through: a leaf with c rays is walked max(1, c / 64)
    times (never for c = 0).  9 bodies: one more than the grid's 8 columns."""
    g = golden(tag)
    verts = torch.tensor(g['verts'][np.arange(nb) % g['verts'].shape[0]], device=dev())
    model = make_model(g['faces'])
    c = rays_per_leaf(model.ray_near_debug(verts))
    lengths, _ = leaf_strip_lengths(g['faces'], g['verts'].shape[1])
    assert c.shape == (nb, len(lengths))
    passes = passes_of(c)
    assert ((c > 0) & (c < 64)).any()
    if tag == 'full':                                    # (the small body's leaves all hold fewer than 64 rays)
        assert ((c > 64) & (c < 128)).any() and ((c > 128) & (c % 64 != 0)).any()
    work = model.ray_work(verts)
    assert work['wavefronts'] == int(passes.sum())
    assert work['elements'] == int((passes * lengths[None, :]).sum())


# ---- 4. NaN and far origins in a set B --------------------------------------------------------------------------------------
def test_nan_and_far_origins_in_a_set_b_equal_the_block_major_walk(small):
    """100 points on one ray, two query blocks (64 + 36): the leaf the line leaves the body through holds all of them, one
    pass with 64 rays in set A and 36 in set B.
    Body 0: points 63 and 64 are NaN (the near test rejects nothing for a NaN ray: they are listed in every leaf).  A
    leaf's range in the pair list holds the listed lanes of block 0 and then those of block 1, or the other way round,
    whichever reserved first: with all of block 0 listed, set B is either block 1 (point 64 is its first lane) or the last
    36 lanes of block 0 (point 63 is its last lane).  Either way a NaN origin rides in a set B.
    Body 1: body and points 20 m off in x, beyond the range the boxes decide for: every origin, those of set B among them,
    is compared as NaN and passes every box.
    (The NaN is an ORIGIN here, not a corner of the mesh: the block-major walk tests every ray of a block against every leaf
    listed for the block, a ray outside a leaf's slabs included, and a triangle with a NaN corner can count for such a ray --
    with a NaN corner the two walks differ already before this file's tiling rule, by pairs the leaf-major walk never
    forms.)"""
    g = small
    v0, faces = g['verts'][0], g['faces']
    q = 100
    pts = points_on_one_ray(v0, faces, q)
    pts_nan = pts.copy()
    pts_nan[63:65] = np.nan
    shift = np.array([20.0, 0.0, 0.0], np.float32)
    assert np.abs((pts + shift)[:, 0] - K_SHEAR[0] * (pts + shift)[:, 2]).min() > K_BOX_RANGE
    verts = torch.tensor(np.stack([v0, v0 + shift]), device=dev())
    tp = torch.tensor(np.stack([pts_nan, pts + shift]), device=dev())
    counts = np.array([q, q - 3], np.int32)
    tc = torch.tensor(counts, device=dev())
    model = make_model(faces)
    listed = np.unpackbits(model.ray_near_debug(verts, tp, tc)['bitmap'], axis=2, bitorder='little').astype(bool)
    c = listed.sum(2)
    rides = listed[0][:, :65].all(1) & (c[0] > 64) & (c[0] < 128)              # all of block 0 and point 64, one pass with a set B
    assert rides.any(), c[0]
    assert ((c[1] > 64) & (c[1] < 128)).any(), c[1]
    assert_both_walks_run(c, q)
    _, want = model.winding_points(verts, tp, tc, flags_only=True)
    model.set_option('ray_pair_cap', 1)
    _, got = model.winding_points(verts, tp, tc, flags_only=True)
    for b in range(2):
        assert torch.equal(got[b][:counts[b]], want[b][:counts[b]])
    # the other 98 points of body 0, and the far body (the near body moved): the integers float64 finds
    want = want.cpu().numpy().astype(bool)
    real = ~np.isnan(pts_nan[:, 0])
    assert np.array_equal(want[0][:q][real], exterior_of(integers(winding_f64(pts[real], v0, faces))))
    n = integers(winding_f64((pts + shift)[:counts[1]], v0 + shift, faces))
    assert np.array_equal(want[1][:counts[1]], exterior_of(n))


# ---- 5. the vertex form with segments: far origins, and a NaN vertex ------------------------------------------------------------
def test_vertex_form_far_bodies_equal_the_reference_and_the_block_major_walk():
    """The medium bodies 20 m off in x: every vertex is a far origin (compared as NaN, it passes every box) and every element
    has the full box, in set A and set B alike, with the per-segment counters on.  The flags are those of the bodies where
    the fixture has them (every |w - 0.99| is far above what moving the body changes), and those of the block-major walk."""
    g = golden('medium')
    shift = np.array([20.0, 0.0, 0.0], np.float32)
    v = g['verts'] + shift
    assert np.abs(v[..., 0] - K_SHEAR[0] * v[..., 2]).min() > K_BOX_RANGE
    verts = torch.tensor(v, device=dev())
    model = golden_model(g)
    c = rays_per_leaf(model.ray_near_debug(verts))
    assert ((c >= 65) & (c <= 127)).any() and (c >= 129).any()
    assert_both_walks_run(c, verts.shape[1])
    want = vertex_results(model, verts)
    assert np.array_equal(want[0].cpu().numpy().astype(bool), ~(g['winding'] > 0.99))
    assert np.array_equal(want[3].cpu().numpy().astype(bool), g['segment_exterior'].astype(bool))
    model.set_option('ray_pair_cap', 1)
    for a, b in zip(want, vertex_results(model, verts)):
        assert torch.equal(a, b)


def test_vertex_form_with_a_nan_vertex_equals_the_block_major_walk_where_the_two_form_the_same_pairs():
    """Body 0 of the medium fixture with one NaN vertex, per-segment counters on.  The NaN vertex is a ray the near test
    lists in EVERY leaf, so it rides in the passes of leaves with a set B (which set it lands in is the order of two atomic
    reservations and cannot be placed).  Its triangles are NaN elements of the leaves that hold them.
    What can be compared: the block-major walk tests every ray of a query block against every leaf listed for the block,
    also a ray outside that leaf's slabs; a clean triangle counts nothing for such a ray, a triangle with a NaN corner can
    (min / max drop the NaN edge functions).  So the two walks must agree for the vertices of every query block whose list
    holds no leaf with the NaN vertex in its strip -- the block of the NaN vertex itself lists every leaf and is left out --
    and for the clean bodies beside it."""
    g = golden('medium')
    bad = 57
    v = g['verts'].copy()
    v[0, bad] = np.nan
    verts = torch.tensor(v, device=dev())
    model = golden_model(g)
    _, tree = leaf_strip_lengths(g['faces'], v.shape[1])
    nodes = tree['nodes']
    leaf_nodes = np.nonzero(nodes[:, 5] < 0)[0]
    touched = np.array([bad in tree['vidx'][nodes[n, 2]:nodes[n, 2] + nodes[n, 3]] for n in leaf_nodes])
    d = model.ray_near_debug(verts)
    listed = np.unpackbits(d['bitmap'], axis=2, bitorder='little').astype(bool)          # [B][L][slots]
    assert listed.shape[1] == len(leaf_nodes) and touched.any()
    c = listed.sum(2)
    pos = model.tree_positions()
    assert listed[0][:, pos[bad]].all()                                       # the NaN ray is listed in every leaf ...
    assert ((c[0] >= 65) & (c[0] % 64 != 0)).any()                            # ... so also in leaves whose last pass has a set B
    assert_both_walks_run(c, v.shape[1])
    blocks = listed.shape[2] // 64
    dirty = np.array([listed[0][touched][:, qb * 64:(qb + 1) * 64].any() for qb in range(blocks)])
    comparable = ~dirty[pos // 64]
    assert dirty[pos[bad] // 64] and comparable.sum() > v.shape[1] // 4, comparable.sum()
    want = model.exterior_flags(verts, apply_segments=False).cpu().numpy()
    model.set_option('ray_pair_cap', 1)
    got = model.exterior_flags(verts, apply_segments=False).cpu().numpy()
    assert np.array_equal(got[0][comparable], want[0][comparable])
    assert np.array_equal(got[1:], want[1:])
    assert np.array_equal(want[1:].astype(bool), ~(g['winding'][1:] > 0.99))
