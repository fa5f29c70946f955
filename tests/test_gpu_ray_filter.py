"""The crossing walk's box filter (csrc/ray_winding.hip: ray_elem_box, ray_filter, ray_exact): a (ray, element) pair is
tested exactly only if the ray's origin lies in the padded 2-D box of the element's projected triangle.  The filter must
never change an answer, so every assertion here is EXACT, on integers and flags: against the reference's own flags in the
golden files, against the library's independent solid-angle path, and against float64 solid-angle sums computed here."""
import numpy as np
import pytest
import torch

from helpers import golden, oracle_segments

pytestmark = pytest.mark.gpu

K_SHEAR = (np.float32(0.3217), np.float32(0.4331))     # csrc/ray_winding.hip: kShearX, kShearY (the ray is (kx, ky, 1))


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


def off_surface_points(verts, faces, q, seed, dist=1e-3):
    """q points 1 mm off the surface: face centroids moved along the face normal, inwards and outwards in turn."""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces)[rng.integers(0, len(faces), q)]
    a, b, c = verts[f[:, 0]].astype(np.float64), verts[f[:, 1]].astype(np.float64), verts[f[:, 2]].astype(np.float64)
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    side = np.where(np.arange(q) % 2 == 0, 1.0, -1.0)[:, None]
    return ((a + b + c) / 3.0 + dist * side * n).astype(np.float32)


# ---- the fixtures: the reference's own flags, and the library's solid-angle path ----------------------------------------
@pytest.mark.parametrize('tag', ['small', 'ico_small', 'medium'])
def test_vertex_flags_equal_the_reference_and_the_solid_angle_path(tag):
    """Every vertex is asserted: no vertex of these fixtures has |w - 0.99| <= 1e-4."""
    g = golden(tag)
    assert (np.abs(g['winding'] - 0.99) <= 1e-4).sum() == 0
    verts = torch.tensor(g['verts'], device=dev())
    model = golden_model(g)
    assert model.ray_work(verts)['elements'] > 0                    # the crossing walk is what runs
    plain = model.exterior_flags(verts, apply_segments=False).cpu().numpy().astype(bool)
    ext, w, _, seg_e = model.exterior_flags(verts, apply_segments=True, return_details=True)
    ext, w, seg_e = ext.cpu().numpy().astype(bool), w.cpu().numpy(), seg_e.cpu().numpy().astype(bool)
    assert np.array_equal(plain, ~(g['winding'] > 0.99))
    assert np.array_equal(plain, w <= np.float32(0.99))
    assert np.array_equal(seg_e, g['segment_exterior'].astype(bool))
    segs = oracle_segments(g)
    for b in range(plain.shape[0]):
        expect, off = plain[b].copy(), 0
        for s in segs:
            expect[s.vidx[~seg_e[b][off:off + len(s.vidx)]]] = True
            off += len(s.vidx)
        assert np.array_equal(ext[b], expect)
    bare = golden_model(g, with_segments=False)                      # the walk without the per-segment counters
    assert np.array_equal(bare.exterior_flags(verts, apply_segments=False).cpu().numpy().astype(bool), plain)


# ---- the points form ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    g = golden('small')
    return g, golden_model(g, with_segments=False), torch.tensor(g['verts'], device=dev())


@pytest.mark.parametrize('q', [1, 63, 64, 65, 129])
def test_points_flags_equal_the_rounded_solid_angle_sums(small, q):
    g, model, verts = small
    nb = verts.shape[0]
    pts = np.stack([off_surface_points(g['verts'][b], g['faces'], q, 11 + b) for b in range(nb)])
    counts = np.array([max(q - 3 * b, 1) for b in range(nb)], np.int32)     # body 1: the last block is partial
    tp, tc = torch.tensor(pts, device=dev()), torch.tensor(counts, device=dev())
    w, _ = model.winding_points(verts, tp, tc, flags_only=False)
    _, ext = model.winding_points(verts, tp, tc, flags_only=True)
    w, ext = w.cpu().numpy(), ext.cpu().numpy().astype(bool)
    for b in range(nb):
        n = integers(w[b][:counts[b]].astype(np.float64))
        assert np.array_equal(ext[b][:counts[b]], exterior_of(n))
        assert np.array_equal(n, integers(winding_f64(pts[b][:counts[b]], g['verts'][b], g['faces'])))
        assert 0 < n.sum() < counts[b] or q == 1                     # points on both sides of the surface


def test_queue_fills_sixty_four_at_a_time(small):
    """129 points on ONE ray through the body: every lane of a tile passes the same boxes, so the queue takes 64 entries per
    element and has to be emptied between two elements (the ring holds 128)."""
    g, model, verts = small
    v0 = g['verts'][0].astype(np.float64)
    centre = v0.mean(0)
    d = np.array([K_SHEAR[0], K_SHEAR[1], 1.0], np.float64)
    reach = np.linalg.norm(v0 - centre, axis=-1).max() * 1.5
    t = np.linspace(-reach, reach * 0.25, 129)
    pts = (centre[None] + 0.013 + t[:, None] * d[None]).astype(np.float32)
    n = integers(winding_f64(pts, g['verts'][0], g['faces']))
    assert (n != 0).sum() > 8 and (n == 0).sum() > 8
    tp = torch.tensor(np.stack([pts] * verts.shape[0]), device=dev())
    _, ext = model.winding_points(verts[:1].expand(verts.shape[0], -1, -1).contiguous(), tp, flags_only=True)
    for b in range(verts.shape[0]):
        assert np.array_equal(ext[b].cpu().numpy().astype(bool), exterior_of(n))


# ---- exact ties and the filter's boundary -------------------------------------------------------------------------------
def tie_mesh():
    """A prism over a star-shaped polygon whose bottom lies in z = 0 (there the sheared coordinates are the plain ones),
    fanned around C0 = (kx, ky, 0), and a small tetrahedron with an edge ALONG the ray direction (two of its faces are
    edge-on: their projections are segments).  P(k) = 2^k (kx, ky, 0):
      C0 = P(0)                      a vertex of the bottom (six triangles around it);
      E1, E2 = P(-2) +- (2^-5, -2^-6) an edge of the bottom's rim (shared with a wall) whose midpoint is exactly P(-2);
      V2, V3                          (C0, V2, V3) has the corner (max x, max y) of its bounding box at P(2), outside it."""
    kx, ky = K_SHEAR
    f32 = np.float32
    p = lambda k: (f32(2.0 ** k) * kx, f32(2.0 ** k) * ky)
    e1 = (p(-2)[0] + f32(2 ** -5), p(-2)[1] - f32(2 ** -6))
    e2 = (p(-2)[0] - f32(2 ** -5), p(-2)[1] + f32(2 ** -6))
    assert (e1[0] + e2[0]) / f32(2) == p(-2)[0] and (e1[1] + e2[1]) / f32(2) == p(-2)[1]
    assert e1[0] - p(-2)[0] == -(e2[0] - p(-2)[0]) and e1[1] - p(-2)[1] == -(e2[1] - p(-2)[1])
    rim = [e2, e1, (1.5, -0.5), (p(2)[0], 0.5), (0.5, p(2)[1]), (-1.0, 1.2)]      # counter-clockwise around C0
    n = len(rim)
    verts = [(kx, ky, 0.0)] + [(x, y, 0.0) for x, y in rim] + [(kx, ky, 1.0)] + [(x, y, 1.0) for x, y in rim]
    bot, top = 0, n + 1
    faces = []
    for i in range(n):
        a, b = 1 + i, 1 + (i + 1) % n
        faces += [(bot, b, a), (top, top + a, top + b), (a, b, top + b), (a, top + b, top + a)]
    # the tetrahedron: T0 at the origin, T1 = 2^-4 (kx, ky, 1): both project to (0, 0) exactly
    t0 = len(verts)
    verts += [(0.0, 0.0, 0.0), (f32(2 ** -4) * kx, f32(2 ** -4) * ky, 2 ** -4), (-0.1, 0.0, 0.0), (0.0, -0.1, 0.02)]
    tet = [(t0, t0 + 1, t0 + 2), (t0, t0 + 3, t0 + 1), (t0, t0 + 2, t0 + 3), (t0 + 1, t0 + 3, t0 + 2)]
    verts = np.asarray(verts, np.float32)
    vol = sum(np.dot(verts[a].astype(np.float64), np.cross(verts[b].astype(np.float64), verts[c].astype(np.float64)))
              for a, b, c in tet)
    faces += tet if vol > 0 else [(a, c, b) for a, b, c in tet]
    faces = np.asarray(faces, np.int64)
    inside = winding_f64(np.array([[0.3, 0.5, 0.5], [-0.02, -0.02, 0.005]], np.float32), verts, faces)
    assert np.array_equal(np.rint(inside), [1, 1])                   # closed, outward oriented, both parts
    return verts, faces


def tie_queries():
    kx, ky = K_SHEAR
    q = [(0.0, 0.0, -(2.0 ** k)) for k in (-3, -2, -1, 0, 1, 2, 3)]   # sheared: exactly P(k) -- P(-2): rim edge, P(0): vertex,
    #                                                                   P(2): box corner; the others generic, on the line
    q += [(-kx * np.float32(2 ** -3), -ky * np.float32(2 ** -3), -(2.0 ** -3))]   # sheared (0, 0): along the tetrahedron's edge
    q += [(0.3, 0.5, 0.5), (kx, ky, 0.5), (0.3, 0.5, -0.5), (-0.02, -0.02, 0.005)]  # inside / above C0 / below / in the tetrahedron
    return np.asarray(q, np.float32)


@pytest.mark.parametrize('flip', [False, True])
def test_rays_through_vertices_edges_and_box_corners(flip):
    """Each ray passes exactly through a vertex, along an edge or through a box corner; with the faces reversed (flip) a
    crossing counted twice shows as +1 where, outward oriented, it would be a -1 the flags cannot see."""
    verts, faces = tie_mesh()
    if flip:
        faces = faces[:, ::-1].copy()
    pts = tie_queries()
    n = integers(winding_f64(pts, verts, faces))
    assert np.array_equal(n[:8], np.zeros(8, np.int64))
    model = make_model(faces)
    tv = torch.tensor(verts[None], device=dev())
    assert model.ray_work(tv)['elements'] > 0
    _, ext = model.winding_points(tv, torch.tensor(pts[None], device=dev()), flags_only=True)
    assert np.array_equal(ext[0].cpu().numpy().astype(bool), exterior_of(n))
    # the same rays for a body standing elsewhere (sheared coordinates no longer those of the construction: generic, but
    # close to every tie), and far beyond the range the boxes decide for
    for shift in ([0.37, -1.21, 2.5], [700.0, -300.0, 90.0]):
        s = np.asarray(shift, np.float32)
        v2, p2 = verts + s, pts + s                                   # float32 sums: the oracle sees the rounded coordinates
        n2 = integers(winding_f64(p2, v2, faces))
        assert np.array_equal(n2, n)
        _, e2 = model.winding_points(torch.tensor(v2[None], device=dev()), torch.tensor(p2[None], device=dev()), flags_only=True)
        assert np.array_equal(e2[0].cpu().numpy().astype(bool), exterior_of(n2))


# ---- overflow path, determinism -----------------------------------------------------------------------------------------
def test_block_major_fallback_takes_the_same_walk():
    g = golden('small')
    model = golden_model(g)
    verts = torch.tensor(g['verts'], device=dev())
    pts = torch.tensor(np.stack([off_surface_points(g['verts'][b], g['faces'], 129, 5 + b) for b in range(verts.shape[0])]),
                       device=dev())
    want = (model.exterior_flags(verts, apply_segments=False), model.exterior_flags(verts, apply_segments=True),
            model.winding_points(verts, pts, flags_only=True)[1])
    work = model.ray_work(verts)['elements']
    model.set_option('ray_pair_cap', 1)
    got = (model.exterior_flags(verts, apply_segments=False), model.exterior_flags(verts, apply_segments=True),
           model.winding_points(verts, pts, flags_only=True)[1])
    assert model.ray_work(verts)['elements'] > work                  # block-major order walks more elements: it ran
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert np.array_equal(got[0].cpu().numpy().astype(bool), ~(g['winding'] > 0.99))


def test_flags_and_segment_verdicts_are_deterministic_also_under_a_graph():
    g = golden('medium')
    model = golden_model(g)
    verts = torch.tensor(g['verts'], device=dev())
    first = model.exterior_flags(verts, apply_segments=True, return_details=True)
    again = model.exterior_flags(verts, apply_segments=True, return_details=True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[3], again[3])
    static_v = verts.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                       # warm-up off the capture
        model.exterior_flags(static_v, apply_segments=True, return_details=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.exterior_flags(static_v, apply_segments=True, return_details=True)
    out[0].fill_(7)
    out[3].fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], first[0]) and torch.equal(out[3], first[3])


def test_no_guard_word_between_the_workspace_regions_is_touched():
    """The boxes are a workspace region of their own (tuch_ws_take): with the canary on, nothing writes behind any region."""
    g = golden('small')
    model = golden_model(g)
    model.set_option('canary', 1)
    verts = torch.tensor(g['verts'], device=dev())
    pts = torch.tensor(np.stack([off_surface_points(g['verts'][b], g['faces'], 65, 5 + b) for b in range(verts.shape[0])]),
                       device=dev())
    model.canary_hits(reset=True)
    ext = model.exterior_flags(verts, apply_segments=True)
    model.winding_points(verts, pts, flags_only=True)
    assert model.canary_hits() == 0
    assert np.array_equal(model.exterior_flags(verts, apply_segments=False).cpu().numpy().astype(bool), ~(g['winding'] > 0.99))
    assert ext.shape == verts.shape[:2]
