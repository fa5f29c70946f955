"""GPU: the mesh renderer (csrc/render.hip, tuch_amd/render.py, tuch_amd/utils/renderer.py) against the numpy rasterisers
of tests/render_cases.py.

Exact cases (tie rules, watertightness, visibility, clipping) use coordinates that are exactly representable (f = 1,
t = (0, 0, 1), vertices at z = 0 on integers and half-integers) and the integer reference with NO exclusions.

Bodies are compared with the float64, unsnapped reference off two sets of pixels, and only these: (a) centre within
1/128 px of a projected edge (four times the 1/512 px snapping error), (b) the reference's two nearest surfaces within
1e-5 relative in depth.  The excluded pixels may not exceed 2 % of the image and 10 % of the covered pixels per view
(the reference alone: 0.8 % / 4.6 % at V = 122 @ 64^2, 0.8 % / 4.7 % at V = 226 @ 96^2, 1.3 % / 8.3 % at full size, rest
poses).  Elsewhere face and coverage are identical, every image channel lies within 1/255 of the float64 shading (a
condition: the pictures end as 8-bit), and depth within DEPTH_RTOL.

DEPTH_RTOL = 4 x the observed maximum (logged through helpers.report_value, written next to the bound below).  Depth and
the shading are interpolated with the barycentrics of the UNSNAPPED projections; with the snapped ones a face seen at a
grazing angle moved depth by 3.1e-4 relative and a channel by 8.6e-3 (V = 226 @ 96^2, measured on the device).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import render_cases as rc
from helpers import report, report_value

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# depth off the excluded set, relative to float64: the largest value observed on the device over the three body cases
# (2.4e-7 at V = 122 @ 64^2, 7.6e-7 at V = 226 @ 96^2, 2.6e-7 at V = 6890 @ 224^2; image channels: 3.3e-6, 1.0e-5, 1.2e-5)
OBSERVED_DEPTH = 7.615e-7
DEPTH_RTOL = 4 * OBSERVED_DEPTH
IMAGE_ATOL = 1.0 / 255
CAP_IMAGE, CAP_COVERED = 0.02, 0.10


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype, device=DEV)


def renderer(faces, res, f=1.0, c=(0.0, 0.0)):
    from tuch_amd.render import MeshRenderer
    return MeshRenderer(np.asarray(faces), img_res=res, focal_length=f, camera_center=c)


def render(faces, verts, res, t=(0.0, 0.0, 1.0), f=1.0, c=(0.0, 0.0), views=('front',), **kw):
    """verts [V,3] or [B,V,3]; t [3] or [B,3] -> numpy dict with the batch axis kept."""
    verts = np.asarray(verts, np.float32)
    verts = verts[None] if verts.ndim == 2 else verts
    t = np.broadcast_to(np.asarray(t, np.float32), (verts.shape[0], 3))
    out = renderer(faces, res, f, c).render(dev(verts), dev(t), views=views, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def flat(points, z=0.0):
    """2-D points -> vertices at depth z (t = (0, 0, 1), f = 1: pixel coordinates are x / (1 + z))."""
    p = np.asarray(points, np.float64)
    return np.concatenate([p, np.full((len(p), 1), z)], 1).astype(np.float32)


def reference(faces, verts, res, t=(0.0, 0.0, 1.0), f=1.0, c=(0.0, 0.0), view='front'):
    from tuch_amd.render import VIEWS
    h, w = (res, res) if np.isscalar(res) else res
    return rc.integer_raster(verts, faces, VIEWS[view], t, f, c[0], c[1], h, w)


def assert_exact(out, b, w, face, depth, what):
    assert np.array_equal(out['face'][b, w], face), what
    assert np.array_equal(out['depth'][b, w] > 0, face >= 0), what
    cov = face >= 0
    if cov.any():
        # float32: the weights, the reciprocals and three terms, <= ten roundings of 6e-8
        assert np.allclose(out['depth'][b, w][cov], depth[cov], rtol=2e-6, atol=0), what
    assert np.all(out['image'][b, w][~cov] == 1.0), what


# ------------------------------------------------------------------------------------------------ 1. tie rules
TIE_TRIANGLES = {
    # the hypotenuse x + y = 13 runs through pixel centres, the corner (2.5, 2.5) is a centre, two edges lie ON centres
    'edges_on_centres': [(2.5, 2.5), (10.5, 2.5), (2.5, 10.5)],
    # integer corners: edges pass through centres at half-integers
    'integer_corners': [(3, 3), (12, 4), (5, 11)],
    'vertex_on_centre': [(8.5, 1.5), (14.5, 13.5), (1.5, 9.5)],
    'horizontal_bottom': [(2.5, 12.5), (13.5, 12.5), (7.5, 3.5)],
}


@pytest.mark.parametrize('name', sorted(TIE_TRIANGLES))
@pytest.mark.parametrize('winding', [(0, 1, 2), (0, 2, 1), (1, 2, 0)])
def test_tie_rules_exactly(name, winding):
    verts = flat(TIE_TRIANGLES[name])
    faces = np.array([winding])
    face, depth = reference(faces, verts, 16)
    # the reference itself does not depend on the winding, and ties do occur in these cases
    assert np.array_equal(face, reference(np.array([[0, 1, 2]]), verts, 16)[0])
    out = render(faces, verts, 16)
    assert 20 < (face >= 0).sum() < 200
    assert_exact(out, 0, 0, face, depth, (name, winding))


# ------------------------------------------------------------------------------------------------ 2. watertightness
def _csr_batch(all_faces, num_verts):
    from tuch_amd import ops
    tabs = [ops.vertex_face_table(f, num_verts) for f in all_faces]
    return (dev(np.stack([t[0] for t in tabs]), torch.int32), dev(np.stack([t[1] for t in tabs]), torch.int32),
            dev(np.stack(all_faces), torch.int32))


def _owners(verts, tris, res):
    """Every triangle rendered alone (F = 1 meshes): masks pairwise disjoint -> owner map [H,W] (-1 = nobody)."""
    owner = np.full((res, res), -1, np.int64)
    for k, tri in enumerate(tris):
        m = render(np.array([tri]), verts, res)['face'][0, 0] >= 0
        assert m.any() and not (m & (owner >= 0)).any(), ('two triangles own a pixel', k)
        owner[m] = k
    return owner


def _check_every_order(verts, tris, res, what):
    from tuch_amd import ops
    tris = np.asarray(tris)
    owner = _owners(verts, tris, res)
    perms = list(itertools.permutations(range(len(tris))))
    all_faces = []
    for n, perm in enumerate(perms):
        f = tris[list(perm)].copy()
        for k in range(len(f)):                       # windings vary with the permutation
            if (n >> k) & 1:
                f[k] = f[k][::-1]
        all_faces.append(f)
    off, ids, faces = _csr_batch(all_faces, len(verts))
    v, t, rot = dev(verts[None]), dev([[0.0, 0.0, 1.0]]), dev(np.eye(3)[None])
    got = torch.stack([ops.render_mesh(v, faces[n], (off[n], ids[n]), t, rot, 1.0, 0.0, 0.0, res, res)['face'][0, 0]
                       for n in range(len(perms))]).cpu().numpy()
    for n, perm in enumerate(perms):
        orig = np.where(got[n] >= 0, np.asarray(perm)[np.maximum(got[n], 0)], -1)
        assert np.array_equal(orig, owner), (what, perm)
    # the union is convex here: the outline rendered as ONE polygon fan has the same mask (no hole along shared edges)
    return owner


def test_watertight_quad_in_both_orders():
    # the diagonal (2.5, 2.5) - (12.5, 12.5) runs through eleven pixel centres
    verts = flat([(2.5, 2.5), (12.5, 2.5), (12.5, 12.5), (2.5, 12.5)])
    owner = _check_every_order(verts, [(0, 1, 2), (0, 2, 3)], 16, 'quad')
    # a 10 x 10 px square with corners on centres: top and left edges in, bottom and right out
    want = np.zeros((16, 16), bool)
    want[2:12, 2:12] = True
    assert np.array_equal(owner >= 0, want)
    assert len(set(owner[np.arange(2, 12), np.arange(2, 12)])) == 1           # the diagonal's centres: one owner


def test_watertight_fan_in_every_order():
    # six triangles around (8.5, 8.5), a pixel centre; spokes through centres (horizontal, vertical, diagonal) and not
    rim = [(14.5, 8.5), (12.5, 14.5), (8.5, 15.5), (2.5, 12.5), (1.5, 3.5), (9.5, 1.5)]
    verts = flat([(8.5, 8.5)] + rim)
    tris = [(0, 1 + k, 1 + (k + 1) % 6) for k in range(6)]
    owner = _check_every_order(verts, tris, 18, 'fan')
    assert owner[8, 8] >= 0                                                   # the hub belongs to exactly one of the six
    face, _ = reference(np.asarray(tris), verts, 18)
    assert np.array_equal(face, owner)


# ------------------------------------------------------------------------------------------------ 3. visibility
@pytest.mark.parametrize('order', [(0, 1), (1, 0)])
def test_nearer_surface_wins_in_both_face_orders(order):
    near = flat([(2.5, 2.5), (13.5, 3.5), (4.5, 12.5)], z=0.0)
    far = flat([(6.0, 4.0), (30.0, 8.0), (10.0, 28.0)], z=1.0)                # projects to half of these coordinates
    verts = np.concatenate([near, far])
    tris = np.array([(0, 1, 2), (3, 4, 5)])[list(order)]
    face, depth = reference(tris, verts, 16)
    out = render(tris, verts, 16)
    assert_exact(out, 0, 0, face, depth, order)
    near_id = order.index(0)
    alone = render(np.array([(0, 1, 2)]), verts, 16)['face'][0, 0] >= 0
    assert np.all(out['face'][0, 0][alone] == near_id) and (out['face'][0, 0] == 1 - near_id).any()
    assert set(np.unique(np.round(out['depth'][0, 0], 4))) == {0.0, 1.0, 2.0}


def test_smaller_face_id_wins_at_equal_depth():
    tri = [(2.5, 2.5), (13.5, 3.5), (4.5, 12.5)]
    verts = np.concatenate([flat(tri), flat(tri)])
    for faces in ([(0, 1, 2), (0, 1, 2)], [(3, 4, 5), (0, 1, 2)], [(0, 1, 2), (3, 4, 5), (0, 1, 2)]):
        out = render(np.array(faces), verts, 16)
        assert set(np.unique(out['face'])) == {-1, 0}, faces


# ------------------------------------------------------------------------------------------------ 4. robustness
def test_broken_triangles_are_dropped_and_do_not_disturb_the_batch():
    faces = np.arange(15).reshape(5, 3)
    good = np.concatenate([flat([(1.5 + 2 * k, 1.5), (6.5 + 2 * k, 2.5 + k), (2.5 + k, 9.5)], z=0.1 * k) for k in range(5)])
    bad = np.concatenate([
        flat([(10.5, 4.5), (22.5, 6.5), (12.5, 25.0)]),                       # partly outside: clipped
        flat([(-30.0, -4.0), (-20.0, -6.0), (-25.0, -25.0)]),                 # wholly outside
        np.array([(2, 2, 0), (9, 3, 0), (4, 9, -1.5)], np.float32),           # a corner behind the camera (p.z = -0.5)
        flat([(3.5, 3.5), (6.5, 6.5), (9.5, 9.5)]),                           # zero area
        np.array([(3, 3, 0), (9, 4, 0), (np.nan, 8, 0)], np.float32)])        # a NaN corner
    both = render(faces, np.stack([good, bad]), 16)
    alone = render(faces, good, 16)
    for k in ('face', 'depth', 'image'):
        assert np.array_equal(both[k][0], alone[k][0]), k
    face, depth = reference(faces, good, 16)
    assert_exact(both, 0, 0, face, depth, 'good body')
    face, depth = reference(faces, bad, 16)
    assert set(np.unique(face)) == {-1, 0} and (face == 0).sum() > 10
    assert_exact(both, 1, 0, face, depth, 'broken body')
    assert np.isfinite(both['image']).all()
    with_near = np.array([(2, 2, 0), (9, 3, 0), (4, 9, -0.9995)], np.float32)  # p.z = 5e-4 <= near
    assert (render(np.array([[0, 1, 2]]), with_near, 16)['face'] == -1).all()


def test_a_full_frame_triangle_is_spread_over_the_wavefront():
    verts = flat([(-20.0, -10.0), (600.0, -10.0), (-20.0, 700.0)])
    faces = np.array([[0, 1, 2]])
    face, depth = reference(faces, verts, 256)
    assert (face == 0).all()
    out = render(faces, verts, 256)
    assert_exact(out, 0, 0, face, depth, 'full frame')
    # a rectangular image, a box that needs both walks, off-centre principal point
    verts = flat([(1.5, 1.5), (37.5, 2.5), (4.5, 20.5), (30.5, 10.5), (33.5, 11.5), (31.5, 13.5)])
    faces = np.array([[0, 1, 2], [3, 4, 5]])
    face, depth = reference(faces, verts, (24, 40), c=(0.5, -0.25))
    out = render(faces, verts, (24, 40), c=(0.5, -0.25))
    assert_exact(out, 0, 0, face, depth, 'rectangular')


# ------------------------------------------------------------------------------------------------ 5. / 6. bodies
VIEW_NAMES = ('front', 'rot2', 'rot3')
T_Z = 5.0


@functools.lru_cache(maxsize=None)
def body_case(rings, segs, res):
    """Posed vertices from SMPL.forward on the device, the device's rendering of all views and the float64 references,
    computed once and shared.  Small bodies: through_pose(2, 7) + random_poses(2, 3); full size: through_pose(1, 7)."""
    from synthetic import make_body, random_poses, through_pose
    from tuch_amd.models.smpl import SMPL
    from tuch_amd.render import VIEWS, MeshRenderer
    full = rings == 84
    body = make_body(rings, segs, with_geodesics=False)
    parts = [through_pose(1, 7)] if full else [through_pose(2, 7), random_poses(2, 3)]
    bp, go, be = [dev(np.concatenate([np.asarray(p[k], np.float32) for p in parts])) for k in range(3)]
    verts = SMPL(model_data=body).to(DEV)(betas=be, body_pose=bp, global_orient=go).vertices.detach().contiguous()
    f = 0.8 * res * T_Z / float(np.ptp(body.v_template, 0).max())            # the body fills about 80 % of the frame
    t = np.tile(np.float32([0.02, -0.03, T_Z]), (verts.shape[0], 1))
    views = VIEW_NAMES[:1] if full else VIEW_NAMES
    v_np = verts.cpu().numpy()
    # smooth vertex colours for half of the bodies, the default albedo for the others
    colors = np.full(v_np.shape, 230, np.uint8)
    colors[::2] = np.clip(128 + 400 * (v_np[::2] - v_np[::2].mean(1, keepdims=True)), 0, 255).astype(np.uint8)
    r = MeshRenderer(body.faces, img_res=res, focal_length=f)
    out = r.render(verts, dev(t), views=views, colors=dev(colors, torch.uint8))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    refs = {(b, name): rc.float_raster(v_np[b], body.faces, VIEWS[name], t[b], f, res // 2, res // 2, res, res, colors=colors[b])
            for b in range(len(v_np)) for name in views}
    return {'body': body, 'verts': verts, 'verts_np': v_np, 't': t, 'f': f, 'views': views, 'out': out, 'refs': refs, 'renderer': r}


def check_against_float64(case, res, what):
    """face and coverage identical, depth within DEPTH_RTOL = 3.0e-6 (4 x the observed 7.6e-7), image within 1/255 (observed
    1.2e-5), all off the excluded pixels, whose share stays under the caps."""
    worst_depth = worst_image = 0.0
    for (b, name), ref in case['refs'].items():
        w = case['views'].index(name)
        ex, cov = rc.excluded(ref), ref['face'] >= 0
        share_img, share_cov = ex.mean(), (ex & cov).sum() / cov.sum()
        report_value('%s body %d %s: excluded share of the image' % (what, b, name), share_img)
        report_value('%s body %d %s: excluded share of the covered pixels' % (what, b, name), share_cov)
        assert cov.mean() > 0.05 and share_img <= CAP_IMAGE and share_cov <= CAP_COVERED, (what, b, name, share_img, share_cov)
        keep = ~ex
        got = {k: case['out'][k][b, w] for k in ('face', 'depth', 'image')}
        wrong = (got['face'] != ref['face']) & keep
        assert not wrong.any(), (what, b, name, int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
        assert np.array_equal((got['depth'] > 0)[keep], cov[keep])
        # everywhere, excluded pixels included: a face id is a face of the mesh, depth > 0 exactly on covered pixels
        assert got['face'].min() >= -1 and got['face'].max() < case['body'].num_faces
        assert np.array_equal(got['depth'] > 0, got['face'] >= 0)
        on = keep & cov
        worst_depth = max(worst_depth, float((np.abs(got['depth'][on] - ref['depth'][on]) / ref['depth'][on]).max()))
        worst_image = max(worst_image, float(np.abs(got['image'][keep] - ref['image'][keep]).max()))
    report_value('%s: max relative depth error off the excluded set (bound %.1e)' % (what, DEPTH_RTOL), worst_depth)
    report_value('%s: max image channel error off the excluded set (bound 1/255)' % what, worst_image)
    assert worst_depth <= DEPTH_RTOL, (what, worst_depth)
    assert worst_image <= IMAGE_ATOL, (what, worst_image)


@pytest.mark.parametrize('rings,segs,res', [(10, 12, 64), (14, 16, 96)])
def test_bodies_against_the_float64_rasteriser(rings, segs, res):
    case = body_case(rings, segs, res)
    assert case['verts'].shape[1] == {10: 122, 14: 226}[rings]
    check_against_float64(case, res, 'V=%d @ %d' % (case['verts'].shape[1], res))
    # the forearm through the trunk of body 0 shows inner faces: no back-face culling
    ref = case['refs'][(0, 'front')]
    assert (ref['face'] >= 0).sum() > 0


def test_full_size_body_and_the_projects_camera():
    from tuch_amd.utils.geometry import perspective_projection
    res = 224
    case = body_case(84, 82, res)
    assert case['verts'].shape[1] == 6890
    check_against_float64(case, res, 'V=6890 @ 224')
    mask = case['out']['depth'][0, 0] > 0
    uv = perspective_projection(case['verts'][:1], torch.eye(3, device=DEV)[None], dev(case['t'][:1]), case['f'],
                                dev([[res // 2, res // 2]]))[0].cpu().numpy()
    col, row = np.floor(uv[:, 0]).astype(int), np.floor(uv[:, 1]).astype(int)
    assert col.min() >= 1 and row.min() >= 1 and col.max() < res - 1 and row.max() < res - 1
    dilated = np.zeros_like(mask)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            dilated[1:-1, 1:-1] |= mask[1 + dr:res - 1 + dr, 1 + dc:res - 1 + dc]
    assert dilated[row, col].all()
    rows, cols = np.nonzero(mask)
    assert abs(rows.min() - row.min()) <= 1 and abs(rows.max() - row.max()) <= 1
    assert abs(cols.min() - col.min()) <= 1 and abs(cols.max() - col.max()) <= 1


# ------------------------------------------------------------------------------------------------ 7. determinism, capture
def test_batch_independence_repeatability_graph_replay_and_no_synchronisation():
    case = body_case(14, 16, 96)
    r, verts, t = case['renderer'], case['verts'], dev(case['t'])
    bg = torch.rand(4, 96, 96, 3, device=DEV)
    kw = dict(views=VIEW_NAMES, background=bg)
    first = {k: v.clone() for k, v in r.render(verts, t, **kw).items()}
    again = r.render(verts, t, **kw)
    for k in first:
        assert torch.equal(first[k], again[k]), k
    for b in range(4):
        alone = r.render(verts[b:b + 1].contiguous(), t[b:b + 1].contiguous(), views=VIEW_NAMES, background=bg[b:b + 1].contiguous())
        for k in first:
            assert torch.equal(alone[k][0], first[k][b]), (k, b)
    # front over the background, the turned views over white
    empty = first['face'] < 0
    assert torch.equal(first['image'][:, 0][empty[:, 0]], bg[empty[:, 0]])
    assert torch.all(first['image'][:, 1:][empty[:, 1:]] == 1.0)
    # no host synchronisation once the tables exist
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r.render(verts, t, **kw)
        r.contact_colors(verts, partner=torch.full(verts.shape[:2], -1, dtype=torch.int32, device=DEV))
    finally:
        torch.cuda.set_sync_debug_mode('default')
    # graph replay
    static_v, static_t = verts.clone(), t.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r.render(static_v, static_t, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = r.render(static_v, static_t, **kw)
    flipped = verts.flip(0).contiguous()
    want = {k: v.clone() for k, v in r.render(flipped, t, **kw).items()}
    static_v.copy_(flipped)
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(out[k], want[k]), k
    assert not torch.equal(want['face'], first['face'])


# ------------------------------------------------------------------------------------------------ 8. colours
def assert_colours(got, want_and_sources, verts_b, what):
    """Identical; one level apart only where the float64 value of (v - min) 255 / max of a vertex the colour was taken
    from lies within 1e-3 of an integer."""
    want, src = want_and_sources
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    diff = np.abs(got - want)
    mc = rc.meshcols64(verts_b)
    near_integer = np.abs(mc - np.rint(mc)) < 1e-3                  # [V,3]
    allowed = ((src[:, :1] >= 0) & (near_integer[src[:, 0]] | near_integer[src[:, 1]])).astype(np.int64)
    n = int((diff > 0).any(1).sum())
    report('%s: vertices whose colour differs by one level' % what, n, len(got))
    assert np.all(diff <= allowed), (what, int(diff.max()), np.argwhere(diff > allowed)[:5].tolist())
    assert n < 0.01 * len(got), (what, n)


@functools.lru_cache(maxsize=None)
def folded():
    from synthetic import folded_poses, make_body
    from tuch_amd.models.smpl import SMPL
    body = make_body(14, 16)
    bp, go, be = [dev(np.asarray(x, np.float32)) for x in folded_poses(6, 11)]
    verts = SMPL(model_data=body).to(DEV)(betas=be, body_pose=bp, global_orient=go).vertices.detach().contiguous()
    return body, verts


def test_pair_colours_from_self_contact_and_adversarial_lists():
    from tuch_amd.contact_detect import SelfContact
    body, verts = folded()
    v_np = verts.cpu().numpy()
    r = renderer(body.faces, 32)
    det = SelfContact(body.geodesics, geothres=0.3, euclthres=0.05)
    found = det(verts)
    lists = det.verts_in_contact(verts)
    got = r.contact_colors(verts, partner=found['partner']).cpu().numpy()
    by_lists = r.contact_colors(verts, pairs=lists).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, by_lists)
    n_pairs = 0
    for b in range(len(v_np)):
        c1, c2 = [x.cpu().numpy() for x in lists[b]]
        n_pairs += len(c1)
        assert_colours(got[b], rc.contact_colors_pairs(v_np[b], c1, c2), v_np[b], 'partner form, body %d' % b)
    assert n_pairs > 20
    # vertices repeated in both columns, a pair of a vertex with itself, an empty list, a missing body, a list as long as V
    rng = np.random.default_rng(3)
    V = v_np.shape[1]
    adversarial = {0: [rng.integers(0, 12, 150), rng.integers(0, 12, 150)], 1: [np.array([5, 5, 7, 5]), np.array([5, 9, 5, 5])],
                   2: [np.zeros(0, np.int64), np.zeros(0, np.int64)], 4: [np.arange(V), np.arange(V)[::-1]],
                   5: [torch.tensor([1, 2, 3, V - 1]), torch.tensor([V - 1, 1, 2, 0])]}
    got = r.contact_colors(verts, pairs=adversarial).cpu().numpy()
    for b in range(len(v_np)):
        c1, c2 = [np.asarray(x) for x in adversarial.get(b, ([], []))]
        assert_colours(got[b], rc.contact_colors_pairs(v_np[b], c1, c2), v_np[b], 'adversarial pairs, body %d' % b)
    assert (got[2] == 230).all() and (got[3] == 230).all() and (got[4] == 230).all() and not (got[0] == 230).all()


def test_region_colours_with_overlapping_regions():
    body, verts = folded()
    v_np = verts.cpu().numpy()
    V = v_np.shape[1]
    names = list(body.regions.keys())[:6]
    csig = {n: np.asarray(body.regions[n]).copy() for n in names}
    csig[names[0]] = np.concatenate([csig[names[1]][-3:][::-1], csig[names[0]]])      # overlap; first listed vertex not the smallest
    csig[names[5]] = np.array([V - 1, 0, V - 1])
    classes = [(names[0], names[1]), (names[2], names[3]), (names[1], names[2]), (names[4], names[4]), (names[5], names[0]),
               (names[3], names[5])]
    contactlist = {'classes': classes, 'csig': csig}
    contact = np.array([[1, 0, 1, 0, 0, 1], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 1, 0], [0, 1, 0, 1, 0, 0],
                        [2, 1, 0, 0, 0, 1]])
    r = renderer(body.faces, 32)
    got = r.contact_colors(verts, contact=torch.as_tensor(contact), contactlist=contactlist).cpu().numpy()
    for b in range(len(v_np)):
        want = rc.contact_colors_regions(v_np[b], contact[b], classes, csig)
        assert_colours(got[b], want, v_np[b], 'region form, body %d' % b)
    assert (got[1] == 230).all() and not (got[2] == 230).all()


# ------------------------------------------------------------------------------------------------ 9. Renderer
def test_reference_style_renderer():
    from tuch_amd.utils.renderer import Renderer
    case = body_case(10, 12, 64)
    body, res = case['body'], 64
    names = list(body.regions.keys())
    contactlist = {'classes': [(names[0], names[1]), (names[2], names[3])], 'csig': {n: np.asarray(body.regions[n]) for n in names}}
    ren = Renderer(contactlist, focal_length=case['f'], img_res=res, faces=body.faces)
    verts, cam = case['verts_np'][0], case['t'][0].copy()
    image = np.random.default_rng(1).random((res, res, 3)).astype(np.float32)
    cam_before = cam.copy()
    front = ren(verts, cam, image, colverts=[np.array([3, 4]), np.array([40, 41])])
    assert isinstance(front, np.ndarray) and front.shape == (res, res, 3) and front.dtype == np.float32
    assert np.array_equal(cam, cam_before)                              # the reference flips cam[0] in place
    mask = case['out']['depth'][0, 0] > 0
    assert np.array_equal(front[~mask], image[~mask]) and not np.array_equal(front[mask], image[mask])
    for w, kw in ((1, dict(dorot2=True)), (2, dict(dorot3=True))):
        side = ren(verts, cam, image, contact=np.array([1, 0]), **kw)
        m = case['out']['depth'][0, w] > 0
        assert np.all(side[~m] == 1.0) and side[m].max() <= 1.0 and side[m].min() >= 0.0
    white = ren(verts, cam, None)
    assert np.all(white[~mask] == 1.0)
    # coloured vertices show: the picture with contact colours differs from the plain one on the mask only
    plain = ren(verts, cam, image)
    assert np.array_equal(plain[~mask], front[~mask])
    # the grid
    B = 3
    images = torch.rand(B, 3, res, res)
    grid = ren.visualize_tbm(torch.tensor(case['verts_np'][:B]), torch.tensor(case['t'][:B]), images,
                             gt_vertsincontact_idx={0: [np.array([3]), np.array([40])], 1: None, 2: None},
                             has_contact=[True, False, False], gt_l3_contact=torch.tensor([[1, 0], [0, 1], [0, 0]]),
                             has_contact_pc=[False, True, True])
    assert grid.shape == (3, B * (res + 2) + 2, 4 * (res + 2) + 2) and grid.dtype == torch.float32
    for b in range(B):
        y = b * (res + 2) + 2
        assert torch.equal(grid[:, y:y + res, 2:2 + res], images[b])
        for w in range(3):
            x = (w + 1) * (res + 2) + 2
            tile = grid[:, y:y + res, x:x + res].permute(1, 2, 0).numpy()
            m = case['out']['depth'][b, w] > 0
            bgd = images[b].permute(1, 2, 0).numpy() if w == 0 else np.ones((res, res, 3), np.float32)
            assert np.array_equal(tile[~m], bgd[~m]), (b, w)
    eft = ren.visualize_eft(torch.tensor(case['verts_np'][:2]), torch.tensor(case['t'][:2]), images[:2],
                            contact=torch.tensor([[1, 1], [0, 0]]))
    assert eft.shape == (3, 2 * (res + 2) + 2, 4 * (res + 2) + 2)
    opti = ren.visu_smplifycontactopti([torch.tensor(case['verts_np'][:2])] * 5, torch.tensor(case['t'][:2]), images[:2],
                                       [np.array([1, 0]), np.array([0, 0])], gt_vertsincontact_idx=None)
    assert opti.shape == (3, 2 * (res + 2) + 2, 7 * (res + 2) + 2)
