"""Reference rasterisers for the renderer tests (tests/test_gpu_render.py, tests/test_render_host.py): plain numpy written
for these tests, one vectorised step per triangle.

  integer_raster   the rules of include/tuch_amd.h restated with integers: float32 projection snapped to 1/256 px, exact
                   edge functions, ties by the geometric definition of the top-left rule -- a centre on an edge is inside
                   when the centre moved by (+eps, +eps^2) is strictly inside --, depth from the barycentrics of the
                   unsnapped float32 projections clamped to the triangle (float64 arithmetic), nearest surface, smaller
                   face id at equal depth.  No exclusions: used where the inputs are exactly representable (tie rules,
                   watertightness, clipping).
  float_raster     float64 throughout and NO snapping: face, depth, the second-nearest depth, the distance of every
                   pixel centre to the nearest projected edge, and the float64 shading.  Used for the bodies, off the
                   pixels that `excluded` marks.
  contact_colors_* the reference's colouring loop (renderer.py:199-224) per body.
"""
import numpy as np

NEAR = 1e-3
SUB = 256
DEFAULT_ALBEDO = 230


def camera_points(verts, rot, t, dtype=np.float64):
    v = np.asarray(verts, dtype)
    return (v @ np.asarray(rot, dtype).T + np.asarray(t, dtype)).astype(dtype)


def project(verts, rot, t, f, cx, cy, dtype=np.float64):
    """(xy [V,2], z [V]) of perspective_projection; rows with z <= NEAR or a non-finite entry are flagged in `ok`."""
    p = camera_points(verts, rot, t, dtype)
    with np.errstate(all='ignore'):
        z = p[:, 2]
        xy = np.stack([dtype(f) * p[:, 0] / z + dtype(cx), dtype(f) * p[:, 1] / z + dtype(cy)], 1)
        ok = np.isfinite(p).all(1) & (z > NEAR) & np.isfinite(xy).all(1)
    return xy, z, ok


def integer_raster(verts, faces, rot, t, f, cx, cy, H, W):
    """-> face [H,W] int32 (-1 = empty), depth [H,W] float64 (0 = empty)."""
    xy, z, ok = project(np.asarray(verts, np.float32), rot, t, f, cx, cy, np.float32)
    with np.errstate(all='ignore'):
        snapped = np.where(ok[:, None], np.rint(xy.astype(np.float64) * SUB), 0).astype(np.int64)
    z = z.astype(np.float64)
    xy = xy.astype(np.float64)
    face = np.full((H, W), -1, np.int32)
    depth = np.full((H, W), np.inf)
    for fid, tri in enumerate(np.asarray(faces)):
        if not ok[tri].all():
            continue
        (x0, y0), (x1, y1), (x2, y2) = [tuple(int(a) for a in snapped[i]) for i in tri]
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area == 0:
            continue
        s = 1 if area > 0 else -1
        xs, ys = (x0, x1, x2), (y0, y1, y2)
        c0, c1 = max(0, -((SUB // 2 - min(xs)) // SUB)), min(W - 1, (max(xs) - SUB // 2) // SUB)
        r0, r1 = max(0, -((SUB // 2 - min(ys)) // SUB)), min(H - 1, (max(ys) - SUB // 2) // SUB)
        if c0 > c1 or r0 > r1:
            continue
        px = (np.arange(c0, c1 + 1, dtype=np.int64) * SUB + SUB // 2)[None, :]
        py = (np.arange(r0, r1 + 1, dtype=np.int64) * SUB + SUB // 2)[:, None]
        inside = np.ones((r1 - r0 + 1, c1 - c0 + 1), bool)
        e, g = [], []
        for i, j in ((1, 2), (2, 0), (0, 1)):                       # the edge opposite corner 0, 1, 2
            dx, dy = s * (xs[j] - xs[i]), s * (ys[j] - ys[i])
            ek = dx * (py - ys[i]) - dy * (px - xs[i])
            # E(p + (eps, eps^2)) = E + eps (-dy) + eps^2 dx > 0
            inside &= (ek > 0) | ((ek == 0) & ((-dy > 0) | ((dy == 0) & (dx > 0))))
            e.append(ek.astype(np.float64) / (s * area))
            ax, ay = xy[tri[i], 0] - px / SUB, xy[tri[i], 1] - py / SUB
            bx, by = xy[tri[j], 0] - px / SUB, xy[tri[j], 1] - py / SUB
            g.append(ax * by - ay * bx)
        if not inside.any():
            continue
        with np.errstate(all='ignore'):
            w = [np.clip(gk / (g[0] + g[1] + g[2]), 0.0, 1.0) for gk in g]
            total = w[0] + w[1] + w[2]
            sane = (total >= 0.25) & (total <= 3.0)
            w = [np.where(sane, w[k] / total, e[k]) for k in range(3)]
        iz = sum(w[k] / z[tri[k]] for k in range(3))
        with np.errstate(all='ignore'):
            zp = np.where(inside, 1.0 / iz, np.inf)
        box = (slice(r0, r1 + 1), slice(c0, c1 + 1))
        win = zp < depth[box]                                          # ascending face ids: the smaller id keeps a tie
        depth[box] = np.where(win, zp, depth[box])
        face[box] = np.where(win, fid, face[box])
    depth[face < 0] = 0.0
    return face, depth


def vertex_normals(verts, faces):
    """Area-weighted vertex normals, float64."""
    v = np.asarray(verts, np.float64)
    faces = np.asarray(faces)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    n[~np.isfinite(n).all(1)] = 0.0
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, faces[:, k], n)
    length = np.linalg.norm(out, axis=1, keepdims=True)
    return np.divide(out, length, out=np.zeros_like(out), where=length > 0)


def float_raster(verts, faces, rot, t, f, cx, cy, H, W, colors=None, background=None):
    """float64, unsnapped -> dict(face, depth, second [H,W] (inf where fewer than two surfaces), edge_dist [H,W] px,
    image [H,W,3])."""
    faces = np.asarray(faces)
    xy, z, ok = project(verts, rot, t, f, cx, cy)
    face = np.full((H, W), -1, np.int32)
    depth = np.full((H, W), np.inf)
    second = np.full((H, W), np.inf)
    edge_dist = np.full((H, W), np.inf)
    pad = 1.0 / 64
    for fid, tri in enumerate(faces):
        if not ok[tri].all():
            continue
        p = xy[tri]
        c0, c1 = max(0, int(np.ceil(p[:, 0].min() - 0.5 - pad))), min(W - 1, int(np.floor(p[:, 0].max() - 0.5 + pad)))
        r0, r1 = max(0, int(np.ceil(p[:, 1].min() - 0.5 - pad))), min(H - 1, int(np.floor(p[:, 1].max() - 0.5 + pad)))
        if c0 > c1 or r0 > r1:
            continue
        px = (np.arange(c0, c1 + 1) + 0.5)[None, :]
        py = (np.arange(r0, r1 + 1) + 0.5)[:, None]
        box = (slice(r0, r1 + 1), slice(c0, c1 + 1))
        area = (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0])
        e = []
        d = np.full((r1 - r0 + 1, c1 - c0 + 1), np.inf)
        for i, j in ((1, 2), (2, 0), (0, 1)):
            dx, dy = p[j, 0] - p[i, 0], p[j, 1] - p[i, 1]
            e.append(dx * (py - p[i, 1]) - dy * (px - p[i, 0]))
            l2 = dx * dx + dy * dy
            u = np.clip(((px - p[i, 0]) * dx + (py - p[i, 1]) * dy) / l2, 0.0, 1.0) if l2 > 0 else 0.0
            d = np.minimum(d, np.hypot(px - (p[i, 0] + u * dx), py - (p[i, 1] + u * dy)))
        edge_dist[box] = np.minimum(edge_dist[box], d)
        if area == 0:
            continue
        w = [ek / area for ek in e]
        inside = (w[0] > 0) & (w[1] > 0) & (w[2] > 0)
        if not inside.any():
            continue
        zp = np.where(inside, 1.0 / (w[0] / z[tri[0]] + w[1] / z[tri[1]] + w[2] / z[tri[2]]), np.inf)
        d1, d2 = depth[box], second[box]
        win = zp < d1
        second[box] = np.where(win, d1, np.minimum(d2, zp))
        depth[box] = np.where(win, zp, d1)
        face[box] = np.where(win, fid, face[box])
    covered = face >= 0
    depth[~covered] = 0.0
    # shading of the visible surface, all pixels at once
    image = np.ones((H, W, 3)) if background is None else np.array(background, np.float64)
    if covered.any():
        rr, cc = np.nonzero(covered)
        tri = faces[face[rr, cc]]
        p = xy[tri]                                                   # [n,3,2]
        q = np.stack([cc + 0.5, rr + 0.5], 1)
        def edge(i, j):
            return (p[:, j, 0] - p[:, i, 0]) * (q[:, 1] - p[:, i, 1]) - (p[:, j, 1] - p[:, i, 1]) * (q[:, 0] - p[:, i, 0])
        e = np.stack([edge(1, 2), edge(2, 0), edge(0, 1)], 1)
        w = e / e.sum(1, keepdims=True)
        pw = w / z[tri]
        pw = pw / pw.sum(1, keepdims=True)                            # perspective-correct weights
        normals = vertex_normals(verts, faces) @ np.asarray(rot, np.float64).T
        n = (pw[:, :, None] * normals[tri]).sum(1)
        length = np.linalg.norm(n, axis=1)
        nz = np.divide(n[:, 2], length, out=np.zeros_like(length), where=length > 0)
        shade = np.minimum(1.0, 0.3 + 0.7 * np.maximum(0.0, -nz))
        if colors is None:
            albedo = np.full((len(rr), 3), float(DEFAULT_ALBEDO))
        else:
            albedo = (pw[:, :, None] * np.asarray(colors, np.float64)[tri]).sum(1)
        image[rr, cc] = np.minimum(1.0, albedo / 255.0 * shade[:, None])
    return {'face': face, 'depth': depth, 'second': second, 'edge_dist': edge_dist, 'image': image}


EDGE_BAND = 1.0 / 128          # px: four times the 1/512 px snapping error
DEPTH_TIE = 1e-5               # relative


def excluded(ref):
    """Pixels left out of a comparison with float_raster: (a) centre within EDGE_BAND of a projected edge, (b) the two
    nearest surfaces within DEPTH_TIE relative in depth."""
    with np.errstate(all='ignore'):
        tie = (ref['face'] >= 0) & np.isfinite(ref['second']) & ((ref['second'] - ref['depth']) < DEPTH_TIE * ref['depth'])
    return (ref['edge_dist'] < EDGE_BAND) | tie


# ------------------------------------------------------------------------------------------------ colours
def meshcols64(verts_b):
    """float64 value of (v - min) * 255 / max before truncation (for the one-level allowance near integers)."""
    v = np.asarray(verts_b, np.float64)
    d = v - v.min(0)
    return d * 255.0 / d.max(0)


def meshcols(verts_b):
    """renderer.py:201-206 on float32 vertices."""
    verts = np.asarray(verts_b, np.float32)
    verts = verts - np.min(verts, axis=0)
    return (verts * 255 / np.max(verts, axis=0)).astype(np.int64)


def contact_colors_pairs(verts_b, c1, c2):
    """-> (colours [V,3], sources [V,2]: the vertices a colour was taken from, -1 = untouched)."""
    mc = meshcols(verts_b)
    col = np.full((len(mc), 3), DEFAULT_ALBEDO, np.int64)
    src = np.full((len(mc), 2), -1, np.int64)
    if len(c1) < len(mc):                                             # renderer.py:210
        for a, b in zip(c1, c2):
            cur = ((mc[a] + mc[b]) / 2).astype(np.int64)
            col[a] = cur
            col[b] = cur
            src[a] = src[b] = (a, b)
    return col, src


def contact_colors_regions(verts_b, contact, classes, csig):
    mc = meshcols(verts_b)
    col = np.full((len(mc), 3), DEFAULT_ALBEDO, np.int64)
    src = np.full((len(mc), 2), -1, np.int64)
    for i1, val in enumerate(contact):
        if val == 1:
            vr1, vr2 = np.asarray(csig[classes[i1][0]]), np.asarray(csig[classes[i1][1]])
            col[vr1] = mc[vr1[0]]
            col[vr2] = mc[vr1[0]]
            src[vr1] = src[vr2] = vr1[0]
    return col, src
