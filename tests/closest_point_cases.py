"""The closest-point query stated in float64, and the meshes and queries its tests share (tests/test_closest_point_host.py
on the CPU, tests/test_gpu_closest_point.py on the device).  No GPU here.

The statement is formulated differently from the kernel (csrc/closest_point.hip classifies the query into one of seven
regions and evaluates one point): the distance to a triangle is the MINIMUM of
  - the distances to its three edges taken as segments, and
  - the distance to its plane, where the projection falls inside a triangle that has an area.
``tri_d2`` is that sentence in whatever dtype its arguments have: float64 is the reference, float32 (``dtype=np.float32``)
only sizes the tolerance -- the error of a float32 evaluation of the same inputs that is not the kernel's.
"""
from __future__ import annotations

import functools

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
FAR = 1e3               # the query 1e3 m away
FLOOR_ULPS = 8.0        # see ``bounds``


def _dot(a, b):
    return (a * b).sum(-1)


def _segment_d2(p, s, e):
    d = e - s
    dd = _dot(d, d)
    one = np.ones_like(dd)
    t = np.clip(np.where(dd > 0, _dot(p - s, d) / np.where(dd > 0, dd, one), 0 * one), 0, 1).astype(dd.dtype)
    r = p - (s + t[..., None] * d)
    return _dot(r, r)


def tri_d2(p, a, b, c):
    """Squared distance from points p [...,3] to triangles (a, b, c) [...,3] (broadcast), in the arguments' dtype."""
    best = np.minimum(np.minimum(_segment_d2(p, a, b), _segment_d2(p, b, c)), _segment_d2(p, c, a))
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    inside = nn > 0
    for s, e in ((a, b), (b, c), (c, a)):
        inside = inside & (_dot(n, np.cross(e - s, p - s)) >= 0)
    h = _dot(n, p - a)
    plane = h * h / np.where(nn > 0, nn, np.ones_like(nn))
    return np.where(inside, plane, best)


def candidates(points, verts, faces):
    """For every query the faces that can hold its nearest point (float64, conservative): those whose bounding sphere
    comes as near as the nearest vertex.  (rows, cols) of the (query, face) pairs."""
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    tri = v[faces]
    centre = tri.mean(1)
    radius = np.linalg.norm(tri - centre[:, None], axis=2).max(1)
    rows, cols = [], []
    for i in range(0, len(p), 256):
        q = p[i:i + 256]
        ub = np.sqrt(((q[:, None] - v[None]) ** 2).sum(2).min(1))
        lb = np.linalg.norm(q[:, None] - centre[None], axis=2) - radius[None]
        r, c = np.nonzero(lb <= ub[:, None] * (1 + 1e-9) + 1e-12)
        rows.append(r + i)
        cols.append(c)
    return np.concatenate(rows), np.concatenate(cols)


def statement(points, verts, faces, dtype=np.float64, pairs=None):
    """(d2 [Q] in `dtype`, face [Q]: the first face that attains it) of one body."""
    faces = np.asarray(faces)
    rows, cols = candidates(points, verts, faces) if pairs is None else pairs
    p, v = np.asarray(points, dtype), np.asarray(verts, dtype)
    tri = v[faces[cols]]
    d = tri_d2(p[rows], tri[:, 0], tri[:, 1], tri[:, 2])
    d2 = np.full(len(p), np.inf, dtype)
    np.minimum.at(d2, rows, d)
    face = np.full(len(p), np.iinfo(np.int64).max, np.int64)
    hit = d == d2[rows]
    np.minimum.at(face, rows[hit], cols[hit])
    return d2, face


def face_d2(points, verts, faces, face):
    """float64 squared distance from every query to the face given for it."""
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    tri = v[np.asarray(faces)[np.asarray(face)]]
    return tri_d2(p, tri[:, 0], tri[:, 1], tri[:, 2])


def runner_up(points, verts, faces):
    """float64: the smallest squared distance to a face other than the nearest one (inf for a one-face mesh)."""
    faces = np.asarray(faces)
    rows, cols = candidates(points, verts, faces)
    _, best = statement(points, verts, faces, pairs=(rows, cols))
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    tri = v[faces[cols]]
    d = tri_d2(p[rows], tri[:, 0], tri[:, 1], tri[:, 2])
    d[cols == best[rows]] = np.inf
    out = np.full(len(p), np.inf)
    np.minimum.at(out, rows, d)
    return out


def bounds(points, verts, d2_64, d2_32):
    """Per query: 4 x the float32 restatement's largest error on this body, floored at FLOOR_ULPS float32 ulps of the
    squared coordinate scale (the rule of tests/test_gpu_mesh_fit.py: the yardstick is a float32 evaluation of the same
    inputs that is not the kernel's).  The scale of a query is the largest coordinate magnitude among the body's vertices
    and the query itself, and the restatement's error is taken over the queries of the same class -- the one query FAR
    away has a d2 of 1e6 whose own ulp (0.06) says nothing about the others.  Why 8 ulps: d2 is a sum of three squares
    of differences of coordinates of size <= s; every difference carries the rounding of s-sized terms, and a result of
    size (2 s)^2 has an ulp of 4 ulp(s^2): two such roundings."""
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    scale = np.maximum(np.abs(v).max(), np.abs(p).max(1))
    far = np.abs(p).max(1) > 0.1 * FAR
    err = np.abs(np.asarray(d2_32, np.float64) - d2_64)
    cls = np.where(far, err[far].max() if far.any() else 0.0, err[~far].max() if (~far).any() else 0.0)
    return np.maximum(4.0 * cls, FLOOR_ULPS * EPS32 * scale ** 2)


# ---------------------------------------------------------------------------------------------------------- meshes
def one_triangle():
    verts = np.array([[0.1, -0.2, 0.05], [0.9, 0.1, -0.1], [0.2, 0.8, 0.3]], np.float32)
    return verts, np.array([[0, 1, 2]], np.int64)


def open_strip(num_faces: int = 130):
    """A wavy open strip: no cluster tree, ceil(F / 64) groups, the last one ragged."""
    i = np.arange(num_faces + 2)
    verts = np.stack([0.03 * (i // 2), 0.05 * (i % 2) + 0.01 * np.sin(0.7 * i), 0.04 * np.sin(0.25 * i)], 1).astype(np.float32)
    faces = np.stack([i[:-2], i[1:-1], i[2:]], 1)
    faces[1::2] = faces[1::2][:, [1, 0, 2]]
    return verts, faces.astype(np.int64)


def tetrahedron():
    verts = np.array([[0.0, 0.0, 0.6], [0.5, 0.0, -0.2], [-0.3, 0.45, -0.2], [-0.3, -0.45, -0.25]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], np.int64)
    return verts, faces


def icosphere():
    """320 faces, 162 vertices, radius about 0.5 with a bump so that no two distances tie by symmetry."""
    from synthetic import _ico_topology, _orient_outward
    dirs, faces = _ico_topology(4)
    verts = (0.5 * dirs * (1.0 + 0.15 * np.sin(3.0 * dirs[:, :1]) * dirs[:, 1:2]) + np.array([0.05, -0.02, 0.1])).astype(np.float32)
    return verts, _orient_outward(verts.astype(np.float64), faces).astype(np.int64)


def degenerate_mesh():
    """The open strip plus a face whose corners are collinear (zero area), a face that names one vertex twice and a
    face whose three corners coincide, all away from the strip: near them they are the nearest 'faces'."""
    verts, faces = open_strip(70)
    n = len(verts)
    extra = np.array([[0.0, 0.0, 0.5], [0.25, 0.0, 0.5], [1.0, 0.0, 0.5],          # collinear, b between a and c
                      [0.2, 0.6, 0.4], [0.7, 0.9, 0.6],                             # a segment named (a, a, c)
                      [1.5, 0.5, -0.4], [1.5, 0.5, -0.4], [1.5, 0.5, -0.4]], np.float32)      # a point
    more = np.array([[n, n + 1, n + 2], [n + 3, n + 3, n + 4], [n + 5, n + 6, n + 7]], np.int64)
    return np.concatenate([verts, extra]), np.concatenate([faces, more])


def body_batch(verts, batch: int, seed: int = 0):
    """`batch` posed copies [batch,V,3] of a mesh: the mesh itself, then copies rotated a little, scaled and shifted."""
    rng = np.random.default_rng(seed)
    out = [np.asarray(verts, np.float32)]
    for _ in range(batch - 1):
        w = 0.3 * rng.standard_normal(3)
        k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        rot = np.linalg.qr(np.eye(3) + k)[0]
        out.append(((np.asarray(verts, np.float64) @ rot.T) * (0.8 + 0.4 * rng.random()) + 0.1 * rng.standard_normal(3)).astype(np.float32))
    return np.stack(out)


def queries(verts_b, faces, count: int, seed: int = 0):
    """`count` queries [count,3] float32 of one body, every kind in turn: a random point in twice the bounding box, one
    of the mesh's own vertices, an edge midpoint; the centroid is query 3 and the point FAR away query 4."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts_b, np.float64)
    faces = np.asarray(faces)
    lo, hi = v.min(0), v.max(0)
    mid, half = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-2)
    out = []
    for i in range(count):
        kind = i % 3
        if i == 3:
            out.append(v.mean(0))
        elif i == 4:
            out.append(mid + np.array([FAR, 0.3 * FAR, -0.2 * FAR]))
        elif kind == 0:
            out.append(mid + half * (2.0 * rng.random(3) - 1.0))
        elif kind == 1:
            out.append(v[rng.integers(len(v))])
        else:
            f = faces[rng.integers(len(faces))]
            k = rng.integers(3)
            out.append(0.5 * (v[f[k]] + v[f[(k + 1) % 3]]))
    return np.asarray(out, np.float32).reshape(count, 3)


def reference(points, verts, faces):
    """Per body of points [B,Q,3] / verts [B,V,3]: dict(d2, face, bound) of float64 / int64 / float64 arrays [B,Q]."""
    d2, face, bound = [], [], []
    for p, v in zip(points, verts):
        pairs = candidates(p, v, np.asarray(faces))
        d64, f64 = statement(p, v, faces, np.float64, pairs)
        d32, _ = statement(p, v, faces, np.float32, pairs)
        d2.append(d64)
        face.append(f64)
        bound.append(bounds(p, v, d64, d32))
    return dict(d2=np.stack(d2), face=np.stack(face), bound=np.stack(bound))


@functools.lru_cache(maxsize=None)
def mesh(name: str):
    """(verts [B0,V,3] float32 of the poses the fixture has, faces [F,3])."""
    if name in ('body122', 'smpl'):
        import golden_io as gio
        g = gio.load('contact_%s.npz' % {'body122': 'small', 'smpl': 'full2'}[name])
        return np.asarray(g['verts'], np.float32), np.asarray(g['faces'], np.int64)
    verts, faces = {'triangle': one_triangle, 'strip': open_strip, 'tetrahedron': tetrahedron, 'icosphere': icosphere,
                    'degenerate': degenerate_mesh}[name]()
    return verts[None], faces


@functools.lru_cache(maxsize=None)
def case(name: str, batch: int, count: int, seed: int = 0):
    """dict(verts [B,V,3], faces, points [B,Q,3], ref: reference(...)); arrays are read-only (shared between tests)."""
    poses, faces = mesh(name)
    if len(poses) >= batch:
        verts = poses[:batch]
    else:
        verts = np.concatenate([poses, body_batch(poses[0], batch - len(poses) + 1, seed + 1)[1:]])
    points = np.stack([queries(verts[b], faces, count, seed + 10 * b) for b in range(batch)])
    out = dict(verts=np.ascontiguousarray(verts), faces=faces, points=points, ref=reference(points, verts, faces))
    for a in (out['verts'], out['points'], *out['ref'].values()):
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------- adjoint
def interior_queries(verts_b, faces, count: int, seed: int, margin: float = 0.2, height=(0.002, 0.02)):
    """`count` queries above face interiors, float32 [count,3]: a point of a random face with every weight >= margin,
    lifted along the normal; kept only where, in float64, the nearest point is inside a face with every weight >= 0.1,
    at least 4 mm away, and the next face is at least 1 mm farther (the caller asserts the same again)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts_b, np.float64)
    faces = np.asarray(faces)
    f = faces[rng.integers(len(faces), size=4 * count)]
    w = margin + (1.0 - 3.0 * margin) * rng.dirichlet(np.ones(3), 4 * count)
    tri = v[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    h = rng.uniform(*height, 4 * count) * rng.choice([-1.0, 1.0], 4 * count)
    p = ((w[:, :, None] * tri).sum(1) + h[:, None] * n).astype(np.float32)
    d2, near = statement(p, v, faces)
    ok = (projection_weights(p.astype(np.float64), v[faces[near]]).min(1) >= 0.1) & (np.sqrt(d2) >= 4e-3) & \
        (np.sqrt(runner_up(p, v, faces)) - np.sqrt(d2) >= 1e-3)
    assert ok.sum() >= count, (ok.sum(), count)
    return p[ok][:count]


def projection_weights(p, tri):
    """float64 barycentric weights of the projection of p onto the plane of tri [..,3,3]."""
    a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    wa = _dot(n, np.cross(c - b, p - b)) / nn
    wb = _dot(n, np.cross(a - c, p - c)) / nn
    return np.stack([wa, wb, 1.0 - wa - wb], -1)


def d2_sum_and_gradients(points, verts, faces, upstream, step: float = 1e-6):
    """sum_q upstream[q] * d2(q) of one body in float64 and its central differences with respect to the points [Q,3]
    and the vertices [V,3] (only the vertices of the nearest faces move the sum: the others' rows are zero)."""
    faces = np.asarray(faces)
    p0, v0 = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    pairs = candidates(p0, v0, faces)
    up = np.asarray(upstream, np.float64)

    def per_query(p, v):
        return statement(p, v, faces, np.float64, pairs)[0]
    _, near = statement(p0, v0, faces, np.float64, pairs)
    gp = np.zeros_like(p0)
    for k in range(3):
        d = np.zeros(3)
        d[k] = step
        gp[:, k] = up * (per_query(p0 + d, v0) - per_query(p0 - d, v0)) / (2 * step)
    gv = np.zeros_like(v0)
    for vi in np.unique(faces[near]):
        for k in range(3):
            vp, vm = v0.copy(), v0.copy()
            vp[vi, k] += step
            vm[vi, k] -= step
            gv[vi, k] = (up * (per_query(p0, vp) - per_query(p0, vm))).sum() / (2 * step)
    return gp, gv


# ---------------------------------------------------------------------------------------------------------- signs
def winding_number(points, verts, faces):
    """float64 winding number (van Oosterom-Strackee solid angles over 4 pi) of one closed mesh at points [Q,3]."""
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    out = np.zeros(len(p))
    for i in range(0, len(p), 256):
        r = v[np.asarray(faces)][None] - p[i:i + 256, None, None]           # [q,F,3,3]
        a, b, c = r[:, :, 0], r[:, :, 1], r[:, :, 2]
        la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
        num = _dot(a, np.cross(b, c))
        den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
        out[i:i + 256] = (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)
    return out


def offset_queries(verts_b, faces, count: int, seed: int, offset: float = 5e-3, keep: float = 1e-4):
    """Surface points pushed +-offset along their face normal, dropped where the float64 distance to the surface comes
    out below `keep` (another sheet of the surface passes there).  float32 [n,3], n <= count."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts_b, np.float64)
    f = np.asarray(faces)[rng.integers(len(faces), size=count)]
    w = rng.dirichlet(np.ones(3), count)
    tri = v[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    p = ((w[:, :, None] * tri).sum(1) + offset * rng.choice([-1.0, 1.0], count)[:, None] * n).astype(np.float32)
    d2, _ = statement(p, v, faces)
    return p[np.sqrt(d2) >= 2.0 * keep]
