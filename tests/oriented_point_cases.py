"""The normal-compatible closest-point query restated for its tests (tests/test_oriented_point_host.py on the CPU,
tests/test_gpu_oriented_point.py on the device).  No GPU here.

  rule32         the admissibility rule of include/tuch_amd.h in numpy float32, op for op (nothing is fused there, so
                 numpy's one-rounding-per-operation arithmetic reproduces every decision bit for bit): for all (query,
                 face) pairs of a body
  reference      the expected answer: the float64 cc.tri_d2 minimum over exactly the admissible set, the first face that
                 attains it, and cc.bounds from the float32 restatement over the same set.  The set is bit-exact, so no
                 query is excluded as "near the threshold".
  normals        a case's normals, in turn: the float64 nearest face's normal (raw: its length is twice the face's
                 area), that normal flipped (unit), a random unit vector, a zero row
  threshold_*    queries 1e-4 above face centroids whose normals sit max_angle (1 +- 2^-20) and max_angle +- 1 degree
                 from the face's
  term_*         the data term over the admissible-set answers: unmatched points add 0 and keep their weight
"""
from __future__ import annotations

import functools
import math

import numpy as np

import closest_point_cases as cc
import scan_fit_cases as sc

ANGLES = (30.0, 60.0, 90.0)
KINDS = ('nearest', 'flipped', 'random', 'zero')
F32 = np.float32


def cos32(angle):
    """The float32 c the C entry points take: cos(max_angle) in double, rounded once."""
    return F32(math.cos(math.radians(float(angle))))


def face_normals32(verts, faces):
    """m = (b - a) x (c - a) and mm of every face, in the rule's float32 sequence."""
    v = np.asarray(verts, F32)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    e1, e2 = b - a, c - a
    m = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                  e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    assert m.dtype == F32
    mm = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
    return m, mm


def unconstrained32(normals):
    """Queries whose nn is 0 or not finite: every face is admissible for them."""
    n = np.asarray(normals, F32)
    with np.errstate(over='ignore', invalid='ignore'):
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    return ~((nn > 0) & (nn < np.inf))


def rule32(verts, faces, normals, c, pairs=None):
    """admissible [Q,F] bool of one body under the float32 rule with threshold cosine c (float32).  pairs = (rows, cols):
    only those (query, face) pairs, as a flat array."""
    n = np.asarray(normals, F32)
    c = F32(c)
    c2 = c * c
    m, mm = face_normals32(verts, faces)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        free = ~((nn > 0) & (nn < np.inf))
        if pairs is None:
            s = (m[None, :, 0] * n[:, None, 0] + m[None, :, 1] * n[:, None, 1]) + m[None, :, 2] * n[:, None, 2]
            ok = (s > 0) & (s * s >= c2 * (mm[None] * nn[:, None]))
            return ok | free[:, None]
        rows, cols = pairs
        s = (m[cols, 0] * n[rows, 0] + m[cols, 1] * n[rows, 1]) + m[cols, 2] * n[rows, 2]
        assert s.dtype == F32
        ok = (s > 0) & (s * s >= c2 * (mm[cols] * nn[rows]))
        return ok | free[rows]


def cos64(verts, faces, normals):
    """float64 cosine of the angle between every (query normal, face normal) pair [Q,F]; NaN where either has no length."""
    v = np.asarray(verts, np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    m = np.cross(b - a, c - a)
    n = np.asarray(normals, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return (n @ m.T) / (np.linalg.norm(n, axis=1)[:, None] * np.linalg.norm(m, axis=1)[None])


def admissible_pairs(points, normals, verts, faces, c, chunk=128):
    """(rows, cols) of the admissible (query, face) pairs that can hold the nearest admissible point (float64,
    conservative): the faces whose bounding sphere comes as near as the nearest admissible face's centroid."""
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    tri = v[np.asarray(faces)]
    centre = tri.mean(1)
    radius = np.linalg.norm(tri - centre[:, None], axis=2).max(1)
    rows, cols = [], []
    for i in range(0, len(p), chunk):
        adm = rule32(verts, faces, np.asarray(normals)[i:i + chunk], c)
        with np.errstate(invalid='ignore'):
            dist = np.linalg.norm(p[i:i + chunk, None] - centre[None], axis=2)
        ub = np.where(adm, dist, np.inf).min(1)
        with np.errstate(invalid='ignore'):
            r, k = np.nonzero(adm & (dist - radius[None] <= ub[:, None] * (1 + 1e-9) + 1e-12))
        rows.append(r + i)
        cols.append(k)
    return np.concatenate(rows), np.concatenate(cols)


def statement(points, normals, verts, faces, c, dtype=np.float64, pairs=None):
    """(d2 [Q] in `dtype`, face [Q]) of one body over the admissible set: +inf / -1 where it is empty."""
    if pairs is None:
        pairs = admissible_pairs(points, normals, verts, faces, c)
    d2, face = cc.statement(points, verts, faces, dtype, pairs)
    face = np.where(face < len(faces), face, -1)
    return d2, face


def reference(points, normals, verts, faces, angle):
    """Per body of a batch: dict(d2 [B,Q] float64 (+inf: no admissible face), face [B,Q] (-1), bound [B,Q])."""
    c = cos32(angle)
    d2, face, bound = [], [], []
    for p, n, v in zip(points, normals, verts):
        pairs = admissible_pairs(p, n, v, faces, c)
        d64, f64 = statement(p, n, v, faces, c, np.float64, pairs)
        d32, _ = statement(p, n, v, faces, c, np.float32, pairs)
        hit = f64 >= 0
        bd = np.zeros(len(p))
        if hit.any():
            bd[hit] = cc.bounds(np.asarray(p)[hit], v, d64[hit], d32[hit])
        d2.append(d64)
        face.append(f64)
        bound.append(bd)
    return dict(d2=np.stack(d2), face=np.stack(face), bound=np.stack(bound))


def face_normal64(verts, faces, face):
    v = np.asarray(verts, np.float64)
    tri = v[np.asarray(faces)[np.asarray(face)]]
    return np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])


def normals(points, verts, faces, nearest, seed=0):
    """[Q,3] float32 of one body, the four kinds in turn (query i gets KINDS[i % 4]); `nearest` [Q] is the float64
    nearest face."""
    rng = np.random.default_rng(seed + 31)
    m = face_normal64(verts, faces, nearest)
    length = np.linalg.norm(m, axis=1, keepdims=True)
    unit = np.where(length > 0, m / np.where(length > 0, length, 1.0), 0.0)
    rand = rng.standard_normal((len(points), 3))
    rand /= np.linalg.norm(rand, axis=1, keepdims=True)
    kind = np.arange(len(points)) % 4
    out = np.where(kind[:, None] == 0, m, np.where(kind[:, None] == 1, -unit, np.where(kind[:, None] == 2, rand, 0.0)))
    return out.astype(F32)


@functools.lru_cache(maxsize=None)
def case(name: str, batch: int, count: int, angle: float, seed: int = 0):
    """cc.case(name, batch, count) + normals [B,Q,3] + angle + ref: reference(...) under the rule."""
    c = cc.case(name, batch, count, seed)
    nrm = np.stack([normals(c['points'][b], c['verts'][b], c['faces'], c['ref']['face'][b], seed + b) for b in range(batch)])
    out = dict(verts=c['verts'], faces=c['faces'], points=c['points'], normals=nrm, angle=angle, plain=c['ref'],
               ref=reference(c['points'], nrm, c['verts'], c['faces'], angle))
    for a in (nrm, *out['ref'].values()):
        a.setflags(write=False)
    return out


def check_body(what, points, nrm, verts, faces, c, ref, d2, face, bary):
    """All checks of one body's outputs against its reference, for ALL its queries; the largest error / bound."""
    assert d2.dtype == np.float32 and face.dtype == np.int32 and bary.dtype == np.float32
    empty = ref['face'] < 0
    assert np.all(face[empty] == -1) and np.all(np.isposinf(d2[empty])) and not bary[empty].any(), what
    hit = ~empty
    if not hit.any():
        return 0.0
    p, n, f, d, w, bound, want = points[hit], nrm[hit], face[hit], d2[hit], bary[hit], ref['bound'][hit], ref['d2'][hit]
    assert np.all((f >= 0) & (f < len(faces))), what
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(w)), what
    assert np.all(rule32(verts, faces, n, c, pairs=(np.arange(len(f)), f))), what       # the face is admissible
    err = np.abs(d.astype(np.float64) - want)
    via_face = cc.face_d2(p, verts, faces, f)
    corners = np.asarray(verts, np.float64)[np.asarray(faces)[f]]
    via_bary = ((np.asarray(p, np.float64) - (w.astype(np.float64)[:, :, None] * corners).sum(1)) ** 2).sum(1)
    assert np.all(err <= bound), (what, int(np.argmax(err / bound)), err.max())
    assert np.all(np.abs(via_face - want) <= bound), what                # the returned face attains the minimum
    assert np.all(np.abs(via_bary - d) <= bound), what                   # the weights reproduce d2
    assert np.all(w >= 0) and np.all(w <= 1) and np.all(np.abs(w.astype(np.float64).sum(1) - 1.0) <= 4 * cc.EPS32), what
    return float(max((err / bound).max(), (np.abs(via_face - want) / bound).max(), (np.abs(via_bary - d) / bound).max()))


def check_case(name, c, d2, face, bary):
    cosine = cos32(c['angle'])
    worst = 0.0
    for b in range(len(c['verts'])):
        ref = {k: v[b] for k, v in c['ref'].items()}
        worst = max(worst, check_body('%s body %d angle %g' % (name, b, c['angle']), c['points'][b], c['normals'][b],
                                      c['verts'][b], c['faces'], cosine, ref, d2[b], face[b], bary[b]))
    return worst


# ---------------------------------------------------------------------------------------------------------- threshold
def _rotate(vec, axis, angle):
    """Rodrigues: vec [..,3] rotated about the unit axis [..,3] by angle [..] (float64)."""
    ca, sa = np.cos(angle)[..., None], np.sin(angle)[..., None]
    return vec * ca + np.cross(axis, vec) * sa + axis * (axis * vec).sum(-1, keepdims=True) * (1 - ca)


THRESHOLD_VARIANTS = ('times 1 - 2^-20', 'times 1 + 2^-20', 'minus 1 degree', 'plus 1 degree')


def threshold_queries(verts_b, faces, angle, num_faces=64, seed=0):
    """(points [4 n,3], normals [4 n,3], face [4 n]): for n faces with an area, the point 1e-4 above the centroid and the
    face's unit normal rotated about its first edge by max_angle (1 - 2^-20), max_angle (1 + 2^-20), max_angle - 1 degree,
    max_angle + 1 degree (variant k of face i is row 4 i + k)."""
    rng = np.random.default_rng(seed + 3)
    v = np.asarray(verts_b, np.float64)
    faces = np.asarray(faces)
    m = face_normal64(v, faces, np.arange(len(faces)))
    good = np.nonzero(np.linalg.norm(m, axis=1) > 1e-9)[0]
    pick = np.sort(rng.choice(good, min(num_faces, len(good)), replace=False))
    tri = v[faces[pick]]
    unit = m[pick] / np.linalg.norm(m[pick], axis=1, keepdims=True)
    edge = tri[:, 1] - tri[:, 0]
    edge /= np.linalg.norm(edge, axis=1, keepdims=True)
    theta = math.radians(angle)
    angles = np.array([theta * (1 - 2.0 ** -20), theta * (1 + 2.0 ** -20), theta - math.radians(1), theta + math.radians(1)])
    points = np.repeat(tri.mean(1) + 1e-4 * unit, 4, axis=0)
    nrm = _rotate(np.repeat(unit, 4, axis=0), np.repeat(edge, 4, axis=0), np.tile(angles, len(pick)))
    return points.astype(F32), nrm.astype(F32), np.repeat(pick, 4)


# ---------------------------------------------------------------------------------------------------------- the term
def term_numpy(points, nrm, verts, faces, transl, counts, weights, rho, sigma, angle, dtype):
    """(per_body [B], floor [B], matched: list of bool arrays) of the term over the admissible-set answers in numpy of
    `dtype`: sum over the matched real points of w rho(d2) / sum over ALL real points of w -- an unmatched point adds 0
    and keeps its weight.  floor as sc.term_numpy: cc.bounds' floor on d2 carried through rho."""
    c = cos32(angle)
    per, floor, matched = [], [], []
    for b in range(len(points)):
        n = len(points[b]) if counts is None else int(min(max(counts[b], 0), len(points[b])))
        w = np.ones(n, dtype) if weights is None else np.asarray(weights[b][:n], dtype)
        q = points[b][:n] - transl[b]                       # float32 inputs: the float32 subtraction the device makes
        d2, face = statement(q, nrm[b][:n], verts[b], faces, c, dtype)
        use = (w != 0) & (face >= 0)
        matched.append(face >= 0)
        if not use.any() or float(w.sum()) == 0.0:
            per.append(dtype(0))
            floor.append(0.0)
            continue
        per.append((w[use] * sc.rho_numpy(d2[use], rho, sigma, dtype)).sum() / w.sum())
        scale = np.maximum(np.abs(np.asarray(verts[b], np.float64)).max(), np.abs(q[use].astype(np.float64)).max(1))
        f = cc.FLOOR_ULPS * cc.EPS32 * scale ** 2
        d64 = d2[use].astype(np.float64)
        change = np.maximum(sc.rho_numpy(d64 + f, rho, sigma) - sc.rho_numpy(d64, rho, sigma),
                            sc.rho_numpy(d64, rho, sigma) - sc.rho_numpy(np.maximum(d64 - f, 0), rho, sigma))
        floor.append(float((w[use].astype(np.float64) * change).sum() / float(w.astype(np.float64).sum())))
    return np.asarray(per), np.asarray(floor), matched


@functools.lru_cache(maxsize=None)
def term_case(name: str, batch: int, count: int, rho: str, angle: float = 60.0, seed: int = 0):
    """sc.term_case's inputs + normals (the four kinds in turn, of the queries points - transl) + per64 [B] and bound [B]:
    4 x the error of the float32 numpy restatement, floored as there; matched: per body which real points have a face."""
    t = sc.term_case(name, batch, count, rho, False, seed)
    nrm = []
    for b in range(batch):
        q = t['points'][b] - t['transl'][b]
        near = np.zeros(count, np.int64)
        ok = np.isfinite(q).all(1)
        near[ok] = cc.statement(q[ok], t['verts'][b], t['faces'])[1]
        nrm.append(normals(q, t['verts'][b], t['faces'], near, seed + b))
    nrm = np.stack(nrm)
    args = (t['points'], nrm, t['verts'], t['faces'], t['transl'], t['counts'], t['weights'], rho, t['sigma'], angle)
    per64, _, matched = term_numpy(*args, np.float64)
    per32, floor, _ = term_numpy(*args, np.float32)
    out = dict(t, normals=nrm, angle=angle, per64=per64, bound=np.maximum(4.0 * np.abs(per32.astype(np.float64) - per64), floor),
               matched=matched)
    nrm.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grad_case(name: str, rho: str, angle: float = 60.0):
    """sc.grad_case (interior queries, central differences of the full float64 statement) + for every query the normal of
    the face it lies above.  That face is admissible with a wide margin and is the nearest by at least 1 mm, so the
    admissible-set minimum is the plain minimum within the difference step (assert_no_decision_near_threshold)."""
    g = sc.grad_case(name, rho)
    nrm = []
    for p, t, v in zip(g['points'], g['transl'], g['verts']):
        near = cc.statement(p - t, v, g['faces'])[1]
        nrm.append(face_normal64(v, g['faces'], near))
    return dict(g, normals=np.stack(nrm).astype(F32), angle=angle)


def assert_no_decision_near_threshold(g):
    """A condition on the INPUTS of grad_case: the admissible-set answer is the plain nearest face, whose float64 cosine to
    the query's normal is 1 (the threshold is cos 60 = 0.5: no step of 1e-6 moves the decision), and sc's own margins."""
    sc.assert_interior_with_margin(g['points'], g['transl'], g['verts'], g['faces'])
    c = cos32(g['angle'])
    for p, t, v, n in zip(g['points'], g['transl'], g['verts'], g['normals']):
        q = p - t
        plain = cc.statement(q, v, g['faces'])[1]
        assert np.array_equal(statement(q, n, v, g['faces'], c)[1], plain)
        cosine = cos64(v, g['faces'], n)[np.arange(len(q)), plain]
        assert np.all(cosine > 0.999) and float(c) < 0.51
