"""Restatements and inputs shared by the oriented point-cloud tests (tests/test_oriented_cloud_host.py on the CPU,
tests/test_gpu_oriented_cloud.py on the device).  No GPU here.

  vertex_normals32   tuch_vertex_normals' rule as an explicit numpy float32 loop in table order: m of every face by
                     oriented_point_cases.face_normals32 (the sequence of tuch_closest_point with normals), u = ((0 + m_1) +
                     m_2) + ..., normalize: / sqrt(uu) with a zero row where uu is 0 or not finite
  vertex_normals64   the same sums in float64
  pair_rule32        THE admissibility of (query normal, point normal) pairs in numpy float32, op for op
  pair_cos64         the float64 cosine of the pairs
  brute_force        cloud_fit_cases.brute_force over the admissible valid points
  cloud_case         clouds sampled from a mesh with normals of four kinds, queries near its vertices with normals of four kinds
  threshold_case     queries whose normal is max_angle (1 +- 2^-20) or +- 1 degree away from their nearest point's
  oriented_loop      the two-sided fit with the model -> scan match restricted to compatible normals, as a CPU loop
  front_scan         the front-only scan of the ico-6 body the feature is for
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import closest_point_cases as cc
import cloud_fit_cases as cf
import lbs_cases
import oriented_point_cases as op
import scan_fit_cases as sc
from oracle import lbs as ol

F32 = np.float32
ANGLES = op.ANGLES
KINDS = ('true', 'flipped', 'random', 'zero')
cos32 = op.cos32


def vertex_table(faces, num_verts):
    """ops.vertex_face_table restated: (off [V+1], ids [3F]), vertex v's faces ascending (a face that names v twice twice)."""
    faces = np.asarray(faces, np.int64)
    lists = [[] for _ in range(num_verts)]
    for f, tri in enumerate(faces):
        for v in tri:
            lists[v].append(f)
    off = np.zeros(num_verts + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    return off, np.asarray([f for l in lists for f in l], np.int32)


def sq32(a):
    a = np.asarray(a, F32)
    return ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]).astype(F32)


def vertex_normals32(verts, faces, off, ids, normalize=False):
    """[V,3] float32 of one body by the rule: an explicit loop in table order."""
    v = np.asarray(verts, F32)
    with np.errstate(over='ignore', invalid='ignore', under='ignore', divide='ignore'):
        m, _ = op.face_normals32(v, faces)
        out = np.zeros((len(v), 3), F32)
        for i in range(len(v)):
            u = np.zeros(3, F32)
            for j in range(off[i], off[i + 1]):
                u = (u + m[ids[j]]).astype(F32)
            out[i] = u
        if normalize:
            uu = sq32(out)
            known = (uu > 0) & np.isfinite(uu)
            length = np.sqrt(uu).astype(F32)
            out = np.where(known[:, None], (out / np.where(known, length, F32(1))[:, None]).astype(F32), F32(0))
    assert out.dtype == F32
    return out


def vertex_normals64(verts, faces, off, ids):
    v = np.asarray(verts, np.float64)
    tri = v[np.asarray(faces)]
    m = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    out = np.zeros((len(v), 3))
    for i in range(len(v)):
        out[i] = m[ids[off[i]:off[i + 1]]].sum(0) if off[i + 1] > off[i] else 0.0
    return out


def pair_rule32(u, n, c, diagonal=False):
    """admissible [N,M] bool (diagonal: [N] for the pairs (u_i, n_i)) under the float32 rule with threshold cosine c."""
    u, n = np.asarray(u, F32), np.asarray(n, F32)
    c = F32(c)
    c2 = c * c
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        uu, nn = sq32(u), sq32(n)
        free_u, free_n = ~((uu > 0) & (uu < np.inf)), ~((nn > 0) & (nn < np.inf))
        if diagonal:
            s = (u[:, 0] * n[:, 0] + u[:, 1] * n[:, 1]) + u[:, 2] * n[:, 2]
            assert s.dtype == F32
            return ((s > 0) & (s * s >= c2 * (uu * nn))) | free_u | free_n
        s = (u[:, None, 0] * n[None, :, 0] + u[:, None, 1] * n[None, :, 1]) + u[:, None, 2] * n[None, :, 2]
        assert s.dtype == F32
        ok = (s > 0) & (s * s >= c2 * (uu[:, None] * nn[None]))
    return ok | free_u[:, None] | free_n[None]


def pair_cos64(u, n):
    """float64 cosine of the angle of every (u_i, n_j) pair [N,M]; NaN where either has no length."""
    u, n = np.asarray(u, np.float64), np.asarray(n, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return (u @ n.T) / (np.linalg.norm(u, axis=1)[:, None] * np.linalg.norm(n, axis=1)[None])


def brute_force(queries, query_normals, points, normals, c, count=None, weights=None, shift=None, tau=None, query_count=None,
                chunk=256):
    """(d2 [N] float32, index [N] int32) of one body: cf.brute_force's sweep over the admissible valid points."""
    x = np.asarray(queries, F32)
    q = x if shift is None else (x + np.asarray(shift, F32)[None]).astype(F32)
    ids = cf.valid_points(points, count, weights)
    s = np.asarray(points, F32)[ids]
    nrm = np.asarray(normals, F32)[ids]
    n = len(q)
    d2 = np.full(n, np.inf, F32)
    index = np.full(n, -1, np.int32)
    real = n if query_count is None else int(min(max(int(query_count), 0), n))
    if len(s) == 0:
        return d2, index
    limit = F32(np.inf) if tau is None else F32(tau) * F32(tau)
    with np.errstate(over='ignore', invalid='ignore'):
        for lo in range(0, real, chunk):
            hi = min(lo + chunk, real)
            qq = q[lo:hi]
            d = (qq[:, None, :] - s[None, :, :]).astype(F32)
            sq = (d * d).astype(F32)
            e = ((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32)
            e = np.where(np.isfinite(e) & (e <= limit), e, F32(np.inf))
            e = np.where(pair_rule32(np.asarray(query_normals, F32)[lo:hi], nrm, c), e, F32(np.inf))
            e[~np.isfinite(qq).all(1)] = np.inf
            k = e.argmin(1)
            best = e[np.arange(len(qq)), k]
            won = np.isfinite(best)
            d2[lo:hi][won] = best[won]
            index[lo:hi][won] = ids[k[won]]
    return d2, index


def brute_force_batch(queries, query_normals, points, normals, c, counts=None, weights=None, shift=None, tau=None,
                      query_counts=None):
    out = [brute_force(queries[b], query_normals[b], points[b], normals[b], c, None if counts is None else counts[b],
                       None if weights is None else weights[b], None if shift is None else shift[b], tau,
                       None if query_counts is None else query_counts[b]) for b in range(len(points))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---------------------------------------------------------------------------------------------------------- the inputs
def oriented_samples(verts_b, faces, count, seed, noise=2e-3):
    """(points [count,3] float32, unit normals [count,3] float64): cf.surface_samples with the normal of the sampled face."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(verts_b, np.float64)[np.asarray(faces)]
    m = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = 0.5 * np.linalg.norm(m, axis=1)
    f = rng.choice(len(tri), count, p=area / area.sum())
    w = rng.dirichlet(np.ones(3), count)
    pts = ((w[:, :, None] * tri[f]).sum(1) + noise * rng.standard_normal((count, 3))).astype(F32)
    return pts, m[f] / np.maximum(np.linalg.norm(m[f], axis=1, keepdims=True), 1e-300)


def mixed_normals(true, kinds, seed):
    """[n,3] float32: row i is true_i, -true_i, a random unit vector or a zero row, as KINDS[(i + seed) % 4] is in `kinds`
    (a kind left out gives way to 'true')."""
    rng = np.random.default_rng(seed + 57)
    rand = rng.standard_normal(true.shape)
    rand /= np.linalg.norm(rand, axis=1, keepdims=True)
    kind = (np.arange(len(true)) + seed) % 4
    use = np.array([KINDS[k] in kinds for k in range(4)])[kind]
    kind = np.where(use, kind, 0)[:, None]
    return np.where(kind == 0, true, np.where(kind == 1, -true, np.where(kind == 2, rand, 0.0))).astype(F32)


@functools.lru_cache(maxsize=None)
def cloud_case(name: str, batch: int, num_points: int, num_queries: int, kinds=KINDS, query_kinds=KINDS, seed: int = 0):
    """dict(points [B,Q,3], normals [B,Q,3], queries [B,N,3], query_normals [B,N,3], shift [B,3], verts, faces): the clouds
    are noisy surface samples of the posed mesh with their faces' normals (kinds in turn), the queries the mesh's
    vertices (cycled / cut to N, 5 mm of noise) with the raw area-weighted vertex normals (kinds in turn; uu about
    1e-7: the rule is scale-free)."""
    verts, faces = cf.mesh_verts(name, batch, seed)
    rng = np.random.default_rng(seed + 31)
    pts, nrm, qn = [], [], []
    off, ids = vertex_table(faces, verts.shape[1])
    pick = np.arange(num_queries) % verts.shape[1]
    for b in range(batch):
        p, m = oriented_samples(verts[b], faces, num_points, seed + 7 * b)
        pts.append(p)
        nrm.append(mixed_normals(m, kinds, seed + b))
        qn.append(mixed_normals(vertex_normals64(verts[b], faces, off, ids)[pick], query_kinds, seed + b + 2))
    shift = (0.05 * rng.standard_normal((batch, 3))).astype(F32)
    queries = (verts[:, pick] + 5e-3 * rng.standard_normal((batch, num_queries, 3)) - shift[:, None]).astype(F32)
    out = dict(points=np.stack(pts), normals=np.stack(nrm), queries=queries, query_normals=np.stack(qn), shift=shift,
               verts=verts, faces=faces)
    for a in out.values():
        a.setflags(write=False)
    return out


def _rotate(vec, axis, angle):
    axis = axis / np.linalg.norm(axis)
    return vec * math.cos(angle) + np.cross(axis, vec) * math.sin(angle) + axis * (axis @ vec) * (1 - math.cos(angle))


THRESHOLD_VARIANTS = ('times 1 - 2^-20', 'times 1 + 2^-20', 'minus 1 degree', 'plus 1 degree')


@functools.lru_cache(maxsize=None)
def threshold_case(angle: float, num_points: int = 257, seed: int = 0):
    """One body: a cloud of the icosphere's samples with true normals; query 4 i + k sits 1 mm off point i along its normal
    and carries that normal rotated by THRESHOLD_VARIANTS[k] of `angle` about a random axis perpendicular to it."""
    verts, faces = cf.mesh_verts('icosphere', 1, seed)
    pts, m = oriented_samples(verts[0], faces, num_points, seed + 3, noise=0.0)
    rng = np.random.default_rng(seed + 91)
    theta = math.radians(angle)
    turns = (theta * (1 - 2.0 ** -20), theta * (1 + 2.0 ** -20), theta - math.radians(1), theta + math.radians(1))
    queries, qn = [], []
    for i in range(64):
        axis = np.cross(m[i], rng.standard_normal(3))
        for t in turns:
            queries.append(pts[i].astype(np.float64) + 1e-3 * m[i])
            qn.append(_rotate(m[i], axis, t) * rng.uniform(0.5, 2.0))
    return dict(points=pts[None], normals=m.astype(F32)[None], queries=np.asarray(queries, F32)[None],
                query_normals=np.asarray(qn, F32)[None])


# ---------------------------------------------------------------------------------------------------------- the term
def oriented_indices(verts, transl, points, normals, faces, c, counts, weights, vw, tau, dtype=np.float32):
    """Per body the index [V] of every vertex's nearest ADMISSIBLE valid point.  The admissible set is the float32 rule's
    on vertex_normals32's raw rows; the nearest point within it is found in `dtype` (-1: none or weight 0)."""
    off, ids = vertex_table(faces, np.asarray(verts).shape[1])
    out = []
    for b in range(len(verts)):
        u = vertex_normals32(verts[b], faces, off, ids)
        count, w = None if counts is None else counts[b], None if weights is None else weights[b]
        if dtype == np.float32:
            idx = brute_force(verts[b], u, points[b], normals[b], c, count, w, transl[b], tau)[1].astype(np.int64)
        else:
            q = (np.asarray(verts[b], F32) + np.asarray(transl[b], F32)[None]).astype(np.float64)
            keep = cf.valid_points(points[b], count, w)
            adm = pair_rule32(u, np.asarray(normals[b], F32)[keep], c)
            e = ((q[:, None] - np.asarray(points[b], np.float64)[keep][None]) ** 2).sum(-1)
            if tau is not None:
                e = np.where(e <= float(F32(tau) * F32(tau)), e, np.inf)
            e = np.where(adm, e, np.inf)
            e[~np.isfinite(q).all(1)] = np.inf
            k = e.argmin(1) if len(keep) else np.zeros(len(q), np.int64)
            idx = np.where(np.isfinite(e[np.arange(len(q)), k]), keep[k], -1) if len(keep) else np.full(len(q), -1, np.int64)
        idx[cf._vertex_weights(vw, b, len(idx), np.float64) == 0] = -1
        out.append(idx)
    return out


@functools.lru_cache(maxsize=None)
def term_case(name: str, rho: str, weighted: str = 'none', tau: bool = False, angle: float = 60.0):
    """cf.term_case(name, rho, weighted, tau) + normals [B,Q,3] (the kinds in turn) + angle + ref: cf.term_statement in
    float64 over the float32 admissible set; the bound is the unoriented case's (the same points, distances and sums)."""
    t = dict(cf.term_case(name, rho, weighted, tau))
    verts, faces = t['verts'], t['faces']
    batch, num_points = t['points'].shape[:2]
    nrm = []
    for b in range(batch):
        # the normal of the nearest face of every point: the cloud is noisy samples of this mesh moved by transl
        face = cc.statement((t['points'][b] - t['transl'][b]).astype(np.float64), verts[b], faces)[1]
        m = op.face_normal64(verts[b], faces, np.minimum(face, len(faces) - 1))
        nrm.append(mixed_normals(m / np.maximum(np.linalg.norm(m, axis=1, keepdims=True), 1e-300), KINDS, b))
    t['normals'] = np.stack(nrm)
    t['angle'] = angle
    c = cos32(angle)
    t['index32'] = oriented_indices(verts, t['transl'], t['points'], t['normals'], faces, c, t['counts'], None, t['vw'], t['tau'])
    index64 = oriented_indices(verts, t['transl'], t['points'], t['normals'], faces, c, t['counts'], None, t['vw'], t['tau'],
                               np.float64)
    t['ref'] = cf.term_statement(verts, t['transl'], t['points'], t['counts'], None, t['vw'], rho, t['sigma'], t['tau'],
                                 t['scale'], index=index64)
    return t


# ---------------------------------------------------------------------------------------------------------- the fit
def oriented_loop(body, points, normals, global_orient, num_iters, rho, lam, angle, oriented, dtype=torch.float64,
                  body_pose0=None, lr=sc.FIT_LR, scan_oriented=True):
    """cf.two_sided_loop with normals: the scan -> model term matches a point only to faces within `angle` of its normal
    (op.statement; scan_oriented False: cc.statement), and with `oriented` the model -> scan term matches a vertex only
    to points whose normal is within `angle` of the vertex's (vertex_normals32 + pair_rule32: the float32 admissible
    set in either dtype, the nearest point within it found in the loop's dtype).  A point or vertex left without a match
    adds nothing and keeps its weight in the normaliser.  Returns two_sided_loop's dict + matched [B]: the share of
    vertices with a match at the final evaluation."""
    m = ol.model_tensors(body, dtype)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    batch = len(points)
    faces = np.asarray(body.faces, np.int64)
    tf = torch.as_tensor(faces, dtype=torch.long)
    pts = [t(p) for p in points]
    c = cos32(angle)
    sigma = sc.SIGMA if rho == 'gmof' else None
    go = t(global_orient)
    bp = (torch.zeros(batch, 69, dtype=dtype) if body_pose0 is None else t(body_pose0)).requires_grad_(True)
    be = torch.zeros(batch, 10, dtype=dtype, requires_grad=True)
    with torch.no_grad():
        v0, _ = ol.smpl_forward(m, be, bp, go)
        tr = torch.stack([pts[b].mean(0) for b in range(batch)]) - v0.mean(1)
    tr = tr.clone().requires_grad_(True)
    params = [bp, be, tr]
    opt = torch.optim.Adam(params, lr=lr)
    matched = np.zeros(batch)

    def terms():
        v, _ = ol.smpl_forward(m, be, bp, go)
        per = []
        for b in range(batch):
            vb = v[b].detach().numpy().astype(npdt)
            trb = tr[b].detach().numpy().astype(npdt)
            q = (pts[b] - tr[b]).detach().numpy().astype(npdt)
            if scan_oriented:
                near = op.statement(q, normals[b], vb, faces, c, npdt)[1]
            else:
                near = cc.statement(q, vb, faces, npdt)[1]
            hit = torch.as_tensor(near >= 0)
            one = v[b].sum() * 0
            if hit.any():
                one = sc.body_term_torch(pts[b][hit], tr[b], v[b], tf, torch.as_tensor(near)[hit], None, rho, sigma) * (
                    float(hit.sum()) / len(near))
            other = one * 0
            if lam > 0:
                if oriented:
                    idx = oriented_indices(vb.astype(F32)[None], trb.astype(F32)[None], [points[b]], [normals[b]], faces, c, None,
                                           None, None, None, npdt)[0]
                else:
                    idx = cf.nearest_indices(vb[None], trb[None], [points[b]], None, None, None, None, npdt)[0]
                matched[b] = float((idx >= 0).mean())
                other = cf.body_term_torch(v[b], tr[b], pts[b], torch.as_tensor(idx), torch.ones(len(vb), dtype=dtype), rho,
                                           sigma, None, lam, len(points[b]))
            per.append(torch.stack([one, other]))
        return torch.stack(per), v
    f64 = lambda x: x.detach().to(torch.float64).numpy().copy()
    history, losses = [], []
    for _ in range(num_iters):
        history.append([f64(p) for p in params])
        opt.zero_grad()
        per, _ = terms()
        per.sum().backward()
        opt.step()
        losses.append(f64(per))
    with torch.no_grad():
        per, v = terms()
    return dict(params=history, loss=np.stack(losses) if losses else None, final=[f64(p) for p in params], final_loss=f64(per),
                vertices=f64(v + tr[:, None]), matched=matched.copy())


FEATURE_ANGLE, FEATURE_ITERS = 60.0, 40
FEATURE_VIEWPOINT = (0.0, 0.0, 3.0)


@functools.lru_cache(maxsize=None)
def front_scan():
    """The ico-6 body in rest pose seen from a sensor on +z: dict(body, true [V,3] float64, points [1,Q,3] float32: its
    vertices whose (float32-rule) normal has a positive z, normals [1,Q,3]: those normals normalised, global_orient)."""
    body = lbs_cases.ico6_body()
    m = ol.model_tensors(body, torch.float64)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    true = ol.smpl_forward(m, z(1, 10), z(1, 69), z(1, 3))[0].numpy()[0]
    faces = np.asarray(body.faces, np.int64)
    off, ids = vertex_table(faces, len(true))
    u = vertex_normals32(true.astype(F32), faces, off, ids, normalize=True)
    front = u[:, 2] > 0
    return dict(body=body, true=true, faces=faces, points=true.astype(F32)[front][None], normals=u[front][None],
                global_orient=np.zeros((1, 3), F32), front=front)


@functools.lru_cache(maxsize=None)
def feature_loops(num_iters: int = FEATURE_ITERS, dtype=torch.float64):
    """Mean vertex-to-true-vertex distance after num_iters iterations of the CPU loops on front_scan(), started at the true
    pose: dict(one_sided, two_sided, oriented, matched: the oriented loop's share of matched vertices)."""
    s = front_scan()
    out = {}
    for name, lam, oriented in (('one_sided', 0.0, False), ('two_sided', 1.0, False), ('oriented', 1.0, True)):
        r = oriented_loop(s['body'], [s['points'][0]], [s['normals'][0]], s['global_orient'], num_iters, 'distance', lam,
                          FEATURE_ANGLE, oriented, dtype)
        out[name] = float(np.linalg.norm(r['vertices'][0] - s['true'], axis=1).mean())
        if oriented:
            out['matched'] = float(r['matched'][0])
    return out


TRAJECTORY_PREFIX = 10


@functools.lru_cache(maxsize=None)
def trajectory(dtype=torch.float64):
    """oriented_loop (oriented) on front_scan() over TRAJECTORY_PREFIX iterations."""
    s = front_scan()
    return oriented_loop(s['body'], [s['points'][0]], [s['normals'][0]], s['global_orient'], TRAJECTORY_PREFIX, 'distance', 1.0,
                         FEATURE_ANGLE, True, dtype)


@functools.lru_cache(maxsize=None)
def trajectory_bound():
    """(holds, bound [TRAJECTORY_PREFIX]): whether the float32 CPU loop stays within sc.TRAJECTORY_FLOOR of the float64 loop,
    and per iteration 4 x its deviation, floored at sc.TRAJECTORY_FLOOR."""
    r64, r32 = trajectory(), trajectory(torch.float32)
    dev = np.array([max(float(np.abs(a - b).max()) for a, b in zip(p32, p64)) for p32, p64 in zip(r32['params'], r64['params'])])
    return bool((dev <= sc.TRAJECTORY_FLOOR).all()), np.maximum(4.0 * dev, sc.TRAJECTORY_FLOOR)
