"""Inputs and statements shared by the point-cloud tests (tests/test_cloud_fit_host.py on the CPU,
tests/test_gpu_cloud_fit.py on the device).  No GPU here.

  brute_force     THE rule of include/tuch_amd.h as a numpy float32 sweep with exactly its operation order: q = x + shift,
                  d = q - s, d2 = (dx dx + dy dy) + dz dz, each product and sum rounded on its own; excluded points are
                  dropped before the sweep, argmin's first occurrence is the tie rule, tau as d2 <= f32(tau) f32(tau)
  nearest_f64     the same sweep in float64: index, d2 and the runner-up's d2
  term_statement  the model -> scan term in torch ops of any dtype, the nearest point held fixed, gradients by autograd
  term_numpy      the FULL statement (the nearest point found in that dtype) in numpy, and the floor of its bound
  cloud_case      noisy surface samples of a mesh of closest_point_cases as the clouds, the posed vertices as queries
  grad_case       queries whose nearest and second-nearest points differ by >= 1 mm, central differences of the full statement
  fit_reference   the two-sided fit as a CPU loop (oracle.lbs.smpl_forward + both statements + torch.optim.Adam)
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import closest_point_cases as cc
import lbs_cases
import scan_fit_cases as sc
from oracle import lbs as ol

EPS32 = cc.EPS32
INT32_MAX, INT32_MIN = sc.INT32_MAX, sc.INT32_MIN
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------- the search
def valid_points(points, count=None, weights=None):
    """Indices (caller's order) of the cloud's valid points: index < count, weight != 0, finite."""
    p = np.asarray(points)
    n = len(p) if count is None else int(min(max(int(count), 0), len(p)))
    keep = np.zeros(len(p), bool)
    keep[:n] = True
    if weights is not None:
        keep &= np.asarray(weights) != 0
    with np.errstate(invalid='ignore'):
        keep &= np.isfinite(p).all(1)
    return np.nonzero(keep)[0]


def brute_force(queries, points, count=None, weights=None, shift=None, tau=None, query_count=None, chunk=512):
    """(d2 [N] float32, index [N] int32) of one body by the rule, in numpy float32."""
    x = np.asarray(queries, F32)
    q = x if shift is None else (x + np.asarray(shift, F32)[None]).astype(F32)
    ids = valid_points(points, count, weights)
    s = np.asarray(points, F32)[ids]
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
            e[~np.isfinite(qq).all(1)] = np.inf
            k = e.argmin(1)                                      # the first occurrence: the smallest index among equal bits
            best = e[np.arange(len(qq)), k]
            won = np.isfinite(best)
            d2[lo:hi][won] = best[won]
            index[lo:hi][won] = ids[k[won]]
    return d2, index


def brute_force_batch(queries, points, counts=None, weights=None, shift=None, tau=None, query_counts=None):
    out = [brute_force(queries[b], points[b], None if counts is None else counts[b], None if weights is None else weights[b],
                       None if shift is None else shift[b], tau, None if query_counts is None else query_counts[b])
           for b in range(len(points))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def nearest_f64(q, points, count=None, weights=None, tau=None, chunk=512):
    """float64: (index [N] (-1: none), d2 [N], runner-up d2 [N]) of queries q (already shifted)."""
    ids = valid_points(points, count, weights)
    s = np.asarray(points, np.float64)[ids]
    q = np.asarray(q, np.float64)
    index, d2, second = np.full(len(q), -1, np.int64), np.full(len(q), np.inf), np.full(len(q), np.inf)
    if len(s) == 0:
        return index, d2, second
    for lo in range(0, len(q), chunk):
        e = ((q[lo:lo + chunk, None] - s[None]) ** 2).sum(-1)
        if tau is not None:
            e = np.where(e <= float(tau) ** 2, e, np.inf)
        k = e.argmin(1)
        rows = np.arange(len(k))
        d2[lo:lo + chunk] = e[rows, k]
        if len(s) > 1:
            e[rows, k] = np.inf
            second[lo:lo + chunk] = e.min(1)
        index[lo:lo + chunk] = np.where(np.isfinite(d2[lo:lo + chunk]), ids[k], -1)
    return index, d2, second


def surface_samples(verts_b, faces, count, seed, noise=2e-3):
    """`count` area-weighted random points of a posed mesh + N(0, noise) per coordinate, float32 [count,3]."""
    rng = np.random.default_rng(seed)
    tri = np.asarray(verts_b, np.float64)[np.asarray(faces)]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    p = area / area.sum() if area.sum() > 0 else None
    f = rng.choice(len(tri), count, p=p)
    w = rng.dirichlet(np.ones(3), count)
    return ((w[:, :, None] * tri[f]).sum(1) + noise * rng.standard_normal((count, 3))).astype(F32)


def mesh_verts(name, batch, seed=0):
    poses, faces = cc.mesh(name)
    if len(poses) >= batch:
        return np.ascontiguousarray(poses[:batch]), faces
    return np.concatenate([poses, cc.body_batch(poses[0], batch - len(poses) + 1, seed + 1)[1:]]), faces


@functools.lru_cache(maxsize=None)
def cloud_case(name: str, batch: int, num_points: int, num_queries: int, seed: int = 0):
    """dict(points [B,Q,3], queries [B,N,3], shift [B,3]): the clouds are noisy surface samples of the posed mesh, the
    queries that mesh's vertices (cycled / cut to N) minus a shift that the call adds again."""
    verts, faces = mesh_verts(name, batch, seed)
    rng = np.random.default_rng(seed + 31)
    points = np.stack([surface_samples(verts[b], faces, num_points, seed + 7 * b) for b in range(batch)])
    shift = (0.05 * rng.standard_normal((batch, 3))).astype(F32)
    pick = np.arange(num_queries) % verts.shape[1]
    queries = (verts[:, pick] + 5e-3 * rng.standard_normal((batch, num_queries, 3)) - shift[:, None]).astype(F32)
    for a in (points, queries, shift):
        a.setflags(write=False)
    return dict(points=points, queries=queries, shift=shift, verts=verts, faces=faces)


HINT_KINDS = ('answer', 'runner_up', 'random', 'none', 'Q', 'int32_max', 'int32_min', 'beyond_counts', 'zero_weight', 'mix')


def hints(kind, queries, shift, points, counts, weights, answer, seed=0):
    """hint [B,N] int32 of the kind; counts / weights as the cloud has them (beyond_counts and zero_weight need them)."""
    answer = np.asarray(answer, np.int64)
    batch, n = answer.shape
    num_points = points.shape[1]
    rng = np.random.default_rng(seed + 23)
    if kind == 'answer':
        out = answer
    elif kind == 'runner_up':
        out = answer.copy()
        for b in range(batch):
            q = (np.asarray(queries[b], F32) + (0 if shift is None else np.asarray(shift[b], F32))).astype(F32)
            ids = valid_points(points[b], None if counts is None else counts[b], None if weights is None else weights[b])
            if len(ids) > 1:
                e = ((q.astype(np.float64)[:, None] - points[b][ids].astype(np.float64)[None]) ** 2).sum(-1)
                e[np.arange(n), e.argmin(1)] = np.inf
                out[b] = ids[e.argmin(1)]
    elif kind == 'random':
        out = rng.integers(num_points, size=answer.shape)
    elif kind == 'beyond_counts':
        lo = np.full(batch, num_points - 1) if counts is None else np.minimum(np.asarray(counts, np.int64), num_points - 1)
        out = np.stack([rng.integers(lo[b], num_points, size=n) for b in range(batch)])
    elif kind == 'zero_weight':
        out = answer.copy()
        if weights is not None:
            for b in range(batch):
                zero = np.nonzero(np.asarray(weights[b]) == 0)[0]
                if len(zero):
                    out[b] = zero[rng.integers(len(zero), size=n)]
    elif kind == 'mix':
        parts = [hints(k, queries, shift, points, counts, weights, answer, seed) for k in HINT_KINDS[:-1]]
        out = np.choose(rng.integers(len(parts), size=answer.shape), parts)
    else:
        out = np.full(answer.shape, {'none': -1, 'Q': num_points, 'int32_max': INT32_MAX, 'int32_min': INT32_MIN}[kind])
    return np.ascontiguousarray(out).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------- the term
def _vertex_weights(vw, b, num_verts, dtype):
    if vw is None:
        return np.ones(num_verts, dtype)
    vw = np.asarray(vw)
    return np.asarray(vw if vw.ndim == 1 else vw[b], dtype)


def body_term_torch(verts, transl, points, index, w, rho, sigma, tau, scale, cloud_size):
    """One body's model -> scan term in torch ops (any dtype, differentiable): scale sum_v w_v rho(d2_v) / sum_v w_v;
    index [V] names the nearest point (-1: none: rho(tau^2) under tau for a cloud that is not empty, else 0, no gradient);
    vertices of weight 0 are left out before anything is computed."""
    zero = verts.sum() * 0
    wsum = w.sum()
    if cloud_size == 0 or float(wsum) == 0.0:
        return zero
    keep = torch.nonzero(w != 0)[:, 0]
    index, w, q = index[keep], w[keep], verts[keep] + transl
    won = index >= 0
    acc = zero
    if won.any():
        d = q[won] - points[index[won]]
        acc = acc + (w[won] * sc.rho_torch((d * d).sum(-1), rho, sigma)).sum()
    if tau is not None and (~won).any():
        t2 = torch.as_tensor(float(F32(tau) * F32(tau)), dtype=verts.dtype)
        acc = acc + w[~won].sum() * sc.rho_torch(t2, rho, sigma)
    return scale * acc / wsum


def nearest_indices(verts, transl, points, counts, weights, vw, tau, dtype=np.float64):
    """Per body the index [V] of every vertex's nearest valid point, found in `dtype` (-1: none or weight 0)."""
    out = []
    for b in range(len(verts)):
        q = (np.asarray(verts[b], F32) + np.asarray(transl[b], F32)[None]).astype(F32) if dtype == np.float32 else \
            np.asarray(verts[b], np.float64) + np.asarray(transl[b], np.float64)[None]
        count, w = None if counts is None else counts[b], None if weights is None else weights[b]
        if dtype == np.float32:
            idx = brute_force(q, points[b], count, w, None, tau)[1].astype(np.int64)
        else:
            ok = np.isfinite(q).all(1)
            idx = np.full(len(q), -1, np.int64)
            idx[ok] = nearest_f64(q[ok], points[b], count, w, tau)[0]
        idx[_vertex_weights(vw, b, len(q), np.float64) == 0] = -1
        out.append(idx)
    return out


def term_statement(verts, transl, points, counts, weights, vw, rho, sigma, tau=None, scale=1.0, dtype=torch.float64, index=None):
    """(per_body [B], total, g_verts [B,V,3], g_transl [B,3]) as float64 numpy, the nearest point held fixed."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    if index is None:
        index = nearest_indices(verts, transl, points, counts, weights, vw, tau)
    v = torch.tensor(np.nan_to_num(np.asarray(verts, np.float64)), dtype=dtype).requires_grad_(True)
    tr = t(transl).requires_grad_(True)
    per = []
    for b in range(len(verts)):
        size = len(valid_points(points[b], None if counts is None else counts[b], None if weights is None else weights[b]))
        w = t(_vertex_weights(vw, b, v.shape[1], np.float64))
        p = torch.tensor(np.nan_to_num(np.asarray(points[b], np.float64), posinf=0.0, neginf=0.0), dtype=dtype)
        per.append(body_term_torch(v[b], tr[b], p, torch.as_tensor(index[b]), w, rho, sigma, tau, scale, size))
    per = torch.stack(per)
    total = per.sum()
    total.backward()
    f64 = lambda x: x.detach().to(torch.float64).numpy()
    return f64(per), float(total.detach()), f64(v.grad), f64(tr.grad)


def term_numpy(verts, transl, points, counts, weights, vw, rho, sigma, tau, scale, dtype):
    """per_body [B] of the FULL statement in numpy of `dtype` (the nearest point found in that dtype by the rule's
    sequence), and per body the floor of its bound: sc.term_numpy's floor -- cc.FLOOR_ULPS float32 ulps of the squared
    coordinate scale on every d2, carried through rho and averaged with the weights like the term itself."""
    per, floor = [], []
    for b in range(len(verts)):
        ids = valid_points(points[b], None if counts is None else counts[b], None if weights is None else weights[b])
        w = _vertex_weights(vw, b, len(verts[b]), dtype)
        use = w != 0
        if len(ids) == 0 or not use.any() or float(w.sum()) == 0.0:
            per.append(dtype(0))
            floor.append(0.0)
            continue
        q = (np.asarray(verts[b], F32) + np.asarray(transl[b], F32)[None]).astype(F32)[use]     # the add the device makes
        s = np.asarray(points[b])[ids].astype(dtype)
        d = q.astype(dtype)[:, None] - s[None]
        sq = d * d
        e = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        d2 = e.min(1)
        if tau is not None:
            t2 = dtype(F32(tau) * F32(tau))
            d2 = np.where(d2 <= t2, d2, t2)
        per.append(dtype(scale) * ((w[use] * sc.rho_numpy(d2, rho, sigma, dtype)).sum() / w.sum()))
        size = np.maximum(np.abs(s.astype(np.float64)).max(), np.abs(q.astype(np.float64)).max(1))
        f = cc.FLOOR_ULPS * EPS32 * size ** 2
        d64 = d2.astype(np.float64)
        change = np.maximum(sc.rho_numpy(d64 + f, rho, sigma) - sc.rho_numpy(d64, rho, sigma),
                            sc.rho_numpy(d64, rho, sigma) - sc.rho_numpy(np.maximum(d64 - f, 0), rho, sigma))
        floor.append(float(scale) * float((w[use].astype(np.float64) * change).sum() / float(w.astype(np.float64).sum())))
    return np.asarray(per), np.asarray(floor)


TERM_TAU = 0.02


@functools.lru_cache(maxsize=None)
def term_case(name: str, rho: str, weighted: str = 'none', tau: bool = False, batch: int = 3, num_points: int = 257,
              seed: int = 0, num_verts: int = None):
    """dict(verts [B,V,3], transl, points, counts (ragged), weights=None, vw, rho, sigma, tau, scale, ref: term_statement
    in float64, bound [B]: 4 x the error of the float32 numpy restatement, floored as sc.term_case floors its bound).
    weighted: 'none', 'V' or 'BV' (a quarter of the vertex weights is 0).  num_verts: the mesh's vertices cycled / cut to
    that many queries, 5 mm of noise on each (the clouds stay samples of the mesh itself)."""
    mesh_v, faces = mesh_verts(name, batch, seed)
    verts = mesh_v
    if num_verts is not None:
        noise = 5e-3 * np.random.default_rng(seed + 43).standard_normal((batch, num_verts, 3))
        verts = (mesh_v[:, np.arange(num_verts) % mesh_v.shape[1]] + noise).astype(F32)
    rng = np.random.default_rng(seed + 41)
    transl = (0.1 * rng.standard_normal((batch, 3))).astype(F32)
    points = np.stack([surface_samples(mesh_v[b], faces, num_points, seed + 3 * b, noise=5e-3) + transl[b] for b in range(batch)])
    points = points.astype(F32)
    counts = sc.ragged_counts(batch, num_points)
    num_verts = verts.shape[1]
    vw = None
    if weighted != 'none':
        vw = (rng.random((batch, num_verts)) + 0.1).astype(F32)
        vw[rng.random((batch, num_verts)) < 0.25] = 0.0
        vw[:, 0] = 1.0
        if weighted == 'V':
            vw = vw[0]
    sigma = sc.SIGMA if rho == 'gmof' else None
    t = TERM_TAU if tau else None
    scale = 0.75
    out = dict(verts=np.ascontiguousarray(verts, F32), transl=transl, points=points, counts=counts, weights=None, vw=vw, rho=rho,
               sigma=sigma, tau=t, scale=scale, faces=faces)
    out['ref'] = term_statement(out['verts'], transl, points, counts, None, vw, rho, sigma, t, scale)
    per64, _ = term_numpy(out['verts'], transl, points, counts, None, vw, rho, sigma, t, scale, np.float64)
    per32, floor = term_numpy(out['verts'], transl, points, counts, None, vw, rho, sigma, t, scale, np.float32)
    out['bound'] = np.maximum(4.0 * np.abs(per32.astype(np.float64) - per64), floor)
    return out


# ---------------------------------------------------------------------------------------------------------- gradients
GRAD_GAP = 1e-3


def full_terms(verts, transl, points, vw, rho, sigma, scale):
    """float64: one body's per-vertex terms scale w_v rho(d2_v) / sum w with the nearest point found at these inputs."""
    q = np.asarray(verts, np.float64) + np.asarray(transl, np.float64)[None]
    d2 = nearest_f64(q, points)[1]
    w = np.ones(len(q)) if vw is None else np.asarray(vw, np.float64)
    return scale * w * sc.rho_numpy(d2, rho, sigma) / w.sum()


def central_differences(verts, transl, points, vw, rho, sigma, scale, step=1e-6):
    """Central differences of the full float64 statement w.r.t. the vertices [V,3] (a vertex moves its own term only) and
    the translation [3]."""
    v0, t0 = np.asarray(verts, np.float64), np.asarray(transl, np.float64)
    gv, gt = np.zeros_like(v0), np.zeros(3)
    for k in range(3):
        d = np.zeros(3)
        d[k] = step
        gv[:, k] = (full_terms(v0 + d, t0, points, vw, rho, sigma, scale) - full_terms(v0 - d, t0, points, vw, rho, sigma, scale)) / (2 * step)
        gt[k] = (full_terms(v0, t0 + d, points, vw, rho, sigma, scale).sum()
                 - full_terms(v0, t0 - d, points, vw, rho, sigma, scale).sum()) / (2 * step)
    return gv, gt


@functools.lru_cache(maxsize=None)
def grad_case(rho: str, batch: int = 2, num_verts: int = 65, num_points: int = 130, weighted: bool = True):
    """Clouds of scattered points (N(0, 0.5 m), decimetres apart) and queries 4 - 30 mm from one of
    them whose nearest and second-nearest points differ by at least GRAD_GAP in distance (assert_gap checks it on the
    float32 queries the term forms); weights in [0.5, 1.5); dict(..., gv, gt: central differences)."""
    rng = np.random.default_rng(13)
    transl = (0.1 * rng.standard_normal((batch, 3))).astype(F32)
    points = (0.5 * rng.standard_normal((batch, num_points, 3))).astype(F32)
    verts = np.zeros((batch, num_verts, 3), F32)
    for b in range(batch):
        got = 0
        while got < num_verts:
            s = points[b, rng.integers(num_points)].astype(np.float64)
            d = rng.standard_normal(3)
            cand = (s + d / np.linalg.norm(d) * rng.uniform(4e-3, 3e-2) - transl[b]).astype(F32)
            _, d2, second = nearest_f64((cand + transl[b]).astype(F32)[None], points[b])
            if np.sqrt(second[0]) - np.sqrt(d2[0]) >= 2 * GRAD_GAP and np.sqrt(d2[0]) >= 2e-3:
                verts[b, got] = cand
                got += 1
    vw = (0.5 + rng.random((batch, num_verts))).astype(F32) if weighted else None
    sigma = sc.SIGMA if rho == 'gmof' else None
    scale = 1.5
    gv, gt = zip(*[central_differences(verts[b], transl[b], points[b], None if vw is None else vw[b], rho, sigma, scale)
                   for b in range(batch)])
    return dict(verts=verts, transl=transl, points=points, counts=None, weights=None, vw=vw, rho=rho, sigma=sigma, tau=None,
                scale=scale, gv=np.stack(gv), gt=np.stack(gt))


def assert_gap(verts, transl, points):
    """The nearest and the second-nearest point of every query the term forms differ by >= GRAD_GAP in distance."""
    for v, t, p in zip(verts, transl, points):
        q = (np.asarray(v, F32) + np.asarray(t, F32)[None]).astype(F32)
        _, d2, second = nearest_f64(q, p)
        assert np.all(np.sqrt(second) - np.sqrt(d2) >= GRAD_GAP)
        assert np.sqrt(d2).min() >= 1e-3


# ---------------------------------------------------------------------------------------------------------- the fit
FIT_LAMBDA = 1.0


def two_sided_loop(body, points, global_orient, num_iters, rho, lam, dtype=torch.float64, body_pose0=None, lr=sc.FIT_LR,
                   fit_global_orient=False):
    """The fit as a CPU loop in `dtype`: oracle.lbs.smpl_forward, the scan -> model term (cc.statement + sc.body_term_torch)
    plus lam x the model -> scan term (the nearest real point of every vertex, found in the numpy dtype of the same
    width, held fixed), torch.optim.Adam; the bodies' terms are summed.  points: list of [n_b,3] real points per body.
    dict of float64 numpy: params per iteration BEFORE the update (body_pose, betas, transl[, global_orient]), loss
    [num_iters, B, 2] (scan -> model, lam x model -> scan) there, final, final_loss [B,2], vertices [B,V,3] (translated)."""
    m = ol.model_tensors(body, dtype)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    batch = len(points)
    faces = np.asarray(body.faces, np.int64)
    tf = torch.as_tensor(faces, dtype=torch.long)
    pts = [t(p) for p in points]
    sigma = sc.SIGMA if rho == 'gmof' else None
    go = t(global_orient).requires_grad_(fit_global_orient)
    bp = (torch.zeros(batch, 69, dtype=dtype) if body_pose0 is None else t(body_pose0)).requires_grad_(True)
    be = torch.zeros(batch, 10, dtype=dtype, requires_grad=True)
    with torch.no_grad():
        v0, _ = ol.smpl_forward(m, be, bp, go)
        tr = torch.stack([pts[b].mean(0) for b in range(batch)]) - v0.mean(1)
    tr = tr.clone().requires_grad_(True)
    params = [bp, be, tr] + ([go] if fit_global_orient else [])
    opt = torch.optim.Adam(params, lr=lr)

    def terms():
        v, _ = ol.smpl_forward(m, be, bp, go)
        per = []
        for b in range(batch):
            vb = v[b].detach().numpy().astype(npdt)
            trb = tr[b].detach().numpy().astype(npdt)
            near = cc.statement((pts[b] - tr[b]).detach().numpy().astype(npdt), vb, faces, npdt)[1]
            one = sc.body_term_torch(pts[b], tr[b], v[b], tf, torch.as_tensor(near), None, rho, sigma)
            other = one * 0
            if lam > 0:
                idx = nearest_indices(vb[None], trb[None], [points[b]], None, None, None, None, npdt)[0]
                other = body_term_torch(v[b], tr[b], pts[b], torch.as_tensor(idx), torch.ones(len(vb), dtype=dtype), rho,
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
                vertices=f64(v + tr[:, None]))


@functools.lru_cache(maxsize=None)
def fit_reference(num_iters: int, rho: str = 'distance', dtype=torch.float64, lam: float = FIT_LAMBDA):
    """two_sided_loop on sc.fit_inputs() (the ico-6 body, B = 3, Q = 257, counts 257 / 64 / 130)."""
    c = sc.fit_inputs()
    points = [c['points'][b, :c['counts'][b]] for b in range(sc.FIT_BATCH)]
    return two_sided_loop(c['body'], points, c['global_orient'], num_iters, rho, lam, dtype)


@functools.lru_cache(maxsize=None)
def trajectory_bound(rho: str = 'distance'):
    """(holds, bound [FIT_PREFIX]): whether the float32 CPU loop stays within sc.TRAJECTORY_FLOOR of the float64 loop over
    all FIT_PREFIX compared iterations, and per iteration 4 x its deviation, floored at sc.TRAJECTORY_FLOOR."""
    r64 = fit_reference(sc.FIT_PREFIX, rho)
    r32 = fit_reference(sc.FIT_PREFIX, rho, torch.float32)
    dev = np.array([max(float(np.abs(a - b).max()) for a, b in zip(p32, p64)) for p32, p64 in zip(r32['params'], r64['params'])])
    return bool((dev <= sc.TRAJECTORY_FLOOR).all()), np.maximum(4.0 * dev, sc.TRAJECTORY_FLOOR)


# ---------------------------------------------------------------------------------------------------------- what it is for
FEATURE_JOINT, FEATURE_AXIS, FEATURE_ANGLE, FEATURE_ITERS = 17, 1, 0.6, 40


@functools.lru_cache(maxsize=None)
def feature_case():
    """One ico-6 body whose scan is the true body (rest pose, its own vertices), the fit started from a pose in which one
    arm is rotated FEATURE_ANGLE rad away at the shoulder (joint 17 about y).  dict(body, points [1,V,3] float32,
    global_orient [1,3], body_pose0 [1,69], true [V,3] float64, one_sided / two_sided: the mean vertex-to-true-vertex
    distance of the float64 CPU loops after FEATURE_ITERS iterations)."""
    body = lbs_cases.ico6_body()
    m = ol.model_tensors(body, torch.float64)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    true = ol.smpl_forward(m, z(1, 10), z(1, 69), z(1, 3))[0].numpy()[0]
    points = true.astype(F32)[None]
    go = np.zeros((1, 3), F32)
    bp0 = np.zeros((1, 69), F32)
    bp0[0, 3 * (FEATURE_JOINT - 1) + FEATURE_AXIS] = FEATURE_ANGLE
    out = dict(body=body, points=points, global_orient=go, body_pose0=bp0, true=true)
    for name, lam in (('one_sided', 0.0), ('two_sided', 1.0)):
        r = two_sided_loop(body, [points[0]], go, FEATURE_ITERS, 'distance', lam, torch.float64, body_pose0=bp0)
        out[name] = float(np.linalg.norm(r['vertices'][0] - true, axis=1).mean())
    return out
