"""Inputs and float64 statements shared by the scan-fit tests (tests/test_scan_fit_host.py on the CPU,
tests/test_gpu_scan_fit.py on the device).  No GPU here.

  hints          the hint contents the hinted search is tried with (the answer, a wrong face, random faces, -1, F,
                 INT32_MAX, INT32_MIN, a per-lane mix)
  term_statement the data term as torch ops in any dtype, the nearest face held fixed (cc.statement names it): the
                 per-body losses, their total and, by autograd, the gradients w.r.t. vertices, translation and points
  term_case      a mesh of closest_point_cases + queries + translations + ragged counts (+ weights); the statement in
                 float64 and the loss bound from a float32 numpy restatement
  grad_case      interior queries (cc.interior_queries: the nearest feature is locally constant) and central differences
                 of the FULL float64 statement (the nearest face found again at every displaced input)
  fit_*          the ico-6 body, three random poses + translations, noisy surface samples as the scan; the fit as a loop
                 in float64 (and float32: the yardstick): oracle.lbs.smpl_forward + cc.statement + the torch statement +
                 torch.optim.Adam
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import closest_point_cases as cc
import helpers
import lbs_cases
from oracle import lbs as ol
from synthetic import random_poses

EPS32 = cc.EPS32
RHOS = ('squared', 'distance', 'gmof')
SIGMA = 0.05                    # gmof's sigma in the tests: the queries of the cases are 0 - 0.5 m from the surface
# the rule of tests/test_gpu_closest_point.py for gradients: |err| <= GRAD_RTOL |ref| + GRAD_FLOOR max|ref|
GRAD_RTOL, GRAD_FLOOR = helpers.GRAD_RTOL, lbs_cases.GRAD_FLOOR
INT32_MAX, INT32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


# ---------------------------------------------------------------------------------------------------------- hints
HINT_KINDS = ('answer', 'wrong', 'random', 'none', 'F', 'int32_max', 'int32_min', 'mix')


def wrong_faces(points, verts, faces, answer):
    """For every query a face other than its nearest: the float64 runner-up where the mesh has one (the hardest wrong
    hint: the bound it gives is the tightest a wrong face can give), else (answer + 1) mod F -- which is the answer itself
    only on a one-face mesh."""
    faces = np.asarray(faces)
    num_faces = len(faces)
    out = (np.asarray(answer, np.int64) + 1) % num_faces
    if num_faces < 2:
        return out
    rows, cols = cc.candidates(points, verts, faces)
    p, v = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    tri = v[faces[cols]]
    d = cc.tri_d2(p[rows], tri[:, 0], tri[:, 1], tri[:, 2])
    d[cols == np.asarray(answer)[rows]] = np.inf
    best = np.full(len(p), np.inf)
    np.minimum.at(best, rows, d)
    pick = np.full(len(p), np.iinfo(np.int64).max, np.int64)
    hit = (d == best[rows]) & np.isfinite(d)
    np.minimum.at(pick, rows[hit], cols[hit])
    found = pick < num_faces
    out[found] = pick[found]
    return out


def hints(kind, points, verts, faces, answer, seed=0):
    """hint [B,Q] int32 of the kind for a batch; `answer` [B,Q] is the unhinted call's face (-1 for padding)."""
    answer = np.asarray(answer, np.int64)
    batch, count = answer.shape
    num_faces = len(faces)
    rng = np.random.default_rng(seed + 17)
    if kind == 'answer':
        out = answer
    elif kind == 'wrong':
        out = np.stack([wrong_faces(points[b], verts[b], faces, np.maximum(answer[b], 0)) for b in range(batch)])
    elif kind == 'random':
        out = rng.integers(num_faces, size=answer.shape)
    elif kind == 'mix':
        parts = [hints(k, points, verts, faces, answer, seed) for k in HINT_KINDS[:-1]]
        out = np.choose(rng.integers(len(parts), size=answer.shape), parts)
    else:
        out = np.full(answer.shape, {'none': -1, 'F': num_faces, 'int32_max': INT32_MAX, 'int32_min': INT32_MIN}[kind])
    return np.ascontiguousarray(out).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------- the term
def rho_numpy(d2, rho, sigma, dtype=np.float64):
    d2 = np.asarray(d2, dtype)
    if rho == 'squared':
        return d2
    if rho == 'distance':
        return np.sqrt(d2)
    s2 = dtype(sigma) * dtype(sigma)
    return s2 * d2 / (s2 + d2)


def rho_torch(d2, rho, sigma):
    if rho == 'squared':
        return d2
    if rho == 'distance':                   # gradient 0 at d2 = 0
        on = d2 > 0
        return torch.where(on, torch.sqrt(torch.where(on, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    s2 = float(sigma) ** 2
    return s2 * d2 / (s2 + d2)


def _tdot(a, b):
    return (a * b).sum(-1)


def _segment_d2_torch(p, s, e):
    d = e - s
    dd = _tdot(d, d)
    t = torch.where(dd > 0, _tdot(p - s, d) / torch.where(dd > 0, dd, torch.ones_like(dd)), torch.zeros_like(dd)).clamp(0, 1)
    r = p - (s + t[..., None] * d)
    return _tdot(r, r)


def tri_d2_torch(p, a, b, c):
    """cc.tri_d2 in torch ops: the minimum over the three edges taken as segments, or the distance to the plane where the
    projection falls inside a triangle with an area."""
    best = torch.minimum(torch.minimum(_segment_d2_torch(p, a, b), _segment_d2_torch(p, b, c)), _segment_d2_torch(p, c, a))
    n = torch.linalg.cross(b - a, c - a)
    nn = _tdot(n, n)
    inside = nn > 0
    for s, e in ((a, b), (b, c), (c, a)):
        inside = inside & (_tdot(n, torch.linalg.cross(e - s, p - s)) >= 0)
    h = _tdot(n, p - a)
    plane = h * h / torch.where(nn > 0, nn, torch.ones_like(nn))
    return torch.where(inside, plane, best)


def body_term_torch(points, transl, verts, faces, near, weights, rho, sigma):
    """One body's term in torch ops (any dtype, differentiable): sum_q w_q rho(d2_q) / sum_q w_q over the points given,
    d2_q to the face near[q] of the mesh posed by verts, the query being points - transl.  Points of weight 0 are left
    out before anything is computed; no points, or a weight sum of 0: 0."""
    if weights is not None:
        keep = torch.nonzero(weights != 0)[:, 0]
        points, near, w = points[keep], near[keep], weights[keep]
    if len(points) == 0:
        return verts.sum() * 0
    tri = verts[faces[near]]
    d2 = tri_d2_torch(points - transl, tri[:, 0], tri[:, 1], tri[:, 2])
    r = rho_torch(d2, rho, sigma)
    if weights is None:
        return r.sum() / len(points)
    wsum = weights.sum()
    return (w * r).sum() / wsum if float(wsum) != 0.0 else verts.sum() * 0


def nearest_faces(points, transl, verts, faces, counts, dtype=np.float64):
    """Per body the nearest face (cc.statement in `dtype`) of its real queries points - transl (formed in float32, as the
    device forms them, when the inputs are float32); list of int64 arrays."""
    out = []
    for b in range(len(points)):
        n = len(points[b]) if counts is None else int(min(max(counts[b], 0), len(points[b])))
        q = points[b][:n] - transl[b]
        ok = np.isfinite(q).all(1)
        face = np.zeros(n, np.int64)
        if ok.any():
            face[ok] = cc.statement(q[ok], verts[b], faces, dtype)[1]
        out.append(face)
    return out


def term_statement(points, verts, faces, transl, counts, weights, rho, sigma, dtype=torch.float64, near=None):
    """(per_body [B], total, g_verts [B,V,3], g_transl [B,3], g_points [B,Q,3]) as float64 numpy: the term in torch ops in
    `dtype` with the nearest face held fixed and autograd."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    if near is None:
        near = nearest_faces(points, transl, verts, faces, counts)
    p, v, tr = t(points).requires_grad_(True), t(verts).requires_grad_(True), t(transl).requires_grad_(True)
    tf = torch.as_tensor(np.asarray(faces), dtype=torch.long)
    per = []
    for b in range(len(points)):
        n = len(near[b])
        w = None if weights is None else t(weights[b][:n])
        per.append(body_term_torch(p[b, :n], tr[b], v[b], tf, torch.as_tensor(near[b]), w, rho, sigma))
    per = torch.stack(per)
    total = per.sum()
    total.backward()
    f64 = lambda x: x.detach().to(torch.float64).numpy()
    return f64(per), float(total.detach()), f64(v.grad), f64(tr.grad), f64(p.grad)


def term_numpy(points, verts, faces, transl, counts, weights, rho, sigma, dtype):
    """per_body [B] of the FULL statement (the nearest face found by cc.statement in `dtype`) in numpy of that dtype, and
    per body the floor of its bound: cc.bounds' floor on d2 (FLOOR_ULPS float32 ulps of the squared coordinate scale)
    carried through rho -- the change of rho over d2 +- that floor, averaged with the weights like the term itself."""
    per, floor = [], []
    for b in range(len(points)):
        n = len(points[b]) if counts is None else int(min(max(counts[b], 0), len(points[b])))
        w = np.ones(n, dtype) if weights is None else np.asarray(weights[b][:n], dtype)
        use = w != 0
        if not use.any() or float(w.sum()) == 0.0:
            per.append(dtype(0))
            floor.append(0.0)
            continue
        q = (points[b][:n] - transl[b])[use]                # float32 inputs: the float32 subtraction the device makes
        d2 = cc.statement(q, verts[b], faces, dtype)[0]
        per.append((w[use] * rho_numpy(d2, rho, sigma, dtype)).sum() / w.sum())
        scale = np.maximum(np.abs(np.asarray(verts[b], np.float64)).max(), np.abs(q.astype(np.float64)).max(1))
        f = cc.FLOOR_ULPS * EPS32 * scale ** 2
        d64 = d2.astype(np.float64)
        change = np.maximum(rho_numpy(d64 + f, rho, sigma) - rho_numpy(d64, rho, sigma),
                            rho_numpy(d64, rho, sigma) - rho_numpy(np.maximum(d64 - f, 0), rho, sigma))
        floor.append(float((w[use].astype(np.float64) * change).sum() / float(w.astype(np.float64).sum())))
    return np.asarray(per), np.asarray(floor)


def ragged_counts(batch, count):
    """Every body another count: all, about a quarter, about half, and round again beyond three bodies (0 and a value above
    Q have tests of their own)."""
    return np.resize(np.array([count, max(count // 4, 1), count // 2 + 1], np.int32), batch)


@functools.lru_cache(maxsize=None)
def term_case(name: str, batch: int, count: int, rho: str, weighted: bool = False, seed: int = 0):
    """dict(verts, faces, points, transl, counts, weights, rho, sigma, ref: term_statement in float64, bound [B]: per body
    4 x the error of the float32 numpy restatement, floored by the floor rule of cc.bounds carried through rho).  The
    points are cc.case's queries moved by the translation, except the one FAR away (query 4), which is pulled in: its d2 of
    1e6 would be the whole sum."""
    c = cc.case(name, batch, count, seed)
    rng = np.random.default_rng(seed + 5)
    transl = (0.1 * rng.standard_normal((batch, 3))).astype(np.float32)
    points = c['points'].copy()
    if count > 4:
        points[:, 4] = points[:, 3] + np.float32(0.3)
    points = (points + transl[:, None]).astype(np.float32)
    counts = ragged_counts(batch, count)
    weights = None
    if weighted:
        weights = (rng.random((batch, count)) + 0.1).astype(np.float32)
        weights[rng.random((batch, count)) < 0.25] = 0.0
        weights[:, 0] = 1.0
    sigma = SIGMA if rho == 'gmof' else None
    out = dict(verts=c['verts'], faces=c['faces'], points=points, transl=transl, counts=counts, weights=weights, rho=rho,
               sigma=sigma)
    out['ref'] = term_statement(points, c['verts'], c['faces'], transl, counts, weights, rho, sigma)
    per64, _ = term_numpy(points, c['verts'], c['faces'], transl, counts, weights, rho, sigma, np.float64)
    per32, floor = term_numpy(points, c['verts'], c['faces'], transl, counts, weights, rho, sigma, np.float32)
    out['bound'] = np.maximum(4.0 * np.abs(per32.astype(np.float64) - per64), floor)
    for a in (points, transl, counts, weights, out['bound']) + out['ref']:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------- gradients
def assert_interior_with_margin(points, transl, verts, faces):
    """The conditions cc.interior_queries keeps its queries by, asserted on the queries the term really forms (points -
    transl in float32): the nearest point is inside a face with every weight >= 0.1, at least 4 mm away, and the next
    face is at least 1 mm farther -- the nearest feature is constant around the query and the fixed-face gradient exact."""
    for p, t, v in zip(points, transl, verts):
        q = p - t
        d2, face = cc.statement(q, v, faces)
        w = cc.projection_weights(q.astype(np.float64), v.astype(np.float64)[np.asarray(faces)[face]])
        assert w.min() >= 0.1
        assert np.all(np.sqrt(cc.runner_up(q, v, faces)) - np.sqrt(d2) >= 1e-3)
        assert np.sqrt(d2).min() >= 4e-3


def body_total(points, transl, verts, faces, weights, rho, sigma, pairs):
    """float64: one body's term with the nearest face found again (among the candidate pairs) at these inputs; also the
    per-query terms w_q rho(d2_q) / sum w."""
    d2 = cc.statement(points - transl, verts, faces, np.float64, pairs)[0]
    w = np.ones(len(points)) if weights is None else np.asarray(weights, np.float64)
    terms = w * rho_numpy(d2, rho, sigma) / w.sum()
    return terms.sum(), terms


def central_differences(points, transl, verts, faces, weights, rho, sigma, step=1e-6):
    """Central differences of body_total w.r.t. the points [Q,3], the translation [3] and the vertices [V,3] (only the
    vertices of the nearest faces move the term)."""
    p0, t0, v0 = (np.asarray(x, np.float64) for x in (points, transl, verts))
    faces = np.asarray(faces)
    pairs = cc.candidates(p0 - t0, v0, faces)
    near = cc.statement(p0 - t0, v0, faces, np.float64, pairs)[1]
    f = lambda p, t, v: body_total(p, t, v, faces, weights, rho, sigma, pairs)
    gp, gt, gv = np.zeros_like(p0), np.zeros(3), np.zeros_like(v0)
    for k in range(3):
        d = np.zeros(3)
        d[k] = step
        gp[:, k] = (f(p0 + d, t0, v0)[1] - f(p0 - d, t0, v0)[1]) / (2 * step)       # a point moves its own term only
        gt[k] = (f(p0, t0 + d, v0)[0] - f(p0, t0 - d, v0)[0]) / (2 * step)
    for vi in np.unique(faces[near]):
        for k in range(3):
            vp, vm = v0.copy(), v0.copy()
            vp[vi, k] += step
            vm[vi, k] -= step
            gv[vi, k] = (f(p0, t0, vp)[0] - f(p0, t0, vm)[0]) / (2 * step)
    return gp, gt, gv


@functools.lru_cache(maxsize=None)
def grad_case(name: str, rho: str, batch: int = 2, count: int = 65, weighted: bool = True):
    """Interior queries above the faces of `batch` posed copies of a mesh, moved by a translation; weights in [0.5, 1.5);
    dict(..., gp, gt, gv: central differences of the full float64 statement)."""
    poses, faces = cc.mesh(name)
    verts = cc.body_batch(poses[0], batch, seed=5)
    rng = np.random.default_rng(9)
    transl = (0.1 * rng.standard_normal((batch, 3))).astype(np.float32)
    queries = np.stack([cc.interior_queries(verts[b], faces, count, seed=20 + b, height=(0.005, 0.03)) for b in range(batch)])
    points = (queries + transl[:, None]).astype(np.float32)
    weights = (0.5 + rng.random((batch, count))).astype(np.float32) if weighted else None
    sigma = SIGMA if rho == 'gmof' else None
    gp, gt, gv = zip(*[central_differences(points[b], transl[b], verts[b], faces, None if weights is None else weights[b],
                                           rho, sigma) for b in range(batch)])
    return dict(verts=verts, faces=faces, points=points, transl=transl, counts=None, weights=weights, rho=rho, sigma=sigma,
                gp=np.stack(gp), gt=np.stack(gt), gv=np.stack(gv))


def grad_within(actual, expected):
    """The gradient rule: (ok, largest error / bound)."""
    a, e = np.asarray(actual, np.float64), np.asarray(expected, np.float64)
    bound = GRAD_RTOL * np.abs(e) + GRAD_FLOOR * np.abs(e).max()
    ratio = float((np.abs(a - e) / np.maximum(bound, 1e-300)).max())
    return ratio <= 1.0, ratio


# ---------------------------------------------------------------------------------------------------------- the fit
FIT_BATCH, FIT_SEED, FIT_LR, FIT_POINTS, FIT_ITERS = 3, 77, 1e-2, 257, 60
FIT_COUNTS = (257, 64, 130)
FIT_PREFIX = 20                 # parameters before each of the first 20 updates are compared
FIT_NOISE = 2e-3
TRAJECTORY_FLOOR = 1e-4
RATIO_MARGIN = 1.25


@functools.lru_cache(maxsize=None)
def fit_inputs():
    """The ico-6 body at random_poses(3, 77) + N(0, 0.1 m) translations; the scan: FIT_POINTS random surface samples of
    each true posed body + 2 mm noise, float32, of which FIT_COUNTS are real (the rest is NaN: never to be read)."""
    body = lbs_cases.ico6_body()
    bp, go, be = random_poses(FIT_BATCH, FIT_SEED)
    m = ol.model_tensors(body, torch.float64)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    verts = ol.smpl_forward(m, t(be), t(bp), t(go))[0].numpy()
    rng = np.random.default_rng(FIT_SEED)
    shift = 0.1 * rng.standard_normal((FIT_BATCH, 3))
    faces = np.asarray(body.faces, np.int64)
    points = np.zeros((FIT_BATCH, FIT_POINTS, 3), np.float32)
    for b in range(FIT_BATCH):
        tri = verts[b][faces]
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
        f = rng.choice(len(faces), FIT_POINTS, p=area / area.sum())
        w = rng.dirichlet(np.ones(3), FIT_POINTS)
        points[b] = ((w[:, :, None] * tri[f]).sum(1) + shift[b] + FIT_NOISE * rng.standard_normal((FIT_POINTS, 3)))
        points[b, FIT_COUNTS[b]:] = np.nan
    points.setflags(write=False)
    return dict(body=body, faces=faces, points=points, counts=np.array(FIT_COUNTS, np.int32), global_orient=go,
                true_body_pose=bp, true_betas=be, true_transl=shift)


def perturbed_orient():
    """The true orientation with every body's vector moved by 0.2 rad along a random direction."""
    go = fit_inputs()['global_orient'].astype(np.float64)
    d = np.random.default_rng(FIT_SEED + 1).standard_normal(go.shape)
    return (go + 0.2 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fit_reference(num_iters: int, rho: str, fit_global_orient: bool, dtype=torch.float64):
    """The fit as a CPU loop in `dtype`: oracle.lbs.smpl_forward, the nearest face of every real point from cc.statement
    (in the numpy dtype of the same width), the torch statement of the term with that face fixed, torch.optim.Adam; the
    bodies' terms are summed.  dict of float64 numpy: params: per iteration the (body_pose, betas, transl[,
    global_orient]) BEFORE the update; loss [num_iters, B] at those parameters; final, final_loss [B]."""
    c = fit_inputs()
    m = ol.model_tensors(c['body'], dtype)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    counts, faces = c['counts'], c['faces']
    tf = torch.as_tensor(faces, dtype=torch.long)
    points = [t(c['points'][b, :counts[b]]) for b in range(FIT_BATCH)]
    sigma = SIGMA if rho == 'gmof' else None
    go = t(perturbed_orient() if fit_global_orient else c['global_orient']).requires_grad_(fit_global_orient)
    bp = torch.zeros(FIT_BATCH, 69, dtype=dtype, requires_grad=True)
    be = torch.zeros(FIT_BATCH, 10, dtype=dtype, requires_grad=True)
    with torch.no_grad():
        v0, _ = ol.smpl_forward(m, be, bp, go)
        tr = torch.stack([points[b].mean(0) for b in range(FIT_BATCH)]) - v0.mean(1)
    tr = tr.clone().requires_grad_(True)
    params = [bp, be, tr] + ([go] if fit_global_orient else [])
    opt = torch.optim.Adam(params, lr=FIT_LR)

    def terms():
        v, _ = ol.smpl_forward(m, be, bp, go)
        per = []
        for b in range(FIT_BATCH):
            q = (points[b] - tr[b]).detach().numpy().astype(npdt)
            near = cc.statement(q, v[b].detach().numpy().astype(npdt), faces, npdt)[1]
            per.append(body_term_torch(points[b], tr[b], v[b], tf, torch.as_tensor(near), None, rho, sigma))
        return torch.stack(per)
    f64 = lambda x: x.detach().to(torch.float64).numpy().copy()
    history, losses = [], []
    for _ in range(num_iters):
        history.append([f64(p) for p in params])
        opt.zero_grad()
        per = terms()
        per.sum().backward()
        opt.step()
        losses.append(f64(per))
    with torch.no_grad():
        final_loss = f64(terms())
    return dict(params=history, loss=np.stack(losses), final=[f64(p) for p in params], final_loss=final_loss)


@functools.lru_cache(maxsize=None)
def trajectory_bound(rho: str, fit_global_orient: bool):
    """(prefix, bound [prefix]): per compared iteration 4 x the largest deviation of the float32 CPU loop's parameters from
    the float64 loop's, floored at TRAJECTORY_FLOOR; the prefix is FIT_PREFIX, cut where the float32 loop itself leaves
    the floor (a face switch taken at another iteration: the yardstick is unstable from there on)."""
    r64 = fit_reference(FIT_PREFIX, rho, fit_global_orient)
    r32 = fit_reference(FIT_PREFIX, rho, fit_global_orient, torch.float32)
    dev = np.array([max(float(np.abs(a - b).max()) for a, b in zip(p32, p64)) for p32, p64 in zip(r32['params'], r64['params'])])
    holds = dev <= TRAJECTORY_FLOOR
    prefix = FIT_PREFIX if holds.all() else int(np.argmin(holds))
    return prefix, np.maximum(4.0 * dev[:prefix], TRAJECTORY_FLOOR)
