"""Statements shared by the k-nearest / point-normal tests (tests/test_point_normals_host.py on the CPU,
tests/test_gpu_point_normals.py on the device).  No GPU here.

  knn_brute_force  cloud_fit_cases.brute_force for the k smallest keys: the same float32 sweep, a STABLE sort of the d2 values
                   over the valid points in the caller's order (equal bits: the smaller index first), the tail -1 / +inf
  cov_f32          the neighbourhood statistics of include/tuch_amd.h in numpy float32, operation for operation
  pca_f64          the float64 scatter matrix of the same neighbours and its eigen-decomposition
  error_bound      E = (n + 256) u T, T = sum_j |d_j|^2 -- the bound csrc/point_cloud.hip derives
"""
from __future__ import annotations

import numpy as np

import cloud_fit_cases as cf

F32 = np.float32
U = 2.0 ** -24
SOLVER_C = 256.0
MAX_K = 32


def knn_brute_force(queries, points, k, count=None, weights=None, shift=None, tau=None, query_count=None, chunk=512):
    """(d2 [N,k] float32, index [N,k] int32) of one body by the rule, in numpy float32."""
    x = np.asarray(queries, F32)
    q = x if shift is None else (x + np.asarray(shift, F32)[None]).astype(F32)
    ids = cf.valid_points(points, count, weights)
    s = np.asarray(points, F32)[ids]
    n = len(q)
    d2 = np.full((n, k), np.inf, F32)
    index = np.full((n, k), -1, np.int32)
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
            order = np.argsort(e, axis=1, kind='stable')[:, :k]          # ids ascend: equal bits keep the smaller index first
            best = np.take_along_axis(e, order, 1)
            won = np.isfinite(best)
            m = order.shape[1]
            d2[lo:hi, :m] = np.where(won, best, F32(np.inf))
            index[lo:hi, :m] = np.where(won, ids[order], -1)
    return d2, index


def knn_brute_force_batch(queries, points, k, counts=None, weights=None, shift=None, tau=None, query_counts=None):
    out = [knn_brute_force(queries[b], points[b], k, None if counts is None else counts[b],
                           None if weights is None else weights[b], None if shift is None else shift[b], tau,
                           None if query_counts is None else query_counts[b]) for b in range(len(points))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def shifted(queries, shift=None):
    """q = x + shift as the device forms it."""
    x = np.asarray(queries, F32)
    return x if shift is None else (x + np.asarray(shift, F32)).astype(F32)


def cov_f32(q, s):
    """float32 mirror of the rule for one query q [3] and its n neighbours s [n,3] in key order:
    (C [6]: xx, xy, xz, yy, yz, zz; m [3]).  n = 0: zeros."""
    q, s = np.asarray(q, F32), np.asarray(s, F32).reshape(-1, 3)
    n = len(s)
    cov, m = np.zeros(6, F32), np.zeros(3, F32)
    if n == 0:
        return cov, m
    with np.errstate(over='ignore', invalid='ignore'):
        d = (s - q[None]).astype(F32)
        m = d[0].copy()
        for j in range(1, n):
            m = (m + d[j]).astype(F32)
        m = (m / F32(n)).astype(F32)
        e = (d - m[None]).astype(F32)
        for at, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            acc = F32(0)
            for j in range(n):
                acc = F32(acc + F32(e[j, a] * e[j, b]))
            cov[at] = acc
    return cov, m


def full(c6):
    c = np.asarray(c6, np.float64)
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])


def pca_f64(q, s):
    """float64: dict(cov [3,3], lam [3] ascending, normal [3] (unit, sign free), total = sum_j |d_j|^2, trace) of the
    same neighbours; every operation in float64 on the float32 inputs."""
    q, s = np.asarray(q, np.float64), np.asarray(s, np.float64).reshape(-1, 3)
    d = s - q[None]
    e = d - d.mean(0)[None]
    cov = e.T @ e
    lam, vec = np.linalg.eigh(cov)
    return dict(cov=cov, lam=lam, normal=vec[:, 0], total=float((d * d).sum()), trace=float(np.trace(cov)))


def error_bound(n, total):
    """E of csrc/point_cloud.hip: (n + 256) u sum_j |d_j|^2."""
    return (n + SOLVER_C) * U * total


def angle(a, b):
    """The angle between two directions, sign removed (float64, accurate for small angles)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), abs(float(a @ b))))


def canonical(n):
    """Is the component of the largest magnitude positive, the first among equals?"""
    n = np.asarray(n)
    return bool(n[int(np.argmax(np.abs(n)))] > 0)
