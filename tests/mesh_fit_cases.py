"""Inputs and float64 references shared by the mesh-fit tests (tests/test_mesh_fit_host.py on the CPU,
tests/test_gpu_mesh_fit.py on the device).  No GPU here.

  term_case      random point sets; the data term and its gradients by torch autograd (float64), and the error of the
                 same statement in float32 on the CPU -- the yardstick of the device's loss bound
  transfer_case  a CSR matrix with rows of 0, 1, 3 and 70 entries; the transfer as a float64 matmul
  fit_case       the ico-6 body, five random poses + a translation as targets; the fit as a float64 loop: oracle.lbs.smpl_forward
                 + torch.optim.Adam, the reference's tuch/utils/smplxtosmpl_mtp.py:78-105 with the per-body sum
"""
from __future__ import annotations

import functools

import numpy as np
import torch

import lbs_cases
from oracle import lbs as ol
from synthetic import random_poses

EPS32 = float(np.finfo(np.float32).eps)
FIT_BATCH, FIT_SEED, FIT_LR = 5, 77, 1e-2
CONVERGED = 0.03                # final loss / initial loss after 300 iterations


def term_statement(verts, transl, target, weights, dtype):
    """The term as torch ops in `dtype` with autograd: (per_body [B], total, g_verts [B,V,3], g_transl [B,3]) as float64
    numpy.  Vertices of weight 0 are left out before anything is computed (their targets may be non-finite)."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    v, tr, tg = t(verts).requires_grad_(True), t(transl).requires_grad_(True), t(target)
    if weights is None:
        per = torch.norm(tg - (v + tr[:, None]), dim=2).mean(1)            # smplxtosmpl_mtp.py:100-101, per body
    else:
        w = t(weights)
        keep = torch.nonzero(w != 0)[:, 0]
        per = (w[keep] * torch.norm(tg[:, keep] - (v[:, keep] + tr[:, None]), dim=2)).sum(1) / w.sum()
    total = per.sum()
    total.backward()
    f64 = lambda x: x.detach().to(torch.float64).numpy()
    return f64(per), float(total.detach()), f64(v.grad), f64(tr.grad)


@functools.lru_cache(maxsize=None)
def term_case(batch: int, num_verts: int, seed: int = 3, weighted: bool = False):
    """dict(verts, transl, target, weights (or None): float32; ref: term_statement in float64; bound: the loss bound)."""
    rng = np.random.default_rng(seed + 1000 * batch + num_verts)
    verts = rng.standard_normal((batch, num_verts, 3)).astype(np.float32)
    target = (verts + 0.3 * rng.standard_normal((batch, num_verts, 3))).astype(np.float32)
    transl = (0.1 * rng.standard_normal((batch, 3))).astype(np.float32)
    weights = None
    if weighted:
        weights = rng.random(num_verts).astype(np.float32) + 0.1
        weights[rng.random(num_verts) < 0.25] = 0.0
        weights[0] = 1.0
    case = dict(verts=verts, transl=transl, target=target, weights=weights)
    case['ref'] = term_statement(verts, transl, target, weights, torch.float64)
    case['bound'] = loss_bound(case)
    for a in (verts, transl, target, weights) + case['ref']:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def rel_err(actual, expected):
    """The largest relative error of the entries (the losses are positive sums: no entry is near zero)."""
    a, e = np.asarray(actual, np.float64), np.asarray(expected, np.float64)
    return float((np.abs(a - e) / np.abs(e)).max())


def loss_bound(case):
    """4 x the largest relative error of the float32 torch restatement of loss and total on the CPU against float64, the
    error floored at float32 epsilon.  The error comes from the restatement on the same inputs, not from a kernel."""
    per32, total32, _, _ = term_statement(case['verts'], case['transl'], case['target'], case['weights'], torch.float32)
    per64, total64 = case['ref'][0], case['ref'][1]
    return 4.0 * max(rel_err(per32, per64), rel_err(total32, total64), EPS32)


# ---- transfer
TRANSFER_ROW_LENGTHS = (0, 1, 3, 70)
TRANSFER_SRC = 100


@functools.lru_cache(maxsize=None)
def transfer_case(num_rows: int, batch: int, seed: int = 9):
    """Row i holds TRANSFER_ROW_LENGTHS[(i + 3) % 4] entries (row 0: 70), distinct random columns in random order, weights
    in (0, 1] normalised per row like barycentric ones.  dict(indptr, indices, data, dense, src, ref, bound)."""
    rng = np.random.default_rng(seed + 10 * num_rows + batch)
    lengths = [TRANSFER_ROW_LENGTHS[(i + 3) % 4] for i in range(num_rows)]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([rng.permutation(TRANSFER_SRC)[:n] for n in lengths]).astype(np.int64)
    data = np.concatenate([(lambda w: w / w.sum())(1.0 - rng.random(n)) for n in lengths]).astype(np.float32)
    dense = np.zeros((num_rows, TRANSFER_SRC), np.float32)
    for i in range(num_rows):
        dense[i, indices[indptr[i]:indptr[i + 1]]] = data[indptr[i]:indptr[i + 1]]
    src = rng.standard_normal((batch, TRANSFER_SRC, 3)).astype(np.float32)
    ref = np.einsum('rn,bnk->brk', dense.astype(np.float64), src.astype(np.float64))
    got32 = torch.matmul(torch.from_numpy(dense), torch.from_numpy(src)).numpy()
    # built like the term's: 4 x the float32 restatement's error, floored at epsilon -- relative to the largest entry
    # (a transferred coordinate may be arbitrarily close to zero, the entries of one mesh share a scale)
    bound = 4.0 * max(scaled_err(got32, ref), EPS32)
    return dict(indptr=indptr, indices=indices, data=data, dense=dense, src=src, ref=ref, bound=bound)


def scaled_err(actual, expected):
    a, e = np.asarray(actual, np.float64), np.asarray(expected, np.float64)
    return float(np.abs(a - e).max() / np.abs(e).max())


# ---- fit
@functools.lru_cache(maxsize=None)
def fit_inputs():
    """The fit case: targets [5,362,3] float32 = the ico-6 body at random_poses(5, 77) (pose and shape) + N(0, 0.1 m)
    translations; the true orientation is given to the fit, which starts from zero pose and betas."""
    body = lbs_cases.ico6_body()
    bp, go, be = random_poses(FIT_BATCH, FIT_SEED)
    m = ol.model_tensors(body, torch.float64)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    verts, _ = ol.smpl_forward(m, t(be), t(bp), t(go))
    shift = 0.1 * np.random.default_rng(FIT_SEED).standard_normal((FIT_BATCH, 3))
    target = (verts.numpy() + shift[:, None]).astype(np.float32)
    target.setflags(write=False)
    return dict(body=body, target=target, global_orient=go, true_body_pose=bp, true_betas=be, true_transl=shift)


def perturbed_orient():
    """The true orientation with every body's vector moved by 0.2 rad along a random direction."""
    go = fit_inputs()['global_orient'].astype(np.float64)
    d = np.random.default_rng(FIT_SEED + 1).standard_normal(go.shape)
    return (go + 0.2 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fit_reference(num_iters: int, dtype=torch.float64, fit_global_orient: bool = False):
    """The loop of smplxtosmpl_mtp.py:63-105 in `dtype` on the CPU with the per-body sum.  dict of float64 numpy:
    params: per iteration the (body_pose, betas, transl[, global_orient]) BEFORE the update; loss [num_iters, B]: the
    bodies' terms at those parameters; final: the parameters after the last update; final_loss [B] at them."""
    c = fit_inputs()
    m = ol.model_tensors(c['body'], dtype)
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    target = t(c['target'])
    go = t(perturbed_orient() if fit_global_orient else c['global_orient']).requires_grad_(fit_global_orient)
    bp = torch.zeros(FIT_BATCH, 69, dtype=dtype, requires_grad=True)
    be = torch.zeros(FIT_BATCH, 10, dtype=dtype, requires_grad=True)
    with torch.no_grad():
        v0, _ = ol.smpl_forward(m, be, bp, go)
        tr = (target.mean(1) - v0.mean(1)).clone()                     # :70-71
    tr.requires_grad_(True)
    params = [bp, be, tr] + ([go] if fit_global_orient else [])
    opt = torch.optim.Adam(params, lr=FIT_LR)                          # :82-85

    def terms():
        v, _ = ol.smpl_forward(m, be, bp, go)
        return torch.norm(target - (v + tr[:, None]), dim=2).mean(1)   # :100-101, one term per body
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
