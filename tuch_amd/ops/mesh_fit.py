"""The fit to target meshes in correspondence on the kernels of csrc/mesh_fit.hip: the data term with its gradients, and
the sparse transfer between mesh topologies."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _C
from ._base import _f32, _hand_over, _need_hip, _ticket, cached_derived


class FitWeights(NamedTuple):
    """vertex_fit's weights, prepared once (fit_weights): float32 [V] on the device and their sum as a host float."""
    tensor: torch.Tensor
    total: float


def fit_weights(weights, num_verts, device) -> FitWeights:
    """Prepare per-vertex weights for vertex_fit.  The sum is taken on the host once (a raw tensor handed to vertex_fit is
    looked up in cached_derived: a loop must not read the sum back in every iteration); a zero or non-finite sum is
    refused here."""
    def build():
        w = torch.as_tensor(weights).detach()
        if w.dim() != 1 or w.shape[0] != num_verts:
            raise ValueError('vertex_fit: weights must be [%d], got %s' % (num_verts, tuple(w.shape)))
        total = float(w.to(torch.float64).sum())
        if not (np.isfinite(total) and float(np.float32(total)) != 0.0):
            raise ValueError('vertex_fit: the weights sum to %r; the term divides by that sum' % total)
        return FitWeights(w.to(device=device, dtype=torch.float32).contiguous(), total)
    if torch.is_tensor(weights):
        return cached_derived([weights], build)
    return build()


class _VertexFit(torch.autograd.Function):
    """The data term of a fit to target meshes in correspondence (tuch/utils/smplxtosmpl_mtp.py:100-101, per body) as ONE
    launch: the bodies' losses, their total and the unit gradients w.r.t. vertices and translation (csrc/mesh_fit.hip:
    vertex_fit_kernel).  backward() only hands the gradients over (scaled unless the upstream gradient is the cached
    unit seed of ops.backward_scalar)."""

    @staticmethod
    def forward(ctx, verts, transl, target, weights, weight_sum):
        v, tr, tg = _f32(verts), _f32(transl), _f32(target)
        b, nv, _ = v.shape
        dev = v.device
        lib = _C.lib()
        scratch = torch.empty(lib.tuch_vertex_fit_scratch_floats(b, nv), dtype=torch.float32, device=dev)
        loss = torch.empty(b, dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        gv = torch.empty_like(v)
        gt = torch.empty(b, 3, dtype=torch.float32, device=dev)
        _C.check(lib.tuch_vertex_fit_terms(_C.ptr(v), _C.ptr(tr), _C.ptr(tg), _C.ptr(weights), b, nv, float(weight_sum),
                                           _C.ptr(scratch), _C.ptr(_ticket(dev)), _C.ptr(loss), _C.ptr(out), _C.ptr(gv),
                                           _C.ptr(gt), _C.stream()))
        ctx.save_for_backward(gv, gt)
        ctx.in_dtypes = (verts.dtype, transl.dtype, target.dtype)
        ctx.mark_non_differentiable(loss)
        ctx.set_materialize_grads(False)        # per_body's absent gradient arrives as None, not as a zero fill per iteration
        return out[0], loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_per_body):
        return _hand_over(ctx, g, 5, lambda gv, gt: (gv, gt, -gv if ctx.needs_input_grad[2] else None))


def vertex_fit(verts, transl, target, weights=None):
    """(total, per_body): per_body[b] = sum_v w_v |verts[b,v] + transl[b] - target[b,v]| / sum_v w_v and total = their sum
    over the bodies -- the bodies are independent, so d total / d (body b's parameters) is the gradient of the reference's
    batch-1 loss ``torch.norm(target - verts, dim=2).mean()``.  verts, target [B,V,3], transl [B,3]; weights [V], a prepared
    FitWeights (fit_weights: what a loop passes) or None (all ones).  A vertex of weight 0 is skipped entirely (its target may be non-finite: a partial mesh); a weight sum of
    zero is refused.  per_body carries no gradient.  There is no host fallback."""
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise ValueError('vertex_fit: verts must be [B,V,3], got %s' % (tuple(verts.shape),))
    b, nv, _ = verts.shape
    if tuple(target.shape) != (b, nv, 3):
        raise ValueError('vertex_fit: target has shape %s, expected %s' % (tuple(target.shape), (b, nv, 3)))
    if tuple(transl.shape) != (b, 3):
        raise ValueError('vertex_fit: transl has shape %s, expected %s' % (tuple(transl.shape), (b, 3)))
    if b == 0 or nv == 0:
        raise ValueError('vertex_fit: empty input %s' % (tuple(verts.shape),))
    if weights is None:
        w, wsum = None, float(nv)
    else:
        w, wsum = weights if isinstance(weights, FitWeights) else fit_weights(weights, nv, verts.device)
        if w.shape[0] != nv:
            raise ValueError('vertex_fit: weights must be [%d], got %s' % (nv, tuple(w.shape)))
    _need_hip('vertex_fit', verts, transl, target)
    return _VertexFit.apply(verts, transl, target, w, wsum)


class TransferTable:
    """A sparse [R,N] matrix in CSR form for mesh_transfer: int32 indptr [R+1] / indices, float32 data, checked on the host
    (transfer_table) and uploaded to a device the first time it is used there."""

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data, self.shape = indptr, indices, data, (int(shape[0]), int(shape[1]))
        self._on = {}

    def on(self, device):
        key = (device.type, device.index)
        hit = self._on.get(key)
        if hit is None:
            # (an empty table still hands the kernel valid pointers)
            pad = lambda a: a if a.size else np.zeros(1, a.dtype)
            hit = self._on[key] = tuple(torch.from_numpy(pad(a)).to(device) for a in (self.indptr, self.indices, self.data))
        return hit


def transfer_table(matrix, num_src=None) -> TransferTable:
    """The table of mesh_transfer from a scipy sparse matrix, a dense [R,N] array or a CSR triple (indptr, indices, data)
    (with num_src = N; default: the largest index + 1).  Stored entries are kept in their order (a row is added up in that
    order); a dense array contributes its non-zeros.  Indices are range-checked HERE, the kernel does not."""
    if isinstance(matrix, (tuple, list)) and len(matrix) == 3:
        indptr, indices, data = (np.asarray(a) for a in matrix)
        if indptr.ndim != 1 or indices.ndim != 1 or data.ndim != 1 or indptr.size < 1:
            raise ValueError('transfer_table: (indptr, indices, data) must be one-dimensional')
        n = int(num_src) if num_src is not None else (int(indices.max()) + 1 if indices.size else 1)
    elif hasattr(matrix, 'tocsr'):
        m = matrix.tocsr()
        indptr, indices, data, n = m.indptr, m.indices, m.data, m.shape[1]
    else:
        dense = np.asarray(matrix)
        if dense.ndim != 2:
            raise ValueError('transfer_table: a dense matrix must be [R,N], got %s' % (dense.shape,))
        rows, cols = np.nonzero(dense)                     # row-major: CSR order
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=dense.shape[0]))])
        indices, data, n = cols, dense[rows, cols], dense.shape[1]
    if num_src is not None and int(num_src) != n:
        raise ValueError('transfer_table: num_src = %d, the matrix has %d columns' % (int(num_src), n))
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    r = indptr.size - 1
    if r < 1 or n < 1:
        raise ValueError('transfer_table: the matrix is empty (%d x %d)' % (r, n))
    if indptr[0] != 0 or np.any(np.diff(indptr) < 0) or indptr[-1] != indices.size or indices.size != np.asarray(data).size:
        raise ValueError('transfer_table: indptr does not describe %d entries' % indices.size)
    if indices.size >= 2 ** 31:
        raise ValueError('transfer_table: %d entries do not fit 32-bit offsets' % indices.size)
    if indices.size and (indices.min() < 0 or indices.max() >= n):
        raise ValueError('transfer_table: column indices must be in [0, %d), got [%d, %d]' % (n, indices.min(), indices.max()))
    return TransferTable(np.ascontiguousarray(indptr, np.int32), np.ascontiguousarray(indices, np.int32),
                         np.ascontiguousarray(data, np.float32), (r, n))


def mesh_transfer(table: TransferTable, verts: torch.Tensor) -> torch.Tensor:
    """table @ verts per body (tuch/utils/smplxtosmpl_mtp.py:58): verts [B,N,3] -> [B,R,3] (or [N,3] -> [R,3]), float32,
    every row added up in float32 in the table's order.  No gradient.  There is no host fallback."""
    single = verts.dim() == 2
    src = verts[None] if single else verts
    r, n = table.shape
    if src.dim() != 3 or src.shape[0] == 0 or tuple(src.shape[1:]) != (n, 3):
        raise ValueError('mesh_transfer: verts must be [B,%d,3] (or [%d,3]), got %s' % (n, n, tuple(verts.shape)))
    _need_hip('mesh_transfer', verts)
    src = _f32(src)
    indptr, indices, data = table.on(src.device)
    out = torch.empty(src.shape[0], r, 3, dtype=torch.float32, device=src.device)
    _C.check(_C.lib().tuch_mesh_transfer(_C.ptr(indptr), _C.ptr(indices), _C.ptr(data), _C.ptr(src), src.shape[0], r, n,
                                         _C.ptr(out), _C.stream()))
    return out[0] if single else out
