"""The dense batch ops on the kernels of csrc/v2v.hip (pairwise distances, the packed geodesic mask, the masked nearest
vertex), csrc/winding.hip (solid angles, winding numbers, the triangle gather) and csrc/solid_angle_bwd.hip (their
adjoints)."""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from .. import _C
from ._base import _f32, _tracked, _workspace


class _PairwiseDist(torch.autograd.Function):
    """tuch/utils/contact.py:23-47 with its gradient (the reference differentiates through the matrix:
    smplify/losses.py:76-78 -> 115-116, eft/loss.py:142).  One kernel forward, one per differentiated input backward."""

    @staticmethod
    def forward(ctx, x, y, squared):
        xf, yf = _f32(x), _f32(y)
        b, nx, _ = xf.shape
        ny = yf.shape[1]
        out = torch.empty(b, nx, ny, dtype=torch.float32, device=xf.device)
        _C.check(_C.lib().tuch_batch_pairwise_dist(_C.ptr(xf), _C.ptr(yf), b, nx, ny, int(squared), _C.ptr(out),
                                                   _C.stream()))
        ctx.save_for_backward(xf, yf)
        ctx.squared = bool(squared)
        ctx.dtypes = (x.dtype, y.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        xf, yf = ctx.saved_tensors
        b, nx, _ = xf.shape
        ny = yf.shape[1]
        g = grad_out.to(torch.float32).contiguous()
        gx = torch.empty_like(xf) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(yf) if ctx.needs_input_grad[1] else None
        if gx is not None or gy is not None:
            _C.check(_C.lib().tuch_batch_pairwise_dist_bwd(_C.ptr(xf), _C.ptr(yf), _C.ptr(g), b, nx, ny, int(ctx.squared),
                                                           _C.ptr(gx), _C.ptr(gy), _C.stream()))
        return (None if gx is None else gx.to(ctx.dtypes[0]), None if gy is None else gy.to(ctx.dtypes[1]), None)


def batch_pairwise_dist(x: torch.Tensor, y: torch.Tensor, squared: bool = True) -> torch.Tensor:
    return _PairwiseDist.apply(x, y, squared)


def _solid_angles_raw(points: torch.Tensor, triangles: torch.Tensor) -> torch.Tensor:
    points, triangles = _f32(points), _f32(triangles)
    b, q, _ = points.shape
    f = triangles.shape[1]
    out = torch.empty(b, q, f, dtype=torch.float32, device=points.device)
    _C.check(_C.lib().tuch_solid_angles(_C.ptr(points), _C.ptr(triangles), b, q, f, _C.ptr(out), _C.stream()))
    return out


def _winding_numbers_raw(points: torch.Tensor, triangles: torch.Tensor, thresh: Optional[float] = None):
    points, triangles = _f32(points), _f32(triangles)
    b, q, _ = points.shape
    f = triangles.shape[1]
    L = _C.lib()
    w = torch.empty(b, q, dtype=torch.float32, device=points.device)
    ext = torch.empty(b, q, dtype=torch.uint8, device=points.device) if thresh is not None else None
    nbytes = L.tuch_winding_workspace_bytes(b, q, f)
    ws = _workspace(nbytes, points.device)
    _C.check(L.tuch_winding_numbers(_C.ptr(points), _C.ptr(triangles), b, q, f, _C.ptr(w), _C.ptr(ext),
                                    float(thresh if thresh is not None else 0.0), _C.ptr(ws), nbytes,
                                    _C.stream()))
    return (w, ext.bool()) if thresh is not None else w


class _SolidAngles(torch.autograd.Function):
    """solid_angles / winding_numbers (tuch/utils/contact.py:49-147) with their gradient: plain differentiable torch ops in the
    reference (which itself only calls them under torch.no_grad()), two adjoint kernels here (csrc/solid_angle_bwd.hip)."""

    @staticmethod
    def forward(ctx, points, triangles, winding):
        pf, tf = _f32(points), _f32(triangles)
        ctx.save_for_backward(pf, tf)
        ctx.winding = bool(winding)
        ctx.dtypes = (points.dtype, triangles.dtype)
        return _winding_numbers_raw(pf, tf) if winding else _solid_angles_raw(pf, tf)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        pf, tf = ctx.saved_tensors
        b, q, _ = pf.shape
        f = tf.shape[1]
        g = grad_out.to(torch.float32).contiguous()
        gp = torch.empty_like(pf) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(tf) if ctx.needs_input_grad[1] else None
        if gp is not None or gt is not None:
            _C.check(_C.lib().tuch_solid_angles_bwd(_C.ptr(pf), _C.ptr(tf), None if ctx.winding else _C.ptr(g),
                                                    _C.ptr(g) if ctx.winding else None, b, q, f, _C.ptr(gp), _C.ptr(gt),
                                                    _C.stream()))
        return (None if gp is None else gp.to(ctx.dtypes[0]), None if gt is None else gt.to(ctx.dtypes[1]), None)


def solid_angles(points: torch.Tensor, triangles: torch.Tensor) -> torch.Tensor:
    if _tracked(points, triangles):
        return _SolidAngles.apply(points, triangles, False)
    return _solid_angles_raw(points, triangles)


def winding_numbers(points: torch.Tensor, triangles: torch.Tensor, thresh: Optional[float] = None):
    """[B,Q,3], [B,F,3,3] -> w [B,Q] (and exterior = w <= thresh if thresh is given)."""
    if thresh is None and _tracked(points, triangles):
        return _SolidAngles.apply(points, triangles, True)
    return _winding_numbers_raw(points, triangles, thresh)


def gather_triangles(verts: torch.Tensor, faces_i32: torch.Tensor) -> torch.Tensor:
    verts = _f32(verts)
    b, v, _ = verts.shape
    f = faces_i32.shape[0]
    out = torch.empty(b, f, 3, 3, dtype=torch.float32, device=verts.device)
    _C.check(_C.lib().tuch_gather_triangles(_C.ptr(verts), _C.ptr(faces_i32), b, v, f, _C.ptr(out),
                                            _C.stream()))
    return out


def pack_geomask(geomask: torch.Tensor) -> torch.Tensor:
    """[V,V] bool on device -> bit-packed words int64 [W,V] (layout of v2v.hip)."""
    gm = geomask.to(torch.uint8).contiguous()
    v = gm.shape[0]
    L = _C.lib()
    bits = torch.empty(L.tuch_geomask_words(v), v, dtype=torch.int64, device=gm.device)
    _C.check(L.tuch_pack_geomask(_C.ptr(gm), v, _C.ptr(bits), _C.stream()))
    return bits


def v2v_min_masked(points: torch.Tensor, mask_bits_ptr, num_points: Optional[int] = None):
    """Masked nearest neighbour: [B,N,3] + packed mask -> (min_d2 [B,N] f32, argmin [B,N] int32)."""
    points = _f32(points)
    b, n, _ = points.shape
    L = _C.lib()
    mn = torch.empty(b, n, dtype=torch.float32, device=points.device)
    arg = torch.empty(b, n, dtype=torch.int32, device=points.device)
    nbytes = L.tuch_v2v_workspace_bytes(b, n)
    ws = _workspace(nbytes, points.device)
    mptr = _C.ptr(mask_bits_ptr) if isinstance(mask_bits_ptr, torch.Tensor) else mask_bits_ptr
    _C.check(L.tuch_v2v_min_masked(_C.ptr(points), mptr, b, n, _C.ptr(mn), _C.ptr(arg), _C.ptr(ws), nbytes,
                                   _C.stream()))
    return mn, arg
