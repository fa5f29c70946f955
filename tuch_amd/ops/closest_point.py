"""The closest point of a posed mesh (csrc/closest_point.hip) and the point-to-surface data term over it
(csrc/scan_fit.hip).  ``model`` is a ContactModel (model.py, which imports this module for its closest_point method)."""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch.autograd.function import once_differentiable

from .. import _C
from . import args
from ._base import _f32, _hand_over, _need_hip, _ticket, _workspace, deterministic


class ClosestPoint(NamedTuple):
    d2: torch.Tensor
    face: torch.Tensor
    bary: torch.Tensor


class _ClosestPoint(torch.autograd.Function):
    """ContactModel.closest_point: tuch_closest_point forward (hint, and normals with their cosine, or None),
    tuch_closest_point_bwd (the envelope form) backward."""

    @staticmethod
    def forward(ctx, verts, points, model: ContactModel, counts, hint, normals, cos):
        v, pts = _f32(verts), _f32(points)
        b, q, _ = pts.shape
        L = _C.lib()
        d2 = torch.empty(b, q, dtype=torch.float32, device=pts.device)
        face = torch.empty(b, q, dtype=torch.int32, device=pts.device)
        bary = torch.empty(b, q, 3, dtype=torch.float32, device=pts.device)
        nbytes = L.tuch_closest_point_workspace_bytes(model._handle, b, q, normals is not None)
        ws = _workspace(nbytes, pts.device)
        if b and q:
            _C.check(L.tuch_closest_point(model._handle, _C.ptr(v), _C.ptr(pts), _C.ptr(normals), cos or 0.0, _C.ptr(counts),
                                          _C.ptr(hint), b, q, _C.ptr(d2), _C.ptr(face), _C.ptr(bary), _C.ptr(ws), nbytes,
                                          _C.stream()))
        ctx.save_for_backward(v, pts, face, bary)
        ctx.model = model
        ctx.mark_non_differentiable(face, bary)
        return d2, face, bary

    @staticmethod
    def backward(ctx, grad_d2, _grad_face, _grad_bary):
        v, pts, face, bary = ctx.saved_tensors
        b, q, _ = pts.shape
        want_v, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        rest = (None,) * 5
        if b == 0 or q == 0 or not (want_v or want_p):
            return ((torch.zeros_like(v) if want_v else None), (torch.zeros_like(pts) if want_p else None)) + rest
        g = grad_d2.to(torch.float32).contiguous()
        gp = torch.empty_like(pts) if want_p else None
        gv = fixed = None
        if want_v and deterministic():
            fixed = torch.zeros(v.numel(), dtype=torch.int64, device=v.device)
            gv = torch.empty_like(v)
        elif want_v:
            gv = torch.zeros_like(v)
        _C.check(_C.lib().tuch_closest_point_bwd(ctx.model._handle, _C.ptr(v), _C.ptr(pts), _C.ptr(face), _C.ptr(bary),
                                                 _C.ptr(g), b, q, _C.ptr(gp), _C.ptr(fixed), _C.ptr(gv), _C.stream()))
        return (gv, gp) + rest


class _ScanFit(torch.autograd.Function):
    """ops.scan_fit: the search, the term and the unit gradients in one C call (csrc/scan_fit.hip: tuch_scan_fit_terms).
    `face` [B,Q] int32 is written in place (it may be the hint tensor).  backward() only hands the gradients over (scaled
    unless the upstream gradient is the cached unit seed of ops.backward_scalar)."""

    @staticmethod
    def forward(ctx, verts, transl, points, model: ContactModel, counts, weights, hint, rho, sigma, face, normals, cos):
        v, tr, pts = _f32(verts), _f32(transl), _f32(points)
        b, q, _ = pts.shape
        dev = pts.device
        L = _C.lib()
        d2 = torch.empty(b, q, dtype=torch.float32, device=dev)
        bary = torch.empty(b, q, 3, dtype=torch.float32, device=dev)
        per_body = torch.empty(b, dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        gv = torch.empty_like(v)
        gt = torch.empty(b, 3, dtype=torch.float32, device=dev)
        gp = torch.empty_like(pts) if ctx.needs_input_grad[2] else None
        nbytes = L.tuch_scan_fit_workspace_bytes(model._handle, b, q, normals is not None)
        ws = _workspace(nbytes, dev)
        _C.check(L.tuch_scan_fit_terms(
            model._handle, _C.ptr(v), _C.ptr(tr), _C.ptr(pts), _C.ptr(normals), cos or 0.0, _C.ptr(counts), _C.ptr(weights),
            _C.ptr(hint), b, q, rho, sigma, _C.ptr(d2), _C.ptr(face), _C.ptr(bary), _C.ptr(_ticket(dev)), _C.ptr(per_body),
            _C.ptr(out), _C.ptr(gv), _C.ptr(gt), _C.ptr(gp), _C.ptr(ws), nbytes, _C.stream()))
        ctx.save_for_backward(gv, gt, gp)
        ctx.in_dtypes = (verts.dtype, transl.dtype, points.dtype)
        ctx.mark_non_differentiable(per_body, d2, bary)
        ctx.set_materialize_grads(False)        # the other outputs' absent gradients arrive as None, not as zero fills
        return out[0], per_body, d2, bary

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_others):
        return _hand_over(ctx, g, 12)


def scan_fit(model: ContactModel, verts, transl, points, counts=None, weights=None, hint=None, rho='distance', sigma=None,
             face_out=None, normals=None, max_angle=None):
    """Point-to-surface data term of a fit to unregistered points: ``(total, per_body, ClosestPoint)``.  The queries are
    ``points[b,q] - transl[b]`` against ``model``'s mesh posed by ``verts[b]``; the ClosestPoint has the bits of
    ``model.closest_point(verts, points - transl[:, None], counts, hint)``.  per_body[b] = sum_q w_q rho(d2_q) / sum_q w_q
    over the body's real points (counts [B]) and total = their sum over the bodies -- the bodies are independent, as in
    vertex_fit.  rho: 'squared' (d2), 'distance' (sqrt d2, gradient 0 at d2 = 0) or 'gmof' (sigma^2 d2 / (sigma^2 + d2),
    needs sigma).  weights [B,Q] or None; a point of weight 0 is never computed from (it may be non-finite); a body whose
    weights sum to 0 or with counts[b] = 0 has loss 0 and zero gradient rows.  total is differentiable w.r.t. verts,
    transl and points with the weights of the nearest point held fixed; the sums into the vertex rows are 64-bit
    fixed-point under ``deterministic()`` and float atomics otherwise, every per-body sum is fixed-order in both modes.
    hint [B,Q] int32 as in ``closest_point``; face_out: a contiguous int32 [B,Q] tensor to receive the faces -- it may be
    the hint tensor itself (a loop's memory of its last answer).
    normals [B,Q,3] with max_angle in degrees, in (0, 90], as in ``closest_point``: the search is the normal-compatible
    one (tuch_scan_fit_terms with normals); normals are not translated and get no gradient.  A real point without an
    admissible face (face = -1) adds 0 to the loss and to every gradient and keeps its weight in the normaliser.  Both or
    neither must be given; with neither the call is the plain one.  There is no host fallback."""
    rho, sigma = args.rho_of('scan_fit', rho, sigma)
    if verts.dim() != 3 or tuple(verts.shape[1:]) != (model.num_verts, 3):
        raise ValueError('scan_fit: verts must be [B,%d,3], got %s' % (model.num_verts, tuple(verts.shape)))
    b = verts.shape[0]
    if points.dim() != 3 or points.shape[0] != b or points.shape[2] != 3:
        raise ValueError('scan_fit: points must be [%d,Q,3], got %s' % (b, tuple(points.shape)))
    q = points.shape[1]
    if tuple(transl.shape) != (b, 3):
        raise ValueError('scan_fit: transl has shape %s, expected %s' % (tuple(transl.shape), (b, 3)))
    if b == 0 or q == 0:
        raise ValueError('scan_fit: empty input %s' % (tuple(points.shape),))
    cos = args.max_angle_cos(normals, max_angle, points, 'scan_fit')
    args.check_weights('scan_fit', weights, b, q)
    counts = args.counts_of('scan_fit', counts, b)
    _need_hip('scan_fit', verts, transl, points, weights, counts, hint, face_out, normals)
    if face_out is not None and (tuple(face_out.shape) != (b, q) or face_out.dtype != torch.int32 or not face_out.is_contiguous()):
        raise ValueError('scan_fit: face_out must be a contiguous int32 [%d,%d] tensor' % (b, q))
    weights = None if weights is None else _f32(weights.detach())
    hint = args.hint_of(hint, points, 'scan_fit')
    face = face_out if face_out is not None else torch.empty(b, q, dtype=torch.int32, device=points.device)
    normals = None if cos is None else _f32(normals.detach())
    total, per_body, d2, bary = _ScanFit.apply(verts, transl, points, model, counts, weights, hint, rho, sigma, face, normals, cos)
    return total, per_body, ClosestPoint(d2, face, bary)
