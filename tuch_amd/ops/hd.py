"""The HD branch of the training loss: HDModel and its fused contact term (csrc/hd_contact.hip, csrc/hd_search.hip),
and the selected HD points (csrc/glue.hip)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _C
from ._base import _f32, _i32, _workspace
from .model import ContactModel


class HDModel:
    """Device tables of the HD vertex regressor for the fused HD branch (wraps tuch_hd_model; csrc/hd_contact.hip).
    hd_idx / hd_w [N,K]: the K <= 8 non-zeros of every regressor row (K = 3: barycentric samples); hd_face [N]:
    faces_vert_is_sampled_from."""

    def __init__(self, contact_model: ContactModel, hd_idx, hd_w, hd_face):
        self.contact_model = contact_model
        self.num_points = int(np.asarray(hd_face).shape[0])
        hd_idx, hd_w = np.asarray(hd_idx), np.asarray(hd_w)
        # [N,K]: K non-zeros per regressor row (3 for barycentric samples; up to 8)
        self.row_nnz = int(hd_idx.shape[-1]) if hd_idx.ndim == 2 else 3
        if not 1 <= self.row_nnz <= 8 or hd_idx.size != self.num_points * self.row_nnz or hd_w.size != hd_idx.size:
            raise ValueError('HDModel: hd_idx / hd_w must be [N,K] with 1 <= K <= 8 (got %s, %s for %d points)'
                             % (hd_idx.shape, hd_w.shape, self.num_points))
        self._host = (_i32(hd_idx.reshape(-1, self.row_nnz)), np.ascontiguousarray(hd_w.reshape(-1, self.row_nnz), np.float32),
                      _i32(hd_face))
        self._h = None

    @property
    def _handle(self):
        if self._h is None:
            idx, w, face = self._host
            handle = ctypes.c_void_p(0)
            cm = self.contact_model._handle
            with _C.create_context(self.contact_model.device):
                _C.check(_C.lib().tuch_hd_model_create(ctypes.byref(handle), cm, self.num_points, self.row_nnz,
                                                       idx.ctypes.data_as(ctypes.c_void_p), w.ctypes.data_as(ctypes.c_void_p),
                                                       face.ctypes.data_as(ctypes.c_void_p)))
            self._h = handle
        return self._h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            try:
                _C.lib().tuch_hd_model_destroy(h)
            except Exception:
                pass
            self._h = None

    def contact_terms(self, verts, exterior, min_d2, partner, valid_u8, euclthres, thresh=0.99):
        """[B,2] (interior sum, exterior sum) over the HD points of loss.py:274-315, differentiable w.r.t. verts."""
        return _HDContact.apply(verts, exterior, min_d2, partner, valid_u8, self, float(euclthres), float(thresh))

    def selection(self, saved, batch):
        """(counts [B], selected [B,N] caller-order ids per slot, -1 padded) of a forward call (tests)."""
        counts = np.zeros(batch, np.int32)
        sel = np.zeros((batch, self.num_points), np.int32)
        _C.check(_C.lib().tuch_hd_contact_selection(self._handle, _C.ptr(saved), batch, counts.ctypes.data_as(ctypes.c_void_p),
                                                    sel.ctypes.data_as(ctypes.c_void_p)))
        return counts, sel


    def details(self, saved, batch):
        """(partner [B,N] caller-order id of every slot's partner or -1, exterior [B,N] bool) of a forward call (tests)."""
        part = np.zeros((batch, self.num_points), np.int32)
        ext = np.zeros((batch, self.num_points), np.uint8)
        _C.check(_C.lib().tuch_hd_contact_details(self._handle, _C.ptr(saved), batch, part.ctypes.data_as(ctypes.c_void_p),
                                                  ext.ctypes.data_as(ctypes.c_void_p)))
        return part, ext.astype(bool)


class _HDContact(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, exterior, min_d2, partner, valid, hm: HDModel, euclthres, thresh):
        v = _f32(verts)
        b = v.shape[0]
        L = _C.lib()
        h = hm._handle
        terms = torch.empty(b, 2, dtype=torch.float32, device=v.device)
        nsaved = L.tuch_hd_contact_saved_bytes(h, b)
        nws = L.tuch_hd_contact_workspace_bytes(h, b)
        saved = torch.empty(nsaved, dtype=torch.uint8, device=v.device)
        ws = _workspace(nws, v.device)
        ext, md, part = exterior.contiguous(), _f32(min_d2), partner.contiguous()
        _C.check(L.tuch_hd_contact_fwd(h, _C.ptr(v), _C.ptr(ext), _C.ptr(md), _C.ptr(part), _C.ptr(valid), b, euclthres, thresh,
                                       _C.ptr(terms), _C.ptr(saved), nsaved, _C.ptr(ws), nws, _C.stream()))
        ctx.save_for_backward(saved)
        ctx.hm, ctx.shape = hm, tuple(v.shape)
        hm.last_saved = saved           # inspection only
        return terms

    @staticmethod
    def backward(ctx, grad_terms):
        saved, = ctx.saved_tensors
        hm = ctx.hm
        b = ctx.shape[0]
        L = _C.lib()
        g = grad_terms.to(torch.float32).contiguous()
        grad = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        nws = L.tuch_hd_contact_workspace_bytes(hm._handle, b)
        ws = _workspace(nws, g.device)
        _C.check(L.tuch_hd_contact_bwd(hm._handle, _C.ptr(saved), _C.ptr(g), b, _C.ptr(grad), _C.ptr(ws), nws, _C.stream()))
        return grad, None, None, None, None, None, None, None


class _HDPoints(torch.autograd.Function):
    """points[n] = sum_k w[hd[n],k] * verts[body[n], idx[hd[n],k]]  (loss.py:285 with the regressor's 3 non-zeros per row)."""

    @staticmethod
    def forward(ctx, verts, body, hd, idx, w):
        v = _f32(verts)
        n = body.shape[0]
        out = torch.empty(n, 3, dtype=torch.float32, device=v.device)
        _C.check(_C.lib().tuch_hd_points_fwd(_C.ptr(v), _C.ptr(body), _C.ptr(hd), _C.ptr(idx), _C.ptr(w), v.shape[1], n,
                                             _C.ptr(out), _C.stream()))
        ctx.save_for_backward(body, hd, idx, w)
        ctx.shape = v.shape
        return out

    @staticmethod
    def backward(ctx, grad):
        body, hd, idx, w = ctx.saved_tensors
        g = grad.to(torch.float32).contiguous()
        gv = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        _C.check(_C.lib().tuch_hd_points_bwd(_C.ptr(g), _C.ptr(body), _C.ptr(hd), _C.ptr(idx), _C.ptr(w), ctx.shape[1],
                                             body.shape[0], _C.ptr(gv), _C.stream()))
        return gv, None, None, None, None


def hd_points(verts, body_of_point, hd_of_point, hd_idx, hd_w):
    """Selected HD points [N,3] of posed vertices [B,V,3]; int32 indices, hd_idx / hd_w [N_hd,3]."""
    return _HDPoints.apply(verts, body_of_point, hd_of_point, hd_idx, hd_w)
