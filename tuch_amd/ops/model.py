"""ContactModel, the device-side constants of one body model (csrc/model.hip), with its host table builders and the
searches that run on them: the cluster tree (csrc/cluster_tree.hip), the inside test (csrc/winding.hip,
csrc/ray_winding.hip), the nearest admissible vertex (csrc/v2v.hip) and the region-pair minimum
(csrc/region_min.hip)."""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _C
from . import args
from ._base import _current_stream, _f32, _i32, _side_stream, _workspace
from .closest_point import ClosestPoint, _ClosestPoint


def region_tables(cdict):
    """{'classes': [(regA, regB), ...], 'csig': {region: vertex ids}} (train_module.py:64-66) ->
    (ordered vertex-id lists, pairs [P,2] of indices into that order).  Region keys are looked up as the
    reference does (``csig[regpair[0]]``), whatever their type; numpy string scalars match their str()."""
    csig = cdict['csig']
    names = list(csig.keys())
    index = {n: i for i, n in enumerate(names)}

    def find(key):
        for k in (key, str(key)):
            try:
                if k in index:
                    return index[k]
            except TypeError:
                pass
        if hasattr(key, 'item'):
            return find(key.item())
        raise KeyError('region %r of cdict[\'classes\'] is not a key of cdict[\'csig\']' % (key,))
    regions = [np.asarray(csig[n], dtype=np.int64) for n in names]
    pairs = np.asarray([[find(p[0]), find(p[1])] for p in cdict['classes']], np.int64).reshape(-1, 2)
    return regions, pairs


def segment_faces(body_faces: np.ndarray, vidx: np.ndarray, bands: Sequence[np.ndarray], first_cap: int,
                  num_verts: Optional[int] = None) -> np.ndarray:
    """Closed-segment face list of tuch/utils/segmentation.py:48-66: body faces whose three
    vertices are all in ``vidx`` followed by the cap fans [b[i+1], b[i], cap_k]; cap k of this
    segment is stored at global vertex index ``first_cap + k``."""
    body_faces = np.asarray(body_faces, np.int64)
    inside = np.isin(body_faces, np.asarray(vidx)).sum(1) == 3
    fans = []
    for k, band in enumerate(bands):
        band = np.asarray(band, np.int64)
        fans.append(np.stack([band[1:], band[:-1], np.full(len(band) - 1, first_cap + k, np.int64)], 1))
    return np.concatenate([body_faces[inside]] + fans, 0) if fans else body_faces[inside]


def near_encode_host(value: float, round_up: bool) -> int:
    """The near test's 16-bit fixed-point level of a single-precision value, by the kernels' own conversion run on the
    host (tests only; tuch_near_encode_host in include/tuch_amd.h)."""
    out = ctypes.c_int(0)
    _C.check(_C.lib().tuch_near_encode_host(ctypes.c_float(value), int(bool(round_up)), ctypes.byref(out)))
    return out.value


def cluster_tree(faces, num_verts: int, leaf_faces: int = 64) -> dict:
    """The face-cluster tree used by the hierarchical winding numbers (host only; see include/tuch_amd.h,
    tuch_cluster_tree_build).  Returns numpy arrays: nodes [N,8], vidx, sign, qperm, frontier_off,
    frontier_nodes, launch_order, rows, face_leaf, plus exact_len."""
    L = _C.lib()
    f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
    h = ctypes.c_void_p()
    _C.check(L.tuch_cluster_tree_build(int(num_verts), f.shape[0], f.ctypes.data_as(ctypes.c_void_p), int(leaf_faces),
                                       ctypes.byref(h)))
    try:
        vals = [ctypes.c_int(0) for _ in range(6)]
        _C.check(L.tuch_cluster_tree_info(h, *[ctypes.byref(v) for v in vals]))
        n, exact_len, stream_len, qblocks, nfr, frtot = [v.value for v in vals]
        out = dict(nodes=np.zeros((n, 8), np.int32), vidx=np.zeros(stream_len, np.int32),
                   sign=np.zeros(stream_len, np.float32), qperm=np.zeros(qblocks * 128, np.int32),
                   frontier_off=np.zeros(nfr + 1, np.int32), frontier_nodes=np.zeros(frtot, np.int32),
                   launch_order=np.zeros(frtot * qblocks, np.int32), rows=np.zeros((n, 2), np.int32),
                   face_leaf=np.zeros(f.shape[0], np.int32))
        _C.check(L.tuch_cluster_tree_export(h, *[out[k].ctypes.data_as(ctypes.c_void_p) for k in
                                                 ('nodes', 'vidx', 'sign', 'qperm', 'frontier_off', 'frontier_nodes',
                                                  'launch_order', 'rows', 'face_leaf')]))
        out['exact_len'] = exact_len
        return out
    finally:
        L.tuch_cluster_tree_free(h)


class _RegionPairMin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, model: ContactModel, select, masked):
        v = _f32(verts)
        b = v.shape[0]
        out = torch.empty(b, model.num_pairs, dtype=torch.float32, device=v.device)
        ij = torch.empty(b, model.num_pairs, 2, dtype=torch.int32, device=v.device)
        sel = select.to(torch.uint8).contiguous() if select is not None else None
        _C.check(_C.lib().tuch_region_pair_min(model._handle, _C.ptr(v), b, _C.ptr(sel), int(masked),
                                               _C.ptr(out), _C.ptr(ij), _C.stream()))
        ctx.save_for_backward(v, ij)
        ctx.model = model
        ctx.mark_non_differentiable(ij)
        return out, ij

    @staticmethod
    def backward(ctx, grad_out, _grad_ij):
        v, ij = ctx.saved_tensors
        grad = torch.zeros_like(v)
        g_out = grad_out.to(torch.float32).contiguous()
        _C.check(_C.lib().tuch_region_pair_min_bwd(ctx.model._handle, _C.ptr(v), v.shape[0], _C.ptr(ij),
                                                   _C.ptr(g_out), _C.ptr(grad), _C.stream()))
        return grad, None, None, None


class ContactModel:
    """Device-side constants of one body model; wraps tuch_contact_model.

    faces      [F,3] ints                       (smpl.faces, train.py:62)
    geomask    [V,V] bool, geod > geothres      (smplifydc.py:65, loss.py:71), optional
    segments   list of (vidx, [band loops])     (segmentation.py), optional
    regions    ordered list of vertex-id lists; pairs [P,2] region indices, optional
    """

    def __init__(self, faces, geomask=None, segments=None, regions=None, pairs=None,
                 device: Optional[torch.device] = None):
        self.device = torch.device(device if device is not None else 'cuda')
        faces = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces)
        self.faces_np = faces.astype(np.int64)
        self._hints = {}
        self.num_verts = int(faces.max()) + 1
        self.num_faces = int(faces.shape[0])
        gm = None
        if geomask is not None:
            gm = geomask.detach().cpu().numpy() if isinstance(geomask, torch.Tensor) else np.asarray(geomask)
            self.num_verts = max(self.num_verts, gm.shape[0])
            gm = np.ascontiguousarray(gm.astype(np.uint8))
            assert gm.shape == (self.num_verts, self.num_verts)
        self.has_mask = gm is not None
        v = self.num_verts
        # segment tables
        segments = list(segments or [])
        seg_q_off, seg_q, seg_f_off, seg_f, cap_off, cap_v = [0], [], [0], [], [0], []
        for vidx, bands in segments:
            first_cap = v + len(cap_off) - 1
            seg_f.append(segment_faces(self.faces_np, vidx, bands, first_cap))
            seg_f_off.append(seg_f_off[-1] + len(seg_f[-1]))
            seg_q.append(np.asarray(vidx, np.int64))
            seg_q_off.append(seg_q_off[-1] + len(vidx))
            for band in bands:
                cap_v.append(np.asarray(band, np.int64))
                cap_off.append(cap_off[-1] + len(band))
        self.num_segments = len(segments)
        self.seg_q_total = seg_q_off[-1]
        self.seg_q_off = seg_q_off
        self.seg_vidx = [np.asarray(s[0], np.int64) for s in segments]
        # region tables
        regions = list(regions or [])
        reg_off = np.cumsum([0] + [len(r) for r in regions])
        self.num_pairs = 0 if pairs is None else len(pairs)
        cat = lambda lst, width=None: (np.concatenate(lst) if lst else np.zeros(0, np.int64))
        keep = dict(
            faces=_i32(faces), seg_q_off=_i32(seg_q_off), seg_q=_i32(cat(seg_q)), seg_f_off=_i32(seg_f_off),
            seg_f=_i32(cat(seg_f).reshape(-1, 3)), cap_off=_i32(cap_off), cap_v=_i32(cat(cap_v)),
            reg_off=_i32(reg_off), reg_v=_i32(cat([np.asarray(r) for r in regions])),
            pairs=_i32(pairs if pairs is not None else np.zeros((0, 2))))
        # the device copy (tuch_contact_model_create: the library's only allocations) is made on first use, so
        # that the callers' constructors (RegressorLoss, SMPLifyDC, ...) also run where no GPU is visible
        self._host = (keep, gm, len(cap_off) - 1, len(regions))
        self._h = None
        self._faces_i32 = None
        # host-side switches, read from the environment once (like the library's own, tuch_contact_model_set_option):
        # overlap = search on a second stream beside the inside test, v2v_hint = partner hints kept between calls
        self._py_options = {'overlap': int(os.environ.get('TUCH_OVERLAP', '1') != '0'),
                            'v2v_hint': int(os.environ.get('TUCH_V2V_HINT', '1') != '0')}
        self._pending_options = {}

    @property
    def _handle(self):
        if self._h is None:
            keep, gm, num_caps, num_regions = self._host
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else ctypes.c_void_p(0)
            handle = ctypes.c_void_p(0)
            with _C.create_context(self.device):
                _C.check(_C.lib().tuch_contact_model_create(
                    ctypes.byref(handle), self.num_verts, self.num_faces, p(keep['faces']),
                    gm.ctypes.data_as(ctypes.c_void_p) if gm is not None else ctypes.c_void_p(0),
                    self.num_segments, p(keep['seg_q_off']), p(keep['seg_q']), p(keep['seg_f_off']), p(keep['seg_f']),
                    num_caps, p(keep['cap_off']), p(keep['cap_v']),
                    num_regions, p(keep['reg_off']), p(keep['reg_v']), self.num_pairs, p(keep['pairs'])))
            self._h = handle
            self._host = None          # the 47 MB byte mask is not needed again
            for name, value in self._pending_options.items():
                _C.check(_C.lib().tuch_contact_model_set_option(handle, name.encode(), int(value)))
            self._pending_options = {}
        return self._h

    def set_option(self, name: str, value: int) -> None:
        """Change one of the model's switches (include/tuch_amd.h: tuch_contact_model_set_option; plus the host-side
        'overlap' and 'v2v_hint').  The environment is read once, when the model is created; hot calls never read it.
        Captured hipGraphs keep the behaviour they were captured with."""
        if name in self._py_options:
            self._py_options[name] = int(value)
        elif self._h is None:
            self._pending_options[name] = int(value)
        else:
            _C.check(_C.lib().tuch_contact_model_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        if name in self._py_options:
            return self._py_options[name]
        out = ctypes.c_int(0)
        _C.check(_C.lib().tuch_contact_model_get_option(self._handle, name.encode(), ctypes.byref(out)))
        return out.value

    def canary_hits(self, reset: bool = True) -> int:
        """Guard words between workspace regions found changed since the last reset (option canary = 1: debug mode,
        include/tuch_amd.h).  Synchronises the device."""
        out = ctypes.c_int(0)
        _C.check(_C.lib().tuch_contact_model_canary_hits(self._handle, ctypes.byref(out), int(reset)))
        return out.value

    def canary_selftest(self) -> int:
        """Overruns a guarded region on purpose: returns the hits counted (1 if the mechanism works)."""
        ws = _workspace(8192, self.device)
        rc = _C.lib().tuch_contact_model_canary_selftest(self._handle, _C.ptr(ws), ws.numel(), _C.stream())
        if rc < 0:
            _C.check(rc)
        return rc

    @property
    def faces_i32(self):
        if self._faces_i32 is None:
            self._faces_i32 = torch.as_tensor(_i32(self.faces_np), device=self.device)
        return self._faces_i32

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            try:
                _C.lib().tuch_contact_model_destroy(h)
            except Exception:
                pass
            self._h = None

    def strips(self):
        """(vertex ids, signs, number of strips) of the triangle-strip walk used by the winding kernel."""
        n, k = ctypes.c_int(0), ctypes.c_int(0)
        L = _C.lib()
        _C.check(L.tuch_contact_model_strips(self._handle, ctypes.byref(n), ctypes.byref(k), None, None))
        vidx = np.zeros(n.value, np.int32)
        sign = np.zeros(n.value, np.float32)
        _C.check(L.tuch_contact_model_strips(self._handle, None, None, vidx.ctypes.data_as(ctypes.c_void_p),
                                             sign.ctypes.data_as(ctypes.c_void_p)))
        return vidx, sign, k.value

    def exterior_and_partner(self, verts: torch.Tensor, apply_segments: bool = True, also=None, zero_floats: int = 0,
                             iterative: bool = False):
        """exterior_flags + v2v_min of the same vertices -> (exterior, min_d2, partner[, also()]).
        The two only share their input: the nearest-vertex search (and the optional callable ``also``,
        e.g. the region pairs) runs on a second stream so that its tail fills the gaps of the long winding
        walk (option overlap = 0 keeps everything on the current stream).
        zero_floats > 0: a float32 buffer of (at least) that many ZEROS is handed to ``also(buffer)`` -- cleared by the
        search's first kernel (tuch_v2v_min_model), not by a fill launch.
        iterative: the caller is an iterative fit (the previous call's partners, kept as hints, are almost this call's):
        the search then uses fewer, longer wavefronts (see v2v_min).  Results never depend on it."""
        zero = torch.empty((int(zero_floats) + 3) // 4 * 4, dtype=torch.float32, device=verts.device) if zero_floats > 0 else None
        call_also = (lambda: None) if also is None else also if zero is None else (lambda: also(zero))
        overlap = bool(verts.is_cuda and self._py_options['overlap'])
        if overlap:
            cur, side = _current_stream(verts.device), _side_stream(verts.device)
            side.wait_stream(cur)       # BEFORE the inside test is enqueued: the search does not wait for it
        # the inside test's chain FIRST (the side stream waits only for what was enqueued before its wait above).
        # Launched -- or captured -- behind the search, the chain's small head kernels find every wave slot taken by
        # the search's 55 k one-wave workgroups and only get going when it is done (eager: ray_leaf_bounds 119 us
        # instead of 14; replayed graph at batch 8: 0.240 against 0.213 ms once tree_inner_bounds_kernel no longer
        # delays the search's start).
        exterior = self.exterior_flags(verts, apply_segments=apply_segments)
        with (torch.cuda.stream(side) if overlap else contextlib.nullcontext()):
            if overlap and zero is not None:
                zero.record_stream(side)
            mn, partner = self.v2v_min(verts, leave_room=overlap, zero=zero, iterative=iterative)
            # (the caller's extra work -- region pairs, reprojection + prior -- FIRST, beside the short head of the inside
            # test's chain, was measured: 0.587 against 0.552 ms per step; it delays the search, which the chain waits for)
            extra = call_also()
        if overlap:
            cur.wait_stream(side)
            for t in (mn, partner, *(extra if isinstance(extra, (tuple, list)) else (extra,))):
                if torch.is_tensor(t):
                    t.record_stream(cur)
        return exterior, mn, partner, extra

    def winding_tree_work(self, verts: torch.Tensor) -> dict:
        """Stream elements the hierarchical winding walk steps through for these vertices (measurement aid)."""
        verts = _f32(verts)
        b = verts.shape[0]
        L = _C.lib()
        nbytes = L.tuch_exterior_workspace_bytes(self._handle, b)
        ws = _workspace(nbytes, verts.device)
        out = (ctypes.c_ulonglong * 4)()
        _C.check(L.tuch_winding_tree_work(self._handle, _C.ptr(verts), b, _C.ptr(ws), nbytes, out, _C.stream()))
        return dict(leaf_elements=int(out[0]), cap_elements=int(out[1]), wavefronts=int(out[2]),
                    flat_stream_elements=int(out[3]), queries_per_step=64,
                    query_blocks=-(-self.num_verts // 128) * 2 * b)

    def ray_work(self, verts: torch.Tensor) -> dict:
        """Strip elements the ray-crossing inside test steps through for these vertices (measurement aid)."""
        verts = _f32(verts)
        b = verts.shape[0]
        L = _C.lib()
        nbytes = L.tuch_exterior_workspace_bytes(self._handle, b)
        ws = _workspace(nbytes, verts.device)
        out = (ctypes.c_ulonglong * 4)()
        _C.check(L.tuch_ray_work(self._handle, _C.ptr(verts), b, _C.ptr(ws), nbytes, out, _C.stream()))
        return dict(elements=int(out[0]), wavefronts=int(out[3]), queries_per_step=64,
                    lanes_inside_leaf_slabs=int(out[1]) / max(int(out[2]), 1))

    def ray_near_debug(self, verts: torch.Tensor, points: Optional[torch.Tensor] = None,
                       counts: Optional[torch.Tensor] = None, waves: int = 0) -> dict:
        """What the near stage of the ray-crossing inside test holds for these vertices (or points): the leaves' padded
        bounds, their 16-bit records, the rays' values and the listed (leaf, slot) pairs (tests only; see
        tuch_ray_near_debug in include/tuch_amd.h).  waves: 0 as the step would, 1 / 4 wavefronts per query block."""
        verts = _f32(verts)
        b, dev = verts.shape[0], verts.device
        L = _C.lib()
        q = 0
        if points is not None:
            points = _f32(points)
            q = points.shape[1]
            if counts is not None:
                counts = counts.to(device=dev, dtype=torch.int32).contiguous()
        dims = (ctypes.c_longlong * 3)()
        null = ctypes.c_void_p(0)
        _C.check(L.tuch_ray_near_debug(self._handle, null, _C.ptr(points) if points is not None else null, null, b, q, waves,
                                       null, 0, dims, null, null, null, null, null, null, _C.stream()))
        leaves, blocks, nbytes = int(dims[0]), int(dims[1]), int(dims[2])
        ws = _workspace(nbytes, dev)
        out = dict(bounds=torch.zeros(b, 13, leaves, dtype=torch.float32, device=dev),
                   records=torch.zeros(b, leaves, 8, dtype=torch.int32, device=dev),
                   rays=torch.full((b, blocks * 64, 9), float('nan'), dtype=torch.float32, device=dev),
                   bitmap=torch.zeros(b, leaves, blocks * 8, dtype=torch.uint8, device=dev),
                   leaves=torch.full((b, blocks, leaves), -1, dtype=torch.int32, device=dev),
                   lengths=torch.zeros(b, blocks, dtype=torch.int32, device=dev))
        _C.check(L.tuch_ray_near_debug(self._handle, _C.ptr(verts), _C.ptr(points) if points is not None else null,
                                       _C.ptr(counts) if counts is not None else null, b, q, waves, _C.ptr(ws), nbytes, dims,
                                       *[_C.ptr(out[k]) for k in ('bounds', 'records', 'rays', 'bitmap', 'leaves', 'lengths')],
                                       _C.stream()))
        torch.cuda.synchronize(dev)
        return {k: v.cpu().numpy() for k, v in out.items()}

    # K2 + K3
    def exterior_flags(self, verts: torch.Tensor, apply_segments: bool = True, thresh: float = 0.99,
                       return_details: bool = False):
        verts = _f32(verts)
        b = verts.shape[0]
        assert verts.shape[1] == self.num_verts
        L = _C.lib()
        ext = torch.empty(b, self.num_verts, dtype=torch.uint8, device=verts.device)
        w = torch.empty(b, self.num_verts, dtype=torch.float32, device=verts.device) if return_details else None
        seg_w = seg_e = None
        if return_details and self.num_segments:
            seg_w = torch.empty(b, self.seg_q_total, dtype=torch.float32, device=verts.device)
            seg_e = torch.empty(b, self.seg_q_total, dtype=torch.uint8, device=verts.device)
        nbytes = L.tuch_exterior_workspace_bytes(self._handle, b)
        ws = _workspace(nbytes, verts.device)
        _C.check(L.tuch_exterior_flags(self._handle, _C.ptr(verts), b, int(apply_segments), float(thresh),
                                       _C.ptr(w), _C.ptr(ext), _C.ptr(seg_w), _C.ptr(seg_e), _C.ptr(ws), nbytes,
                                       _C.stream()))
        return (ext, w, seg_w, seg_e) if return_details else ext

    # K1
    def v2v_min(self, verts: torch.Tensor, leave_room: bool = False, zero: Optional[torch.Tensor] = None, iterative: bool = False):
        """leave_room: other kernels run beside the search on another stream (TUCH_V2V_LEAVE_ROOM of tuch_v2v_min_model).
        iterative: the hints are expected to be near-final (SMPLify-DC's loops): a quarter of the wavefronts, each over more
        leaves -- faster with good bounds (0.412 against 0.426 ms per stage-2 step at batch 64), slower on new bodies.
        zero: a caller tensor (numel * itemsize a multiple of 16) cleared by the call's first kernel."""
        if not self.has_mask:
            raise _C.TuchError('ContactModel was created without a geodesic mask')
        verts = _f32(verts)
        b = verts.shape[0]
        assert verts.shape[1] == self.num_verts
        L = _C.lib()
        mn = torch.empty(b, self.num_verts, dtype=torch.float32, device=verts.device)
        arg = torch.empty(b, self.num_verts, dtype=torch.int32, device=verts.device)
        nbytes = L.tuch_v2v_model_workspace_bytes(self._handle, b)
        ws = _workspace(nbytes, verts.device)
        flags = int(bool(leave_room)) | (2 if iterative else 0)
        zbytes = zero.numel() * zero.element_size() if zero is not None else 0
        _C.check(L.tuch_v2v_min_model(self._handle, _C.ptr(verts), b, _C.ptr(mn), _C.ptr(arg),
                                      _C.ptr(self._v2v_hint(b)), _C.ptr(ws), nbytes, flags, _C.ptr(zero), zbytes, _C.stream()))
        return mn, arg

    def _v2v_hint(self, batch: int) -> Optional[torch.Tensor]:
        """Persistent per-batch-size buffer in which the search leaves its partners for the next call (an iterative
        fit re-finds almost the same partners): seeds only, the results never depend on it (option v2v_hint = 0: off).
        Buffers are kept for the life of the model (a captured hipGraph may hold their addresses)."""
        if not self._py_options['v2v_hint']:
            return None
        buf = self._hints.get(batch)
        if buf is None:
            n = _C.lib().tuch_v2v_hint_bytes(self._handle, batch)
            if n == 0:
                return None
            buf = torch.zeros(n, dtype=torch.uint8, device=self.device)
            self._hints[batch] = buf
        return buf

    def winding_points(self, verts: torch.Tensor, points: torch.Tensor, counts: Optional[torch.Tensor] = None,
                       thresh: float = 0.99, flags_only: bool = False):
        """Winding numbers of arbitrary points [B,Q,3] against this mesh posed by verts [B,V,3]
        (cluster-tree walk; flat triangle strips for meshes without a tree); counts [B] int32 marks how many points per
        body are real.  Any point order is exact; blocks of 64 consecutive points that are close in space are fast.
        flags_only: return (None, exterior); for points OFF the surface the winding number is an integer and the flags
        come from signed ray crossings (csrc/ray_winding.hip) instead of the solid-angle sum."""
        v, pts = _f32(verts), _f32(points)
        b, q, _ = pts.shape
        L = _C.lib()
        w = torch.empty(b, q, dtype=torch.float32, device=pts.device) if not flags_only else None
        ext = torch.empty(b, q, dtype=torch.uint8, device=pts.device)
        nbytes = L.tuch_winding_points_workspace_bytes(self._handle, b, q)
        ws = _workspace(nbytes, pts.device)
        _C.check(L.tuch_winding_points(self._handle, _C.ptr(v), _C.ptr(pts), _C.ptr(counts), b, q, float(thresh),
                                       _C.ptr(w), _C.ptr(ext), _C.ptr(ws), nbytes, _C.stream()))
        return w, ext

    def closest_point(self, verts: torch.Tensor, points: torch.Tensor, counts: Optional[torch.Tensor] = None,
                      hint: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
                      max_angle: Optional[float] = None) -> 'ClosestPoint':
        """The nearest point of this mesh posed by verts [B,V,3] for arbitrary points [B,Q,3] (csrc/closest_point.hip):
        ``ClosestPoint(d2 [B,Q], face [B,Q] int32, bary [B,Q,3])`` with the nearest point = sum_k bary[k] *
        verts[faces[face][k]].  counts [B] int32 marks how many points per body are real; the others get d2 = inf,
        face = -1, bary = 0.  The same bits for a query alone or in any batch and for any order of the queries; any order
        is exact, blocks of 64 consecutive points that are close in space are fast (a wavefront visits the face groups
        any of its 64 queries needs).  d2 is differentiable with respect to verts and points with the weights held fixed
        (exact wherever the closest feature does not change), bit-reproducibly under ``deterministic()``; face and bary
        are not differentiable.
        hint [B,Q] int32: per query a face that is probably the answer (a fitting loop passes the previous iteration's
        ``face``).  It changes no bit of the result, whatever it holds (wrong faces and indices out of range included);
        a valid one lets the query start from that face's exact distance instead of from a walk over every box of the
        body (tuch_closest_point with a hint).
        normals [B,Q,3] with max_angle in degrees, in (0, 90]: the normal-compatible search (tuch_closest_point with normals).
        A face is a candidate for a query only if its normal (b - a) x (c - a) is within max_angle of the query's normal
        (any length, in the frame of verts) -- decided by one fixed float32 sequence (include/tuch_amd.h), so the same
        bits hold alone or in a batch, for any order, any hint and any grouping of the faces.  A query with a zero or
        non-finite normal is unconstrained (the plain call's bits); one without an admissible face gets d2 = inf,
        face = -1, bary = 0 and no gradient.  Normals are constants: they get no gradient.  Both or neither must be
        given; with neither the call is the plain one."""
        cos = args.max_angle_cos(normals, max_angle, points, 'closest_point')
        if verts.dim() != 3 or points.dim() != 3 or verts.shape[0] != points.shape[0] or verts.shape[1] != self.num_verts:
            raise _C.TuchError('closest_point: verts [B,%d,3] and points [B,Q,3] expected, got %s and %s'
                               % (self.num_verts, tuple(verts.shape), tuple(points.shape)))
        if counts is not None:
            counts = counts.to(torch.int32).contiguous()
        hint = args.hint_of(hint, points, 'closest_point')
        normals = None if cos is None else _f32(normals.detach())
        return ClosestPoint(*_ClosestPoint.apply(verts, points, self, counts, hint, normals, cos))

    def face_groups(self):
        """The face groups the closest-point search walks, as host arrays: (group_off [G+1], face_list [F], face_group
        [F]); face_group is the inverse of face_list -- the group a hinted query starts from."""
        n = ctypes.c_int(0)
        L = _C.lib()
        _C.check(L.tuch_contact_model_face_groups(self._handle, ctypes.byref(n), None, None, None))
        off, lst, grp = np.zeros(n.value + 1, np.int32), np.zeros(self.num_faces, np.int32), np.zeros(self.num_faces, np.int32)
        _C.check(L.tuch_contact_model_face_groups(self._handle, None, *(a.ctypes.data_as(ctypes.c_void_p) for a in (off, lst, grp))))
        return off, lst, grp

    def signed_distance(self, verts: torch.Tensor, points: torch.Tensor, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Distance [B,Q] from points [B,Q,3] to this mesh posed by verts, negative where the point is interior
        (``winding_points(..., flags_only=True)``); +inf for entries beyond counts.  Only the magnitude is differentiable
        (the gradient is zero at a point on the surface).  Needs a closed mesh: a model without a cluster tree raises."""
        if self.tree_positions() is None:
            raise _C.TuchError('signed_distance: the model has no cluster tree (an open or non-manifold mesh has no inside)')
        d2 = self.closest_point(verts, points, counts).d2
        _, exterior = self.winding_points(verts, points, counts, flags_only=True)
        off = d2 > 0
        dist = torch.where(off, torch.sqrt(torch.where(off, d2, torch.ones_like(d2))), torch.zeros_like(d2))
        return torch.where(exterior.bool(), dist, -dist)

    def v2v_min_indexed(self, points: torch.Tensor, vertex_ids: torch.Tensor, offsets: torch.Tensor,
                        max_points: int, tree_order: bool = False, mfma: bool = False):
        """Ragged masked nearest neighbour (HD points, loss.py:288-291).  points [N,3], vertex_ids [N]
        int32, offsets [B+1] int32 -> (min_d2 [N], argmin [N] int32 relative to the body's first point).
        tree_order: vertex_ids are positions in the cluster tree's vertex order (``tree_positions``) and the
        mask packed in that order is used -- the same answer, far fewer distinct mask words per wavefront.
        mfma: the matrix-core form the HD branch runs (tuch_v2v_min_indexed_mfma: winners may differ between rows that tie
        within ~1e-6 relative)."""
        if not self.has_mask:
            raise _C.TuchError('ContactModel was created without a geodesic mask')
        pts = _f32(points)
        n = pts.shape[0]
        mn = torch.empty(n, dtype=torch.float32, device=pts.device)
        arg = torch.empty(n, dtype=torch.int32, device=pts.device)
        L = _C.lib()
        bits = L.tuch_contact_model_tree_mask_bits(self._handle) if tree_order else \
            L.tuch_contact_model_mask_bits(self._handle)
        if not bits:
            raise _C.TuchError('ContactModel has no mask in tree order (no cluster tree)')
        size_fn, fn = (L.tuch_v2v_min_indexed_mfma_workspace_bytes, L.tuch_v2v_min_indexed_mfma) if mfma else \
            (L.tuch_v2v_min_indexed_workspace_bytes, L.tuch_v2v_min_indexed)
        nbytes = size_fn(offsets.shape[0] - 1, int(max_points))
        ws = _workspace(nbytes, pts.device)
        vertex_ids, offsets = vertex_ids.contiguous(), offsets.contiguous()
        _C.check(fn(_C.ptr(pts), _C.ptr(vertex_ids), _C.ptr(offsets),
                    ctypes.c_void_p(bits), offsets.shape[0] - 1, self.num_verts, int(max_points),
                    _C.ptr(mn), _C.ptr(arg), _C.ptr(ws), nbytes, _C.stream()))
        return mn, arg

    def tree_positions(self) -> Optional[np.ndarray]:
        """position of every vertex in the cluster tree's vertex order (inverse of the MODEL'S OWN qperm, whatever leaf
        size it was built with: tuch_contact_model_tree_order), or None without tree."""
        qperm = np.zeros(self.num_verts, np.int32)
        try:
            _C.check(_C.lib().tuch_contact_model_tree_order(self._handle, qperm.ctypes.data_as(ctypes.c_void_p), None))
        except _C.TuchError:
            return None
        pos = np.empty(self.num_verts, np.int32)
        pos[qperm] = np.arange(self.num_verts, dtype=np.int32)
        return pos

    # K5
    def region_pair_min(self, verts: torch.Tensor, select: Optional[torch.Tensor] = None, masked: bool = False):
        return _RegionPairMin.apply(verts, self, select, masked)
