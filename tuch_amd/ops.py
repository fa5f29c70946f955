"""torch-facing wrappers over the C ABI: device tensors in, device tensors out.

Everything here runs the hand-written HIP kernels of libtuch_amd.so; there is no
eager/CPU fallback.  Index outputs are int64 like the reference's torch ops.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import weakref
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _C, backward_pass
from .backward_pass import backward_scalar          # noqa: F401 (the fitting loops and the bench call ops.backward_scalar)

MODE_SMPLIFY = 0   # tuch/smplify/losses.py:96-105
MODE_TRAIN = 1     # tuch/train/loss.py:303-315


def _f32(t: torch.Tensor) -> torch.Tensor:
    if t.dtype is torch.float32 and t.is_contiguous():       # (the usual case: one call instead of three on the eager path)
        return t.detach()
    return t.detach().to(torch.float32).contiguous()


_SIDE_STREAMS = {}
_STREAM_OBJECTS = {}


def _current_stream(device) -> 'torch.cuda.Stream':
    """torch.cuda.current_stream(device) without building a new Stream object through torch's device-index helpers on
    every call (~9 us, several times per eager step): one object per (device, raw stream handle) is kept."""
    raw, cur = _C._raw_stream, _C._cur_device
    if raw is None or cur is None:
        return torch.cuda.current_stream(device)
    index = device.index if device.index is not None else cur()
    key = (index, raw(index))
    s = _STREAM_OBJECTS.get(key)
    if s is None:
        s = _STREAM_OBJECTS[key] = torch.cuda.current_stream(device)
    return s


def _side_stream(device) -> 'torch.cuda.Stream':
    """The companion stream of the CURRENT stream (one per stream: callers that run several fits on streams of
    their own must not be coupled through a shared side stream)."""
    key = (device.type, device.index, _current_stream(device).cuda_stream)
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return s


_GRAPH_STREAMS = {}


@contextlib.contextmanager
def off_default_stream(device):
    """Run the body on a non-default stream when the current stream is the legacy default (NULL) stream.

    hipGraph replays on the NULL stream are not reliably ordered against the kernels, copies and memsets enqueued
    around them (ROCm 7.2, graphs with forked branches: observed as stale inputs / un-reset optimiser state in about
    every second call, never on a created stream).  Every place in this package that replays a captured graph does it
    inside this context; the two streams are joined with events on entry and exit, so callers see stream semantics."""
    device = torch.device(device)
    cur = torch.cuda.current_stream(device)
    if cur != torch.cuda.default_stream(device):
        yield cur
        return
    key = (device.index if device.index is not None else torch.cuda.current_device())
    s = _GRAPH_STREAMS.get(key)
    if s is None:
        s = _GRAPH_STREAMS[key] = torch.cuda.Stream(device=device)
    s.wait_stream(cur)
    try:
        with torch.cuda.stream(s):
            yield s
    finally:
        cur.wait_stream(s)


def deterministic() -> bool:
    """Deterministic mode of the library (include/tuch_amd.h: tuch_set_deterministic): on unless TUCH_DETERMINISTIC=0."""
    return bool(_C.lib().tuch_get_deterministic())


@contextlib.contextmanager
def deterministic_mode(on: bool):
    """``with ops.deterministic_mode(False): ...`` -- the mode for the calls inside, the previous one restored after."""
    before = deterministic()
    set_deterministic(on)
    try:
        yield
    finally:
        set_deterministic(before)


def set_deterministic(on: bool) -> None:
    """True (the default): gradient scatters through 64-bit fixed-point integer atomics instead of float atomics: an SMPLify-DC fit reproduces
    bit for bit (stage-2 tail, SMPL adjoint, the training loss's plain term -- _ContactTerms -- and its HD term).
    Graphs captured before the switch keep the mode they were captured in."""
    _C.lib().tuch_set_deterministic(int(bool(on)))


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------- raw functions
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


def _tracked(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


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


MAX_CONTACT_REGIONS = 128     # tuch_self_contact's limit (the DSC annotation has 75 regions)


def vertex_region_table(regions, num_verts: int) -> Tuple[np.ndarray, np.ndarray]:
    """Ordered list of vertex-id lists (regions may overlap or be empty, a vertex may belong to none) -> the
    vertex -> regions CSR lists of tuch_self_contact: (off int32 [V+1], ids int32 [nnz]); vertex v belongs to the
    regions ids[off[v]:off[v+1]], ascending.  A vertex listed twice in one region counts once.  Host only (numpy)."""
    regions = [np.asarray(r, np.int64).reshape(-1) for r in regions]
    num_verts = int(num_verts)
    if len(regions) > MAX_CONTACT_REGIONS:
        raise ValueError('%d regions, at most %d are supported' % (len(regions), MAX_CONTACT_REGIONS))
    for k, r in enumerate(regions):
        if r.size and (r.min() < 0 or r.max() >= num_verts):
            raise ValueError('region %d has a vertex id outside [0, %d): [%d, %d]' % (k, num_verts, r.min(), r.max()))
    regions = [np.unique(r) for r in regions]
    vert = np.concatenate(regions) if regions else np.zeros(0, np.int64)
    reg = np.concatenate([np.full(len(r), k, np.int64) for k, r in enumerate(regions)]) if regions else np.zeros(0, np.int64)
    order = np.lexsort((reg, vert))
    off = np.zeros(num_verts + 1, np.int64)
    np.cumsum(np.bincount(vert, minlength=num_verts), out=off[1:])
    return off.astype(np.int32), np.ascontiguousarray(reg[order], dtype=np.int32)


def self_contact(verts: torch.Tensor, mask_bits, euclthres: float, vreg=None, num_regions: int = 0) -> dict:
    """tuch_self_contact (include/tuch_amd.h): verts [B,V,3] + packed mask (pack_geomask's tensor, or a model's pointer)
    -> {'in_contact' [B,V] bool, 'partner' [B,V] int32, 'min_d2' [B,V], 'cnc_d2' [B]} and, with vreg = (off, ids) device
    int32 tensors of vertex_region_table and num_regions = R, 'sig_d2' [B,R,R].  SQUARED distances, +inf = none.
    Two launches on the current stream, nothing else: capturable."""
    verts = _f32(verts)
    b, v, _ = verts.shape
    dev = verts.device
    flags = torch.empty(b, v, dtype=torch.uint8, device=dev)
    out = {'partner': torch.empty(b, v, dtype=torch.int32, device=dev),
           'min_d2': torch.empty(b, v, dtype=torch.float32, device=dev),
           'cnc_d2': torch.empty(b, dtype=torch.float32, device=dev)}
    off = ids = sig = None
    if vreg is not None:
        off, ids = vreg
        if off.dtype != torch.int32 or ids.dtype != torch.int32 or off.numel() != v + 1:
            raise ValueError('vreg must be the (off [V+1], ids) int32 tensors of vertex_region_table')
        if ids.numel() == 0:                       # (a NULL pointer would read as "no table")
            ids = torch.zeros(1, dtype=torch.int32, device=dev)
        sig = out['sig_d2'] = torch.empty(b, int(num_regions), int(num_regions), dtype=torch.float32, device=dev)
    mptr = _C.ptr(mask_bits) if isinstance(mask_bits, torch.Tensor) else mask_bits
    _C.check(_C.lib().tuch_self_contact(_C.ptr(verts), mptr, b, v, float(euclthres), _C.ptr(off), _C.ptr(ids),
                                        int(num_regions), _C.ptr(flags), _C.ptr(out['partner']), _C.ptr(out['min_d2']),
                                        _C.ptr(sig), _C.ptr(out['cnc_d2']), _C.stream()))
    out['in_contact'] = flags.view(torch.bool)
    return out


MAX_RENDER_VIEWS = 32         # tuch_render_mesh's limit (one bit per view in background_views)


def vertex_face_table(faces, num_verts: int) -> Tuple[np.ndarray, np.ndarray]:
    """faces [F,3] -> the vertex -> faces CSR lists of tuch_render_mesh: (off int32 [V+1], ids int32 [3F]); vertex v is a
    corner of the faces ids[off[v]:off[v+1]], ascending (a face that names a vertex twice is listed twice).  Host only."""
    faces = np.asarray(faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise ValueError('faces must be [F, 3] with F >= 1, got %s' % (faces.shape,))
    faces = faces.astype(np.int64)
    num_verts = int(num_verts)
    if faces.min() < 0 or faces.max() >= num_verts:
        raise ValueError('faces name vertices outside [0, %d): [%d, %d]' % (num_verts, faces.min(), faces.max()))
    vert = faces.reshape(-1)
    face = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    order = np.lexsort((face, vert))
    off = np.zeros(num_verts + 1, np.int64)
    np.cumsum(np.bincount(vert, minlength=num_verts), out=off[1:])
    return off.astype(np.int32), np.ascontiguousarray(face[order], dtype=np.int32)


class VertexNormalTable(NamedTuple):
    """What tuch_vertex_normals and the oriented cloud term read of a mesh: int32 device tensors faces [F,3] and the
    vertex -> faces lists (off [V+1], ids [3F]) of vertex_face_table."""
    faces: torch.Tensor
    off: torch.Tensor
    ids: torch.Tensor


def vertex_normal_table(faces, num_verts: int, device) -> VertexNormalTable:
    """faces [F,3] (array or tensor) -> the VertexNormalTable of the mesh on ``device``."""
    faces = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    off, ids = vertex_face_table(faces, num_verts)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=device)
    return VertexNormalTable(up(faces), up(off), up(ids))


def _check_normal_table(what, table, num_verts, device):
    if not isinstance(table, VertexNormalTable):
        raise ValueError('%s: the table must be a VertexNormalTable (ops.vertex_normal_table), got %r'
                         % (what, type(table).__name__))
    if table.off.numel() != num_verts + 1 or table.ids.numel() != 3 * table.faces.shape[0]:
        raise ValueError('%s: the table is for %d vertices and %d faces (%d entries), the vertices are %d'
                         % (what, table.off.numel() - 1, table.faces.shape[0], table.ids.numel(), num_verts))
    if table.faces.device != device:
        raise RuntimeError('%s: the table is on %s, the vertices on %s' % (what, table.faces.device, device))


def vertex_normals(verts: torch.Tensor, table: VertexNormalTable, normalize: bool = False) -> torch.Tensor:
    """Posed vertex normals [B,V,3] (tuch_vertex_normals; the rule is in include/tuch_amd.h): the sum of the normals
    (b - a) x (c - a) of every vertex's faces in ascending face order -- the area-weighted normal -- as one fixed
    float32 sequence; ``normalize`` makes them unit vectors, with a zero row where the sum is 0 or not finite.  The same
    bits for a vertex alone or in any batch.  No gradients; there is no host fallback."""
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[0] == 0 or verts.shape[1] == 0:
        raise ValueError('vertex_normals: verts must be [B,V,3] with B, V > 0, got %s' % (tuple(verts.shape),))
    _need_hip('vertex_normals', verts)
    _check_normal_table('vertex_normals', table, verts.shape[1], verts.device)
    v = _f32(verts.detach())
    b, n, _ = v.shape
    out = torch.empty_like(v)
    with torch.cuda.device(v.device):
        _C.check(_C.lib().tuch_vertex_normals(_C.ptr(v), _C.ptr(table.faces), _C.ptr(table.off), _C.ptr(table.ids), b, n,
                                              int(table.faces.shape[0]), int(bool(normalize)), _C.ptr(out), _C.stream()))
    return out


def render_mesh(verts: torch.Tensor, faces_i32: torch.Tensor, vface, cam_t: torch.Tensor, view_rot: torch.Tensor,
                focal: float, cx: float, cy: float, height: int, width: int, colors: Optional[torch.Tensor] = None,
                background: Optional[torch.Tensor] = None, background_views: int = 0) -> dict:
    """tuch_render_mesh (include/tuch_amd.h): verts [B,V,3], faces [F,3] int32, vface = (off [V+1], ids) int32 device
    tensors of vertex_face_table, cam_t [B,3], view_rot [n,3,3] -> {'face' [B,n,H,W] int32 (-1 = empty), 'depth' [B,n,H,W]
    (0 = empty), 'image' [B,n,H,W,3] in [0,1]}.  colors [B,V,3] uint8 or None (230); background [B,H,W,3] float32 or None,
    used by the views whose bit is set in background_views, white elsewhere.  One memset and three launches on the current
    stream, nothing else: capturable."""
    verts, cam_t, view_rot = _f32(verts), _f32(cam_t), _f32(view_rot)
    b, v, _ = verts.shape
    dev = verts.device
    n, h, w = int(view_rot.shape[0]), int(height), int(width)
    off, ids = vface
    if off.dtype != torch.int32 or ids.dtype != torch.int32 or off.numel() != v + 1:
        raise ValueError('vface must be the (off [V+1], ids) int32 tensors of vertex_face_table')
    if faces_i32.dtype != torch.int32 or faces_i32.dim() != 2 or faces_i32.shape[1] != 3:
        raise ValueError('faces must be [F, 3] int32')
    if cam_t.shape != (b, 3) or view_rot.shape[1:] != (3, 3):
        raise ValueError('cam_t must be [B, 3] and view_rot [n, 3, 3]')
    if colors is not None and (colors.dtype != torch.uint8 or colors.shape != (b, v, 3)):
        raise ValueError('colors must be [B, V, 3] uint8')
    if background is not None:
        background = _f32(background)
        if background.shape != (b, h, w, 3):
            raise ValueError('background must be [B, H, W, 3]')
    f = int(faces_i32.shape[0])
    L = _C.lib()
    out = {'face': torch.empty(b, n, h, w, dtype=torch.int32, device=dev),
           'depth': torch.empty(b, n, h, w, dtype=torch.float32, device=dev),
           'image': torch.empty(b, n, h, w, 3, dtype=torch.float32, device=dev)}
    nbytes = L.tuch_render_workspace_bytes(b, n, v, f, h, w)
    ws = _workspace(nbytes, dev)
    _C.check(L.tuch_render_mesh(_C.ptr(verts), _C.ptr(faces_i32), _C.ptr(off), _C.ptr(ids), b, v, f, _C.ptr(cam_t),
                                _C.ptr(view_rot), n, float(focal), float(cx), float(cy), h, w, _C.ptr(colors),
                                _C.ptr(background), int(background_views) & 0xffffffff, _C.ptr(out['face']),
                                _C.ptr(out['depth']), _C.ptr(out['image']), _C.ptr(ws), nbytes, _C.stream()))
    return out


def contact_vertex_colors(verts: torch.Tensor, pairs=None, regions=None) -> torch.Tensor:
    """tuch_contact_vertex_colors (include/tuch_amd.h): verts [B,V,3] -> colors [B,V,3] uint8, the reference's contact
    colouring (renderer.py:199-224).  Exactly one of
      pairs   = (off [B+1], c1 [N], c2 [N]) int32 device tensors: body b owns the pairs off[b] .. off[b+1];
      regions = (contact [B,P] uint8, pairs [P,2] int32, region_first [R] int32, vreg_off [V+1] int32, vreg int32).
    Three launches on the current stream: capturable."""
    if (pairs is None) == (regions is None):
        raise ValueError('give exactly one of pairs= and regions=')
    verts = _f32(verts)
    b, v, _ = verts.shape
    dev = verts.device
    colors = torch.empty(b, v, 3, dtype=torch.uint8, device=dev)
    L = _C.lib()
    none = _C.ptr(None)
    if pairs is not None:
        off, c1, c2 = pairs
        if any(t.dtype != torch.int32 for t in (off, c1, c2)) or off.numel() != b + 1 or c1.shape != c2.shape or c1.dim() != 1:
            raise ValueError('pairs must be (off [B+1], c1 [N], c2 [N]) int32 tensors')
        n = int(c1.numel())
        nbytes = L.tuch_contact_vertex_colors_workspace_bytes(b, v, 0)
        ws = _workspace(nbytes, dev)
        _C.check(L.tuch_contact_vertex_colors(_C.ptr(verts), b, v, _C.ptr(off), _C.ptr(c1) if n else none,
                                              _C.ptr(c2) if n else none, n, none, none, 0, none, none, none, 0,
                                              _C.ptr(colors), _C.ptr(ws), nbytes, _C.stream()))
        return colors
    contact, rp, first, voff, vreg = regions
    if contact.dtype != torch.uint8 or contact.dim() != 2 or contact.shape[0] != b:
        raise ValueError('contact must be [B, P] uint8')
    contact = contact.contiguous()
    p, r = int(contact.shape[1]), int(first.numel())
    if rp.dtype != torch.int32 or rp.shape != (p, 2) or first.dtype != torch.int32 or voff.dtype != torch.int32 \
            or vreg.dtype != torch.int32 or voff.numel() != v + 1 or p == 0 or r == 0:
        raise ValueError('regions must be (contact [B,P] uint8, pairs [P,2], region_first [R], vreg_off [V+1], vreg) int32')
    if vreg.numel() == 0:
        vreg = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = L.tuch_contact_vertex_colors_workspace_bytes(b, v, r)
    ws = _workspace(nbytes, dev)
    _C.check(L.tuch_contact_vertex_colors(_C.ptr(verts), b, v, none, none, none, 0, _C.ptr(contact),
                                          _C.ptr(rp), p, _C.ptr(first), _C.ptr(voff), _C.ptr(vreg), r, _C.ptr(colors),
                                          _C.ptr(ws), nbytes, _C.stream()))
    return colors


class _ContactTerms(torch.autograd.Function):
    """terms[b] = (interior sum, exterior sum); gradient flows to the points only."""

    @staticmethod
    def forward(ctx, points, partner, exterior, valid, mode, euclthres, grad_masked=False):
        pts = _f32(points)
        b, n, _ = pts.shape
        terms = torch.empty(b, 2, dtype=torch.float32, device=pts.device)
        _C.check(_C.lib().tuch_contact_terms_fwd(_C.ptr(pts), _C.ptr(partner), _C.ptr(exterior), _C.ptr(valid),
                                                 b, n, int(mode), float(euclthres), _C.ptr(terms), _C.stream()))
        ctx.save_for_backward(pts, partner, exterior, valid)
        ctx.mode, ctx.euclthres = int(mode), float(euclthres)
        ctx.grad_masked = bool(grad_masked)     # the caller reduces the terms with valid_mean: its gradient is 0 for the others
        return terms

    @staticmethod
    def backward(ctx, grad_terms):
        pts, partner, exterior, valid = ctx.saved_tensors
        b, n, _ = pts.shape
        g = grad_terms.to(torch.float32)
        if valid is not None and not ctx.grad_masked:
            g = g * valid.to(g.dtype)[:, None]
        g = g.contiguous()   # [B,2]: upstream gradient of the interior and of the exterior sum
        if deterministic():
            # 64-bit fixed-point accumulators + integer atomics: the plain training term's gradient is bit-reproducible too
            fixed = torch.zeros(b * n * 3, dtype=torch.int64, device=pts.device)
            grad = torch.empty_like(pts)
            _C.check(_C.lib().tuch_contact_terms_bwd_fixed(_C.ptr(pts), _C.ptr(partner), _C.ptr(exterior), _C.ptr(g), b, n,
                                                           ctx.mode, ctx.euclthres, _C.ptr(fixed), _C.ptr(grad), _C.stream()))
            return grad, None, None, None, None, None, None
        grad = torch.zeros_like(pts)
        _C.check(_C.lib().tuch_contact_terms_bwd(_C.ptr(pts), _C.ptr(partner), _C.ptr(exterior), _C.ptr(g),
                                                 b, n, ctx.mode, ctx.euclthres, _C.ptr(grad), _C.stream()))
        return grad, None, None, None, None, None, None


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


class _ContactTermsRagged(torch.autograd.Function):
    """terms[b] over the ragged point set of body b (HD points): points [N,3], global partner indices."""

    @staticmethod
    def forward(ctx, points, partner, exterior, offsets, body_of_point, mode, euclthres):
        pts = _f32(points)
        b = offsets.shape[0] - 1
        terms = torch.empty(b, 2, dtype=torch.float32, device=pts.device)
        _C.check(_C.lib().tuch_contact_terms_ragged_fwd(_C.ptr(pts), _C.ptr(partner), _C.ptr(exterior),
                                                        _C.ptr(offsets), b, int(mode), float(euclthres),
                                                        _C.ptr(terms), _C.stream()))
        ctx.save_for_backward(pts, partner, exterior, body_of_point)
        ctx.mode, ctx.euclthres = int(mode), float(euclthres)
        return terms

    @staticmethod
    def backward(ctx, grad_terms):
        pts, partner, exterior, body_of_point = ctx.saved_tensors
        grad = torch.zeros_like(pts)
        g = grad_terms.to(torch.float32).contiguous()
        _C.check(_C.lib().tuch_contact_terms_ragged_bwd(_C.ptr(pts), _C.ptr(partner), _C.ptr(exterior),
                                                        _C.ptr(body_of_point), _C.ptr(g), pts.shape[0], ctx.mode,
                                                        ctx.euclthres, _C.ptr(grad), _C.stream()))
        return grad, None, None, None, None, None, None


def contact_terms_ragged(points, partner_i32, exterior_u8, offsets_i32, body_of_point_i32, mode, euclthres):
    """[B,2] (interior sum, exterior sum) per body over a concatenated ragged point set."""
    return _ContactTermsRagged.apply(points, partner_i32, exterior_u8, offsets_i32, body_of_point_i32, mode,
                                     euclthres)


def contact_terms(points, partner_i32, exterior_u8, valid_u8, mode, euclthres):
    """Sum of pull/push terms per body: [B] = interior + exterior (differentiable wrt points)."""
    terms = _ContactTerms.apply(points, partner_i32, exterior_u8, valid_u8, mode, euclthres)
    return terms.sum(dim=1), terms


class _ValidMean(torch.autograd.Function):
    """sum of terms [B,K] over the valid bodies / their number (loss.py:317), one launch each way."""

    @staticmethod
    def forward(ctx, terms, valid_u8):
        t = _f32(terms)
        b = t.shape[0]
        k = t.numel() // b
        out = torch.empty(2, dtype=torch.float32, device=t.device)
        _C.check(_C.lib().tuch_valid_mean_fwd(_C.ptr(t), _C.ptr(valid_u8), b, k, _C.ptr(out), _C.stream()))
        ctx.save_for_backward(out, valid_u8)
        ctx.shape = tuple(terms.shape)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        out, valid_u8 = ctx.saved_tensors
        b = ctx.shape[0]
        k = int(torch.Size(ctx.shape).numel()) // b
        grad = torch.empty(ctx.shape, dtype=torch.float32, device=out.device)
        up = g.to(torch.float32).reshape(1).contiguous()
        _C.check(_C.lib().tuch_valid_mean_bwd(_C.ptr(up), _C.ptr(out), _C.ptr(valid_u8), b, k, _C.ptr(grad), _C.stream()))
        return grad, None


def as_u8(mask):
    """A [B] boolean / byte mask as uint8 without a copy where the bytes are already there."""
    if mask.dtype == torch.bool and mask.is_contiguous():
        return mask.view(torch.uint8)
    return mask.to(torch.uint8).contiguous()


def valid_mean(terms, valid_u8):
    """Scalar: terms [B,...] summed over the bodies with valid != 0, divided by their number (NaN when there is none, like
    the reference's ``loss.sum() / valid_fit.sum()``, loss.py:317).  The gradient of the other bodies' terms is 0."""
    return _ValidMean.apply(terms, valid_u8)


def contact_terms_mean(points, partner_i32, exterior_u8, valid_u8, mode, euclthres):
    """``contact_terms(...)[0].sum() / valid.sum()`` of RegressorLoss.contact_loss (loss.py:259-272, 317) in two launches
    forward and two backward."""
    terms = _ContactTerms.apply(points, partner_i32, exterior_u8, valid_u8, mode, euclthres, True)
    return valid_mean(terms, valid_u8)


class _SmallTerms(torch.autograd.Function):
    """Reprojection + max-mixture prior of the SMPLify-DC objective in one kernel; returns [B,2]."""

    @staticmethod
    def forward(ctx, joints, camera_t, body_pose, camera_center, joints_2d, joints_conf, means, precisions,
                log_weights, focal, sigma, prior_scale):
        j = _f32(joints)
        b, nj, _ = j.shape
        out = torch.empty(b, 2, dtype=torch.float32, device=j.device)
        gj = torch.empty_like(j)
        gc = torch.empty(b, 3, dtype=torch.float32, device=j.device)
        gp = torch.empty(b, 69, dtype=torch.float32, device=j.device) if body_pose is not None else None
        # bound to locals: a converted copy must stay alive until the kernel has been enqueued
        cam_t, cam_c, j2d, conf = _f32(camera_t), _f32(camera_center), _f32(joints_2d), _f32(joints_conf)
        pose = _f32(body_pose) if body_pose is not None else None
        _C.check(_C.lib().tuch_smplify_small_terms(
            _C.ptr(j), _C.ptr(cam_t), _C.ptr(cam_c), _C.ptr(j2d), _C.ptr(conf), _C.ptr(pose),
            _C.ptr(means), _C.ptr(precisions), _C.ptr(log_weights), b, nj,
            means.shape[0] if means is not None else 0, float(focal), float(sigma), float(prior_scale),
            _C.ptr(out), _C.ptr(gj), _C.ptr(gc), _C.ptr(gp), _C.stream()))
        ctx.save_for_backward(gj, gc, gp)
        return out

    @staticmethod
    def backward(ctx, g):
        gj, gc, gp = ctx.saved_tensors
        g_rep, g_pri = g[:, 0].contiguous(), g[:, 1].contiguous()
        return (gj * g_rep[:, None, None], gc * g_rep[:, None],
                gp * g_pri[:, None] if gp is not None else None) + (None,) * 9


def smplify_small_terms(joints, camera_t, body_pose, camera_center, joints_2d, joints_conf, means, precisions,
                        log_weights, focal, sigma, prior_scale):
    return _SmallTerms.apply(joints, camera_t, body_pose, camera_center, joints_2d, joints_conf, means,
                             precisions, log_weights, focal, sigma, prior_scale)


class _Objective(torch.autograd.Function):
    """sum(small) + contact_scale * sum(terms) + r2r_scale * sum(r2r) as one deterministic kernel."""

    @staticmethod
    def forward(ctx, small, terms, r2r, contact_scale, r2r_scale):
        small, terms = small.contiguous(), terms.contiguous()
        b = small.shape[0]
        p = r2r.shape[1] if r2r is not None else 0
        out = torch.empty(1, dtype=torch.float32, device=small.device)
        r2r_c = r2r.contiguous() if p else None
        _C.check(_C.lib().tuch_smplify_objective(_C.ptr(small), _C.ptr(terms), _C.ptr(r2r_c), b, p,
                                                 float(contact_scale), float(r2r_scale), _C.ptr(out), _C.stream()))
        ctx.shape = (b, p, float(contact_scale), float(r2r_scale))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        b, p, cs, rs = ctx.shape
        g = g.reshape(1).to(torch.float32).contiguous()
        gs = torch.empty(b, 2, dtype=torch.float32, device=g.device)
        gt = torch.empty(b, 2, dtype=torch.float32, device=g.device)
        gr = torch.empty(b, p, dtype=torch.float32, device=g.device) if p else None
        _C.check(_C.lib().tuch_smplify_objective_bwd(_C.ptr(g), b, p, cs, rs, _C.ptr(gs), _C.ptr(gt), _C.ptr(gr),
                                                     _C.stream()))
        return gs, gt, gr, None, None


def smplify_objective(small, terms, r2r, contact_scale, r2r_scale):
    return _Objective.apply(small, terms, r2r, contact_scale, r2r_scale)


_TICKETS = {}


def _ticket(device) -> torch.Tensor:
    """A zeroed int: the arrival counter of kernels whose last block finishes the job (they leave it zero).
    Eager calls: one per (device, stream) -- calls on one stream are ordered, so they can share it; another stream gets its
    own.  Under hipGraph capture: a counter of the call's own, allocated from the capturing graph's pool and cleared by a
    memset node of that graph -- a captured graph may be replayed on ANY stream, beside other graphs that were captured on
    the same (shared) capture stream, so a counter keyed by the capture stream would be shared by launches that are not
    ordered against each other (and would live in the pool of whichever graph happened to be captured first)."""
    if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
        return torch.zeros(1, dtype=torch.int32, device=device)
    key = (device.index, _current_stream(device).cuda_stream)
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


def _rows_of(t, b, tail, name):
    """float32, contiguous, [b, *tail]; a batch of one is broadcast like the torch-op form would (the kernels index raw
    pointers by body: any other shape would be an out-of-bounds read)."""
    t = _f32(t)
    if t.dim() == len(tail) + 1 and t.shape[0] == 1 and b > 1:
        t = t.expand(b, *t.shape[1:]).contiguous()
    if tuple(t.shape) != (b,) + tuple(tail):
        raise ValueError('stage-1 objective: %s has shape %s, expected %s' % (name, tuple(t.shape), (b,) + tuple(tail)))
    return t


class _Stage1Objective(torch.autograd.Function):
    """camera_fitting_loss (tuch/smplify/losses.py:125-152) as ONE launch: reprojection + depth term + shape prior, the
    scalar total and the unit gradients w.r.t. joints / camera translation / betas (csrc/small_terms.hip:
    stage1_terms_kernel).  backward() only hands the gradients over (scaled unless the upstream gradient is the cached
    unit seed of ops.backward_scalar)."""

    @staticmethod
    def forward(ctx, joints, camera_t, betas, camera_t_est, camera_center, joints_2d, joints_conf, focal, sigma, depth_w,
                shape_w):
        j = _f32(joints)
        if j.dim() != 3 or j.shape[2] != 3:
            raise ValueError('stage-1 objective: joints must be [B,J,3], got %s' % (tuple(j.shape),))
        b, nj, _ = j.shape
        ct = _rows_of(camera_t, b, (3,), 'camera_t')
        be = None
        if betas is not None and shape_w != 0.0:
            if betas.dim() != 2:
                raise ValueError('stage-1 objective: betas must be [B,n], got %s' % (tuple(betas.shape),))
            be = _rows_of(betas, b, (betas.shape[1],), 'betas')
        est, cc = _rows_of(camera_t_est, b, (3,), 'camera_t_est'), _rows_of(camera_center, b, (2,), 'camera_center')
        j2d, conf = _rows_of(joints_2d, b, (nj, 2), 'joints_2d'), _rows_of(joints_conf, b, (nj,), 'joints_conf')
        out = torch.empty(1, dtype=torch.float32, device=j.device)
        share = torch.empty(b, dtype=torch.float32, device=j.device)
        gj = torch.empty_like(j)
        gc = torch.empty(b, 3, dtype=torch.float32, device=j.device)
        gb = torch.empty_like(be) if be is not None else None
        _C.check(_C.lib().tuch_smplify_stage1_terms(
            _C.ptr(j), _C.ptr(ct), _C.ptr(est), _C.ptr(cc), _C.ptr(j2d), _C.ptr(conf), _C.ptr(be), b, nj,
            be.shape[1] if be is not None else 0, float(focal), float(sigma), float(depth_w), float(shape_w), _C.ptr(share),
            _C.ptr(_ticket(j.device)), _C.ptr(out), _C.ptr(gj), _C.ptr(gc), _C.ptr(gb), _C.stream()))
        ctx.save_for_backward(gj, gc, gb)
        ctx.in_dtypes = (joints.dtype, camera_t.dtype, betas.dtype if betas is not None else None)
        ctx.in_shapes = (tuple(camera_t.shape), tuple(betas.shape) if betas is not None else None)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gj, gc, gb = ctx.saved_tensors
        if not backward_pass.is_unit_seed(g):
            g = g.reshape(()).to(torch.float32)
            gj, gc, gb = gj * g, gc * g, (gb * g if gb is not None else None)
        dj, dc, db = ctx.in_dtypes
        sc, sb = ctx.in_shapes
        if tuple(gc.shape) != sc:                     # a broadcast batch of one: its gradient is the sum over the bodies
            gc = gc.sum(0, keepdim=True)
        if gb is not None and tuple(gb.shape) != sb:
            gb = gb.sum(0, keepdim=True)
        return (gj.to(dj), gc.to(dc), gb.to(db) if gb is not None else None) + (None,) * 8


def smplify_stage1_objective(joints, camera_t, betas, camera_t_est, camera_center, joints_2d, joints_conf, focal, sigma,
                             depth_weight, shape_weight):
    return _Stage1Objective.apply(joints, camera_t, betas, camera_t_est, camera_center, joints_2d, joints_conf, focal, sigma,
                                  depth_weight, shape_weight)


def _need_hip(what, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('%s runs on a HIP device (there is no host fallback); got a tensor on %s' % (what, t.device))


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


def _hand_over(ctx, g, num_inputs, expand=None):
    """backward() of the fit terms (_VertexFit, _ScanFit, _CloudFit): the saved unit gradients (None where one was not
    asked for), scaled unless the upstream gradient g is the cached unit seed of ops.backward_scalar, then expand(*grads)
    where the inputs that get one are more than the saved tensors, each cast to its input's dtype (ctx.in_dtypes: the
    leading inputs); None for every other input, and for all of them when g is None."""
    if g is None:
        return (None,) * num_inputs
    grads = ctx.saved_tensors
    if not backward_pass.is_unit_seed(g):
        g = g.reshape(()).to(torch.float32)
        grads = tuple(None if x is None else x * g for x in grads)
    if expand is not None:
        grads = expand(*grads)
    return tuple(None if x is None else x.to(d) for x, d in zip(grads, ctx.in_dtypes)) + (None,) * (num_inputs - len(grads))


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


class _Stage2Tail(torch.autograd.Function):
    """Everything of the stage-2 objective behind the body model as ONE autograd node (tuch/smplify/losses.py:56-123):
    inside test + nearest admissible vertex (no gradient), contact sums, region minima, reprojection + prior, the
    weighted total.  The same kernels as the separate nodes (_SmallTerms, _ContactTerms, _RegionPairMin, _Objective);
    what goes away is the torch glue between them -- in the backward pass ~10 small launches per step (scalings by the
    upstream gradient, dtype / layout copies, a zero fill and an add per gradient path into the vertices).  Backward:
    one kernel turns the upstream scalar into the weights of every term, then the contact and region kernels
    accumulate into one vertex gradient."""

    @staticmethod
    def forward(ctx, verts, joints, camera_t, body_pose, model, valid, select, const):
        v, j = _f32(verts), _f32(joints)
        cam_t, pose = _f32(camera_t), _f32(body_pose)
        b, nj, _ = j.shape
        L = _C.lib()
        cam_c, j2d, conf = _f32(const['camera_center']), _f32(const['joints_2d']), _f32(const['joints_conf'])
        means, precisions, logw = const['means'], const['precisions'], const['log_weights']
        small = torch.empty(b, 2, dtype=torch.float32, device=v.device)
        gj = torch.empty_like(j)
        gc = torch.empty(b, 3, dtype=torch.float32, device=v.device)
        gp = torch.empty(b, 69, dtype=torch.float32, device=v.device)
        p = model.num_pairs if select is not None else 0

        # ONE cleared buffer: the vertex gradient the unit backward accumulates into, the arrival counter of the
        # tail kernel ("the last block adds up": it belongs to THIS call -- no counter shared between streams, none
        # left non-zero by an aborted launch) and the region pairs' keys (tuch_region_pair_keys wants them zero).  It is
        # cleared by the FIRST kernel of the search (a fill launch of its own was 5 us of the second stream's chain).
        n = v.numel()
        k0 = n + 1 + ((n + 1) & 1)                  # the 64-bit keys start on an even word behind the counter
        det = 2 * n if deterministic() else 0       # deterministic mode: 64-bit fixed-point accumulators

        def beside_the_walk(zeros):          # on the second stream (ContactModel.exterior_and_partner), behind the search
            keys = zeros[k0:k0 + 2 * b * p].view(torch.int64) if p else None
            fixed = zeros[k0 + 2 * b * p:k0 + 2 * b * p + det].view(torch.int64) if det else None
            if p:
                _C.check(L.tuch_region_pair_keys(model._handle, _C.ptr(v), b, _C.ptr(select), 1, _C.ptr(keys), _C.stream()))
            _C.check(L.tuch_smplify_small_terms(
                _C.ptr(j), _C.ptr(cam_t), _C.ptr(cam_c), _C.ptr(j2d), _C.ptr(conf), _C.ptr(pose), _C.ptr(means),
                _C.ptr(precisions), _C.ptr(logw), b, nj, means.shape[0], float(const['focal']), float(const['sigma']),
                float(const['prior_scale']), _C.ptr(small), _C.ptr(gj), _C.ptr(gc), _C.ptr(gp), _C.stream()))
            return (keys, fixed, small, gj, gc, gp, zeros[:n].view(v.shape), zeros[n:n + 1].view(torch.int32))
        exterior, _, partner, _extra = model.exterior_and_partner(v, apply_segments=const['apply_segments'],
                                                                  also=beside_the_walk, zero_floats=k0 + 2 * b * p + det,
                                                                  iterative=True)       # SMPLify-DC's stage-2 loop
        out = torch.empty(1, dtype=torch.float32, device=v.device)
        share = torch.empty(L.tuch_smplify_stage2_fused_scratch_floats(b), dtype=torch.float32, device=v.device)
        # the objective is the root of the fit's graph: its vertex gradient for a unit upstream gradient is written by the
        # same launch that forms the sums (csrc/contact_terms.hip: stage2_fused_kernel); backward() only hands it over
        want_grad = any(ctx.needs_input_grad[:4])
        gv = _extra[6] if want_grad else None
        # deterministic mode: the vertex gradient stays in its 64-bit fixed-point accumulators (no conversion launch here);
        # backward() hands them to the body model's node, whose skinning adjoint reads them -- or converts them if the pass
        # is not the plain `objective.backward()` of a fit.  gv (zeros nobody writes in this mode) is what autograd carries.
        fixed = _extra[1] if want_grad else None
        _C.check(L.tuch_smplify_stage2_fused(_C.ptr(v), _C.ptr(partner), _C.ptr(exterior), _C.ptr(valid), b, v.shape[1],
                                             MODE_SMPLIFY, float(const['euclthres']), _C.ptr(small), p,
                                             float(const['contact_scale']), float(const['r2r_scale']), _C.ptr(share),
                                             _C.ptr(_extra[7]), _C.ptr(out), _C.ptr(gv) if fixed is None else None,
                                             model._handle if p else None, _C.ptr(_extra[0]),
                                             _C.ptr(fixed), _C.stream()))
        if want_grad:
            # (fixed: a view of gv's buffer, only read by backward() and the skinning adjoint; saved like the others, so a
            # retained graph's next pass finds it again and a plain pass releases the buffer where it always did)
            ctx.save_for_backward(gv, gj, gc, gp, fixed)
        ctx.in_dtypes = (verts.dtype, joints.dtype, camera_t.dtype, body_pose.dtype)
        # body_pose also feeds the body model that made `verts`: that node's backward runs after this one and can add the prior's
        # pose gradient inside its own last kernel (backward_pass.Handover): autograd then has no two gradients to sum in a launch
        node = verts.grad_fn
        ctx.verts_ref = weakref.ref(verts)          # backward() asks whether somebody watches the vertices' own gradient
        ref = getattr(node, 'pose_ref', None) if node is not None else None
        ctx.lbs_node = node if (want_grad and ctx.needs_input_grad[0] and ctx.needs_input_grad[3] and ref is not None
                                and ref() is body_pose) else None
        return out[0]

    @staticmethod
    @once_differentiable          # the gradients were formed in forward(): constants of a second differentiation
    def backward(ctx, g):
        gv, gj, gc, gp, fixed = ctx.saved_tensors
        dv, dj, dc, dp = ctx.in_dtypes
        # (the rules of what follows: the table of backward_pass.  root: not a loss like `tail + other(body_pose)`, which
        # reaches this node with the same unit seed, but whose pose gradient does not all flow through here)
        task = backward_pass.pass_id()
        unit = backward_pass.is_unit_seed(g)
        root = unit and backward_pass.is_root(ctx)
        leave = ctx.lbs_node is not None and task >= 0
        # (somebody who retains / hooks the vertices' own gradient must see the real numbers, not the carrier of zeros;
        # asked NOW: both can be added after the loss was built.  Nobody holds a tensor that is gone: no .grad to fill)
        verts = ctx.verts_ref()
        watched = verts is not None and (verts.retains_grad or bool(getattr(verts, '_backward_hooks', None)))
        hand_over = fixed is not None and leave and root and not watched
        if fixed is not None and not hand_over:
            # anything but the plain backward of a fit (scaled, watched vertices, further terms): the float gradient, converted
            gv = torch.empty_like(gv)
            _C.check(_C.lib().tuch_fixed_to_float(_C.ptr(fixed), fixed.numel(), _C.ptr(gv), _C.stream()))
        if not unit:
            g = g.reshape(()).to(torch.float32)
            gv, gj, gc, gp = gv * g, gj * g, gc * g, gp * g
        left = leave and backward_pass.leave(ctx.lbs_node, backward_pass.Handover(task, gp, fixed if hand_over else None, root))
        return gv.to(dv), gj.to(dj), gc.to(dc), None if left else gp.to(dp), None, None, None, None


def smplify_stage2_tail(verts, joints, camera_t, body_pose, model, valid_u8, select_u8, **const):
    """Scalar stage-2 objective behind the body model (see _Stage2Tail); const: camera_center, joints_2d, joints_conf,
    means, precisions, log_weights, focal, sigma, prior_scale, euclthres, contact_scale, r2r_scale, apply_segments."""
    return _Stage2Tail.apply(verts, joints, camera_t, body_pose, model, valid_u8, select_u8, const)


_DERIVED = {}


def cached_derived(key_tensors, build):
    """Small per-call tensors derived from caller inputs that do not change between iterations
    (validity / selection masks): rebuilt only when an input was modified in place or replaced.  The
    entry holds its source tensors, so their addresses cannot be reused while it is cached.  A captured
    hipGraph holds the address of the derived tensor: entries are kept for 256 distinct inputs before the oldest
    is dropped, far more than the graphs a process keeps alive at once."""
    key = tuple((t.data_ptr(), t._version, tuple(t.shape)) if t is not None else None for t in key_tensors)
    hit = _DERIVED.get(key)
    if hit is None:
        while len(_DERIVED) >= 256:
            _DERIVED.pop(next(iter(_DERIVED)))
        hit = (build(), key_tensors)
        _DERIVED[key] = hit
    return hit[0]


# ------------------------------------------------------------------------- model
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


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)


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
        cos = _max_angle_cos(normals, max_angle, points, 'closest_point')
        if verts.dim() != 3 or points.dim() != 3 or verts.shape[0] != points.shape[0] or verts.shape[1] != self.num_verts:
            raise _C.TuchError('closest_point: verts [B,%d,3] and points [B,Q,3] expected, got %s and %s'
                               % (self.num_verts, tuple(verts.shape), tuple(points.shape)))
        if counts is not None:
            counts = counts.to(torch.int32).contiguous()
        hint = _hint_of(hint, points, 'closest_point')
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


class ClosestPoint(NamedTuple):
    d2: torch.Tensor
    face: torch.Tensor
    bary: torch.Tensor


def _hint_of(hint, points, what):
    """hint as the kernels read it: int32 [B,Q] on the points' device, contiguous (the tensor itself where it already is:
    a loop's hint tensor may be the one the faces are written to)."""
    if hint is None:
        return None
    if tuple(hint.shape) != tuple(points.shape[:2]) or hint.device != points.device:
        raise _C.TuchError('%s: hint must be [B,Q] = %s on %s, got %s on %s'
                           % (what, tuple(points.shape[:2]), points.device, tuple(hint.shape), hint.device))
    return hint.to(torch.int32).contiguous()


def _max_angle_cos(normals, max_angle, points, what):
    """None without normals and angle; otherwise the float32 cosine the C entry points take: cos(max_angle) in double,
    rounded once.  One of the two alone, an angle outside (0, 90] degrees or normals of another shape raise ValueError."""
    if not _both(what, 'normals', normals, 'max_angle', max_angle):
        return None
    angle = _angle_of(what, 'max_angle', max_angle)
    if not torch.is_tensor(normals) or tuple(normals.shape) != tuple(points.shape) or normals.device != points.device:
        raise ValueError('%s: normals must be [B,Q,3] = %s on %s, got %s'
                         % (what, tuple(points.shape), points.device,
                            (tuple(normals.shape), normals.device) if torch.is_tensor(normals) else type(normals)))
    cos = float(np.float32(math.cos(math.radians(angle))))
    # (90 degrees: cos is 6e-17 in double; anything in [0, 1) is the contract)
    return min(max(cos, 0.0), float(np.nextafter(np.float32(1.0), np.float32(0.0))))


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


SCAN_RHO = {'squared': 0, 'distance': 1, 'gmof': 2}


def _rho_of(what, rho, sigma):
    """(rho, sigma) as the C entry points of scan_fit and cloud_fit take them."""
    if rho not in SCAN_RHO:
        raise ValueError('%s: rho must be one of %s, got %r' % (what, sorted(SCAN_RHO), rho))
    if rho == 'gmof' and not (sigma is not None and float(sigma) > 0.0):
        raise ValueError("%s: rho='gmof' needs sigma > 0, got %r" % (what, sigma))
    return SCAN_RHO[rho], float(sigma) if sigma is not None else 0.0


def _angle_of(what, name, max_angle) -> float:
    """The largest normal angle in degrees, in (0, 90]; ``name`` is what the caller's argument is called."""
    angle = float(max_angle)
    if not (0.0 < angle <= 90.0):
        raise ValueError('%s: %s must be in (0, 90] degrees, got %r' % (what, name, max_angle))
    return angle


def _resolution_of(what, resolution) -> int:
    """Cells of a PointCloud's grid along the longest extent."""
    if not (isinstance(resolution, int) and 1 <= resolution <= 256):
        raise ValueError('%s: resolution must be an int in 1 .. 256, got %r' % (what, resolution))
    return resolution


def _counts_of(what, counts, b):
    """counts [B] (real entries per body) as the C entry points take it: int32, contiguous; None stays None."""
    if counts is None:
        return None
    if tuple(counts.shape) != (b,):
        raise ValueError('%s: counts must be [%d], got %s' % (what, b, tuple(counts.shape)))
    return counts.to(torch.int32).contiguous()


def _check_weights(what, weights, b, q):
    if weights is not None and tuple(weights.shape) != (b, q):
        raise ValueError('%s: weights must be [%d,%d], got %s' % (what, b, q, tuple(weights.shape)))


def _both(what, name_a, a, name_b, b) -> bool:
    """Two arguments that go together: False with neither, True with both; one alone raises."""
    if (a is None) != (b is None):
        raise ValueError('%s: %s and %s go together, got %s only' % (what, name_a, name_b, name_b if a is None else name_a))
    return a is not None


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
    rho, sigma = _rho_of('scan_fit', rho, sigma)
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
    cos = _max_angle_cos(normals, max_angle, points, 'scan_fit')
    _check_weights('scan_fit', weights, b, q)
    counts = _counts_of('scan_fit', counts, b)
    _need_hip('scan_fit', verts, transl, points, weights, counts, hint, face_out, normals)
    if face_out is not None and (tuple(face_out.shape) != (b, q) or face_out.dtype != torch.int32 or not face_out.is_contiguous()):
        raise ValueError('scan_fit: face_out must be a contiguous int32 [%d,%d] tensor' % (b, q))
    weights = None if weights is None else _f32(weights.detach())
    hint = _hint_of(hint, points, 'scan_fit')
    face = face_out if face_out is not None else torch.empty(b, q, dtype=torch.int32, device=points.device)
    normals = None if cos is None else _f32(normals.detach())
    total, per_body, d2, bary = _ScanFit.apply(verts, transl, points, model, counts, weights, hint, rho, sigma, face, normals, cos)
    return total, per_body, ClosestPoint(d2, face, bary)


class NearestPoint(NamedTuple):
    d2: torch.Tensor
    index: torch.Tensor


class KNearest(NamedTuple):
    d2: torch.Tensor
    index: torch.Tensor


class PointNormals(NamedTuple):
    normal: torch.Tensor
    variation: torch.Tensor
    count: torch.Tensor
    cov: Optional[torch.Tensor]


MAX_NEIGHBOURS = 32


def _check_k(what, k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_NEIGHBOURS:
        raise ValueError('%s: k must be an int in 1 .. %d, got %r' % (what, MAX_NEIGHBOURS, k))


class CloudGrid(NamedTuple):
    """Host copies of a PointCloud's per-body headers: origin [B,3] float32, cell [B] float32, dims [B,3] int32."""
    origin: np.ndarray
    cell: np.ndarray
    dims: np.ndarray


def set_cloud_canary(on: bool) -> bool:
    """Guard words behind the regions of every PointCloud workspace sized from now on (tuch_point_cloud_set_canary:
    process-wide; set it before constructing the cloud).  Returns the previous setting."""
    return bool(_C.lib().tuch_point_cloud_set_canary(int(bool(on))))


class _CloudNearest(torch.autograd.Function):
    """PointCloud.nearest: tuch_point_cloud_nearest forward; backward is 2 g (q - s) for queries and its sum over a body's
    queries for shift, the index held fixed (a handful of element-wise torch ops: not on any loop's path -- the loops
    use cloud_fit, whose gradients come out of the kernel)."""

    @staticmethod
    def forward(ctx, queries, shift, cloud, counts, hint, tau, index, query_normals, cos):
        qs = _f32(queries)
        sh = None if shift is None else _f32(shift)
        b, n, _ = qs.shape
        d2 = torch.empty(b, n, dtype=torch.float32, device=qs.device)
        # (the points' normals go with the queries': an oriented cloud asked without them answers the plain query)
        normals = None if query_normals is None else cloud.point_normals
        _C.check(_C.lib().tuch_point_cloud_nearest(
            _C.ptr(cloud._ws), cloud._nbytes, _C.ptr(cloud.points), _C.ptr(cloud.counts), _C.ptr(cloud.weights),
            _C.ptr(normals), _C.ptr(qs), _C.ptr(query_normals), _C.ptr(sh), _C.ptr(counts), _C.ptr(hint), tau, cos or 0.0,
            _C.ptr(cloud._cones), cloud._cones_bytes(), b, cloud.num_points, n, _C.ptr(d2), _C.ptr(index), _C.stream()))
        ctx.save_for_backward(qs, sh, index)
        ctx.cloud_points = cloud.points
        ctx.in_dtypes = (queries.dtype, None if shift is None else shift.dtype)
        return d2

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        qs, sh, index = ctx.saved_tensors
        won = index >= 0
        s = torch.gather(ctx.cloud_points, 1, index.clamp(min=0).long()[:, :, None].expand(-1, -1, 3))
        q = qs if sh is None else qs + sh[:, None]
        zero = torch.zeros((), dtype=torch.float32, device=qs.device)
        gq = torch.where(won[:, :, None], 2.0 * g.to(torch.float32)[:, :, None] * (q - s), zero)
        dq, ds = ctx.in_dtypes
        return (gq.to(dq) if ctx.needs_input_grad[0] else None,
                gq.sum(1).to(ds) if sh is not None and ctx.needs_input_grad[1] else None) + (None,) * 7


class PointCloud:
    """A batch of static point clouds with a uniform grid per body for exact nearest-point queries
    (csrc/point_cloud.hip; the rule is in include/tuch_amd.h).  ``PointCloud(points [B,Q,3], counts=None, weights=None,
    resolution=64)`` owns the workspace and builds on construction, on the current stream.  The cloud of body b is its
    VALID points: index < counts[b], weight != 0, finite.  The tensors are kept by reference (float32 contiguous inputs
    are not copied): change them in place and call ``rebuild()``.  There is no host fallback."""

    def __init__(self, points, counts=None, weights=None, resolution=64):
        self.resolution = _resolution_of('PointCloud', resolution)
        self._ws = None
        self.rebuild(points, counts, weights)

    def rebuild(self, points, counts=None, weights=None):
        """Build again, in place where the batch and point counts are unchanged (the workspace is kept): for a session
        that keeps its buffers.  Capturable."""
        if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] == 0 or points.shape[1] == 0:
            raise ValueError('PointCloud: points must be [B,Q,3] with B, Q > 0, got %s' % (tuple(points.shape),))
        b, q = points.shape[0], points.shape[1]
        counts = _counts_of('PointCloud', counts, b)
        _check_weights('PointCloud', weights, b, q)
        _need_hip('PointCloud', points, counts, weights)
        self.points = _f32(points)
        self.counts = counts
        self.weights = None if weights is None else _f32(weights)
        L = _C.lib()
        nbytes = L.tuch_point_cloud_workspace_bytes(b, q, self.resolution)
        if self._ws is None or self._nbytes != nbytes or self._ws.device != points.device:
            # (zeroed once: the first word counts changed guard words under the canary option)
            self._ws = torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device=points.device)
            self._nbytes = nbytes
        self.batch, self.num_points = b, q
        # a rebuild leaves the cloud unoriented (the cones would be stale): call orient() again; the cone buffer is kept
        self.point_normals = None
        self._cones = None
        with torch.cuda.device(points.device):
            _C.check(L.tuch_point_cloud_build(_C.ptr(self.points), _C.ptr(self.counts), _C.ptr(self.weights), b, q,
                                              self.resolution, _C.ptr(self._ws), nbytes, _C.stream()))
        return self

    def orient(self, normals, cones=True):
        """Give the cloud its points' normals [B,Q,3], in the points' order (kept by reference like the points; zero or
        non-finite rows mean "unknown"), for ``nearest(query_normals=, max_angle=)`` and ``cloud_fit(max_angle=)``.
        ``cones``: also build the per-block normal cones that let a query pass by blocks of the grid without an
        admissible point (tuch_point_cloud_build_cones, one launch, capturable; they change no bit of any result).
        ``rebuild()`` drops both: call ``orient`` again after it."""
        if not torch.is_tensor(normals) or tuple(normals.shape) != (self.batch, self.num_points, 3):
            raise ValueError('PointCloud.orient: normals must be [%d,%d,3], got %s'
                             % (self.batch, self.num_points, tuple(normals.shape) if torch.is_tensor(normals) else type(normals)))
        _need_hip('PointCloud.orient', normals)
        if normals.device != self.points.device:
            raise RuntimeError('PointCloud.orient: normals on %s, the cloud on %s' % (normals.device, self.points.device))
        self.point_normals = _f32(normals.detach())
        self._cones = None
        if cones:
            L = _C.lib()
            nbytes = int(L.tuch_point_cloud_cones_bytes(self.batch, self.resolution))
            buf = getattr(self, '_cone_buffer', None)
            if buf is None or buf.numel() != nbytes or buf.device != self.points.device:
                buf = self._cone_buffer = torch.zeros(nbytes, dtype=torch.uint8, device=self.points.device)
            with torch.cuda.device(self.points.device):
                _C.check(L.tuch_point_cloud_build_cones(_C.ptr(self._ws), self._nbytes, _C.ptr(self.point_normals), self.batch,
                                                        self.num_points, self.resolution, _C.ptr(buf), nbytes, _C.stream()))
            self._cones = buf
        return self

    def _cones_bytes(self) -> int:
        return 0 if self._cones is None else int(self._cones.numel())

    def _oriented_cos(self, what, max_angle) -> float:
        """The float32 cosine the oriented C entry points take (as _max_angle_cos); the cloud must be oriented."""
        if self.point_normals is None:
            raise ValueError('%s: max_angle needs an oriented cloud (PointCloud.orient; rebuild() drops the normals)' % what)
        return _max_angle_cos(self.point_normals, max_angle, self.points, what)

    def _check_queries(self, what, queries, shift, hint, name='queries'):
        if queries.dim() != 3 or queries.shape[0] != self.batch or queries.shape[2] != 3 or queries.shape[1] == 0:
            raise ValueError('%s: %s must be [%d,N,3] with N > 0, got %s' % (what, name, self.batch, tuple(queries.shape)))
        if shift is not None and tuple(shift.shape) != (self.batch, 3):
            raise ValueError('%s: shift / transl has shape %s, expected %s' % (what, tuple(shift.shape), (self.batch, 3)))
        _need_hip(what, queries, shift, hint)
        if queries.device != self.points.device:
            raise RuntimeError('%s: %s on %s, the cloud on %s' % (what, name, queries.device, self.points.device))
        if hint is not None and (tuple(hint.shape) != tuple(queries.shape[:2]) or hint.dtype != torch.int32
                                 or not hint.is_contiguous()):
            raise ValueError('%s: hint must be a contiguous int32 %s tensor' % (what, tuple(queries.shape[:2])))

    def nearest(self, queries, shift=None, counts=None, hint=None, max_distance=None, index_out=None, query_normals=None,
                max_angle=None) -> NearestPoint:
        """For every real query ``queries[b,n] + shift[b]`` the nearest valid point of body b's cloud:
        ``NearestPoint(d2 [B,N], index [B,N] int32)``; no winner: index -1, d2 +inf.  counts [B]: real queries per body;
        hint [B,N] int32: a guess per query that changes no bit of any result (it may be ``index_out``, the tensor the
        indices are written to); max_distance tau > 0: only points with d2 <= f32(tau)^2 can win.  d2 is differentiable
        w.r.t. queries and shift with the index held fixed.
        query_normals [B,N,3] with max_angle in degrees, in (0, 90], on an oriented cloud (``orient``): the nearest valid
        point whose normal is within the angle of the query's (tuch_point_cloud_nearest with normals; a query or a point
        whose normal is a zero or non-finite row is unconstrained; normals are not shifted and get no gradient).  Both
        or neither must be given; with neither the call is the plain one."""
        what = 'PointCloud.nearest'
        self._check_queries(what, queries, shift, hint)
        b, n = queries.shape[0], queries.shape[1]
        counts = _counts_of(what, counts, b)
        tau = _tau_of(what, max_distance)
        _need_hip(what, counts, index_out)
        cos = None
        if _both(what, 'query_normals', query_normals, 'max_angle', max_angle):
            if not torch.is_tensor(query_normals) or tuple(query_normals.shape) != (b, n, 3):
                raise ValueError('%s: query_normals must be [%d,%d,3], got %s'
                                 % (what, b, n, tuple(query_normals.shape) if torch.is_tensor(query_normals) else
                                    type(query_normals)))
            _need_hip(what, query_normals)
            query_normals, cos = _f32(query_normals.detach()), self._oriented_cos(what, max_angle)
        index = _index_out(what, index_out, b, n, queries.device)
        d2 = _CloudNearest.apply(queries, shift, self, counts, hint, tau, index, query_normals, cos)
        return NearestPoint(d2, index)

    def _knn_args(self, what, queries, k, shift, counts, max_distance):
        """The checks and conversions knn and normals share: (queries, shift, counts, tau) as the C ABI takes them."""
        _check_k(what, k)
        own = queries is None
        if own:
            queries = self.points
        self._check_queries(what, queries, shift, None)
        counts = _counts_of(what, counts, queries.shape[0])
        tau = _tau_of(what, max_distance)
        _need_hip(what, counts)
        qs = _f32(queries)
        if own:
            # the cloud's own points in the caller's order: an invalid point is no query (beyond counts: query_counts;
            # weight 0: made non-finite, which the rule answers with the no-winner outputs)
            if counts is None:
                counts = self.counts
            if self.weights is not None:
                qs = torch.where((self.weights != 0)[:, :, None], qs, torch.full_like(qs, float('nan')))
        return qs, None if shift is None else _f32(shift), counts, tau

    def knn(self, queries=None, k=8, shift=None, counts=None, max_distance=None) -> KNearest:
        """For every real query ``queries[b,n] + shift[b]`` the k (1 .. 32) nearest valid points of body b's cloud in
        ascending order of the packed key (d2, then index): ``KNearest(d2 [B,N,k], index [B,N,k] int32)``, the tail -1 /
        +inf where fewer than k points are admissible.  ``queries=None``: the cloud's own points in the caller's order
        (each valid point finds itself first, or its smallest-index duplicate; invalid points get -1 / +inf).  The bits
        are those of a sorted float32 brute-force sweep (tuch_point_cloud_knn).  No gradients."""
        qs, sh, counts, tau = self._knn_args('PointCloud.knn', queries, k, shift, counts, max_distance)
        b, n = qs.shape[0], qs.shape[1]
        d2 = torch.empty(b, n, k, dtype=torch.float32, device=qs.device)
        index = torch.empty(b, n, k, dtype=torch.int32, device=qs.device)
        with torch.cuda.device(qs.device):
            _C.check(_C.lib().tuch_point_cloud_knn(
                _C.ptr(self._ws), self._nbytes, _C.ptr(self.points), _C.ptr(self.counts), _C.ptr(self.weights), _C.ptr(qs),
                _C.ptr(sh), _C.ptr(counts), tau, b, self.num_points, n, k, _C.ptr(d2), _C.ptr(index), _C.stream()))
        return KNearest(d2, index)

    def normals(self, queries=None, k=16, viewpoint=None, shift=None, counts=None, max_distance=None,
                with_cov=False) -> PointNormals:
        """PCA normals over the k nearest valid points of every query (tuch_point_cloud_normals; the rule, the error bound
        and the zero rows are in include/tuch_amd.h): ``PointNormals(normal [B,N,3], variation [B,N], count [B,N] int32,
        cov [B,N,6] or None)``.  ``viewpoint`` [B,3] or [B,N,3], the sensor's position in the frame of the shifted
        queries, turns every normal towards it; without one the sign is canonical (the component of the largest
        magnitude is positive).  A zero row means "unknown" (fewer than 3 neighbours, collinear, coincident or isotropic
        ones) and is what scan_fit's ``normals`` treats as unconstrained.  ``queries=None``: the cloud's own points.
        No gradients."""
        what = 'PointCloud.normals'
        _check_k(what, k)
        n_of = self.num_points if queries is None else (queries.shape[1] if queries.dim() == 3 else -1)
        layout = 0
        if viewpoint is not None:
            if tuple(viewpoint.shape) == (self.batch, 3):
                layout = 1
            elif tuple(viewpoint.shape) == (self.batch, n_of, 3):
                layout = 2
            else:
                raise ValueError('%s: viewpoint must be [%d,3] or [%d,N,3], got %s'
                                 % (what, self.batch, self.batch, tuple(viewpoint.shape)))
        qs, sh, counts, tau = self._knn_args(what, queries, k, shift, counts, max_distance)
        _need_hip(what, viewpoint)
        view = None if viewpoint is None else _f32(viewpoint)
        b, n = qs.shape[0], qs.shape[1]
        normal = torch.empty(b, n, 3, dtype=torch.float32, device=qs.device)
        variation = torch.empty(b, n, dtype=torch.float32, device=qs.device)
        count = torch.empty(b, n, dtype=torch.int32, device=qs.device)
        cov = torch.empty(b, n, 6, dtype=torch.float32, device=qs.device) if with_cov else None
        with torch.cuda.device(qs.device):
            _C.check(_C.lib().tuch_point_cloud_normals(
                _C.ptr(self._ws), self._nbytes, _C.ptr(self.points), _C.ptr(self.counts), _C.ptr(self.weights), _C.ptr(qs),
                _C.ptr(sh), _C.ptr(counts), tau, b, self.num_points, n, k, _C.ptr(view), layout, _C.ptr(normal),
                _C.ptr(variation), _C.ptr(count), _C.ptr(cov), _C.stream()))
        return PointNormals(normal, variation, count, cov)

    def grid(self) -> CloudGrid:
        """The headers the build wrote, as host arrays (synchronises; for tests and tools)."""
        origin = np.empty((self.batch, 3), np.float32)
        cell = np.empty(self.batch, np.float32)
        dims = np.empty((self.batch, 3), np.int32)
        as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        with torch.cuda.device(self.points.device):
            _C.check(_C.lib().tuch_point_cloud_grid(_C.ptr(self._ws), self.batch, self.resolution, as_p(origin), as_p(cell),
                                                    as_p(dims)))
        return CloudGrid(origin, cell, dims)

    def canary_hits(self, reset: bool = True) -> int:
        """Guard words of this cloud's workspace (and of the term's scratch) found changed (set_cloud_canary)."""
        out = ctypes.c_int(0)
        with torch.cuda.device(self.points.device):
            _C.check(_C.lib().tuch_point_cloud_canary_hits(_C.ptr(self._ws), ctypes.byref(out), int(reset)))
        return out.value


def _tau_of(what, max_distance) -> float:
    if max_distance is None:
        return 0.0
    tau = float(max_distance)
    if not tau > 0.0:
        raise ValueError('%s: max_distance must be > 0 (or None), got %r' % (what, max_distance))
    return tau


def _index_out(what, index_out, b, n, device):
    if index_out is None:
        return torch.empty(b, n, dtype=torch.int32, device=device)
    if tuple(index_out.shape) != (b, n) or index_out.dtype != torch.int32 or not index_out.is_contiguous():
        raise ValueError('%s: index_out must be a contiguous int32 [%d,%d] tensor' % (what, b, n))
    return index_out


class _CloudFit(torch.autograd.Function):
    """ops.cloud_fit: the query, the term and the unit gradients in one launch (tuch_point_cloud_fit_terms).  `index`
    [B,V] int32 is written in place (it may be the hint tensor).  backward() only hands the gradients over, as
    _ScanFit's."""

    @staticmethod
    def forward(ctx, verts, transl, cloud, vw, layout, hint, rho, sigma, tau, scale, index, cos, table):
        v, tr = _f32(verts), _f32(transl)
        b, n, _ = v.shape
        dev = v.device
        L = _C.lib()
        d2 = torch.empty(b, n, dtype=torch.float32, device=dev)
        per_body = torch.empty(b, dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        gv = torch.empty_like(v)
        gt = torch.empty(b, 3, dtype=torch.float32, device=dev)
        nbytes = L.tuch_point_cloud_fit_scratch_bytes(b, n)
        scratch = _workspace(nbytes, dev)
        # (the cosine and the table select the form: an oriented cloud asked without them answers the plain term)
        normals = None if cos is None else cloud.point_normals
        faces, off, ids = table or (None, None, None)
        _C.check(L.tuch_point_cloud_fit_terms(
            _C.ptr(cloud._ws), cloud._nbytes, _C.ptr(cloud.points), _C.ptr(cloud.counts), _C.ptr(cloud.weights),
            _C.ptr(normals), cos or 0.0, _C.ptr(faces), _C.ptr(off), _C.ptr(ids), 0 if faces is None else int(faces.shape[0]),
            _C.ptr(cloud._cones), cloud._cones_bytes(), _C.ptr(v), _C.ptr(tr), _C.ptr(hint), tau, b, cloud.num_points, n,
            _C.ptr(vw), layout, rho, sigma, scale, _C.ptr(d2), _C.ptr(index), _C.ptr(_ticket(dev)), _C.ptr(per_body),
            _C.ptr(out), _C.ptr(gv), _C.ptr(gt), _C.ptr(scratch), nbytes, _C.stream()))
        ctx.save_for_backward(gv, gt)
        ctx.in_dtypes = (verts.dtype, transl.dtype)
        ctx.mark_non_differentiable(per_body, d2)
        ctx.set_materialize_grads(False)
        return out[0], per_body, d2

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_others):
        return _hand_over(ctx, g, 13)


def cloud_fit(cloud: PointCloud, verts, transl, vertex_weights=None, hint=None, rho='distance', sigma=None,
              max_distance=None, scale=1.0, index_out=None, max_angle=None, normal_table=None):
    """Model -> scan data term of a two-sided fit: ``(total, per_body, NearestPoint)``.  The queries are ``verts[b,v] +
    transl[b]`` against ``cloud``; the NearestPoint has the bits of ``cloud.nearest(verts, transl, hint=hint,
    max_distance=max_distance)`` (a vertex of weight 0 is not computed from: -1 / +inf).  per_body[b] = scale sum_v w_v
    rho(d2_v) / sum_v w_v with vertex_weights [V], [B,V] or None (ones) and rho / sigma as in ``scan_fit``; a vertex
    without winner contributes rho(tau^2) under max_distance tau when the body's cloud is not empty, else 0; total is
    their sum over the bodies, differentiable w.r.t. verts and transl with the nearest point held fixed (there is no
    gradient w.r.t. the cloud's points: they are data).  Every sum is fixed-order: the same bits on every call, in
    either mode of ``deterministic()``, for a body alone or in a batch.  hint / index_out as in ``PointCloud.nearest``.
    max_angle (degrees, in (0, 90]) with normal_table (``vertex_normal_table`` of the mesh the vertices belong to), on an
    oriented cloud: a vertex is matched only to points whose normal is within the angle of the vertex's own
    (tuch_point_cloud_fit_terms with normals, still one launch: the kernel forms the posed vertex normals itself).  The
    NearestPoint then has the bits of ``cloud.nearest(verts, transl, ..., query_normals=vertex_normals(verts,
    normal_table), max_angle=max_angle)``; a vertex without an admissible point is one without winner (index -1).
    Normals only decide the match: they get no gradient.  Both or neither must be given.
    There is no host fallback."""
    if not isinstance(cloud, PointCloud):
        raise ValueError('cloud_fit: cloud must be a PointCloud, got %r' % type(cloud).__name__)
    rho, sigma = _rho_of('cloud_fit', rho, sigma)
    if transl is None or tuple(transl.shape) != (cloud.batch, 3):
        raise ValueError('cloud_fit: transl must be [%d,3], got %s'
                         % (cloud.batch, None if transl is None else tuple(transl.shape)))
    cloud._check_queries('cloud_fit', verts, transl, hint, name='verts')
    b, n = verts.shape[0], verts.shape[1]
    layout, vw = 0, None
    if vertex_weights is not None:
        if tuple(vertex_weights.shape) == (n,):
            layout = 1
        elif tuple(vertex_weights.shape) == (b, n):
            layout = 2
        else:
            raise ValueError('cloud_fit: vertex_weights must be [%d] or [%d,%d], got %s' % (n, b, n, tuple(vertex_weights.shape)))
        _need_hip('cloud_fit', vertex_weights)
        vw = _f32(vertex_weights)
    tau = _tau_of('cloud_fit', max_distance)
    _need_hip('cloud_fit', index_out)
    index = _index_out('cloud_fit', index_out, b, n, verts.device)
    cos = None
    if _both('cloud_fit', 'max_angle', max_angle, 'normal_table', normal_table):
        _check_normal_table('cloud_fit', normal_table, n, verts.device)
        cos = cloud._oriented_cos('cloud_fit', max_angle)
    total, per_body, d2 = _CloudFit.apply(verts, transl, cloud, vw, layout, hint, rho, sigma, tau, float(scale), index, cos,
                                          normal_table)
    return total, per_body, NearestPoint(d2, index)


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


# ------------------------------------------------------------------- the regressor's input crops (csrc/image_crop.hip)
# tuch_crop_record of include/tuch_amd.h, field for field
CROP_RECORD = np.dtype([('offset', '<i8'), ('stride', '<i8'), ('ax', '<i8', (3,)), ('ay', '<i8', (3,)),
                        ('height', '<i4'), ('width', '<i4'), ('channels', '<i4'), ('type', '<i4'),
                        ('pw', '<i4'), ('ph', '<i4'), ('ox', '<i4'), ('oy', '<i4'), ('K', '<i4'), ('flip', '<i4'),
                        ('pn', '<f4', (3,)), ('reserved', '<i4')])
assert CROP_RECORD.itemsize == 120
# where an image lies in a packed buffer: byte offset of its first texel, bytes between rows, size, 0 = uint8 / 1 = float32
IMAGE_TABLE = np.dtype([('offset', '<i8'), ('stride', '<i8'), ('height', '<i4'), ('width', '<i4'), ('channels', '<i4'),
                        ('type', '<i4')])
CROP_MAX_RES = 1024
CROP_MAX_K = 16
CROP_FRAC_BITS = 32          # fractional bits of the integer affine; positions are its values >> 16 (units of 2^-16 px)
_CROP_LIMIT = 1 << 29


def pack_images(images, device=None, row_align: int = 4):
    """A list of HWC (or HW) arrays, uint8 or float32 (anything else is converted to float32), of any sizes -> (buffer,
    table): one uint8 device tensor holding all of them and the IMAGE_TABLE array saying where.  Rows are padded to
    ``row_align`` bytes and images start on 16-byte boundaries; the bytes are assembled in ONE pinned host buffer and go to
    the device in one asynchronous copy."""
    if row_align < 1:
        raise ValueError('row_align must be positive')
    device = torch.device('cuda' if device is None else device)
    table = np.zeros(len(images), IMAGE_TABLE)
    arrays, at = [], 0
    for n, img in enumerate(images):
        a = np.asarray(img.detach().cpu() if torch.is_tensor(img) else img)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError('image %d: expected [H, W], [H, W, 1] or [H, W, 3], got shape %s' % (n, a.shape))
        if a.dtype != np.uint8:
            a = a.astype(np.float32)
        es = a.dtype.itemsize
        row = a.shape[1] * a.shape[2] * es
        align = max(int(row_align), es)
        stride = (row + align - 1) // align * align
        if es == 4 and stride % 4:
            stride = (stride + 3) // 4 * 4
        at = (at + 15) // 16 * 16
        table[n] = (at, stride, a.shape[0], a.shape[1], a.shape[2], 1 if es == 4 else 0)
        arrays.append(a)
        at += stride * a.shape[0]
    host = torch.zeros(max(at, 1), dtype=torch.uint8)
    if device.type == 'cuda':
        host = host.pin_memory()
    flat = host.numpy()
    for a, t in zip(arrays, table):
        rows = flat[t['offset']:t['offset'] + t['stride'] * t['height']].reshape(t['height'], t['stride'])
        rows[:, :a.shape[1] * a.shape[2] * a.dtype.itemsize] = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
    return host.to(device, non_blocking=True), table


def crop_box(center, scale, rot, res):
    """The reference's integer box (imutils.py:73-85): (ul [2], br [2], pad) with the pad already 0 at rot == 0."""
    from .utils import imutils
    ul = np.array(imutils.transform([1, 1], center, scale, [res, res], invert=1)) - 1
    br = np.array(imutils.transform([res + 1, res + 1], center, scale, [res, res], invert=1)) - 1
    pad = int(np.linalg.norm(br - ul) / 2 - float(br[1] - ul[1]) / 2)
    return ul, br, (pad if not rot == 0 else 0)


def crop_records(table, center, scale, rot, flip, pn, res) -> np.ndarray:
    """The per-sample records of tuch_crop_batch, built in float64 on the host: table [B] (IMAGE_TABLE, sample b crops
    image table[b]), center [B,2], scale [B], rot [B] in degrees, flip [B], pn [B,3] or None (ones), res = R.
    The box is the reference's integer box; the integer affine carries CROP_FRAC_BITS fractional bits (see
    include/tuch_amd.h).  A box without area raises ValueError, as the reference's array of negative size does."""
    res = int(res)
    if not 1 <= res <= CROP_MAX_RES:
        raise ValueError('res must be in [1, %d]' % CROP_MAX_RES)
    table = np.atleast_1d(np.asarray(table, IMAGE_TABLE))
    b = table.shape[0]
    center = np.asarray(center, np.float64).reshape(b, 2)
    scale = np.asarray(scale, np.float64).reshape(b)
    rot = np.asarray(rot, np.float64).reshape(b)
    flip = np.asarray(flip).reshape(b)
    pn = np.ones((b, 3), np.float64) if pn is None else np.asarray(pn, np.float64).reshape(b, 3)
    rec = np.zeros(b, CROP_RECORD)
    for k in ('offset', 'stride', 'height', 'width', 'channels', 'type'):
        rec[k] = table[k]
    one = float(1 << CROP_FRAC_BITS)
    for n in range(b):
        ul, br, p = crop_box(center[n], scale[n], rot[n], res)
        bw, bh = int(br[0] - ul[0]), int(br[1] - ul[1])
        if bw <= 0 or bh <= 0:
            raise ValueError('sample %d: the box has no area (%d x %d)' % (n, bw, bh))
        pw, ph = bw + 2 * p, bh + 2 * p
        ox, oy = int(ul[0]) - p, int(ul[1]) - p
        if max(pw, ph, abs(ox), abs(oy)) > _CROP_LIMIT:
            raise ValueError('sample %d: the box is out of range' % n)
        k = min(max(-(-max(bw, bh) // res), 1), CROP_MAX_K)
        if rot[n] == 0:
            cs, sn = 1.0, 0.0
        else:
            cs, sn = np.cos(np.deg2rad(rot[n])), np.sin(np.deg2rad(rot[n]))
        cx, cy = pw / 2.0, ph / 2.0
        sx, sy = bw / (2.0 * k * res), bh / (2.0 * k * res)           # box units per grid step
        ax = (cs * sx, -sn * sy, cs * (p - cx) - sn * (p - cy) + cx - 0.5)
        ay = (sn * sx, cs * sy, sn * (p - cx) + cs * (p - cy) + cy - 0.5)
        half = 1 << (CROP_FRAC_BITS - 16 - 1)                        # round to the nearest 2^-16 px
        rec['ax'][n] = [int(np.rint(ax[0] * one)), int(np.rint(ax[1] * one)), int(np.rint(ax[2] * one)) + half]
        rec['ay'][n] = [int(np.rint(ay[0] * one)), int(np.rint(ay[1] * one)), int(np.rint(ay[2] * one)) + half]
        rec['pw'][n], rec['ph'][n], rec['ox'][n], rec['oy'][n] = pw, ph, ox, oy
        rec['K'][n], rec['flip'][n] = k, 1 if flip[n] else 0
        rec['pn'][n] = pn[n]
    return rec


def check_crop_records(records: np.ndarray, buffer_bytes: int, channels: int) -> None:
    """Every image of every record lies inside the packed buffer and every field is in range, or ValueError: what the
    kernel may address is decided here, on the host, before anything is launched."""
    r = records
    if r.dtype != CROP_RECORD or r.ndim != 1:
        raise ValueError('records must be a 1-D CROP_RECORD array (crop_records)')
    es = np.where(r['type'] == 1, 4, 1).astype(np.int64)
    row = r['width'].astype(np.int64) * r['channels'] * es
    end = r['offset'] + (r['height'].astype(np.int64) - 1) * r['stride'] + row
    bad = ~np.isin(r['type'], (0, 1)) | ~np.isin(r['channels'], (1, 3)) | ((r['channels'] == 3) & (channels != 3))
    bad |= (r['K'] < 1) | (r['K'] > CROP_MAX_K) | (r['height'] < 1) | (r['width'] < 1) | (r['pw'] < 1) | (r['ph'] < 1)
    bad |= (r['pw'] > _CROP_LIMIT) | (r['ph'] > _CROP_LIMIT) | (np.abs(r['ox']) > _CROP_LIMIT) | (np.abs(r['oy']) > _CROP_LIMIT)
    bad |= (r['offset'] < 0) | (r['stride'] < row) | (r['stride'] > (1 << 40)) | (r['offset'] > (1 << 60))
    bad |= (r['type'] == 1) & (((r['offset'] | r['stride']) & 3) != 0)
    bad |= (end < 0) | (end > int(buffer_bytes))
    if bad.any():
        n = int(np.argmax(bad))
        raise ValueError('crop record %d is out of range or addresses outside the packed buffer of %d bytes: %r'
                         % (n, buffer_bytes, r[n]))


class DeviceCropRecords:
    """Records that were checked against a buffer and uploaded (upload_crop_records): crop_batch launches on them without
    touching the host -- what a captured graph needs."""

    def __init__(self, tensor, count, buffer_bytes, channels_checked):
        self.tensor, self.count, self.buffer_bytes, self.channels_checked = tensor, count, buffer_bytes, channels_checked


def upload_crop_records(buffer: torch.Tensor, records: np.ndarray, channels: int = 3) -> DeviceCropRecords:
    check_crop_records(records, buffer.numel() * buffer.element_size(), channels)
    host = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1).copy())
    if buffer.is_cuda:
        host = host.pin_memory()
    return DeviceCropRecords(host.to(buffer.device, non_blocking=True), int(records.shape[0]),
                             buffer.numel() * buffer.element_size(), int(channels))


def crop_batch(buffer: torch.Tensor, records, res: int, mean, std, raw: bool = False):
    """tuch_crop_batch (include/tuch_amd.h): buffer = pack_images' device tensor, records = crop_records' array (checked
    against the buffer and uploaded here) or upload_crop_records' object, mean / std = one float per output channel (1 or
    3) -> out [B,C,R,R] float32 = (raw - mean) / std, and with raw=True also raw [B,C,R,R] in [0,1].  One launch on the
    current stream; with uploaded records nothing else: capturable."""
    mean = [float(x) for x in np.asarray(mean, np.float64).reshape(-1)]
    std = [float(x) for x in np.asarray(std, np.float64).reshape(-1)]
    ch = len(mean)
    if ch not in (1, 3) or len(std) != ch:
        raise ValueError('mean and std need 1 or 3 entries each')
    if not buffer.is_cuda or buffer.dtype != torch.uint8 or buffer.dim() != 1:
        raise _C.TuchError('crop_batch needs the 1-D uint8 device buffer of pack_images')
    res = int(res)
    if not 1 <= res <= CROP_MAX_RES:
        raise ValueError('res must be in [1, %d]' % CROP_MAX_RES)
    with torch.cuda.device(buffer.device):
        if not isinstance(records, DeviceCropRecords):
            records = upload_crop_records(buffer, records, ch)
        if records.buffer_bytes != buffer.numel() or (records.channels_checked != ch and ch != 3):
            raise ValueError('these records were checked against another buffer or channel count')
        b = records.count
        out = torch.empty(b, ch, res, res, dtype=torch.float32, device=buffer.device)
        raw_out = torch.empty_like(out) if raw else None
        fl = ctypes.c_float * ch
        _C.check(_C.lib().tuch_crop_batch(_C.ptr(buffer), buffer.numel(), _C.ptr(records.tensor) if b else _C.ptr(None), b, res,
                                          ch, fl(*mean), fl(*std), _C.ptr(out), _C.ptr(raw_out), _C.stream()))
    return (out, raw_out) if raw else out
