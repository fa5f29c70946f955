"""Posed vertex normals (csrc/vertex_normals.hip) and the mesh renderer with the contact colouring (csrc/render.hip),
with the host tables both read a mesh by (tuch_amd/render.py is the caller-facing renderer)."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _C
from ._base import _f32, _need_hip, _workspace


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
