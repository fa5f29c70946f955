"""Mesh renderer on the device: face ids, depth and shaded views of a batch of bodies (csrc/render.hip).

An Instinct accelerator has no graphics pipeline, and the reference's pictures all go through pyrender / OpenGL
(tuch/utils/renderer.py).  This is a compute rasteriser over what SMPLifyDC, SMPL.forward and SelfContact already
return on the device:

    r = MeshRenderer(faces, img_res=224, focal_length=5000.)
    out = r.render(verts, camera_translation, views=('front', 'rot2', 'rot3'))      # no host synchronisation
    out['face']    [B,n,H,W]    int32     triangle id at the pixel centre, -1 = empty
    out['depth']   [B,n,H,W]    float32   camera-space z in metres, 0 = empty (the reference's `rend_depth > 0`)
    out['image']   [B,n,H,W,3]  float32   in [0,1]
    cols = r.contact_colors(verts, partner=SelfContact(...)(verts)['partner'])      # [B,V,3] uint8
    out = r.render(verts, camera_translation, colors=cols)

Geometry and visibility are exact (integer coverage with a top-left rule, nearest surface, smaller face id at equal
depth; bit-identical from run to run and in any batch) and the vertex colours are the reference's.  The LOOK is not
pyrender's: its physically based shading is not emulated and cannot be compared against here; a pixel is
``albedo / 255 * min(1, 0.3 + 0.7 * max(0, -n_z))`` -- the reference's ambient term 0.3 (renderer.py:229) and its four
directional lights, which all have identity orientation (renderer.py:250-256 sets only their positions) and so shine
along the viewing direction.

The camera is utils/geometry.perspective_projection: p = R_view v + t lands at (f p.x / p.z + cx, f p.y / p.z + cy), the
pixel in row r, column c has its centre at (c + 0.5, r + 0.5).

The views.  The reference turns the mesh by 180 degrees about x, then optionally by 60 degrees about y (``dorot2``) or
about x (``dorot3``), in pyrender's frame (camera at t' = (-t.x, t.y, t.z) after its ``camera_translation[0] *= -1``,
looking down -z, y up): q = M C v - t' with C = R_x(180) = diag(1, -1, -1) and M = I, R_y(60) or R_x(60); pyrender
projects q to (f q.x / -q.z + cx, cy - f q.y / -q.z).  In the perspective_projection frame p = C q = (C M C) v - C t',
and -C t' = t.  C M C is I for M = I, and conjugating with a half turn about x reverses rotations about y and keeps those
about x:

    front = I             the picture coincides with perspective_projection(verts, I, t, f, c)
    rot2  = R_y(-60 deg)
    rot3  = R_x(+60 deg)

each applied about the origin before t is added.  tests/test_render_host.py composes the reference's 4x4 matrices.

Constructing needs no device; calling does.  There is no host fallback.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _C, ops


def _rot_x(deg: float) -> np.ndarray:
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def _rot_y(deg: float) -> np.ndarray:
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


VIEWS = {'front': np.eye(3), 'rot2': _rot_y(-60.0), 'rot3': _rot_x(60.0)}


def view_matrix(view) -> np.ndarray:
    """A view name of VIEWS or a 3x3 rotation -> [3,3] float64."""
    if isinstance(view, str):
        if view not in VIEWS:
            raise ValueError('unknown view %r (one of %s, or a 3x3 matrix)' % (view, ', '.join(sorted(VIEWS))))
        return VIEWS[view]
    m = np.asarray(view.detach().cpu() if torch.is_tensor(view) else view, np.float64)
    if m.shape != (3, 3):
        raise ValueError('a view is a name or a [3, 3] matrix, got shape %s' % (m.shape,))
    return m


def image_grid(tiles: torch.Tensor, nrow: int, padding: int = 2, pad_value: float = 0.0) -> torch.Tensor:
    """[N,C,H,W] -> the [C, rows (H + p) + p, cols (W + p) + p] grid torchvision.utils.make_grid gives for a list of N > 1
    images: ``cols = min(nrow, N)`` images per row, tile k at (r (H + p) + p, c (W + p) + p) with r, c = divmod(k, cols),
    everything else ``pad_value``."""
    if tiles.dim() != 4:
        raise ValueError('tiles must be [N, C, H, W]')
    n, ch, h, w = tiles.shape
    if n == 0 or nrow < 1:
        raise ValueError('image_grid needs at least one tile and nrow >= 1')
    cols = min(int(nrow), n)
    rows = (n + cols - 1) // cols
    grid = tiles.new_full((ch, rows * (h + padding) + padding, cols * (w + padding) + padding), pad_value)
    for k in range(n):
        r, c = divmod(k, cols)
        y, x = r * (h + padding) + padding, c * (w + padding) + padding
        grid[:, y:y + h, x:x + w] = tiles[k]
    return grid


class MeshRenderer:
    """faces         [F,3] triangle list (numpy or tensor), rendered as it is: no back-face culling;
    img_res       224 or (H, W);
    focal_length  in pixels;
    camera_center (cx, cy); default (W // 2, H // 2), the reference's ``img_res // 2`` (renderer.py:48).
    Device tables (faces, the vertex -> faces lists, view matrices) are made on first use and kept."""

    def __init__(self, faces, img_res=224, focal_length: float = 5000., camera_center=None):
        f = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0:
            raise ValueError('faces must be [F, 3] with F >= 1, got %s' % (f.shape,))
        if f.min() < 0:
            raise ValueError('faces has a negative vertex id')
        self.faces = np.ascontiguousarray(f.astype(np.int64))
        if isinstance(img_res, (tuple, list)):
            if len(img_res) != 2:
                raise ValueError('img_res must be an integer or (H, W)')
            self.height, self.width = int(img_res[0]), int(img_res[1])
        else:
            self.height = self.width = int(img_res)
        if self.height < 1 or self.width < 1:
            raise ValueError('img_res must be positive, got %r' % (img_res,))
        self.focal_length = float(focal_length)
        if not self.focal_length > 0:
            raise ValueError('focal_length must be positive, got %r' % (focal_length,))
        if camera_center is None:
            camera_center = (self.width // 2, self.height // 2)
        self.camera_center = (float(camera_center[0]), float(camera_center[1]))
        self._tables = {}
        self._views = {}
        self._regions = {}

    # ------------------------------------------------------------------------------------------- device tables
    def _check_verts(self, verts):
        if not torch.is_tensor(verts) or verts.dim() != 3 or verts.shape[2] != 3:
            raise ValueError('verts must be a [B, V, 3] tensor')
        if int(self.faces.max()) >= verts.shape[1]:
            raise ValueError('faces name vertex %d, verts has %d' % (int(self.faces.max()), verts.shape[1]))
        if verts.device.type != 'cuda':
            raise _C.TuchError('tuch_amd kernels need tensors on a HIP device, got %s' % verts.device)

    def _mesh_tables(self, num_verts, device):
        key = (int(num_verts), device)
        hit = self._tables.get(key)
        if hit is None:
            off, ids = ops.vertex_face_table(self.faces, num_verts)
            hit = self._tables[key] = (torch.as_tensor(self.faces.astype(np.int32), device=device),
                                       (torch.as_tensor(off, device=device), torch.as_tensor(ids, device=device)))
        return hit

    def _view_table(self, views, device):
        mats = np.stack([view_matrix(v) for v in views]).astype(np.float32)
        key = (mats.tobytes(), device)
        hit = self._views.get(key)
        if hit is None:
            hit = self._views[key] = torch.as_tensor(mats, device=device)
        return hit

    # ------------------------------------------------------------------------------------------- rendering
    def render(self, verts, camera_translation, views: Sequence = ('front',), colors=None, background=None,
               background_views: Optional[Sequence[bool]] = None) -> dict:
        """verts [B,V,3] and camera_translation [B,3] on the device; views: names of VIEWS or 3x3 rotations (at most 32);
        colors [B,V,3] uint8 (contact_colors) or None for the reference's 230; background [B,H,W,3] in [0,1] or None.
        Empty pixels take the background in the views flagged in background_views -- by default the views that are the
        identity, as the reference composites its front view over the photograph and its turned views over white
        (renderer.py:264-270) -- and 1.0 elsewhere.  Returns {'face', 'depth', 'image'} (module docstring)."""
        self._check_verts(verts)
        views = list(views)
        if not 1 <= len(views) <= ops.MAX_RENDER_VIEWS:
            raise ValueError('%d views, 1 to %d are supported' % (len(views), ops.MAX_RENDER_VIEWS))
        if not torch.is_tensor(camera_translation) or camera_translation.shape != (verts.shape[0], 3):
            raise ValueError('camera_translation must be a [B, 3] tensor')
        mats = [view_matrix(v) for v in views]
        if background_views is None:
            background_views = [bool(np.array_equal(m, np.eye(3))) for m in mats]
        background_views = list(background_views)
        if len(background_views) != len(views):
            raise ValueError('background_views needs one flag per view')
        bits = sum(1 << k for k, on in enumerate(background_views) if on)
        dev = verts.device
        with torch.cuda.device(dev):
            faces, vface = self._mesh_tables(verts.shape[1], dev)
            rot = self._view_table(mats, dev)
            return ops.render_mesh(verts, faces, vface, camera_translation, rot, self.focal_length, self.camera_center[0],
                                   self.camera_center[1], self.height, self.width, colors, background, bits)

    # ------------------------------------------------------------------------------------------- contact colours
    def _region_tables(self, contactlist, num_verts, device):
        key = (id(contactlist), int(num_verts), device)
        hit = self._regions.get(key)
        if hit is None:
            names = list(contactlist['csig'].keys())
            index = {n: k for k, n in enumerate(names)}
            lists = [np.asarray(contactlist['csig'][n], np.int64).reshape(-1) for n in names]
            first = np.array([int(r[0]) if r.size else -1 for r in lists], np.int32)
            pairs = np.array([[index[a], index[b]] for a, b in contactlist['classes']], np.int32).reshape(-1, 2)
            off, ids = ops.vertex_region_table(lists, num_verts)
            hit = self._regions[key] = tuple(torch.as_tensor(a, device=device) for a in (pairs, first, off, ids)) + (contactlist,)
        return hit[:4]

    def contact_colors(self, verts, pairs=None, partner=None, contact=None, contactlist=None) -> torch.Tensor:
        """The reference's vertex colours (renderer.py:199-224) for a batch: [B,V,3] uint8 on the device.  Exactly one of

        pairs=    per body the two vertex lists of ``colverts`` -- a dict {b: [idxs1, idxs2]} as
                  SelfContact.verts_in_contact / get_verts_in_contact return it (a missing body or None: no pairs), or a
                  sequence of B such entries: both vertices of a pair get the mean of their position colours, pairs in
                  list order, the last write wins.  As in the reference, a body whose list is not shorter than V is left
                  uncoloured.  The lists are uploaded (they may live on the host).
        partner=  SelfContact's [B,V] int32 output directly: the pairs (i, partner[i]) of the in-contact i in increasing
                  order, exactly what verts_in_contact lists.  No host synchronisation.
        contact=  [B,P] 0/1 with contactlist={'classes': P pairs of region names, 'csig': {name: vertex ids}}: all vertices
                  of both regions of every active pair get the position colour of the first region's first listed vertex,
                  pairs in increasing order, the last wins.
        Untouched vertices keep 230."""
        if sum(x is not None for x in (pairs, partner, contact)) != 1:
            raise ValueError('give exactly one of pairs=, partner= and contact=')
        self._check_verts(verts)
        b, v, _ = verts.shape
        dev = verts.device
        with torch.cuda.device(dev):
            if partner is not None:
                if not torch.is_tensor(partner) or partner.shape != (b, v):
                    raise ValueError('partner must be a [B, V] tensor')
                # every vertex is a pair of its own; those without a partner (-1) are ignored by the kernel
                off = torch.arange(0, (b + 1) * v, v, dtype=torch.int32, device=dev)
                c1 = torch.arange(v, dtype=torch.int32, device=dev).repeat(b)
                c2 = partner.to(torch.int32).reshape(-1).contiguous()
                return ops.contact_vertex_colors(verts, pairs=(off, c1, c2))
            if pairs is not None:
                entries = [pairs.get(k) for k in range(b)] if isinstance(pairs, dict) else list(pairs)
                if len(entries) != b:
                    raise ValueError('pairs needs one entry per body')
                l1, l2 = [], []
                for e in entries:
                    a, c = (np.zeros(0, np.int64),) * 2 if e is None else [
                        np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, np.int64).reshape(-1) for x in e]
                    if len(a) != len(c):
                        raise ValueError('the two vertex lists of a body differ in length')
                    if len(a) >= v:                               # renderer.py:210
                        a, c = a[:0], c[:0]
                    l1.append(a)
                    l2.append(c)
                off = np.zeros(b + 1, np.int64)
                np.cumsum([len(a) for a in l1], out=off[1:])
                up = [torch.as_tensor(x.astype(np.int32), device=dev) for x in (off, np.concatenate(l1), np.concatenate(l2))]
                return ops.contact_vertex_colors(verts, pairs=tuple(up))
            if contactlist is None:
                raise ValueError("contact= needs contactlist={'classes': ..., 'csig': ...}")
            rp, first, voff, vreg = self._region_tables(contactlist, v, dev)
            contact = torch.as_tensor(contact, device=dev)
            if contact.shape != (b, rp.shape[0]):
                raise ValueError('contact must be [B, %d], got %s' % (rp.shape[0], tuple(contact.shape)))
            return ops.contact_vertex_colors(verts, regions=((contact == 1).to(torch.uint8), rp, first, voff, vreg))
