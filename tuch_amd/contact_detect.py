"""Self-contact detection on the device: which vertices of a body touch, and which body regions do they join.

Vertices i, j are in contact when ``|v_i - v_j| < euclthres`` and ``geodesic(i, j) >= geothres`` -- the paper's
definition and ``TUCH.get_verts_in_contact``'s (tuch/train/train_module.py:93-110, which builds the [V,V] distance
matrix per body in a Python loop).  Here one kernel pass (csrc/self_contact.hip) gives, for a whole batch,

    det = SelfContact(geodists, geothres=0.3, euclthres=0.02, regions=csig)
    out = det(verts)                       # verts [B,V,3] on the device; no host synchronisation
    out['in_contact']   [B,V]   bool       vertex has a contact partner
    out['partner']      [B,V]   int32      the nearest one (smallest index among equals), -1 without contact
    out['dist']         [B,V]   float32    metres to it, inf without contact
    out['cnc']          [B]     float32    the body's smallest contact distance, inf = no contact: what
                                           eval.pose_summary(cnc=...) / Evaluator(contact=det) split the errors by
    out['signature']    [B,R,R] float32    smallest contact distance between vertices of region r1 and of region r2
                                           (inf = the regions do not touch); only with ``regions``

    det.verts_in_contact(verts)            # {bidx: [idxs1, idxs2]} as the reference function (synchronises, as it does)

The defaults are configs/config.py:90-91.  There is no host fallback: calls need a HIP device; constructing does not.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _C, ops


class SelfContact:
    """geodists  [V,V] geodesic distances (numpy or tensor); the mask is ``geodists >= geothres`` -- the reference
                 function's ``>=`` (train_module.py:96); the loss masks use ``>`` and are built elsewhere.
    geomask=     instead of geodists: an explicit [V,V] bool mask (entry [i][j] admits j as a contact partner of i), or
                 an ``ops.ContactModel`` created with a mask, whose packed device copy is reused.
    regions      a ``csig``-style dict {name: vertex ids} or an ordered list of vertex-id lists (at most 128; they may
                 overlap or be empty); ``region_names`` keeps the order of the signature's axes.
    Device tables (the packed mask, the vertex -> regions lists) are made on first use."""

    def __init__(self, geodists=None, geothres: float = 0.3, euclthres: float = 0.02, regions=None, *, geomask=None,
                 device: Optional[torch.device] = None):
        if (geodists is None) == (geomask is None):
            raise ValueError('give exactly one of geodists and geomask=')
        self.geothres, self.euclthres = float(geothres), float(euclthres)
        self.device = torch.device(device) if device is not None else None
        self._model = self._mask = None
        if isinstance(geomask, ops.ContactModel):
            if not geomask.has_mask:
                raise ValueError('the ContactModel was created without a geodesic mask')
            self._model = geomask
            self.num_verts = geomask.num_verts
        else:
            if geodists is not None:
                g = geodists.detach() if torch.is_tensor(geodists) else torch.as_tensor(np.asarray(geodists))
                mask = g >= self.geothres
            else:
                mask = geomask.detach() if torch.is_tensor(geomask) else torch.as_tensor(np.asarray(geomask))
                mask = mask.to(torch.bool)
            if mask.dim() != 2 or mask.shape[0] != mask.shape[1] or mask.shape[0] == 0:
                raise ValueError('the mask must be [V, V], got %s' % (tuple(mask.shape),))
            self._mask = mask
            self.num_verts = int(mask.shape[0])
        self.region_names = None
        self.num_regions = 0
        self._vreg_host = None
        if regions is not None:
            if isinstance(regions, dict):
                self.region_names = list(regions.keys())
                regions = [regions[n] for n in self.region_names]
            else:
                regions = list(regions)
                self.region_names = list(range(len(regions)))
            if not regions:
                raise ValueError('regions is empty (pass None for no signature)')
            self._vreg_host = ops.vertex_region_table(regions, self.num_verts)
            self.num_regions = len(regions)
        self._tables = {}

    def _device_tables(self, device):
        """(packed mask: tensor or the model's pointer, (off, ids) or None) on `device`."""
        hit = self._tables.get(device)
        if hit is None:
            if device.type != 'cuda':
                raise _C.TuchError('tuch_amd kernels need tensors on a HIP device, got %s' % device)
            with torch.cuda.device(device):
                if self._model is not None:
                    if self._model.device.index not in (None, device.index):
                        raise ValueError('vertices on %s, the ContactModel on %s' % (device, self._model.device))
                    bits = _C.lib().tuch_contact_model_mask_bits(self._model._handle)
                elif self._mask is not None:
                    bits = ops.pack_geomask(self._mask.to(device))
                    self._mask = None                      # the [V,V] matrix is not needed again
                else:                                      # a second device: the packed words of the first
                    bits = next(iter(self._tables.values()))[0].to(device)
                vreg = None
                if self._vreg_host is not None:
                    vreg = tuple(torch.as_tensor(a, device=device) for a in self._vreg_host)
            hit = self._tables[device] = (bits, vreg)
        return hit

    def _squared(self, verts):
        if not torch.is_tensor(verts) or verts.dim() != 3 or verts.shape[1:] != (self.num_verts, 3):
            raise ValueError('verts must be a [B, %d, 3] tensor' % self.num_verts)
        if self.device is not None and (verts.device.type != self.device.type or
                                        self.device.index not in (None, verts.device.index)):
            raise ValueError('vertices on %s, the detector on %s' % (verts.device, self.device))
        bits, vreg = self._device_tables(verts.device)
        with torch.cuda.device(verts.device):
            return ops.self_contact(verts, bits, self.euclthres, vreg, self.num_regions)

    def cnc(self, verts) -> torch.Tensor:
        """[B]: the bodies' smallest contact distance in metres (inf = no contact); ``self(verts)['cnc']``."""
        return torch.sqrt(self._squared(verts)['cnc_d2'])

    def __call__(self, verts) -> dict:
        r = self._squared(verts)
        out = {'in_contact': r['in_contact'], 'partner': r['partner'], 'dist': torch.sqrt(r['min_d2']),
               'cnc': torch.sqrt(r['cnc_d2'])}
        if 'sig_d2' in r:
            out['signature'] = torch.sqrt(r['sig_d2'])
        return out

    def verts_in_contact(self, verts) -> dict:
        """{bidx: [idxs1, idxs2]}: the vertices in contact and their nearest contact partners, int64 tensors on the
        vertices' device -- what the reference's get_verts_in_contact returns (train_module.py:93-110)."""
        r = self._squared(verts)
        flags, partner = r['in_contact'], r['partner'].to(torch.int64)
        return {b: [torch.where(flags[b])[0], partner[b][flags[b]]] for b in range(verts.shape[0])}
