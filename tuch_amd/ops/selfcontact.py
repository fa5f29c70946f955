"""Self-contact detection on the kernels of csrc/self_contact.hip, and the host table of the regions it reports by
(contact_detect.py is the caller-facing form)."""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from .. import _C
from ._base import _f32


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
