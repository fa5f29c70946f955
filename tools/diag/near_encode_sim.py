"""Host emulation behind the 16-bit fixed-point records of the near test (ray_winding.hip: ray_leaf_bounds_kernel,
ray_near_kernel): how many (ray, leaf) pairs does the 13-slab test list when the leaves' bounds and the rays' values
are rounded outwards to
    half / single : half-precision records against single-precision ray values (the encoding up to round 7),
    fixed 2^-13   : signed 16-bit levels of 2^-13 m (+-4 m) on BOTH sides, bounds and rays rounded apart,
    fixed 2^-12   : the same with 2^-12 m (+-8 m)?
`exact` is the single-precision test without any encoding (the floor of all three).  The bench's bodies: make_body(84,
82, seed=1234), random_poses at batch 8.      python tools/diag/near_encode_sim.py [bodies] [seed]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from synthetic import make_body, random_poses
from tuch_amd import ops
from oracle import lbs as olbs

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 8
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1002
body = make_body(84, 82, seed=1234)
m = olbs.model_tensors(body)
bp, go, be = random_poses(nb, seed)
v, _ = olbs.smpl_forward(m, torch.tensor(be), torch.tensor(bp), torch.tensor(go))
verts = v.numpy().astype(np.float32)
faces = body.faces.astype(np.int64)
F = faces.shape[0]
tree = ops.cluster_tree(faces, body.num_verts, max(32, F // 850))
nodes = tree['nodes']
leaves = [n for n in range(nodes.shape[0]) if nodes[n, 5] < 0]
KX, KY = np.float32(0.3217), np.float32(0.4331)
f32 = np.float32


def project(x, y, z):          # slab_project, single precision
    return np.stack([x, y, z, x + y, x - y, x + z, x - z, y + z, y - z]).astype(f32)


def half_below(x):
    h = x.astype(np.float16)
    hf = h.astype(f32)
    return np.where(hf > x, np.nextafter(h, np.float16(-np.inf)), h).astype(f32)


def half_above(x):
    h = x.astype(np.float16)
    hf = h.astype(f32)
    return np.where(hf < x, np.nextafter(h, np.float16(np.inf)), h).astype(f32)


def fixed(x, scale, up):
    t = x.astype(np.float64) * scale
    return np.clip(np.ceil(t) if up else np.floor(t), -32768, 32767)


LO = [0, 1, 3, 4, 6, 8]          # slabs whose LOWER bound the test uses
HI = [0, 1, 2, 3, 4, 5, 7]       # ... whose UPPER bound
counts = dict(exact=0, half=0, fx13=0, fx12=0)
beyond = dict(fx13=0, fx12=0)
for b in range(nb):
    x = (verts[b, :, 0].astype(np.float64) - np.float64(KX) * verts[b, :, 2]).astype(f32)      # fma: one rounding
    y = (verts[b, :, 1].astype(np.float64) - np.float64(KY) * verts[b, :, 2]).astype(f32)
    z = verts[b, :, 2]
    pr = project(x, y, z)                                   # [9][V]
    lo_p = np.empty((9, len(leaves)), f32); hi_p = np.empty((9, len(leaves)), f32)
    for i, n in enumerate(leaves):
        vs = tree['vidx'][nodes[n, 2]:nodes[n, 2] + nodes[n, 3]]
        lo = pr[:, vs].min(1); hi = pr[:, vs].max(1)
        pad = (f32(4e-7) * np.maximum(np.abs(lo), np.abs(hi)) + f32(1e-9)).astype(f32)
        lo_p[:, i] = lo - pad; hi_p[:, i] = hi + pad
    v0 = tree['vidx'][0]
    pc = project(x[v0:v0 + 1], y[v0:v0 + 1], z[v0:v0 + 1])  # [9][1]
    pad = (f32(4e-6) * (np.abs(lo_p) + np.abs(hi_p) + np.abs(pc)) + f32(1e-7)).astype(f32)
    lo_r = (lo_p - pc - pad).astype(f32); hi_r = (hi_p - pc + pad).astype(f32)
    # queries: every vertex once (the order of the blocks does not matter for a count)
    rx, ry, rz = x - pc[0], y - pc[1], z - pc[2]
    r = project(rx, ry, rz)                                 # [9][V], formed as the kernel forms them
    enc = {
        'exact': (lo_r, hi_r, r, r),
        'half': (half_below(lo_r), half_above(hi_r), r, r),
        'fx13': (fixed(lo_r, 8192.0, False), fixed(hi_r, 8192.0, True), fixed(r, 8192.0, True), fixed(r, 8192.0, False)),
        'fx12': (fixed(lo_r, 4096.0, False), fixed(hi_r, 4096.0, True), fixed(r, 4096.0, True), fixed(r, 4096.0, False)),
    }
    for name, (lo_e, hi_e, r_up, r_dn) in enc.items():
        ok = np.ones((len(leaves), r.shape[1]), bool)
        for k in LO:
            ok &= ~(lo_e[k][:, None] > r_up[k][None, :])
        for k in HI:
            ok &= ~(r_dn[k][None, :] > hi_e[k][:, None])
        counts[name] += int(ok.sum())
    for name, rng in (('fx13', 4.0), ('fx12', 8.0)):
        beyond[name] += int((np.abs(lo_r) >= rng).sum() + (np.abs(hi_r) >= rng).sum() + (np.abs(r) >= rng).sum())
print('bodies %d  leaves %d  vertices %d' % (nb, len(leaves), verts.shape[1]))
for name in ('exact', 'half', 'fx13', 'fx12'):
    print('%-6s listed (ray, leaf) pairs %9d  per ray %.3f  vs half %+.3f %%%s'
          % (name, counts[name], counts[name] / (nb * verts.shape[1]), 100.0 * (counts[name] / counts['half'] - 1.0),
             '   values beyond the range: %d' % beyond[name] if name in beyond else ''))
