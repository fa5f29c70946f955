"""Host count behind the crossing walk's tiling rule (ray_winding.hip: ray_tiles_fill_kernel, ray_leaf_kernel): how many
rays does each (leaf, body) hold, how many of the walk's passes are remainder tiles (c mod 64 rays), and how many passes
are left when a leaf's remainder rides its last full tile as a second ray set?  The near test is near_encode_sim.py's
`exact` one (single precision, no encoding: the floor of what the device lists -- the fixed-point lists hold +0.5 % more).
The bench's bodies: make_body(84, 82, seed=1234), random_poses at batch 8.
    python tools/diag/ray_tile_sim.py [bodies] [seed]"""
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
strip = np.array([nodes[n, 3] for n in leaves], np.int64)
KX, KY = np.float32(0.3217), np.float32(0.4331)
f32 = np.float32


def project(x, y, z):          # slab_project, single precision
    return np.stack([x, y, z, x + y, x - y, x + z, x - z, y + z, y - z]).astype(f32)


LO = [0, 1, 3, 4, 6, 8]          # slabs whose LOWER bound the test uses
HI = [0, 1, 2, 3, 4, 5, 7]       # ... whose UPPER bound
c = np.zeros((nb, len(leaves)), np.int64)
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
    r = project(x - pc[0], y - pc[1], z - pc[2])            # [9][V], formed as the kernel forms them
    ok = np.ones((len(leaves), r.shape[1]), bool)
    for k in LO:
        ok &= ~(lo_r[k][:, None] > r[k][None, :])
    for k in HI:
        ok &= ~(r[k][None, :] > hi_r[k][:, None])
    c[b] = ok.sum(1)

full = c // 64
rem = c % 64
has_rem = rem > 0
tiles = full + has_rem                                      # a tile per 64 rays and one for what is left over
rides = has_rem & (full > 0)                                # a remainder whose leaf has a full tile as well
passes = np.where(c > 0, np.maximum(1, full), 0)            # the tiling rule: the remainder rides the last full tile
print('bodies %d  leaves %d  vertices %d  listed (ray, leaf) pairs %d' % (nb, len(leaves), verts.shape[1], int(c.sum())))
print('tiles of <= 64 rays       %6d  (%.0f per body): full %d, remainder %d (%.0f %%), %.1f rays in a remainder on average, '
      '%d of them hold <= 16 rays'
      % (tiles.sum(), tiles.sum() / nb, full.sum(), has_rem.sum(), 100.0 * has_rem.sum() / tiles.sum(), rem[has_rem].mean(),
         (has_rem & (rem <= 16)).sum()))
print('remainders beside a full tile %6d  (%d of them hold <= 16 rays)' % (rides.sum(), (rides & (rem <= 16)).sum()))
print('passes with the remainder riding the last full tile %6d  (%+.1f %%)'
      % (passes.sum(), 100.0 * (passes.sum() / tiles.sum() - 1.0)))
print('strip elements stepped through by passes: %d -> %d (%+.1f %%); filter steps (elements x ray sets): %d both ways'
      % ((tiles * strip[None]).sum(), (passes * strip[None]).sum(),
         100.0 * ((passes * strip[None]).sum() / (tiles * strip[None]).sum() - 1.0), (tiles * strip[None]).sum()))
