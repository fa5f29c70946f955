#!/usr/bin/env python3
"""Timing of self-contact detection (csrc/self_contact.hip), DESIGN.md "Self-contact detection":

    python tools/self_contact_time.py                  # one JSON line: ms per call of both routes and their ratio
    python tools/self_contact_time.py --only new       # for a rocprofv3 --kernel-trace --stats run of its own

Shape: batch 64, V = 6890, 24 regions, synthetic.make_body() posed with random_poses.  Two routes to the same numbers
(per-vertex contact flags and partners, the body minimum, the R x R contact signature):
  * new:   SelfContact.__call__ -- one search launch behind a preset launch, plus torch's square roots;
  * route before this kernel existed: ContactModel.v2v_min (nearest masked vertex of every vertex) +
    region_pair_min(masked=True) over all R (R + 1) / 2 region pairs, thresholded with torch.
HIP events around blocks of --iters back-to-back eager calls after a warm-up; the median of --blocks blocks, the two
routes alternating block by block.  The results of the two routes are compared before anything is timed.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from oracle import lbs as olbs                                  # noqa: E402
from synthetic import make_body, random_poses                   # noqa: E402
from tuch_amd import ops                                        # noqa: E402
from tuch_amd.contact_detect import SelfContact                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--euclthres', type=float, default=0.02)
    ap.add_argument('--only', choices=['new', 'before'], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('self_contact_time.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    body = make_body()
    bp, go, be = random_poses(a.batch, 1002)
    verts, _ = olbs.smpl_forward(olbs.model_tensors(body), torch.tensor(be), torch.tensor(bp), torch.tensor(go))
    verts = verts.to(torch.float32).to(dev).contiguous()
    mask = body.geodesics >= 0.3
    names = list(body.regions.keys())
    lists = [np.asarray(body.regions[n], np.int64) for n in names]
    R = len(lists)
    iu = np.triu_indices(R)
    pairs = np.stack(iu, 1)                                                       # all R (R + 1) / 2 pairs, r1 <= r2
    det = SelfContact(geomask=mask, euclthres=a.euclthres, regions=lists, device=dev)
    model = ops.ContactModel(body.faces, mask, None, lists, pairs, device=dev)
    e2 = float(np.float32(a.euclthres) * np.float32(a.euclthres))
    r1, r2 = (torch.tensor(x, device=dev) for x in iu)
    inf = torch.tensor(float('inf'), device=dev)

    def new():
        return det(verts)

    def before():
        mn, arg = model.v2v_min(verts)
        ic = mn < e2
        pm = model.region_pair_min(verts, masked=True)[0]
        pm = torch.where((pm < e2) & (pm > 0), pm, inf)        # (0: a pair of regions without an admissible vertex pair)
        sig = torch.full((verts.shape[0], R, R), float('inf'), device=dev)
        sig[:, r1, r2] = pm
        sig = torch.minimum(sig, sig.transpose(1, 2))           # the mask and the distances are symmetric
        d2 = torch.where(ic, mn, inf)
        return {'in_contact': ic, 'partner': torch.where(ic, arg, -1), 'dist': torch.sqrt(d2),
                'cnc': torch.sqrt(d2.min(1)[0]), 'signature': torch.sqrt(sig)}

    routes = {'new': new, 'before': before}
    if a.only:
        routes = {a.only: routes[a.only]}
    outs = {k: f() for k, f in routes.items()}
    torch.cuda.synchronize()
    agree = None
    if len(outs) == 2:
        n, o = outs['new'], outs['before']
        agree = {'in_contact': bool(torch.equal(n['in_contact'], o['in_contact'])),
                 'dist': bool(torch.equal(n['dist'], o['dist'])), 'cnc': bool(torch.equal(n['cnc'], o['cnc'])),
                 # the intra-region entries (r, r) of the pair route see each pair from both sides: the same minimum
                 'signature': bool(torch.equal(n['signature'], o['signature'])),
                 'contact_vertices_per_body': float(n['in_contact'].sum().item()) / a.batch}
    for f in routes.values():                                   # warm-up of every shape the timed window uses
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.blocks):
        for k, f in routes.items():
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.iters)
    res = {'what': 'self_contact', 'batch': a.batch, 'V': body.num_verts, 'R': R, 'pairs': int(len(pairs)),
           'euclthres': a.euclthres, 'iters': a.iters, 'blocks': a.blocks, 'agree': agree}
    for k, t in times.items():
        res[k + '_ms_per_call'] = round(float(np.median(t)), 4)
        res[k + '_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
    if len(times) == 2:
        res['before_over_new'] = round(res['before_ms_per_call'] / res['new_ms_per_call'], 2)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
