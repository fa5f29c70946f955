#!/usr/bin/env python3
"""Timing of the fit to target meshes (tuch_amd/fit.py: MeshFitter, csrc/mesh_fit.hip), DESIGN.md §3:

    python tools/mesh_fit_timing.py                 # all of it, one JSON line each
    python tools/mesh_fit_timing.py --only fit      # warm-up + ONE call of --iters replayed iterations: for a
                                                    # rocprofv3 --kernel-trace --stats run of its own (launches per iteration)

Batch 64 on the synthetic full body (V = 6890), targets = the body at random poses + a translation.
* the loop: device events around whole calls of --iters iterations (>= 200), --repeats blocks per version, the versions
  alternating within the process.  `MeshFitter` on a kept session (replays only; the call's input copies and its
  final evaluation are inside the window: two body-model passes per call), `MeshFitter(use_graph=False)`, and the baseline --
  what the package lets a user write without this module: SMPL(...) + torch.norm(...).mean(1).sum() +
  torch.optim.Adam(capturable=True), eager on the device;
* the data term alone: replays of a graph that holds ten ops.vertex_fit calls (the device time of one launch), and the
  bytes it has to move (verts + target read, the vertex gradient written) over that time against the HBM peak.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from synthetic import make_body, random_poses      # noqa: E402
from tuch_amd import ops                           # noqa: E402
from tuch_amd.fit import MeshFitter                # noqa: E402
from tuch_amd.models.smpl import SMPL              # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, MI355X specification (about 6.3e12 is what a plain copy reaches)
BATCH = 64


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def spread(ms_per_iter):
    return {'median_ms': round(statistics.median(ms_per_iter), 5), 'min_ms': round(min(ms_per_iter), 5),
            'max_ms': round(max(ms_per_iter), 5)}


def baseline_loop(smpl, target, global_orient, iters):
    """The reference's loop (tuch/utils/smplxtosmpl_mtp.py:63-105) as torch ops around the package's body model."""
    batch = target.shape[0]
    z = lambda n: torch.zeros(batch, n, device=target.device, requires_grad=True)
    body_pose, betas = z(69), z(10)
    with torch.no_grad():
        verts = smpl(global_orient=global_orient, body_pose=body_pose, betas=betas).vertices
        transl = (target.mean(1) - verts.mean(1)).clone()
    transl.requires_grad_(True)
    opt = torch.optim.Adam([body_pose, betas, transl], lr=1e-2, capturable=True)
    for _ in range(iters):
        opt.zero_grad()
        verts = smpl(global_orient=global_orient, body_pose=body_pose, betas=betas).vertices
        loss = torch.norm(target - (verts + transl[:, None]), dim=2).mean(1).sum()
        loss.backward()
        opt.step()
    return body_pose, betas, transl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', choices=('fit',), default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    body = make_body(with_geodesics=False)
    assert body.num_verts == 6890
    smpl = SMPL(model_data=body, batch_size=BATCH).to(dev)
    bp, go, be = (torch.tensor(x, device=dev) for x in random_poses(BATCH, 5))
    with torch.no_grad():
        shift = 0.1 * torch.randn(BATCH, 3, device=dev, generator=torch.Generator(dev).manual_seed(5))
        target = smpl(global_orient=go, body_pose=bp, betas=be).vertices + shift[:, None]
    fitter = MeshFitter(smpl, num_iters=a.iters)
    fit = fitter(target, go)                     # three eager iterations, the capture, iters - 3 replays
    torch.cuda.synchronize()
    if a.only == 'fit':
        ms = timed(lambda: fitter(target, go))
        print(json.dumps({'what': 'MeshFitter, kept session', 'iters': a.iters, 'replayed': fitter.graph_replayed,
                          'ms_per_iter': round(ms / a.iters, 5)}), flush=True)
        return
    eager = MeshFitter(smpl, num_iters=a.iters, use_graph=False)
    eager(target, go)
    base = baseline_loop(smpl, target, go, a.iters)
    torch.cuda.synchronize()
    # the same fit: the baseline's trajectory is the float32 one of the same loop (it departs past ~100 iterations)
    short = MeshFitter(smpl, num_iters=50, use_graph=False)(target, go)
    short_base = baseline_loop(smpl, target, go, 50)
    agree = max(float((x - y).abs().max()) for x, y in zip((short.body_pose, short.betas, short.transl), short_base))
    t = {'graph': [], 'eager': [], 'baseline': []}
    for _ in range(a.repeats):
        t['graph'].append(timed(lambda: fitter(target, go)) / a.iters)
        t['eager'].append(timed(lambda: eager(target, go)) / a.iters)
        t['baseline'].append(timed(lambda: baseline_loop(smpl, target, go, a.iters)) / a.iters)
    for name, what in (('graph', 'MeshFitter, kept session (replays)'), ('eager', 'MeshFitter(use_graph=False)'),
                       ('baseline', 'SMPL + torch.norm + torch.optim.Adam(capturable), eager')):
        print(json.dumps(dict({'what': what, 'batch': BATCH, 'V': 6890, 'iters': a.iters, 'repeats': a.repeats},
                              **spread(t[name]))), flush=True)
    print(json.dumps({'what': 'final / initial loss after %d iterations (largest body)' % a.iters,
                      'value': float((fit.loss / MeshFitter(smpl, num_iters=0)(target, go).loss).max()),
                      'params_vs_baseline_after_50_iterations_max_abs': agree}), flush=True)
    # ---- the data term alone
    verts = smpl(global_orient=go, body_pose=bp, betas=be).vertices.detach()
    transl = torch.zeros(BATCH, 3, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        ops.vertex_fit(verts, transl, target)
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(10):
                ops.vertex_fit(verts, transl, target)
        graph.replay()
        torch.cuda.synchronize()
        per_call = [timed(lambda: [graph.replay() for _ in range(a.iters // 10)]) / (a.iters // 10 * 10) for _ in range(a.repeats)]
    nbytes = BATCH * 6890 * 3 * 4 * 3
    ms = statistics.median(per_call)
    print(json.dumps(dict({'what': 'vertex_fit alone (graph of ten calls)', 'bytes': nbytes,
                           'achieved_TB_per_s': round(nbytes / (ms * 1e-3) / 1e12, 3),
                           'share_of_hbm_peak': round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}, **spread(per_call))), flush=True)


if __name__ == '__main__':
    main()
