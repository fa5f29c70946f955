#!/usr/bin/env python3
"""Timing of the mesh renderer (csrc/render.hip), DESIGN.md §3 "Rendering":

    python tools/render_timing.py                      # one JSON line
    python tools/render_timing.py --only eager         # for a rocprofv3 --kernel-trace --stats run of its own

Shape: batch 64, V = 6890 (synthetic.make_body() posed with random_poses through SMPL.forward), the three reference
views at 224 x 224, vertex colours from contact_colors(partner=...) of a SelfContact-style partner list, the front view
over a background.  Reported, in milliseconds:
  * eager:  MeshRenderer.render per call -- HIP events around blocks of --iters back-to-back calls after a warm-up, the
            median of --blocks blocks;
  * graph:  the same call captured once and replayed, measured the same way;
  * colors: MeshRenderer.contact_colors(partner=...) per call, eager;
  * kernels: average device time of each kernel of one eager call (torch.profiler; null when the profiler reports no
            device activity -- use rocprofv3 --kernel-trace --stats with --only eager then).
There is no threshold: no earlier implementation exists on this hardware.
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from synthetic import make_body, random_poses                   # noqa: E402
from tuch_amd import ops                                        # noqa: E402
from tuch_amd.models.smpl import SMPL                           # noqa: E402
from tuch_amd.render import MeshRenderer                        # noqa: E402

VIEWS = ('front', 'rot2', 'rot3')


def timed(fn, iters, blocks):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(blocks):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def kernel_times(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            t = getattr(ev, 'device_time', None)
            if t is None:
                t = getattr(ev, 'cuda_time', 0.0)
            name = re.search(r'render_\w+|colors_\w+|Memset', ev.key)
            if t and name:
                out[name.group(0)] = round(float(t) / 1000.0, 4)
        return out or None
    except Exception as exc:                                    # the profiler is optional; the three totals are not
        return {'error': repr(exc)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--res', type=int, default=224)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=9)
    ap.add_argument('--only', choices=['eager', 'graph'], default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('render_timing.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    body = make_body(with_geodesics=False)
    bp, go, be = [torch.tensor(x, device=dev) for x in random_poses(a.batch, 1002)]
    verts = SMPL(model_data=body).to(dev)(betas=be, body_pose=bp, global_orient=go).vertices.detach().contiguous()
    b, v, _ = verts.shape
    tz = 5.0
    f = 0.8 * a.res * tz / float(np.ptp(body.v_template, 0).max())
    cam = torch.tensor([[0.0, 0.0, tz]], device=dev).repeat(b, 1)
    rng = np.random.default_rng(0)
    partner = torch.full((b, v), -1, dtype=torch.int32, device=dev)             # a few hundred contact vertices per body
    idx = torch.tensor(rng.integers(0, v, (b, 300)), device=dev)
    partner.scatter_(1, idx, torch.tensor(rng.integers(0, v, (b, 300)), dtype=torch.int32, device=dev))
    bg = torch.rand(b, a.res, a.res, 3, device=dev)
    r = MeshRenderer(body.faces, img_res=a.res, focal_length=f)
    colors = r.contact_colors(verts, partner=partner)

    def eager():
        return r.render(verts, cam, views=VIEWS, colors=colors, background=bg)

    def colour():
        return r.contact_colors(verts, partner=partner)

    out = eager()
    torch.cuda.synchronize()
    res = {'what': 'render', 'batch': b, 'V': v, 'F': body.num_faces, 'views': len(VIEWS), 'res': a.res,
           'covered_share': round(float((out['face'] >= 0).float().mean().item()), 4), 'iters': a.iters, 'blocks': a.blocks}
    for _ in range(5):
        eager()
        colour()
    torch.cuda.synchronize()
    if a.only != 'graph':
        t = timed(eager, a.iters, a.blocks)
        res['eager_ms_per_call'] = round(float(np.median(t)), 4)
        res['eager_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
    if a.only is None:
        t = timed(colour, a.iters, a.blocks)
        res['colors_ms_per_call'] = round(float(np.median(t)), 4)
    if a.only != 'eager':
        with ops.off_default_stream(dev):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                captured = eager()
            g.replay()
            torch.cuda.synchronize()
            res['graph_equals_eager'] = bool(all(torch.equal(captured[k], out[k]) for k in out))
            t = timed(g.replay, a.iters, a.blocks)
        res['graph_ms_per_replay'] = round(float(np.median(t)), 4)
        res['graph_ms_min_max'] = [round(min(t), 4), round(max(t), 4)]
    if a.only is None:
        res['kernels_ms'] = kernel_times(eager)
        res['colors_kernels_ms'] = kernel_times(colour)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
