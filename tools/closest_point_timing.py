#!/usr/bin/env python3
"""Timing of the closest-point query (ContactModel.closest_point, csrc/closest_point.hip), DESIGN.md §3:

    python tools/closest_point_timing.py            # one JSON line per measurement

Batch 64 on the synthetic full body (V = 6890, F = 13776) at random poses.  Queries: the vertices of a second, slightly
displaced body in vertex order (Q = 6890), three points per face of it in face order (Q = 41 328, the HD size), and the
same two sets shuffled -- the stated slow case: a wavefront's 64 queries are then all over the body.
* before anything is timed: d2 of body 0 against a chunked torch restatement of the all-pairs computation in float64,
  within the bound of tests/closest_point_cases.py (4 x the float32 restatement's error, floored at 8 ulps of the squared
  coordinate scale);
* time per call with device events after a warm-up: eager calls, and replays of a graph that holds the call; --repeats
  blocks per version, the versions alternating, medians;
* group visits per wavefront, computed from the posed boxes and the answers (a group counts for a wavefront when some
  lane's box bound, with the kernel's margin, is within that lane's final d2: what the kernel visits once its bound has
  settled), the exact tests they stand for, and the vector-instruction issue estimate that follows;
* for scale, the all-pairs restatement in float32, chunked, at the largest batch that is practical (--pairs-batch).
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
from tuch_amd import _C                            # noqa: E402
from tuch_amd.models.smpl import SMPL              # noqa: E402
from tuch_amd.ops import ContactModel              # noqa: E402

BATCH = 64
EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 64.0 * 2.0 ** -24          # kCpMargin of csrc/closest_point.hip
VALU_PER_TEST = 145                 # vector instructions of one (query, triangle) test in the inner loop of cp_search_kernel (ISA count, area > 0)
VALU_PER_BOX = 29                   # ... of one box test (ISA count of sweep 1); both sweeps look at every box
SIMDS, CLOCK = 1024, 2.4e9          # MI355X: 256 CUs x 4 SIMDs; a wave64 vector instruction issues over 2 cycles


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def spread(ms):
    return {'median_ms': round(statistics.median(ms), 5), 'min_ms': round(min(ms), 5), 'max_ms': round(max(ms), 5)}


def _dot(a, b):
    return (a * b).sum(-1)


def _segment(p, s, e):
    d = e - s
    dd = _dot(d, d)
    t = torch.where(dd > 0, _dot(p - s, d) / torch.where(dd > 0, dd, torch.ones_like(dd)), torch.zeros_like(dd)).clamp(0, 1)
    r = p - (s + t[..., None] * d)
    return _dot(r, r)


def all_pairs_d2(points, tri, chunk=128):
    """min over faces of the point-triangle distance, every pair evaluated: points [Q,3], tri [F,3,3] (their dtype)."""
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    n = torch.cross(b - a, c - a, dim=-1)
    nn = _dot(n, n)
    out = []
    for i in range(0, len(points), chunk):
        p = points[i:i + chunk, None]
        best = torch.minimum(torch.minimum(_segment(p, a, b), _segment(p, b, c)), _segment(p, c, a))
        inside = nn > 0
        for s, e in ((a, b), (b, c), (c, a)):
            inside = inside & (_dot(n, torch.cross((e - s).expand(len(p), -1, -1), p - s, dim=-1)) >= 0)
        h = _dot(n, p - a)
        out.append(torch.where(inside, h * h / torch.where(nn > 0, nn, torch.ones_like(nn)), best).min(1).values)
    return torch.cat(out)


def group_visits(model, verts, points, d2):
    """Per wavefront of 64 consecutive queries: groups visited and exact tests run (see the module docstring)."""
    leaf = np.zeros(model.num_faces, np.int32)
    _C.check(_C.lib().tuch_contact_model_tree_order(model._handle, None, leaf.ctypes.data_as(_C.c_void_p)))
    dev = verts.device
    leaf_t = torch.as_tensor(leaf, device=dev).long()
    groups = int(leaf.max()) + 1
    size = torch.bincount(leaf_t, minlength=groups).float()
    visits, tests = [], []
    for b in range(0, verts.shape[0], 8):
        corners = verts[b:b + 8][:, model.faces_i32.long()].reshape(-1, model.num_faces, 9)       # [b,F,9]
        idx = leaf_t[None, :, None].expand(corners.shape[0], -1, 3)
        lo = torch.full((corners.shape[0], groups, 3), float('inf'), device=dev)
        hi = -lo
        for k in range(3):
            lo = lo.scatter_reduce(1, idx, corners[:, :, 3 * k:3 * k + 3], 'amin')
            hi = hi.scatter_reduce(1, idx, corners[:, :, 3 * k:3 * k + 3], 'amax')
        p = points[b:b + 8][:, :, None]                                                             # [b,Q,1,3]
        near = torch.maximum(torch.maximum(lo[:, None] - p, p - hi[:, None]), torch.zeros((), device=dev))
        far = torch.maximum(p - lo[:, None], hi[:, None] - p)
        admit = _dot(near, near) - MARGIN * _dot(far, far) <= d2[b:b + 8][:, :, None]               # [b,Q,G]
        q = admit.shape[1]
        pad = (-q) % 64
        if pad:
            admit = torch.cat([admit, torch.zeros(admit.shape[0], pad, groups, dtype=torch.bool, device=dev)], 1)
        wave = admit.view(admit.shape[0], -1, 64, groups).any(2)                                    # [b,waves,G]
        visits.append(wave.sum(2).float().flatten())
        tests.append((wave.float() * size).sum(2).flatten())
    return torch.cat(visits), torch.cat(tests), groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20, help='calls per timed block')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--pairs-batch', type=int, default=2)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    body = make_body(with_geodesics=False)
    assert body.num_verts == 6890
    smpl = SMPL(model_data=body, batch_size=BATCH).to(dev)
    bp, go, be = (torch.tensor(x, device=dev) for x in random_poses(BATCH, 5))
    gen = torch.Generator(dev).manual_seed(5)
    with torch.no_grad():
        verts = smpl(global_orient=go, body_pose=bp, betas=be).vertices.contiguous()
        other = smpl(global_orient=go, body_pose=bp + 0.02 * torch.randn(bp.shape, device=dev, generator=gen), betas=be).vertices
        other = (other + 5e-3 * torch.randn(BATCH, 1, 3, device=dev, generator=gen)).contiguous()
    model = ContactModel(body.faces, device=dev)
    faces = model.faces_i32.long()
    w = torch.rand(len(faces), 3, 3, device=dev, generator=gen)
    w = w / w.sum(2, keepdim=True)
    hd = (w[None, :, :, :, None] * other[:, faces][:, :, None]).sum(3).reshape(BATCH, -1, 3).contiguous()        # [B,3F,3]
    sets = {}
    for name, pts in (('Q=6890 vertex order', other), ('Q=41328 face order', hd)):
        sets[name] = pts
        sets[name.replace('order', 'order, shuffled')] = pts[:, torch.randperm(pts.shape[1], device=dev, generator=gen)].contiguous()
    # ---- the answers first
    tri = verts[0][faces]
    for name, pts in sets.items():
        if 'Q=6890' not in name:
            continue
        got = model.closest_point(verts[:1], pts[:1]).d2[0].double()
        d64 = all_pairs_d2(pts[0].double(), tri.double())
        d32 = all_pairs_d2(pts[0], tri).double()
        scale = max(float(verts[0].abs().max()), float(pts[0].abs().max()))
        bound = max(4.0 * float((d32 - d64).abs().max()), 8.0 * EPS32 * scale ** 2)
        err = float((got - d64).abs().max())
        print(json.dumps({'what': 'd2 against the float64 all-pairs restatement, body 0, ' + name, 'max_abs_err': err,
                          'bound': bound}), flush=True)
        assert err <= bound, (name, err, bound)
    # ---- time per call
    runs = {}
    for name, pts in sets.items():
        model.closest_point(verts, pts)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.closest_point(verts, pts)
            torch.cuda.current_stream().synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                kept = model.closest_point(verts, pts)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        runs[name] = (pts, graph, kept)
    t = {(name, how): [] for name in sets for how in ('eager', 'replayed')}
    for _ in range(a.repeats):
        for name, (pts, graph, _) in runs.items():
            t[name, 'eager'].append(timed(lambda: [model.closest_point(verts, pts) for _ in range(a.calls)]) / a.calls)
            t[name, 'replayed'].append(timed(lambda: [graph.replay() for _ in range(a.calls)]) / a.calls)
    for (name, how), ms in t.items():
        print(json.dumps(dict({'what': 'closest_point, %s, %s' % (name, how), 'batch': BATCH, 'calls': a.calls,
                               'repeats': a.repeats}, **spread(ms))), flush=True)
    # ---- what the wavefronts visit
    for name, (pts, _, kept) in runs.items():
        visits, tests, groups = group_visits(model, verts, pts, kept.d2)
        waves = visits.numel()
        valu = float(tests.sum()) * VALU_PER_TEST + 2.0 * waves * groups * VALU_PER_BOX
        print(json.dumps({'what': 'group visits per wavefront, ' + name, 'groups': groups, 'mean': round(float(visits.mean()), 2),
                          'max': int(visits.max()), 'exact_tests_per_wavefront_mean': round(float(tests.mean()), 1),
                          'issue_estimate_ms': round(valu * 2.0 / (SIMDS * CLOCK) * 1e3, 4)}), flush=True)
    # ---- for scale: every pair, float32, chunked
    nb = a.pairs_batch
    pts = sets['Q=6890 vertex order']
    all_pairs_d2(pts[0], tri)
    ms = [timed(lambda: [all_pairs_d2(pts[b], verts[b][faces]) for b in range(nb)]) for _ in range(3)]
    print(json.dumps(dict({'what': 'torch all-pairs restatement (float32, chunks of 128 queries), Q=6890', 'batch': nb,
                           'ms_per_body': round(statistics.median(ms) / nb, 3)}, **spread(ms))), flush=True)


if __name__ == '__main__':
    main()
