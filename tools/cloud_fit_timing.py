#!/usr/bin/env python3
"""Timing of the nearest-point query of a point cloud (csrc/point_cloud.hip; ops.PointCloud, ops.cloud_fit) and of the
two-sided ScanFitter (tuch_amd/fit.py), DESIGN.md §3:

    python tools/cloud_fit_timing.py                 # all of it, one JSON line each
    python tools/cloud_fit_timing.py --only build    # (a) the build at Q = 6890 and Q = 41 328
    python tools/cloud_fit_timing.py --only nearest  # (b) the query, hinted and unhinted, late in a fit and at its start
    python tools/cloud_fit_timing.py --only fit      # (c) ScanFitter per iteration, model_to_scan 1.0 against 0.0
    python tools/cloud_fit_timing.py --only trace    # warm-up + ONE two-sided call of --iters replayed iterations: for a
                                                     # rocprofv3 --kernel-trace --stats run of its own

Batch 64 on the synthetic full body (V = 6890).  The scan of a body is the surface of that body at a random pose + a
translation: its vertices (Q = 6890) and three points per face (Q = 41 328).  Device events, --repeats blocks per
version, the versions alternating, medians.  Every GPU step of a job that runs this tool belongs under a `timeout` of
its own.
* the query: replays of a graph that holds one `nearest` call over all 64 x 6890 vertices.  "late": the vertices of the
  fit's state before update --at, hinted with the answers of the state one Adam step earlier (not the exact answer, which
  flatters); "start": the zero pose at the centroid translation, where the answers are decimetres away, hinted with the
  answers of the same mesh moved by one Adam step's worth (1 cm).
* the visits: from the headers (PointCloud.grid) and the answers, computed on the host for body 0 -- per query the
  occupied cells whose box is within the query's final distance (what ANY exact grid walk opens at least; the walk's own
  bound is larger while it runs, so it opens these and some more) and the points in them (the exact tests at least).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from closest_point_timing import spread, timed     # noqa: E402
from scan_fit_timing import graph_of               # noqa: E402
from synthetic import make_body, random_poses      # noqa: E402
from tuch_amd.fit import ScanFitter                # noqa: E402
from tuch_amd.models.smpl import SMPL              # noqa: E402
from tuch_amd.ops import ContactModel, PointCloud  # noqa: E402

BATCH = 64


def visits(cloud, points, queries, d2, body=0, chunk=256):
    """(cells, tests) per query of one body, float64 on the host: occupied cells whose box lies within sqrt(d2) of the
    query, and the points filed in them."""
    g = cloud.grid()
    o, cell, dims = g.origin[body].astype(np.float64), float(g.cell[body]), g.dims[body].astype(np.int64)
    p = points[body].cpu().numpy()
    t32 = ((p - g.origin[body]).astype(np.float32) * np.float32(1.0 / g.cell[body])).astype(np.float32)     # as pc_t
    c = np.clip(t32.astype(np.int64), 0, dims - 1)
    lin = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    used, count = np.unique(lin, return_counts=True)
    cz, rem = np.divmod(used, dims[0] * dims[1])
    cy, cx = np.divmod(rem, dims[0])
    lo = o + np.stack([cx, cy, cz], 1) * cell
    q = queries[body].cpu().numpy().astype(np.float64)
    r2 = d2[body].cpu().numpy().astype(np.float64)
    cells, tests = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
    for s in range(0, len(q), chunk):
        gap = np.maximum(np.maximum(lo[None] - q[s:s + chunk, None], q[s:s + chunk, None] - (lo[None] + cell)), 0.0)
        near = (gap ** 2).sum(-1) <= r2[s:s + chunk, None]
        cells[s:s + chunk] = near.sum(1)
        tests[s:s + chunk] = (near * count[None]).sum(1)
    return cells, tests, len(used)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10, help='calls per timed block')
    ap.add_argument('--at', type=int, default=60, help='the late state: the fit\'s parameters before update AT')
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--only', choices=('build', 'nearest', 'fit', 'trace'), default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    body = make_body(with_geodesics=False)
    assert body.num_verts == 6890
    smpl = SMPL(model_data=body, batch_size=BATCH).to(dev)
    model = ContactModel(body.faces, device=dev)
    bp, go, be = (torch.tensor(x, device=dev) for x in random_poses(BATCH, 5))
    gen = torch.Generator(dev).manual_seed(5)
    with torch.no_grad():
        shift = 0.1 * torch.randn(BATCH, 3, device=dev, generator=gen)
        true = smpl(global_orient=go, body_pose=bp, betas=be).vertices + shift[:, None]
        faces = model.faces_i32.long()
        w = torch.rand(len(faces), 3, 3, device=dev, generator=gen)
        w = w / w.sum(2, keepdim=True)
        hd = (w[None, :, :, :, None] * true[:, faces][:, :, None]).sum(3).reshape(BATCH, -1, 3).contiguous()
    scans = {'Q=6890': true.contiguous(), 'Q=41328': hd}
    say = lambda line: print(json.dumps(line), flush=True)
    if a.only in (None, 'build'):
        clouds = {name: PointCloud(points, resolution=a.resolution) for name, points in scans.items()}
        graphs = {name: graph_of(lambda c=clouds[name], p=scans[name]: c.rebuild(p))[0] for name in scans}
        t = {name: [] for name in scans}
        for _ in range(a.repeats):
            for name, graph in graphs.items():
                t[name].append(timed(lambda: [graph.replay() for _ in range(a.calls)]) / a.calls)
        for name, ms in t.items():
            say(dict({'what': 'PointCloud build, replayed, ' + name, 'batch': BATCH, 'resolution': a.resolution,
                      'workspace_MiB': round(clouds[name]._nbytes / 2 ** 20, 1)}, **spread(ms)))
    if a.only in (None, 'nearest'):
        probe = ScanFitter(smpl, model, num_iters=a.at + 1, fit_global_orient=False, use_graph=False, record_history=True,
                           model_to_scan=1.0, resolution=a.resolution)
        probe(scans['Q=6890'], go)
        step = torch.full((BATCH, 1, 3), 0.01 / 3 ** 0.5, device=dev)
        with torch.no_grad():
            states = {}
            for i in (a.at - 1, a.at):
                s = probe.history['fit'][i]['params']
                states[i] = (smpl(global_orient=go, body_pose=s[0], betas=s[1]).vertices + s[2][:, None]).contiguous()
            s = probe.history['fit'][0]['params']
            start = (smpl(global_orient=go, body_pose=s[0], betas=s[1]).vertices + s[2][:, None]).contiguous()
        for name, points in scans.items():
            cloud = PointCloud(points, resolution=a.resolution)
            for state, verts, earlier in (('late', states[a.at], states[a.at - 1]), ('start', start, (start + step).contiguous())):
                with torch.no_grad():
                    hint = cloud.nearest(earlier).index
                    graphs = {'unhinted': graph_of(lambda: cloud.nearest(verts)),
                              'hinted': graph_of(lambda: cloud.nearest(verts, hint=hint))}
                    for x, y in zip(graphs['unhinted'][1], graphs['hinted'][1]):
                        assert torch.equal(x, y)
                t = {k: [] for k in graphs}
                for _ in range(a.repeats):
                    for k, (graph, _) in graphs.items():
                        t[k].append(timed(lambda: [graph.replay() for _ in range(a.calls)]) / a.calls)
                answer = graphs['unhinted'][1]
                for k, ms in t.items():
                    say(dict({'what': 'nearest %s, replayed, %s, %s' % (k, state, name), 'batch': BATCH, 'N': 6890,
                              'calls': a.calls, 'repeats': a.repeats}, **spread(ms)))
                cells, tests, occupied = visits(cloud, points, verts, answer.d2)
                say({'what': 'visits per query at least (body 0), %s, %s' % (state, name), 'occupied_cells': occupied,
                     'median_distance_m': round(float(answer.d2[0].sqrt().median()), 5),
                     'hints_not_the_answer': round(float((hint != answer.index).float().mean()), 4),
                     'cells_mean': round(float(cells.mean()), 2), 'cells_max': int(cells.max()),
                     'tests_mean': round(float(tests.mean()), 2), 'tests_max': int(tests.max())})
    if a.only in (None, 'fit', 'trace'):
        points = scans['Q=6890']
        two = ScanFitter(smpl, model, num_iters=a.iters, fit_global_orient=False, model_to_scan=1.0, resolution=a.resolution)
        two(points, go)                             # three eager iterations, the capture, iters - 3 replays
        torch.cuda.synchronize()
        if a.only == 'trace':
            ms = timed(lambda: two(points, go))
            say({'what': 'ScanFitter(model_to_scan=1.0), kept session', 'iters': a.iters, 'replayed': two.graph_replayed,
                 'ms_per_iter': round(ms / a.iters, 5)})
            return
        one = ScanFitter(smpl, model, num_iters=a.iters, fit_global_orient=False)
        one(points, go)
        torch.cuda.synchronize()
        t = {'two': [], 'one': []}
        for _ in range(a.repeats):
            t['two'].append(timed(lambda: two(points, go)) / a.iters)
            t['one'].append(timed(lambda: one(points, go)) / a.iters)
        for key, what in (('one', 'ScanFitter(model_to_scan=0.0), kept session (replays)'),
                          ('two', 'ScanFitter(model_to_scan=1.0), kept session (replays, the cloud rebuilt per call)')):
            say(dict({'what': what, 'batch': BATCH, 'Q': 6890, 'iters': a.iters, 'repeats': a.repeats}, **spread(t[key])))
        say({'what': 'two-sided / one-sided per iteration',
             'value': round(spread(t['two'])['median_ms'] / spread(t['one'])['median_ms'], 4)})


if __name__ == '__main__':
    main()
