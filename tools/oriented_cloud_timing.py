#!/usr/bin/env python3
"""Timing of the normal-compatible model -> scan term (csrc/point_cloud.hip: tuch_point_cloud_fit_terms with normals;
ops.cloud_fit with max_angle) against the unoriented term, and of a whole two-sided ScanFitter iteration with and
without model_to_scan_normals, DESIGN.md §3:

    python tools/oriented_cloud_timing.py                # all of it, one JSON line each
    python tools/oriented_cloud_timing.py --only term    # the term: unoriented, oriented with cones, oriented without
    python tools/oriented_cloud_timing.py --only fit     # ScanFitter per iteration, flag on against flag off
    python tools/oriented_cloud_timing.py --max-distance 0.1     # the same with the term truncated at 10 cm

Batch 64 on the synthetic full body (V = 6890).  The scan of a body sees one side of it: of three points per face of the
body at a random pose + a translation, those whose face normal has a positive z (a sensor on +z), about 20 000 per body,
with those faces' unit normals; the clouds are ragged (counts).  The term's vertices are the true body moved by 1 cm --
a fit close to its end -- hinted with the answers one further centimetre away, as a fitter's loop hints it.  Device
events, --repeats blocks per version, the versions alternating, medians; replays of a graph that holds one call.  Every
GPU step of a job that runs this tool belongs under a `timeout` of its own.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from closest_point_timing import spread, timed     # noqa: E402
from scan_fit_timing import graph_of               # noqa: E402
from synthetic import make_body, random_poses      # noqa: E402
from tuch_amd import ops                           # noqa: E402
from tuch_amd.fit import ScanFitter                # noqa: E402
from tuch_amd.models.smpl import SMPL              # noqa: E402
from tuch_amd.ops import ContactModel, PointCloud  # noqa: E402

BATCH = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10, help='calls per timed block')
    ap.add_argument('--angle', type=float, default=60.0)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--max-distance', type=float, default=None, help='tau of the model -> scan term (default: none)')
    ap.add_argument('--only', choices=('term', 'fit'), default=None)
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
        verts = smpl(global_orient=go, body_pose=bp, betas=be).vertices.contiguous()
        faces = model.faces_i32.long()
        tri = (verts + shift[:, None])[:, faces]                                 # [B,F,3,3]
        w = torch.rand(len(faces), 3, 3, device=dev, generator=gen)
        w = w / w.sum(2, keepdim=True)
        samples = (w[None, :, :, :, None] * tri[:, :, None]).sum(3)             # [B,F,3 samples,3]
        normal = torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=2)
        normal = normal / normal.norm(dim=2, keepdim=True).clamp_min(1e-20)
        seen = (normal[:, :, 2] > 0)[:, :, None].expand(-1, -1, 3).reshape(BATCH, -1)
        samples, normal = samples.reshape(BATCH, -1, 3), normal[:, :, None].expand(-1, -1, 3, -1).reshape(BATCH, -1, 3)
        counts = seen.sum(1).to(torch.int32)
        order = torch.argsort((~seen).to(torch.int8), dim=1, stable=True)[:, :int(counts.max())]   # the seen points first
        take = lambda x: torch.gather(x, 1, order[:, :, None].expand(-1, -1, 3)).contiguous()
        points, normals = take(samples), take(normal)
        beyond = torch.arange(points.shape[1], device=dev)[None] >= counts[:, None]
        points[beyond] = float('nan')                                           # never to be read
    say = lambda line: print(json.dumps(line), flush=True)
    say({'what': 'one-sided scan', 'batch': BATCH, 'points_per_body_mean': round(float(counts.float().mean()), 1),
         'points_per_body_min': int(counts.min()), 'points_per_body_max': int(counts.max())})
    table = ops.vertex_normal_table(body.faces, body.num_verts, dev)
    if a.only in (None, 'term'):
        step = torch.full((BATCH, 3), 0.01 / 3 ** 0.5, device=dev)
        transl, earlier = (shift + step).contiguous(), (shift + 2 * step).contiguous()
        clouds = {'unoriented': PointCloud(points, counts, resolution=a.resolution),
                  'oriented, cones': PointCloud(points, counts, resolution=a.resolution).orient(normals, cones=True),
                  'oriented, no cones': PointCloud(points, counts, resolution=a.resolution).orient(normals, cones=False)}
        graphs, unmatched = {}, None
        with torch.no_grad():
            for name, cloud in clouds.items():
                kw = dict(max_distance=a.max_distance, **({} if name == 'unoriented' else dict(max_angle=a.angle, normal_table=table)))
                hint = ops.cloud_fit(cloud, verts, earlier, **kw)[2].index
                graphs[name] = graph_of(lambda c=cloud, h=hint, kw=kw: ops.cloud_fit(c, verts, transl, hint=h, **kw))
                graphs[name + ', unhinted'] = graph_of(lambda c=cloud, kw=kw: ops.cloud_fit(c, verts, transl, **kw))
            a_out, b_out = graphs['oriented, cones'][1], graphs['oriented, no cones'][1]
            assert torch.equal(a_out[2].index, b_out[2].index) and torch.equal(a_out[2].d2, b_out[2].d2)
            assert torch.equal(a_out[0], b_out[0])
            unmatched = float((a_out[2].index < 0).float().mean())
            cone_graph = graph_of(lambda: clouds['oriented, cones'].orient(normals, cones=True))[0]
        say({'what': 'share of vertices without a match, oriented', 'angle': a.angle, 'max_distance': a.max_distance, 'value': round(unmatched, 4)})
        t = {k: [] for k in graphs}
        t['cone build'] = []
        for _ in range(a.repeats):
            for k, (graph, _) in graphs.items():
                t[k].append(timed(lambda: [graph.replay() for _ in range(a.calls)]) / a.calls)
            t['cone build'].append(timed(lambda: [cone_graph.replay() for _ in range(a.calls)]) / a.calls)
        for k, ms in t.items():
            say(dict({'what': 'cloud_fit %s, replayed' % k if k != 'cone build' else 'PointCloud.orient (the cone build), replayed',
                      'batch': BATCH, 'V': 6890, 'resolution': a.resolution, 'calls': a.calls, 'repeats': a.repeats},
                     **spread(ms)))
        base = spread(t['unoriented'])['median_ms']
        for k in ('oriented, cones', 'oriented, no cones'):
            say({'what': '%s / unoriented (hinted)' % k, 'value': round(spread(t[k])['median_ms'] / base, 4)})
        base = spread(t['unoriented, unhinted'])['median_ms']
        for k in ('oriented, cones, unhinted', 'oriented, no cones, unhinted'):
            say({'what': '%s / unoriented (unhinted)' % k, 'value': round(spread(t[k])['median_ms'] / base, 4)})
    if a.only in (None, 'fit'):
        make = lambda flag: ScanFitter(smpl, model, num_iters=a.iters, fit_global_orient=False, model_to_scan=1.0,
                                       resolution=a.resolution, max_normal_angle=a.angle, max_distance=a.max_distance,
                                       model_to_scan_normals=flag)
        fitters = {'off': make(False), 'on': make(True)}
        for f in fitters.values():
            f(points, go, counts=counts, normals=normals)          # three eager iterations, the capture, iters - 3 replays
        torch.cuda.synchronize()
        t = {k: [] for k in fitters}
        for _ in range(a.repeats):
            for k, f in fitters.items():
                t[k].append(timed(lambda: f(points, go, counts=counts, normals=normals)) / a.iters)
        for k, ms in t.items():
            say(dict({'what': 'ScanFitter(model_to_scan=1.0, model_to_scan_normals=%s), kept session, per iteration' % (k == 'on'),
                      'batch': BATCH, 'iters': a.iters, 'repeats': a.repeats}, **spread(ms)))
        say({'what': 'flag on / flag off per iteration',
             'value': round(spread(t['on'])['median_ms'] / spread(t['off'])['median_ms'], 4)})


if __name__ == '__main__':
    main()
