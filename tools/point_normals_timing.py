#!/usr/bin/env python3
"""Timing of the k nearest points of a cloud and of the PCA normals over them (csrc/point_cloud.hip; PointCloud.knn,
PointCloud.normals), DESIGN.md §3:

    python tools/point_normals_timing.py                      # all of it, one JSON line each
    python tools/point_normals_timing.py --sizes 6890         # one size only
    python tools/point_normals_timing.py --no-baseline        # without torch.cdist + topk

The clouds are surfaces of the synthetic full body at random poses: its vertices (Q = 6890) and random points of its
faces + 2 mm of noise (Q = 100 000); the queries are the cloud's own points (N = Q), as for scan normals.  k in {8, 16,
32}, batch 1 and 8, --resolution cells along the longest extent.  Device events around --calls replays of a graph that
holds one call, --repeats blocks per version, the versions alternating, medians.  The build of the grid is timed beside
them (it is paid once per cloud).  The baseline is what a user would write otherwise, on the same device: per body
torch.cdist of a block of queries against the cloud, squared, and topk(k, largest=False), the blocks sized so that the
distance matrix stays below --block-MiB; it is run eagerly (its allocations do not capture) --baseline-repeats times
after one warm-up.  Its neighbours are checked against knn's on the first block: the same indices wherever the float32
distances of cdist do not tie or swap within their own rounding.  Every GPU step of a job that runs this tool belongs
under a `timeout` of its own."""
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
from tuch_amd.models.smpl import SMPL              # noqa: E402
from tuch_amd.ops import PointCloud                # noqa: E402

KS = (8, 16, 32)


def clouds_of(batch, size, dev, seed=5):
    """[batch, size, 3] float32: the posed body's vertices (size 6890) or noisy random points of its faces."""
    body = make_body(with_geodesics=False)
    smpl = SMPL(model_data=body, batch_size=batch).to(dev)
    bp, go, be = (torch.tensor(x, device=dev) for x in random_poses(batch, seed))
    gen = torch.Generator(dev).manual_seed(seed)
    with torch.no_grad():
        verts = smpl(global_orient=go, body_pose=bp, betas=be).vertices
        if size == verts.shape[1]:
            return verts.contiguous()
        faces = torch.as_tensor(body.faces.astype('int64'), device=dev)
        tri = verts[:, faces]                                                # [B,F,3,3]
        area = torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1).norm(dim=-1)
        pick = torch.multinomial(area, size, replacement=True, generator=gen)                # [B,size]
        w = torch.rand(batch, size, 3, device=dev, generator=gen)
        w = w / w.sum(2, keepdim=True)
        corners = torch.gather(tri, 1, pick[:, :, None, None].expand(-1, -1, 3, 3))
        noise = 2e-3 * torch.randn(batch, size, 3, device=dev, generator=gen)
        return ((w[:, :, :, None] * corners).sum(2) + noise).contiguous()


def baseline(points, k, block_bytes):
    """torch.cdist + topk per body and block of queries: (d2 [B,N,k], index [B,N,k])."""
    b, n, _ = points.shape
    rows = max(1, min(n, block_bytes // (4 * n)))
    d2 = torch.empty(b, n, k, device=points.device)
    index = torch.empty(b, n, k, dtype=torch.int64, device=points.device)
    for body in range(b):
        for lo in range(0, n, rows):
            d = torch.cdist(points[body, lo:lo + rows], points[body])
            near = torch.topk(d, k, dim=1, largest=False)
            d2[body, lo:lo + rows] = near.values ** 2
            index[body, lo:lo + rows] = near.indices
    return d2, index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[6890, 100000])
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=5, help='replays per timed block')
    ap.add_argument('--baseline-repeats', type=int, default=2)
    ap.add_argument('--block-MiB', type=int, default=2048)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--no-baseline', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    say = lambda line: print(json.dumps(line), flush=True)
    for size in a.sizes:
        for batch in a.batches:
            points = clouds_of(batch, size, dev)
            view = points.mean(1) + torch.tensor([0.0, 0.0, 3.0], device=dev)
            cloud = PointCloud(points, resolution=a.resolution)
            shape = {'batch': batch, 'Q': size, 'N': size, 'resolution': a.resolution}
            graphs = {'build': graph_of(lambda: cloud.rebuild(points))[0]}
            kept = {}
            for k in KS:
                graphs['knn k=%d' % k], kept[k] = graph_of(lambda k=k: cloud.knn(None, k))
                graphs['normals k=%d' % k], normals = graph_of(lambda k=k: cloud.normals(None, k, view))
                shape_k = dict(shape, k=k)
                say(dict({'what': 'normals: share of zero rows', 'value': round(float((normals.normal == 0).all(2).float().mean()), 6)},
                         **shape_k))
            t = {name: [] for name in graphs}
            for _ in range(a.repeats):
                for name, graph in graphs.items():
                    t[name].append(timed(lambda: [graph.replay() for _ in range(a.calls)]) / a.calls)
            for name, ms in t.items():
                say(dict({'what': name + ', replayed', 'calls': a.calls, 'repeats': a.repeats}, **shape, **spread(ms)))
            if a.no_baseline:
                continue
            for k in KS:
                with torch.no_grad():
                    d2, index = baseline(points, k, a.block_MiB << 20)       # warm-up, and the comparison
                    same = float((index == kept[k].index.long()).float().mean())
                    ms = [timed(lambda: baseline(points, k, a.block_MiB << 20)) for _ in range(a.baseline_repeats)]
                say(dict({'what': 'torch.cdist + topk k=%d, eager' % k, 'repeats': a.baseline_repeats,
                          'block_MiB': a.block_MiB, 'indices_equal_to_knn': round(same, 6)}, **shape, **spread(ms)))
                say(dict({'what': 'cdist + topk / knn k=%d' % k,
                          'value': round(spread(ms)['median_ms'] / spread(t['knn k=%d' % k])['median_ms'], 2)}, **shape))
            del d2, index
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
