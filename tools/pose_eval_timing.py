#!/usr/bin/env python3
"""Timing of the pose evaluation (csrc/pose_eval.hip), DESIGN.md §5:

    python tools/pose_eval_timing.py                 # device times + the numpy comparison, one JSON line each
    python tools/pose_eval_timing.py --device-only   # for a rocprofv3 --kernel-trace --stats run of its own

* pose_errors at batch 32 / 64 / 256, V = 6890, R = 17, J = 14 (gt vertices, so v2v too): HIP events around
  --iters back-to-back eager calls after a warm-up (Python included), and around replays of a graph that holds ten
  calls (the device time of one launch);
* reconstruction_error numpy in / numpy out on 35 515 bodies of 14 joints (a 3DPW test pass) next to a host numpy
  loop that restates the reference's (one np.linalg.svd per body, tuch/utils/pose_utils.py:28-92).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))

from tuch_amd.eval import pose_errors                          # noqa: E402
from tuch_amd.utils.pose_utils import reconstruction_error     # noqa: E402
import pose_eval_cases as pc                                   # noqa: E402


def host_loop(S1, S2):
    """The reference's per-body Procrustes, restated (numpy, one SVD per body)."""
    out = np.empty(S1.shape[0], S1.dtype)
    for i in range(S1.shape[0]):
        X1, X2 = S1[i].T, S2[i].T
        mu1, mu2 = X1.mean(1, keepdims=True), X2.mean(1, keepdims=True)
        A, Bm = X1 - mu1, X2 - mu2
        K = A @ Bm.T
        U, _, Vh = np.linalg.svd(K)
        Z = np.eye(3)
        Z[-1, -1] *= np.sign(np.linalg.det(U @ Vh))
        R = Vh.T @ Z @ U.T
        s = np.trace(R @ K) / np.sum(A ** 2)
        hat = s * R @ X1 + (mu2 - s * R @ mu1)
        out[i] = np.sqrt(((hat.T - S2[i]) ** 2).sum(-1)).mean()
    return out


def device_times(iters):
    dev = torch.device('cuda:0')
    pred, gt, reg, _ = pc.mesh_case(11, 256, 6890, 17, 14)
    pred, gt, reg = (torch.tensor(x, device=dev) for x in (pred, gt, reg))
    jmap = torch.tensor(pc.H36M_TO_J14, dtype=torch.int32, device=dev)
    for B in (32, 64, 256):
        p, g = pred[:B].contiguous(), gt[:B].contiguous()
        for _ in range(20):
            pose_errors(p, reg, jmap, gt_vertices=g)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            pose_errors(p, reg, jmap, gt_vertices=g)
        e1.record()
        torch.cuda.synchronize()
        eager = e0.elapsed_time(e1) / iters
        # device time without the Python side: 10 calls captured in one graph, replayed
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            pose_errors(p, reg, jmap, gt_vertices=g)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(10):
                pose_errors(p, reg, jmap, gt_vertices=g)
        graph.replay()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(iters // 10):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps({'what': 'pose_errors', 'batch': B, 'V': 6890, 'R': 17, 'J': 14, 'iters': iters,
                          'eager_ms_per_call': round(eager, 5),
                          'graph_ms_per_call': round(e0.elapsed_time(e1) / (iters // 10 * 10), 5)}), flush=True)


def numpy_times():
    rng = np.random.default_rng(0)
    n = 35515
    S1 = (rng.standard_normal((n, 14, 3)) * 0.3).astype(np.float32)
    S2 = (S1 * 1.1 + rng.standard_normal((n, 14, 3)) * 0.02).astype(np.float32)
    reconstruction_error(S1[:64], S2[:64], reduction=None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = reconstruction_error(S1, S2, reduction=None)
    t1 = time.perf_counter()
    host = host_loop(S1, S2)
    t2 = time.perf_counter()
    print(json.dumps({'what': 'reconstruction_error numpy in/out', 'bodies': n, 'device_s': round(t1 - t0, 5),
                      'host_loop_s': round(t2 - t1, 4), 'max_abs_diff': float(np.abs(dev - host).max())}), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--device-only', action='store_true')
    a = ap.parse_args()
    device_times(a.iters)
    if not a.device_only:
        numpy_times()
