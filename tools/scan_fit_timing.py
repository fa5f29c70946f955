#!/usr/bin/env python3
"""Timing of the fit to unregistered points (tuch_amd/fit.py: ScanFitter, csrc/scan_fit.hip) and of the hinted
closest-point search (csrc/closest_point.hip: tuch_closest_point with a hint), DESIGN.md §3:

    python tools/scan_fit_timing.py                 # all of it, one JSON line each
    python tools/scan_fit_timing.py --only search   # the search alone
    python tools/scan_fit_timing.py --only fit      # warm-up + ONE call of --iters replayed iterations: for a
                                                    # rocprofv3 --kernel-trace --stats run of its own (launches per iteration)
    python tools/scan_fit_timing.py --normals 60    # + the normal-compatible search and fit at that angle (degrees)

Batch 64 on the synthetic full body (V = 6890, F = 13776).  The scan of a body is the surface of that body at a random
pose + a translation: its vertices in vertex order (Q = 6890) and three points per face in face order (Q = 41 328).
* the search: the two consecutive states of a real fit -- the parameters before updates --at and --at + 1 of a ScanFitter
  run, one Adam step apart.  The mesh of the later state is searched unhinted and with the faces found on the earlier state
  as the hint (NOT the exact answer, which flatters); replays of a graph that holds the call, device events, --repeats
  blocks per version, the versions alternating, medians.  The share of hints that are not the answer, and the group visits
  per wavefront computed on the host side from the posed boxes and the answers: unhinted as closest_point_timing.py counts
  them (a lane's final d2 as its bound), hinted at most what a lane admits from its start (the nearest corner of the
  hinted face as its bound: an upper bound of that face's d2);
* the loop: device events around whole calls of --iters iterations, `ScanFitter` on a kept session (replays) with and
  without the hint, and the baseline -- what the package lets a user write without this module: SMPL(...) +
  closest_point + torch ops for rho + torch.optim.Adam(capturable=True), eager on the device.
* --normals ANGLE: the scan carries the true body's normals (area-weighted vertex normals for the vertex scan, the face's
  normal for the face samples, computed with torch).  On the same two states the oriented search
  (tuch_closest_point with normals) against the unoriented one, unhinted and hinted, the versions alternating; the share of
  matched points, the share of answers the filter changed, the group visits of both searches (the oriented ones: the box
  test under the lane's final d2 -- +inf for an unmatched lane -- and the group's normal cone, restated here, not proving
  the group inadmissible); `ScanFitter` per iteration with and without normals.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from closest_point_timing import MARGIN, group_visits, spread, timed      # noqa: E402
from synthetic import make_body, random_poses      # noqa: E402
from tuch_amd import _C, ops                       # noqa: E402
from tuch_amd.fit import ScanFitter                # noqa: E402
from tuch_amd.models.smpl import SMPL              # noqa: E402
from tuch_amd.ops import ContactModel              # noqa: E402

BATCH = 64


def graph_of(fn):
    """A graph that holds one call of fn (warmed up off the capture), and what the call returned."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        torch.cuda.current_stream().synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            kept = fn()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    return graph, kept


def scan_normals(model, true):
    """(vertex normals [B,V,3]: the area-weighted sum of the faces around every vertex, normalised; three copies of every
    face's unit normal [B,3F,3]) of the true bodies."""
    faces = model.faces_i32.long()
    tri = true[:, faces]
    m = torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1)           # twice the area, along the normal
    vn = torch.zeros_like(true)
    for k in range(3):
        vn.index_add_(1, faces[:, k], m)
    unit = lambda x: x / x.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    return unit(vn).contiguous(), unit(m)[:, :, None].expand(-1, -1, 3, -1).reshape(true.shape[0], -1, 3).contiguous()


CONE_MARGIN = 256.0 * 2.0 ** -24    # kCpConeMargin of csrc/closest_point.hip


def oriented_group_visits(model, verts, points, normals, d2, cosine):
    """group_visits for the oriented search: a group counts for a lane when its box is within the lane's final d2 AND its
    normal cone (the kernel's, restated) does not prove every face of it inadmissible for the lane's normal."""
    import numpy as np
    leaf = np.zeros(model.num_faces, np.int32)
    _C.check(_C.lib().tuch_contact_model_tree_order(model._handle, None, leaf.ctypes.data_as(_C.c_void_p)))
    dev = verts.device
    leaf_t = torch.as_tensor(leaf, device=dev).long()
    groups = int(leaf.max()) + 1
    size = torch.bincount(leaf_t, minlength=groups).float()
    faces = model.faces_i32.long()
    visits, tests = [], []
    dot = lambda a, b: (a * b).sum(-1)
    for b in range(0, verts.shape[0], 4):
        tri = verts[b:b + 4][:, faces]                                                          # [b,F,3,3]
        nb = tri.shape[0]
        m = torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1)
        u = m / m.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        axis = torch.zeros(nb, groups, 3, device=dev).index_add_(1, leaf_t, u)
        axis = axis / axis.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        cos_f = dot(axis[:, leaf_t], u)                                                         # [b,F]
        cb = torch.full((nb, groups), 2.0, device=dev).scatter_reduce(1, leaf_t[None].expand(nb, -1), cos_f, 'amin')
        sb = torch.sqrt((1.0 - cb * cb).clamp_min(0.0))
        idx = leaf_t[None, :, None].expand(nb, -1, 3)
        lo = torch.full((nb, groups, 3), float('inf'), device=dev)
        hi = -lo
        for k in range(3):
            lo = lo.scatter_reduce(1, idx, tri[:, :, k], 'amin')
            hi = hi.scatter_reduce(1, idx, tri[:, :, k], 'amax')
        p = points[b:b + 4][:, :, None]
        near = torch.maximum(torch.maximum(lo[:, None] - p, p - hi[:, None]), torch.zeros((), device=dev))
        far = torch.maximum(p - lo[:, None], hi[:, None] - p)
        admit = dot(near, near) - MARGIN * dot(far, far) <= d2[b:b + 4][:, :, None]              # [b,Q,G]
        n = normals[b:b + 4]
        n = n / n.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        ca = torch.einsum('bqc,bgc->bqg', n, axis)
        sa = torch.sqrt((1.0 - ca * ca).clamp_min(0.0))
        out = (ca < cb[:, None] - CONE_MARGIN) & (ca * cb[:, None] + sa * sb[:, None] <= cosine - CONE_MARGIN)
        admit = admit & ~out
        pad = (-admit.shape[1]) % 64
        if pad:
            admit = torch.cat([admit, torch.zeros(nb, pad, groups, dtype=torch.bool, device=dev)], 1)
        wave = admit.view(nb, -1, 64, groups).any(2)
        visits.append(wave.sum(2).float().flatten())
        tests.append((wave.float() * size).sum(2).flatten())
    return torch.cat(visits), torch.cat(tests), groups


def baseline_loop(smpl, model, points, global_orient, iters):
    """The loop as torch ops around the package's body model and closest_point ('distance', gradient 0 at d2 = 0)."""
    batch = points.shape[0]
    z = lambda n: torch.zeros(batch, n, device=points.device, requires_grad=True)
    body_pose, betas = z(69), z(10)
    with torch.no_grad():
        verts = smpl(global_orient=global_orient, body_pose=body_pose, betas=betas).vertices
        transl = (points.mean(1) - verts.mean(1)).clone()
    transl.requires_grad_(True)
    opt = torch.optim.Adam([body_pose, betas, transl], lr=1e-2, capturable=True)
    for _ in range(iters):
        opt.zero_grad()
        verts = smpl(global_orient=global_orient, body_pose=body_pose, betas=betas).vertices
        d2 = model.closest_point(verts, points - transl[:, None]).d2
        on = d2 > 0
        loss = torch.where(on, torch.sqrt(torch.where(on, d2, torch.ones_like(d2))), torch.zeros_like(d2)).mean(1).sum()
        loss.backward()
        opt.step()
    return body_pose, betas, transl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10, help='search calls per timed block')
    ap.add_argument('--at', type=int, default=10, help='the search is timed on the fit\'s states before updates AT and AT + 1')
    ap.add_argument('--only', choices=('fit', 'search'), default=None)
    ap.add_argument('--normals', type=float, default=None, metavar='ANGLE',
                    help='also the normal-compatible search and fit, at this max angle in degrees')
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
        vertex_normals, face_normals = scan_normals(model, true) if a.normals is not None else (None, None)
    scans = {'Q=6890 vertex order': true.contiguous(), 'Q=41328 face order': hd}
    normals_of = {'Q=6890 vertex order': vertex_normals, 'Q=41328 face order': face_normals}
    if a.only != 'fit':
        for name, points in scans.items():
            probe = ScanFitter(smpl, model, num_iters=a.at + 2, fit_global_orient=False, use_graph=False, record_history=True)
            probe(points, go)
            states = [probe.history['fit'][i]['params'] for i in (a.at, a.at + 1)]
            with torch.no_grad():
                verts = [smpl(global_orient=go, body_pose=s[0], betas=s[1]).vertices.contiguous() for s in states]
                queries = [(points - s[2][:, None]).contiguous() for s in states]
                earlier = model.closest_point(verts[0], queries[0])
                graphs = {'unhinted': graph_of(lambda: model.closest_point(verts[1], queries[1]))}
                graphs['hinted'] = graph_of(lambda: model.closest_point(verts[1], queries[1], hint=earlier.face))
                for x, y in zip(graphs['unhinted'][1], graphs['hinted'][1]):
                    assert torch.equal(x, y)
                if a.normals is not None:
                    nrm = normals_of[name]
                    oriented = lambda v, q, **kw: model.closest_point(v, q, normals=nrm, max_angle=a.normals, **kw)
                    earlier_oriented = oriented(verts[0], queries[0])
                    graphs['oriented unhinted'] = graph_of(lambda: oriented(verts[1], queries[1]))
                    graphs['oriented hinted'] = graph_of(lambda: oriented(verts[1], queries[1], hint=earlier_oriented.face))
                    for x, y in zip(graphs['oriented unhinted'][1], graphs['oriented hinted'][1]):
                        assert torch.equal(x, y)
            t = {k: [] for k in graphs}
            for _ in range(a.repeats):
                for k, (graph, _) in graphs.items():
                    t[k].append(timed(lambda: [graph.replay() for _ in range(a.calls)]) / a.calls)
            for k, ms in t.items():
                print(json.dumps(dict({'what': 'closest_point %s, replayed, %s' % (k, name), 'batch': BATCH, 'calls': a.calls,
                                       'repeats': a.repeats}, **spread(ms))), flush=True)
            with torch.no_grad():
                answer = graphs['unhinted'][1]
                stale = float((earlier.face != answer.face).float().mean())
                visits, tests, groups = group_visits(model, verts[1], queries[1], answer.d2)
                line = {'what': 'group visits per wavefront, ' + name, 'groups': groups, 'hints_not_the_answer': round(stale, 4),
                        'unhinted_mean': round(float(visits.mean()), 2), 'unhinted_tests_mean': round(float(tests.mean()), 1)}
                # A hinted lane's bound from the start is the hinted face's d2 on the later mesh and only shrinks; the
                # nearest of that face's three corners bounds it from above without any triangle code, so these counts
                # are what the hinted walk visits AT MOST (sweep 1's box test of every group per lane is gone besides).
                corners = torch.stack([verts[1][b][faces[earlier.face[b].long()]] for b in range(BATCH)])      # [B,Q,3,3]
                corner = ((queries[1][:, :, None] - corners) ** 2).sum(-1).min(2).values
                hv, ht, _ = group_visits(model, verts[1], queries[1], torch.maximum(corner, answer.d2))
                line.update(hinted_start_mean_at_most=round(float(hv.mean()), 2),
                            hinted_start_tests_mean_at_most=round(float(ht.mean()), 1))
                print(json.dumps(line), flush=True)
                if a.normals is not None:
                    found = graphs['oriented unhinted'][1]
                    cosine = ops.args.max_angle_cos(nrm, a.normals, queries[1], 'scan_fit_timing')
                    ov, ot, _ = oriented_group_visits(model, verts[1], queries[1], nrm, found.d2, cosine)
                    print(json.dumps({'what': 'oriented search at %g degrees, %s' % (a.normals, name),
                                      'matched': round(float((found.face >= 0).float().mean()), 5),
                                      'answers_the_filter_changed': round(float((found.face != answer.face).float().mean()), 5),
                                      'hints_not_the_answer': round(float((earlier_oriented.face != found.face).float().mean()), 4),
                                      'group_visits_mean': round(float(ov.mean()), 2), 'tests_mean': round(float(ot.mean()), 1),
                                      'unoriented_group_visits_mean': round(float(visits.mean()), 2),
                                      'unoriented_tests_mean': round(float(tests.mean()), 1)}), flush=True)
        if a.only == 'search':
            return
    points = scans['Q=6890 vertex order']
    fitter = ScanFitter(smpl, model, num_iters=a.iters, fit_global_orient=False, use_hint=True)
    fit = fitter(points, go)                     # three eager iterations, the capture, iters - 3 replays
    torch.cuda.synchronize()
    if a.only == 'fit':
        ms = timed(lambda: fitter(points, go))
        print(json.dumps({'what': 'ScanFitter(use_hint=True), kept session', 'iters': a.iters, 'replayed': fitter.graph_replayed,
                          'ms_per_iter': round(ms / a.iters, 5)}), flush=True)
        return
    plain = ScanFitter(smpl, model, num_iters=a.iters, fit_global_orient=False, use_hint=False)
    plain(points, go)
    if a.normals is not None:
        with_normals = ScanFitter(smpl, model, num_iters=a.iters, fit_global_orient=False, use_hint=True,
                                  max_normal_angle=a.normals)
        fit_normals = with_normals(points, go, normals=vertex_normals)
    base_iters = max(a.iters // 5, 10)
    baseline_loop(smpl, model, points, go, 5)
    torch.cuda.synchronize()
    t = {'hint': [], 'plain': [], 'baseline': []}
    if a.normals is not None:
        t['normals'] = []
    for _ in range(a.repeats):
        t['hint'].append(timed(lambda: fitter(points, go)) / a.iters)
        if a.normals is not None:
            t['normals'].append(timed(lambda: with_normals(points, go, normals=vertex_normals)) / a.iters)
        t['plain'].append(timed(lambda: plain(points, go)) / a.iters)
        t['baseline'].append(timed(lambda: baseline_loop(smpl, model, points, go, base_iters)) / base_iters)
    for name, what in (('hint', 'ScanFitter(use_hint=True), kept session (replays)'),
                       ('normals', 'ScanFitter(use_hint=True, max_normal_angle=%s) with normals, kept session (replays)' % a.normals),
                       ('plain', 'ScanFitter(use_hint=False), kept session (replays)'),
                       ('baseline', 'SMPL + closest_point + torch ops + torch.optim.Adam(capturable), eager')):
        if name not in t:
            continue
        print(json.dumps(dict({'what': what, 'batch': BATCH, 'Q': 6890, 'iters': a.iters if name != 'baseline' else base_iters,
                               'repeats': a.repeats}, **spread(t[name]))), flush=True)
    start = ScanFitter(smpl, model, num_iters=0, fit_global_orient=False)(points, go)
    print(json.dumps({'what': 'final / initial loss after %d iterations (largest body)' % a.iters,
                      'value': float((fit.loss / start.loss).max())}), flush=True)
    if a.normals is not None:
        print(json.dumps({'what': 'with normals: final / initial loss after %d iterations (largest body)' % a.iters,
                          'value': float((fit_normals.loss / start.loss).max()),
                          'matched_at_the_end': round(float((fit_normals.face >= 0).float().mean()), 5)}), flush=True)


if __name__ == '__main__':
    main()
