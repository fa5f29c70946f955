"""Inputs and float64 references shared by the SMPL forward/backward tests (tests/test_oracle_lbs.py on the CPU,
tests/test_gpu_lbs.py on the device).  No GPU here.

The kernels of csrc/smpl_lbs.hip change form with the batch size alone (blend_kernel<1> / <2> / blend_ksplit_kernel,
blend_bwd_kernel<1> / <2> / <4>), not with the number of vertices: a 362-vertex body at every batch form costs a float64
autograd oracle a fraction of a second.  The poses put the edges of Rodrigues' formula (0, next to 0, next to pi,
beyond pi) on the rows where a ragged 16-body group or 64-row block goes wrong: the first rows, 15 | 16, 31 | 32 and
the last three."""
from __future__ import annotations

import functools

import numpy as np
import torch

import helpers
from oracle import lbs as ol
from synthetic import make_body, random_poses

# every batch form of the forward and the backward blend, full and ragged: 1 / 2 body tiles per wavefront, the K-split
# form with one full 64-row block (64), a ragged one (33, 48) and two blocks (65); 1 / 2 / 4 sixteen-body groups per
# workgroup of the blend adjoint with the last group full (16, 32, 48, 64) and holding one body (17, 33, 65)
BATCHES = (1, 16, 17, 32, 33, 48, 64, 65)

CLASSES = ('rest', 'tiny', 'small', 'near_pi', 'beyond_pi', 'mixed_zero')
ANGLE = {'tiny': 1e-4, 'small': 1e-2, 'near_pi': np.pi - 1e-3, 'beyond_pi': 4.0}
TAIL = ('rest', 'near_pi', 'mixed_zero')            # second copies on the last three rows
SEAMS = {15: 'near_pi', 16: 'rest', 31: 'mixed_zero', 32: 'beyond_pi'}   # last / first row of a 16-body group, a 32-row tile

# the project's bounds of the LBS tests (tests/test_gpu_lbs.py)
FWD_RTOL, FWD_ATOL = 1e-4, 5e-6
GRAD_FLOOR, GRAD_RTOL = 2e-5, helpers.GRAD_RTOL
GV_SEED, POSE_SEED = 5, 33


@functools.lru_cache(maxsize=None)
def ico6_body():
    """V = 362: two skinning-adjoint blocks, the second ragged; 3V = 1086: five 256-column chunks of the blend adjoint,
    the last ragged; at most 4 weights per vertex: the sparse skinning kernels."""
    body = make_body(topology='ico', freq=6, with_geodesics=False)
    assert body.num_verts == 362 and int((body.lbs_weights != 0).sum(1).max()) <= 4
    return body


def _class_pose(name, rng, random_row):
    """One body's [24,3] axis-angle pose of the class: a random unit axis per joint times the class's angle."""
    if name == 'rest':
        return np.zeros((24, 3))
    if name == 'mixed_zero':
        pose = np.array(random_row, np.float64).reshape(24, 3)
        pose[::2] = 0.0
        return pose
    axis = rng.standard_normal((24, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    return axis * ANGLE[name]


def edge_poses(batch: int, seed: int):
    """(full_pose [B,72] float32, betas [B,10] float32, class of every row).  random_poses with whole bodies replaced:
    the six classes on the first rows (as many as fit), copies on rows 15 | 16 (B > 16) and 31 | 32 (B > 32), and
    rest / near_pi / mixed_zero once more on the last three rows (where they do not displace a first-row class).
    Every other row stays 'random'."""
    bp, go, be = random_poses(batch, seed)
    full = np.concatenate([go, bp], 1).astype(np.float64)
    rng = np.random.default_rng(seed + 1000)
    rows = {}
    if batch > 16:
        rows.update({r: SEAMS[r] for r in (15, 16)})
    if batch > 32:
        rows.update({r: SEAMS[r] for r in (31, 32)})
    for i, name in enumerate(TAIL):
        rows[batch - 3 + i] = name
    for r, name in enumerate(CLASSES):
        rows[r] = name
    classes = ['random'] * batch
    for r in sorted(rows):
        if 0 <= r < batch:
            full[r] = _class_pose(rows[r], rng, full[r]).reshape(72)
            classes[r] = rows[r]
    return full.astype(np.float32), be, classes


def upstream(batch: int, num_verts: int, seed: int = GV_SEED):
    """Standard normal g_verts [B,V,3] and g_joints [B,49,3], float32."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((batch, num_verts, 3)).astype(np.float32),
            rng.standard_normal((batch, 49, 3)).astype(np.float32))


def rotmats(full_pose):
    """[B,24,3,3] float64: the oracle's Rodrigues of the float32 pose (what pose2rot=False runs are fed, cast to float32)."""
    full64 = torch.as_tensor(np.asarray(full_pose), dtype=torch.float64)
    return ol.rodrigues(full64.reshape(-1, 3)).reshape(full64.shape[0], 24, 3, 3)


def reference(body, full_pose, betas, gv, gj, pose2rot, dtype=torch.float64):
    """The oracle's forward and autograd backward in `dtype`: smplx lbs, the picked and the regressed joints, the joint
    map; the objective is sum(verts * gv) + sum(joints * gj), gv or gj may be None.
    Returns numpy (verts [B,V,3], joints [B,49,3], g_pose [B,72] or [B,216], g_betas [B,10])."""
    m = ol.model_tensors(body, dtype)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    batch = len(betas)
    be = t(betas).clone().requires_grad_(True)
    if pose2rot:
        pose = t(full_pose).clone().requires_grad_(True)
    else:
        pose = rotmats(full_pose).to(dtype).clone().requires_grad_(True)
    v, j = ol.lbs(be, pose, m, pose2rot=pose2rot)
    picked = v[:, m['extra_vertex_ids']]
    extra = torch.einsum('bvk,jv->bjk', v, m['J_regressor_extra'])
    joints = torch.cat([j, picked, extra], 1)[:, m['joint_map']]
    loss = 0
    if gv is not None:
        loss = loss + (v * t(gv)).sum()
    if gj is not None:
        loss = loss + (joints * t(gj)).sum()
    loss.backward()
    return (v.detach().numpy(), joints.detach().numpy(), pose.grad.reshape(batch, -1).numpy(), be.grad.numpy())


@functools.lru_cache(maxsize=None)
def edge_case(batch: int, pose2rot: bool, which: str = 'both', dtype=torch.float64):
    """The ico-6 body with edge_poses at this batch size, computed once per process and shared (treat as read-only):
    dict of full_pose, betas, classes, gv, gj (the one `which` leaves out is None) and ref = reference(...)."""
    body = ico6_body()
    full, be, classes = edge_poses(batch, POSE_SEED)
    gv, gj = upstream(batch, body.num_verts)
    gv, gj = (gv if which != 'joints' else None), (gj if which != 'verts' else None)
    ref = reference(body, full, be, gv, gj, pose2rot, dtype)
    for a in (full, be, gv, gj) + ref:
        if a is not None:
            a.setflags(write=False)
    return dict(full_pose=full, betas=be, classes=classes, gv=gv, gj=gj, ref=ref)


def body_ratio(actual, expected, floor, rtol=GRAD_RTOL):
    """Per body: (max |err| / that body's max |expected|, max |err| / bound), the bound being helpers.grad_close's with
    the BODY's own maximum as the scale: rtol |expected| + floor[b] * max_b |expected|."""
    a = np.asarray(actual, np.float64).reshape(len(actual), -1)
    e = np.asarray(expected, np.float64).reshape(len(expected), -1)
    scale = np.abs(e).max(1)
    err = np.abs(a - e)
    bound = rtol * np.abs(e) + (np.asarray(floor, np.float64) * scale)[:, None]
    return err.max(1) / np.maximum(scale, 1e-300), (err / np.maximum(bound, 1e-300)).max(1)


def e_tiny(batch: int, which: str = 'both'):
    """{row: error of the FLOAT32 oracle's pose gradient on a body of class 'tiny' with pose2rot=True, relative to that
    body's largest float64 entry}.  float32's cos(1e-4) is within an ulp of 1, so the (1 - cos t) / t term of the
    Rodrigues adjoint carries a relative error of about t / 2 there: the reference's own formula in float32, not a
    kernel -- the device test takes its floor for these bodies from this number (same batch, same objective: `which`)."""
    c64, c32 = edge_case(batch, True, which), edge_case(batch, True, which, torch.float32)
    rel, _ = body_ratio(c32['ref'][2], c64['ref'][2], GRAD_FLOOR)
    return {r: float(rel[r]) for r, name in enumerate(c64['classes']) if name == 'tiny'}


def grad_floors(batch: int, pose2rot: bool, classes, which: str = 'both'):
    """Floor of the pose gradient per body: GRAD_FLOOR, and for 'tiny' bodies under pose2rot max(GRAD_FLOOR, 4 e_tiny):
    HIP's cosf may sit 1-2 ulp from the correctly rounded value and e_tiny is half an ulp of cos t, so the error of
    1 - cos t can be 2-4 times the reference's and no more."""
    floors = np.full(len(classes), GRAD_FLOOR)
    if pose2rot:
        for r, e in e_tiny(batch, which).items():
            floors[r] = max(GRAD_FLOOR, 4.0 * e)
    return floors


def grad_close_per_body(actual, expected, floors, classes, what, rtol=GRAD_RTOL):
    """helpers.grad_close for every body with the body's own maximum as the scale (one wrong body is not hidden behind
    the others' magnitudes).  Logs the worst body of every pose class, then asserts all of them."""
    floors = np.broadcast_to(np.asarray(floors, np.float64), (len(actual),))
    rel, ratio = body_ratio(actual, expected, floors, rtol)
    for name in sorted(set(classes)):
        rows = [r for r, c in enumerate(classes) if c == name]
        worst = max(rows, key=lambda r: ratio[r])
        helpers._log('grad %-60s max|err|/max|ref| %.2e   max err/bound %.3f   (body %d)'
                     % ('%s [%s]' % (what, name), rel[rows].max(), ratio[worst], worst))
    a = np.asarray(actual, np.float64).reshape(len(actual), -1)
    e = np.asarray(expected, np.float64).reshape(len(expected), -1)
    for b in range(len(a)):
        helpers.assert_close(a[b], e[b], rtol, floors[b] * np.abs(e[b]).max(), '%s body %d [%s]' % (what, b, classes[b]))


def forward_close_per_class(actual, expected, classes, what):
    """The forward bound (1e-4 relative + 5e-6) on every entry, the worst body of every pose class logged first."""
    a = np.asarray(actual, np.float64).reshape(len(actual), -1)
    e = np.asarray(expected, np.float64).reshape(len(expected), -1)
    err = np.abs(a - e)
    ratio = (err / (FWD_ATOL + FWD_RTOL * np.abs(e))).max(1)
    rel = err.max(1) / np.abs(e).max(1)
    for name in sorted(set(classes)):
        rows = [r for r, c in enumerate(classes) if c == name]
        worst = max(rows, key=lambda r: ratio[r])
        helpers._log('loop %-64s max|err|/max|ref| %.2e   max err/bound %.3f   (body %d)'
                     % ('%s [%s]' % (what, name), rel[rows].max(), ratio[worst], worst))
    helpers.assert_close(actual, expected, FWD_RTOL, FWD_ATOL, what)
