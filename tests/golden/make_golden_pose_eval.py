#!/usr/bin/env python3
"""Golden vectors for the pose evaluation (tuch_amd.utils.pose_utils, tuch_amd.eval), produced by the REFERENCE's own
functions (tuch/utils/pose_utils.py, imported, never copied; it needs numpy only) on synthetic inputs:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pose_eval.py /path/to/reference/checkout

Writes tests/golden/pose_eval.npz:
  * joint sets  <case>_S1, <case>_S2 (the inputs), <case>_hat (compute_similarity_transform_batch),
    <case>_re (reconstruction_error(..., None)), <case>_re_mean, <case>_re_sum;
  * mesh cases  mesh_<name>_{mpjpe,pa_mpjpe,v2v,joints}: eval.py's numbers in float64 on inputs that
    tests/pose_eval_cases.py regenerates from the seeds listed there (the inputs themselves are not stored).
Left out on purpose: "S2 collinear, S1 not" -- the rotation is not unique there and the reference returns LAPACK's pick.
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
if len(sys.argv) != 2:
    sys.exit('usage: make_golden_pose_eval.py <reference checkout (the directory that holds tuch/)>')
sys.path.insert(1, os.path.abspath(sys.argv[1]))

import numpy as np                                          # noqa: E402

from tuch.utils import pose_utils as ref                    # noqa: E402
import pose_eval_cases as pc                                # noqa: E402

rng = np.random.default_rng(2024)


def similar(S1, mirror=False, noise=0.01, d=3):
    """S2 = s R S1 + t + noise per body ([B, N, d] points-first)."""
    out = np.empty_like(S1)
    for b in range(S1.shape[0]):
        R = pc.random_rotation(rng, d)
        if mirror:
            R[:, 0] = -R[:, 0]
        out[b] = rng.uniform(0.5, 2.0) * S1[b] @ R.T + rng.uniform(-1, 1, d) + rng.standard_normal(S1[b].shape) * noise
    return out


cases = {}
S1 = rng.standard_normal((64, 14, 3)) * 0.3
cases['j14_f64'] = (S1, similar(S1))
S1 = rng.standard_normal((64, 14, 3)) * 0.3
cases['j14_f32'] = (S1.astype(np.float32), similar(S1).astype(np.float32))
S1 = rng.standard_normal((16, 14, 3)) * 0.3
cases['mirror'] = (S1, similar(S1, mirror=True))
S1 = rng.standard_normal((16, 14, 3)) * 0.3
cases['mirror_f32'] = (S1.astype(np.float32), similar(S1, mirror=True).astype(np.float32))
P = rng.standard_normal((16, 14, 3)) * 0.3
P[:, :, 2] = 0
S1 = np.stack([p @ pc.random_rotation(rng).T for p in P])
cases['coplanar'] = (S1, similar(S1))
cases['coplanar_exact'] = (S1, similar(S1, noise=0.0))
line = rng.standard_normal((8, 14, 1)) * np.array([0.3, -0.1, 0.2]) + rng.uniform(-1, 1, (8, 1, 3))
cases['collinear_s1'] = (line, rng.standard_normal((8, 14, 3)) * 0.3)
S1 = rng.standard_normal((32, 17, 3)) * 0.3
cases['n17'] = (S1, similar(S1))
S1 = rng.standard_normal((16, 3, 3)) * 0.3                  # [B,3,3]: read as coordinates x points
cases['n3'] = (S1, similar(S1.transpose(0, 2, 1)).transpose(0, 2, 1).copy())
S1 = rng.standard_normal((16, 3, 14)) * 0.3                 # [B,3,14]: coordinates x points
cases['t3x14'] = (S1, similar(S1.transpose(0, 2, 1)).transpose(0, 2, 1).copy())
S1 = rng.standard_normal((16, 14, 2)) * 0.3
cases['d2'] = (S1, similar(S1, d=2))
cases['d2_mirror'] = (S1, similar(S1, mirror=True, d=2))
S1 = rng.standard_normal((16, 2, 14)) * 0.3                 # [B,2,14]: coordinates x points
cases['d2t'] = (S1, similar(S1.transpose(0, 2, 1), d=2).transpose(0, 2, 1).copy())
S1 = rng.standard_normal((2, 1000, 3)) * 0.3
cases['n1000'] = (S1, similar(S1))
S1 = np.repeat(rng.integers(-8, 8, (4, 1, 3)) / 4.0, 14, axis=1)  # all points of S1 equal (exact mean): NaN
cases['nan'] = (S1, rng.standard_normal((4, 14, 3)))

out = {'joint_cases': np.asarray(sorted(cases))}
with warnings.catch_warnings():
    warnings.simplefilter('ignore', RuntimeWarning)          # 0 / 0 of the NaN case
    for name, (a, b) in cases.items():
        out[name + '_S1'], out[name + '_S2'] = a, b
        out[name + '_hat'] = ref.compute_similarity_transform_batch(a, b)
        out[name + '_re'] = ref.reconstruction_error(a, b, reduction=None)
        out[name + '_re_mean'] = np.asarray(ref.reconstruction_error(a, b, reduction='mean'))
        out[name + '_re_sum'] = np.asarray(ref.reconstruction_error(a, b, reduction='sum'))
    out['single_hat'] = ref.compute_similarity_transform(cases['j14_f32'][0][0], cases['j14_f32'][1][0])
    out['single_t_hat'] = ref.compute_similarity_transform(cases['t3x14'][0][0], cases['t3x14'][1][0])

for name, seed, B, V, R, jmap, gt_kind in pc.MESH_CASES:
    pred, gt, reg, gt_joints = pc.mesh_case(seed, B, V, R, len(jmap))
    mpjpe, pa, v2v, pj = pc.mesh_expected(pred, gt, reg, jmap, gt_joints if gt_kind == 'joints' else None,
                                          ref.reconstruction_error)
    out['mesh_%s_mpjpe' % name], out['mesh_%s_pa_mpjpe' % name], out['mesh_%s_joints' % name] = mpjpe, pa, pj
    if v2v is not None:
        out['mesh_%s_v2v' % name] = v2v

path = os.path.join(HERE, 'pose_eval.npz')
np.savez_compressed(path, **out)
print('wrote', path, os.path.getsize(path), 'bytes')
