"""Seeded inputs of the pose-evaluation tests, shared by tests/golden/make_golden_pose_eval.py (which stores only the
seeds and the expected results) and tests/test_gpu_pose_eval.py (which regenerates the inputs from the seeds)."""
from __future__ import annotations

import numpy as np

# SPIN's constants.H36M_TO_J17 / H36M_TO_J14 (the joint maps eval.py uses)
H36M_TO_J17 = [6, 5, 4, 1, 2, 3, 16, 15, 14, 11, 12, 13, 8, 10, 0, 7, 9]
H36M_TO_J14 = H36M_TO_J17[:14]

# (name, seed, B, V, R, joint map, ground truth: 'vertices' or 'joints')
MESH_CASES = [
    ('h36m_j14_v6890', 11, 64, 6890, 17, H36M_TO_J14, 'vertices'),
    ('h36m_j17_v6890_gtjoints', 12, 16, 6890, 17, H36M_TO_J17, 'joints'),
    ('r24_j14_v1000', 13, 9, 1000, 24, H36M_TO_J14, 'vertices'),
]


def random_rotation(rng, d=3):
    q, r = np.linalg.qr(rng.standard_normal((d, d)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def mesh_case(seed, B, V, R, J):
    """pred_vertices, gt_vertices [B,V,3] and gt_joints [B,J,3] float32 (metres, body-sized), a dense signed regressor
    [R,V] float32 whose rows sum to 1 (negative entries included)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((V, 3)) * np.array([0.25, 0.6, 0.15])
    gt = np.empty((B, V, 3))
    pred = np.empty((B, V, 3))
    for b in range(B):
        g = base + rng.standard_normal((V, 3)) * 0.03
        gt[b] = g @ random_rotation(rng).T + rng.uniform(-1, 1, 3)
        p = (g + rng.standard_normal((V, 3)) * 0.02) * rng.uniform(0.9, 1.1)
        pred[b] = p @ random_rotation(rng).T + rng.uniform(-1, 1, 3)
    # every entry non-zero: a small signed background plus 40 vertices around a seed vertex per joint
    reg = rng.uniform(-1.0, 1.0, (R, V)) * (0.05 / V)
    for r in range(R):
        near = np.argsort(((base - base[rng.integers(V)]) ** 2).sum(1))[:40]
        reg[r, near] += rng.uniform(0.2, 1.0, 40)
    reg /= reg.sum(1, keepdims=True)
    gt_joints = rng.standard_normal((B, J, 3)) * 0.3
    return pred.astype(np.float32), gt.astype(np.float32), reg.astype(np.float32), gt_joints.astype(np.float32)


def mesh_expected(pred, gt, reg, jmap, gt_joints, recon_error):
    """eval.py:172-194 in float64 on the float32 inputs; recon_error: the reference's reconstruction_error."""
    p = pred.astype(np.float64)
    r = reg.astype(np.float64)
    pj = np.einsum('rv,bvc->brc', r, p)
    pk = pj[:, jmap] - pj[:, [0]]
    if gt_joints is None:
        gj = np.einsum('rv,bvc->brc', r, gt.astype(np.float64))
        gk = gj[:, jmap] - gj[:, [0]]
        v2v = np.sqrt(((p - gt.astype(np.float64)) ** 2).sum(-1)).mean(-1)
    else:
        gk = gt_joints.astype(np.float64)
        v2v = None
    mpjpe = np.sqrt(((pk - gk) ** 2).sum(-1)).mean(-1)
    pa = recon_error(pk, gk, reduction=None)
    return mpjpe, pa, v2v, pj
