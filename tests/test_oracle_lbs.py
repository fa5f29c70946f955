"""CPU: known-answer tests of the SMPL LBS oracle.  The reference delegates this arithmetic to
smplx==0.1.13, which is absent (parity unpinned, see oracle/lbs.py); the oracle is therefore
checked against mathematics, not against reference outputs."""
import numpy as np
import pytest
import torch

from helpers import assert_close
from oracle import lbs as ol
from synthetic import make_body, random_poses


@pytest.fixture(scope='module')
def body():
    return make_body(12, 14, with_geodesics=False)


def test_zero_pose_is_shape_blend_only(body):
    m = ol.model_tensors(body)
    betas = torch.tensor(random_poses(2, 3)[2])
    v, j = ol.lbs(betas, torch.zeros(2, 72), m)
    want = m['v_template'][None] + torch.einsum('bl,vkl->bvk', betas, m['shapedirs'])
    assert_close(v.numpy(), want.numpy(), 0, 2e-6, 'zero-pose verts')
    assert_close(j.numpy(), torch.einsum('bvk,jv->bjk', want, m['J_regressor']).numpy(), 0, 2e-6, 'joints')


def test_root_rotation_is_rigid(body):
    m = ol.model_tensors(body, torch.float64)
    betas = torch.tensor(random_poses(1, 4)[2], dtype=torch.float64)
    pose = torch.zeros(1, 72, dtype=torch.float64)
    v0, j0 = ol.lbs(betas, pose, m)
    pose[0, :3] = torch.tensor([0.3, -0.5, 0.2])
    v1, j1 = ol.lbs(betas, pose, m)
    rot = ol.rodrigues(pose[:, :3])[0]
    root = j0[0, 0]
    assert_close(v1[0].numpy(), ((v0[0] - root) @ rot.T + root).numpy(), 0, 1e-9, 'rigid verts')
    assert_close(torch.det(rot).item(), 1.0, 0, 1e-12, 'det')


def test_float32_tracks_float64(body):
    bp, go, be = random_poses(3, 7)
    out32 = ol.smpl_forward(ol.model_tensors(body), torch.tensor(be), torch.tensor(bp), torch.tensor(go))
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    out64 = ol.smpl_forward(ol.model_tensors(body, torch.float64), t64(be), t64(bp), t64(go))
    assert_close(out32[0].numpy(), out64[0].numpy(), 1e-5, 2e-6, 'verts')
    assert_close(out32[1].numpy(), out64[1].numpy(), 1e-5, 2e-6, 'joints')
    assert out32[1].shape == (3, 49, 3)


def test_rotmat_input_equals_axis_angle_input(body):
    m = ol.model_tensors(body, torch.float64)
    bp, go, be = [torch.tensor(a, dtype=torch.float64) for a in random_poses(2, 9)]
    full = torch.cat([go, bp], 1)
    va, ja = ol.lbs(be, full, m, pose2rot=True)
    rot = ol.rodrigues(full.reshape(-1, 3)).reshape(2, 24, 3, 3)
    vr, jr = ol.lbs(be, rot, m, pose2rot=False)
    assert_close(va.numpy(), vr.numpy(), 0, 1e-12, 'verts')


def test_autograd_matches_finite_differences(body):
    m = ol.model_tensors(body, torch.float64)
    bp, go, be = [torch.tensor(a, dtype=torch.float64) for a in random_poses(1, 11)]
    w = torch.tensor(np.random.default_rng(0).standard_normal((1, body.num_verts, 3)))

    def f(bp_, be_):
        v, j = ol.smpl_forward(m, be_, bp_, go)
        return (v * w).sum() + j.sum()
    bp_ = bp.clone().requires_grad_(True)
    be_ = be.clone().requires_grad_(True)
    f(bp_, be_).backward()
    for idx in (0, 17, 44, 68):
        e = torch.zeros_like(bp)
        e[0, idx] = 1e-6
        fd = (f(bp + e, be) - f(bp - e, be)) / 2e-6
        assert_close(bp_.grad[0, idx].item(), fd.item(), 1e-5, 1e-7, 'd/dpose')
    for idx in (0, 9):
        e = torch.zeros_like(be)
        e[0, idx] = 1e-6
        fd = (f(bp, be + e) - f(bp, be - e)) / 2e-6
        assert_close(be_.grad[0, idx].item(), fd.item(), 1e-5, 1e-7, 'd/dbeta')


@pytest.mark.parametrize('pose2rot', [True, False])
def test_float32_oracle_tracks_float64_per_body_on_the_edge_poses(pose2rot):
    """The premise of the device tests (tests/test_gpu_lbs.py): on the 362-vertex body, with rest / tiny / small /
    near-pi / beyond-pi / every-other-joint-zero poses on the first, seam and last rows of a batch of 65, the float32
    oracle stays far inside the LBS bounds PER BODY (scale = that body's own largest float64 entry) -- so a kernel that
    exceeds them is wrong, not merely float32.  Measured: verts and joints <= 4.7e-7 of the maximum, g_betas <= 6.3e-7 and
    g_pose <= 8.8e-7 of the body's maximum, EXCEPT g_pose of the 'tiny' class (every joint at 1e-4 rad) under pose2rot:
    3.5e-5, float32's 1 - cos(t) next to t = 0 in the reference's own formula.  Nothing fixed is asserted of that body: its
    error is lbs_cases.e_tiny(), which the device test takes its floor from."""
    import lbs_cases as lc
    from helpers import report_value
    batch = 65
    c64, c32 = lc.edge_case(batch, pose2rot), lc.edge_case(batch, pose2rot, 'both', torch.float32)
    classes = c64['classes']
    assert set(classes) == set(lc.CLASSES) | {'random'}
    assert [classes[r] for r in (0, 1, 15, 16, 31, 32, 62, 63, 64)] == [
        'rest', 'tiny', 'near_pi', 'rest', 'mixed_zero', 'beyond_pi', 'rest', 'near_pi', 'mixed_zero']
    v32, j32, gp32, gb32 = c32['ref']
    v64, j64, gp64, gb64 = c64['ref']
    what = 'oracle f32 vs f64 ico6 B=%d pose2rot=%s' % (batch, pose2rot)
    lc.forward_close_per_class(v32, v64, classes, what + ' verts')
    lc.forward_close_per_class(j32, j64, classes, what + ' joints')
    lc.grad_close_per_body(gb32, gb64, lc.GRAD_FLOOR, classes, what + ' grad betas')
    # the 'tiny' bodies under pose2rot: whatever the float32 formula gives (reported); everywhere else the project's bound
    tiny = lc.e_tiny(batch) if pose2rot else {}
    floors = np.full(batch, lc.GRAD_FLOOR)
    for r, e in tiny.items():
        report_value(what + ' e_tiny (body %d)' % r, e)
        assert np.isfinite(e)
        floors[r] = np.inf
    assert sorted(tiny) == ([1] if pose2rot else [])
    lc.grad_close_per_body(gp32, gp64, floors, classes, what + ' grad pose')
    # more than 20x room everywhere else
    _, ratio = lc.body_ratio(gp32, gp64, floors)
    assert ratio.max() < 0.05, ratio.max()


def test_edge_poses_places_the_classes_on_the_seams():
    import lbs_cases as lc
    for batch in (1, 5, 8, 9, 16, 17, 33, 65):
        full, be, classes = lc.edge_poses(batch, 3)
        assert full.shape == (batch, 72) and full.dtype == np.float32 and be.shape == (batch, 10) and len(classes) == batch
        assert classes[:6] == list(lc.CLASSES)[:batch]
        if batch >= 9:
            assert classes[-3:] == list(lc.TAIL)
        ang = np.linalg.norm(full.reshape(batch, 24, 3).astype(np.float64), axis=2)
        for r, name in enumerate(classes):
            if name in lc.ANGLE:
                assert np.allclose(ang[r], lc.ANGLE[name], rtol=1e-6, atol=0), (batch, r, name)
            elif name == 'rest':
                assert not full[r].any()
            elif name == 'mixed_zero':
                assert not ang[r, ::2].any() and ang[r, 1::2].all()
    assert lc.edge_poses(33, 3)[2][15:17] == ['near_pi', 'rest'] and lc.edge_poses(17, 3)[2][14:] == list(lc.TAIL)
