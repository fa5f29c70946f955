"""Drop-in for the reference's ``tuch/utils/imutils.py`` (SPIN's image utilities) without skimage, cv2 or scipy.misc.

Same names and signatures: get_transform, transform, crop, rot_aa, flip_img, flip_kp, flip_pose -- plus
``transform_points``, the vectorised ``transform``.  ``uncrop`` is not provided (nothing on the train / eval / demo path
calls it).

* ``get_transform`` / ``transform`` repeat the reference's float64 operations in the reference's order (np.dot,
  np.linalg.inv, truncation toward zero), so the integers are the reference's integers; tests/test_imutils_host.py holds
  them against values recorded from the reference's own functions.
* ``crop`` runs the device op (tuch_amd.ops.crop_batch, csrc/image_crop.hip) on one image: the reference's integer box,
  rotation and resize in one resampling pass whose rule is stated in include/tuch_amd.h.  It needs a HIP device; there is
  no host fallback.  Two stated deviations from skimage: shrinking averages K x K bilinear samples per pixel instead of
  a Gaussian pre-filter, and a box that misses the image gives zeros where the reference raises.
* ``rot_aa`` composes the rotation in float64 on the host (a 3-vector per sample).  cv2.Rodrigues and this code both
  return the rotation vector of R; they differ only in how they round at angles within ~1e-3 of 0 or pi (at pi the sign
  of the axis is a convention).
"""
from __future__ import annotations

import numpy as np

from ..models.smpl import SPIN_JOINT_NAMES, reference_constants
from ..train.fits_dict import SMPL_POSE_FLIP_PERM


def get_transform(center, scale, res, rot=0):
    """Generate transformation matrix (imutils.py:32-56, operation for operation)."""
    h = 200 * scale
    t = np.zeros((3, 3))
    t[0, 0] = float(res[1]) / h
    t[1, 1] = float(res[0]) / h
    t[0, 2] = res[1] * (-float(center[0]) / h + .5)
    t[1, 2] = res[0] * (-float(center[1]) / h + .5)
    t[2, 2] = 1
    if not rot == 0:
        rot = -rot                                       # to match the direction of rotation from cropping
        rot_mat = np.zeros((3, 3))
        rot_rad = rot * np.pi / 180
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        rot_mat[0, :2] = [cs, -sn]
        rot_mat[1, :2] = [sn, cs]
        rot_mat[2, 2] = 1
        t_mat = np.eye(3)                                # rotate around the centre of the crop
        t_mat[0, 2] = -res[1] / 2
        t_mat[1, 2] = -res[0] / 2
        t_inv = t_mat.copy()
        t_inv[:2, 2] *= -1
        t = np.dot(t_inv, np.dot(rot_mat, np.dot(t_mat, t)))
    return t


def transform(pt, center, scale, res, invert=0, rot=0):
    """Transform pixel location to different reference (imutils.py:58-65)."""
    t = get_transform(center, scale, res, rot=rot)
    if invert:
        t = np.linalg.inv(t)
    new_pt = np.array([pt[0] - 1, pt[1] - 1, 1.]).T
    new_pt = np.dot(t, new_pt)
    return new_pt[:2].astype(int) + 1


def transform_points(pts, center, scale, res, invert=0, rot=0):
    """``transform`` for [N,2] points at once: one matrix (and one inverse) instead of one per point, the same integers.
    Every point goes through the same np.dot(t, [x-1, y-1, 1]) as in ``transform``: the product of a 3x3 matrix with one
    vector, so the sums are formed in the same order and round the same way."""
    pts = np.asarray(pts).reshape(-1, 2)
    m1 = (pts - 1).astype(np.float64)                    # ``pt[0] - 1`` in the caller's dtype, as the reference forms it
    t = get_transform(center, scale, res, rot=rot)
    if invert:
        t = np.linalg.inv(t)
    out = np.empty((pts.shape[0], 2), np.int64)
    vec = np.ones(3)
    for n in range(pts.shape[0]):
        vec[0], vec[1] = m1[n, 0], m1[n, 1]
        out[n] = np.dot(t, vec)[:2].astype(int) + 1
    return out


def crop(img, center, scale, res, rot=0):
    """Crop image according to the supplied bounding box (imutils.py:67-106) -> [res0,res1(,C)] float64.  uint8 input is
    scaled to [0,1], as skimage does; float input keeps its range.  One image through the device op with pn = 1, no
    flip, no normalisation."""
    from .. import ops
    if res[0] != res[1]:
        raise ValueError('crop: a square res is supported, got %r' % (res,))
    img = np.asarray(img)
    if img.dtype != np.uint8:
        img = img.astype(np.float32)
    buf, table = ops.pack_images([img])
    rec = ops.crop_records(table, [center], [scale], [rot], [0], None, int(res[0]))
    ch = 1 if img.ndim == 2 or img.shape[2] == 1 else 3
    _, raw = ops.crop_batch(buf, rec, int(res[0]), [0.0] * ch, [1.0] * ch, raw=True)
    out = raw[0].permute(1, 2, 0).cpu().numpy().astype(np.float64)
    if img.dtype != np.uint8:
        out = out * 255.0            # the op's raw is value / 255 clamped to [0, 1]; float sources keep their range in [0, 255]
    return out[:, :, 0] if img.ndim == 2 else out


def _rodrigues(aa):
    """Rotation vector [3] -> matrix [3,3], float64."""
    aa = np.asarray(aa, np.float64).reshape(3)
    th = np.linalg.norm(aa)
    K = np.array([[0, -aa[2], aa[1]], [aa[2], 0, -aa[0]], [-aa[1], aa[0], 0]])
    if th < 1e-8:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / (th * th) * (K @ K)


def _rotvec(R):
    """Rotation matrix -> rotation vector, float64, through the largest quaternion component (stable at every angle)."""
    m = np.asarray(R, np.float64)
    q = np.empty(4)                       # (w, x, y, z)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        q[:] = [1 + tr, m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]]
    else:
        i = int(np.argmax([m[0, 0], m[1, 1], m[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        q[0] = m[k, j] - m[j, k]
        q[1 + i] = 1 + m[i, i] - m[j, j] - m[k, k]
        q[1 + j] = m[j, i] + m[i, j]
        q[1 + k] = m[k, i] + m[i, k]
    q /= np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    s = np.linalg.norm(q[1:])
    if s < 1e-12:
        return 2 * q[1:]
    return 2 * np.arctan2(s, q[0]) / s * q[1:]


def rot_aa(aa, rot):
    """Rotate axis angle parameters (imutils.py:135-146): the rotation vector of R_z(-rot) R(aa)."""
    a = np.deg2rad(-rot)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return _rotvec(np.dot(R, _rodrigues(aa)))


def _swap_sides(names):
    """The permutation that exchanges every 'Left x' / 'Right x' (or 'OP Lx' / 'OP Rx') pair of a list of joint names."""
    index = {n: i for i, n in enumerate(names)}
    perm = []
    for n in names:
        if n.startswith('OP L') or n.startswith('OP R'):
            other = 'OP ' + ('R' if n[3] == 'L' else 'L') + n[4:]
        elif n.startswith('Left '):
            other = 'Right ' + n[5:]
        elif n.startswith('Right '):
            other = 'Left ' + n[6:]
        else:
            other = n
        perm.append(index.get(other, index[n]))
    return perm


def derived_flip_perms():
    """(J24_FLIP_PERM, J49_FLIP_PERM) from SPIN_JOINT_NAMES (models/smpl.py:32): left and right exchanged among the 24
    ground-truth joints and among the 25 OpenPose joints."""
    j24 = _swap_sides(SPIN_JOINT_NAMES[25:])
    j25 = _swap_sides(SPIN_JOINT_NAMES[:25])
    return j24, j25 + [25 + i for i in j24]


def flip_perms():
    """constants.J24_FLIP_PERM / J49_FLIP_PERM when the data folder is importable, else the derived tables."""
    c = reference_constants()
    if c is not None and hasattr(c, 'J24_FLIP_PERM') and hasattr(c, 'J49_FLIP_PERM'):
        return list(c.J24_FLIP_PERM), list(c.J49_FLIP_PERM)
    return derived_flip_perms()


def _pose_flip_perm():
    c = reference_constants()
    return list(getattr(c, 'SMPL_POSE_FLIP_PERM', SMPL_POSE_FLIP_PERM)) if c is not None else list(SMPL_POSE_FLIP_PERM)


def flip_img(img):
    """Flip rgb images or masks; channels come last, e.g. (256,256,3)."""
    return np.fliplr(img)


def flip_kp(kp):
    """Flip keypoints (imutils.py:155-163): 24 or 49 rows; works on [..., N, D] as well."""
    j24, j49 = flip_perms()
    n = kp.shape[-2]
    if n == 24:
        flipped_parts = j24
    elif n == 49:
        flipped_parts = j49
    else:
        raise ValueError('flip_kp: 24 or 49 keypoints, got %d' % n)
    kp = kp[..., flipped_parts, :]
    kp[..., 0] = -kp[..., 0]
    return kp


def flip_pose(pose):
    """Flip pose (imutils.py:165-174), based on SMPL parameters; works on [..., 72] as well."""
    pose = pose[..., _pose_flip_perm()]
    pose[..., 1::3] = -pose[..., 1::3]
    pose[..., 2::3] = -pose[..., 2::3]
    return pose
