#!/usr/bin/env python3
"""Golden vectors for the regressor's input side, produced by running the REFERENCE'S OWN ``tuch/utils/imutils.py`` and
the processing methods of ``tuch/datasets/base_dataset.py`` on the CPU -> tests/golden/imutils.npz (arrays only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_imutils.py

Stubs (the packages are absent here and not vendored):
  * ``skimage.transform.resize`` / ``rotate`` are RECORDERS: they keep the array and the arguments they were handed and
    return an array of the right shape.  What is recorded is the reference's geometry -- the integer box, the pad, the
    zero-padded copy, the angle -- without skimage's filters;
  * ``cv2.Rodrigues`` is scipy's ``Rotation`` (as in make_golden_train.py), ``scipy.misc`` an empty module;
  * ``data.essentials.constants`` carries SPIN's flip permutations and IMG_RES;
  * ``torchvision``, ``joblib`` and ``configs.config`` are empty stand-ins when they cannot be imported (only
    ``BaseDataset``'s processing methods are called, unbound, on a SimpleNamespace).
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('TUCH_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(1, REF)

import numpy as np
from scipy.spatial.transform import Rotation

from tuch_amd.train.fits_dict import SMPL_POSE_FLIP_PERM

J24_FLIP_PERM = [5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13, 14, 15, 16, 17, 18, 19, 21, 20, 23, 22]
J49_FLIP_PERM = [0, 1, 5, 6, 7, 2, 3, 4, 8, 12, 13, 14, 9, 10, 11, 16, 15, 18, 17, 22, 23, 24, 19, 20, 21] \
    + [25 + i for i in J24_FLIP_PERM]
RECORD = {'resize': [], 'rotate': []}


def _install_stubs():
    def module(name, **attrs):
        mod = types.ModuleType(name)
        mod.__path__ = []
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
        return mod

    def resize(img, res, *a, **kw):
        RECORD['resize'].append(np.array(img, copy=True))
        return np.zeros(tuple(res) + tuple(img.shape[2:]))

    def rotate(img, angle, *a, **kw):
        RECORD['rotate'].append((img.shape, float(angle), np.array(img, copy=True)))
        return img
    sk = module('skimage')
    sk.transform = module('skimage.transform', resize=resize, rotate=rotate)
    module('cv2', Rodrigues=lambda x: (
        (Rotation.from_rotvec(np.asarray(x, np.float64).reshape(3)).as_matrix(), None) if np.size(x) == 3
        else (Rotation.from_matrix(np.asarray(x, np.float64)).as_rotvec().reshape(3, 1), None)))
    import scipy
    scipy.misc = module('scipy.misc')
    data = module('data')
    ess = module('data.essentials')
    data.essentials = ess
    ess.constants = module('data.essentials.constants', IMG_RES=224, J24_FLIP_PERM=J24_FLIP_PERM,
                           J49_FLIP_PERM=J49_FLIP_PERM, SMPL_POSE_FLIP_PERM=list(SMPL_POSE_FLIP_PERM),
                           IMG_NORM_MEAN=[0.485, 0.456, 0.406], IMG_NORM_STD=[0.229, 0.224, 0.225])
    for name, attrs in (('torchvision', {}), ('torchvision.transforms', {'Normalize': lambda **kw: None}),
                        ('joblib', {}), ('configs', {}), ('configs.config', {})):
        try:
            __import__(name)
        except Exception:
            module(name, **attrs)
    if not hasattr(sys.modules['configs'], 'config'):
        sys.modules['configs'].config = sys.modules['configs.config']
    if not hasattr(sys.modules['torchvision'], 'transforms'):
        sys.modules['torchvision'].transforms = sys.modules['torchvision.transforms']


_install_stubs()
from tuch.utils import imutils as ref                      # noqa: E402
from tuch.datasets.base_dataset import BaseDataset          # noqa: E402


def main():
    rng = np.random.default_rng(20240607)
    out = {}

    # ---- get_transform / transform, both directions ---------------------------------------------------------------
    n, npts = 300, 6
    params = np.zeros((n, 5))
    for k in range(n):
        res = int(rng.choice([8, 16, 224]))
        kind = k % 5
        if kind == 0:                                        # inside a small image
            c = rng.uniform(0, 40, 2)
        elif kind == 1:                                      # negative and beyond-the-image centres
            c = rng.uniform(-300, 1500, 2)
        elif kind == 2:                                      # exactly representable half-integers
            c = rng.integers(-20, 400, 2) + 0.5
        elif kind == 3:                                      # integers
            c = rng.integers(0, 400, 2).astype(np.float64)
        else:
            c = rng.uniform(0, 1100, 2)
        scale = float(rng.choice([res / 200.0, rng.uniform(0.05, 6.0), rng.integers(1, 9) * 0.25]))
        rot = float(rng.choice([0.0, 0.0, rng.uniform(-60, 60), rng.choice([30.0, -77.5, 90.0, 180.0, 270.0])]))
        params[k] = (c[0], c[1], scale, rot, res)
    pts = np.concatenate([rng.uniform(-50, 1200, (n, npts - 2, 2)), rng.integers(-5, 300, (n, 1, 2)) + 0.5,
                          rng.integers(1, 300, (n, 1, 2)).astype(np.float64)], 1)
    mats = np.zeros((n, 3, 3))
    fwd, inv = np.zeros((n, npts, 2), np.int64), np.zeros((n, npts, 2), np.int64)
    for k in range(n):
        cx, cy, s, rot, res = params[k]
        res = [int(res), int(res)]
        mats[k] = ref.get_transform([cx, cy], s, res, rot=rot)
        for p in range(npts):
            fwd[k, p] = ref.transform(pts[k, p], [cx, cy], s, res, rot=rot)
            inv[k, p] = ref.transform(pts[k, p], [cx, cy], s, res, invert=1, rot=rot)
    out.update(gt_params=params, gt_matrix=mats, gt_points=pts, gt_forward=fwd, gt_inverse=inv)

    # ---- crops: the reference's box, pad and zero-padded copy -------------------------------------------------------
    shapes = [(1, 1, 3), (7, 5, 1), (30, 40, 3), (23, 17, 3), (12, 31, 1)]
    images = [rng.integers(0, 256, s).astype(np.uint8) for s in shapes]
    for k, im in enumerate(images):
        out['image_%d' % k] = im
    draws = []
    for k in range(64):                                      # identity scale, rot 0: the box side is R
        res = int(rng.choice([8, 16]))
        img = int(rng.integers(0, len(images)))
        h, w = shapes[img][:2]
        c = rng.uniform(-res / 2, max(h, w) + res / 2, 2) if k % 3 else rng.integers(-4, max(h, w) + 4, 2) + 0.5 * (k % 2)
        draws.append((img, c[0], c[1], res / 200.0, 0.0, res))
    for k in range(18):                                      # quarter turns at the identity scale
        res = int(rng.choice([8, 16]))
        img = int(rng.choice([2, 3]))
        h, w = shapes[img][:2]
        draws.append((img, float(rng.integers(4, w - 4)), float(rng.integers(4, h - 4)), res / 200.0, [90.0, 180.0, 270.0][k % 3], res))
    draws.append((2, 3.2, 28.7, 0.2, 0.0, 16))             # the ragged 39 x 40 box
    draws.append((2, 3.2, 28.7, 0.2, 30.0, 16))
    for k in range(60):                                      # general draws
        res = int(rng.choice([8, 16]))
        img = int(rng.integers(0, len(images)))
        h, w = shapes[img][:2]
        draws.append((img, rng.uniform(-10, w + 10), rng.uniform(-10, h + 10), rng.uniform(0.02, 0.24),
                      float(rng.choice([0.0, 30.0, -77.5, rng.uniform(-60, 60)])), res))
    kept, boxes, handed, handed_shape, rot_shape, skipped = [], [], [], [], [], 0
    for d in draws:
        img, cx, cy, s, rot, res = d
        RECORD['resize'].clear()
        RECORD['rotate'].clear()
        try:
            ref.crop(images[img].astype(np.float64) if images[img].shape[2] > 1 else images[img][:, :, 0].astype(np.float64),
                     [cx, cy], s, [res, res], rot=rot)
        except ValueError:                                   # the box misses the image: the reference cannot broadcast
            skipped += 1
            continue
        ul = np.array(ref.transform([1, 1], [cx, cy], s, [res, res], invert=1)) - 1
        br = np.array(ref.transform([res + 1, res + 1], [cx, cy], s, [res, res], invert=1)) - 1
        pad = int(np.linalg.norm(br - ul) / 2 - float(br[1] - ul[1]) / 2)
        kept.append(d)
        boxes.append([ul[0], ul[1], br[0], br[1], pad])
        if rot == 0:
            a = RECORD['resize'][0]
            rot_shape.append([0, 0, 0])
        else:
            shp, angle, a = RECORD['rotate'][0]
            assert angle == rot
            rot_shape.append([shp[0], shp[1], 1])
        a = a[:, :, None] if a.ndim == 2 else a
        assert np.array_equal(a, np.round(a)) and a.min() >= 0 and a.max() <= 255
        handed.append(a.astype(np.uint8).reshape(-1))
        handed_shape.append(list(a.shape))
    out.update(crop_draws=np.array(kept, np.float64), crop_boxes=np.array(boxes, np.int64),
               crop_handed=np.concatenate(handed), crop_handed_shape=np.array(handed_shape, np.int64),
               crop_rotate_shape=np.array(rot_shape, np.int64), crop_skipped=np.array([skipped], np.int64))

    # ---- rot_aa, flips, the dataset's processing methods ------------------------------------------------------------
    m = 40
    aa = rng.normal(0, 1.0, (m, 3))
    aa[0] = 0
    aa[1] = [0, 0, 1e-5]
    rots = np.where(rng.uniform(size=m) < 0.3, 0.0, rng.uniform(-60, 60, m))
    out.update(rot_aa_in=aa, rot_aa_rot=rots, rot_aa_out=np.stack([ref.rot_aa(aa[k].copy(), rots[k]) for k in range(m)]))
    kp24, kp49, pose = rng.normal(0, 1, (24, 4)), rng.normal(0, 1, (49, 3)), rng.normal(0, 0.6, 72)
    out.update(flip_kp24_in=kp24, flip_kp24_out=ref.flip_kp(kp24.copy()), flip_kp49_in=kp49, flip_kp49_out=ref.flip_kp(kp49.copy()),
               flip_pose_in=pose, flip_pose_out=ref.flip_pose(pose.copy()))
    ns = types.SimpleNamespace()
    b = 24
    p_center, p_scale = rng.uniform(50, 600, (b, 2)), rng.uniform(0.4, 4.0, b)
    p_rot = np.where(rng.uniform(size=b) < 0.4, 0.0, rng.uniform(-60, 60, b))
    p_flip = (rng.uniform(size=b) < 0.5).astype(np.int64)
    kp = np.concatenate([rng.uniform(-20, 900, (b, 49, 2)), rng.uniform(0, 1, (b, 49, 1))], 2)
    kp[:, :4, :2] = np.round(kp[:, :4, :2]) + 0.5
    kp32 = kp.astype(np.float32)
    S = np.concatenate([rng.normal(0, 0.5, (b, 24, 3)), np.ones((b, 24, 1))], 2)
    poses = rng.normal(0, 0.5, (b, 72))
    out.update(proc_center=p_center, proc_scale=p_scale, proc_rot=p_rot, proc_flip=p_flip, proc_kp=kp, proc_kp32=kp32,
               proc_S=S, proc_pose=poses)
    out['proc_kp_out'] = np.stack([BaseDataset.j2d_processing(ns, kp[k].copy(), p_center[k], p_scale[k], p_rot[k], p_flip[k])
                                   for k in range(b)])
    out['proc_kp32_out'] = np.stack([BaseDataset.j2d_processing(ns, kp32[k].copy(), p_center[k], p_scale[k], p_rot[k], p_flip[k])
                                     for k in range(b)])
    out['proc_S_out'] = np.stack([BaseDataset.j3d_processing(ns, S[k].copy(), p_rot[k], p_flip[k]) for k in range(b)])
    out['proc_S3_out'] = np.stack([BaseDataset.j3d_processing(ns, S[k, :, :3].copy(), p_rot[k], p_flip[k]) for k in range(b)])
    out['proc_pose_out'] = np.stack([BaseDataset.pose_processing(ns, poses[k].copy(), p_rot[k], p_flip[k]) for k in range(b)])

    path = os.path.join(HERE, 'imutils.npz')
    np.savez_compressed(path, **out)
    print('%s: %d bytes, %d crop draws kept, %d skipped (box misses the image)' % (path, os.path.getsize(path), len(kept), skipped))


if __name__ == '__main__':
    main()
