"""The regressor's input side for a whole batch: augmentation parameters, image crops on the device, keypoints and poses.

The reference does this per sample in dataset workers (tuch/datasets/base_dataset.py:163-248 with tuch/utils/imutils.py,
cv2 and skimage) and once more in demo_tuch.py:80-102.  Here a dataset hands over the raw images and annotations of a
batch and gets the tensors the regressor eats:

    ri = RegressorInput(options, img_res=224, is_train=True)
    flip, pn, rot, sc = ri.augm_params(B, rng)                                   # base_dataset.py:163-190, per sample
    img = ri.rgb_processing(images, center, sc * scale, rot, flip, pn)           # [B,3,224,224] on the device, normalised
    kp = ri.j2d_processing(keypoints, center, sc * scale, rot, flip)             # [B,49,3] float32
    S = ri.j3d_processing(pose_3d, rot, flip)                                    # [B,24,4] float32
    pose = ri.pose_processing(pose, rot, flip)                                   # [B,72] float32

``rgb_processing`` is one launch of csrc/image_crop.hip (rule: include/tuch_amd.h) and returns the NORMALISED image, i.e.
base_dataset.py:192-205 followed by ``normalize_img``; ``raw=True`` adds the image in [0,1].  It reads the original image:
the reference's 448-pixel pre-resize (base_dataset.py:259-265) exists only to make its host crop affordable, the K x K
samples of the rule take its place.  The other three run on the host in the reference's arithmetic, a batch per call.
"""
from __future__ import annotations

import types

import numpy as np

from .utils import imutils

# SPIN's constants.IMG_NORM_MEAN / IMG_NORM_STD (the ImageNet statistics) and its default augmentation options
IMG_NORM_MEAN = [0.485, 0.456, 0.406]
IMG_NORM_STD = [0.229, 0.224, 0.225]
DEFAULT_OPTIONS = dict(noise_factor=0.4, rot_factor=30, scale_factor=0.25)


def bbox_from_openpose(keypoints, rescale=1.2, detection_thresh=0.2):
    """Centre and scale from OpenPose detections [N,3] (demo_tuch.py:51-65)."""
    keypoints = np.reshape(np.asarray(keypoints), (-1, 3))
    valid_keypoints = keypoints[keypoints[:, -1] > detection_thresh][:, :-1]
    center = valid_keypoints.mean(axis=0)
    bbox_size = (valid_keypoints.max(axis=0) - valid_keypoints.min(axis=0)).max()
    return center, bbox_size / 200.0 * rescale


def bbox_from_xywh(bbox):
    """Centre and scale from [top_left(x), top_left(y), width, height] (demo_tuch.py:67-78)."""
    bbox = np.asarray(bbox).astype(np.float32)
    return bbox[:2] + 0.5 * bbox[2:], max(bbox[2], bbox[3]) / 200.0


class RegressorInput:
    def __init__(self, options=None, img_res=224, mean=IMG_NORM_MEAN, std=IMG_NORM_STD, is_train=True,
                 use_augmentation=True, device=None):
        if options is None:
            options = types.SimpleNamespace(**DEFAULT_OPTIONS)
        self.options = options
        self.img_res = int(img_res)
        self.mean, self.std = [float(m) for m in mean], [float(s) for s in std]
        self.is_train, self.use_augmentation = bool(is_train), bool(use_augmentation)
        self.device = device

    # ------------------------------------------------------------------------------------------- parameters
    def augm_params(self, n, generator=None):
        """base_dataset.py:163-190 for n samples -> (flip [n] int, pn [n,3], rot [n], sc [n]).  The draws of one sample
        follow one another in the reference's order (flip, pixel noise, rotation, scale, the 3/5 chance of no rotation),
        sample after sample, from ``generator`` (a numpy.random.Generator).  Without training or augmentation: 0, 1, 0, 1."""
        flip, pn = np.zeros(n, np.int64), np.ones((n, 3))
        rot, sc = np.zeros(n), np.ones(n)
        if self.is_train and self.use_augmentation:
            g = np.random.default_rng() if generator is None else generator
            o = self.options
            for k in range(n):
                if g.uniform() <= 0.5:
                    flip[k] = 1
                pn[k] = g.uniform(1 - o.noise_factor, 1 + o.noise_factor, 3)
                rot[k] = min(2 * o.rot_factor, max(-2 * o.rot_factor, g.standard_normal() * o.rot_factor))
                sc[k] = min(1 + o.scale_factor, max(1 - o.scale_factor, g.standard_normal() * o.scale_factor + 1))
                if g.uniform() <= 0.6:
                    rot[k] = 0
        return flip, pn, rot, sc

    # ------------------------------------------------------------------------------------------- images
    def rgb_processing(self, images, center, scale, rot, flip, pn, raw=False):
        """base_dataset.py:192-205 + normalisation for a batch on the device.  images: a list of HWC arrays (uint8, or
        float in [0,255]) of any sizes, or the (buffer, table) of ops.pack_images.  -> [B,C,R,R] float32, normalised;
        with raw=True (normalised, in [0,1])."""
        from . import ops
        buf, table = images if isinstance(images, tuple) else ops.pack_images(images, device=self.device)
        rec = ops.crop_records(table, center, scale, rot, flip, pn, self.img_res)
        return ops.crop_batch(buf, rec, self.img_res, self.mean, self.std, raw=raw)

    def process_image(self, img, bbox=None, keypoints=None):
        """demo_tuch.py:80-102 for an image already read (RGB, HWC): bbox = [x, y, width, height], else keypoints =
        OpenPose detections [N,3], else the person is assumed centred.  -> (img [3,R,R] in [0,1], norm_img [1,3,R,R])."""
        img = np.asarray(img)
        if bbox is not None:
            center, scale = bbox_from_xywh(bbox)
        elif keypoints is not None:
            center, scale = bbox_from_openpose(keypoints)
        else:
            height, width = img.shape[0], img.shape[1]
            center, scale = np.array([width // 2, height // 2]), max(height, width) / 200
        norm, raw = self.rgb_processing([img], [center], [scale], [0], [0], None, raw=True)
        return raw[0], norm

    # ------------------------------------------------------------------------------------------- annotations
    def j2d_processing(self, kp, center, scale, r, f):
        """base_dataset.py:207-219 for kp [B,N,3] (N = 24 or 49): every keypoint through imutils.transform (the same
        integers), normalised to [-1,1], flipped where f.  The arithmetic runs in kp's dtype, as the reference's does."""
        kp = np.array(kp, copy=True)
        res = [self.img_res, self.img_res]
        for b in range(kp.shape[0]):
            kp[b, :, 0:2] = imutils.transform_points(kp[b, :, 0:2] + 1, center[b], scale[b], res, rot=r[b])
        kp[:, :, :-1] = 2. * kp[:, :, :-1] / self.img_res - 1.
        out = kp.astype('float32')
        for b in np.nonzero(np.asarray(f))[0]:
            out[b] = imutils.flip_kp(kp[b]).astype('float32')
        return out

    def j3d_processing(self, S, r, f):
        """base_dataset.py:221-238 for S [B,24,3 or 4].  The reference builds the in-plane rotation matrix when r != 0
        and then NEVER APPLIES it: the product sits in the ``elif`` branches of that very test (base_dataset.py:223-233),
        so it runs only at r == 0, with the identity.  That behaviour is kept: 3D joints are not rotated, only flipped."""
        S = np.array(S, copy=True)
        out = S.astype('float32')
        for b in np.nonzero(np.asarray(f))[0]:
            out[b] = imutils.flip_kp(S[b]).astype('float32')
        return out

    def pose_processing(self, pose, r, f):
        """base_dataset.py:240-248 for pose [B,72]: the global orientation turned by r (imutils.rot_aa), flipped where f."""
        pose = np.array(pose, copy=True)
        for b in range(pose.shape[0]):
            pose[b, :3] = imutils.rot_aa(pose[b, :3], r[b])
        out = pose.astype('float32')
        for b in np.nonzero(np.asarray(f))[0]:
            out[b] = imutils.flip_pose(pose[b]).astype('float32')
        return out
