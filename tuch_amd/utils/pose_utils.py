"""Procrustes alignment and reconstruction error (reference: tuch/utils/pose_utils.py), on the device.

Same names, signatures and results as the reference, which loops over the bodies on the host with one
np.linalg.svd each; here one HIP kernel per call (csrc/pose_eval.hip: tuch_procrustes), one wavefront per body,
float64 inside.  numpy in -> numpy out (dtype and shape as the reference returns them, eval.py:194 calls it so);
tensors on the GPU stay there, with no host synchronisation.  There is no host fallback: without a HIP device
these functions raise.

Layout rule of the reference (pose_utils.py:35-39): a per-body matrix whose first axis is 2 or 3 is read as
coordinates x points, anything else as points x coordinates (then the coordinates must be 2 or 3 here).
"""
from __future__ import annotations

import numpy as np
import torch


def _layout(shape):
    """(N, D, coords_first) of one body's matrix shape."""
    if len(shape) != 2:
        raise ValueError('pose_utils: a body is a 2-D matrix of points, got shape %s' % (tuple(shape),))
    a, b = int(shape[0]), int(shape[1])
    if a in (2, 3):
        return b, a, True
    if b not in (2, 3):
        raise ValueError('pose_utils: points must have 2 or 3 coordinates, got a body of shape (%d, %d)' % (a, b))
    return a, b, False


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('tuch_amd.utils.pose_utils runs on a HIP device and none is available '
                           '(there is no host fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def _procrustes(S1, S2, want_hat):
    """Batched [B, a, b] inputs of one type (numpy or tensor) -> (S1_hat or None, err [B]) of the same type."""
    is_np = isinstance(S1, np.ndarray)
    if is_np != isinstance(S2, np.ndarray) or (not is_np and not (torch.is_tensor(S1) and torch.is_tensor(S2))):
        raise TypeError('pose_utils: S1 and S2 must both be numpy arrays or both torch tensors')
    if tuple(S1.shape) != tuple(S2.shape):
        raise ValueError('pose_utils: S1 %s and S2 %s differ in shape' % (tuple(S1.shape), tuple(S2.shape)))
    if S1.ndim != 3:
        raise ValueError('pose_utils: expected [B, N, D] (or [B, D, N]) arrays, got shape %s' % (tuple(S1.shape),))
    N, D, coords_first = _layout(S1.shape[1:])
    B = int(S1.shape[0])
    if is_np:
        if S1.dtype != S2.dtype:
            raise TypeError('pose_utils: S1 (%s) and S2 (%s) differ in dtype' % (S1.dtype, S2.dtype))
        dt = S1.dtype if S1.dtype in (np.float32, np.float64) else np.dtype(np.float64)
        if B == 0:
            return (np.zeros(S1.shape, dt) if want_hat else None), np.zeros(0, dt)
        dev = _device()
        a = torch.from_numpy(np.ascontiguousarray(S1, dtype=dt)).to(dev)
        b = torch.from_numpy(np.ascontiguousarray(S2, dtype=dt)).to(dev)
    else:
        if S1.dtype != S2.dtype or S1.dtype not in (torch.float32, torch.float64):
            raise TypeError('pose_utils: S1 and S2 must both be float32 or both float64, got %s and %s'
                            % (S1.dtype, S2.dtype))
        if S1.device != S2.device:
            raise ValueError('pose_utils: S1 and S2 are on different devices')
        if B == 0:
            return (torch.zeros_like(S1) if want_hat else None), S1.new_zeros(0)
        if not S1.is_cuda:
            _device()
            raise RuntimeError('pose_utils: tensors must be on the HIP device (there is no host fallback), got %s'
                               % S1.device)
        a, b = S1.detach().contiguous(), S2.detach().contiguous()
    from .. import _C
    hat = torch.empty_like(a) if want_hat else None
    err = torch.empty(B, dtype=a.dtype, device=a.device)
    with torch.cuda.device(a.device):
        _C.check(_C.lib().tuch_procrustes(_C.ptr(a), _C.ptr(b), B, N, D, int(coords_first),
                                          int(a.dtype == torch.float64), _C.ptr(hat), _C.ptr(err), _C.stream()))
    if is_np:
        return (hat.cpu().numpy() if want_hat else None), err.cpu().numpy()
    return hat, err


def compute_similarity_transform(S1, S2):
    """The similarity transform (s R, t) that takes the points S1 closest to S2 (orthogonal Procrustes), applied to
    S1: one body, [N, D] or [D, N].  Like the reference, a numpy result is float64 (its R is)."""
    if isinstance(S1, np.ndarray) and isinstance(S2, np.ndarray):
        S1, S2 = S1.astype(np.float64), S2.astype(np.float64)
    hat, _ = _procrustes(S1[None], S2[None], True)
    return hat[0]


def compute_similarity_transform_batch(S1, S2):
    """Batched version of compute_similarity_transform: [B, N, D] (or [B, D, N]) -> S1_hat of S1's shape and dtype."""
    hat, _ = _procrustes(S1, S2, True)
    return hat


def reconstruction_error(S1, S2, reduction='mean'):
    """Procrustes-align S1 to S2 and return the mean point distance per body; reduction 'mean' or 'sum' over the
    bodies, anything else -> the per-body array [B]."""
    _, re = _procrustes(S1, S2, False)
    if reduction == 'mean':
        re = re.mean()
    elif reduction == 'sum':
        re = re.sum()
    return re
