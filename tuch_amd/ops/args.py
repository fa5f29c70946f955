"""The rules for caller arguments that more than one operation (and fit.py's constructors) share, and nothing else:
each takes ``what`` -- the caller's name for the message -- and returns the argument as the C entry points take it
(the ``check_`` ones return nothing), or raises.  No kernel is bound here."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _C


def both(what, name_a, a, name_b, b) -> bool:
    """Two arguments that go together: False with neither, True with both; one alone raises."""
    if (a is None) != (b is None):
        raise ValueError('%s: %s and %s go together, got %s only' % (what, name_a, name_b, name_b if a is None else name_a))
    return a is not None


def angle_of(what, name, max_angle) -> float:
    """The largest normal angle in degrees, in (0, 90]; ``name`` is what the caller's argument is called."""
    angle = float(max_angle)
    if not (0.0 < angle <= 90.0):
        raise ValueError('%s: %s must be in (0, 90] degrees, got %r' % (what, name, max_angle))
    return angle


def max_angle_cos(normals, max_angle, points, what):
    """None without normals and angle; otherwise the float32 cosine the C entry points take: cos(max_angle) in double,
    rounded once.  One of the two alone, an angle outside (0, 90] degrees or normals of another shape raise ValueError."""
    if not both(what, 'normals', normals, 'max_angle', max_angle):
        return None
    angle = angle_of(what, 'max_angle', max_angle)
    if not torch.is_tensor(normals) or tuple(normals.shape) != tuple(points.shape) or normals.device != points.device:
        raise ValueError('%s: normals must be [B,Q,3] = %s on %s, got %s'
                         % (what, tuple(points.shape), points.device,
                            (tuple(normals.shape), normals.device) if torch.is_tensor(normals) else type(normals)))
    cos = float(np.float32(math.cos(math.radians(angle))))
    # (90 degrees: cos is 6e-17 in double; anything in [0, 1) is the contract)
    return min(max(cos, 0.0), float(np.nextafter(np.float32(1.0), np.float32(0.0))))


def hint_of(hint, points, what):
    """hint as the kernels read it: int32 [B,Q] on the points' device, contiguous (the tensor itself where it already is:
    a loop's hint tensor may be the one the faces are written to)."""
    if hint is None:
        return None
    if tuple(hint.shape) != tuple(points.shape[:2]) or hint.device != points.device:
        raise _C.TuchError('%s: hint must be [B,Q] = %s on %s, got %s on %s'
                           % (what, tuple(points.shape[:2]), points.device, tuple(hint.shape), hint.device))
    return hint.to(torch.int32).contiguous()


SCAN_RHO = {'squared': 0, 'distance': 1, 'gmof': 2}


def rho_of(what, rho, sigma):
    """(rho, sigma) as the C entry points of scan_fit and cloud_fit take them."""
    if rho not in SCAN_RHO:
        raise ValueError('%s: rho must be one of %s, got %r' % (what, sorted(SCAN_RHO), rho))
    if rho == 'gmof' and not (sigma is not None and float(sigma) > 0.0):
        raise ValueError("%s: rho='gmof' needs sigma > 0, got %r" % (what, sigma))
    return SCAN_RHO[rho], float(sigma) if sigma is not None else 0.0


def resolution_of(what, resolution) -> int:
    """Cells of a PointCloud's grid along the longest extent."""
    if not (isinstance(resolution, int) and 1 <= resolution <= 256):
        raise ValueError('%s: resolution must be an int in 1 .. 256, got %r' % (what, resolution))
    return resolution


def counts_of(what, counts, b):
    """counts [B] (real entries per body) as the C entry points take it: int32, contiguous; None stays None."""
    if counts is None:
        return None
    if tuple(counts.shape) != (b,):
        raise ValueError('%s: counts must be [%d], got %s' % (what, b, tuple(counts.shape)))
    return counts.to(torch.int32).contiguous()


def check_weights(what, weights, b, q):
    if weights is not None and tuple(weights.shape) != (b, q):
        raise ValueError('%s: weights must be [%d,%d], got %s' % (what, b, q, tuple(weights.shape)))


MAX_NEIGHBOURS = 32


def check_k(what, k):
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_NEIGHBOURS:
        raise ValueError('%s: k must be an int in 1 .. %d, got %r' % (what, MAX_NEIGHBOURS, k))


def tau_of(what, max_distance) -> float:
    if max_distance is None:
        return 0.0
    tau = float(max_distance)
    if not tau > 0.0:
        raise ValueError('%s: max_distance must be > 0 (or None), got %r' % (what, max_distance))
    return tau


def index_out(what, index_out, b, n, device):
    if index_out is None:
        return torch.empty(b, n, dtype=torch.int32, device=device)
    if tuple(index_out.shape) != (b, n) or index_out.dtype != torch.int32 or not index_out.is_contiguous():
        raise ValueError('%s: index_out must be a contiguous int32 [%d,%d] tensor' % (what, b, n))
    return index_out
