"""The resampling rule of tuch_crop_batch (include/tuch_amd.h) restated in plain numpy float64, for the tests.

  crop_from_records   consumes the INTEGER records (ops.crop_records): the same texels and the same weights frac / 65536 as
                      the kernel, every product and sum in float64 -- what the kernel must match to float32 rounding.
  closed_form         the float64 map of the rule written out from centre, scale, rot and flip, without any integer
                      affine -- what the records must match to 2^-12 px.
  record_positions    the positions the records give, as floats in pixels, on the same grid.

Nothing here imports tuch_amd except for the reference's integer box, which closed_form takes as an argument.
"""
import numpy as np


def grid(K, R, pixels=None):
    """Integer grid coordinates of every sample: (gx, gy) [N, K*K] for the N pixels (i, j) (default: all R*R, row-major),
    samples in the kernel's order (v outermost)."""
    if pixels is None:
        i, j = np.divmod(np.arange(R * R, dtype=np.int64), R)
    else:
        i, j = np.asarray(pixels, np.int64).reshape(-1, 2).T
    v, u = np.divmod(np.arange(K * K, dtype=np.int64), K)
    return 2 * K * j[:, None] + 2 * u[None, :] + 1, 2 * K * i[:, None] + 2 * v[None, :] + 1


def record_fixed(rec, R, pixels=None):
    """(X, Y) int64 in units of 2^-16 px, texel-index coordinates of the padded box P."""
    K = int(rec['K'])
    gx, gy = grid(K, R, pixels)
    if rec['flip']:
        gx = 2 * K * R - gx
    ax, ay = [int(a) for a in rec['ax']], [int(a) for a in rec['ay']]
    return (ax[0] * gx + ax[1] * gy + ax[2]) >> 16, (ay[0] * gx + ay[1] * gy + ay[2]) >> 16


def record_positions(rec, R, pixels=None):
    X, Y = record_fixed(rec, R, pixels)
    return X / 65536.0, Y / 65536.0


def closed_form(ul, br, rot, flip, R, K, pixels=None):
    """The map of the rule in float64: output point -> box -> shift by p -> rotate by +rot about the centre of P ->
    minus 0.5; texel-index coordinates of P (add ul - p for image texels)."""
    bw, bh = int(br[0] - ul[0]), int(br[1] - ul[1])
    p = int(np.linalg.norm(np.asarray(br) - np.asarray(ul)) / 2 - float(bh) / 2) if rot != 0 else 0
    gx, gy = grid(K, R, pixels)
    xo, yo = gx / (2.0 * K), gy / (2.0 * K)
    if flip:
        xo = R - xo
    x, y = xo * bw / R + p, yo * bh / R + p
    cx, cy = (bw + 2 * p) / 2.0, (bh + 2 * p) / 2.0
    th = np.deg2rad(float(rot))
    c, s = (np.cos(th), np.sin(th)) if rot != 0 else (1.0, 0.0)
    dx, dy = x - cx, y - cy
    return c * dx - s * dy + cx - 0.5, s * dx + c * dy + cy - 0.5


def _texels(buf, rec, sx, sy):
    """Source values [N, S, C] float64 at image texels (sx, sy); 0 outside the image."""
    H, W, C, stride, off = int(rec['height']), int(rec['width']), int(rec['channels']), int(rec['stride']), int(rec['offset'])
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    cx, cy = np.where(inside, sx, 0), np.where(inside, sy, 0)
    if rec['type'] == 1:
        words = buf[off:off + (H - 1) * stride + W * C * 4].copy().view(np.float32)
        at = cy * (stride // 4) + cx * C
        vals = np.stack([words[at + c] for c in range(C)], -1).astype(np.float64)
    else:
        at = off + cy * stride + cx * C
        vals = np.stack([buf[at + c] for c in range(C)], -1).astype(np.float64)
    return vals * inside[..., None]


def crop_from_records(buf, rec, R, mean, std, pixels=None):
    """buf: the packed bytes (numpy uint8), rec: ONE record.  -> (raw, out) float64 [C_out, N] for the N pixels (default
    all, row-major: reshape to [C_out, R, R])."""
    buf = np.asarray(buf, np.uint8)
    mean, std = np.asarray(mean, np.float64).reshape(-1), np.asarray(std, np.float64).reshape(-1)
    K = int(rec['K'])
    X, Y = record_fixed(rec, R, pixels)
    ix, iy, fx, fy = X >> 16, Y >> 16, (X & 0xffff) / 65536.0, (Y & 0xffff) / 65536.0
    pw, ph, ox, oy = int(rec['pw']), int(rec['ph']), int(rec['ox']), int(rec['oy'])
    x0, x1 = np.clip(ix, 0, pw - 1) + ox, np.clip(ix + 1, 0, pw - 1) + ox
    y0, y1 = np.clip(iy, 0, ph - 1) + oy, np.clip(iy + 1, 0, ph - 1) + oy
    t00, t01, t10, t11 = (_texels(buf, rec, a, b) for a, b in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)))
    fx, fy = fx[..., None], fy[..., None]
    top = t00 * (1 - fx) + t01 * fx
    bot = t10 * (1 - fx) + t11 * fx
    m = (top * (1 - fy) + bot * fy).sum(1) / (K * K)                     # [N, C]
    if m.shape[1] == 1:
        m = np.repeat(m, len(mean), 1)
    v = np.clip(m * np.asarray(rec['pn'], np.float64)[None, :len(mean)], 0.0, 255.0)
    raw = v / 255.0
    return raw.T, ((raw - mean[None]) / std[None]).T


def centroid(plane):
    """Intensity centroid (x, y) of a [R, R] plane in pixel coordinates (pixel k spans [k, k+1): its centre is k + 0.5)."""
    plane = np.asarray(plane, np.float64)
    total = plane.sum()
    ys, xs = np.mgrid[0:plane.shape[0], 0:plane.shape[1]]
    return ((xs + 0.5) * plane).sum() / total, ((ys + 0.5) * plane).sum() / total
