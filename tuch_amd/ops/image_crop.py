"""The regressor's input crops on the kernel of csrc/image_crop.hip: packed images, the per-sample records built and
checked on the host, and the batched crop."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _C


# tuch_crop_record of include/tuch_amd.h, field for field
CROP_RECORD = np.dtype([('offset', '<i8'), ('stride', '<i8'), ('ax', '<i8', (3,)), ('ay', '<i8', (3,)),
                        ('height', '<i4'), ('width', '<i4'), ('channels', '<i4'), ('type', '<i4'),
                        ('pw', '<i4'), ('ph', '<i4'), ('ox', '<i4'), ('oy', '<i4'), ('K', '<i4'), ('flip', '<i4'),
                        ('pn', '<f4', (3,)), ('reserved', '<i4')])
assert CROP_RECORD.itemsize == 120
# where an image lies in a packed buffer: byte offset of its first texel, bytes between rows, size, 0 = uint8 / 1 = float32
IMAGE_TABLE = np.dtype([('offset', '<i8'), ('stride', '<i8'), ('height', '<i4'), ('width', '<i4'), ('channels', '<i4'),
                        ('type', '<i4')])
CROP_MAX_RES = 1024
CROP_MAX_K = 16
CROP_FRAC_BITS = 32          # fractional bits of the integer affine; positions are its values >> 16 (units of 2^-16 px)
_CROP_LIMIT = 1 << 29


def pack_images(images, device=None, row_align: int = 4):
    """A list of HWC (or HW) arrays, uint8 or float32 (anything else is converted to float32), of any sizes -> (buffer,
    table): one uint8 device tensor holding all of them and the IMAGE_TABLE array saying where.  Rows are padded to
    ``row_align`` bytes and images start on 16-byte boundaries; the bytes are assembled in ONE pinned host buffer and go to
    the device in one asynchronous copy."""
    if row_align < 1:
        raise ValueError('row_align must be positive')
    device = torch.device('cuda' if device is None else device)
    table = np.zeros(len(images), IMAGE_TABLE)
    arrays, at = [], 0
    for n, img in enumerate(images):
        a = np.asarray(img.detach().cpu() if torch.is_tensor(img) else img)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError('image %d: expected [H, W], [H, W, 1] or [H, W, 3], got shape %s' % (n, a.shape))
        if a.dtype != np.uint8:
            a = a.astype(np.float32)
        es = a.dtype.itemsize
        row = a.shape[1] * a.shape[2] * es
        align = max(int(row_align), es)
        stride = (row + align - 1) // align * align
        if es == 4 and stride % 4:
            stride = (stride + 3) // 4 * 4
        at = (at + 15) // 16 * 16
        table[n] = (at, stride, a.shape[0], a.shape[1], a.shape[2], 1 if es == 4 else 0)
        arrays.append(a)
        at += stride * a.shape[0]
    host = torch.zeros(max(at, 1), dtype=torch.uint8)
    if device.type == 'cuda':
        host = host.pin_memory()
    flat = host.numpy()
    for a, t in zip(arrays, table):
        rows = flat[t['offset']:t['offset'] + t['stride'] * t['height']].reshape(t['height'], t['stride'])
        rows[:, :a.shape[1] * a.shape[2] * a.dtype.itemsize] = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)
    return host.to(device, non_blocking=True), table


def crop_box(center, scale, rot, res):
    """The reference's integer box (imutils.py:73-85): (ul [2], br [2], pad) with the pad already 0 at rot == 0."""
    from ..utils import imutils
    ul = np.array(imutils.transform([1, 1], center, scale, [res, res], invert=1)) - 1
    br = np.array(imutils.transform([res + 1, res + 1], center, scale, [res, res], invert=1)) - 1
    pad = int(np.linalg.norm(br - ul) / 2 - float(br[1] - ul[1]) / 2)
    return ul, br, (pad if not rot == 0 else 0)


def crop_records(table, center, scale, rot, flip, pn, res) -> np.ndarray:
    """The per-sample records of tuch_crop_batch, built in float64 on the host: table [B] (IMAGE_TABLE, sample b crops
    image table[b]), center [B,2], scale [B], rot [B] in degrees, flip [B], pn [B,3] or None (ones), res = R.
    The box is the reference's integer box; the integer affine carries CROP_FRAC_BITS fractional bits (see
    include/tuch_amd.h).  A box without area raises ValueError, as the reference's array of negative size does."""
    res = int(res)
    if not 1 <= res <= CROP_MAX_RES:
        raise ValueError('res must be in [1, %d]' % CROP_MAX_RES)
    table = np.atleast_1d(np.asarray(table, IMAGE_TABLE))
    b = table.shape[0]
    center = np.asarray(center, np.float64).reshape(b, 2)
    scale = np.asarray(scale, np.float64).reshape(b)
    rot = np.asarray(rot, np.float64).reshape(b)
    flip = np.asarray(flip).reshape(b)
    pn = np.ones((b, 3), np.float64) if pn is None else np.asarray(pn, np.float64).reshape(b, 3)
    rec = np.zeros(b, CROP_RECORD)
    for k in ('offset', 'stride', 'height', 'width', 'channels', 'type'):
        rec[k] = table[k]
    one = float(1 << CROP_FRAC_BITS)
    for n in range(b):
        ul, br, p = crop_box(center[n], scale[n], rot[n], res)
        bw, bh = int(br[0] - ul[0]), int(br[1] - ul[1])
        if bw <= 0 or bh <= 0:
            raise ValueError('sample %d: the box has no area (%d x %d)' % (n, bw, bh))
        pw, ph = bw + 2 * p, bh + 2 * p
        ox, oy = int(ul[0]) - p, int(ul[1]) - p
        if max(pw, ph, abs(ox), abs(oy)) > _CROP_LIMIT:
            raise ValueError('sample %d: the box is out of range' % n)
        k = min(max(-(-max(bw, bh) // res), 1), CROP_MAX_K)
        if rot[n] == 0:
            cs, sn = 1.0, 0.0
        else:
            cs, sn = np.cos(np.deg2rad(rot[n])), np.sin(np.deg2rad(rot[n]))
        cx, cy = pw / 2.0, ph / 2.0
        sx, sy = bw / (2.0 * k * res), bh / (2.0 * k * res)           # box units per grid step
        ax = (cs * sx, -sn * sy, cs * (p - cx) - sn * (p - cy) + cx - 0.5)
        ay = (sn * sx, cs * sy, sn * (p - cx) + cs * (p - cy) + cy - 0.5)
        half = 1 << (CROP_FRAC_BITS - 16 - 1)                        # round to the nearest 2^-16 px
        rec['ax'][n] = [int(np.rint(ax[0] * one)), int(np.rint(ax[1] * one)), int(np.rint(ax[2] * one)) + half]
        rec['ay'][n] = [int(np.rint(ay[0] * one)), int(np.rint(ay[1] * one)), int(np.rint(ay[2] * one)) + half]
        rec['pw'][n], rec['ph'][n], rec['ox'][n], rec['oy'][n] = pw, ph, ox, oy
        rec['K'][n], rec['flip'][n] = k, 1 if flip[n] else 0
        rec['pn'][n] = pn[n]
    return rec


def check_crop_records(records: np.ndarray, buffer_bytes: int, channels: int) -> None:
    """Every image of every record lies inside the packed buffer and every field is in range, or ValueError: what the
    kernel may address is decided here, on the host, before anything is launched."""
    r = records
    if r.dtype != CROP_RECORD or r.ndim != 1:
        raise ValueError('records must be a 1-D CROP_RECORD array (crop_records)')
    es = np.where(r['type'] == 1, 4, 1).astype(np.int64)
    row = r['width'].astype(np.int64) * r['channels'] * es
    end = r['offset'] + (r['height'].astype(np.int64) - 1) * r['stride'] + row
    bad = ~np.isin(r['type'], (0, 1)) | ~np.isin(r['channels'], (1, 3)) | ((r['channels'] == 3) & (channels != 3))
    bad |= (r['K'] < 1) | (r['K'] > CROP_MAX_K) | (r['height'] < 1) | (r['width'] < 1) | (r['pw'] < 1) | (r['ph'] < 1)
    bad |= (r['pw'] > _CROP_LIMIT) | (r['ph'] > _CROP_LIMIT) | (np.abs(r['ox']) > _CROP_LIMIT) | (np.abs(r['oy']) > _CROP_LIMIT)
    bad |= (r['offset'] < 0) | (r['stride'] < row) | (r['stride'] > (1 << 40)) | (r['offset'] > (1 << 60))
    bad |= (r['type'] == 1) & (((r['offset'] | r['stride']) & 3) != 0)
    bad |= (end < 0) | (end > int(buffer_bytes))
    if bad.any():
        n = int(np.argmax(bad))
        raise ValueError('crop record %d is out of range or addresses outside the packed buffer of %d bytes: %r'
                         % (n, buffer_bytes, r[n]))


class DeviceCropRecords:
    """Records that were checked against a buffer and uploaded (upload_crop_records): crop_batch launches on them without
    touching the host -- what a captured graph needs."""

    def __init__(self, tensor, count, buffer_bytes, channels_checked):
        self.tensor, self.count, self.buffer_bytes, self.channels_checked = tensor, count, buffer_bytes, channels_checked


def upload_crop_records(buffer: torch.Tensor, records: np.ndarray, channels: int = 3) -> DeviceCropRecords:
    check_crop_records(records, buffer.numel() * buffer.element_size(), channels)
    host = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1).copy())
    if buffer.is_cuda:
        host = host.pin_memory()
    return DeviceCropRecords(host.to(buffer.device, non_blocking=True), int(records.shape[0]),
                             buffer.numel() * buffer.element_size(), int(channels))


def crop_batch(buffer: torch.Tensor, records, res: int, mean, std, raw: bool = False):
    """tuch_crop_batch (include/tuch_amd.h): buffer = pack_images' device tensor, records = crop_records' array (checked
    against the buffer and uploaded here) or upload_crop_records' object, mean / std = one float per output channel (1 or
    3) -> out [B,C,R,R] float32 = (raw - mean) / std, and with raw=True also raw [B,C,R,R] in [0,1].  One launch on the
    current stream; with uploaded records nothing else: capturable."""
    mean = [float(x) for x in np.asarray(mean, np.float64).reshape(-1)]
    std = [float(x) for x in np.asarray(std, np.float64).reshape(-1)]
    ch = len(mean)
    if ch not in (1, 3) or len(std) != ch:
        raise ValueError('mean and std need 1 or 3 entries each')
    if not buffer.is_cuda or buffer.dtype != torch.uint8 or buffer.dim() != 1:
        raise _C.TuchError('crop_batch needs the 1-D uint8 device buffer of pack_images')
    res = int(res)
    if not 1 <= res <= CROP_MAX_RES:
        raise ValueError('res must be in [1, %d]' % CROP_MAX_RES)
    with torch.cuda.device(buffer.device):
        if not isinstance(records, DeviceCropRecords):
            records = upload_crop_records(buffer, records, ch)
        if records.buffer_bytes != buffer.numel() or (records.channels_checked != ch and ch != 3):
            raise ValueError('these records were checked against another buffer or channel count')
        b = records.count
        out = torch.empty(b, ch, res, res, dtype=torch.float32, device=buffer.device)
        raw_out = torch.empty_like(out) if raw else None
        fl = ctypes.c_float * ch
        _C.check(_C.lib().tuch_crop_batch(_C.ptr(buffer), buffer.numel(), _C.ptr(records.tensor) if b else _C.ptr(None), b, res,
                                          ch, fl(*mean), fl(*std), _C.ptr(out), _C.ptr(raw_out), _C.stream()))
    return (out, raw_out) if raw else out
