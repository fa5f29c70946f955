#!/usr/bin/env python3
"""Timing of the batched crop (csrc/image_crop.hip), DESIGN.md "Regressor input":

    python tools/crop_timing.py                        # one JSON line per row, then a markdown table

Shape: batch 64 of distinct 750 x 1101 RGB uint8 sources, R = 224, boxes of side 112, 224, 448 and 896 px around the
image centre, at rot 0 and 30, every sample with flip and pixel noise drawn as in training.  Per row, in milliseconds:
  * crop:   ops.crop_batch on uploaded records, one launch per call -- HIP events around blocks of --iters back-to-back
            calls after a warm-up, the median of --blocks blocks (device time; the launch overhead of back-to-back calls
            overlaps);
  * floor:  the bytes the call has to move -- B x 3 x R x R x 4 written plus the bytes of the padded boxes that lie
            inside the images, read once -- at the achievable HBM rate (6.3 TB/s);
  * torch:  K = 1 rows only, where the two compute the same thing: affine_grid + grid_sample (bilinear, zeros) + noise,
            clamp, / 255 and normalisation on float32 [B,3,H,W] copies of the same batch PREPARED AHEAD (the uint8 ->
            float32 conversion of 158 MB is not counted), same measurement.  The chain samples the same box up to the
            reference's integer truncation of its corners: it is timed, not compared.
There is no threshold.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from tuch_amd import ops                                        # noqa: E402
from tuch_amd.augment import IMG_NORM_MEAN, IMG_NORM_STD         # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def timed(fn, iters, blocks):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(blocks):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def box_bytes(rec):
    """Bytes of the padded boxes that lie inside their images (what a perfect kernel reads once)."""
    total = 0
    for r in rec:
        w = min(int(r['ox']) + int(r['pw']), int(r['width'])) - max(int(r['ox']), 0)
        h = min(int(r['oy']) + int(r['ph']), int(r['height'])) - max(int(r['oy']), 0)
        total += max(w, 0) * max(h, 0) * int(r['channels']) * (4 if r['type'] else 1)
    return total


def torch_chain(src, theta, pn, mean, std, res):
    grid = torch.nn.functional.affine_grid(theta, (src.shape[0], 3, res, res), align_corners=False)
    v = torch.nn.functional.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    v = (v * pn[:, :, None, None]).clamp_(0.0, 255.0) / 255.0
    return (v - mean[None, :, None, None]) / std[None, :, None, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--res', type=int, default=224)
    ap.add_argument('--height', type=int, default=750)
    ap.add_argument('--width', type=int, default=1101)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('crop_timing.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    b, res, h, w = a.batch, a.res, a.height, a.width
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(b)]
    buf, table = ops.pack_images(images, device=dev)
    center = np.tile([[w / 2.0, h / 2.0]], (b, 1)) + rng.uniform(-20, 20, (b, 2))
    flip = rng.integers(0, 2, b)
    pn = rng.uniform(0.6, 1.4, (b, 3))
    src = torch.stack([torch.as_tensor(im, device=dev).permute(2, 0, 1).float() for im in images]).contiguous()
    mean_t, std_t = torch.tensor(IMG_NORM_MEAN, device=dev), torch.tensor(IMG_NORM_STD, device=dev)
    pn_t = torch.tensor(pn, dtype=torch.float32, device=dev)
    rows = []
    for side in (112, 224, 448, 896):
        for rot in (0.0, 30.0):
            rec = ops.crop_records(table, center, np.full(b, side / 200.0), np.full(b, rot), flip, pn, res)
            dev_rec = ops.upload_crop_records(buf, rec)

            def crop():
                return ops.crop_batch(buf, dev_rec, res, IMG_NORM_MEAN, IMG_NORM_STD)
            for _ in range(5):
                crop()
            torch.cuda.synchronize()
            t = timed(crop, a.iters, a.blocks)
            written, read = b * 3 * res * res * 4, box_bytes(rec)
            row = {'what': 'crop', 'batch': b, 'res': res, 'source': [h, w], 'box': side, 'rot': rot, 'K': int(rec['K'][0]),
                   'crop_ms': round(float(np.median(t)), 4), 'crop_ms_min_max': [round(min(t), 4), round(max(t), 4)],
                   'written_MB': round(written / 1e6, 2), 'read_MB': round(read / 1e6, 2),
                   'floor_ms': round((written + read) / HBM_BYTES_PER_S * 1e3, 4), 'torch_ms': None,
                   'launches_timed': a.iters * a.blocks}
            if int(rec['K'][0]) == 1:
                # the same geometry as a normalised affine map (the box around the centre, turned by rot, mirrored by flip)
                th = np.deg2rad(rot)
                theta = np.zeros((b, 2, 3), np.float32)
                sx = np.where(flip == 1, -1.0, 1.0) * side / w
                theta[:, 0, 0], theta[:, 0, 1] = np.cos(th) * sx, -np.sin(th) * side / w
                theta[:, 1, 0], theta[:, 1, 1] = np.sin(th) * sx * w / h, np.cos(th) * side / h
                theta[:, 0, 2], theta[:, 1, 2] = 2 * center[:, 0] / w - 1, 2 * center[:, 1] / h - 1
                theta_t = torch.tensor(theta, device=dev)

                def chain():
                    return torch_chain(src, theta_t, pn_t, mean_t, std_t, res)
                for _ in range(5):
                    chain()
                torch.cuda.synchronize()
                tt = timed(chain, a.iters, a.blocks)
                row['torch_ms'] = round(float(np.median(tt)), 4)
            rows.append(row)
            print(json.dumps(row), flush=True)
    print('| box | rot | K | crop ms | read MB | floor ms | torch ms |')
    print('|---|---|---|---|---|---|---|')
    for r in rows:
        print('| %d | %g | %d | %.3f | %.1f | %.4f | %s |' % (r['box'], r['rot'], r['K'], r['crop_ms'], r['read_MB'], r['floor_ms'],
                                                             '-' if r['torch_ms'] is None else '%.3f' % r['torch_ms']))


if __name__ == '__main__':
    main()
