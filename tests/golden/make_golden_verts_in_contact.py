#!/usr/bin/env python3
"""Golden vectors for self-contact detection, produced by the REFERENCE'S OWN ``TUCH.get_verts_in_contact``
(tuch/train/train_module.py:93-110) on CPU, called with a stand-in ``self`` that only carries ``geodistssmpl`` (all the
function reads), at the reference's thresholds (configs/config.py:90-91: geothres 0.3, euclthres 0.02).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_verts_in_contact.py

Stubs: those of make_golden_train.py (importing it installs them).  Input: make_body(rings=40, segs=40) -- V = 1602 =
6 x 256 + 66 -- with eight bodies: random_poses(3, 1001), through_pose(2, 7), folded_poses(3, 11), posed with oracle.lbs.
Stored: the vertices, the ``>=`` mask, the regions, and idxs1 / idxs2 per body as ragged arrays.  The script also checks
the reference's sets against a float64 brute force and prints how far the closest row is from the threshold.
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_train as mgt          # noqa: E402  (installs the stubs, puts the reference on sys.path)

import numpy as np                       # noqa: E402
import torch                             # noqa: E402

import golden_io as gio                  # noqa: E402
from oracle import lbs as olbs           # noqa: E402
from synthetic import folded_poses, make_body, random_poses, through_pose      # noqa: E402


def main():
    rings, segs = 40, 40
    body = make_body(rings=rings, segs=segs)
    m = olbs.model_tensors(body)
    parts = [random_poses(3, 1001), through_pose(2, 7), folded_poses(3, 11)]
    bp, go, be = [np.concatenate([np.asarray(p[k], np.float32) for p in parts]) for k in range(3)]
    verts, _ = olbs.smpl_forward(m, torch.tensor(be), torch.tensor(bp), torch.tensor(go))
    verts = verts.to(torch.float32)
    geod = torch.tensor(body.geodesics)
    geothres, euclthres = mgt.ref_config.geothres, mgt.ref_config.euclthres
    stand_in = types.SimpleNamespace(geodistssmpl=geod)
    ref = mgt.ref_train_module.TUCH.get_verts_in_contact(stand_in, verts)

    mask = (geod >= geothres).numpy()
    out = {'rings': np.int64(rings), 'segs': np.int64(segs), 'verts': verts.numpy(), 'geothres': np.float64(geothres),
           'euclthres': np.float64(euclthres)}
    gio.pack_mask(mask, out)
    gio.pack_regions(body.regions, body.region_pairs, out)
    gio.pack_ragged('idxs1', [ref[b][0].numpy() for b in range(len(ref))], out)
    gio.pack_ragged('idxs2', [ref[b][1].numpy() for b in range(len(ref))], out)

    # the reference against a float64 brute force
    closest = np.inf
    for b in range(verts.shape[0]):
        v = verts[b].numpy().astype(np.float64)
        d2 = ((v[:, None, :] - v[None, :, :]) ** 2).sum(-1)
        q = mask & (d2 < euclthres ** 2)
        rows = np.where(q.any(1))[0]
        arg = np.where(q, d2, np.inf).argmin(1)[rows]
        same = np.array_equal(rows, ref[b][0].numpy()) and np.array_equal(arg, ref[b][1].numpy())
        rel = np.abs(d2[mask] / euclthres ** 2 - 1.0).min()
        closest = min(closest, rel)
        print('body %d: %3d vertices in contact, equal to the float64 brute force: %s' % (b, len(rows), same))
    print('closest masked pair to the threshold: %.2e relative in d2' % closest)
    path = os.path.join(HERE, 'verts_in_contact.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, '%.1f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
