"""Drop-in for the reference's ``tuch/utils/smplxtosmpl_mtp.py``: turn the MTP dataset's SMPL-X pseudo ground truth into
the SMPL parameters training consumes.

Same behaviour: every ``**/*.pkl`` under ``folder`` whose ``/smplx/`` -> ``/smpl/`` twin does not exist yet is read
(``vertices``, ``body_pose``, ``global_orient``), its SMPL-X vertices are mapped onto SMPL topology with the sparse
[6890 x 10475] matrix (:58), SMPL's ``body_pose``, ``betas`` and ``transl`` are fitted to them with Adam at lr 1e-2
(:78-105) from the SMPL-X body pose padded with six zeros (:64), and ``{'pose': float64 [72], 'betas': float64 [10]}`` is
written to the twin path.  Differences:
  * the two hard-coded cluster paths (:38,:43) are arguments: ``smpl`` (a tuch_amd.models.smpl.SMPL, default: built from
    ``config_path('SMPL_MODEL_DIR')``) and ``smplx_to_smpl`` (the matrix, a path to the pickle that holds it under
    'matrix', default ``config_path('SMPLX_TO_SMPL')``); a missing file raises FileNotFoundError;
  * files are processed ``batch_size`` at a time on the device (ops.mesh_transfer, fit.MeshFitter) instead of one by one
    on the host; the last chunk is padded by repeating its last body, so one captured loop serves every chunk, and the
    padded bodies are not written.
"""
from __future__ import annotations

import argparse
import glob
import os
import os.path as osp
import pickle

import numpy as np
import torch


def _transfer_matrix(smplx_to_smpl):
    from ..assets import config_path
    if smplx_to_smpl is None:
        smplx_to_smpl = config_path('SMPLX_TO_SMPL')
    if isinstance(smplx_to_smpl, (str, os.PathLike)):
        if not osp.exists(smplx_to_smpl):
            raise FileNotFoundError('the SMPL-X -> SMPL transfer matrix %s does not exist (smplx_to_smpl=...)' % smplx_to_smpl)
        with open(smplx_to_smpl, 'rb') as f:
            smplx_to_smpl = pickle.load(f, encoding='latin1')
    return smplx_to_smpl['matrix'] if isinstance(smplx_to_smpl, dict) else smplx_to_smpl          # :43-44


def _body_model(smpl, batch_size):
    if smpl is not None:
        return smpl
    from ..assets import config_path
    from ..models.smpl import SMPL
    model_dir = config_path('SMPL_MODEL_DIR')
    if not osp.exists(model_dir):
        raise FileNotFoundError('the SMPL model directory %s does not exist (smpl=...)' % model_dir)
    return SMPL(model_dir, batch_size=batch_size, create_transl=False)


def SMPLXtoSMPL(folder, sidx=None, cbs=None, smpl=None, smplx_to_smpl=None, batch_size=64, max_iterations=5000):
    """Convert the SMPL-X fits under ``folder`` to SMPL parameters.  sidx, cbs: start index and batch size of a cluster
    job (files sidx * cbs ... sidx * cbs + cbs - 1 of the list, :45-50).  Returns the paths written."""
    from .. import ops
    from ..fit import MeshFitter
    dataset_files = glob.glob(osp.join(folder, '**', '*.pkl'), recursive=True)
    dataset_files = [x for x in dataset_files if not osp.exists(x.replace('/smplx/', '/smpl/'))]
    dataset_size = len(dataset_files)
    print(f'Processing {dataset_size} files ...')
    smpl = _body_model(smpl, batch_size)
    table = ops.transfer_table(_transfer_matrix(smplx_to_smpl))
    if not torch.cuda.is_available():
        raise RuntimeError('SMPLXtoSMPL fits on a HIP device; none is visible (there is no host fallback)')
    device = torch.device('cuda', torch.cuda.current_device())
    if sidx is None:
        todo = dataset_files
    else:
        sidx, cbs = int(sidx), int(cbs)
        todo = [dataset_files[i] for i in range(sidx * cbs, sidx * cbs + cbs)]
    fitter = MeshFitter(smpl, step_size=1e-2, num_iters=max_iterations)
    written = []
    for start in range(0, len(todo), batch_size):
        paths = todo[start:start + batch_size]
        datasets = []
        for path in paths:
            with open(path, 'rb') as f:
                datasets.append(pickle.load(f))
        datasets += [datasets[-1]] * (batch_size - len(paths))
        rows = lambda key, width: torch.from_numpy(np.stack(
            [np.asarray(d[key], np.float32).reshape(-1)[:width] for d in datasets])).to(device)
        smplx_vertices = torch.from_numpy(np.stack([np.asarray(d['vertices'], np.float32).reshape(-1, 3)
                                                    for d in datasets])).to(device)
        global_orient = rows('global_orient', 3)
        body_pose = torch.cat([rows('body_pose', 63), torch.zeros(batch_size, 6, device=device)], 1)       # :64
        target = ops.mesh_transfer(table, smplx_vertices)                                                  # :58
        fit = fitter(target, global_orient, body_pose=body_pose)
        pose = torch.cat([fit.global_orient, fit.body_pose], 1).cpu().numpy().astype(np.float64)           # :115
        betas = fit.betas.cpu().numpy().astype(np.float64)
        for i, path in enumerate(paths):
            path_out = path.replace('/smplx/', '/smpl/')
            print(path_out)
            os.makedirs(osp.dirname(path_out), exist_ok=True)
            with open(path_out, 'wb') as f:
                pickle.dump({'pose': pose[i], 'betas': betas[i]}, f)
            written.append(path_out)
    return written


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument('--folder', required=True, help='path to pt file to be processed')
    parser.add_argument('--idx', required=False, default=None, help='process single index of pt file')
    parser.add_argument('--cbs', required=False, default=None, help='batch size for cluster jobs')
    args = parser.parse_args()
    SMPLXtoSMPL(args.folder, args.idx, args.cbs)
