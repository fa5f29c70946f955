"""Pose evaluation on the device: MPJPE, PA-MPJPE (reconstruction error) and v2v in one kernel per batch.

The reference computes these on the host (eval.py:158-195: a .cpu() per batch and one np.linalg.svd per body) or
with a chain of torch ops over the concatenated validation set (trainer.py:229-267).  Here:

    out = pose_errors(pred_vertices, J_regressor, joint_map, gt_vertices=gt_vertices)
    # {'mpjpe': [B], 'pa_mpjpe': [B], 'v2v': [B]} float32 device tensors, metres

    ev = Evaluator(J_regressor, H36M_TO_J14, capacity=len(dataset))
    for batch in loader:
        ev.add(pred_vertices, gt_vertices=gt_vertices)        # no host synchronisation
    ev.summary(cnc=cnc_arr)                                   # what print_final_result prints, millimetres

    ev = Evaluator(..., contact=SelfContact(geodists))        # contact_detect.py: cnc of the gt vertices recorded by add()
    ev.summary()                                              # ... and the contact / no-contact / unclear split from it

One launch of tuch_pose_metrics (csrc/pose_eval.hip) per call: the H36M joints of pred (and gt) are regressed with
every entry of the regressor, the pelvis (row pelvis_index) is subtracted before the joint map, and the aligned error
comes from the same Procrustes device function as tuch_amd.utils.pose_utils.  With gt_joints instead of gt_vertices
(the mpi-inf-3dhp branch, eval.py:168-170) the ground truth is used as given and there is no v2v.
"""
from __future__ import annotations

import numpy as np
import torch

MAX_REGRESSED_JOINTS = 24
MAX_MAPPED_JOINTS = 64


def _as_regressor(J_regressor, device):
    """[R, V] float32, contiguous, on `device` (no copy when it already is)."""
    r = torch.as_tensor(J_regressor)
    if r.dim() != 2:
        raise ValueError('J_regressor must be [R, V], got shape %s' % (tuple(r.shape),))
    if not 0 < r.shape[0] <= MAX_REGRESSED_JOINTS or r.shape[1] == 0:
        raise ValueError('J_regressor [R, V] needs 1 <= R <= %d and V > 0, got %s'
                         % (MAX_REGRESSED_JOINTS, tuple(r.shape)))
    if not r.is_floating_point():
        raise TypeError('J_regressor must be floating point, got %s' % r.dtype)
    if device is not None:
        r = r.to(device=device, dtype=torch.float32)
    return r.to(torch.float32).contiguous()


def _as_joint_map(joint_map, R, device):
    """[J] int32 on `device`; host maps are range-checked here (device maps are taken as they are: an entry outside
    [0, R) gives NaN for the bodies, the kernel never reads out of bounds)."""
    if torch.is_tensor(joint_map) and joint_map.is_cuda:
        m = joint_map
    else:
        a = np.asarray(joint_map)
        if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError('joint_map must be a non-empty 1-D sequence of integers')
        if a.min() < 0 or a.max() >= R:
            raise ValueError('joint_map entries must lie in [0, %d), got [%d, %d]' % (R, a.min(), a.max()))
        m = torch.as_tensor(a.astype(np.int32))
    if m.dim() != 1 or not 0 < m.shape[0] <= MAX_MAPPED_JOINTS:
        raise ValueError('joint_map must have 1 to %d entries, got shape %s' % (MAX_MAPPED_JOINTS, tuple(m.shape)))
    if device is not None:
        m = m.to(device)
    return m.to(torch.int32).contiguous()


def _check_batch(pred_vertices, gt_vertices, gt_joints, V, J):
    if not torch.is_tensor(pred_vertices) or pred_vertices.dim() != 3 or pred_vertices.shape[2] != 3:
        raise ValueError('pred_vertices must be a [B, V, 3] tensor')
    if pred_vertices.dtype != torch.float32:
        raise TypeError('pred_vertices must be float32, got %s' % pred_vertices.dtype)
    B = pred_vertices.shape[0]
    if pred_vertices.shape[1] != V:
        raise ValueError('pred_vertices has %d vertices, the regressor %d' % (pred_vertices.shape[1], V))
    if (gt_vertices is None) == (gt_joints is None):
        raise ValueError('give exactly one of gt_vertices and gt_joints')
    gt = gt_vertices if gt_vertices is not None else gt_joints
    want = (B, V, 3) if gt_vertices is not None else (B, J, 3)
    if not torch.is_tensor(gt) or tuple(gt.shape) != want:
        raise ValueError('%s must be a tensor of shape %s, got %s'
                         % ('gt_vertices' if gt_vertices is not None else 'gt_joints', want,
                            tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__))
    if gt.dtype != torch.float32:
        raise TypeError('ground truth must be float32 like pred_vertices, got %s' % gt.dtype)
    if gt.device != pred_vertices.device:
        raise ValueError('pred and ground truth are on different devices')
    return B


def _launch(pred, gt_vertices, gt_joints, reg, jmap, pelvis_index, mpjpe, pa, v2v, joints):
    from . import _C
    if not pred.is_cuda:
        raise RuntimeError('tuch_amd.eval runs on a HIP device (there is no host fallback); got tensors on %s'
                           % pred.device)
    B, V, _ = pred.shape
    R, J = reg.shape[0], jmap.shape[0]
    p = pred.detach().contiguous()
    gv = gt_vertices.detach().contiguous() if gt_vertices is not None else None
    gj = gt_joints.detach().contiguous() if gt_joints is not None else None
    with torch.cuda.device(p.device):
        _C.check(_C.lib().tuch_pose_metrics(_C.ptr(p), _C.ptr(gv), _C.ptr(gj), _C.ptr(reg), _C.ptr(jmap), B, V, R, J,
                                            int(pelvis_index), _C.ptr(mpjpe), _C.ptr(pa), _C.ptr(v2v), _C.ptr(joints),
                                            _C.stream()))


def pose_errors(pred_vertices, J_regressor, joint_map, gt_vertices=None, gt_joints=None, pelvis_index=0,
                return_joints=False):
    """Per-body errors of one batch, in one kernel launch (capturable in a torch.cuda.graph when J_regressor and
    joint_map are already device tensors: float32 [R, V] and int32 [J]).

    pred_vertices [B, V, 3] float32; exactly one of gt_vertices [B, V, 3] or gt_joints [B, J, 3] (mpi-inf-3dhp: used as
    given, no pelvis subtracted).  Returns a dict of float32 device tensors, metres:
        'mpjpe' [B], 'pa_mpjpe' [B], 'v2v' [B] (only with gt_vertices), 'joints' [B, R, 3] (only with return_joints:
        the regressed pred joints before the pelvis is subtracted, eval.py:184)."""
    dev = pred_vertices.device if torch.is_tensor(pred_vertices) and pred_vertices.is_cuda else None
    reg = _as_regressor(J_regressor, dev)
    if not 0 <= pelvis_index < reg.shape[0]:
        raise ValueError('pelvis_index %d not in [0, %d)' % (pelvis_index, reg.shape[0]))
    jmap = _as_joint_map(joint_map, reg.shape[0], dev)
    B = _check_batch(pred_vertices, gt_vertices, gt_joints, reg.shape[1], jmap.shape[0])
    kw = dict(dtype=torch.float32, device=pred_vertices.device)
    out = {'mpjpe': torch.empty(B, **kw), 'pa_mpjpe': torch.empty(B, **kw)}
    if gt_vertices is not None:
        out['v2v'] = torch.empty(B, **kw)
    if return_joints:
        out['joints'] = torch.empty(B, reg.shape[0], 3, **kw)
    if B:
        _launch(pred_vertices, gt_vertices, gt_joints, reg, jmap, pelvis_index, out['mpjpe'], out['pa_mpjpe'],
                out.get('v2v'), out.get('joints'))
    return out


def pose_summary(mpjpe, recon_err, cnc=None, euclthres_lower=0.01):
    """The numbers print_final_result prints (eval.py:75-89), millimetres, from per-body errors in metres.

    Keys: 'mpjpe', 'recon_err'; with cnc (the per-body minimum contact signature distance, eval.py:135-136) also
    'n_contact', 'n_no_contact', 'n_unclear' and 'mpjpe_contact', 'mpjpe_no_contact', 'mpjpe_unclear',
    'recon_err_contact', 'recon_err_no_contact', 'recon_err_unclear'.  contact: cnc < euclthres_lower; no contact:
    cnc == inf; unclear: the rest.  The mean of an empty subset is NaN, as numpy's."""
    mpjpe = np.asarray(mpjpe, dtype=np.float64)
    recon_err = np.asarray(recon_err, dtype=np.float64)

    def mm(a):
        return float(1000 * a.mean()) if a.size else float('nan')

    out = {'mpjpe': mm(mpjpe), 'recon_err': mm(recon_err)}
    if cnc is None:
        return out
    cnc = np.asarray(cnc)
    if cnc.shape != mpjpe.shape:
        raise ValueError('cnc has shape %s, the errors %s' % (cnc.shape, mpjpe.shape))
    contact, no_contact = cnc < euclthres_lower, cnc == np.inf
    unclear = ~(no_contact | contact)
    for name, sel in (('contact', contact), ('no_contact', no_contact), ('unclear', unclear)):
        out['n_' + name] = int(sel.sum())
        out['mpjpe_' + name] = mm(mpjpe[sel])
        out['recon_err_' + name] = mm(recon_err[sel])
    return out


class Evaluator:
    """Per-body errors of a whole evaluation, accumulated on the device.

    The regressor and joint map are prepared on the device once; add() writes each batch's results at a running
    offset (no host synchronisation); results() copies them out; summary() / validation_metrics() reduce them.

    contact: a ``contact_detect.SelfContact``.  add() then also records every body's smallest self-contact distance
    ('cnc': inf = no contact) -- the number eval.py:135-136 reads from a file -- and summary() splits the errors by it."""

    def __init__(self, J_regressor, joint_map, capacity, pelvis_index=0, device=None, return_joints=False, contact=None):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError('tuch_amd.eval.Evaluator needs a HIP device (there is no host fallback)')
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = torch.device(device)
        self.J_regressor = _as_regressor(J_regressor, self.device)
        R = self.J_regressor.shape[0]
        if not 0 <= pelvis_index < R:
            raise ValueError('pelvis_index %d not in [0, %d)' % (pelvis_index, R))
        self.joint_map = _as_joint_map(joint_map, R, self.device)
        self.pelvis_index = int(pelvis_index)
        self.capacity = int(capacity)
        kw = dict(dtype=torch.float32, device=self.device)
        self._mpjpe = torch.full((self.capacity,), float('nan'), **kw)
        self._pa = torch.full((self.capacity,), float('nan'), **kw)
        self._v2v = torch.full((self.capacity,), float('nan'), **kw)
        self._joints = torch.full((self.capacity, R, 3), float('nan'), **kw) if return_joints else None
        self._has_v2v = False
        self.contact = contact
        self._cnc = torch.full((self.capacity,), float('nan'), **kw) if contact is not None else None
        self.count = 0

    def reset(self):
        self._mpjpe.fill_(float('nan'))
        self._pa.fill_(float('nan'))
        self._v2v.fill_(float('nan'))
        if self._joints is not None:
            self._joints.fill_(float('nan'))
        if self._cnc is not None:
            self._cnc.fill_(float('nan'))
        self._has_v2v = False
        self.count = 0

    def add(self, pred_vertices, gt_vertices=None, gt_joints=None, contact_vertices=None):
        """One batch (pose_errors's arguments); returns the slice [start, stop) its bodies were written to.
        With a contact detector: the self-contact distance of contact_vertices [B, V', 3] (default: gt_vertices) is
        recorded beside the errors; a batch with neither leaves NaN."""
        if contact_vertices is not None and self.contact is None:
            raise ValueError('contact_vertices given, but the Evaluator was created without contact=')
        B = _check_batch(pred_vertices, gt_vertices, gt_joints, self.J_regressor.shape[1], self.joint_map.shape[0])
        if pred_vertices.device != self.device:
            raise ValueError('batch on %s, evaluator on %s' % (pred_vertices.device, self.device))
        start = self.count
        if start + B > self.capacity:
            raise ValueError('Evaluator capacity %d exceeded (%d + %d bodies)' % (self.capacity, start, B))
        if B:
            s = slice(start, start + B)
            _launch(pred_vertices, gt_vertices, gt_joints, self.J_regressor, self.joint_map, self.pelvis_index,
                    self._mpjpe[s], self._pa[s], self._v2v[s] if gt_vertices is not None else None,
                    self._joints[s] if self._joints is not None else None)
            if self.contact is not None:
                cv = contact_vertices if contact_vertices is not None else gt_vertices
                if cv is not None:
                    if cv.shape[0] != B:
                        raise ValueError('contact_vertices has %d bodies, the batch %d' % (cv.shape[0], B))
                    self._cnc[s] = self.contact.cnc(cv)
        self._has_v2v |= gt_vertices is not None
        self.count = start + B
        return start, self.count

    def results(self):
        """numpy float32 per-body arrays of the bodies added so far: 'mpjpe', 'pa_mpjpe' (metres), 'v2v' (when any
        batch had gt_vertices; NaN for the bodies of the others), 'joints' [n, R, 3] (with return_joints) and 'cnc'
        (with a contact detector: metres, inf = no contact, NaN for bodies added without vertices to look at)."""
        n = self.count
        out = {'mpjpe': self._mpjpe[:n].cpu().numpy(), 'pa_mpjpe': self._pa[:n].cpu().numpy()}
        if self._has_v2v:
            out['v2v'] = self._v2v[:n].cpu().numpy()
        if self._joints is not None:
            out['joints'] = self._joints[:n].cpu().numpy()
        if self._cnc is not None:
            out['cnc'] = self._cnc[:n].cpu().numpy()
        return out

    def summary(self, cnc=None, euclthres_lower=0.01):
        """pose_summary of the bodies added so far (keys there); cnc defaults to the recorded values when the evaluator
        has a contact detector."""
        r = self.results()
        if cnc is None:
            cnc = r.get('cnc')
        return pose_summary(r['mpjpe'], r['pa_mpjpe'], cnc, euclthres_lower)

    def validation_metrics(self):
        """{'mpjpe', 'v2v'} in millimetres, the means over all bodies as validate_final_step computes them
        (trainer.py:246-254)."""
        r = self.results()
        if 'v2v' not in r:
            raise ValueError('validation_metrics needs batches added with gt_vertices')
        return {'mpjpe': float(np.mean(r['mpjpe'], dtype=np.float64) * 1000),
                'v2v': float(np.mean(r['v2v'], dtype=np.float64) * 1000)}


def validation_metrics(gt_vertices, pred_vertices, J_regressor, joint_mapper):
    """validate_final_step's numbers (trainer.py:229-267): {'mpjpe', 'v2v'} in millimetres over the validation set.
    gt_vertices / pred_vertices: [N, V, 3] tensors, or equally long lists of chunks (the trainer's
    evaluation_accumulators), which are fed to an Evaluator one by one instead of being concatenated."""
    gts = list(gt_vertices) if isinstance(gt_vertices, (list, tuple)) else [gt_vertices]
    preds = list(pred_vertices) if isinstance(pred_vertices, (list, tuple)) else [pred_vertices]
    if len(gts) != len(preds):
        raise ValueError('%d gt chunks, %d pred chunks' % (len(gts), len(preds)))
    dev = preds[0].device if preds and torch.is_tensor(preds[0]) and preds[0].is_cuda else None
    ev = Evaluator(J_regressor, joint_mapper, sum(int(p.shape[0]) for p in preds), device=dev)
    for g, p in zip(gts, preds):
        ev.add(p, gt_vertices=g)
    return ev.validation_metrics()
