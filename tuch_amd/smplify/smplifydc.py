"""Drop-in for the reference's ``tuch/smplify/smplifydc.py``: the SMPLify-DC optimiser.

Same constructor and ``__call__`` signature / 7-tuple return as the reference
(smplifydc.py:27-276).  Differences, all behind the interface:
  * the assets the reference loads from disk inside ``__init__`` (SMPL .pkl, GMM prior,
    constants.JOINT_IDS) may be injected (``smpl=``, ``pose_prior=``, ``ign_joints=``) because
    they do not ship; with the licensed files present the reference's paths are used;
  * the device follows the inputs (the reference hard-codes 'cuda');
  * the contact term of every iteration is one batched pass over the HIP kernels.

One driver (``__call__``): get a session for the call's constants (static tensors, the three iteration closures, the two
loops), copy the inputs into it, run stage 1, run stage 2, evaluate, return clones.  The loops are run by the package's one
loop runner (``fit_loop.Stage``; its three modes and its one fallback are described there), and the loop settings, the
call prelude and the kept sessions are ``fit_loop.LoopOwner``'s, shared with the fitters of ``tuch_amd/fit.py``.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .losses import body_fitting_loss, camera_fitting_loss, contact_model_for, stage2_objective
from .prior import MaxMixturePrior
from ..fit_loop import LoopOwner, Stage

# smplifydc.py:46-47: joints ignored during the fit, by name; resolved through constants.JOINT_IDS when the
# data folder is importable, else through SPIN's published table (models/smpl.py) -> [1, 9, 12, 27, 28]
IGNORED_JOINT_NAMES = ['OP Neck', 'OP RHip', 'OP LHip', 'Right Hip', 'Left Hip']


def default_ignored_joints():
    from ..models.smpl import spin_joint_ids
    ids = spin_joint_ids()
    return [ids[n] for n in IGNORED_JOINT_NAMES]


class SMPLifyDC(LoopOwner):
    """SMPLify with discrete self-contact: stage 1 fits camera translation (+ betas when contact is
    used), stage 2 fits pose and global orientation against the contact objective."""

    def __init__(self,
                 step_size=1e-2,
                 batch_size=66,
                 num_iters=100,
                 focal_length=5000,
                 geodistssmpl=None,
                 geothres=0.0,
                 euclthres=0.0,
                 device=torch.device('cuda'),
                 smpl=None, pose_prior=None, ign_joints=None,
                 smpl_model_dir=None, prior_folder=None, use_graph=True, record_history=False):
        from ..assets import config_path
        self.device = device
        self.focal_length = focal_length
        # (record_history is not in the reference: self.history = {'stage1': [...], 'stage2': [...]}; sessions are keyed
        # by batch size and the call's constant arguments)
        self._init_loops(step_size, num_iters, use_graph, record_history)
        self.ign_joints = list(default_ignored_joints() if ign_joints is None else ign_joints)
        self._ign_index = {}          # device -> index tensor (a Python list index is re-uploaded on every use)
        if pose_prior is None:             # smplifydc.py:50-52
            pose_prior = MaxMixturePrior(prior_folder=prior_folder or config_path('PRIOR_FOLDER'),
                                         num_gaussians=8, dtype=torch.float32)
        self.pose_prior = pose_prior.to(device)
        if smpl is None:                   # smplifydc.py:54-56
            from ..models.smpl import SMPL
            smpl = SMPL(smpl_model_dir or config_path('SMPL_MODEL_DIR'), batch_size=batch_size,
                        create_transl=False)
        self.smpl = smpl.to(self.device)
        self.face_tensor = torch.tensor(self.smpl.faces.astype(np.int64), dtype=torch.long,
                                        device=self.device).unsqueeze_(0).repeat([batch_size, 1, 1])
        self.geodistssmpl = geodistssmpl
        self.geothres = geothres
        self.geomask = self.geodistssmpl > self.geothres            # smplifydc.py:65 (strict >)
        self.euclthres = euclthres
        self.fused_adam = os.environ.get('TUCH_FUSED_ADAM', '1') != '0'      # 0: Adam as a launch of its own (A/B, tests)

    _Stage = Stage            # (the name the benchmark's comments and older notes use)

    def _session(self, batch, use_contact, contactlist, segments, contact_loss_weight, with_pairs, like):
        """(key, session) of a fit with these constants: the stored one, or a new one (``_build``)."""
        # everything a captured loop bakes in: the tables (the session keeps them alive, so their ids cannot be reused by
        # other objects) and the fitter's own settings -- changing one of those after a call starts a new session
        key = (batch, bool(use_contact), id(contactlist), id(segments), float(contact_loss_weight), bool(with_pairs),
               float(self.step_size), float(self.euclthres), float(self.focal_length), tuple(self.ign_joints),
               id(self.pose_prior), int(self.num_iters), bool(self.record_history), bool(self.fused_adam))
        return key, self._session_for(key, self._build, batch, use_contact, contactlist, segments, contact_loss_weight,
                                      with_pairs, like.device)

    def _build(self, batch, use_contact, contactlist, segments, contact_loss_weight, with_pairs, dev):
        """A session: the static tensors, the three iteration closures and the two loops."""
        f32 = torch.float32
        z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype, device=dev)
        t = dict(body_pose=z(batch, 69), global_orient=z(batch, 3), betas=z(batch, 10), cam=z(batch, 3), init_cam=z(batch, 3),
                 centre=z(batch, 2), j2d=z(batch, 49, 2), conf1=z(batch, 49), conf2=z(batch, 49),
                 valid=z(batch, dtype=torch.uint8))
        model = None
        if use_contact:
            model = contact_model_for(self.geomask, self.face_tensor, segments, contactlist, device=dev)
            t['select'] = z(batch, model.num_pairs, dtype=torch.uint8) if (with_pairs and model.num_pairs > 0) else None
        body_pose, global_orient, betas, cam = t['body_pose'], t['global_orient'], t['betas'], t['cam']
        spw = 1.0 if use_contact else 0.0

        def camera_iteration():
            out = self.smpl(global_orient=global_orient, body_pose=body_pose, betas=betas)
            return camera_fitting_loss(out, cam, t['init_cam'], t['centre'], t['j2d'], t['conf1'],
                                       focal_length=self.focal_length, shape_prior_weight=spw), out.vertices

        def contact_iteration():
            out = self.smpl(global_orient=global_orient, body_pose=body_pose, betas=betas)
            loss = stage2_objective(model, t['valid'], t['select'], body_pose, betas, out.joints, self.euclthres, cam,
                                    t['centre'], t['j2d'], t['conf2'], self.pose_prior, out.vertices,
                                    focal_length=self.focal_length, contact_loss_weight=contact_loss_weight,
                                    apply_segments=segments is not None)
            return loss, out.vertices

        def body_iteration():
            out = self.smpl(global_orient=global_orient, body_pose=body_pose, betas=betas)
            return body_fitting_loss(body_pose, betas, out.joints, cam, t['centre'], t['j2d'], t['conf2'], self.pose_prior,
                                     focal_length=self.focal_length), out.vertices

        def flags(bp, go, be, ct):
            body_pose.requires_grad, global_orient.requires_grad, betas.requires_grad, cam.requires_grad = bp, go, be, ct
        # stage 1 optimises [betas, cam] with contact, [global_orient, cam] without (smplifydc.py:104-117); stage 2 is built
        # by the first call, once its flags are set
        stage1_flags = (False, not use_contact, bool(use_contact), True)
        flags(*stage1_flags)
        sess = dict(t=t, flags=flags, stage1_flags=stage1_flags, stage2=None, keys_alive=(contactlist, segments, self.pose_prior),
                    stage1=Stage(self, 'stage1', [betas, cam] if use_contact else [global_orient, cam], camera_iteration,
                                 dict(betas=(0.9, 0.999))))
        if use_contact:
            sess['stage2_flags'] = (True, True, False, False)
            sess['make_stage2'] = lambda: Stage(self, 'stage2', [body_pose, global_orient], contact_iteration, {},
                                                fuse_backward=self.fused_adam)
        else:
            sess['stage2_flags'] = (True, True, True, False)
            sess['make_stage2'] = lambda: Stage(self, 'stage2', [body_pose, betas, global_orient], body_iteration,
                                                dict(betas=(0.9, 0.999)))
        return sess

    def __call__(self, init_pose, init_betas, init_cam_t,
                 camera_center, keypoints_2d, use_contact=False,
                 contactlist=[], gt_contact=None,
                 ignore_idxs=None, has_discrete_contact=None,
                 has_gt_keypoints=None, contact_loss_weight=1,
                 contact_loss_return='sum', segments=None):
        """Fit a batch of bodies.  Returns (vertices, joints, pose, betas, camera_translation,
        reprojection_loss, optiverts) exactly like the reference (smplifydc.py:231-236)."""
        if use_contact and ignore_idxs is None:
            raise ValueError('SMPLifyDC: use_contact=True needs ignore_idxs, a [B] bool tensor (all False: every body gets '
                             'contact terms)')
        with self._loops(init_pose.device, self.use_graph and init_pose.is_cuda, 'stage1', 'stage2') as capture:
            with_pairs = gt_contact is not None and gt_contact[0] is not None
            key, sess = self._session(init_pose.shape[0], use_contact, contactlist, segments, contact_loss_weight, with_pairs,
                                      init_pose)
            t = sess['t']
            with torch.no_grad():
                put = lambda dst, src: dst.copy_(src)
                put(t['body_pose'], init_pose[:, 3:]); put(t['global_orient'], init_pose[:, :3]); put(t['betas'], init_betas)
                put(t['cam'], init_cam_t); put(t['init_cam'], init_cam_t); put(t['centre'], camera_center)
                put(t['j2d'], keypoints_2d[:, :, :2]); put(t['conf1'], keypoints_2d[:, :, -1])
                put(t['conf2'], keypoints_2d[:, :, -1])
                t['conf2'].index_fill_(1, self._ignored(t['conf2'].device), 0.0)                                     # smplifydc.py:153,198
                if use_contact:
                    put(t['valid'], ~ignore_idxs)
                    if t.get('select') is not None:
                        put(t['select'], (gt_contact[0] == 1) & has_discrete_contact.bool()[:, None] & (~ignore_idxs)[:, None])
            # ---- stage 1: camera translation (+ shape with contact, + orientation without)
            sess['flags'](*sess['stage1_flags'])
            capture = sess['stage1'].run(self.num_iters, None, capture)
            # ---- stage 2: pose + global orientation (+ shape without contact)
            sess['flags'](*sess['stage2_flags'])
            if sess['stage2'] is None:
                sess['stage2'] = sess['make_stage2']()
            optiverts = []
            capture = sess['stage2'].run(self.num_iters, optiverts, capture)
            self._settle(key, sess, capture)
            # ---- final evaluation
            with torch.no_grad():
                out = self.smpl(global_orient=t['global_orient'], body_pose=t['body_pose'], betas=t['betas'], return_full_pose=True)
                conf = t['conf2'].clone()
                if has_gt_keypoints is not None:                                         # smplifydc.py:219-220, no host sync
                    conf[:, :25] = torch.where(has_gt_keypoints.bool()[:, None], torch.zeros_like(conf[:, :25]), conf[:, :25])
                reprojection_loss = body_fitting_loss(t['body_pose'], t['betas'], out.joints, t['cam'], t['centre'], t['j2d'], conf,
                                                      self.pose_prior, focal_length=self.focal_length, output='reprojection')
            pose = torch.cat([t['global_orient'], t['body_pose']], dim=-1).detach().clone()
            return (out.vertices.detach(), out.joints.detach(), pose, t['betas'].detach().clone(), t['cam'].detach().clone(),
                    reprojection_loss, optiverts if optiverts else None)

    def _ignored(self, device):
        """ign_joints as an index tensor on `device`."""
        idx = self._ign_index.get(device)
        if idx is None:
            idx = self._ign_index[device] = torch.tensor(self.ign_joints, dtype=torch.int64, device=device)
        return idx

    def get_fitting_loss(self, pose, betas, cam_t, camera_center, keypoints_2d, has_gt_keypoints=None):
        """Per-joint reprojection loss of given parameters (reference: smplifydc.py:238-276;
        like the reference, zeroing the ignored joints writes through into ``keypoints_2d``)."""
        joints_2d = keypoints_2d[:, :, :2]
        joints_conf = keypoints_2d[:, :, -1]
        joints_conf.index_fill_(1, self._ignored(joints_conf.device), 0.0)
        if has_gt_keypoints is not None:
            joints_conf = joints_conf.clone()
            joints_conf[has_gt_keypoints, :25] = 0
        with torch.no_grad():
            out = self.smpl(global_orient=pose[:, :3], body_pose=pose[:, 3:], betas=betas,
                            return_full_pose=True)
            return body_fitting_loss(pose[:, 3:], betas, out.joints, cam_t, camera_center, joints_2d,
                                     joints_conf, self.pose_prior, focal_length=self.focal_length,
                                     output='reprojection')
