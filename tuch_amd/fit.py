"""Fit SMPL to target meshes in correspondence (MeshFitter) and to unregistered points (ScanFitter, at the end of the file).
MeshFitter is the optimisation loop of the reference's ``tuch/utils/smplxtosmpl_mtp.py`` (:63-105), batched and on the device.

The reference fits ``body_pose``, ``betas`` and ``transl`` of ONE body with Adam (lr 1e-2, 5000 iterations) against
``torch.norm(target - verts, dim=2).mean()`` and starts over for every file.  Here a batch of bodies is fitted at once: the
objective is the SUM of the bodies' terms, so every body's gradient -- and with Adam's element-wise update its whole
trajectory -- is that of the reference's batch-1 loop.  One iteration is the body model's forward pass, the data term with
its gradients as one launch (ops.vertex_fit), the backward pass from the cached unit seed (ops.backward_scalar) and Adam as
one launch (optim.make_adam); the loop is run by the package's one loop runner (fit_loop.Stage: three eager
iterations, capture, replay as a hipGraph), and sessions -- the static tensors plus the captured loop -- are kept between
calls like SMPLifyDC's (fit_loop.LoopOwner).  ``TUCH_GRAPH_STRICT`` and ``TUCH_SMPLIFY_SESSIONS`` mean what they mean there.
What the two fitters share -- the body's parameter buffers, their seeding and checks, the result clones -- is BodyFitter.

Constructing needs no device; calling does.  There is no host fallback.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops
from .fit_loop import LoopOwner, Stage

MeshFit = namedtuple('MeshFit', ['global_orient', 'body_pose', 'betas', 'transl', 'vertices', 'loss'])


def _posed(smpl, t):
    """The body model's vertices [B,V,3] (without the translation) at a session's parameter tensors."""
    return smpl(global_orient=t['global_orient'], body_pose=t['body_pose'], betas=t['betas']).vertices


class BodyFitter(LoopOwner):
    """What MeshFitter and ScanFitter share: a body model whose ``body_pose``, ``betas``, ``transl`` (and ``global_orient``
    with ``fit_global_orient``) are fitted by one loop called 'fit'.  With ``record_history`` the objective and the
    parameters *before* every update are kept in ``self.history['fit']``, the parameters in the optimiser's order:
    body_pose, betas, transl (, global_orient)."""

    def __init__(self, smpl, step_size, num_iters, fit_global_orient, use_graph, record_history):
        self.smpl = smpl
        self.fit_global_orient = fit_global_orient
        self._init_loops(step_size, num_iters, use_graph, record_history)

    def _check_shapes(self, *named):
        """Each of ``named`` is (name, tensor or None, the shape it must have)."""
        for name, value, shape in named:
            if value is not None and tuple(value.shape) != shape:
                raise ValueError('%s: %s has shape %s, expected %s' % (type(self).__name__, name, tuple(value.shape), shape))

    def _to_device(self, device):
        if device.type != 'cuda':
            raise RuntimeError('%s runs on a HIP device (there is no host fallback); got tensors on %s'
                               % (type(self).__name__, device))
        if self.smpl.v_template.device != device:
            self.smpl = self.smpl.to(device)

    @staticmethod
    def _parameters(batch, device):
        """The static parameter tensors every session starts its ``t`` with."""
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=device)
        return dict(body_pose=z(batch, 69), betas=z(batch, 10), transl=z(batch, 3), global_orient=z(batch, 3))

    def _stage(self, t, iteration):
        """The 'fit' loop over the fitted parameters of ``t`` (smplxtosmpl_mtp.py:82-85)."""
        params = [t['body_pose'], t['betas'], t['transl']] + ([t['global_orient']] if self.fit_global_orient else [])
        for p in params:
            p.requires_grad = True
        return Stage(self, 'fit', params, iteration, {})

    @staticmethod
    def _seed(t, body_pose, betas):
        for name, value in (('body_pose', body_pose), ('betas', betas)):
            t[name].zero_() if value is None else t[name].copy_(value)

    @staticmethod
    def _fitted(t):
        """The caller's own copies of the parameters, in the order the result tuples begin with."""
        return tuple(t[name].detach().clone() for name in ('global_orient', 'body_pose', 'betas', 'transl'))


class MeshFitter(BodyFitter):
    """``MeshFitter(smpl)(target_vertices, global_orient)`` -> MeshFit.  ``vertices`` [B,V,3] include the translation,
    ``loss`` [B] is every body's term after the last update.  ``global_orient`` is held fixed (the reference passes it in
    on every call, :95-98) unless ``fit_global_orient`` is set.  Inputs are never modified."""

    def __init__(self, smpl, step_size=1e-2, num_iters=5000, fit_global_orient=False, use_graph=True, record_history=False):
        super().__init__(smpl, step_size, num_iters, fit_global_orient, use_graph, record_history)

    def _session(self, batch, num_verts, vertex_weights, device):
        """(key, session) of a fit with these constants: the stored one, or a new one (``_build``)."""
        # everything the captured loop bakes in; the session keeps the weights alive, so their id cannot be reused
        key = (batch, num_verts, id(vertex_weights) if vertex_weights is not None else None, device.index,
               float(self.step_size), bool(self.fit_global_orient), bool(self.record_history))
        return key, self._session_for(key, self._build, batch, num_verts, vertex_weights, device)

    def _build(self, batch, num_verts, vertex_weights, device):
        """A session: the static tensors, the iteration closure and the loop."""
        t = self._parameters(batch, device)
        t['target'] = torch.zeros(batch, num_verts, 3, dtype=torch.float32, device=device)
        weights = None if vertex_weights is None else ops.fit_weights(vertex_weights, num_verts, device)
        smpl = self.smpl

        def iteration():
            verts = _posed(smpl, t)
            total, _ = ops.vertex_fit(verts, t['transl'], t['target'], weights)
            return total, verts
        return dict(t=t, weights=weights, keys_alive=(vertex_weights,), stage=self._stage(t, iteration))

    def __call__(self, target_vertices, global_orient, body_pose=None, betas=None, transl=None, vertex_weights=None):
        smpl_verts = int(self.smpl.v_template.shape[0])
        if target_vertices.dim() != 3 or tuple(target_vertices.shape[1:]) != (smpl_verts, 3) or target_vertices.shape[0] == 0:
            raise ValueError('MeshFitter: target_vertices must be [B,%d,3] (the body model\'s topology), got %s'
                             % (smpl_verts, tuple(target_vertices.shape)))
        batch = target_vertices.shape[0]
        self._check_shapes(('global_orient', global_orient, (batch, 3)), ('body_pose', body_pose, (batch, 69)),
                           ('betas', betas, (batch, 10)), ('transl', transl, (batch, 3)))
        device = target_vertices.device
        self._to_device(device)
        with self._loops(device, bool(self.use_graph), 'fit') as capture:
            key, sess = self._session(batch, smpl_verts, vertex_weights, device)
            t, weights = sess['t'], sess['weights']
            with torch.no_grad():
                t['target'].copy_(target_vertices)
                t['global_orient'].copy_(global_orient)
                self._seed(t, body_pose, betas)
                if transl is not None:
                    t['transl'].copy_(transl)
                else:                          # :70-71, over the vertices that carry weight (their targets may be non-finite)
                    verts = _posed(self.smpl, t)
                    if weights is None:
                        t['transl'].copy_(t['target'].mean(1) - verts.mean(1))
                    else:
                        used = (weights.tensor != 0)[None, :, None]
                        gap = torch.where(used, t['target'] - verts, torch.zeros_like(verts))
                        t['transl'].copy_(gap.sum(1) / used.sum())
            self._settle(key, sess, sess['stage'].run(self.num_iters, None, capture))
            with torch.no_grad():
                verts = _posed(self.smpl, t)
                _, loss = ops.vertex_fit(verts, t['transl'], t['target'], weights)
                vertices = verts + t['transl'][:, None]
            return MeshFit(*self._fitted(t), vertices, loss)


ScanFit = namedtuple('ScanFit', ['global_orient', 'body_pose', 'betas', 'transl', 'vertices', 'loss', 'face', 'bary'])
CloudFit = namedtuple('CloudFit', ['loss', 'd2', 'index'])


class ScanFitter(BodyFitter):
    """Fit SMPL to unregistered points -- a scan, a depth point cloud, a mesh of another topology: ``ScanFitter(smpl,
    model)(points [B,Q,3], global_orient)`` -> ScanFit.  ``model`` is a ``ContactModel`` over the body model's faces (no
    geodesic mask is needed).  The data term is ops.scan_fit: every real point's distance to the nearest point of the posed,
    translated mesh under ``rho`` ('distance', 'squared' or 'gmof' with ``sigma``), averaged per body with ``weights``
    [B,Q]; ``counts`` [B] marks how many points per body are real.  The loop is MeshFitter's: body model forward, the term
    with its gradients as one call, backward from the cached unit seed, Adam as one launch, run by fit_loop.Stage and kept
    as a session (at most four; ``TUCH_GRAPH_STRICT`` and ``TUCH_SMPLIFY_SESSIONS`` as there).

    ``use_hint``: the session holds a [B,Q] int32 tensor that is both the search's hint and where it writes its faces, so
    every iteration starts each point from the face it found last time; the tensor is reset to -1 at the start of every
    call.  The hint changes no bit of any result (tuch_closest_point with a hint).

    ``model_to_scan`` lambda > 0 makes the fit two-sided: the iteration's objective is the scan -> model term plus
    lambda times the model -> scan term (ops.cloud_fit: every vertex's distance to the nearest real point of the scan
    under the same ``rho`` / ``sigma``, averaged per body with ``vertex_weights`` [V] or [B,V], truncated at
    ``max_distance`` for partial scans).  The session then holds an ops.PointCloud over its static points / counts /
    weights buffers (``resolution`` cells along the longest extent) and a [B,V] int32 tensor that is the query's hint and
    where it writes its indices; the cloud is rebuilt and the tensor reset to -1 at the start of every call, outside the
    replayed loop.  With the default 0.0 nothing of this exists: the bits and the launches are those of the one-sided fit.

    ``max_normal_angle`` (degrees, in (0, 90]) with ``normals`` [B,Q,3] at the call makes the scan -> model term
    normal-compatible (ops.scan_fit with normals: a point is matched only to faces whose normal is within the angle of
    its own; zero rows are unconstrained; a point left without a match adds nothing and keeps its weight in the
    normaliser).  The session then holds a static normals buffer.  Unless ``model_to_scan_normals`` is set, normals affect
    the scan -> model term only: the
    model -> scan term stays as it is and keeps ``max_distance`` as its rejection.  Without normals every launch and every
    bit is that of the fit without the option.  ``face`` is -1 for the points left without a match at the final
    evaluation: the share matched is ``(face >= 0)``.

    ``model_to_scan_normals`` (needs ``model_to_scan > 0``, ``max_normal_angle`` and normals at the call, passed or
    estimated) makes the model -> scan term normal-compatible too: a vertex is matched only to scan points whose normal
    is within ``max_normal_angle`` of the vertex's own posed normal (ops.cloud_fit with max_angle: the area-weighted sum
    of its faces' normals, formed inside the term's one launch; scan points with a zero normal row stay unconstrained).
    This is for scans that see one side of the body: without it every vertex of the unseen side is pulled to the
    nearest point of the seen side, which drags the body towards the sensor and flattens it; ``max_distance`` only
    bounds that.  A vertex without an admissible point is one without winner: rho(max_distance^2) under
    ``max_distance``, else 0, and no gradient; ``model_to_scan_result.index == -1`` marks them.  The session's cloud is
    oriented with the session's normals buffer (``PointCloud.orient``) at the start of every call, after the rebuild and
    after ``estimate_normals`` has filled the buffer, outside the replayed loop.  Give it ``max_distance``: without one a
    vertex whose admissible points are far away, or that has none, walks the whole cloud past every nearer inadmissible
    point (1.3 x the iteration at 10 cm, 13 x without).  With the default False every launch and
    every bit is that of the fitter without the argument.

    ``estimate_normals`` k (1 .. 32; needs ``max_normal_angle``) is for points that arrive without normals, a depth point
    cloud: at the start of every call, outside the replayed loop, the session's normals buffer is filled with
    ``PointCloud.normals(k=k, viewpoint=viewpoint)`` of the scan itself (PCA over every real point's k nearest real
    points; ``viewpoint`` [B,3] at the call, the sensor's position, turns them towards the sensor; points whose
    neighbourhood determines no normal get a zero row and stay unconstrained).  The cloud is the two-sided fit's when
    ``model_to_scan > 0``, otherwise one the session keeps for this.  The loop's launches and the bits of the result are
    those of the same fit called with these normals; passing ``normals=`` as well is an error.  Pass ``viewpoint``
    whenever the sensor's position is known: without it the normals carry the canonical sign (the component of the
    largest magnitude positive), which has nothing to do with inside and outside, and every point whose normal so
    signed faces away from the surface's outward normal is left without a match by ``max_normal_angle``, silently
    -- about half of a closed body.  With ``model_to_scan_normals`` this holds in both directions: such a point is
    also never a vertex's match.

    ``vertices`` [B,V,3] include the translation; ``loss`` [B] (the scan -> model term), ``face`` [B,Q] and ``bary``
    [B,Q,3] are those of the evaluation after the last update; the other direction's is ``self.model_to_scan_result`` =
    CloudFit(loss [B], d2 [B,V], index [B,V]) (None when the option is off).  ``global_orient`` is held fixed unless ``fit_global_orient`` is set.  Inputs are
    never modified; there is no host fallback."""

    def __init__(self, smpl, model, step_size=1e-2, num_iters=300, fit_global_orient=True, rho='distance', sigma=None,
                 use_hint=True, use_graph=True, record_history=False, model_to_scan=0.0, vertex_weights=None,
                 max_distance=None, resolution=64, max_normal_angle=None, estimate_normals=None,
                 model_to_scan_normals=False):
        ops.args.rho_of('ScanFitter', rho, sigma)
        if not float(model_to_scan) >= 0.0:
            raise ValueError('ScanFitter: model_to_scan must be >= 0, got %r' % (model_to_scan,))
        ops.args.tau_of('ScanFitter', max_distance)
        if max_normal_angle is not None:
            max_normal_angle = ops.args.angle_of('ScanFitter', 'max_normal_angle', max_normal_angle)
        ops.args.resolution_of('ScanFitter', resolution)
        if estimate_normals is not None:
            ops.args.check_k('ScanFitter: estimate_normals', estimate_normals)
            if max_normal_angle is None:
                raise ValueError('ScanFitter: estimate_normals needs max_normal_angle')
        if model_to_scan_normals and not (float(model_to_scan) > 0.0 and max_normal_angle is not None):
            raise ValueError('ScanFitter: model_to_scan_normals needs model_to_scan > 0 and max_normal_angle')
        num_verts = int(smpl.v_template.shape[0])
        if vertex_weights is not None and (not torch.is_tensor(vertex_weights) or vertex_weights.dim() not in (1, 2)
                                           or vertex_weights.shape[-1] != num_verts):
            raise ValueError('ScanFitter: vertex_weights must be a [%d] or [B,%d] tensor' % (num_verts, num_verts))
        super().__init__(smpl, step_size, num_iters, fit_global_orient, use_graph, record_history)
        self.model = model
        self.rho, self.sigma = rho, sigma
        self.use_hint = use_hint
        self.model_to_scan = float(model_to_scan)
        self.vertex_weights = vertex_weights
        self.max_distance = None if max_distance is None else float(max_distance)
        self.resolution = resolution
        self.max_normal_angle = max_normal_angle
        self.estimate_normals = estimate_normals
        self.model_to_scan_normals = bool(model_to_scan_normals)
        self.model_to_scan_result = None

    def _session(self, batch, num_points, with_counts, with_weights, device, with_normals=False):
        """(key, session) of a fit with these constants: the stored one, or a new one (``_build``)."""
        key = (batch, num_points, bool(with_counts), bool(with_weights), device.index, float(self.step_size),
               bool(self.fit_global_orient), self.rho, None if self.sigma is None else float(self.sigma), bool(self.use_hint),
               bool(self.record_history), self.model_to_scan,
               id(self.vertex_weights) if self.vertex_weights is not None else None, self.max_distance, self.resolution,
               bool(with_normals), self.max_normal_angle if with_normals else None)
        if self.model_to_scan_normals:           # (with the flag off the key is the one it has always been)
            key += ('model_to_scan_normals',)
        return key, self._session_for(key, self._build, batch, num_points, with_counts, with_weights, device, with_normals)

    def _build(self, batch, num_points, with_counts, with_weights, device, with_normals):
        """A session: the static tensors, the iteration closure and the loop."""
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=device)
        t = self._parameters(batch, device)
        t.update(points=z(batch, num_points, 3), hint=z(batch, num_points, dtype=torch.int32),
                 counts=z(batch, dtype=torch.int32) if with_counts else None,
                 weights=z(batch, num_points) if with_weights else None,
                 normals=z(batch, num_points, 3) if with_normals else None)
        smpl, model = self.smpl, self.model
        angle = self.max_normal_angle if with_normals else None
        hint = t['hint'] if self.use_hint else None
        cloud = vw = near = None
        if self.model_to_scan > 0.0:
            num_verts = int(smpl.v_template.shape[0])
            if self.vertex_weights is not None:
                if self.vertex_weights.dim() == 2 and self.vertex_weights.shape[0] != batch:
                    raise ValueError('ScanFitter: vertex_weights are %s, the batch is %d'
                                     % (tuple(self.vertex_weights.shape), batch))
                vw = self.vertex_weights.detach().to(device=device, dtype=torch.float32).contiguous()
            # (over the session's own buffers: rebuilt in place at the start of every call)
            cloud = ops.PointCloud(t['points'], t['counts'], t['weights'], self.resolution)
            t['near'] = z(batch, num_verts, dtype=torch.int32)
            near = t['near'] if self.use_hint else None
        # model_to_scan_normals: the model -> scan term is the oriented one (the cloud is oriented with t['normals'] at
        # the start of every call, after the rebuild and after the normals buffer has been filled)
        oriented = dict(max_angle=angle, normal_table=ops.vertex_normal_table(model.faces_np, int(smpl.v_template.shape[0]),
                                                                              device)) if self.model_to_scan_normals else {}

        def iteration():
            verts = _posed(smpl, t)
            # (the hint tensor receives the new faces: the aliasing tuch_closest_point allows)
            total, _, _ = ops.scan_fit(model, verts, t['transl'], t['points'], t['counts'], t['weights'], hint,
                                       self.rho, self.sigma, face_out=hint, normals=t['normals'], max_angle=angle)
            if cloud is not None:
                # the two vertex gradients meet in autograd's accumulation (one add of [B,V,3])
                other, _, _ = ops.cloud_fit(cloud, verts, t['transl'], vw, near, self.rho, self.sigma,
                                            self.max_distance, self.model_to_scan, index_out=near, **oriented)
                total = total + other
            return total, verts
        return dict(t=t, cloud=cloud, normals_cloud=None, vertex_weights=vw, keys_alive=(self.vertex_weights,), oriented=oriented,
                    stage=self._stage(t, iteration))

    def __call__(self, points, global_orient, counts=None, weights=None, body_pose=None, betas=None, transl=None,
                 normals=None, viewpoint=None):
        if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] == 0 or points.shape[1] == 0:
            raise ValueError('ScanFitter: points must be [B,Q,3], got %s' % (tuple(points.shape),))
        batch, num_points = points.shape[0], points.shape[1]
        self._check_shapes(('global_orient', global_orient, (batch, 3)), ('body_pose', body_pose, (batch, 69)),
                           ('betas', betas, (batch, 10)), ('transl', transl, (batch, 3)), ('counts', counts, (batch,)),
                           ('weights', weights, (batch, num_points)))
        if normals is not None and self.max_normal_angle is None:
            raise ValueError('ScanFitter: normals need max_normal_angle (the fitter was created without it)')
        self._check_shapes(('normals', normals, (batch, num_points, 3)))
        if self.estimate_normals is not None and normals is not None:
            raise ValueError('ScanFitter: normals were passed to a fitter that estimates them (estimate_normals=%d)'
                             % self.estimate_normals)
        if viewpoint is not None and self.estimate_normals is None:
            raise ValueError('ScanFitter: viewpoint needs estimate_normals (the fitter was created without it)')
        self._check_shapes(('viewpoint', viewpoint, (batch, 3)))
        with_normals = normals is not None or self.estimate_normals is not None
        if self.model_to_scan_normals and not with_normals:
            raise ValueError('ScanFitter: model_to_scan_normals needs normals at the call (pass normals= or create the '
                             'fitter with estimate_normals)')
        device = points.device
        self._to_device(device)
        if int(self.model.num_verts) != int(self.smpl.v_template.shape[0]):
            raise ValueError('ScanFitter: the ContactModel has %d vertices, the body model %d'
                             % (self.model.num_verts, self.smpl.v_template.shape[0]))
        with self._loops(device, bool(self.use_graph), 'fit') as capture:
            key, sess = self._session(batch, num_points, counts is not None, weights is not None, device, with_normals)
            t = sess['t']
            with torch.no_grad():
                t['points'].copy_(points)
                t['global_orient'].copy_(global_orient)
                t['hint'].fill_(-1)                       # no memory of another call's answers
                if counts is not None:
                    t['counts'].copy_(counts.clamp(0, num_points))
                if weights is not None:
                    t['weights'].copy_(weights)
                if normals is not None:
                    t['normals'].copy_(normals)
                self._seed(t, body_pose, betas)
                if transl is not None:
                    t['transl'].copy_(transl)
                else:               # the centroid of each body's real, weighted points minus that of its initial vertices
                    verts = _posed(self.smpl, t)
                    w = torch.ones(batch, num_points, device=device) if weights is None else t['weights'].clone()
                    if counts is not None:
                        w = w * (torch.arange(num_points, device=device)[None] < t['counts'][:, None])
                    used = (w != 0)[:, :, None]
                    centre = torch.where(used, w[:, :, None] * t['points'], torch.zeros_like(t['points'])).sum(1)
                    wsum = w.sum(1, keepdim=True)
                    centre = torch.where(wsum != 0, centre / torch.where(wsum != 0, wsum, torch.ones_like(wsum)),
                                         verts.mean(1))       # (a body without points stays where it is)
                    t['transl'].copy_(centre - verts.mean(1))
                if sess['cloud'] is not None:
                    sess['cloud'].rebuild(t['points'], t['counts'], t['weights'])
                    t['near'].fill_(-1)                   # no memory of another call's answers
                if self.estimate_normals is not None:
                    # the scan's normals from the scan itself, once per call: the loop is that of a fit given normals
                    cloud = sess['cloud']
                    if cloud is None:
                        if sess['normals_cloud'] is None:
                            sess['normals_cloud'] = ops.PointCloud(t['points'], t['counts'], t['weights'], self.resolution)
                        else:
                            sess['normals_cloud'].rebuild(t['points'], t['counts'], t['weights'])
                        cloud = sess['normals_cloud']
                    t['normals'].copy_(cloud.normals(k=self.estimate_normals, viewpoint=viewpoint).normal)
                if self.model_to_scan_normals:
                    # after the rebuild (which drops them) and after the buffer holds this call's normals
                    sess['cloud'].orient(t['normals'])
            self._settle(key, sess, sess['stage'].run(self.num_iters, None, capture))
            with torch.no_grad():
                verts = _posed(self.smpl, t)
                hint = t['hint'] if self.use_hint else None
                _, loss, near = ops.scan_fit(self.model, verts, t['transl'], t['points'], t['counts'], t['weights'], hint,
                                             self.rho, self.sigma, normals=t['normals'],
                                             max_angle=self.max_normal_angle if with_normals else None)
                vertices = verts + t['transl'][:, None]
                self.model_to_scan_result = None
                if sess['cloud'] is not None:
                    _, other, found = ops.cloud_fit(sess['cloud'], verts, t['transl'], sess['vertex_weights'],
                                                    t['near'] if self.use_hint else None, self.rho, self.sigma,
                                                    self.max_distance, self.model_to_scan, **sess['oriented'])
                    self.model_to_scan_result = CloudFit(other, found.d2, found.index)
            return ScanFit(*self._fitted(t), vertices, loss, near.face, near.bary)
