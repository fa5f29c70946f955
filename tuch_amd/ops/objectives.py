"""The SMPLify-DC objectives: reprojection + prior, the weighted total and the stage-1 objective on the kernels of
csrc/small_terms.hip, and the fused stage-2 tail of csrc/contact_terms.hip."""
from __future__ import annotations

import weakref

import torch
from torch.autograd.function import once_differentiable

from .. import _C, backward_pass
from ._base import _f32, _ticket, deterministic
from .terms import MODE_SMPLIFY


class _SmallTerms(torch.autograd.Function):
    """Reprojection + max-mixture prior of the SMPLify-DC objective in one kernel; returns [B,2]."""

    @staticmethod
    def forward(ctx, joints, camera_t, body_pose, camera_center, joints_2d, joints_conf, means, precisions,
                log_weights, focal, sigma, prior_scale):
        j = _f32(joints)
        b, nj, _ = j.shape
        out = torch.empty(b, 2, dtype=torch.float32, device=j.device)
        gj = torch.empty_like(j)
        gc = torch.empty(b, 3, dtype=torch.float32, device=j.device)
        gp = torch.empty(b, 69, dtype=torch.float32, device=j.device) if body_pose is not None else None
        # bound to locals: a converted copy must stay alive until the kernel has been enqueued
        cam_t, cam_c, j2d, conf = _f32(camera_t), _f32(camera_center), _f32(joints_2d), _f32(joints_conf)
        pose = _f32(body_pose) if body_pose is not None else None
        _C.check(_C.lib().tuch_smplify_small_terms(
            _C.ptr(j), _C.ptr(cam_t), _C.ptr(cam_c), _C.ptr(j2d), _C.ptr(conf), _C.ptr(pose),
            _C.ptr(means), _C.ptr(precisions), _C.ptr(log_weights), b, nj,
            means.shape[0] if means is not None else 0, float(focal), float(sigma), float(prior_scale),
            _C.ptr(out), _C.ptr(gj), _C.ptr(gc), _C.ptr(gp), _C.stream()))
        ctx.save_for_backward(gj, gc, gp)
        return out

    @staticmethod
    def backward(ctx, g):
        gj, gc, gp = ctx.saved_tensors
        g_rep, g_pri = g[:, 0].contiguous(), g[:, 1].contiguous()
        return (gj * g_rep[:, None, None], gc * g_rep[:, None],
                gp * g_pri[:, None] if gp is not None else None) + (None,) * 9


def smplify_small_terms(joints, camera_t, body_pose, camera_center, joints_2d, joints_conf, means, precisions,
                        log_weights, focal, sigma, prior_scale):
    return _SmallTerms.apply(joints, camera_t, body_pose, camera_center, joints_2d, joints_conf, means,
                             precisions, log_weights, focal, sigma, prior_scale)


class _Objective(torch.autograd.Function):
    """sum(small) + contact_scale * sum(terms) + r2r_scale * sum(r2r) as one deterministic kernel."""

    @staticmethod
    def forward(ctx, small, terms, r2r, contact_scale, r2r_scale):
        small, terms = small.contiguous(), terms.contiguous()
        b = small.shape[0]
        p = r2r.shape[1] if r2r is not None else 0
        out = torch.empty(1, dtype=torch.float32, device=small.device)
        r2r_c = r2r.contiguous() if p else None
        _C.check(_C.lib().tuch_smplify_objective(_C.ptr(small), _C.ptr(terms), _C.ptr(r2r_c), b, p,
                                                 float(contact_scale), float(r2r_scale), _C.ptr(out), _C.stream()))
        ctx.shape = (b, p, float(contact_scale), float(r2r_scale))
        return out[0]

    @staticmethod
    def backward(ctx, g):
        b, p, cs, rs = ctx.shape
        g = g.reshape(1).to(torch.float32).contiguous()
        gs = torch.empty(b, 2, dtype=torch.float32, device=g.device)
        gt = torch.empty(b, 2, dtype=torch.float32, device=g.device)
        gr = torch.empty(b, p, dtype=torch.float32, device=g.device) if p else None
        _C.check(_C.lib().tuch_smplify_objective_bwd(_C.ptr(g), b, p, cs, rs, _C.ptr(gs), _C.ptr(gt), _C.ptr(gr),
                                                     _C.stream()))
        return gs, gt, gr, None, None


def smplify_objective(small, terms, r2r, contact_scale, r2r_scale):
    return _Objective.apply(small, terms, r2r, contact_scale, r2r_scale)


def _rows_of(t, b, tail, name):
    """float32, contiguous, [b, *tail]; a batch of one is broadcast like the torch-op form would (the kernels index raw
    pointers by body: any other shape would be an out-of-bounds read)."""
    t = _f32(t)
    if t.dim() == len(tail) + 1 and t.shape[0] == 1 and b > 1:
        t = t.expand(b, *t.shape[1:]).contiguous()
    if tuple(t.shape) != (b,) + tuple(tail):
        raise ValueError('stage-1 objective: %s has shape %s, expected %s' % (name, tuple(t.shape), (b,) + tuple(tail)))
    return t


class _Stage1Objective(torch.autograd.Function):
    """camera_fitting_loss (tuch/smplify/losses.py:125-152) as ONE launch: reprojection + depth term + shape prior, the
    scalar total and the unit gradients w.r.t. joints / camera translation / betas (csrc/small_terms.hip:
    stage1_terms_kernel).  backward() only hands the gradients over (scaled unless the upstream gradient is the cached
    unit seed of ops.backward_scalar)."""

    @staticmethod
    def forward(ctx, joints, camera_t, betas, camera_t_est, camera_center, joints_2d, joints_conf, focal, sigma, depth_w,
                shape_w):
        j = _f32(joints)
        if j.dim() != 3 or j.shape[2] != 3:
            raise ValueError('stage-1 objective: joints must be [B,J,3], got %s' % (tuple(j.shape),))
        b, nj, _ = j.shape
        ct = _rows_of(camera_t, b, (3,), 'camera_t')
        be = None
        if betas is not None and shape_w != 0.0:
            if betas.dim() != 2:
                raise ValueError('stage-1 objective: betas must be [B,n], got %s' % (tuple(betas.shape),))
            be = _rows_of(betas, b, (betas.shape[1],), 'betas')
        est, cc = _rows_of(camera_t_est, b, (3,), 'camera_t_est'), _rows_of(camera_center, b, (2,), 'camera_center')
        j2d, conf = _rows_of(joints_2d, b, (nj, 2), 'joints_2d'), _rows_of(joints_conf, b, (nj,), 'joints_conf')
        out = torch.empty(1, dtype=torch.float32, device=j.device)
        share = torch.empty(b, dtype=torch.float32, device=j.device)
        gj = torch.empty_like(j)
        gc = torch.empty(b, 3, dtype=torch.float32, device=j.device)
        gb = torch.empty_like(be) if be is not None else None
        _C.check(_C.lib().tuch_smplify_stage1_terms(
            _C.ptr(j), _C.ptr(ct), _C.ptr(est), _C.ptr(cc), _C.ptr(j2d), _C.ptr(conf), _C.ptr(be), b, nj,
            be.shape[1] if be is not None else 0, float(focal), float(sigma), float(depth_w), float(shape_w), _C.ptr(share),
            _C.ptr(_ticket(j.device)), _C.ptr(out), _C.ptr(gj), _C.ptr(gc), _C.ptr(gb), _C.stream()))
        ctx.save_for_backward(gj, gc, gb)
        ctx.in_dtypes = (joints.dtype, camera_t.dtype, betas.dtype if betas is not None else None)
        ctx.in_shapes = (tuple(camera_t.shape), tuple(betas.shape) if betas is not None else None)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gj, gc, gb = ctx.saved_tensors
        if not backward_pass.is_unit_seed(g):
            g = g.reshape(()).to(torch.float32)
            gj, gc, gb = gj * g, gc * g, (gb * g if gb is not None else None)
        dj, dc, db = ctx.in_dtypes
        sc, sb = ctx.in_shapes
        if tuple(gc.shape) != sc:                     # a broadcast batch of one: its gradient is the sum over the bodies
            gc = gc.sum(0, keepdim=True)
        if gb is not None and tuple(gb.shape) != sb:
            gb = gb.sum(0, keepdim=True)
        return (gj.to(dj), gc.to(dc), gb.to(db) if gb is not None else None) + (None,) * 8


def smplify_stage1_objective(joints, camera_t, betas, camera_t_est, camera_center, joints_2d, joints_conf, focal, sigma,
                             depth_weight, shape_weight):
    return _Stage1Objective.apply(joints, camera_t, betas, camera_t_est, camera_center, joints_2d, joints_conf, focal, sigma,
                                  depth_weight, shape_weight)


class _Stage2Tail(torch.autograd.Function):
    """Everything of the stage-2 objective behind the body model as ONE autograd node (tuch/smplify/losses.py:56-123):
    inside test + nearest admissible vertex (no gradient), contact sums, region minima, reprojection + prior, the
    weighted total.  The same kernels as the separate nodes (_SmallTerms, _ContactTerms, _RegionPairMin, _Objective);
    what goes away is the torch glue between them -- in the backward pass ~10 small launches per step (scalings by the
    upstream gradient, dtype / layout copies, a zero fill and an add per gradient path into the vertices).  Backward:
    one kernel turns the upstream scalar into the weights of every term, then the contact and region kernels
    accumulate into one vertex gradient."""

    @staticmethod
    def forward(ctx, verts, joints, camera_t, body_pose, model, valid, select, const):
        v, j = _f32(verts), _f32(joints)
        cam_t, pose = _f32(camera_t), _f32(body_pose)
        b, nj, _ = j.shape
        L = _C.lib()
        cam_c, j2d, conf = _f32(const['camera_center']), _f32(const['joints_2d']), _f32(const['joints_conf'])
        means, precisions, logw = const['means'], const['precisions'], const['log_weights']
        small = torch.empty(b, 2, dtype=torch.float32, device=v.device)
        gj = torch.empty_like(j)
        gc = torch.empty(b, 3, dtype=torch.float32, device=v.device)
        gp = torch.empty(b, 69, dtype=torch.float32, device=v.device)
        p = model.num_pairs if select is not None else 0

        # ONE cleared buffer: the vertex gradient the unit backward accumulates into, the arrival counter of the
        # tail kernel ("the last block adds up": it belongs to THIS call -- no counter shared between streams, none
        # left non-zero by an aborted launch) and the region pairs' keys (tuch_region_pair_keys wants them zero).  It is
        # cleared by the FIRST kernel of the search (a fill launch of its own was 5 us of the second stream's chain).
        n = v.numel()
        k0 = n + 1 + ((n + 1) & 1)                  # the 64-bit keys start on an even word behind the counter
        det = 2 * n if deterministic() else 0       # deterministic mode: 64-bit fixed-point accumulators

        def beside_the_walk(zeros):          # on the second stream (ContactModel.exterior_and_partner), behind the search
            keys = zeros[k0:k0 + 2 * b * p].view(torch.int64) if p else None
            fixed = zeros[k0 + 2 * b * p:k0 + 2 * b * p + det].view(torch.int64) if det else None
            if p:
                _C.check(L.tuch_region_pair_keys(model._handle, _C.ptr(v), b, _C.ptr(select), 1, _C.ptr(keys), _C.stream()))
            _C.check(L.tuch_smplify_small_terms(
                _C.ptr(j), _C.ptr(cam_t), _C.ptr(cam_c), _C.ptr(j2d), _C.ptr(conf), _C.ptr(pose), _C.ptr(means),
                _C.ptr(precisions), _C.ptr(logw), b, nj, means.shape[0], float(const['focal']), float(const['sigma']),
                float(const['prior_scale']), _C.ptr(small), _C.ptr(gj), _C.ptr(gc), _C.ptr(gp), _C.stream()))
            return (keys, fixed, small, gj, gc, gp, zeros[:n].view(v.shape), zeros[n:n + 1].view(torch.int32))
        exterior, _, partner, _extra = model.exterior_and_partner(v, apply_segments=const['apply_segments'],
                                                                  also=beside_the_walk, zero_floats=k0 + 2 * b * p + det,
                                                                  iterative=True)       # SMPLify-DC's stage-2 loop
        out = torch.empty(1, dtype=torch.float32, device=v.device)
        share = torch.empty(L.tuch_smplify_stage2_fused_scratch_floats(b), dtype=torch.float32, device=v.device)
        # the objective is the root of the fit's graph: its vertex gradient for a unit upstream gradient is written by the
        # same launch that forms the sums (csrc/contact_terms.hip: stage2_fused_kernel); backward() only hands it over
        want_grad = any(ctx.needs_input_grad[:4])
        gv = _extra[6] if want_grad else None
        # deterministic mode: the vertex gradient stays in its 64-bit fixed-point accumulators (no conversion launch here);
        # backward() hands them to the body model's node, whose skinning adjoint reads them -- or converts them if the pass
        # is not the plain `objective.backward()` of a fit.  gv (zeros nobody writes in this mode) is what autograd carries.
        fixed = _extra[1] if want_grad else None
        _C.check(L.tuch_smplify_stage2_fused(_C.ptr(v), _C.ptr(partner), _C.ptr(exterior), _C.ptr(valid), b, v.shape[1],
                                             MODE_SMPLIFY, float(const['euclthres']), _C.ptr(small), p,
                                             float(const['contact_scale']), float(const['r2r_scale']), _C.ptr(share),
                                             _C.ptr(_extra[7]), _C.ptr(out), _C.ptr(gv) if fixed is None else None,
                                             model._handle if p else None, _C.ptr(_extra[0]),
                                             _C.ptr(fixed), _C.stream()))
        if want_grad:
            # (fixed: a view of gv's buffer, only read by backward() and the skinning adjoint; saved like the others, so a
            # retained graph's next pass finds it again and a plain pass releases the buffer where it always did)
            ctx.save_for_backward(gv, gj, gc, gp, fixed)
        ctx.in_dtypes = (verts.dtype, joints.dtype, camera_t.dtype, body_pose.dtype)
        # body_pose also feeds the body model that made `verts`: that node's backward runs after this one and can add the prior's
        # pose gradient inside its own last kernel (backward_pass.Handover): autograd then has no two gradients to sum in a launch
        node = verts.grad_fn
        ctx.verts_ref = weakref.ref(verts)          # backward() asks whether somebody watches the vertices' own gradient
        ref = getattr(node, 'pose_ref', None) if node is not None else None
        ctx.lbs_node = node if (want_grad and ctx.needs_input_grad[0] and ctx.needs_input_grad[3] and ref is not None
                                and ref() is body_pose) else None
        return out[0]

    @staticmethod
    @once_differentiable          # the gradients were formed in forward(): constants of a second differentiation
    def backward(ctx, g):
        gv, gj, gc, gp, fixed = ctx.saved_tensors
        dv, dj, dc, dp = ctx.in_dtypes
        # (the rules of what follows: the table of backward_pass.  root: not a loss like `tail + other(body_pose)`, which
        # reaches this node with the same unit seed, but whose pose gradient does not all flow through here)
        task = backward_pass.pass_id()
        unit = backward_pass.is_unit_seed(g)
        root = unit and backward_pass.is_root(ctx)
        leave = ctx.lbs_node is not None and task >= 0
        # (somebody who retains / hooks the vertices' own gradient must see the real numbers, not the carrier of zeros;
        # asked NOW: both can be added after the loss was built.  Nobody holds a tensor that is gone: no .grad to fill)
        verts = ctx.verts_ref()
        watched = verts is not None and (verts.retains_grad or bool(getattr(verts, '_backward_hooks', None)))
        hand_over = fixed is not None and leave and root and not watched
        if fixed is not None and not hand_over:
            # anything but the plain backward of a fit (scaled, watched vertices, further terms): the float gradient, converted
            gv = torch.empty_like(gv)
            _C.check(_C.lib().tuch_fixed_to_float(_C.ptr(fixed), fixed.numel(), _C.ptr(gv), _C.stream()))
        if not unit:
            g = g.reshape(()).to(torch.float32)
            gv, gj, gc, gp = gv * g, gj * g, gc * g, gp * g
        left = leave and backward_pass.leave(ctx.lbs_node, backward_pass.Handover(task, gp, fixed if hand_over else None, root))
        return gv.to(dv), gj.to(dj), gc.to(dc), None if left else gp.to(dp), None, None, None, None


def smplify_stage2_tail(verts, joints, camera_t, body_pose, model, valid_u8, select_u8, **const):
    """Scalar stage-2 objective behind the body model (see _Stage2Tail); const: camera_center, joints_2d, joints_conf,
    means, precisions, log_weights, focal, sigma, prior_scale, euclthres, contact_scale, r2r_scale, apply_segments."""
    return _Stage2Tail.apply(verts, joints, camera_t, body_pose, model, valid_u8, select_u8, const)
