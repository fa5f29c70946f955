"""PointCloud, a batch of static point clouds with a uniform grid per body, on the kernels of csrc/point_cloud.hip:
nearest point, k nearest neighbours, PCA normals, and the model-to-scan data term."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import _C
from . import args
from ._base import _f32, _hand_over, _need_hip, _ticket, _workspace
from .normals_render import _check_normal_table


class NearestPoint(NamedTuple):
    d2: torch.Tensor
    index: torch.Tensor


class KNearest(NamedTuple):
    d2: torch.Tensor
    index: torch.Tensor


class PointNormals(NamedTuple):
    normal: torch.Tensor
    variation: torch.Tensor
    count: torch.Tensor
    cov: Optional[torch.Tensor]


class CloudGrid(NamedTuple):
    """Host copies of a PointCloud's per-body headers: origin [B,3] float32, cell [B] float32, dims [B,3] int32."""
    origin: np.ndarray
    cell: np.ndarray
    dims: np.ndarray


def set_cloud_canary(on: bool) -> bool:
    """Guard words behind the regions of every PointCloud workspace sized from now on (tuch_point_cloud_set_canary:
    process-wide; set it before constructing the cloud).  Returns the previous setting."""
    return bool(_C.lib().tuch_point_cloud_set_canary(int(bool(on))))


class _CloudNearest(torch.autograd.Function):
    """PointCloud.nearest: tuch_point_cloud_nearest forward; backward is 2 g (q - s) for queries and its sum over a body's
    queries for shift, the index held fixed (a handful of element-wise torch ops: not on any loop's path -- the loops
    use cloud_fit, whose gradients come out of the kernel)."""

    @staticmethod
    def forward(ctx, queries, shift, cloud, counts, hint, tau, index, query_normals, cos):
        qs = _f32(queries)
        sh = None if shift is None else _f32(shift)
        b, n, _ = qs.shape
        d2 = torch.empty(b, n, dtype=torch.float32, device=qs.device)
        # (the points' normals go with the queries': an oriented cloud asked without them answers the plain query)
        normals = None if query_normals is None else cloud.point_normals
        _C.check(_C.lib().tuch_point_cloud_nearest(
            _C.ptr(cloud._ws), cloud._nbytes, _C.ptr(cloud.points), _C.ptr(cloud.counts), _C.ptr(cloud.weights),
            _C.ptr(normals), _C.ptr(qs), _C.ptr(query_normals), _C.ptr(sh), _C.ptr(counts), _C.ptr(hint), tau, cos or 0.0,
            _C.ptr(cloud._cones), cloud._cones_bytes(), b, cloud.num_points, n, _C.ptr(d2), _C.ptr(index), _C.stream()))
        ctx.save_for_backward(qs, sh, index)
        ctx.cloud_points = cloud.points
        ctx.in_dtypes = (queries.dtype, None if shift is None else shift.dtype)
        return d2

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        qs, sh, index = ctx.saved_tensors
        won = index >= 0
        s = torch.gather(ctx.cloud_points, 1, index.clamp(min=0).long()[:, :, None].expand(-1, -1, 3))
        q = qs if sh is None else qs + sh[:, None]
        zero = torch.zeros((), dtype=torch.float32, device=qs.device)
        gq = torch.where(won[:, :, None], 2.0 * g.to(torch.float32)[:, :, None] * (q - s), zero)
        dq, ds = ctx.in_dtypes
        return (gq.to(dq) if ctx.needs_input_grad[0] else None,
                gq.sum(1).to(ds) if sh is not None and ctx.needs_input_grad[1] else None) + (None,) * 7


class PointCloud:
    """A batch of static point clouds with a uniform grid per body for exact nearest-point queries
    (csrc/point_cloud.hip; the rule is in include/tuch_amd.h).  ``PointCloud(points [B,Q,3], counts=None, weights=None,
    resolution=64)`` owns the workspace and builds on construction, on the current stream.  The cloud of body b is its
    VALID points: index < counts[b], weight != 0, finite.  The tensors are kept by reference (float32 contiguous inputs
    are not copied): change them in place and call ``rebuild()``.  There is no host fallback."""

    def __init__(self, points, counts=None, weights=None, resolution=64):
        self.resolution = args.resolution_of('PointCloud', resolution)
        self._ws = None
        self.rebuild(points, counts, weights)

    def rebuild(self, points, counts=None, weights=None):
        """Build again, in place where the batch and point counts are unchanged (the workspace is kept): for a session
        that keeps its buffers.  Capturable."""
        if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] == 0 or points.shape[1] == 0:
            raise ValueError('PointCloud: points must be [B,Q,3] with B, Q > 0, got %s' % (tuple(points.shape),))
        b, q = points.shape[0], points.shape[1]
        counts = args.counts_of('PointCloud', counts, b)
        args.check_weights('PointCloud', weights, b, q)
        _need_hip('PointCloud', points, counts, weights)
        self.points = _f32(points)
        self.counts = counts
        self.weights = None if weights is None else _f32(weights)
        L = _C.lib()
        nbytes = L.tuch_point_cloud_workspace_bytes(b, q, self.resolution)
        if self._ws is None or self._nbytes != nbytes or self._ws.device != points.device:
            # (zeroed once: the first word counts changed guard words under the canary option)
            self._ws = torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device=points.device)
            self._nbytes = nbytes
        self.batch, self.num_points = b, q
        # a rebuild leaves the cloud unoriented (the cones would be stale): call orient() again; the cone buffer is kept
        self.point_normals = None
        self._cones = None
        with torch.cuda.device(points.device):
            _C.check(L.tuch_point_cloud_build(_C.ptr(self.points), _C.ptr(self.counts), _C.ptr(self.weights), b, q,
                                              self.resolution, _C.ptr(self._ws), nbytes, _C.stream()))
        return self

    def orient(self, normals, cones=True):
        """Give the cloud its points' normals [B,Q,3], in the points' order (kept by reference like the points; zero or
        non-finite rows mean "unknown"), for ``nearest(query_normals=, max_angle=)`` and ``cloud_fit(max_angle=)``.
        ``cones``: also build the per-block normal cones that let a query pass by blocks of the grid without an
        admissible point (tuch_point_cloud_build_cones, one launch, capturable; they change no bit of any result).
        ``rebuild()`` drops both: call ``orient`` again after it."""
        if not torch.is_tensor(normals) or tuple(normals.shape) != (self.batch, self.num_points, 3):
            raise ValueError('PointCloud.orient: normals must be [%d,%d,3], got %s'
                             % (self.batch, self.num_points, tuple(normals.shape) if torch.is_tensor(normals) else type(normals)))
        _need_hip('PointCloud.orient', normals)
        if normals.device != self.points.device:
            raise RuntimeError('PointCloud.orient: normals on %s, the cloud on %s' % (normals.device, self.points.device))
        self.point_normals = _f32(normals.detach())
        self._cones = None
        if cones:
            L = _C.lib()
            nbytes = int(L.tuch_point_cloud_cones_bytes(self.batch, self.resolution))
            buf = getattr(self, '_cone_buffer', None)
            if buf is None or buf.numel() != nbytes or buf.device != self.points.device:
                buf = self._cone_buffer = torch.zeros(nbytes, dtype=torch.uint8, device=self.points.device)
            with torch.cuda.device(self.points.device):
                _C.check(L.tuch_point_cloud_build_cones(_C.ptr(self._ws), self._nbytes, _C.ptr(self.point_normals), self.batch,
                                                        self.num_points, self.resolution, _C.ptr(buf), nbytes, _C.stream()))
            self._cones = buf
        return self

    def _cones_bytes(self) -> int:
        return 0 if self._cones is None else int(self._cones.numel())

    def _oriented_cos(self, what, max_angle) -> float:
        """The float32 cosine the oriented C entry points take (as args.max_angle_cos); the cloud must be oriented."""
        if self.point_normals is None:
            raise ValueError('%s: max_angle needs an oriented cloud (PointCloud.orient; rebuild() drops the normals)' % what)
        return args.max_angle_cos(self.point_normals, max_angle, self.points, what)

    def _check_queries(self, what, queries, shift, hint, name='queries'):
        if queries.dim() != 3 or queries.shape[0] != self.batch or queries.shape[2] != 3 or queries.shape[1] == 0:
            raise ValueError('%s: %s must be [%d,N,3] with N > 0, got %s' % (what, name, self.batch, tuple(queries.shape)))
        if shift is not None and tuple(shift.shape) != (self.batch, 3):
            raise ValueError('%s: shift / transl has shape %s, expected %s' % (what, tuple(shift.shape), (self.batch, 3)))
        _need_hip(what, queries, shift, hint)
        if queries.device != self.points.device:
            raise RuntimeError('%s: %s on %s, the cloud on %s' % (what, name, queries.device, self.points.device))
        if hint is not None and (tuple(hint.shape) != tuple(queries.shape[:2]) or hint.dtype != torch.int32
                                 or not hint.is_contiguous()):
            raise ValueError('%s: hint must be a contiguous int32 %s tensor' % (what, tuple(queries.shape[:2])))

    def nearest(self, queries, shift=None, counts=None, hint=None, max_distance=None, index_out=None, query_normals=None,
                max_angle=None) -> NearestPoint:
        """For every real query ``queries[b,n] + shift[b]`` the nearest valid point of body b's cloud:
        ``NearestPoint(d2 [B,N], index [B,N] int32)``; no winner: index -1, d2 +inf.  counts [B]: real queries per body;
        hint [B,N] int32: a guess per query that changes no bit of any result (it may be ``index_out``, the tensor the
        indices are written to); max_distance tau > 0: only points with d2 <= f32(tau)^2 can win.  d2 is differentiable
        w.r.t. queries and shift with the index held fixed.
        query_normals [B,N,3] with max_angle in degrees, in (0, 90], on an oriented cloud (``orient``): the nearest valid
        point whose normal is within the angle of the query's (tuch_point_cloud_nearest with normals; a query or a point
        whose normal is a zero or non-finite row is unconstrained; normals are not shifted and get no gradient).  Both
        or neither must be given; with neither the call is the plain one."""
        what = 'PointCloud.nearest'
        self._check_queries(what, queries, shift, hint)
        b, n = queries.shape[0], queries.shape[1]
        counts = args.counts_of(what, counts, b)
        tau = args.tau_of(what, max_distance)
        _need_hip(what, counts, index_out)
        cos = None
        if args.both(what, 'query_normals', query_normals, 'max_angle', max_angle):
            if not torch.is_tensor(query_normals) or tuple(query_normals.shape) != (b, n, 3):
                raise ValueError('%s: query_normals must be [%d,%d,3], got %s'
                                 % (what, b, n, tuple(query_normals.shape) if torch.is_tensor(query_normals) else
                                    type(query_normals)))
            _need_hip(what, query_normals)
            query_normals, cos = _f32(query_normals.detach()), self._oriented_cos(what, max_angle)
        index = args.index_out(what, index_out, b, n, queries.device)
        d2 = _CloudNearest.apply(queries, shift, self, counts, hint, tau, index, query_normals, cos)
        return NearestPoint(d2, index)

    def _knn_args(self, what, queries, k, shift, counts, max_distance):
        """The checks and conversions knn and normals share: (queries, shift, counts, tau) as the C ABI takes them."""
        args.check_k(what, k)
        own = queries is None
        if own:
            queries = self.points
        self._check_queries(what, queries, shift, None)
        counts = args.counts_of(what, counts, queries.shape[0])
        tau = args.tau_of(what, max_distance)
        _need_hip(what, counts)
        qs = _f32(queries)
        if own:
            # the cloud's own points in the caller's order: an invalid point is no query (beyond counts: query_counts;
            # weight 0: made non-finite, which the rule answers with the no-winner outputs)
            if counts is None:
                counts = self.counts
            if self.weights is not None:
                qs = torch.where((self.weights != 0)[:, :, None], qs, torch.full_like(qs, float('nan')))
        return qs, None if shift is None else _f32(shift), counts, tau

    def knn(self, queries=None, k=8, shift=None, counts=None, max_distance=None) -> KNearest:
        """For every real query ``queries[b,n] + shift[b]`` the k (1 .. 32) nearest valid points of body b's cloud in
        ascending order of the packed key (d2, then index): ``KNearest(d2 [B,N,k], index [B,N,k] int32)``, the tail -1 /
        +inf where fewer than k points are admissible.  ``queries=None``: the cloud's own points in the caller's order
        (each valid point finds itself first, or its smallest-index duplicate; invalid points get -1 / +inf).  The bits
        are those of a sorted float32 brute-force sweep (tuch_point_cloud_knn).  No gradients."""
        qs, sh, counts, tau = self._knn_args('PointCloud.knn', queries, k, shift, counts, max_distance)
        b, n = qs.shape[0], qs.shape[1]
        d2 = torch.empty(b, n, k, dtype=torch.float32, device=qs.device)
        index = torch.empty(b, n, k, dtype=torch.int32, device=qs.device)
        with torch.cuda.device(qs.device):
            _C.check(_C.lib().tuch_point_cloud_knn(
                _C.ptr(self._ws), self._nbytes, _C.ptr(self.points), _C.ptr(self.counts), _C.ptr(self.weights), _C.ptr(qs),
                _C.ptr(sh), _C.ptr(counts), tau, b, self.num_points, n, k, _C.ptr(d2), _C.ptr(index), _C.stream()))
        return KNearest(d2, index)

    def normals(self, queries=None, k=16, viewpoint=None, shift=None, counts=None, max_distance=None,
                with_cov=False) -> PointNormals:
        """PCA normals over the k nearest valid points of every query (tuch_point_cloud_normals; the rule, the error bound
        and the zero rows are in include/tuch_amd.h): ``PointNormals(normal [B,N,3], variation [B,N], count [B,N] int32,
        cov [B,N,6] or None)``.  ``viewpoint`` [B,3] or [B,N,3], the sensor's position in the frame of the shifted
        queries, turns every normal towards it; without one the sign is canonical (the component of the largest
        magnitude is positive).  A zero row means "unknown" (fewer than 3 neighbours, collinear, coincident or isotropic
        ones) and is what scan_fit's ``normals`` treats as unconstrained.  ``queries=None``: the cloud's own points.
        No gradients."""
        what = 'PointCloud.normals'
        args.check_k(what, k)
        n_of = self.num_points if queries is None else (queries.shape[1] if queries.dim() == 3 else -1)
        layout = 0
        if viewpoint is not None:
            if tuple(viewpoint.shape) == (self.batch, 3):
                layout = 1
            elif tuple(viewpoint.shape) == (self.batch, n_of, 3):
                layout = 2
            else:
                raise ValueError('%s: viewpoint must be [%d,3] or [%d,N,3], got %s'
                                 % (what, self.batch, self.batch, tuple(viewpoint.shape)))
        qs, sh, counts, tau = self._knn_args(what, queries, k, shift, counts, max_distance)
        _need_hip(what, viewpoint)
        view = None if viewpoint is None else _f32(viewpoint)
        b, n = qs.shape[0], qs.shape[1]
        normal = torch.empty(b, n, 3, dtype=torch.float32, device=qs.device)
        variation = torch.empty(b, n, dtype=torch.float32, device=qs.device)
        count = torch.empty(b, n, dtype=torch.int32, device=qs.device)
        cov = torch.empty(b, n, 6, dtype=torch.float32, device=qs.device) if with_cov else None
        with torch.cuda.device(qs.device):
            _C.check(_C.lib().tuch_point_cloud_normals(
                _C.ptr(self._ws), self._nbytes, _C.ptr(self.points), _C.ptr(self.counts), _C.ptr(self.weights), _C.ptr(qs),
                _C.ptr(sh), _C.ptr(counts), tau, b, self.num_points, n, k, _C.ptr(view), layout, _C.ptr(normal),
                _C.ptr(variation), _C.ptr(count), _C.ptr(cov), _C.stream()))
        return PointNormals(normal, variation, count, cov)

    def grid(self) -> CloudGrid:
        """The headers the build wrote, as host arrays (synchronises; for tests and tools)."""
        origin = np.empty((self.batch, 3), np.float32)
        cell = np.empty(self.batch, np.float32)
        dims = np.empty((self.batch, 3), np.int32)
        as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        with torch.cuda.device(self.points.device):
            _C.check(_C.lib().tuch_point_cloud_grid(_C.ptr(self._ws), self.batch, self.resolution, as_p(origin), as_p(cell),
                                                    as_p(dims)))
        return CloudGrid(origin, cell, dims)

    def canary_hits(self, reset: bool = True) -> int:
        """Guard words of this cloud's workspace (and of the term's scratch) found changed (set_cloud_canary)."""
        out = ctypes.c_int(0)
        with torch.cuda.device(self.points.device):
            _C.check(_C.lib().tuch_point_cloud_canary_hits(_C.ptr(self._ws), ctypes.byref(out), int(reset)))
        return out.value


class _CloudFit(torch.autograd.Function):
    """ops.cloud_fit: the query, the term and the unit gradients in one launch (tuch_point_cloud_fit_terms).  `index`
    [B,V] int32 is written in place (it may be the hint tensor).  backward() only hands the gradients over, as
    _ScanFit's."""

    @staticmethod
    def forward(ctx, verts, transl, cloud, vw, layout, hint, rho, sigma, tau, scale, index, cos, table):
        v, tr = _f32(verts), _f32(transl)
        b, n, _ = v.shape
        dev = v.device
        L = _C.lib()
        d2 = torch.empty(b, n, dtype=torch.float32, device=dev)
        per_body = torch.empty(b, dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        gv = torch.empty_like(v)
        gt = torch.empty(b, 3, dtype=torch.float32, device=dev)
        nbytes = L.tuch_point_cloud_fit_scratch_bytes(b, n)
        scratch = _workspace(nbytes, dev)
        # (the cosine and the table select the form: an oriented cloud asked without them answers the plain term)
        normals = None if cos is None else cloud.point_normals
        faces, off, ids = table or (None, None, None)
        _C.check(L.tuch_point_cloud_fit_terms(
            _C.ptr(cloud._ws), cloud._nbytes, _C.ptr(cloud.points), _C.ptr(cloud.counts), _C.ptr(cloud.weights),
            _C.ptr(normals), cos or 0.0, _C.ptr(faces), _C.ptr(off), _C.ptr(ids), 0 if faces is None else int(faces.shape[0]),
            _C.ptr(cloud._cones), cloud._cones_bytes(), _C.ptr(v), _C.ptr(tr), _C.ptr(hint), tau, b, cloud.num_points, n,
            _C.ptr(vw), layout, rho, sigma, scale, _C.ptr(d2), _C.ptr(index), _C.ptr(_ticket(dev)), _C.ptr(per_body),
            _C.ptr(out), _C.ptr(gv), _C.ptr(gt), _C.ptr(scratch), nbytes, _C.stream()))
        ctx.save_for_backward(gv, gt)
        ctx.in_dtypes = (verts.dtype, transl.dtype)
        ctx.mark_non_differentiable(per_body, d2)
        ctx.set_materialize_grads(False)
        return out[0], per_body, d2

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_others):
        return _hand_over(ctx, g, 13)


def cloud_fit(cloud: PointCloud, verts, transl, vertex_weights=None, hint=None, rho='distance', sigma=None,
              max_distance=None, scale=1.0, index_out=None, max_angle=None, normal_table=None):
    """Model -> scan data term of a two-sided fit: ``(total, per_body, NearestPoint)``.  The queries are ``verts[b,v] +
    transl[b]`` against ``cloud``; the NearestPoint has the bits of ``cloud.nearest(verts, transl, hint=hint,
    max_distance=max_distance)`` (a vertex of weight 0 is not computed from: -1 / +inf).  per_body[b] = scale sum_v w_v
    rho(d2_v) / sum_v w_v with vertex_weights [V], [B,V] or None (ones) and rho / sigma as in ``scan_fit``; a vertex
    without winner contributes rho(tau^2) under max_distance tau when the body's cloud is not empty, else 0; total is
    their sum over the bodies, differentiable w.r.t. verts and transl with the nearest point held fixed (there is no
    gradient w.r.t. the cloud's points: they are data).  Every sum is fixed-order: the same bits on every call, in
    either mode of ``deterministic()``, for a body alone or in a batch.  hint / index_out as in ``PointCloud.nearest``.
    max_angle (degrees, in (0, 90]) with normal_table (``vertex_normal_table`` of the mesh the vertices belong to), on an
    oriented cloud: a vertex is matched only to points whose normal is within the angle of the vertex's own
    (tuch_point_cloud_fit_terms with normals, still one launch: the kernel forms the posed vertex normals itself).  The
    NearestPoint then has the bits of ``cloud.nearest(verts, transl, ..., query_normals=vertex_normals(verts,
    normal_table), max_angle=max_angle)``; a vertex without an admissible point is one without winner (index -1).
    Normals only decide the match: they get no gradient.  Both or neither must be given.
    There is no host fallback."""
    if not isinstance(cloud, PointCloud):
        raise ValueError('cloud_fit: cloud must be a PointCloud, got %r' % type(cloud).__name__)
    rho, sigma = args.rho_of('cloud_fit', rho, sigma)
    if transl is None or tuple(transl.shape) != (cloud.batch, 3):
        raise ValueError('cloud_fit: transl must be [%d,3], got %s'
                         % (cloud.batch, None if transl is None else tuple(transl.shape)))
    cloud._check_queries('cloud_fit', verts, transl, hint, name='verts')
    b, n = verts.shape[0], verts.shape[1]
    layout, vw = 0, None
    if vertex_weights is not None:
        if tuple(vertex_weights.shape) == (n,):
            layout = 1
        elif tuple(vertex_weights.shape) == (b, n):
            layout = 2
        else:
            raise ValueError('cloud_fit: vertex_weights must be [%d] or [%d,%d], got %s' % (n, b, n, tuple(vertex_weights.shape)))
        _need_hip('cloud_fit', vertex_weights)
        vw = _f32(vertex_weights)
    tau = args.tau_of('cloud_fit', max_distance)
    _need_hip('cloud_fit', index_out)
    index = args.index_out('cloud_fit', index_out, b, n, verts.device)
    cos = None
    if args.both('cloud_fit', 'max_angle', max_angle, 'normal_table', normal_table):
        _check_normal_table('cloud_fit', normal_table, n, verts.device)
        cos = cloud._oriented_cos('cloud_fit', max_angle)
    total, per_body, d2 = _CloudFit.apply(verts, transl, cloud, vw, layout, hint, rho, sigma, tau, float(scale), index, cos,
                                          normal_table)
    return total, per_body, NearestPoint(d2, index)
