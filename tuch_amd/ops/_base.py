"""Plumbing every module of this package shares: float32 views, the stream helpers and their companion streams, the
deterministic switch (csrc/api.hip), the byte workspaces the ``*_workspace_bytes`` entry points size
(csrc/workspace.hip), arrival tickets, the cache of derived per-call tensors and the hand-over of unit gradients.

State lives here once: _SIDE_STREAMS, _STREAM_OBJECTS, _GRAPH_STREAMS, _TICKETS and _DERIVED are changed in place and
never rebound; no other module keeps a copy."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from .. import _C, backward_pass


def _f32(t: torch.Tensor) -> torch.Tensor:
    if t.dtype is torch.float32 and t.is_contiguous():       # (the usual case: one call instead of three on the eager path)
        return t.detach()
    return t.detach().to(torch.float32).contiguous()


_SIDE_STREAMS = {}
_STREAM_OBJECTS = {}


def _current_stream(device) -> 'torch.cuda.Stream':
    """torch.cuda.current_stream(device) without building a new Stream object through torch's device-index helpers on
    every call (~9 us, several times per eager step): one object per (device, raw stream handle) is kept."""
    raw, cur = _C._raw_stream, _C._cur_device
    if raw is None or cur is None:
        return torch.cuda.current_stream(device)
    index = device.index if device.index is not None else cur()
    key = (index, raw(index))
    s = _STREAM_OBJECTS.get(key)
    if s is None:
        s = _STREAM_OBJECTS[key] = torch.cuda.current_stream(device)
    return s


def _side_stream(device) -> 'torch.cuda.Stream':
    """The companion stream of the CURRENT stream (one per stream: callers that run several fits on streams of
    their own must not be coupled through a shared side stream)."""
    key = (device.type, device.index, _current_stream(device).cuda_stream)
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return s


_GRAPH_STREAMS = {}


@contextlib.contextmanager
def off_default_stream(device):
    """Run the body on a non-default stream when the current stream is the legacy default (NULL) stream.

    hipGraph replays on the NULL stream are not reliably ordered against the kernels, copies and memsets enqueued
    around them (ROCm 7.2, graphs with forked branches: observed as stale inputs / un-reset optimiser state in about
    every second call, never on a created stream).  Every place in this package that replays a captured graph does it
    inside this context; the two streams are joined with events on entry and exit, so callers see stream semantics."""
    device = torch.device(device)
    cur = torch.cuda.current_stream(device)
    if cur != torch.cuda.default_stream(device):
        yield cur
        return
    key = (device.index if device.index is not None else torch.cuda.current_device())
    s = _GRAPH_STREAMS.get(key)
    if s is None:
        s = _GRAPH_STREAMS[key] = torch.cuda.Stream(device=device)
    s.wait_stream(cur)
    try:
        with torch.cuda.stream(s):
            yield s
    finally:
        cur.wait_stream(s)


def deterministic() -> bool:
    """Deterministic mode of the library (include/tuch_amd.h: tuch_set_deterministic): on unless TUCH_DETERMINISTIC=0."""
    return bool(_C.lib().tuch_get_deterministic())


@contextlib.contextmanager
def deterministic_mode(on: bool):
    """``with ops.deterministic_mode(False): ...`` -- the mode for the calls inside, the previous one restored after."""
    before = deterministic()
    set_deterministic(on)
    try:
        yield
    finally:
        set_deterministic(before)


def set_deterministic(on: bool) -> None:
    """True (the default): gradient scatters through 64-bit fixed-point integer atomics instead of float atomics: an SMPLify-DC fit reproduces
    bit for bit (stage-2 tail, SMPL adjoint, the training loss's plain term -- _ContactTerms -- and its HD term).
    Graphs captured before the switch keep the mode they were captured in."""
    _C.lib().tuch_set_deterministic(int(bool(on)))


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


_TICKETS = {}


def _ticket(device) -> torch.Tensor:
    """A zeroed int: the arrival counter of kernels whose last block finishes the job (they leave it zero).
    Eager calls: one per (device, stream) -- calls on one stream are ordered, so they can share it; another stream gets its
    own.  Under hipGraph capture: a counter of the call's own, allocated from the capturing graph's pool and cleared by a
    memset node of that graph -- a captured graph may be replayed on ANY stream, beside other graphs that were captured on
    the same (shared) capture stream, so a counter keyed by the capture stream would be shared by launches that are not
    ordered against each other (and would live in the pool of whichever graph happened to be captured first)."""
    if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
        return torch.zeros(1, dtype=torch.int32, device=device)
    key = (device.index, _current_stream(device).cuda_stream)
    t = _TICKETS.get(key)
    if t is None:
        t = _TICKETS[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


_DERIVED = {}


def cached_derived(key_tensors, build):
    """Small per-call tensors derived from caller inputs that do not change between iterations
    (validity / selection masks): rebuilt only when an input was modified in place or replaced.  The
    entry holds its source tensors, so their addresses cannot be reused while it is cached.  A captured
    hipGraph holds the address of the derived tensor: entries are kept for 256 distinct inputs before the oldest
    is dropped, far more than the graphs a process keeps alive at once."""
    key = tuple((t.data_ptr(), t._version, tuple(t.shape)) if t is not None else None for t in key_tensors)
    hit = _DERIVED.get(key)
    if hit is None:
        while len(_DERIVED) >= 256:
            _DERIVED.pop(next(iter(_DERIVED)))
        hit = (build(), key_tensors)
        _DERIVED[key] = hit
    return hit[0]


def _need_hip(what, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('%s runs on a HIP device (there is no host fallback); got a tensor on %s' % (what, t.device))


def _hand_over(ctx, g, num_inputs, expand=None):
    """backward() of the fit terms (_VertexFit, _ScanFit, _CloudFit): the saved unit gradients (None where one was not
    asked for), scaled unless the upstream gradient g is the cached unit seed of ops.backward_scalar, then expand(*grads)
    where the inputs that get one are more than the saved tensors, each cast to its input's dtype (ctx.in_dtypes: the
    leading inputs); None for every other input, and for all of them when g is None."""
    if g is None:
        return (None,) * num_inputs
    grads = ctx.saved_tensors
    if not backward_pass.is_unit_seed(g):
        g = g.reshape(()).to(torch.float32)
        grads = tuple(None if x is None else x * g for x in grads)
    if expand is not None:
        grads = expand(*grads)
    return tuple(None if x is None else x.to(d) for x, d in zip(grads, ctx.in_dtypes)) + (None,) * (num_inputs - len(grads))


def _tracked(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)


def as_u8(mask):
    """A [B] boolean / byte mask as uint8 without a copy where the bytes are already there."""
    if mask.dtype == torch.bool and mask.is_contiguous():
        return mask.view(torch.uint8)
    return mask.to(torch.uint8).contiguous()
