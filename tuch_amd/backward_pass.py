"""Which backward pass is running, and the one hand-over between two autograd nodes of the same pass.

ops.objectives._Stage2Tail (the producer: the stage-2 objective) leaves a Handover on the node of lbs._SmplLBS (the consumer: the body
model that made its vertices), whose backward runs later in the same pass and takes it.  The rules:

| decision | condition |
|---|---|
| leave anything at all | the producer found the consumer by identity of body_pose (`pose_ref() is body_pose`), gradients for vertices and pose are wanted, and pass_id() >= 0 |
| hand the fixed-point accumulators over instead of converting them | deterministic mode, unit seed, the producer is the root, vertices unwatched, and the row above |
| otherwise in deterministic mode | one tuch_fixed_to_float launch; a non-unit upstream gradient scales all four gradients |
| the producer returns None for the pose | exactly when something was left (the consumer adds it) |
| Adam inside the consumer's last kernel | pose2rot, a pose_grad was taken, root, no betas gradient wanted, optim.fusable_for returns an optimiser for exactly these two tensor objects with matching storage, and it has not been applied already (else a warning) |
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

_SEEDS = {}     # (device, dtype, shape) -> the cached tensor of ones backward_scalar() seeds a pass with
_ROOTS = {}     # id(node) -> node: the autograd nodes of the losses of the RUNNING backward_scalar() calls (a plain dict:
                # the engine runs a device's nodes on its own worker thread, a thread-local would be invisible there)


def pass_id() -> int:
    """id of the running autograd backward pass (-1 outside one, or where this torch build has no such query)"""
    f = getattr(torch._C, '_current_graph_task_id', None)
    return int(f()) if f is not None else -1


def backward_scalar(loss: torch.Tensor) -> None:
    """``loss.backward()`` for a scalar loss with the seed gradient (ones) taken from a cache: autograd otherwise fills a
    fresh one per call, a launch of its own at the head of every backward chain.  The loss's own autograd node is
    remembered for the duration of the pass: a node that finds ITSELF there (is_root) is the root of the pass -- every
    gradient of the pass flows through what it returns (the seed's address alone does not say so: AddBackward hands it on)."""
    key = (loss.device, loss.dtype, tuple(loss.shape))
    seed = _SEEDS.get(key)
    if seed is None:
        seed = _SEEDS[key] = torch.ones(loss.shape, dtype=loss.dtype, device=loss.device)
    node = loss.grad_fn
    if node is not None:
        _ROOTS[id(node)] = node
    try:
        loss.backward(gradient=seed)
    finally:
        if node is not None:
            _ROOTS.pop(id(node), None)


def is_unit_seed(g: torch.Tensor) -> bool:
    """The upstream gradient IS a cached seed of backward_scalar(): recognised by its address (no device round trip)."""
    return any(g.data_ptr() == seed.data_ptr() for seed in _SEEDS.values())


def is_root(node) -> bool:
    """True inside a backward pass started by backward_scalar() on the output of exactly this autograd node."""
    return node is not None and _ROOTS.get(id(node)) is node


class Handover(NamedTuple):
    """What a producer node leaves for a consumer node of the same backward pass."""
    pass_id: int                                    # the backward pass that left it
    pose_grad: Optional[torch.Tensor] = None        # the prior's pose gradient
    verts_fixed: Optional[torch.Tensor] = None      # the vertex gradient's 64-bit fixed-point accumulators
    root: bool = False                              # the producer was the root of a backward_scalar() pass


def leave(node, handover: Handover) -> bool:
    """Leave it on the consumer's node; False (nothing left: the producer returns its gradients itself) outside a pass."""
    if handover.pass_id >= 0:
        node.handover = handover
    return handover.pass_id >= 0


def take(node):
    """Empty the node's slot; the Handover if a node of THIS backward pass left it, else None (one left by a pass that never
    reached the consumer -- only camera_t asked for -- is dropped here, not added to a later pass's gradient)."""
    handover, node.handover = getattr(node, 'handover', None), None
    return handover if handover is not None and 0 <= handover.pass_id == pass_id() else None
