"""CPU: the bookkeeping of tuch_amd.backward_pass (pass ids, unit seeds, root nodes, the hand-over between two autograd
nodes) driven by two toy autograd functions -- no kernels.  The consumer is y = 2 x; the producer is the scalar
sum(y) + 3 sum(x) + sum(c): it finds the consumer's node through y.grad_fn and leaves its own gradient for x there, as
ops.objectives._Stage2Tail does with the pose prior's gradient and lbs._SmplLBS's node.  d/dx is 5 however it travels."""
import pytest
import torch

from tuch_amd import backward_pass as bp


class _Consumer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, log):
        ctx.log = log
        ctx.handover = None
        return 2.0 * x

    @staticmethod
    def backward(ctx, g):
        left = bp.take(ctx)
        ctx.log.append(('taken', left))
        return (2.0 * g if left is None else 2.0 * g + left.pose_grad), None


class _Producer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, x, c, log):
        ctx.log, ctx.node = log, y.grad_fn
        ctx.save_for_backward(torch.ones_like(y), torch.ones_like(c))
        return y.sum() + 3.0 * x.sum() + c.sum()

    @staticmethod
    def backward(ctx, g):
        ones, ones_c = ctx.saved_tensors
        unit, root = bp.is_unit_seed(g), bp.is_root(ctx)
        left = bp.leave(ctx.node, bp.Handover(bp.pass_id(), pose_grad=3.0 * g * ones, root=root))
        ctx.log.append(('producer', unit, root, left))
        return g * ones, (None if left else 3.0 * g * ones), g * ones_c, None


def _graph():
    log = []
    x = torch.arange(4, dtype=torch.float32).requires_grad_(True)
    c = torch.zeros(3, requires_grad=True)
    y = _Consumer.apply(x, log)
    return x, c, y, _Producer.apply(y, x, c, log), log


def test_pass_id_is_known_inside_a_backward_pass_only():
    assert bp.pass_id() == -1
    x, c, y, loss, log = _graph()
    seen = []
    y.register_hook(lambda g: seen.append(bp.pass_id()))
    loss.backward()
    assert len(seen) == 1 and seen[0] >= 0
    assert bp.pass_id() == -1


def test_handover_left_and_taken_within_one_pass_arrives_and_the_slot_is_empty_afterwards():
    x, c, y, loss, log = _graph()
    node = y.grad_fn
    bp.backward_scalar(loss)
    (_, unit, root, left), (_, taken) = log
    assert unit and root and left
    assert isinstance(taken, bp.Handover) and taken.root and taken.verts_fixed is None and taken.pass_id >= 0
    assert torch.equal(taken.pose_grad, torch.full((4,), 3.0))
    assert node.handover is None
    assert torch.equal(x.grad, torch.full((4,), 5.0)) and torch.equal(c.grad, torch.ones(3))


def test_handover_of_a_pass_that_never_reached_the_consumer_is_dropped_by_a_later_pass():
    x, c, y, loss, log = _graph()
    node = y.grad_fn
    g_c, = torch.autograd.grad(loss, [c], retain_graph=True)           # bypasses the consumer
    assert torch.equal(g_c, torch.ones(3))
    assert [e[0] for e in log] == ['producer'] and log[0][3]
    assert isinstance(node.handover, bp.Handover)                      # left behind
    g_x, = torch.autograd.grad(y.sum(), [x], retain_graph=True)        # a later pass through the consumer alone
    assert log[-1] == ('taken', None)                                  # not taken ...
    assert node.handover is None                                       # ... and the slot is cleared
    assert torch.equal(g_x, torch.full((4,), 2.0))
    g_x, = torch.autograd.grad(loss, [x])                              # and a whole pass still adds up
    assert torch.equal(g_x, torch.full((4,), 5.0))


def test_root_is_the_node_backward_scalar_was_called_on_and_nothing_else():
    x, c, y, loss, log = _graph()
    bp.backward_scalar(loss)
    assert log[0][1:3] == (True, True)
    x, c, y, loss, log = _graph()
    bp.backward_scalar(loss + (x ** 2).sum())                          # AddBackward hands the same cached seed on
    assert log[0][1:3] == (True, False)
    assert log[1][1].root is False
    x, c, y, loss, log = _graph()
    loss.backward()
    assert log[0][1:3] == (False, False)
    assert not bp._ROOTS


def test_a_scaled_loss_does_not_arrive_as_the_unit_seed():
    x, c, y, loss, log = _graph()
    bp.backward_scalar(2.0 * loss)
    assert log[0][1:3] == (False, False)
    assert torch.equal(x.grad, torch.full((4,), 10.0))
    assert not bp.is_unit_seed(torch.ones(()))                         # equal values, another tensor


def test_without_a_pass_id_nothing_is_left_or_taken(monkeypatch):
    monkeypatch.setattr(bp, 'pass_id', lambda: -1)
    x, c, y, loss, log = _graph()
    node = y.grad_fn
    bp.backward_scalar(loss)
    assert log == [('producer', True, True, False), ('taken', None)]
    assert node.handover is None
    assert torch.equal(x.grad, torch.full((4,), 5.0))                  # the producer returned its gradient itself
    node.handover = bp.Handover(-1, pose_grad=torch.ones(4))           # (even one put there by hand)
    assert bp.take(node) is None and node.handover is None
    assert not bp.leave(node, bp.Handover(-1)) and node.handover is None


def test_root_registry_is_empty_again_after_a_backward_that_raises():
    class Raises(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.sum()

        @staticmethod
        def backward(ctx, g):
            assert bp.is_root(ctx)
            raise RuntimeError('backward fails')
    loss = Raises.apply(torch.ones(2, requires_grad=True))
    with pytest.raises(RuntimeError, match='backward fails'):
        bp.backward_scalar(loss)
    assert not bp._ROOTS
