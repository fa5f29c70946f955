"""The package's one loop runner (``Stage``) and what its three owners -- ``SMPLifyDC``, ``MeshFitter``, ``ScanFitter`` --
share around it (``LoopOwner``): the loop settings, the call prelude, and the sessions kept between calls.

``Stage.run`` has three modes: eager launches (``use_graph=False``, not a HIP device, ``num_iters <= 4``), unrolled into an
enclosing capture, or three eager iterations + capture + replay (replay only on later calls of a kept session).  One
fallback: a capture that fails (and ``TUCH_GRAPH_STRICT`` unset) is logged, and the rest of the fit runs eagerly through the
same runner.  ``record_history`` and ``TUCH_SMPLIFY_SESSIONS`` do not select other code: the first adds clones around each
iteration, the second decides whether the session outlives the call.
"""
from __future__ import annotations

import contextlib
import gc
import logging
import os

import torch

from . import ops
from .optim import make_adam


class Stage:
    """One Adam loop on a session's static tensors, and the only loop runner: eager launches, unrolled into an enclosing
    capture, or three eager iterations + capture the first time and replays afterwards.  ``owner`` is a ``LoopOwner`` (what
    is read from it is listed there)."""

    def __init__(self, owner, name, params, iteration, adam_kwargs, fuse_backward=False):
        self.owner, self.name, self.params, self.iteration = owner, name, params, iteration
        # fuse_backward (the contact stage 2: parameters = the body model's two pose tensors, objective = one root node):
        # the body model's last backward kernel applies Adam's update itself, step() is then a no-op (optim.py)
        self.optimizer = make_adam(params, owner.step_size, capturable=True, fuse_backward=fuse_backward, **adam_kwargs)
        self.graph, self.verts, self.loss, self.before = None, None, None, None

    def _one(self):
        record = self.owner.record_history
        if record:
            self.before = [p.detach().clone() for p in self.params]
        loss, verts = self.iteration()
        self.optimizer.zero_grad(set_to_none=True)
        ops.backward_scalar(loss)
        self.optimizer.step()
        self.verts, self.loss = verts, loss.detach().clone() if record else loss.detach()

    def run(self, num_iters, collect, capture):
        """Returns whether the loop ran captured (replayed or unrolled); False: eager launches, as asked for or because
        the capture failed -- the caller then runs what is left of the fit eagerly and does not keep the session."""
        owner = self.owner
        for state in self.optimizer.state.values():            # a fresh optimiser per call (smplifydc.py:117,150)
            for v in state.values():
                if torch.is_tensor(v):
                    v.zero_()
        history = owner.history[self.name] if owner.record_history else None

        def iterate(count, step):
            for _ in range(count):
                step()
                if collect is not None:
                    collect.append(self.verts.detach().clone())
                if history is not None:
                    history.append({'loss': self.loss.clone(), 'params': [p.clone() for p in self.before]})
        if not capture:
            iterate(num_iters, self._one)
            return False
        if torch.cuda.is_current_stream_capturing():
            # an ENCLOSING capture is recording (TUCH.forward_train_step --run_smplify captured as one hipGraph: BASELINE
            # config 5): a child graph cannot be replayed into it -- the iterations are unrolled into the enclosing graph
            iterate(num_iters, self._one)
            owner.graph_replayed[self.name] = 0
            return True
        done = 0
        if self.graph is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                iterate(3, self._one)
            torch.cuda.current_stream().wait_stream(side)
            done = 3
            # Python's cycle collector must not run inside the capture.  A fitter and its stages refer to each other, so a
            # dropped fitter's sessions -- captured graphs and their memory pools -- die only when the collector
            # finds them, and destroying a graph while a stream is capturing aborts the process (seen in the test
            # suite: which allocation triggers a collection depends on everything that ran before).  Dead sessions
            # are collected here, before the capture, and the collector rests until the capture has ended.  (The
            # collector's switch is process-wide: two threads capturing at once may re-enable it early for each
            # other, which is then no worse than before.)
            gc.collect()
            collecting = gc.isenabled()
            gc.disable()
            try:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                    self._one()
            except Exception as exc:
                if collecting:
                    gc.enable()
                    collecting = False
                # a loop that cannot be captured still runs (eagerly), but never silently: TUCH_GRAPH_STRICT=1
                # (set by the tests) turns this into an error
                if owner.graph_strict:
                    raise
                logging.getLogger(type(owner).__module__).warning(
                    '%s: hipGraph capture of the %s loop failed (%r); finishing with eager launches',
                    type(owner).__name__, self.name, exc)
                torch.cuda.synchronize()
                self.optimizer.zero_grad()       # a half-recorded fused update must not swallow the next step()
                iterate(num_iters - done, self._one)
                return False
            finally:
                if collecting:
                    gc.enable()
            self.graph = graph
        iterate(num_iters - done, self.graph.replay)
        owner.graph_replayed[self.name] = num_iters - done
        return True


class LoopOwner:
    """Base of the classes that run ``Stage`` loops and keep their sessions between calls.  No ``__init__`` (SMPLifyDC
    keeps the reference's constructor): the subclass calls ``_init_loops`` from its own.

    What a ``Stage`` reads from its owner: ``step_size`` (at construction, Adam's learning rate), ``record_history`` and
    ``history`` (with the flag set, ``history[stage name]`` is the list that receives one ``{'loss', 'params'}`` record per
    iteration, the parameters as they were BEFORE the update), ``graph_strict`` (a failed capture raises instead of
    finishing eagerly) and ``graph_replayed`` (``{stage name: replays of the last call}``; 0 for a loop unrolled into an
    enclosing capture, no entry for an eager one).  The class and module names go into the one warning.

    A session is a dict of whatever a fit with one set of constants holds -- static tensors, closures, stages -- under a
    key of everything its captured loops bake in.  Sessions refer back to their owner through their stages, so a dropped
    owner's graphs live until the cycle collector finds them (``Stage.run`` collects before it captures)."""

    MAX_SESSIONS = 4

    def _init_loops(self, step_size, num_iters, use_graph, record_history):
        self.step_size = step_size
        self.num_iters = num_iters
        # replay each optimisation loop as a hipGraph after three eager iterations (same arithmetic, no per-kernel launch
        # cost: at small batch the loop is launch-bound otherwise)
        self.use_graph = use_graph
        # measurement / test aid: with record_history the objective and the parameters *before* every update are kept per
        # stage in self.history = {stage name: [...]}, the parameters in the optimiser's order
        self.record_history = record_history
        # read once: TUCH_GRAPH_STRICT=1 turns a failed capture into an error (the tests set it), TUCH_SMPLIFY_SESSIONS=0
        # makes every call build its session and capture its loops afresh
        self.graph_strict = os.environ.get('TUCH_GRAPH_STRICT', '0') == '1'
        self.keep_sessions = os.environ.get('TUCH_SMPLIFY_SESSIONS', '1') != '0'
        self.history = None
        self.graph_replayed = {}
        # captured loops are kept between calls: a training step with SMPLify-DC in the loop runs 10 + 10 iterations per
        # call, far too few to pay for two captures each time
        self._sessions = {}

    @contextlib.contextmanager
    def _loops(self, device, on_gpu, *stages):
        """The prelude of a call: a fresh history for ``stages``, the body off the NULL stream (graph replays never run on
        it: ops.off_default_stream), and whether the loops are to be captured."""
        if self.record_history:
            self.history = {name: [] for name in stages}
        with ops.off_default_stream(device) if on_gpu else contextlib.nullcontext():
            yield on_gpu and self.num_iters > 4

    def _session_for(self, key, build, *args):
        """The session stored under ``key``, or ``build(*args)`` (stored, or not, by ``_settle`` once its loops have run)."""
        sess = self._sessions.get(key)
        return build(*args) if sess is None else sess

    def _settle(self, key, sess, captured):
        """Captured loops are kept for the next call; a session that ran eagerly (or lost a capture) is dropped."""
        if not (captured and self.keep_sessions):
            self._sessions.pop(key, None)
        elif key not in self._sessions:
            while len(self._sessions) >= self.MAX_SESSIONS:
                self._sessions.pop(next(iter(self._sessions)))
            self._sessions[key] = sess
