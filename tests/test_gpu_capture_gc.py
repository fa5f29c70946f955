"""GPU: Python's cycle collector stays out of the loop runner's capture (SMPLifyDC._Stage.run).  A fitter and its stages
refer to each other, so a dropped fitter's captured graph dies only when the collector finds it; were that to happen while
another loop is being captured, the graph would be destroyed inside the capture.  The runner collects before it captures
and switches the collector off until the capture has ended.  Nothing here provokes that situation: the test looks at the
collector's state from inside a capture, and at whether a dropped fitter's graph is gone by then."""
import functools
import gc
import weakref

import pytest
import torch

import scan_fit_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def body_model():
    from tuch_amd.ops import ContactModel
    return ContactModel(sc.fit_inputs()['faces'], device=DEV)


def test_the_collector_rests_during_the_capture_and_dead_sessions_go_before_it(monkeypatch):
    from tuch_amd import ops
    from tuch_amd.fit import ScanFitter
    from tuch_amd.models.smpl import SMPL
    c = sc.fit_inputs()
    smpl = SMPL(model_data=c['body'], batch_size=sc.FIT_BATCH).to(DEV)
    points, go, counts = (torch.tensor(c[k], device=DEV) for k in ('points', 'global_orient', 'counts'))
    make = lambda: ScanFitter(smpl, body_model(), num_iters=6, fit_global_orient=False)
    assert gc.isenabled()
    dropped = make()
    dropped(points, go, counts=counts)
    graph = weakref.ref(next(iter(dropped._sessions.values()))['stage'].graph)
    assert graph() is not None
    was = gc.isenabled()
    gc.disable()                                                            # (so that only the runner can collect it)
    try:
        del dropped
        assert graph() is not None                                          # a cycle: dropping the fitter frees nothing
        seen = []
        scan_fit = ops.scan_fit

        def watched(*args, **kw):
            if torch.cuda.is_current_stream_capturing():
                seen.append((gc.isenabled(), graph() is None))
            return scan_fit(*args, **kw)
        monkeypatch.setattr(ops, 'scan_fit', watched)
        fitter = make()
        fitter(points, go, counts=counts)
        assert fitter.graph_replayed == {'fit': 3}
        assert seen == [(False, True)], seen       # one captured iteration: collector off, the dropped graph already gone
        assert not gc.isenabled()                                           # the runner restores what it found: off here
    finally:
        if was:
            gc.enable()
    seen.clear()
    again = make()
    again(points, go, counts=counts)
    assert seen == [(False, True)] and gc.isenabled()                       # ... and on where it was on
