"""Host: the loop runner (fit_loop.Stage) in its eager mode on host tensors, the session keeper of fit_loop.LoopOwner on
plain dicts, and what the three owners -- SMPLifyDC, MeshFitter, ScanFitter -- take from the base class.  No device."""
import inspect
import types

import torch


def _owner(step_size=1e-2, record_history=True):
    """The five attributes Stage reads from its owner."""
    return types.SimpleNamespace(step_size=step_size, record_history=record_history, history={'fit': []}, graph_strict=False,
                                 graph_replayed={})


def test_stage_runs_eagerly_on_host_tensors():
    from tuch_amd.fit_loop import Stage
    start = torch.tensor([0.0, 1.0, -2.0])
    x = start.clone().requires_grad_(True)
    owner = _owner()
    stage = Stage(owner, 'fit', [x], lambda: (((x - 0.5) ** 2).sum(), x), {})
    assert stage.run(5, None, False) is False and owner.graph_replayed == {}
    first = x.detach().clone()
    # the same bits as five steps of torch's Adam, the recorded parameters being those BEFORE each update
    y = start.clone().requires_grad_(True)
    adam = torch.optim.Adam([y], lr=owner.step_size)
    history = owner.history['fit']
    assert len(history) == 5
    for record in history:
        assert len(record['params']) == 1 and torch.equal(record['params'][0], y.detach())
        adam.zero_grad()
        loss = ((y - 0.5) ** 2).sum()
        assert torch.equal(record['loss'], loss.detach())
        loss.backward()
        adam.step()
    assert torch.equal(first, y.detach()) and not torch.equal(first, start)
    # every run starts from a fresh optimiser state
    with torch.no_grad():
        x.copy_(start)
    owner.history = {'fit': []}
    collected = []
    assert stage.run(5, collected, False) is False
    assert torch.equal(x.detach(), first) and len(collected) == 5 and len(owner.history['fit']) == 5


def _keeper(monkeypatch, sessions=None):
    from tuch_amd.fit_loop import LoopOwner
    if sessions is not None:
        monkeypatch.setenv('TUCH_SMPLIFY_SESSIONS', sessions)
    else:
        monkeypatch.delenv('TUCH_SMPLIFY_SESSIONS', raising=False)
    owner = LoopOwner()
    owner._init_loops(1e-2, 10, True, False)
    return owner


def test_keeper_holds_four_captured_sessions(monkeypatch):
    owner = _keeper(monkeypatch)
    assert owner.MAX_SESSIONS == 4 and owner.keep_sessions and owner._sessions == {} and owner.history is None
    sessions = {k: {'name': k} for k in 'abcde'}
    built = []
    build = lambda k: built.append(k) or sessions[k]
    assert owner._session_for('a', build, 'a') is sessions['a'] and built == ['a'] and owner._sessions == {}
    owner._settle('a', sessions['a'], True)
    assert list(owner._sessions) == ['a']
    assert owner._session_for('a', build, 'a') is sessions['a'] and built == ['a']          # stored: not built again
    for k in 'bcde':
        owner._settle(k, sessions[k], True)
    assert list(owner._sessions) == ['b', 'c', 'd', 'e']                 # the first-inserted went, the order stays
    owner._settle('b', {'name': 'another b'}, True)                      # a stored key: neither re-inserted nor moved
    assert list(owner._sessions) == ['b', 'c', 'd', 'e'] and owner._sessions['b'] is sessions['b']
    owner._settle('c', sessions['c'], False)                             # ran eagerly or lost its capture: dropped
    assert list(owner._sessions) == ['b', 'd', 'e']
    owner._settle('x', {}, False)
    assert list(owner._sessions) == ['b', 'd', 'e']


def test_keeper_stores_nothing_with_sessions_off(monkeypatch):
    owner = _keeper(monkeypatch, sessions='0')
    assert not owner.keep_sessions
    for k in 'ab':
        owner._settle(k, {}, True)
        assert owner._sessions == {}


def test_prelude_resets_the_history_and_sets_the_capture_threshold(monkeypatch):
    owner = _keeper(monkeypatch)
    for num_iters, on_gpu, want in ((10, False, False), (4, False, False), (0, False, False)):
        owner.num_iters = num_iters
        with owner._loops(torch.device('cpu'), on_gpu, 'fit') as capture:
            assert not capture and capture == want
    assert owner.history is None                                         # record_history is off
    owner.record_history = True
    with owner._loops(torch.device('cpu'), False, 'stage1', 'stage2'):
        owner.history['stage1'].append(1)
    with owner._loops(torch.device('cpu'), False, 'stage1', 'stage2'):
        assert owner.history == {'stage1': [], 'stage2': []}


def test_flags_and_classes(monkeypatch):
    from tuch_amd import fit_loop
    from tuch_amd.fit import BodyFitter, MeshFitter, ScanFitter
    from tuch_amd.smplify.smplifydc import SMPLifyDC
    smpl = types.SimpleNamespace(v_template=torch.zeros(12, 3))
    monkeypatch.delenv('TUCH_GRAPH_STRICT', raising=False)
    assert not MeshFitter(smpl).graph_strict
    monkeypatch.setenv('TUCH_GRAPH_STRICT', '1')
    fitter = MeshFitter(smpl)
    assert fitter.graph_strict and fitter.keep_sessions
    assert (fitter.step_size, fitter.num_iters, fitter.use_graph, fitter.record_history) == (1e-2, 5000, True, False)
    assert fitter.history is None and fitter.graph_replayed == {} and fitter._sessions == {}
    assert ScanFitter(smpl, types.SimpleNamespace(num_verts=12)).graph_strict
    for cls in (SMPLifyDC, MeshFitter, ScanFitter):
        assert issubclass(cls, fit_loop.LoopOwner)
    assert issubclass(MeshFitter, BodyFitter) and issubclass(ScanFitter, BodyFitter)
    assert '__init__' not in vars(fit_loop.LoopOwner)
    assert SMPLifyDC._Stage is fit_loop.Stage
    assert list(inspect.signature(SMPLifyDC.__init__).parameters) == [
        'self', 'step_size', 'batch_size', 'num_iters', 'focal_length', 'geodistssmpl', 'geothres', 'euclthres', 'device',
        'smpl', 'pose_prior', 'ign_joints', 'smpl_model_dir', 'prior_folder', 'use_graph', 'record_history']
    assert list(inspect.signature(SMPLifyDC.__call__).parameters) == [
        'self', 'init_pose', 'init_betas', 'init_cam_t', 'camera_center', 'keypoints_2d', 'use_contact', 'contactlist',
        'gt_contact', 'ignore_idxs', 'has_discrete_contact', 'has_gt_keypoints', 'contact_loss_weight',
        'contact_loss_return', 'segments']
