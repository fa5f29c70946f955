"""GPU: the normal-compatible closest point (csrc/closest_point.hip: tuch_closest_point with normals), the data term over it
(csrc/scan_fit.hip: tuch_scan_fit_terms with normals) and fit.ScanFitter with scan normals, against the float32 rule and the
float64 admissible-set statement of tests/oriented_point_cases.py: answers, threshold queries, bit identity under
batching, query order, replay, hints and face grouping, the reductions to the plain call, NaN bodies and normals, padding,
the workspace guards, the SMPL-size case, the term with its gradients, the fitter.

Observed on an MI355X (2026-10-20): largest error / bound of test_distance_face_weights_and_no_match 0.44 (icosphere; 0.15 -
0.37 for the other meshes), 4.4e-4 at SMPL size, where 309 of 2048 plain answers lie on a face the rule rejects; term error /
bound at most 0.11 ('squared'); gradients at most 0.15 of the bound.  DESIGN.md section 3, "Normal-compatible closest point"."""
import functools

import numpy as np
import pytest
import torch

import closest_point_cases as cc
import helpers
import oriented_point_cases as oc
import scan_fit_cases as sc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MESHES = ('triangle', 'strip', 'tetrahedron', 'icosphere', 'degenerate', 'body122')
INT32_MAX, INT32_MIN = sc.INT32_MAX, sc.INT32_MIN


def _dev(a, **kw):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV, **kw)


@functools.lru_cache(maxsize=None)
def model(name):
    from tuch_amd.ops import ContactModel
    return ContactModel(cc.mesh(name)[1], device=DEV)


def search(m, verts, points, normals, angle, counts=None, hint=None):
    """ClosestPoint of the oriented call (tensors on the device)."""
    return m.closest_point(_dev(verts), _dev(points), None if counts is None else _dev(np.asarray(counts, np.int32)),
                           None if hint is None else _dev(np.asarray(hint, np.int32)), normals=_dev(normals), max_angle=angle)


def _np(out):
    return out.d2.cpu().numpy(), out.face.cpu().numpy(), out.bary.cpu().numpy()


def _same(a, b, what):
    for field, x, y in zip(('d2', 'face', 'bary'), a, b):
        assert torch.equal(x, y), (what, field)


# ---------------------------------------------------------------------------------------------------------- 1 answers
@pytest.mark.parametrize('angle', oc.ANGLES)
@pytest.mark.parametrize('count', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('name', MESHES)
def test_distance_face_weights_and_no_match(name, batch, count, angle):
    c = oc.case(name, batch, count, angle)
    d2, face, bary = _np(search(model(name), c['verts'], c['points'], c['normals'], angle))
    worst = oc.check_case(name, c, d2, face, bary)
    helpers.report_value('oriented closest_point %s B=%d Q=%d %g deg: largest error / bound' % (name, batch, count, angle), worst)


# ---------------------------------------------------------------------------------------------------------- 2 threshold
def _threshold_batch(name, angle):
    poses, faces = cc.mesh(name)
    verts = cc.body_batch(poses[0], 2, seed=4)
    p, n, f = zip(*[oc.threshold_queries(verts[b], faces, angle, seed=b) for b in range(2)])
    return verts, faces, np.stack(p), np.stack(n), np.stack(f)


def _check_threshold(m, name, angle):
    verts, faces, points, normals, target = _threshold_batch(name, angle)
    out = search(m, verts, points, normals, angle)
    face = out.face.cpu().numpy()
    c = oc.cos32(angle)
    admitted = 0
    for b in range(2):
        rows = np.arange(len(target[b]))
        adm = oc.rule32(verts[b], faces, normals[b], c, pairs=(rows, target[b]))
        assert np.array_equal(face[b] == target[b], adm), (name, angle, b, np.nonzero((face[b] == target[b]) != adm)[0])
        other = face[b][~adm]
        # (whatever else was returned is admissible itself)
        hit = other >= 0
        assert np.all(oc.rule32(verts[b], faces, normals[b][~adm][hit], c, pairs=(np.arange(int(hit.sum())), other[hit])))
        assert adm[2::4].all() and not adm[3::4].any()
        admitted += int(adm[0::4].sum() + adm[1::4].sum())
    return out, admitted


@pytest.mark.parametrize('angle', oc.ANGLES)
@pytest.mark.parametrize('name', ['icosphere', 'body122'])
def test_threshold_queries_follow_the_float32_rule(name, angle):
    _, admitted = _check_threshold(model(name), name, angle)
    helpers.report_value('oriented closest_point %s %g deg: threshold queries at (1 +- 2^-20) the rule admits, of 256'
                         % (name, angle), admitted)


# ---------------------------------------------------------------------------------------------------------- 3 same bits
@pytest.mark.parametrize('name', ['strip', 'icosphere', 'body122'])
def test_same_bits_alone_in_any_batch_position_in_any_query_order_and_twice(name):
    c = oc.case(name, 3, 257, 60.0)
    m = model(name)
    run = lambda v, p, n: search(m, v, p, n, 60.0)
    first = run(c['verts'], c['points'], c['normals'])
    _same(first, run(c['verts'], c['points'], c['normals']), 'twice')
    for b in range(3):                                  # alone
        got = run(c['verts'][b:b + 1], c['points'][b:b + 1], c['normals'][b:b + 1])
        _same([x[b:b + 1] for x in first], got, (name, 'alone', b))
    order = [2, 0, 1]                                   # another position in the batch
    _same([x[order] for x in first], run(c['verts'][order], c['points'][order], c['normals'][order]), (name, 'position'))
    perm = np.random.default_rng(1).permutation(257)    # the queries in another order: other neighbours in the wavefront
    _same([x[:, perm] for x in first], run(c['verts'], c['points'][:, perm], c['normals'][:, perm]), (name, 'order'))
    _same([x[:, 100:165] for x in first], run(c['verts'], c['points'][:, 100:165], c['normals'][:, 100:165]), (name, 'blocks'))


@pytest.mark.parametrize('name', ['strip', 'icosphere', 'body122'])
def test_captured_replay_equals_eager(name):
    c = oc.case(name, 3, 257, 60.0)
    m = model(name)
    verts, points, normals = _dev(c['verts']), _dev(c['points']), _dev(c['normals'])
    counts = _dev(np.array([257, 0, 100], np.int32))
    call = lambda: m.closest_point(verts, points, counts, normals=normals, max_angle=60.0)
    eager = [x.clone() for x in call()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                          # warm-up off the capture
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for x in out:
        x.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    _same(eager, out, name)


# ---------------------------------------------------------------------------------------------------------- 4 hints
HINT_KINDS = ('answer', 'inadmissible', 'random', 'none', 'F', 'int32_max', 'int32_min', 'mix')


def _hints(kind, c, answer, seed=0):
    """hint [B,Q] int32.  'inadmissible': the float64 nearest face of the plain query -- for the queries whose normal is
    that face's flipped the rule rejects it."""
    rng = np.random.default_rng(seed + 17)
    num_faces = len(c['faces'])
    if kind == 'answer':
        out = answer
    elif kind == 'inadmissible':
        out = c['plain']['face']
    elif kind == 'random':
        out = rng.integers(num_faces, size=answer.shape)
    elif kind == 'mix':
        parts = [_hints(k, c, answer, seed) for k in HINT_KINDS[:-1]]
        out = np.choose(rng.integers(len(parts), size=answer.shape), parts)
    else:
        out = np.full(answer.shape, {'none': -1, 'F': num_faces, 'int32_max': INT32_MAX, 'int32_min': INT32_MIN}[kind])
    return np.ascontiguousarray(out).astype(np.int32)


@pytest.mark.parametrize('angle', [30.0, 60.0])
@pytest.mark.parametrize('name', ['strip', 'icosphere', 'body122', 'degenerate'])
def test_hints_change_nothing(name, angle):
    c = oc.case(name, 3, 257, angle)
    m = model(name)
    for counts in (None, [257, 40, 130]):
        plain = search(m, c['verts'], c['points'], c['normals'], angle, counts)
        answer = plain.face.cpu().numpy()
        flipped = np.arange(257) % 4 == 1
        rejected = ~oc.rule32(c['verts'][0], c['faces'], c['normals'][0][flipped], oc.cos32(angle),
                              pairs=(np.arange(int(flipped.sum())), c['plain']['face'][0][flipped]))
        assert rejected.any()                                           # the 'inadmissible' hints are what they claim
        for kind in HINT_KINDS:
            hint = _hints(kind, c, answer)
            _same(plain, search(m, c['verts'], c['points'], c['normals'], angle, counts, hint), (name, angle, kind))


@pytest.mark.parametrize('name', ['strip', 'body122'])
def test_hint_may_alias_the_face_output(name):
    """The C call with face == hint: every lane reads its hint before it writes its face."""
    from tuch_amd import _C
    c = oc.case(name, 3, 257, 60.0)
    m = model(name)
    verts, points, normals = _dev(c['verts']), _dev(c['points']), _dev(c['normals'])
    counts = _dev(np.array([257, 40, 130], np.int32))
    plain = m.closest_point(verts, points, counts, normals=normals, max_angle=60.0)
    L = _C.lib()
    nbytes = L.tuch_closest_point_workspace_bytes(m._handle, 3, 257, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    cosine = float(oc.cos32(60.0))
    for kind in HINT_KINDS:
        both = _dev(_hints(kind, c, plain.face.cpu().numpy()))
        d2, bary = torch.empty_like(plain.d2), torch.empty_like(plain.bary)
        for again in range(2):                                          # the second from what the first left: the loop's use
            _C.check(L.tuch_closest_point(m._handle, _C.ptr(verts), _C.ptr(points), _C.ptr(normals), cosine, _C.ptr(counts),
                                          _C.ptr(both), 3, 257, _C.ptr(d2), _C.ptr(both), _C.ptr(bary), _C.ptr(ws), nbytes,
                                          _C.stream()))
            _same(plain, (d2, both, bary), (name, kind, again))


# ---------------------------------------------------------------------------------------------------------- 5 grouping
@pytest.mark.parametrize('angle', [30.0, 60.0])
def test_strip_faces_in_another_order_regroups_them_and_changes_nothing(angle):
    """Permuted faces: every face in another group with other neighbours, boxes and cones.  d2 and the set of unmatched
    queries must not move by a bit; the face is the same one up to ties (its float64 distance is within the bound)."""
    from tuch_amd.ops import ContactModel
    c = oc.case('strip', 3, 257, angle)
    faces = c['faces']
    perm = np.random.default_rng(3).permutation(len(faces))
    d2, face, _ = _np(search(model('strip'), c['verts'], c['points'], c['normals'], angle))
    d2p, facep, _ = _np(search(ContactModel(faces[perm], device=DEV), c['verts'], c['points'], c['normals'], angle))
    assert np.array_equal(d2, d2p) and np.array_equal(face < 0, facep < 0)
    back = np.where(facep >= 0, perm[np.maximum(facep, 0)], -1)
    same = 0
    for b in range(3):
        hit = face[b] >= 0
        via = cc.face_d2(c['points'][b][hit], c['verts'][b], faces, back[b][hit])
        assert np.all(np.abs(via - c['ref']['d2'][b][hit]) <= c['ref']['bound'][b][hit])
        same += int((back[b][hit] == face[b][hit]).sum())
    assert same > 150


def test_other_leaf_sizes_give_the_same_bits(monkeypatch):
    """Trees with leaves of 8 and 20 faces group the closed meshes' faces otherwise: other boxes and other cones.  A cone
    margin that is not conservative shows here, most at 30 degrees and on the threshold queries."""
    from tuch_amd.ops import ContactModel
    for name in ('icosphere', 'body122'):
        firsts = {}
        for angle in oc.ANGLES:
            c = oc.case(name, 3, 257, angle)
            firsts[angle] = search(model(name), c['verts'], c['points'], c['normals'], angle)
        tv, tf, tp, tn, _ = _threshold_batch(name, 30.0)
        first_threshold = search(model(name), tv, tp, tn, 30.0)
        for leaf in ('8', '20'):
            monkeypatch.setenv('TUCH_TREE_LEAF_FACES', leaf)
            other = ContactModel(cc.mesh(name)[1], device=DEV)
            for angle in oc.ANGLES:                                     # (the model's tables are built at its first call)
                c = oc.case(name, 3, 257, angle)
                _same(firsts[angle], search(other, c['verts'], c['points'], c['normals'], angle), (name, leaf, angle))
            _same(first_threshold, search(other, tv, tp, tn, 30.0), (name, leaf, 'threshold'))
            for angle in (60.0, 90.0):
                _same(_check_threshold(model(name), name, angle)[0], _check_threshold(other, name, angle)[0],
                      (name, leaf, angle, 'threshold'))
            monkeypatch.delenv('TUCH_TREE_LEAF_FACES')


# ---------------------------------------------------------------------------------------------------------- 6 reductions
@pytest.mark.parametrize('name', ['strip', 'icosphere', 'body122', 'degenerate'])
def test_reductions_to_the_plain_call(name):
    c = oc.case(name, 3, 257, 60.0)
    m = model(name)
    verts, points = _dev(c['verts']), _dev(c['points'])
    plain = m.closest_point(verts, points)
    _same(plain, m.closest_point(verts, points, normals=None, max_angle=None), 'None')
    zero = np.zeros_like(c['normals'])
    for angle in oc.ANGLES:
        _same(plain, search(m, c['verts'], c['points'], zero, angle), ('zero normals', angle))
    only1 = zero.copy()
    only1[1] = c['normals'][1]
    got = search(m, c['verts'], c['points'], only1, 60.0)
    full = search(m, c['verts'], c['points'], c['normals'], 60.0)
    for b in (0, 2):
        _same([x[b] for x in plain], [x[b] for x in got], ('body', b))
    _same([x[1] for x in full], [x[1] for x in got], 'body 1')
    assert not torch.equal(plain.face[1], got.face[1])                  # (the filter does change body 1)
    # with a hint, zero normals are still the plain call
    _same(plain, search(m, c['verts'], c['points'], zero, 60.0, hint=plain.face.cpu().numpy()), 'zero normals, hinted')


@pytest.mark.parametrize('name', ['strip', 'body122'])
def test_plain_form_ignores_the_cosine(name):
    """The C call with normals = NULL, whatever max_angle_cos holds, through a workspace of the plain size (no cones): the
    bits of ContactModel.closest_point without normals."""
    from tuch_amd import _C
    c = oc.case(name, 3, 257, 60.0)
    m = model(name)
    verts, points = _dev(c['verts']), _dev(c['points'])
    counts = _dev(np.array([257, 40, 130], np.int32))
    plain = m.closest_point(verts, points, counts)
    L = _C.lib()
    nbytes = L.tuch_closest_point_workspace_bytes(m._handle, 3, 257, 0)
    assert 0 < nbytes < L.tuch_closest_point_workspace_bytes(m._handle, 3, 257, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for cosine in (0.0, 0.5, float('nan')):
        d2, face, bary = torch.empty_like(plain.d2), torch.empty_like(plain.face), torch.empty_like(plain.bary)
        _C.check(L.tuch_closest_point(m._handle, _C.ptr(verts), _C.ptr(points), None, cosine, _C.ptr(counts), None, 3, 257,
                                      _C.ptr(d2), _C.ptr(face), _C.ptr(bary), _C.ptr(ws), nbytes, _C.stream()))
        _same(plain, (d2, face, bary), (name, cosine))


# ---------------------------------------------------------------------------------------------------------- 7 robustness
@pytest.mark.parametrize('name', ['strip', 'body122'])
def test_nan_body_leaves_the_others_alone(name):
    c = oc.case(name, 3, 257, 60.0)
    m = model(name)
    clean = search(m, c['verts'], c['points'], c['normals'], 60.0)
    verts, points, normals = c['verts'].copy(), c['points'].copy(), c['normals'].copy()
    verts[1, ::5] = np.nan
    verts[1, 3] = np.inf
    points[1, ::9] = np.nan
    normals[1, ::7] = np.inf
    for hint in (None, clean.face.cpu().numpy()):
        got = search(m, verts, points, normals, 60.0, hint=hint)
        for b in (0, 2):
            _same([x[b] for x in clean], [x[b] for x in got], (name, b))
        face = got.face.cpu().numpy()
        assert np.all((face >= -1) & (face < len(c['faces'])))
    verts[1] = np.nan                                    # nothing finite at all
    face = search(m, verts, points, normals, 60.0).face.cpu().numpy()
    assert np.all(face[1] == -1)


def test_nan_and_inf_normals_are_unconstrained():
    c = oc.case('icosphere', 3, 257, 60.0)
    m = model('icosphere')
    plain = m.closest_point(_dev(c['verts']), _dev(c['points']))
    full = search(m, c['verts'], c['points'], c['normals'], 60.0)
    normals = c['normals'].copy()
    normals[:, 0::4, 0] = np.nan
    normals[:, 1::4, 1] = np.inf
    normals[:, 2::4] = np.float32(3e19)                                 # the squared length overflows
    got = search(m, c['verts'], c['points'], normals, 60.0)
    for k in (0, 1, 2):
        _same([x[:, k::4] for x in plain], [x[:, k::4] for x in got], k)
    _same([x[:, 3::4] for x in full], [x[:, 3::4] for x in got], 'untouched rows')


def test_padding_ragged_counts():
    c = oc.case('icosphere', 3, 257, 60.0)
    m = model('icosphere')
    full = _np(search(m, c['verts'], c['points'], c['normals'], 60.0))
    for counts in ([257, 0, 65], [1000, -5, 64]):
        d2, face, bary = _np(search(m, c['verts'], c['points'], c['normals'], 60.0, counts))
        for b, n in enumerate(np.clip(counts, 0, 257)):
            for a, got in zip(full, (d2, face, bary)):
                assert np.array_equal(a[b, :n], got[b, :n])
            assert np.all(np.isposinf(d2[b, n:])) and np.all(face[b, n:] == -1) and np.all(bary[b, n:] == 0)


def test_workspace_guards_stay_intact():
    from tuch_amd.ops import ContactModel
    for name, batch, count in (('strip', 3, 257), ('icosphere', 1, 65), ('body122', 3, 257)):
        c = oc.case(name, batch, count, 60.0)
        m = ContactModel(c['faces'], device=DEV)
        m.set_option('canary', 1)
        assert m.canary_selftest() == 1
        m.canary_hits()
        got = search(m, c['verts'], c['points'], c['normals'], 60.0)
        hinted = search(m, c['verts'], c['points'], c['normals'], 60.0, hint=got.face.cpu().numpy())
        assert m.canary_hits() == 0
        want = search(model(name), c['verts'], c['points'], c['normals'], 60.0)
        _same(want, got, name)
        _same(want, hinted, name)


# ---------------------------------------------------------------------------------------------------------- 8 SMPL size
def test_smpl_size_with_the_forearm_through_the_trunk():
    """Queries 5 mm off the surface with the normal of the face they were lifted from, 60 degrees: every query whose plain
    answer lies on a face the rule rejects (another sheet of the surface is nearer) returns a different, admissible face."""
    poses, faces = cc.mesh('smpl')
    verts = poses[:2]
    assert verts.shape == (2, 6890, 3) and len(faces) == 13776
    points, normals = [], []
    for b in range(2):
        p = cc.offset_queries(verts[b], faces, 1400, seed=40 + b)[:1024]
        assert len(p) == 1024
        # the face a query was lifted from: the nearest face of the point moved back onto the surface, i.e. the face whose
        # plane is 5 mm away and holds the projection -- found as the float64 nearest face among those 5 mm away
        rng = np.random.default_rng(40 + b)                             # (offset_queries' own draws, repeated)
        f = np.asarray(faces)[rng.integers(len(faces), size=1400)]
        w = rng.dirichlet(np.ones(3), 1400)
        tri = verts[b].astype(np.float64)[f]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        q = ((w[:, :, None] * tri).sum(1) + 5e-3 * rng.choice([-1.0, 1.0], 1400)[:, None] * n).astype(np.float32)
        keep = np.sqrt(cc.statement(q, verts[b], faces)[0]) >= 2e-4
        assert np.array_equal(q[keep][:1024], p)
        points.append(p)
        normals.append(n[keep][:1024].astype(np.float32))
    points, normals = np.stack(points), np.stack(normals)
    m = model('smpl')
    ref = oc.reference(points, normals, verts, faces, 60.0)
    got = search(m, verts, points, normals, 60.0)
    d2, face, bary = _np(got)
    c = dict(verts=verts, faces=faces, points=points, normals=normals, angle=60.0, ref=ref)
    worst = oc.check_case('smpl', c, d2, face, bary)
    helpers.report_value('oriented closest_point smpl B=2 Q=1024 60 deg: largest error / bound', worst)
    plain = m.closest_point(_dev(verts), _dev(points)).face.cpu().numpy()
    cosine = oc.cos32(60.0)
    changed = 0
    for b in range(2):
        rejected = ~oc.rule32(verts[b], faces, normals[b], cosine, pairs=(np.arange(1024), plain[b]))
        changed += int(rejected.sum())
        assert np.all(face[b][rejected] != plain[b][rejected])
        hit = rejected & (face[b] >= 0)
        assert np.all(oc.rule32(verts[b], faces, normals[b][hit], cosine, pairs=(np.arange(int(hit.sum())), face[b][hit])))
    helpers.report_value('oriented closest_point smpl B=2 Q=1024 60 deg: queries whose plain answer the rule rejects', changed)
    helpers.report_value('oriented closest_point smpl B=2 Q=1024 60 deg: share matched', float((face >= 0).mean()))
    assert changed > 0
    # a hint from the plain answer changes nothing
    _same(got, search(m, verts, points, normals, 60.0, hint=plain), 'smpl hinted')


# ---------------------------------------------------------------------------------------------------------- 9 the term
def _term(m, c, grad_points=True, hint=None, normals='case'):
    from tuch_amd import ops
    v, tr = _dev(c['verts'], requires_grad=True), _dev(c['transl'], requires_grad=True)
    p = _dev(c['points'], requires_grad=grad_points)
    n = _dev(c['normals']) if isinstance(normals, str) else normals
    total, per, near = ops.scan_fit(m, v, tr, p, _dev(c['counts']), _dev(c['weights']), hint, c['rho'], c['sigma'],
                                    normals=n, max_angle=c['angle'])
    ops.backward_scalar(total)
    out = dict(per=per.cpu().numpy(), total=total.item(), gv=v.grad.cpu().numpy(), gt=tr.grad.cpu().numpy(),
               gp=p.grad.cpu().numpy() if grad_points else None)
    return out, near


# 60 degrees: the angle of a fit.  5 degrees: the closed meshes have a face for every direction within 60 degrees, so only
# a narrow angle leaves points of theirs without a match (the random normals between two face normals).
@pytest.mark.parametrize('angle', [60.0, 5.0])
@pytest.mark.parametrize('rho', sc.RHOS)
@pytest.mark.parametrize('count', [64, 65, 257])
@pytest.mark.parametrize('name', ['icosphere', 'body122'])
def test_term_matches_float64_and_unmatched_points_stay_in_the_normaliser(name, count, rho, angle):
    from tuch_amd import ops
    c = oc.term_case(name, 3, count, rho, angle)
    m = model(name)
    got, near = _term(m, c)
    err = np.abs(got['per'].astype(np.float64) - c['per64'])
    helpers.report_value('oriented scan_fit %s Q=%d %s %g deg: largest per-body error / bound' % (name, count, rho, angle),
                         (err / c['bound']).max())
    print('oriented scan_fit', name, count, rho, 'per_body error', err, 'bound', c['bound'])
    assert np.all(err <= c['bound']), (err, c['bound'])
    assert abs(got['total'] - c['per64'].sum()) <= c['bound'].sum()
    # the ClosestPoint is the oriented closest_point's on the shifted points, bit for bit
    shifted = _dev(c['points']) - _dev(c['transl'])[:, None]
    want = m.closest_point(_dev(c['verts']), shifted, _dev(c['counts']), normals=_dev(c['normals']), max_angle=c['angle'])
    _same(want, near, (name, count, rho))
    face = near.face.cpu().numpy()
    unmatched = 0
    for b, n in enumerate(c['counts']):
        assert np.array_equal(face[b, :n] >= 0, c['matched'][b])
        unmatched += int((~c['matched'][b]).sum())
        # an unmatched point: no gradient of its own
        assert not got['gp'][b, :n][~c['matched'][b]].any()
    assert unmatched > 0 or angle == 60.0
    # ... and it keeps its weight: per_body equals the plain term over the matched points with the unmatched at weight 0,
    # times (number matched / number real), up to the rounding of that product -- compared in float64 under the bound
    weights = np.zeros((3, count), np.float32)
    for b, n in enumerate(c['counts']):
        weights[b, :n] = c['matched'][b]
    _, per_w, _ = ops.scan_fit(m, _dev(c['verts']), _dev(c['transl']), _dev(c['points']), _dev(c['counts']), _dev(weights), None,
                               c['rho'], c['sigma'], normals=_dev(c['normals']), max_angle=c['angle'])
    share = np.array([c['matched'][b].sum() / float(n) for b, n in enumerate(c['counts'])])
    assert np.all(np.abs(per_w.cpu().numpy().astype(np.float64) * share - got['per']) <= c['bound'] + 4 * cc.EPS32 * got['per'])
    # a hint changes nothing, and face_out may be the hint tensor
    both = near.face.clone()
    total, per, again = ops.scan_fit(m, _dev(c['verts']), _dev(c['transl']), _dev(c['points']), _dev(c['counts']), None, both,
                                     c['rho'], c['sigma'], face_out=both, normals=_dev(c['normals']), max_angle=c['angle'])
    assert again.face is both
    _same(near, again, 'hinted')
    assert total.item() == got['total'] and np.array_equal(per.cpu().numpy(), got['per'])


@pytest.mark.parametrize('rho', sc.RHOS)
@pytest.mark.parametrize('name', ['icosphere', 'body122'])
def test_gradients_against_central_differences(name, rho):
    from tuch_amd import ops
    c = oc.grad_case(name, rho)
    oc.assert_no_decision_near_threshold(c)
    m = model(name)
    for mode in (True, False):
        with ops.deterministic_mode(mode):
            got, near = _term(m, c)
        assert (near.face >= 0).all()
        for key, what in (('gp', 'points'), ('gt', 'transl'), ('gv', 'verts')):
            ok, ratio = sc.grad_within(got[key], c[key])
            helpers.report_value('oriented scan_fit %s %s grad_%s, deterministic=%d: error / bound' % (name, rho, what, mode), ratio)
            assert ok, (name, rho, what, mode, ratio)


def test_deterministic_mode_gives_equal_bits_twice():
    from tuch_amd import ops
    from tuch_amd.ops._base import _ticket
    for rho in ('distance', 'gmof'):
        c = oc.term_case('body122', 3, 257, rho, 5.0)
        m = model('body122')
        with ops.deterministic_mode(True):
            first, second, third = _term(m, c)[0], _term(m, c)[0], _term(m, c)[0]
        for key in first:
            assert np.array_equal(first[key], second[key]) and np.array_equal(first[key], third[key]), key
    assert int(_ticket(torch.device(DEV)).item()) == 0


def test_term_workspace_guards_stay_intact():
    from tuch_amd import ops
    from tuch_amd.ops import ContactModel
    c = oc.term_case('body122', 3, 257, 'distance')
    guarded = ContactModel(c['faces'], device=DEV)
    guarded.set_option('canary', 1)
    assert guarded.canary_selftest() == 1
    guarded.canary_hits()
    with ops.deterministic_mode(True):
        want, _ = _term(model('body122'), c)
        got, _ = _term(guarded, c)
    assert guarded.canary_hits() == 0
    for key in want:
        assert np.array_equal(want[key], got[key]), key


# ---------------------------------------------------------------------------------------------------------- 10 the fitter
@pytest.fixture(scope='module')
def smpl():
    from tuch_amd.models.smpl import SMPL
    return SMPL(model_data=sc.fit_inputs()['body'], batch_size=sc.FIT_BATCH).to(DEV)


@functools.lru_cache(maxsize=None)
def body_model():
    from tuch_amd.ops import ContactModel
    return ContactModel(sc.fit_inputs()['faces'], device=DEV)


@functools.lru_cache(maxsize=None)
def scan_normals():
    """[B,Q,3] float32: for every real point of the fitter's scan the unit normal of the nearest face of the TRUE posed
    body it was sampled from (NaN rows are padding: zero there)."""
    from oracle import lbs as ol
    c = sc.fit_inputs()
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)
    verts = ol.smpl_forward(ol.model_tensors(c['body'], torch.float64), t(c['true_betas']), t(c['true_body_pose']),
                            t(c['global_orient']))[0].numpy()
    out = np.zeros_like(c['points'])
    for b, n in enumerate(c['counts']):
        q = c['points'][b, :n].astype(np.float64) - c['true_transl'][b]
        near = cc.statement(q, verts[b], c['faces'])[1]
        m = oc.face_normal64(verts[b], c['faces'], near)
        out[b, :n] = m / np.linalg.norm(m, axis=1, keepdims=True)
    return out


def _fitter(smpl, **kw):
    from tuch_amd.fit import ScanFitter
    return ScanFitter(smpl, body_model(), num_iters=sc.FIT_ITERS, fit_global_orient=False, **kw)


def test_fitter_with_zero_normals_is_the_fit_without(smpl):
    from tuch_amd import ops
    c = sc.fit_inputs()
    points, go, counts = _dev(c['points']), _dev(c['global_orient']), _dev(c['counts'])
    with ops.deterministic_mode(True):
        plain = _fitter(smpl)(points, go, counts=counts)
        zero = _fitter(smpl, max_normal_angle=60.0)(points, go, counts=counts, normals=torch.zeros_like(points))
        unused = _fitter(smpl, max_normal_angle=60.0)(points, go, counts=counts)         # the option without normals
    for field, a, b, d in zip(plain._fields, plain, zero, unused):
        assert torch.equal(a, b), field
        assert torch.equal(a, d), field


def test_fitter_with_normals(smpl, monkeypatch):
    from tuch_amd import ops
    monkeypatch.setenv('TUCH_GRAPH_STRICT', '1')
    c = sc.fit_inputs()
    points, go, counts = _dev(c['points']), _dev(c['global_orient']), _dev(c['counts'])
    normals = _dev(scan_normals())
    with ops.deterministic_mode(True):
        hinted = _fitter(smpl, max_normal_angle=60.0, record_history=True)
        first = hinted(points, go, counts=counts, normals=normals)
        assert hinted.graph_replayed == {'fit': sc.FIT_ITERS - 3} and len(hinted._sessions) == 1
        history = hinted.history['fit']
        for name, fit in (('use_hint=False', _fitter(smpl, max_normal_angle=60.0, use_hint=False)),
                          ('eager', _fitter(smpl, max_normal_angle=60.0, use_graph=False)),
                          ('fresh', _fitter(smpl, max_normal_angle=60.0))):
            got = fit(points, go, counts=counts, normals=normals)
            for field, a, b in zip(first._fields, first, got):
                assert torch.equal(a, b), (name, field)
        again = hinted(points, go, counts=counts, normals=normals)      # the kept session
        assert len(hinted._sessions) == 1
        for field, a, b in zip(first._fields, first, again):
            assert torch.equal(a, b), ('kept session', field)
        # the objective before update 0 is a standalone ops.scan_fit with normals on the initial state
        start = history[0]
        bp, be, tr = start['params'][:3]
        verts = smpl(global_orient=go, body_pose=bp, betas=be).vertices
        total, per, _ = ops.scan_fit(body_model(), verts, tr, points, counts, None, None, 'distance', normals=normals,
                                     max_angle=60.0)
        assert total.item() == start['loss'].item()
    assert first.loss.sum().item() < per.sum().item(), (first.loss, per)         # the final loss is below the initial one
    # every returned face is admissible for the final vertices; most points are matched
    final = smpl(global_orient=first.global_orient, body_pose=first.body_pose, betas=first.betas).vertices
    assert torch.equal(final + first.transl[:, None], first.vertices)
    face = first.face.cpu().numpy()
    fv, fn = final.cpu().numpy(), scan_normals()
    for b, n in enumerate(c['counts']):
        assert np.all(face[b, n:] == -1)
        hit = np.nonzero(face[b, :n] >= 0)[0]
        assert np.all(oc.rule32(fv[b], c['faces'], fn[b][hit], oc.cos32(60.0), pairs=(np.arange(len(hit)), face[b][hit])))
    helpers.report_value('ScanFitter with normals, 60 deg: share matched at the final evaluation',
                         float((face >= 0).sum() / c['counts'].sum()))


def test_fitter_normals_need_the_angle(smpl):
    c = sc.fit_inputs()
    points, go = _dev(c['points']), _dev(c['global_orient'])
    with pytest.raises(ValueError, match='max_normal_angle'):
        _fitter(smpl)(points, go, normals=torch.zeros_like(points))
    with pytest.raises(ValueError, match='normals'):
        _fitter(smpl, max_normal_angle=60.0)(points, go, normals=torch.zeros(3, 5, 3, device=DEV))
