"""GPU: ContactModel.closest_point / signed_distance (csrc/closest_point.hip) against the float64 statement of
tests/closest_point_cases.py: distances, the returned face and weights, bit identity under batching, query order, face
order and replay, padding, a NaN body, the workspace guards, the adjoint against central differences, the signs.

Observed on an MI355X (2026-10-19): largest error / bound of test_distance_face_and_weights 0.21 (tetrahedron; 0.12 - 0.15
for the other meshes), 0.17 at SMPL size; gradients within 2.0e-6 of the largest entry (0.056 of the bound).  DESIGN.md §3."""
import functools

import numpy as np
import pytest
import torch

import closest_point_cases as cc
import helpers
import lbs_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MESHES = ('triangle', 'strip', 'tetrahedron', 'icosphere', 'body122', 'degenerate')
CLOSED = ('tetrahedron', 'icosphere', 'body122')


def _dev(a, **kw):
    return None if a is None else torch.tensor(np.asarray(a), device=DEV, **kw)


@functools.lru_cache(maxsize=None)
def model(name):
    from tuch_amd.ops import ContactModel
    return ContactModel(cc.mesh(name)[1], device=DEV)


def query(m, verts, points, counts=None):
    out = m.closest_point(_dev(verts), _dev(points), None if counts is None else _dev(np.asarray(counts, np.int32)))
    return out.d2.cpu().numpy(), out.face.cpu().numpy(), out.bary.cpu().numpy()


def check_body(what, points, verts, faces, ref_d2, bound, d2, face, bary):
    """Checks 1 and 2 of one body for ALL its queries; returns the largest error / bound."""
    num_faces = len(faces)
    assert d2.dtype == np.float32 and face.dtype == np.int32 and bary.dtype == np.float32
    assert np.all(np.isfinite(d2)) and np.all(np.isfinite(bary)), what
    assert np.all((face >= 0) & (face < num_faces)), what
    err = np.abs(d2.astype(np.float64) - ref_d2)
    via_face = cc.face_d2(points, verts, faces, face)
    corners = np.asarray(verts, np.float64)[np.asarray(faces)[face]]
    nearest = (bary.astype(np.float64)[:, :, None] * corners).sum(1)
    via_bary = ((np.asarray(points, np.float64) - nearest) ** 2).sum(1)
    worst = max((err / bound).max(), (np.abs(via_face - ref_d2) / bound).max(), (np.abs(via_bary - d2) / bound).max())
    assert np.all(err <= bound), (what, int(np.argmax(err / bound)), err.max())
    assert np.all(np.abs(via_face - ref_d2) <= bound), what              # the returned face attains the minimum
    assert np.all(np.abs(via_bary - d2) <= bound), what                  # the weights reproduce d2
    assert np.all(bary >= 0) and np.all(bary <= 1), what
    assert np.all(np.abs(bary.astype(np.float64).sum(1) - 1.0) <= 4 * cc.EPS32), what
    return worst


def check_case(name, c, d2, face, bary):
    worst = 0.0
    for b in range(len(c['verts'])):
        worst = max(worst, check_body('%s body %d' % (name, b), c['points'][b], c['verts'][b], c['faces'], c['ref']['d2'][b],
                                      c['ref']['bound'][b], d2[b], face[b], bary[b]))
    return worst


# Q: one lane, a wavefront less one, exactly one, one more, several with a ragged tail
@pytest.mark.parametrize('count', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('name', MESHES)
def test_distance_face_and_weights(name, batch, count):
    c = cc.case(name, batch, count)
    d2, face, bary = query(model(name), c['verts'], c['points'])
    worst = check_case(name, c, d2, face, bary)
    helpers.report_value('closest_point %s B=%d Q=%d: largest error / bound' % (name, batch, count), worst)


def test_groups_are_the_tree_leaves_or_runs_of_64():
    """What the fixtures are meant to exercise: no tree for the open meshes (one group; three, the last ragged), a tree
    for the closed ones."""
    assert model('triangle').tree_positions() is None and model('strip').tree_positions() is None
    assert len(cc.mesh('strip')[1]) == 130 and len(cc.mesh('triangle')[1]) == 1
    assert model('degenerate').tree_positions() is None
    for name in CLOSED:
        assert model(name).tree_positions() is not None, name
    assert len(cc.mesh('icosphere')[1]) == 320 and cc.mesh('body122')[0].shape[1] == 122


def test_smpl_size_with_the_forearm_through_the_trunk():
    c = cc.case('smpl', 2, 1024)
    assert c['verts'].shape == (2, 6890, 3) and len(c['faces']) == 13776
    d2, face, bary = query(model('smpl'), c['verts'], c['points'])
    worst = check_case('smpl', c, d2, face, bary)
    helpers.report_value('closest_point smpl B=2 Q=1024: largest error / bound', worst)
    helpers.report_value('closest_point smpl B=2 Q=1024: largest |d2 - float64| of the queries near the body',
                         np.abs(d2 - c['ref']['d2'])[np.abs(c['points']).max(2) < 100].max())
    # the body's own vertices pushed 1 mm inward are 1 mm from the surface or nearer (the forearm inside the trunk too)
    v = c['verts'].astype(np.float64)
    inward = (v - 1e-3 * (v - v.mean(1, keepdims=True)) / np.linalg.norm(v - v.mean(1, keepdims=True), axis=2, keepdims=True))
    d2v = query(model('smpl'), c['verts'], inward[:, ::7].astype(np.float32))[0]
    assert d2v.max() <= (1e-3 + 1e-5) ** 2


@pytest.mark.parametrize('name', ['strip', 'icosphere', 'body122'])
def test_same_bits_alone_in_any_batch_position_in_any_query_order_and_twice(name):
    c = cc.case(name, 3, 257)
    m = model(name)
    first = query(m, c['verts'], c['points'])
    for a, b in zip(first, query(m, c['verts'], c['points'])):
        assert np.array_equal(a, b)
    for b in range(3):                                  # alone
        for a, got in zip(first, query(m, c['verts'][b:b + 1], c['points'][b:b + 1])):
            assert np.array_equal(a[b], got[0]), (name, b)
    order = [2, 0, 1]                                   # another position in the batch
    for a, got in zip(first, query(m, c['verts'][order], c['points'][order])):
        assert np.array_equal(a[order], got), name
    perm = np.random.default_rng(1).permutation(257)    # the queries in another order: other neighbours in the wavefront
    for a, got in zip(first, query(m, c['verts'], c['points'][:, perm])):
        assert np.array_equal(a[:, perm], got), name
    # fewer queries: other blocks
    for a, got in zip(first, query(m, c['verts'], c['points'][:, 100:165])):
        assert np.array_equal(a[:, 100:165], got), name


def test_captured_replay_equals_eager():
    c = cc.case('body122', 3, 257)
    m = model('body122')
    verts, points, counts = _dev(c['verts']), _dev(c['points']), _dev(np.array([257, 0, 100], np.int32))
    eager = [x.clone() for x in m.closest_point(verts, points, counts)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                          # warm-up off the capture
        m.closest_point(verts, points, counts)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.closest_point(verts, points, counts)
    for x in out:
        x.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(out._fields, eager, out):
        assert torch.equal(a, b), name


def test_strip_faces_in_another_order_regroups_them_and_changes_nothing():
    """The open strip's groups are runs of 64 faces in index order: permuting the faces puts every face into another
    group with other neighbours and other boxes.  d2 must not move by a bit (pruning is conservative, the distance is
    a function of the pair), and the face is the same one wherever the float64 runner-up is farther than the bound."""
    from tuch_amd.ops import ContactModel
    c = cc.case('strip', 3, 257)
    faces = c['faces']
    perm = np.random.default_rng(3).permutation(len(faces))
    d2, face, _ = query(model('strip'), c['verts'], c['points'])
    d2p, facep, _ = query(ContactModel(faces[perm], device=DEV), c['verts'], c['points'])
    assert np.array_equal(d2, d2p)
    clear = 0
    for b in range(3):
        second = cc.runner_up(c['points'][b], c['verts'][b], faces)
        sure = second - c['ref']['d2'][b] > 2 * c['ref']['bound'][b]
        assert np.array_equal(perm[facep[b]][sure], face[b][sure])
        clear += int(sure.sum())
    assert clear > 150                                   # (the random queries are clear of ties)


def test_other_leaf_sizes_give_the_same_bits(monkeypatch):
    """The closed meshes' groups are the cluster tree's leaves: trees with other leaf sizes group the faces otherwise."""
    from tuch_amd.ops import ContactModel
    for name in ('icosphere', 'body122'):
        c = cc.case(name, 3, 257)
        first = query(model(name), c['verts'], c['points'])
        for leaf in ('8', '20'):
            monkeypatch.setenv('TUCH_TREE_LEAF_FACES', leaf)
            other = ContactModel(c['faces'], device=DEV)
            got = query(other, c['verts'], c['points'])             # (the model's tables are built at its first call)
            for a, b in zip(first, got):
                assert np.array_equal(a, b), (name, leaf)


def test_padding_ragged_counts():
    c = cc.case('icosphere', 3, 257)
    m = model('icosphere')
    full = query(m, c['verts'], c['points'])
    counts = [257, 0, 65]
    d2, face, bary = query(m, c['verts'], c['points'], counts)
    for b, n in enumerate(counts):
        for a, got in zip(full, (d2, face, bary)):
            assert np.array_equal(a[b, :n], got[b, :n])
        assert np.all(np.isposinf(d2[b, n:])) and np.all(face[b, n:] == -1) and np.all(bary[b, n:] == 0)
    # counts beyond Q or below 0 are clamped
    d2c, facec, _ = query(m, c['verts'], c['points'], [1000, -5, 64])
    assert np.array_equal(d2c[0], full[0][0]) and np.all(facec[1] == -1) and np.all(facec[2, 64:] == -1)
    empty = m.closest_point(_dev(c['verts']), _dev(c['points'][:, :0]))
    assert empty.d2.shape == (3, 0) and empty.bary.shape == (3, 0, 3)


@pytest.mark.parametrize('name', ['strip', 'body122'])
def test_nan_body_leaves_the_others_alone(name):
    c = cc.case(name, 3, 257)
    m = model(name)
    clean = query(m, c['verts'], c['points'])
    verts, points = c['verts'].copy(), c['points'].copy()
    verts[1, ::5] = np.nan
    verts[1, 3] = np.inf
    points[1, ::9] = np.nan
    points[1, 4] = -np.inf
    d2, face, bary = query(m, verts, points)
    for b in (0, 2):
        for a, got in zip(clean, (d2, face, bary)):
            assert np.array_equal(a[b], got[b]), (name, b)
    assert np.all((face >= -1) & (face < len(c['faces'])))
    verts[1] = np.nan                                    # nothing finite at all
    face = query(m, verts, points)[1]
    assert np.all((face >= -1) & (face < len(c['faces'])))


def test_workspace_guards_stay_intact():
    from tuch_amd.ops import ContactModel
    for name, batch, count in (('strip', 3, 257), ('icosphere', 1, 65), ('smpl', 2, 1024)):
        c = cc.case(name, batch, count)
        m = ContactModel(c['faces'], device=DEV)
        m.set_option('canary', 1)
        assert m.canary_selftest() == 1
        m.canary_hits()
        d2 = query(m, c['verts'], c['points'])[0]
        assert m.canary_hits() == 0
        assert np.array_equal(d2, query(model(name), c['verts'], c['points'])[0])


# ---------------------------------------------------------------------------------------------------------- adjoint
@functools.lru_cache(maxsize=None)
def adjoint_case(name, batch=2, count=65):
    poses, faces = cc.mesh(name)
    verts = cc.body_batch(poses[0], batch, seed=5)
    points = np.stack([cc.interior_queries(verts[b], faces, count, seed=20 + b, height=(0.005, 0.03)) for b in range(batch)])
    rng = np.random.default_rng(9)
    upstream = (0.5 + rng.random((batch, count))).astype(np.float32)
    gp, gv = zip(*[cc.d2_sum_and_gradients(points[b], verts[b], faces, upstream[b]) for b in range(batch)])
    return dict(verts=verts, faces=faces, points=points, upstream=upstream, gp=np.stack(gp), gv=np.stack(gv))


def _assert_interior_with_margin(c):
    """A condition on the INPUTS: every query's nearest point is inside a face, every weight >= 0.1, and the next face is
    at least 1 mm farther: the closest feature is constant around the query and the envelope form exact."""
    for p, v in zip(c['points'], c['verts']):
        d2, face = cc.statement(p, v, c['faces'])
        w = cc.projection_weights(p.astype(np.float64), v.astype(np.float64)[c['faces'][face]])
        assert w.min() >= 0.1
        assert np.all(np.sqrt(cc.runner_up(p, v, c['faces'])) - np.sqrt(d2) >= 1e-3)
        assert np.sqrt(d2).min() >= 4e-3


def _gradients(m, c, scale=1.0):
    v, p = _dev(c['verts'], requires_grad=True), _dev(c['points'], requires_grad=True)
    out = m.closest_point(v, p)
    assert out.d2.requires_grad and not out.face.requires_grad and not out.bary.requires_grad
    (scale * (out.d2 * _dev(c['upstream'])).sum()).backward()
    return p.grad.cpu().numpy(), v.grad.cpu().numpy()


@pytest.mark.parametrize('name', ['icosphere', 'body122'])
def test_adjoint_against_central_differences(name):
    from tuch_amd import ops
    c = adjoint_case(name)
    _assert_interior_with_margin(c)
    m = model(name)
    with ops.deterministic_mode(True):
        gp, gv = _gradients(m, c)
        gp2, gv2 = _gradients(m, c)
    assert np.array_equal(gp, gp2) and np.array_equal(gv, gv2)              # bit-reproducible
    helpers.grad_close(gp, c['gp'], lbs_cases.GRAD_FLOOR, 'closest_point %s grad_points' % name)
    helpers.grad_close(gv, c['gv'], lbs_cases.GRAD_FLOOR, 'closest_point %s grad_verts' % name)
    with ops.deterministic_mode(False):
        gpa, gva = _gradients(m, c)
    assert np.array_equal(gpa, gp)                                          # (no scatter in this one)
    helpers.grad_close(gva, c['gv'], lbs_cases.GRAD_FLOOR, 'closest_point %s grad_verts, float atomics' % name)
    with ops.deterministic_mode(True):
        gps, gvs = _gradients(m, c, scale=2.5)
    helpers.grad_close(gps, 2.5 * c['gp'], lbs_cases.GRAD_FLOOR, 'closest_point %s grad_points x 2.5' % name)
    helpers.grad_close(gvs, 2.5 * c['gv'], lbs_cases.GRAD_FLOOR, 'closest_point %s grad_verts x 2.5' % name)


def test_adjoint_skips_padding_and_one_input_at_a_time():
    c = adjoint_case('icosphere')
    m = model('icosphere')
    counts = _dev(np.array([65, 20], np.int32))
    v, p = _dev(c['verts'], requires_grad=True), _dev(c['points'], requires_grad=True)
    d2 = m.closest_point(v, p, counts).d2
    torch.where(torch.isfinite(d2), d2, torch.zeros_like(d2)).sum().backward()
    assert torch.isfinite(p.grad).all() and torch.isfinite(v.grad).all()
    assert torch.equal(p.grad[1, 20:], torch.zeros(45, 3, device=DEV)) and p.grad[1, :20].abs().sum() > 0
    gp_only = torch.autograd.grad(m.closest_point(_dev(c['verts']), p).d2.sum(), [p])[0]
    gv_only = torch.autograd.grad(m.closest_point(v, _dev(c['points'])).d2.sum(), [v])[0]
    both = torch.autograd.grad(m.closest_point(v, p).d2.sum(), [p, v])
    assert torch.equal(gp_only, both[0]) and torch.equal(gv_only, both[1])


# ---------------------------------------------------------------------------------------------------------- signs
@pytest.mark.parametrize('name', CLOSED)
def test_signed_distance(name):
    poses, faces = cc.mesh(name)
    verts = poses[:1]
    points = cc.offset_queries(verts[0], faces, 200, seed=2)
    assert len(points) >= 100
    d2, _ = cc.statement(points, verts[0], faces)
    w = cc.winding_number(points, verts[0], faces)
    assert np.sqrt(d2).min() >= 1e-4 and np.abs(w - 0.99).min() > 1e-4            # conditions on the inputs
    inside = w > 0.99
    assert inside.any() and (~inside).any()
    m = model(name)
    v, p = _dev(verts, requires_grad=True), _dev(points[None], requires_grad=True)
    sd = m.signed_distance(v, p)
    got = sd.detach().cpu().numpy()[0]
    assert np.array_equal(got < 0, inside), np.nonzero((got < 0) != inside)[0]
    assert torch.equal(sd.detach().abs(), torch.sqrt(m.closest_point(v, p).d2.detach()))
    bound = cc.reference(points[None], verts, faces)['bound'][0]
    assert np.all(np.abs(got.astype(np.float64) ** 2 - d2) <= bound + 4 * cc.EPS32 * d2)
    sd.abs().sum().backward()                                                       # the magnitude is differentiable
    unit = np.linalg.norm(p.grad.cpu().numpy()[0], axis=1)
    assert np.all(np.abs(unit - 1.0) <= 1e-3)                                        # |grad of a distance| = 1
    padded = m.signed_distance(v, p, _dev(np.array([10], np.int32)))
    assert torch.equal(padded[0, :10], sd[0, :10].detach()) and torch.isposinf(padded[0, 10:]).all()


def test_signed_distance_needs_a_closed_mesh():
    from tuch_amd._C import TuchError
    c = cc.case('strip', 1, 65)
    with pytest.raises(TuchError, match='cluster tree'):
        model('strip').signed_distance(_dev(c['verts']), _dev(c['points']))


def test_wrong_shapes_raise():
    from tuch_amd._C import TuchError
    c = cc.case('strip', 3, 65)
    with pytest.raises(TuchError):
        model('strip').closest_point(_dev(c['verts'][:2]), _dev(c['points']))
    with pytest.raises(TuchError):
        model('strip').closest_point(_dev(c['verts'][:, :-1]), _dev(c['points']))
