"""GPU: self-contact detection (csrc/self_contact.hip, tuch_amd/contact_detect.py) against
  * the reference's own TUCH.get_verts_in_contact (tests/golden/make_golden_verts_in_contact.py): exact, nothing left out;
  * a float64 brute force written here (chunks of 512 rows), computed once per (fixture, body, threshold) and shared;
  * the kernels it must agree with bit for bit (v2v_min_masked, region_pair_min);
plus determinism, batch independence, graph replay and the Evaluator's accumulation.

Tolerance against float64: 2e-6 relative on distances.  The float32 evaluation of d^2 from float32 inputs is three exactly
rounded differences, three products and two sums: <= 5e-7 relative, half of that again after the square root.  Decisions
(in contact or not, which signature entries are finite) are compared EXACTLY, after asserting in float64 that no masked
pair lies within 1e-5 relative of the threshold in d^2 (observed: 6e-3 and 1.7e-4 on the V = 1602 golden at 0.02 / 0.05,
8.5e-4 on the full-size fixture).  The observed maxima are logged through helpers.report_value.
"""
import functools

import numpy as np
import pytest
import torch

import golden_io as gio
from helpers import golden, golden_mask, report_value

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
RTOL = 2e-6
MARGIN = 1e-5


# ------------------------------------------------------------------------------------------------ fixtures
@functools.lru_cache(maxsize=None)
def vic():
    """The V = 1602 golden: eight bodies (body 0 without contact), the >= mask, 24 regions, the reference's sets."""
    g = gio.load('verts_in_contact.npz')
    regions, _ = gio.unpack_regions(g)
    return {'verts': g['verts'], 'mask': gio.unpack_mask(g), 'regions': regions,
            'idxs1': gio.unpack_ragged('idxs1', g), 'idxs2': gio.unpack_ragged('idxs2', g)}


@functools.lru_cache(maxsize=None)
def small(kind):
    """V = 122 (uv) / V = 162 (ico): under one workgroup, no multiple of 64.  Five bodies: through_pose(2, 7),
    folded_poses(3, 11)."""
    from oracle import lbs as olbs
    from synthetic import folded_poses, make_body, through_pose
    body = make_body(rings=10, segs=12) if kind == 'uv122' else make_body(topology='ico', freq=4)
    parts = [through_pose(2, 7), folded_poses(3, 11)]
    bp, go, be = [torch.tensor(np.concatenate([np.asarray(p[k], np.float32) for p in parts])) for k in range(3)]
    verts, _ = olbs.smpl_forward(olbs.model_tensors(body), be, bp, go)
    verts = verts.numpy().astype(np.float32)
    assert verts.shape[1] == {'uv122': 122, 'ico162': 162}[kind]
    return {'verts': verts, 'mask': body.geodesics >= 0.3, 'regions': dict(body.regions)}


def full2():
    g = golden('full2')
    regions, pairs = gio.unpack_regions(g)
    return {'verts': g['verts'], 'mask': golden_mask('full2'), 'regions': regions, 'pairs': pairs, 'faces': g['faces']}


def region_variant(regions, name, num_verts):
    """Ordered vertex-id lists for the table variants of the small-shape test."""
    lists = [np.asarray(v, np.int64) for v in regions.values()]
    if name == 'r24':
        return lists
    if name == 'r1':
        return [np.concatenate(lists[:3])]
    if name == 'r80':                                                # 24 regions split into 80 (R > 64); some are empty
        out = []
        for k, r in enumerate(lists):
            out += [np.asarray(p, np.int64) for p in np.array_split(r, 4 if k < 8 else 3)]
        assert len(out) == 80
        return out
    if name == 'overlap':                                            # regions 0 and 1 overlap; ten vertices in no region
        gone = np.arange(3, num_verts, num_verts // 10)[:10]
        lists = [np.setdiff1d(r, gone) for r in lists]
        lists[0] = np.union1d(lists[0], lists[1][: max(1, len(lists[1]) // 2)])
        return lists
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ float64 truth
_TRUTH = {}


def brute_force(verts_b, mask, e, lists=None):
    v = np.asarray(verts_b, np.float64)
    V, e2 = v.shape[0], float(e) ** 2
    min_d2 = np.full(V, np.inf)
    member = None
    if lists is not None:
        member = np.zeros((len(lists), V), bool)
        for r, ids in enumerate(lists):
            member[r, ids] = True
        sig = np.full((len(lists), len(lists)), np.inf)
    margin = np.inf
    for r0 in range(0, V, 512):
        r1 = min(V, r0 + 512)
        d2 = ((v[r0:r1, None, :] - v[None, :, :]) ** 2).sum(-1)
        m = mask[r0:r1]
        if m.any() and e2 > 0:
            margin = min(margin, float(np.abs(d2[m] / e2 - 1.0).min()))
        dq = np.where(m & (d2 < e2), d2, np.inf)
        min_d2[r0:r1] = dq.min(1)
        if member is not None:
            col = np.stack([dq[:, member[r]].min(1, initial=np.inf) for r in range(len(lists))], 1)      # [rows, R]
            for r in range(len(lists)):
                rows = member[r, r0:r1]
                if rows.any():
                    sig[r] = np.minimum(sig[r], col[rows].min(0))
    out = {'min_d2': min_d2, 'in_contact': np.isfinite(min_d2), 'cnc_d2': min_d2.min(), 'margin': margin}
    if member is not None:
        out['sig_d2'] = sig
    return out


def truth(key, verts_b, mask, e, lists=None):
    if key not in _TRUTH:
        _TRUTH[key] = brute_force(verts_b, mask, e, lists)
    return _TRUTH[key]


def rel_err(got, want_d2):
    """max relative error of distances against the roots of float64 squared distances; the inf patterns must be equal."""
    got, want = np.asarray(got, np.float64), np.sqrt(np.asarray(want_d2, np.float64))
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), 'finite pattern differs'
    assert np.all(got[~fin] == np.inf)
    if not fin.any():
        return 0.0
    return float((np.abs(got[fin] - want[fin]) / want[fin]).max())


def check_body(out, b, t, verts_b, mask, e, what):
    """One body of a SelfContact result against its float64 truth `t`; returns the number of vertices in contact."""
    assert t['margin'] > MARGIN, ('a masked pair within %g of the threshold' % MARGIN, what, t['margin'])
    ic = out['in_contact'][b].cpu().numpy()
    assert ic.dtype == np.bool_ and np.array_equal(ic, t['in_contact']), what
    errs = [rel_err(out['dist'][b].cpu().numpy(), t['min_d2']), rel_err(out['cnc'][b].cpu().numpy(), t['cnc_d2'])]
    if 'sig_d2' in t:
        errs.append(rel_err(out['signature'][b].cpu().numpy(), t['sig_d2']))
    else:
        assert 'signature' not in out
    part = out['partner'][b].cpu().numpy()
    assert part.dtype == np.int32 and np.all(part[~ic] == -1), what
    rows = np.where(ic)[0]
    if len(rows):
        p = part[rows].astype(np.int64)
        assert p.min() >= 0 and p.max() < len(ic) and np.all(mask[rows, p]), what
        v = np.asarray(verts_b, np.float64)
        d2 = ((v[rows] - v[p]) ** 2).sum(-1)
        assert np.all(d2 < float(e) ** 2), what
        errs.append(float((d2 / t['min_d2'][rows] - 1.0).max()))
    report_value('self_contact %-52s max rel err' % what, max(errs))
    assert max(errs) <= RTOL, (what, errs)
    return len(rows)


def detector(fx, e, lists=None):
    from tuch_amd.contact_detect import SelfContact
    return SelfContact(geomask=fx['mask'], euclthres=e, regions=lists, device=DEV)


# ------------------------------------------------------------------------------------------------ 1
def test_reference_parity():
    from tuch_amd.contact_detect import SelfContact
    from tuch_amd.train.train_module import TUCH
    g = gio.load('verts_in_contact.npz')
    fx = vic()
    verts = torch.tensor(fx['verts'], device=DEV)
    # the mask stands in for the geodesic distances (1 where >= geothres, 0 elsewhere): `geodists >= geothres` is the mask
    geod = torch.tensor(fx['mask'].astype(np.float32))
    regions, pairs = gio.unpack_regions(g)
    module = TUCH(contactlists={'classes': pairs, 'csig': regions}, faces=np.array([[0, 1, 2], [1, 2, 1601]]),
                  geodistssmpl=geod, device=DEV)
    for name, got in (('TUCH.get_verts_in_contact', module.get_verts_in_contact(verts)),
                      ('SelfContact.verts_in_contact', SelfContact(geod, 0.3, 0.02, device=DEV).verts_in_contact(verts))):
        assert sorted(got) == list(range(8)), name
        for b in range(8):
            i1, i2 = got[b]
            assert i1.dtype == torch.int64 and i2.dtype == torch.int64 and i1.device == verts.device, name
            assert np.array_equal(i1.cpu().numpy(), fx['idxs1'][b]), (name, b)
            assert np.array_equal(i2.cpu().numpy(), fx['idxs2'][b]), (name, b)
        assert got[0][0].numel() == 0 and got[0][1].numel() == 0
    assert [len(a) for a in fx['idxs1']] == [0, 21, 8, 6, 76, 46, 13, 7]


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('e', [0.02, 0.05])
def test_truth_v1602(e):
    fx = vic()
    lists = region_variant(fx['regions'], 'r24', 1602)
    verts = torch.tensor(fx['verts'], device=DEV)
    out = detector(fx, e, lists)(verts)
    assert out['dist'].shape == (8, 1602) and out['signature'].shape == (8, 24, 24) and out['cnc'].shape == (8,)
    counts = []
    for b in range(8):
        t = truth(('vic', b, e, 'r24'), fx['verts'][b], fx['mask'], e, lists)
        counts.append(check_body(out, b, t, fx['verts'][b], fx['mask'], e, 'V=1602 e=%g body %d' % (e, b)))
    if e == 0.02:
        assert counts == [len(a) for a in fx['idxs1']]


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize('kind', ['uv122', 'ico162'])
def test_small_and_awkward_shapes(kind):
    fx = small(kind)
    V = fx['verts'].shape[1]
    total = 0
    for e in (0.05, 0.02):
        for variant in ('r24', 'r1', 'r80', 'overlap', None):
            lists = region_variant(fx['regions'], variant, V) if variant else None
            det = detector(fx, e, lists)
            for bodies in ([0, 1, 2, 3, 4], [0], [3]):                              # B = 5 and B = 1
                out = det(torch.tensor(fx['verts'][bodies], device=DEV))
                assert ('signature' in out) == (variant is not None)
                for k, b in enumerate(bodies):
                    t = truth((kind, b, e, variant), fx['verts'][b], fx['mask'], e, lists)
                    n = check_body(out, k, t, fx['verts'][b], fx['mask'], e, '%s e=%g %s body %d of %d' % (kind, e, variant, b, len(bodies)))
                    total += n if e == 0.05 else 0
    assert total > 0, 'no body of the fixture has contact at 0.05: the test would check nothing'


# ------------------------------------------------------------------------------------------------ 4
def test_dense_hit_path():
    fx = small('ico162')
    lists = region_variant(fx['regions'], 'overlap', 162)
    e = 1e3                                                                           # every masked pair qualifies
    out = detector(fx, e, lists)(torch.tensor(fx['verts'], device=DEV))
    for b in range(5):
        t = truth(('ico162', b, e, 'overlap'), fx['verts'][b], fx['mask'], e, lists)
        check_body(out, b, t, fx['verts'][b], fx['mask'], e, 'dense V=162 body %d' % b)
        assert np.array_equal(out['in_contact'][b].cpu().numpy(), fx['mask'].any(1))


# ------------------------------------------------------------------------------------------------ 5
def test_nothing_qualifies():
    fx = small('uv122')
    lists = region_variant(fx['regions'], 'r24', 122)
    verts = torch.tensor(fx['verts'], device=DEV)
    empty = {'mask': np.zeros_like(fx['mask'])}
    for what, det in (('euclthres 0', detector(fx, 0.0, lists)), ('euclthres < 0', detector(fx, -1.0, lists)),
                      ('all-false mask', detector(empty, 1e3, lists))):
        out = det(verts)
        assert not out['in_contact'].any(), what
        assert (out['partner'] == -1).all(), what
        for k in ('dist', 'cnc', 'signature'):
            assert (out[k] == float('inf')).all(), (what, k)
        got = det.verts_in_contact(verts)
        assert all(got[b][0].numel() == 0 and got[b][1].numel() == 0 for b in range(5)), what


# ------------------------------------------------------------------------------------------------ 6
def test_full_size():
    fx = full2()
    lists = region_variant(fx['regions'], 'r24', 6890)
    out = detector(fx, 0.02, lists)(torch.tensor(fx['verts'], device=DEV))
    for b in range(2):
        t = truth(('full2', b, 0.02, 'r24'), fx['verts'][b], fx['mask'], 0.02, lists)
        n = check_body(out, b, t, fx['verts'][b], fx['mask'], 0.02, 'V=6890 body %d' % b)
        assert n > 100                                                                # (135 and 166 when this was written)


# ------------------------------------------------------------------------------------------------ 7
def test_bit_consistent_with_v2v_and_region_pair_min():
    from tuch_amd import ops
    fx = full2()
    names = list(fx['regions'].keys())
    lists = [np.asarray(fx['regions'][n], np.int64) for n in names]
    pair_idx = np.asarray([[names.index(a), names.index(b)] for a, b in fx['pairs']], np.int64)
    model = ops.ContactModel(fx['faces'], fx['mask'], None, lists, pair_idx, device=DEV)
    verts = torch.tensor(fx['verts'], device=DEV)
    e32 = np.float32(0.02)
    bits = ops.pack_geomask(torch.tensor(fx['mask'], device=DEV))
    vreg = tuple(torch.tensor(a, device=DEV) for a in ops.vertex_region_table(lists, 6890))
    raw = ops.self_contact(verts, bits, float(e32), vreg, len(lists))
    # the model's packed mask gives the same bits as ours
    from tuch_amd.contact_detect import SelfContact
    out = SelfContact(geomask=model, euclthres=float(e32), regions=fx['regions'])(verts)
    assert out['signature'].shape == (2, 24, 24)
    assert torch.equal(out['dist'], torch.sqrt(raw['min_d2'])) and torch.equal(out['partner'], raw['partner'])
    assert torch.equal(out['signature'], torch.sqrt(raw['sig_d2'])) and torch.equal(out['cnc'], torch.sqrt(raw['cnc_d2']))
    # the nearest masked vertex, where it is a contact
    mn, arg = ops.v2v_min_masked(verts, bits)
    ic = raw['in_contact']
    assert int(ic.sum()) > 200
    assert torch.equal(raw['min_d2'][ic], mn[ic]) and torch.equal(raw['partner'][ic], arg[ic])
    assert bool((mn[~ic] >= float(e32 * e32)).all())
    # every listed region pair
    rp, ij = [x.cpu().numpy() for x in model.region_pair_min(verts, masked=True)]
    sig = raw['sig_d2'].cpu().numpy()
    assert rp.dtype == np.float32 and sig.dtype == np.float32
    touching = 0
    for p, (r1, r2) in enumerate(pair_idx):
        for b in range(2):
            if np.isinf(sig[b, r1, r2]):
                # (a pair of regions without any admissible vertex pair reports 0 and the vertices (-1, -1))
                assert rp[b, p] >= e32 * e32 or ij[b, p, 0] < 0, (b, p)
            else:
                assert rp[b, p].view(np.uint32) == sig[b, r1, r2].view(np.uint32), (b, p, rp[b, p], sig[b, r1, r2])
                touching += 1
    assert touching > 0


# ------------------------------------------------------------------------------------------------ 8
def test_deterministic_and_batch_independent():
    fx = vic()
    lists = region_variant(fx['regions'], 'r24', 1602)
    det = detector(fx, 0.05, lists)
    verts = torch.tensor(fx['verts'], device=DEV)
    first, second = det(verts), det(verts)
    for k in first:
        assert torch.equal(first[k], second[k]), k
    assert bool(first['in_contact'][3].any())
    alone = det(verts[3:4].contiguous())
    pair = det(torch.stack([verts[3], verts[5]]))
    last = det(torch.cat([verts[:3], verts[4:], verts[3:4]]))                         # body 3 as body 7 of 8
    for k in first:
        for what, got in (('alone', alone[k][0]), ('body 0 of 2', pair[k][0]), ('body 7 of 8', last[k][7])):
            assert torch.equal(got, first[k][3]), (k, what)


# ------------------------------------------------------------------------------------------------ 9
def test_graph_replay_bit_identical_to_eager():
    fx = vic()
    lists = region_variant(fx['regions'], 'r24', 1602)
    det = detector(fx, 0.05, lists)
    batches = [torch.tensor(fx['verts'][:4], device=DEV), torch.tensor(fx['verts'][4:], device=DEV)]
    eager = [{k: v.clone() for k, v in det(x).items()} for x in batches]
    static = batches[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                                         # warm-up off the capture
        det(static)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = det(static)
    for x, want in zip(batches[::-1], eager[::-1]):
        static.copy_(x)
        for v in out.values():
            v.zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(out[k], want[k]), k


# ------------------------------------------------------------------------------------------------ 10
def test_evaluator_records_cnc():
    from tuch_amd.eval import Evaluator, pose_summary
    fx = vic()
    det = detector(fx, 0.02)
    rng = np.random.default_rng(5)
    reg = rng.random((24, 1602)).astype(np.float32)
    reg /= reg.sum(1, keepdims=True)
    jmap = list(range(14))
    gt = torch.tensor(fx['verts'], device=DEV)
    pred = gt + torch.tensor(rng.normal(0, 0.01, fx['verts'].shape).astype(np.float32), device=DEV)
    ev = Evaluator(reg, jmap, capacity=16, contact=det)
    assert ev.add(pred[:3], gt_vertices=gt[:3]) == (0, 3)
    assert ev.add(pred[3:], gt_vertices=gt[3:]) == (3, 8)
    r = ev.results()
    direct = det(gt)['cnc'].cpu().numpy()
    assert np.array_equal(r['cnc'], direct)
    t = [truth(('vic', b, 0.02, None), fx['verts'][b], fx['mask'], 0.02) for b in range(8)]
    assert min(x['margin'] for x in t) > MARGIN
    cnc64 = np.sqrt(np.array([x['cnc_d2'] for x in t]))
    assert min(abs(c / 0.01 - 1.0) for c in cnc64) > 1e-5                             # nobody sits on the 10 mm line
    s = ev.summary(euclthres_lower=0.01)
    assert (s['n_contact'], s['n_no_contact'], s['n_unclear']) == (
        int((cnc64 < 0.01).sum()), int(np.isinf(cnc64).sum()), int(((cnc64 >= 0.01) & np.isfinite(cnc64)).sum()))
    assert s['n_no_contact'] == 1 and s['n_contact'] + s['n_unclear'] == 7
    np.testing.assert_equal(s, pose_summary(r['mpjpe'], r['pa_mpjpe'], direct, 0.01))      # (NaN means of empty subsets)
    # contact_vertices overrides gt_vertices; a batch with neither leaves NaN
    ev.reset()
    ev.add(pred[:2], gt_vertices=gt[:2], contact_vertices=gt[4:6])
    ev.add(pred[:2], gt_joints=torch.zeros(2, 14, 3, device=DEV))
    r2 = ev.results()['cnc']
    assert np.array_equal(r2[:2], direct[4:6]) and np.isnan(r2[2:]).all() and len(r2) == 4
    # without a detector nothing changes
    plain = Evaluator(reg, jmap, capacity=16)
    plain.add(pred, gt_vertices=gt)
    rp = plain.results()
    assert set(rp) == {'mpjpe', 'pa_mpjpe', 'v2v'}
    np.testing.assert_equal(plain.summary(), pose_summary(rp['mpjpe'], rp['pa_mpjpe']))
    assert set(plain.summary()) == {'mpjpe', 'recon_err'}
    assert np.array_equal(rp['mpjpe'], r['mpjpe']) and np.array_equal(rp['pa_mpjpe'], r['pa_mpjpe'])
    with pytest.raises(ValueError):
        plain.add(pred, gt_vertices=gt, contact_vertices=gt)
