"""GPU parity tests of the HIP contact kernels (through the C ABI) against the golden
vectors from the reference and against the CPU oracle.  Run with `-m gpu` on MI355X.

Tolerances (see DESIGN.md "Parity"):
  * winding numbers: 99 % of the vertices within 5e-6 absolute, 99.5 % within 1e-5, all within 2e-4
    (one ill-conditioned term can move a vertex by a few 1e-5 in the reference itself),
    exterior flags identical wherever |w - 0.99| > 1e-4;
  * squared distances taken by value: 1e-6 absolute (the reference's bmm form carries that
    much noise; ours are direct differences);
  * losses: 1e-4 relative (north_star), gradients 1e-4 relative + 1e-6 of the largest entry.
"""
import contextlib

import numpy as np
import pytest
import torch

import golden_io as gio
from helpers import (GRAD_RTOL, assert_close, golden, golden_mask, grad_close, hd_picks_vs_oracle, oracle_segments, report_value,
                     region_pair_lists, report, touches_surface)
from oracle import contact as oc

pytestmark = pytest.mark.gpu
SMALL = ['small', 'medium', 'ico_small', 'ico_medium']   # ico_*: irregular topology (valence 4-9, V % 64 != 0, painted segments)
FULL = ['full', 'full2', 'ico_full']                      # SMPL-sized; full2: B=2, a forearm THROUGH the trunk + an ignored body
TAGS = SMALL + FULL


def dev():
    return torch.device('cuda:0')


def make_model(g, gm, with_segments=True, with_regions=True):
    from tuch_amd.ops import ContactModel
    segs = gio.unpack_segments(g)
    seg_list = [(s['vidx'], list(s['bands'].values())) for s in segs.values()] if with_segments else None
    regions, pairs = gio.unpack_regions(g)
    names = list(regions.keys())
    pair_idx = np.asarray([[names.index(a), names.index(b)] for a, b in pairs], np.int64)
    return ContactModel(g['faces'], gm, seg_list, [regions[n] for n in names] if with_regions else None,
                        pair_idx if with_regions else None, device=dev())


WINDING_MAX_ERR = 1e-4      # 3 x the observed maximum (3.5e-5: tree walk, medium body 0; gpurun_out/parity_counts.txt)


def check_winding(w, w_ref, what=None):
    err = np.abs(w - w_ref)
    if what is not None:
        report_value('winding max |err| vs reference [%s]' % what, float(err.max()))
    assert np.percentile(err, 99) < 5e-6, np.percentile(err, 99)
    assert (err > 1e-5).mean() < 5e-3, (err > 1e-5).mean()
    assert err.max() < WINDING_MAX_ERR, err.max()
    clear = np.abs(w_ref - 0.99) > 1e-4
    assert np.array_equal((w <= 0.99)[clear], (w_ref <= 0.99)[clear])


@pytest.mark.parametrize('tag', TAGS)
def test_winding_numbers_vs_reference(tag):
    from tuch_amd import ops
    g = golden(tag)
    verts = torch.tensor(g['verts'], device=dev())
    faces = torch.tensor(g['faces'].astype(np.int32), device=dev())
    tris = ops.gather_triangles(verts, faces)
    assert np.array_equal(tris.cpu().numpy()[0], oc.gather_tris(g['verts'][0], g['faces']))
    w, ext = ops.winding_numbers(verts, tris, thresh=0.99)
    w = w.cpu().numpy()
    for b in range(w.shape[0]):
        check_winding(w[b], g['winding'][b], 'flat sum, %s body %d' % (tag, b))
    assert np.array_equal(ext.cpu().numpy(), w <= np.float32(0.99))


def test_solid_angles_and_pairwise_dense():
    from tuch_amd import ops
    g = golden('small')
    verts = torch.tensor(g['verts'][:1], device=dev())
    tris = ops.gather_triangles(verts, torch.tensor(g['faces'].astype(np.int32), device=dev()))
    sa = ops.solid_angles(verts, tris).cpu().numpy()[0]
    assert_close(sa, g['solid_angles_b0'], 1e-5, 1e-5, 'solid angles')
    p = ops.batch_pairwise_dist(verts, verts).cpu().numpy()[0]
    assert_close(p, g['pairwise_b0'], 0, 1e-6, 'pairwise')


def test_batch_pairwise_dist_gradient_vs_reference_autograd():
    """The reference differentiates through the materialised matrix (tuch/smplify/losses.py:76-78 -> 115-116,
    tuch/eft/loss.py:142).  Goldens: torch autograd through the reference's own function on the CPU
    (tests/golden/make_golden_pairwise_grad.py).  Tolerance: float32 sums of up to 130 terms of size <= 40, 2e-5 abs."""
    from tuch_amd.utils.contact import batch_pairwise_dist
    g = gio.load('pairwise_grad.npz')
    G = torch.tensor(g['G'], device=dev())
    for tag, squared in (('sq', True), ('root', False)):
        x = torch.tensor(g['x'], device=dev(), requires_grad=True)
        y = torch.tensor(g['y'], device=dev(), requires_grad=True)
        P = batch_pairwise_dist(x, y, squared=squared)
        assert P.requires_grad
        assert_close(P.detach().cpu().numpy(), g['P_' + tag], 1e-6, 2e-6, 'P ' + tag)
        (P * G).sum().backward()
        assert_close(x.grad.cpu().numpy(), g['gx_' + tag], 1e-5, 2e-5, 'grad x ' + tag)
        assert_close(y.grad.cpu().numpy(), g['gy_' + tag], 1e-5, 2e-5, 'grad y ' + tag)
        # only one side differentiated; bit-reproducible (fixed summation order)
        x2 = torch.tensor(g['x'], device=dev(), requires_grad=True)
        P2 = batch_pairwise_dist(x2, y.detach(), squared=squared)
        (P2 * G).sum().backward()
        assert torch.equal(x2.grad, x.grad)
    # one tensor as both arguments + block minima: the region-to-region term as the reference spells it (losses.py:112-116)
    v = torch.tensor(g['v'], device=dev(), requires_grad=True)
    P = batch_pairwise_dist(v[[0]], v[[0]], squared=True)
    loss = 0
    for r1, r2 in zip(g['blocks_a'], g['blocks_b']):
        r1, r2 = torch.as_tensor(r1, device=dev()), torch.as_tensor(r2, device=dev())
        loss = loss + torch.min(P[:, r1, :][:, :, r2])
    loss.backward()
    assert_close(loss.item(), g['r2r_loss'], 1e-5, 1e-6, 'r2r loss')
    assert_close(v.grad.cpu().numpy(), g['r2r_grad'], 1e-5, 2e-6, 'r2r grad')
    # many bodies, one region pair (train_module.py:83-88)
    xa = torch.tensor(g['xa'], device=dev(), requires_grad=True)
    ya = torch.tensor(g['ya'], device=dev(), requires_grad=True)
    d = batch_pairwise_dist(xa, ya)
    d.reshape(d.shape[0], -1).min(1)[0].sum().backward()
    assert_close(xa.grad.cpu().numpy(), g['gxa'], 1e-5, 2e-6, 'wide grad x')
    assert_close(ya.grad.cpu().numpy(), g['gya'], 1e-5, 2e-6, 'wide grad y')


def test_solid_angles_and_winding_numbers_gradient_vs_reference_autograd():
    """The reference's solid_angles / winding_numbers are plain differentiable torch ops (it calls them under no_grad itself);
    ours carry adjoint kernels.  Goldens: torch autograd through the reference's own functions on the CPU
    (tests/golden/make_golden_solid_angle_grad.py).  float32 sums of ~100 - 150 terms with entries up to 1e2: 1e-4 relative
    + 2e-4 of the largest entry."""
    from tuch_amd.utils.contact import solid_angles, winding_numbers
    g = gio.load('solid_angle_grad.npz')
    t = lambda k, grad=False: torch.tensor(g[k], device=dev(), requires_grad=grad)

    def close(a, want, what):
        want = np.asarray(want)
        assert_close(a.detach().cpu().numpy(), want, 1e-4, 2e-4 * float(np.abs(want).max()), what)
    p, tr = t('points', True), t('triangles', True)
    sa = solid_angles(p, tr)
    assert sa.requires_grad
    close(sa, g['solid_angles'], 'solid angles')
    (sa * t('G')).sum().backward()
    close(p.grad, g['sa_grad_points'], 'd solid_angles / d points')
    close(tr.grad, g['sa_grad_triangles'], 'd solid_angles / d triangles')
    p, tr = t('points', True), t('triangles', True)
    w = winding_numbers(p, tr)
    close(w, g['winding'], 'winding numbers')
    (w * t('gw')).sum().backward()
    close(p.grad, g['w_grad_points'], 'd winding / d points')
    close(tr.grad, g['w_grad_triangles'], 'd winding / d triangles')
    # only the points differentiated, a closed mesh, points inside and outside
    p2 = t('octa_points', True)
    w2 = winding_numbers(p2, t('octa'))
    close(w2, g['octa_winding'], 'octahedron winding')
    (w2 ** 2).sum().backward()
    # (off a CLOSED surface the winding number is constant: the exact gradient is zero, both sides return rounding noise)
    assert_close(p2.grad.cpu().numpy(), g['octa_grad_points'], 1e-4, 2e-5, 'd winding^2 / d points (octahedron)')
    # no graph recorded: nothing changes (every call site of the reference)
    with torch.no_grad():
        assert not winding_numbers(p2, t('octa')).requires_grad
    assert not solid_angles(p2.detach(), t('octa')).requires_grad


@pytest.mark.parametrize('tag', TAGS)
def test_v2v_min_masked_vs_reference(tag):
    g, gm = golden(tag), golden_mask(tag)
    model = make_model(g, gm, False, False)
    mn, arg = model.v2v_min(torch.tensor(g['verts'], device=dev()))
    mn, arg = mn.cpu().numpy(), arg.cpu().numpy().astype(np.int64)
    for b in range(mn.shape[0]):
        assert_close(mn[b], g['v2v_min'][b], 0, 1e-6, 'v2v min')
        same = arg[b] == g['v2v_argmin'][b]
        report('v2v argmin != reference [%s, body %d]' % (tag, b), int((~same).sum()), same.size)
        # index work is exact up to VERIFIED ties (below): observed 0 - 1 per body on every fixture, 0 at SMPL size
        assert (~same).sum() <= 2
        v = g['verts'][b].astype(np.float64)
        d_ours = ((v - v[arg[b]]) ** 2).sum(1)
        d_ref = ((v - v[g['v2v_argmin'][b]]) ** 2).sum(1)
        assert np.all(np.abs(d_ours - d_ref)[~same] < 2e-6)
        # exact property: our argmin attains the true (fp64) masked minimum up to fp32 rounding
        assert gm[arg[b], np.arange(len(arg[b]))].all()


def test_pack_geomask_matches_host_packing():
    from tuch_amd import ops
    gm = golden_mask('small')
    bits = ops.pack_geomask(torch.tensor(gm, device=dev())).cpu().numpy().view(np.uint64)
    v = gm.shape[0]
    for w in range(bits.shape[0]):
        for j in range(0, v, 17):
            word = int(bits[w, j])
            for k in range(64):
                i = 64 * w + k
                assert ((word >> k) & 1) == (int(gm[j, i]) if i < v else 0)


@pytest.mark.parametrize('tag', TAGS)
def test_exterior_flags_and_segments(tag):
    g, gm = golden(tag), golden_mask(tag)
    model = make_model(g, gm, True, False)
    verts = torch.tensor(g['verts'], device=dev())
    ext, w, seg_w, seg_e = model.exterior_flags(verts, apply_segments=True, return_details=True)
    ext_plain = model.exterior_flags(verts, apply_segments=False)
    ext, w, seg_e, ext_plain = ext.cpu().numpy().astype(bool), w.cpu().numpy(), seg_e.cpu().numpy(), \
        ext_plain.cpu().numpy().astype(bool)
    segs = oracle_segments(g)
    for b in range(ext.shape[0]):
        check_winding(w[b], g['winding'][b], 'tree walk, %s body %d' % (tag, b))
        assert np.array_equal(ext_plain[b], w[b] <= np.float32(0.99))
        want = g['segment_exterior'][b].astype(bool)
        report('segment flags != reference [%s, body %d]' % (tag, b), int((seg_e[b].astype(bool) != want).sum()), want.size)
        report('exterior flags (w <= 0.99) != reference [%s, body %d]' % (tag, b),
               int(((w[b] <= np.float32(0.99)) != (g['winding'][b] <= np.float32(0.99))).sum()), w[b].size)
        assert (seg_e[b].astype(bool) != want).sum() == 0          # flags are exact (observed: 0 on every fixture)
        expect = ext_plain[b].copy()
        off = 0
        for s in segs:
            expect[s.vidx[~seg_e[b][off:off + len(s.vidx)].astype(bool)]] = True
            off += len(s.vidx)
        assert np.array_equal(ext[b], expect)
        ext_ref, _ = oc.exterior_flags(g['verts'][b], g['faces'], segs, always_filter=True)
        assert (ext[b] != ext_ref).sum() == 0


@pytest.mark.parametrize('tag', SMALL)
@pytest.mark.parametrize('mode', [0, 1])
def test_contact_terms_forward_backward(tag, mode):
    from tuch_amd import ops
    g, gm = golden(tag), golden_mask(tag)
    eucl = float(g['euclthres'])
    verts = torch.tensor(g['verts'], device=dev(), requires_grad=True)
    b_count = verts.shape[0]
    partner = np.stack([oc.v2v_min_masked(g['verts'][b], gm)[1] for b in range(b_count)])
    ext = np.stack([oc.exterior_flags(g['verts'][b], g['faces'], None, False)[0] for b in range(b_count)])
    per_body, terms = ops.contact_terms(verts, torch.tensor(partner.astype(np.int32), device=dev()),
                                        torch.tensor(ext.astype(np.uint8), device=dev()), None, mode, eucl)
    weights = torch.tensor(np.linspace(1.0, 2.0, b_count), device=dev(), dtype=torch.float32)
    (per_body * weights).sum().backward()
    grad = verts.grad.cpu().numpy()
    for b in range(b_count):
        diff, d = oc._pair_distance(g['verts'][b], partner[b])
        if mode == 0:
            vin, dd_in = oc._tanh2_terms(d, ~ext[b], 1.0, 0.04)
            vex, dd_ex = oc._tanh2_terms(d, ext[b] & (d < np.float32(eucl)), 0.005, 0.005)
        else:
            vin, dd_in = oc._tanh2_terms(d, ~ext[b], 1.0, 0.04)
            vex, dd_ex = oc._tanh2_terms(d, ext[b], 0.005, 0.005)
        assert_close(terms[b, 0].item(), vin, 1e-5, 1e-7, 'interior sum')
        assert_close(terms[b, 1].item(), vex, 1e-5, 1e-7, 'exterior sum')
        gref = oc._scatter_pair_grad(diff, d, dd_in + dd_ex, partner[b], len(d)) * float(weights[b])
        assert_close(grad[b], gref, 1e-4, 1e-6 * max(np.abs(gref).max(), 1e-3), 'contact grad')


@pytest.mark.parametrize('tag', SMALL)
def test_region_pair_min(tag):
    g, gm = golden(tag), golden_mask(tag)
    model = make_model(g, gm, False, True)
    verts = torch.tensor(g['verts'], device=dev(), requires_grad=True)
    out, ij = model.region_pair_min(verts)                      # train_module.py:69-91
    assert_close(out.detach().cpu().numpy(), g['contact_from_verts'], 0, 1e-6, 'contact_from_verts')
    regions, pairs = gio.unpack_regions(g)
    ij_np = ij.cpu().numpy()
    for b in range(out.shape[0]):
        for k in range(0, len(pairs), 7):
            mn, i, j = oc.region_min_f64(g['verts'][b], regions[pairs[k][0]], regions[pairs[k][1]])
            assert abs(out[b, k].item() - mn) < 1e-7 + 1e-5 * mn
            v = g['verts'][b].astype(np.float64)
            assert abs(((v[ij_np[b, k, 0]] - v[ij_np[b, k, 1]]) ** 2).sum() - mn) < 1e-9
    # masked + selected variant (losses.py:107-117) with gradient
    sel = torch.tensor((g['gt_contact'] == 1) & g['has_discrete_contact'][:, None], device=dev())
    out_m, ij_m = model.region_pair_min(verts, select=sel, masked=True)
    out_m.sum().backward()
    grad = verts.grad.cpu().numpy()
    for b in range(out.shape[0]):
        rp = region_pair_lists(g, b) if g['has_discrete_contact'][b] else None
        r = oc.smplify_contact_body(g['verts'][b], g['faces'], gm, 0.0, None, rp)
        assert_close(out_m[b].sum().item(), r['r2r'], 1e-4, 1e-6, 'r2r')
        assert_close(grad[b], r['grad_r2r'], 1e-4, 1e-6, 'r2r grad')


@pytest.mark.parametrize('tag', ['medium', 'ico_medium'])
@pytest.mark.parametrize('masked', [True, False])
def test_region_pairs_selected_form_equals_the_all_pairs_form(tag, masked):
    """The few-pairs kernel (wavefronts find their share of a body's selected pairs in its row of `select`; tasks of 64
    rows x a quarter of the columns, merged with atomics) against the all-pairs kernel (one workgroup per pair): the
    same minima and the same (first) index pairs, bit for bit -- with more than 256 pairs (the select row is read 256
    bytes at a time), bodies with none, one, a few and ALL pairs selected."""
    from tuch_amd.ops import ContactModel
    g, gm = golden(tag), golden_mask(tag)
    regions, pairs = gio.unpack_regions(g)
    names = list(regions.keys())
    base = np.asarray([[names.index(a), names.index(b)] for a, b in pairs], np.int64)
    reps = -(-300 // len(base))
    pair_idx = np.concatenate([base, base[:, ::-1]] * reps)[:300]           # 300 pairs, both orders of every pair
    model = ContactModel(g['faces'], gm, None, [regions[n] for n in names], pair_idx, device=dev())
    verts = torch.tensor(np.concatenate([g['verts']] * 3)[:5], device=dev())
    B, P = verts.shape[0], len(pair_idx)
    rng = np.random.default_rng(5)
    sel = np.zeros((B, P), bool)
    sel[1, 299] = True
    sel[2, rng.choice(P, 7, replace=False)] = True
    sel[3] = True
    sel[4, rng.choice(P, 40, replace=False)] = True
    sel_t = torch.tensor(sel, device=dev())
    out_all, ij_all = model.region_pair_min(verts, masked=masked)
    out_sel, ij_sel = model.region_pair_min(verts, select=sel_t, masked=masked)
    out_all, ij_all, out_sel, ij_sel = (t.cpu().numpy() for t in (out_all, ij_all, out_sel, ij_sel))
    assert np.array_equal(out_sel[sel], out_all[sel])
    finite = sel & np.isfinite(out_all)
    assert np.array_equal(ij_sel[finite], ij_all[finite])
    assert np.all(out_sel[~sel] == 0) or np.all(~np.isfinite(out_sel[~sel]) | (out_sel[~sel] == 0))


def _fitting_inputs(g, full):
    from tuch_amd.smplify.prior import MaxMixturePrior
    d = dev()
    t = lambda a: torch.tensor(a, device=d)
    if full:
        prior = MaxMixturePrior(num_gaussians=8, gmm={k: g['gmm_' + k] for k in ('means', 'covars', 'weights')}).to(d)
        conf = t(g['joints_conf'])
    else:
        prior = lambda pose, betas: torch.zeros(pose.shape[0], device=d)
        conf = torch.zeros_like(t(g['joints_conf']))
    return t, prior, conf


@pytest.mark.parametrize('tag', SMALL)
@pytest.mark.parametrize('eu', ['e0', 'e2'])
@pytest.mark.parametrize('sg', ['nos', 'seg'])
@pytest.mark.parametrize('full', [False, True])
@pytest.mark.parametrize('fused_tail', ['1', '0'])
def test_contact_fitting_loss_vs_reference(tag, eu, sg, full, fused_tail, monkeypatch):
    """a6 of SURVEY.md §8a through the reference's own call signature (losses.py:34-123); with the prior of the full
    objective the part behind the body model runs as one autograd node (losses.FUSED_TAIL, default) or as separate ones."""
    if fused_tail == '0' and not full:
        pytest.skip('the switch only matters for the full objective')
    from tuch_amd.smplify import losses
    from tuch_amd.smplify.losses import contact_fitting_loss
    monkeypatch.setattr(losses, 'FUSED_TAIL', fused_tail == '1')
    from tuch_amd.utils.segmentation import BatchBodySegment
    g, gm = golden(tag), golden_mask(tag)
    t, prior, conf = _fitting_inputs(g, full)
    batch = g['verts'].shape[0]
    regions, pairs = gio.unpack_regions(g)
    cdict = {'classes': [list(p) for p in pairs], 'csig': regions}
    face_tensor = t(g['faces'])[None].repeat(batch, 1, 1)
    segs = gio.unpack_segments(g)
    segments = BatchBodySegment(list(segs.keys()), face_tensor[0], segs) if sg == 'seg' else None
    verts = t(g['verts']).requires_grad_(True)
    mj = t(g['model_joints']).requires_grad_(True)
    pose = t(g['body_pose']).requires_grad_(True)
    loss = contact_fitting_loss(
        pose, t(g['global_orient']), None, None, t(g['betas']), mj, t(gm),
        0.0 if eu == 'e0' else float(g['euclthres']), t(g['camera_t']), t(g['camera_center']),
        t(g['joints_2d']), conf, prior, cdict, [t(g['gt_contact']), None], t(g['ignore_idxs']),
        t(g['has_discrete_contact']), verts, face_tensor=face_tensor, focal_length=5000.,
        contact_loss_weight=float(g['contact_loss_weight']), segments=segments)
    loss.backward()
    key = 'smplify_%s_%s_%s' % (eu, sg, 'full' if full else 'contact')
    # the r2r term enters by value with weight 2000: its bmm-form reference value carries ~1e-6
    # absolute noise per selected pair (DESIGN.md "Parity")
    n_sel = float(((g['gt_contact'] == 1) & g['has_discrete_contact'][:, None]).sum())
    assert_close(loss.item(), g[key + '_loss'], 1e-4, 2000 * 1e-6 * n_sel, key)
    gv = g[key + '_grad_verts']
    grad_close(verts.grad.cpu().numpy(), gv, 2e-6, '%s %s grad verts' % (tag, key))
    if full:
        grad_close(mj.grad.cpu().numpy(), g[key + '_grad_joints'], 1e-5, '%s %s grad joints' % (tag, key))
        grad_close(pose.grad.cpu().numpy(), g[key + '_grad_pose'], 1e-5, '%s %s grad pose' % (tag, key))


@pytest.mark.parametrize('det', [True, False])
def test_stage2_tail_value_float_and_fixed_paths(det):
    """The three forms of the fused stage-2 tail (ops.objectives._Stage2Tail: value only, float atomics, fixed-point sums) on the
    full objective of `small` (V = 122: 16 points per block, eight blocks per body; region pairs, segments, real prior
    and confidences).  No golden of SMALL lists an ignored body, so the bit-for-bit properties are checked twice: with
    the golden's ignore_idxs and with body 1 ignored; the comparison with the golden uses its own ignore_idxs."""
    from tuch_amd import ops
    from tuch_amd.smplify.losses import contact_fitting_loss
    from tuch_amd.utils.segmentation import BatchBodySegment
    tag, key = 'small', 'smplify_e2_seg_full'
    g, gm = golden(tag), golden_mask(tag)
    t, prior, conf = _fitting_inputs(g, True)
    batch = g['verts'].shape[0]
    regions, pairs = gio.unpack_regions(g)
    assert len(pairs) > 0 and ((g['gt_contact'] == 1) & g['has_discrete_contact'][:, None]).any()
    cdict = {'classes': [list(p) for p in pairs], 'csig': regions}
    face_tensor = t(g['faces'])[None].repeat(batch, 1, 1)
    segs = gio.unpack_segments(g)
    segments = BatchBodySegment(list(segs.keys()), face_tensor[0], segs)
    geomask = t(gm)
    fixed_inputs = [t(g[k]) for k in ('global_orient', 'betas', 'camera_t', 'camera_center', 'joints_2d', 'gt_contact',
                                      'has_discrete_contact')]
    go, betas, cam_t, cam_c, j2d, gt, hdc = fixed_inputs

    def call(ignore, grads):
        verts, mj, pose = (t(g[k]).requires_grad_(True) for k in ('verts', 'model_joints', 'body_pose'))
        with contextlib.nullcontext() if grads else torch.no_grad():
            loss = contact_fitting_loss(
                pose, go, None, None, betas, mj, geomask, float(g['euclthres']), cam_t, cam_c, j2d, conf, prior, cdict,
                [gt, None], ignore, hdc, verts, face_tensor=face_tensor, focal_length=5000.,
                contact_loss_weight=float(g['contact_loss_weight']), segments=segments)
        assert loss.requires_grad == grads
        if grads:
            loss.backward()
        return loss.detach(), verts.grad, mj.grad, pose.grad

    ignored_1 = torch.zeros(batch, dtype=torch.bool, device=dev())
    ignored_1[1] = True
    with ops.deterministic_mode(det):
        for ignore in (t(g['ignore_idxs']), ignored_1):
            value = call(ignore, False)[0]
            loss, gv, gj, gp = call(ignore, True)
            # fixed-order sums: the value does not depend on whether the scatter runs
            assert torch.equal(value, loss), (value.item(), loss.item())
            if det:
                again = call(ignore, True)[1]
                assert gv.abs().max() > 0 and torch.equal(gv, again)
        if not det:     # (the last pass of the loop was body 1 ignored: the golden's own ignore_idxs again)
            loss, gv, gj, gp = call(t(g['ignore_idxs']), True)
            n_sel = float(((g['gt_contact'] == 1) & g['has_discrete_contact'][:, None]).sum())
            assert_close(loss.item(), g[key + '_loss'], 1e-4, 2000 * 1e-6 * n_sel, key)
            grad_close(gv.cpu().numpy(), g[key + '_grad_verts'], 2e-6, '%s %s float atomics grad verts' % (tag, key))
            grad_close(gj.cpu().numpy(), g[key + '_grad_joints'], 1e-5, '%s %s float atomics grad joints' % (tag, key))
            grad_close(gp.cpu().numpy(), g[key + '_grad_pose'], 1e-5, '%s %s float atomics grad pose' % (tag, key))


def _full_train(tag='full'):
    data = gio.load('contact_%s_train.npz' % tag)
    return {k: data[k] for k in data.files}


@pytest.mark.parametrize('tag', FULL)
@pytest.mark.parametrize('eu', ['e0', 'e2'])
def test_contact_fitting_loss_vs_reference_fullsize(eu, tag):
    """a6 at SMPL size (V=6890, F=13776; ico_full: V=6762 irregular): the reference's contact_fitting_loss with segments
    and three annotated region pairs per body (tests/golden/make_golden.py:fullsize_case) -- loss and gradient.  full2:
    body 0 has a forearm pushed through the trunk, body 1 is listed in ignore_idxs (losses.py:74)."""
    from tuch_amd.smplify.losses import contact_fitting_loss
    from tuch_amd.utils.segmentation import BatchBodySegment
    g, gm = golden(tag), golden_mask(tag)
    d = dev()
    t = lambda a: torch.tensor(a, device=d)
    n = g['verts'].shape[0]
    ignore = g['ignore_idxs'] if 'ignore_idxs' in g else np.zeros(n, bool)
    regions, pairs = gio.unpack_regions(g)
    cdict = {'classes': [list(p) for p in pairs], 'csig': regions}
    face_tensor = t(g['faces'])[None]
    segs = gio.unpack_segments(g)
    segments = BatchBodySegment(list(segs.keys()), face_tensor[0], segs)
    verts = t(g['verts']).requires_grad_(True)
    zero_prior = lambda pose, betas: torch.zeros(pose.shape[0], device=d)
    loss = contact_fitting_loss(
        torch.zeros(n, 69, device=d), torch.zeros(n, 3, device=d), None, None, torch.zeros(n, 10, device=d),
        torch.ones(n, 49, 3, device=d), t(gm), 0.0 if eu == 'e0' else float(g['euclthres']),
        torch.tensor([[0., 0., 20.]], device=d).repeat(n, 1), torch.zeros(n, 2, device=d), torch.zeros(n, 49, 2, device=d),
        torch.zeros(n, 49, device=d), zero_prior, cdict, [t(g['gt_contact']), None],
        t(ignore), torch.ones(n, dtype=torch.bool, device=d), verts,
        face_tensor=face_tensor, contact_loss_weight=float(g['contact_loss_weight']), segments=segments)
    loss.backward()
    key = 'smplify_%s_seg_contact' % eu
    n_sel = float((g['gt_contact'][~ignore] == 1).sum())
    assert_close(loss.item(), g[key + '_loss'], 1e-4, 2000 * 1e-6 * n_sel, key)
    gv = g[key + '_grad_verts']
    assert np.all(gv[ignore] == 0) and np.all(verts.grad.cpu().numpy()[ignore] == 0)
    grad_close(verts.grad.cpu().numpy(), gv, 2e-6, '%s %s grad verts' % (tag, key))


@pytest.mark.parametrize('tag', FULL)
@pytest.mark.parametrize('use_hd', [False, True])
def test_regressor_contact_loss_vs_reference_fullsize(use_hd, tag):
    """a7 at SMPL size with all N_hd = 3 F (41 328) HD points: the configuration bench.py times."""
    import types
    from tuch_amd.train.loss import RegressorLoss
    from tuch_amd.utils.segmentation import BatchBodySegment
    g, gm, gt = golden(tag), golden_mask(tag), _full_train(tag)
    d = dev()
    face_tensor = torch.tensor(g['faces'], device=d)[None]
    segs = gio.unpack_segments(g)
    segments = BatchBodySegment(list(segs.keys()), face_tensor[0], segs)
    geod = torch.tensor(np.where(gm, 1.0, 0.0).astype(np.float32), device=d)
    crit = RegressorLoss(types.SimpleNamespace(contact_loss_weight=1.0), d, g['verts'].shape[1], face_tensor,
                         geod, geothres=0.3, euclthres=float(g['euclthres']), face_tensor=face_tensor,
                         use_hd=use_hd, segments=segments, hd_regressor=(g['hd_idx'], g['hd_w']),
                         hd_faces=g['hd_face'])
    assert not use_hd or crit.hd_idx.shape[0] == 3 * g['faces'].shape[0]
    verts = torch.tensor(g['verts'], device=d, requires_grad=True)
    loss = crit.contact_loss(verts, torch.ones(verts.shape[0], dtype=torch.bool, device=d))
    loss.backward()
    key = 'train_hd' if use_hd else 'train_plain'
    assert_close(loss.item(), gt[key + '_loss'], 1e-4, 0, key)
    want = gt[key + '_grad_verts'].astype(np.float64).copy()
    if use_hd:
        # the reference picks an HD point's partner by its bmm-form squared distance (~1e-6 of noise: percent-level at
        # contact distances, DESIGN.md "Parity"); where the device picks another candidate tied within that noise, the
        # expected gradient is the reference's plus the oracle's difference between the two picks
        n_b = verts.shape[0]
        for b in range(n_b):
            r, r2 = hd_picks_vs_oracle(crit._hd, crit._hd.last_saved, n_b, b, g['verts'][b], g['faces'], gm, float(g['euclthres']),
                                       oracle_segments(g), g['hd_idx'], g['hd_w'], g['hd_face'], '%s body %d' % (tag, b))
            want[b] += (r2['grad'] - r['grad']) / n_b
    grad_close(verts.grad.cpu().numpy(), want, 5e-6, '%s %s grad' % (tag, key), quantum=use_hd)


@pytest.mark.parametrize('tag', FULL)
def test_eft_contact_loss_vs_reference_fullsize(tag):
    import types
    from tuch_amd.eft.loss import EFTLoss
    from tuch_amd.utils.segmentation import BatchBodySegment
    g, gm, gt = golden(tag), golden_mask(tag), _full_train(tag)
    d = dev()
    face_tensor = torch.tensor(g['faces'], device=d)[None]
    segs = gio.unpack_segments(g)
    regions, pairs = gio.unpack_regions(g)
    crit = EFTLoss(types.SimpleNamespace(batch_size=1, img_res=224), d, None, g['verts'].shape[1], None,
                   torch.tensor(np.where(gm, 1.0, 0.0).astype(np.float32), device=d), 0.3, face_tensor=face_tensor,
                   cdict={'classes': [list(p) for p in pairs], 'csig': regions},
                   segments=BatchBodySegment(list(segs.keys()), face_tensor[0], segs))
    for b in range(g['verts'].shape[0]):           # the reference's EFT loss is a batch-1 call (eft/loss.py:150)
        verts = torch.tensor(g['verts'][b:b + 1], device=d, requires_grad=True)
        loss = crit.contact_loss(torch.tensor(g['gt_contact'][b:b + 1], device=d), verts)
        loss.backward()
        n_sel = float((g['gt_contact'][b] == 1).sum())
        assert_close(loss.item(), gt['eft_loss'][b], 1e-4, 50 * 1e-6 * n_sel, 'eft loss')
        grad_close(verts.grad.cpu().numpy()[0], gt['eft_grad_verts'][b], 5e-6, '%s eft grad body %d' % (tag, b))


def test_batch_pairwise_dist_batched_regions():
    """a1 as contact_from_verts calls it (train_module.py:83-88): full batch, two different region subsets."""
    from tuch_amd import ops
    g = golden('medium')
    regions, pairs = gio.unpack_regions(g)
    verts = torch.tensor(g['verts'], device=dev())
    for k in (0, len(pairs) // 2, len(pairs) - 1):
        r1, r2 = regions[pairs[k][0]], regions[pairs[k][1]]
        x, y = verts[:, torch.as_tensor(r1, device=dev())], verts[:, torch.as_tensor(r2, device=dev())]
        p = ops.batch_pairwise_dist(x.contiguous(), y.contiguous()).cpu().numpy()
        assert p.shape == (verts.shape[0], len(r1), len(r2))
        for b in range(verts.shape[0]):
            assert_close(p[b], oc.pairwise_sq(g['verts'][b][r1], g['verts'][b][r2]), 0, 1e-6, 'pairwise block')
        assert_close(p.reshape(p.shape[0], -1).min(1), g['contact_from_verts'][:, k], 0, 1e-6, 'block minimum')


@pytest.mark.parametrize('tag', TAGS)
def test_triangle_strips_cover_every_face_once(tag):
    g = golden(tag)
    model = make_model(g, None, False, False)
    vidx, sign, nstrips = model.strips()
    faces = g['faces']
    emitted = {}
    for p in range(len(vidx)):
        if sign[p] == 0:
            continue
        tri = (int(vidx[p - 2]), int(vidx[p - 1]), int(vidx[p]))
        key = tuple(sorted(tri))
        assert key not in emitted
        emitted[key] = (tri, sign[p])
    assert len(emitted) == len(faces)
    for f in faces:
        tri, sg = emitted[tuple(sorted(int(x) for x in f))]
        rots = [tuple(int(x) for x in np.roll(f, k)) for k in range(3)]
        assert (tri in rots) == (sg > 0)
    assert (sign[:2] == 0).all() and nstrips >= 1
    print(tag, 'faces', len(faces), 'stream', len(vidx), 'strips', nstrips)


@pytest.mark.parametrize('tag', SMALL)
@pytest.mark.parametrize('use_hd', [False, True])
def test_regressor_contact_loss_vs_reference(tag, use_hd):
    """a7 of SURVEY.md §8a: RegressorLoss.contact_loss (loss.py:240-317), both branches."""
    import types
    from tuch_amd.train.loss import RegressorLoss
    from tuch_amd.utils.segmentation import BatchBodySegment
    g, gm = golden(tag), golden_mask(tag)
    d = dev()
    batch = g['verts'].shape[0]
    face_tensor = torch.tensor(g['faces'], device=d)[None].repeat(batch, 1, 1)
    segs = gio.unpack_segments(g)
    segments = BatchBodySegment(list(segs.keys()), face_tensor[0], segs)
    geod = torch.tensor(np.where(gm, 1.0, 0.0).astype(np.float32), device=d)     # geod > 0.3 <=> mask
    crit = RegressorLoss(types.SimpleNamespace(contact_loss_weight=1.0), d, g['verts'].shape[1], face_tensor,
                         geod, geothres=0.3, euclthres=float(g['euclthres']), face_tensor=face_tensor,
                         use_hd=use_hd, segments=segments, hd_regressor=(g['hd_idx'], g['hd_w']),
                         hd_faces=g['hd_face'])
    verts = torch.tensor(g['verts'], device=d, requires_grad=True)
    loss = crit.contact_loss(verts, torch.tensor(g['valid_fit'], device=d))
    loss.backward()
    key = 'train_hd' if use_hd else 'train_plain'
    assert_close(loss.item(), g[key + '_loss'], 1e-4, 0, key)
    gv = g[key + '_grad_verts']
    grad_close(verts.grad.cpu().numpy(), gv, 5e-6, '%s %s grad' % (tag, key), quantum=use_hd)


@pytest.mark.parametrize('tag', SMALL)
def test_regressor_contact_loss_hd_asymmetric_mask(tag):
    """A geodesic mask is symmetric, but nothing in loss.py:288-291 needs it to be: with pairs dropped one way only,
    row and column of geomask[vid_row][vid_col] must not be mixed up anywhere in the HD branch -- same loss and gradient
    as the restated reference on that mask."""
    import types
    from tuch_amd.train.loss import RegressorLoss
    from tuch_amd.utils.segmentation import BatchBodySegment
    g, gm = golden(tag), golden_mask(tag)
    rng = np.random.default_rng(5)
    asym = gm & (rng.random(gm.shape) < 0.6)
    assert (asym != asym.T).any()
    d = dev()
    batch = g['verts'].shape[0]
    face_tensor = torch.tensor(g['faces'], device=d)[None].repeat(batch, 1, 1)
    segs = gio.unpack_segments(g)
    segments = BatchBodySegment(list(segs.keys()), face_tensor[0], segs)
    geod = torch.tensor(np.where(asym, 1.0, 0.0).astype(np.float32), device=d)
    crit = RegressorLoss(types.SimpleNamespace(contact_loss_weight=1.0), d, g['verts'].shape[1], face_tensor,
                         geod, geothres=0.3, euclthres=float(g['euclthres']), face_tensor=face_tensor,
                         use_hd=True, segments=segments, hd_regressor=(g['hd_idx'], g['hd_w']), hd_faces=g['hd_face'])
    verts = torch.tensor(g['verts'], device=d, requires_grad=True)
    loss = crit.contact_loss(verts, torch.tensor(g['valid_fit'], device=d))
    loss.backward()
    ref_loss, ref_grad, _ = oc.train_contact_loss(g['verts'], g['valid_fit'], g['faces'], asym, float(g['euclthres']),
                                                  oracle_segments(g), True, hd_idx=g['hd_idx'], hd_w=g['hd_w'],
                                                  hd_face=g['hd_face'])
    assert_close(loss.item(), ref_loss, 1e-4, 0, 'hd loss, asymmetric mask')
    grad_close(verts.grad.cpu().numpy(), ref_grad, 5e-6, tag + ' hd grad, asymmetric mask', quantum=True)


def test_contact_from_verts_class():
    from tuch_amd.train.train_module import TUCH
    g = golden('medium')
    regions, pairs = gio.unpack_regions(g)
    t = TUCH(contactlists={'classes': [list(p) for p in pairs], 'csig': regions}, faces=g['faces'], device=dev())
    out = t.contact_from_verts(torch.tensor(g['verts'], device=dev()))
    assert_close(out.cpu().numpy(), g['contact_from_verts'], 0, 1e-6, 'contact_from_verts')


@pytest.mark.parametrize('tag', SMALL)
def test_eft_contact_loss_vs_reference(tag):
    """EFTLoss.contact_loss (tuch/eft/loss.py:129-181) on the kernels, whole batch at once."""
    import types
    from tuch_amd.eft.loss import EFTLoss
    from tuch_amd.utils.segmentation import BatchBodySegment
    g, gm = golden(tag), golden_mask(tag)
    d = dev()
    batch = g['verts'].shape[0]
    face_tensor = torch.tensor(g['faces'], device=d)[None].repeat(batch, 1, 1)
    segs = gio.unpack_segments(g)
    regions, pairs = gio.unpack_regions(g)
    crit = EFTLoss(types.SimpleNamespace(batch_size=batch, img_res=224), d, None, g['verts'].shape[1], None,
                   torch.tensor(np.where(gm, 1.0, 0.0).astype(np.float32), device=d), 0.3, face_tensor=face_tensor,
                   cdict={'classes': [list(p) for p in pairs], 'csig': regions},
                   segments=BatchBodySegment(list(segs.keys()), face_tensor[0], segs))
    verts = torch.tensor(g['verts'], device=d, requires_grad=True)
    loss = crit.contact_loss(torch.tensor(g['gt_contact'], device=d), verts)
    loss.backward()
    n_sel = float((g['gt_contact'] == 1).sum())
    assert_close(loss.item(), g['eft_loss'].sum(), 1e-4, 50 * 1e-6 * n_sel, 'eft loss')
    gv = g['eft_grad_verts']
    grad_close(verts.grad.cpu().numpy(), gv, 5e-6, tag + ' eft grad')


@pytest.mark.parametrize('tag', TAGS)
def test_winding_points_ragged_vs_oracle(tag):
    """tuch_winding_points: arbitrary query points against the posed mesh (strip kernel), with a
    ragged count per body; checked against the CPU oracle."""
    g = golden(tag)
    model = make_model(g, None, False, False)
    verts_np = g['verts']
    b_count, v_count = verts_np.shape[:2]
    rng = np.random.default_rng(3)
    q = min(300, v_count)
    # points just off the surface (vertex + small random offset) and a few far away
    pts = np.stack([verts_np[b][rng.choice(v_count, q, replace=False)] for b in range(b_count)])
    pts = (pts + 0.003 * rng.standard_normal(pts.shape)).astype(np.float32)
    pts[:, :5] += 3.0
    counts = np.array([q - 7 * b for b in range(b_count)], np.int32)
    w, ext = model.winding_points(torch.tensor(verts_np, device=dev()), torch.tensor(pts, device=dev()),
                                  torch.tensor(counts, device=dev()))
    w, ext = w.cpu().numpy(), ext.cpu().numpy()
    for b in range(b_count):
        wo = oc.winding_numbers(pts[b][:counts[b]], oc.gather_tris(verts_np[b], g['faces']))
        err = np.abs(w[b][:counts[b]] - wo)
        # points inside several layers have w = 2, 3: float32 accumulation noise scales with |w|
        assert np.percentile(err / np.maximum(1.0, np.abs(wo)), 99) < 5e-6 and err.max() < 2e-4
        clear = np.abs(wo - 0.99) > 1e-4
        assert np.array_equal(ext[b][:counts[b]][clear].astype(bool), (wo <= 0.99)[clear])


def test_contact_terms_ragged_matches_dense():
    from tuch_amd import ops
    g, gm = golden('medium'), golden_mask('medium')
    verts_np = g['verts']
    b_count, v_count = verts_np.shape[:2]
    partner = np.stack([oc.v2v_min_masked(verts_np[b], gm)[1] for b in range(b_count)]).astype(np.int32)
    ext = (np.arange(b_count * v_count).reshape(b_count, v_count) % 3 != 0).astype(np.uint8)
    d = dev()
    vd = torch.tensor(verts_np, device=d, requires_grad=True)
    dense = ops.contact_terms(vd, torch.tensor(partner, device=d), torch.tensor(ext, device=d), None, 1, 0.02)[1]
    (dense * torch.tensor([[1.0, 2.0]], device=d)).sum().backward()
    flat = torch.tensor(verts_np.reshape(-1, 3), device=d, requires_grad=True)
    off = torch.arange(b_count + 1, dtype=torch.int32, device=d) * v_count
    gpart = torch.tensor((partner + np.arange(b_count)[:, None] * v_count).reshape(-1).astype(np.int32), device=d)
    body_of = torch.arange(b_count, dtype=torch.int32, device=d).repeat_interleave(v_count).contiguous()
    ragged = ops.contact_terms_ragged(flat, gpart, torch.tensor(ext.reshape(-1), device=d), off, body_of, 1, 0.02)
    (ragged * torch.tensor([[1.0, 2.0]], device=d)).sum().backward()
    assert_close(ragged.detach().cpu().numpy(), dense.detach().cpu().numpy(), 1e-6, 1e-7, 'ragged terms')
    assert_close(flat.grad.cpu().numpy().reshape(b_count, v_count, 3), vd.grad.cpu().numpy(), 1e-5, 1e-7, 'ragged grad')


def _flags_and_winding(model, verts, tree, monkeypatch):
    model.set_option('winding_tree', int(tree))
    ext, w = model.exterior_flags(verts, apply_segments=False, return_details=True)[:2]
    return ext.cpu().numpy().astype(bool), w.cpu().numpy()


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('batch', [1, 3, 9])
def test_tree_walk_matches_flat_walk(tag, batch, monkeypatch):
    """The hierarchical evaluation (cluster tree + boundary caps) against the flat walk over every
    face, both on the device, and both against the reference's output."""
    g = golden(tag)
    model = make_model(g, None, False, False)
    base = torch.tensor(g['verts'], device=dev())
    verts = base[torch.arange(batch, device=dev()) % base.shape[0]].contiguous()
    if batch > base.shape[0]:        # perturb the repeats: shear + offset keeps the surface closed
        k = (torch.arange(batch, device=dev(), dtype=torch.float32) - (base.shape[0] - 1)).clamp(min=0).view(-1, 1)
        verts[:, :, 0] += 0.03 * k * verts[:, :, 1]
        verts[:, :, 2] += 0.1 * k
    ext_t, w_t = _flags_and_winding(model, verts, True, monkeypatch)
    ext_f, w_f = _flags_and_winding(model, verts, False, monkeypatch)
    for b in range(batch):
        check_winding(w_t[b], w_f[b])
        if b < base.shape[0]:
            check_winding(w_t[b], g['winding'][b])
    clear = np.abs(w_f - 0.99) > 1e-4
    assert np.array_equal(ext_t[clear], ext_f[clear])


def test_open_mesh_keeps_the_flat_walk():
    """A mesh with a hole has no cluster tree (the cap identity needs a closed surface); the model
    still answers, through the flat walk, and agrees with the oracle."""
    g = golden('small')
    from tuch_amd.ops import ContactModel
    faces = g['faces'][:-3]
    model = ContactModel(faces, None, None, None, None, device=dev())
    verts = torch.tensor(g['verts'], device=dev())
    w = model.exterior_flags(verts, apply_segments=False, return_details=True)[1].cpu().numpy()
    for b in range(verts.shape[0]):
        ref = oc.winding_numbers(g['verts'][b], g['verts'][b][faces])
        assert np.abs(w[b] - ref).max() < 2e-5


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('batch', [1, 5])
def test_v2v_tree_walk_matches_flat_search(tag, batch, monkeypatch):
    """The pruned nearest-vertex search (cluster tree, box distances, static mask table) against the flat
    all-rows kernel: identical minima bit for bit; the partner may differ only between exactly tied rows."""
    g, gm = golden(tag), golden_mask(tag)
    model = make_model(g, gm, False, False)
    base = torch.tensor(g['verts'], device=dev())
    verts = base[torch.arange(batch, device=dev()) % base.shape[0]].contiguous()
    k = (torch.arange(batch, device=dev(), dtype=torch.float32) - (base.shape[0] - 1)).clamp(min=0).view(-1, 1)
    verts[:, :, 0] += 0.05 * k * verts[:, :, 1]
    model.set_option('v2v_tree', 0)
    mn_f, arg_f = model.v2v_min(verts)
    model.set_option('v2v_tree', 1)
    # the search: lanes over the subtree's leaves first (v2v_scan_kernel).  (Other forms -- a stackless walk, leaf boxes
    # four at a time, aligned row tiles on the matrix cores -- gave the same keys and were slower; removed, DESIGN.md
    # section 3 keeps their measurements.)
    # pairs (round 5): a leaf in reach of fewer columns of a wavefront than this is not walked row by row; its
    # (leaf, column) pairs are queued and evaluated one per lane -- 0: off (round 4's scan), 24: the default, 33: nearly all
    for waves, pairs in (('1', 24), ('4096', 24), ('1000000', 24), ('1', 0), ('4096', 0), ('4096', 4), ('4096', 33), ('1', 33)):
        model.set_option('v2v_waves', int(waves))        # one subtree ... as many as the model has
        model.set_option('v2v_pairs', pairs)
        mn_t, arg_t = model.v2v_min(verts)
        assert torch.equal(mn_t, mn_f)
        diff = (arg_t != arg_f).nonzero()
        v = verts.double()
        for b, i in diff.tolist():
            d_t = ((v[b, i] - v[b, arg_t[b, i]]) ** 2).sum()
            d_f = ((v[b, i] - v[b, arg_f[b, i]]) ** 2).sum()
            assert abs(float(d_t - d_f)) < 1e-9 and gm[int(arg_t[b, i]), i]
        assert len(diff) <= 2
    # repeatable despite the atomics
    mn_again, arg_again = model.v2v_min(verts)
    assert torch.equal(mn_again, mn_t) and torch.equal(arg_again, arg_t)
    model.set_option('v2v_waves', 0)
    model.set_option('v2v_pairs', 24)


@pytest.mark.parametrize('tag', ['small', 'ico_small'])
@pytest.mark.parametrize('batch', [1, 5])
def test_v2v_heads_under_guard_words(tag, batch):
    """Both heads of the tree search -- rows and seed in one launch from the previous call's partners (v2v_hint = 1), two
    launches with the seed from the leaf boxes (v2v_hint = 0) -- alone and beside other work (leave_room), with guard words
    between the regions of the workspace: minima bit for bit those of the all-rows kernel, partners differing only between
    exactly tied rows, no guard word touched."""
    g, gm = golden(tag), golden_mask(tag)
    model = make_model(g, gm, False, False)
    base = torch.tensor(g['verts'], device=dev())
    verts = base[torch.arange(batch, device=dev()) % base.shape[0]].contiguous()
    k = (torch.arange(batch, device=dev(), dtype=torch.float32) - (base.shape[0] - 1)).clamp(min=0).view(-1, 1)
    verts[:, :, 0] += 0.05 * k * verts[:, :, 1]
    model.set_option('canary', 1)
    model.set_option('v2v_tree', 0)
    mn_f, arg_f = model.v2v_min(verts)
    model.set_option('v2v_tree', 1)
    v = verts.double()
    for hint in (0, 1):
        model.set_option('v2v_hint', hint)
        for leave_room in (False, True):
            for _ in range(2):          # (with hints the second call starts from the first one's partners)
                mn_t, arg_t = model.v2v_min(verts, leave_room=leave_room)
                assert torch.equal(mn_t, mn_f)
                diff = (arg_t != arg_f).nonzero()
                for b, i in diff.tolist():
                    d_t = ((v[b, i] - v[b, arg_t[b, i]]) ** 2).sum()
                    d_f = ((v[b, i] - v[b, arg_f[b, i]]) ** 2).sum()
                    assert abs(float(d_t - d_f)) < 1e-9 and gm[int(arg_t[b, i]), i]
                assert len(diff) <= 2
            assert model.canary_hits() == 0, (hint, leave_room)
    assert model.canary_selftest() > 0          # (a silent mechanism cannot pass)


@pytest.mark.parametrize('tag', ['medium', 'ico_medium'])
def test_v2v_asymmetric_mask_takes_the_scan_without_lane_pairs(tag):
    """The lane pairs read a column's admissible rows of a leaf from THAT column's row of the bit matrix: valid for a
    symmetric mask only (a geodesic mask is).  A mask with pairs dropped one way only must fall back to the round-4 scan
    (checked when the model is made) and still give the flat all-rows search's minima and partners; masking by the
    reference's rule is P[:, ~mask] = inf with mask[row j, column i]."""
    g, gm = golden(tag), golden_mask(tag).copy()
    rng = np.random.default_rng(3)
    drop = rng.random(gm.shape) < 0.3
    gm[np.triu(drop, 1)] = False                      # rows j < columns i lose pairs; the mirrored entries stay
    assert not np.array_equal(gm, gm.T)
    model = make_model(g, gm, False, False)
    verts = torch.tensor(g['verts'], device=dev())
    model.set_option('v2v_tree', 0)
    mn_f, arg_f = model.v2v_min(verts)
    model.set_option('v2v_tree', 1)
    for pairs in (24, 0):
        model.set_option('v2v_pairs', pairs)
        mn_t, arg_t = model.v2v_min(verts)
        assert torch.equal(mn_t, mn_f)
        assert int((arg_t != arg_f).sum()) <= 2
    v = g['verts'][0].astype(np.float64)
    d = ((v[:, None, :] - v[None, :, :]) ** 2).sum(2)
    d[~gm] = np.inf
    fin = np.isfinite(d.min(0))
    got = mn_f[0].cpu().numpy()
    assert np.array_equal(np.isfinite(got), fin) and np.allclose(got[fin], d.min(0)[fin], rtol=2e-6, atol=1e-9)


@pytest.mark.parametrize('tag', ['medium', 'ico_medium', 'full', 'ico_full'])
def test_winding_points_tree_matches_flat(tag, monkeypatch):
    """tuch_winding_points through the cluster tree (queries in the caller's order) against the flat strips."""
    g = golden(tag)
    model = make_model(g, None, False, False)
    verts_np = g['verts']
    rng = np.random.default_rng(11)
    b_count, v_count = verts_np.shape[:2]
    q = 700
    # points on / near the surface in random order (incoherent blocks: slow but exact) and sorted by vertex id
    idx = np.stack([rng.choice(v_count, q, replace=True) for _ in range(b_count)])
    for order in ('random', 'sorted'):
        ids = np.sort(idx, axis=1) if order == 'sorted' else idx
        pts = np.stack([verts_np[b][ids[b]] for b in range(b_count)]) + 0.002 * rng.standard_normal((b_count, q, 3))
        pts = torch.tensor(pts.astype(np.float32), device=dev())
        counts = torch.tensor([q - 37 * b for b in range(b_count)], dtype=torch.int32, device=dev())
        verts = torch.tensor(verts_np, device=dev())
        res = {}
        for tree in ('0', '1'):
            model.set_option('winding_tree', int(tree))
            w, ext = model.winding_points(verts, pts, counts)
            res[tree] = (w.cpu().numpy(), ext.cpu().numpy())
        for b in range(b_count):
            n = int(counts[b])
            err = np.abs(res['1'][0][b][:n] - res['0'][0][b][:n])
            assert np.percentile(err / np.maximum(1.0, np.abs(res['0'][0][b][:n])), 99) < 5e-6 and err.max() < 2e-4
            clear = np.abs(res['0'][0][b][:n] - 0.99) > 1e-4
            assert np.array_equal(res['1'][1][b][:n][clear], res['0'][1][b][:n][clear])
            assert (res['1'][0][b][n:] == 0).all() and (res['1'][1][b][n:] == 1).all()      # padding: w = 0, exterior


def test_exterior_and_partner_matches_the_separate_calls(monkeypatch):
    """The two-stream form used by the loss functions returns exactly what the two calls return."""
    g, gm = golden('medium'), golden_mask('medium')
    model = make_model(g, gm, True, True)
    verts = torch.tensor(g['verts'], device=dev())
    ext = model.exterior_flags(verts, apply_segments=True)
    mn, arg = model.v2v_min(verts)
    for overlap in ('1', '0'):
        model.set_option('overlap', int(overlap))
        e2, mn2, arg2, extra = model.exterior_and_partner(verts, apply_segments=True,
                                                          also=lambda: model.region_pair_min(verts, masked=True))
        torch.cuda.synchronize()
        assert torch.equal(e2, ext) and torch.equal(mn2, mn) and torch.equal(arg2, arg)
        r2r, _ = model.region_pair_min(verts, masked=True)
        assert torch.equal(extra[0], r2r)


@pytest.mark.parametrize('order', ['sorted', 'shuffled'])
def test_v2v_min_indexed_matches_brute_force(order):
    """tuch_v2v_min_indexed (ragged point sets, chunk pruning) against a float64 brute force: the minimum is
    the true masked minimum, the argmin is the first row attaining the float32 minimum."""
    g, gm = golden('medium'), golden_mask('medium')
    model = make_model(g, gm, False, False)
    rng = np.random.default_rng(4)
    v = g['verts'].shape[1]
    counts = [900, 0, 317, 64, 1]
    pts, vids = [], []
    for b, n in enumerate(counts):
        base = rng.choice(v, n, replace=True)
        if order == 'sorted':
            base = np.sort(base)
        pts.append(g['verts'][b % g['verts'].shape[0]][base] + 0.004 * rng.standard_normal((n, 3)))
        vids.append(base)
    pts = np.concatenate(pts).astype(np.float32)
    vids = np.concatenate(vids).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    mn, arg = model.v2v_min_indexed(torch.tensor(pts, device=dev()), torch.tensor(vids, device=dev()),
                                    torch.tensor(offsets, device=dev()), max(counts))
    # the same search with ids given as positions in the model's own tree order (and the mask packed in that order)
    pos = model.tree_positions()
    assert pos is not None and np.array_equal(np.sort(pos), np.arange(v))
    mn_t, arg_t = model.v2v_min_indexed(torch.tensor(pts, device=dev()), torch.tensor(pos[vids], device=dev()),
                                        torch.tensor(offsets, device=dev()), max(counts), tree_order=True)
    assert torch.equal(mn_t, mn) and torch.equal(arg_t, arg)
    mn, arg = mn.cpu().numpy(), arg.cpu().numpy()
    for b, n in enumerate(counts):
        lo = offsets[b]
        p, vid = pts[lo:lo + n], vids[lo:lo + n]
        if n == 0:
            continue
        d = ((p[:, None].astype(np.float32) - p[None].astype(np.float32)) ** 2)
        d32 = (d[..., 2] + (d[..., 1] + d[..., 0])).astype(np.float32)        # same association as the kernel, no fma
        allowed = gm[vid[None, :], vid[:, None]]                              # [column a, row r] = geomask[vid[r]][vid[a]]
        d64 = ((p[:, None].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(2)
        d64 = np.where(allowed, d64, np.inf)
        want = d64.min(1)
        got = mn[lo:lo + n]
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin)
        np.testing.assert_allclose(got[fin], want[fin], rtol=2e-6, atol=1e-9)
        a = arg[lo:lo + n]
        assert (a[~fin] == 0).all()
        # the returned row attains the minimum and is admissible; no earlier row does strictly better
        rows = np.arange(n)
        assert allowed[rows[fin], a[fin]].all()
        np.testing.assert_allclose(d64[rows[fin], a[fin]], want[fin], rtol=2e-6, atol=1e-9)


@pytest.mark.parametrize('tag,order', [('medium', 'patch'), ('medium', 'shuffled'), ('full', 'patch')])
def test_v2v_min_indexed_mfma_vs_exact(tag, order):
    """The matrix-core form of the ragged search (hd_search.hip, what the HD branch runs) against the exact kernel:
    every winner is admissible, its reported distance is its direct-difference distance, and that distance exceeds the
    exact float32 minimum by no more than the key's rounding (1e-6 relative) + a few ulp of the column block's squared
    radius -- 2e-8 for points sorted by surface patch (the HD branch keeps them so), 4e-6 for any order.  Columns
    without an admissible row report (inf, 0).  Two runs agree bit for bit."""
    g, gm = golden(tag), golden_mask(tag)
    model = make_model(g, gm, False, False)
    rng = np.random.default_rng(11)
    v = g['verts'].shape[1]
    pos = model.tree_positions()
    counts = [2900, 0, 317, 64, 1, 33, 1000] if tag == 'medium' else [6100, 97, 4000]
    pts, vids = [], []
    for b, n in enumerate(counts):
        base = rng.choice(v, n, replace=True)
        if order == 'patch':
            base = base[np.argsort(pos[base], kind='stable')]
        pts.append(g['verts'][b % g['verts'].shape[0]][base] + 0.004 * rng.standard_normal((n, 3)))
        vids.append(base)
    pts = np.concatenate(pts).astype(np.float32)
    vids = np.concatenate(vids).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    args = (torch.tensor(pts, device=dev()), torch.tensor(vids, device=dev()), torch.tensor(offsets, device=dev()), max(counts))
    mn0, arg0 = model.v2v_min_indexed(*args)
    mn1, arg1 = model.v2v_min_indexed(*args, mfma=True)
    mn2, arg2 = model.v2v_min_indexed(*args, mfma=True)
    assert torch.equal(mn1, mn2) and torch.equal(arg1, arg2)
    mn0, arg0, mn1, arg1 = (t.cpu().numpy() for t in (mn0, arg0, mn1, arg1))
    fin = np.isfinite(mn0)
    assert np.array_equal(np.isfinite(mn1), fin)
    assert (arg1[~fin] == 0).all()
    worst, differ = 0.0, 0
    for b, n in enumerate(counts):
        lo = offsets[b]
        if n == 0:
            continue
        f = fin[lo:lo + n]
        a1 = arg1[lo:lo + n].astype(np.int64)
        assert ((a1 >= 0) & (a1 < n)).all()
        if not f.any():
            continue
        p, vid = pts[lo:lo + n], vids[lo:lo + n]
        cols = np.arange(n)[f]
        assert gm[vid[a1[f]], vid[cols]].all()                         # geomask[vid[row]][vid[column]]
        d = p[cols] - p[a1[f]]
        direct = (d[:, 2] * d[:, 2] + (d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0])).astype(np.float32)
        np.testing.assert_allclose(mn1[lo:lo + n][f], direct, rtol=3e-7, atol=0)
        excess = mn1[lo:lo + n][f].astype(np.float64) - mn0[lo:lo + n][f]
        assert (excess >= -1e-12).all()
        tol = 2e-6 * mn0[lo:lo + n][f] + (2e-8 if order == 'patch' else 4e-6)
        assert (excess <= tol).all(), (b, excess.max())
        worst = max(worst, float(excess.max()))
        differ += int((a1[f] != arg0[lo:lo + n][f]).sum())
    report('v2v_min_indexed_mfma %s/%s: winners != exact kernel (ties within the key rounding), worst excess %.2e' %
           (tag, order, worst), differ, int(fin.sum()))


def test_winding_tree_work_counts():
    """The measurement aid behind bench.py's roofline: element steps walked by the tree, far below the flat walk."""
    g = golden('full')
    model = make_model(g, None, False, False)
    verts = torch.tensor(g['verts'], device=dev())
    w = model.winding_tree_work(verts)
    steps = w['leaf_elements'] + w['cap_elements']
    flat = w['query_blocks'] * w['flat_stream_elements']
    assert w['leaf_elements'] > 0 and w['cap_elements'] > 0 and w['queries_per_step'] == 64
    assert 0.05 < steps / flat < 0.5
    assert w == model.winding_tree_work(verts)           # counts are deterministic


def test_v2v_hints_never_change_the_result(monkeypatch):
    """The partner hints kept between calls only seed the pruning: whatever the buffer holds (garbage included),
    minima and partners are those of a call without hints."""
    g, gm = golden('medium'), golden_mask('medium')
    model = make_model(g, gm, False, False)
    verts = torch.tensor(g['verts'], device=dev())
    model.set_option('v2v_hint', 0)
    mn0, arg0 = model.v2v_min(verts)
    model.set_option('v2v_hint', 1)
    mn1, arg1 = model.v2v_min(verts)                       # zero-initialised hints
    mn2, arg2 = model.v2v_min(verts)                       # hints = the partners just found
    buf = model._v2v_hint(verts.shape[0])
    assert buf is not None
    junk = torch.randint(-5, 3 * verts.shape[1], (buf.numel() // 4,), dtype=torch.int32, device=dev())
    buf.view(torch.int32).copy_(junk)
    mn3, arg3 = model.v2v_min(verts)                       # garbage, out-of-range and inadmissible rows included
    moved = verts + 0.01 * torch.randn_like(verts)
    model.set_option('v2v_hint', 0)
    mn4, arg4 = model.v2v_min(moved)
    model.set_option('v2v_hint', 1)
    mn5, arg5 = model.v2v_min(moved)                       # hints from the other pose
    for mn, arg in ((mn1, arg1), (mn2, arg2), (mn3, arg3)):
        assert torch.equal(mn, mn0) and torch.equal(arg, arg0)
    assert torch.equal(mn5, mn4) and torch.equal(arg5, arg4)


@pytest.mark.parametrize('tag', ['full', 'ico_full'])
def test_v2v_fresh_bodies_foreign_hints_and_no_hints_agree_bit_for_bit_fullsize(tag):
    """A training loop never sees the same bodies twice (tuch/train/train_module.py:302-317 -> tuch/train/loss.py:240-317):
    at SMPL size, batches of DIFFERENT bodies in turn -- every call seeded by the previous batch's partners (a foreign
    hint) --, the same with the hint buffer cleared, filled with garbage, holding the call's own answer, and with hints
    switched off give identical minima and partners, bit for bit; and every one of them is the fp64 brute-force masked
    minimum of a sampled body up to float32 rounding."""
    g, gm = golden(tag), golden_mask(tag)
    model = make_model(g, gm, False, False)
    batch = 5
    batches = []
    for k in range(3):
        _, v = _posed_batch(tag, batch, seed=100 + k, scale=1.0 + 0.5 * k)
        if k:       # other bodies, not the fixture's first ones again
            v = v.flip(0).contiguous() * (1.0 + 0.03 * k)
        batches.append(v)
    model.set_option('v2v_hint', 0)
    want = [tuple(t.clone() for t in model.v2v_min(v)) for v in batches]
    model.set_option('v2v_hint', 1)
    buf = model._v2v_hint(batch)
    assert buf is not None
    order = [0, 1, 2, 1, 1, 0, 2, 0]             # foreign, foreign, foreign, foreign, OWN answer, foreign, ...
    for n, i in enumerate(order):
        # (iterative: the caller's word that its hints are near-final -- fewer, longer wavefronts; a wrong word costs time only)
        mn, arg = model.v2v_min(batches[i], iterative=bool(n & 1), leave_room=bool(n & 2))
        assert torch.equal(mn, want[i][0]) and torch.equal(arg, want[i][1]), 'hinted call differs (batch %d)' % i
    for fill in ('zero', 'junk', 'minus one'):
        if fill == 'zero':
            buf.zero_()
        elif fill == 'junk':
            buf.view(torch.int32).copy_(torch.randint(-7, 2 * g['verts'].shape[1], (buf.numel() // 4,), dtype=torch.int32,
                                                      device=dev()))
        else:
            buf.view(torch.int32).fill_(-1)
        mn, arg = model.v2v_min(batches[1])
        assert torch.equal(mn, want[1][0]) and torch.equal(arg, want[1][1]), 'hint buffer = %s changes the result' % fill
    # ... and they are the masked minimum: fp64 brute force on one body of a batch the fixture does not hold
    v = batches[2][1].cpu().numpy().astype(np.float64)
    d = ((v[:, None, :] - v[None, :, :]) ** 2).sum(2)
    d[~gm] = np.inf
    got_mn, got_arg = want[2][0][1].cpu().numpy(), want[2][1][1].cpu().numpy().astype(np.int64)
    fin = np.isfinite(d.min(0))
    assert np.array_equal(np.isfinite(got_mn), fin)
    assert gm[got_arg[fin], np.flatnonzero(fin)].all()
    assert np.allclose(got_mn[fin], d.min(0)[fin], rtol=2e-6, atol=1e-9)
    assert np.allclose(d[got_arg[fin], np.flatnonzero(fin)], d.min(0)[fin], rtol=2e-6, atol=1e-9)


# ---- inside test by ray crossings (csrc/ray_winding.hip) against the solid-angle sums ------------------------------
def _posed_batch(tag, batch, seed, scale=1.0):
    """`batch` bodies of the fixture's mesh in new poses: the golden ones followed by sheared / squeezed copies
    (affine maps keep the surface closed; squeezing x makes limbs interpenetrate)."""
    g = golden(tag)
    base = torch.tensor(g['verts'], device=dev())
    verts = base[torch.arange(batch, device=dev()) % base.shape[0]].clone()
    rng = np.random.default_rng(seed)
    for b in range(base.shape[0], batch):
        a = torch.tensor(np.eye(3) + 0.25 * scale * rng.standard_normal((3, 3)), dtype=torch.float32, device=dev())
        verts[b] = verts[b] @ a.T + torch.tensor(rng.standard_normal(3), dtype=torch.float32, device=dev())
    return g, verts.contiguous()


@pytest.mark.parametrize('tag', TAGS)
@pytest.mark.parametrize('batch', [1, 7])
def test_ray_crossing_flags_match_the_solid_angle_sums(tag, batch, monkeypatch):
    """Vertices: w = crossings - fan angles (TUCH_WINDING_RAY=2 reports it) against the summed solid angles of the
    tree walk and of the reference; flags identical wherever w is not within 1e-4 of the threshold."""
    g, verts = _posed_batch(tag, batch, 5)
    model = make_model(g, None, False, False)
    model.set_option('winding_ray', 0)
    ext_s, w_s = model.exterior_flags(verts, apply_segments=False, return_details=True)[:2]
    model.set_option('winding_ray', 2)
    ext_r, w_r = model.exterior_flags(verts, apply_segments=False, return_details=True)[:2]
    model.set_option('winding_ray', 1)
    ext_1 = model.exterior_flags(verts, apply_segments=False)
    w_s, w_r = w_s.cpu().numpy(), w_r.cpu().numpy()
    ext_s, ext_r, ext_1 = ext_s.cpu().numpy(), ext_r.cpu().numpy(), ext_1.cpu().numpy()
    assert np.array_equal(ext_r, ext_1)
    err = np.abs(w_r - w_s)
    # a vertex that TOUCHES another triangle (LBS folds the synthetic skin flat between the legs) sits on a jump of
    # the winding number: either side is legitimate, for the reference's own float32 sum too
    jump = np.argwhere(err > 0.5)
    report('ray vs solid-angle w: vertices on a jump (touching a triangle) [%s, B=%d]' % (tag, batch), len(jump), w_s.size)
    assert len(jump) <= 2 * batch
    for b, v in jump:
        assert touches_surface(verts[b].cpu().numpy(), g['faces'], int(v)), (b, v, w_r[b, v], w_s[b, v])
        err[b, v] = 0.0
        w_r[b, v], ext_r[b, v] = w_s[b, v], ext_s[b, v]
    report('ray vs solid-angle w: max |dw| [%s, B=%d] x1e7' % (tag, batch), int(err.max() * 1e7), w_s.size)
    assert err.max() < 2e-4, err.max()             # 2e-4 = the bound of check_winding
    clear = np.abs(w_s - 0.99) > 1e-4
    assert np.array_equal(ext_r[clear], ext_s[clear])
    report('ray flags != solid-angle flags [%s, B=%d]' % (tag, batch), int((ext_r != ext_s).sum()), ext_s.size)
    for b in range(min(batch, g['verts'].shape[0])):
        check_winding(w_r[b], g['winding'][b])


@pytest.mark.parametrize('tag,batch', [('medium', 130), ('ico_medium', 130), ('full', 70), ('ico_full', 70), ('small', 300)])
def test_big_batches_ray_crossings_match_the_solid_angle_sums(tag, batch):
    """Batch sizes that are not multiples of 8 (XCD columns of the crossing kernel) and need more than one pass of the
    grids: flags by ray crossings against flags from the solid-angle sums, with and without the segment filter;
    a mismatching vertex must touch another triangle (it sits on a jump of the winding number)."""
    g, verts = _posed_batch(tag, batch, 5)
    model = make_model(g, golden_mask(tag), True, False)
    model.set_option('winding_ray', 0)
    e0, w0 = model.exterior_flags(verts, apply_segments=False, return_details=True)[:2]
    es0 = model.exterior_flags(verts, apply_segments=True)
    model.set_option('winding_ray', 2)
    e1, w1 = model.exterior_flags(verts, apply_segments=False, return_details=True)[:2]
    model.set_option('winding_ray', 1)
    e2 = model.exterior_flags(verts, apply_segments=False)
    es1 = model.exterior_flags(verts, apply_segments=True)
    assert torch.equal(e1, e2)
    bad = torch.nonzero(e0 != e1).cpu().numpy()
    report('big batch [%s, B=%d]: ray flags != solid-angle flags (must touch a triangle)' % (tag, batch), len(bad), e0.numel())
    assert len(bad) <= 8
    vnp = verts.cpu().numpy()
    for b, vid in bad:
        assert touches_surface(vnp[b], g['faces'], int(vid)), (b, vid)
    dw = (w0 - w1).abs()
    jumps = torch.nonzero((dw > 0.5) & (e0 == e1)).cpu().numpy()     # on a jump, but both sides of it give the same flag
    for b, vid in jumps:
        assert touches_surface(vnp[b], g['faces'], int(vid)), (b, vid)
    rest = dw[(e0 == e1) & (dw <= 0.5)]
    report('big batch [%s, B=%d]: max |dw| off the jumps x1e7' % (tag, batch), int(float(rest.max()) * 1e7), rest.numel())
    assert float(torch.quantile(rest.flatten()[::3].float(), 0.999)) < 5e-5 and float(rest.max()) < 1e-3 and len(jumps) <= 8
    seg_bad = torch.nonzero(es0 != es1).cpu().numpy()
    report('big batch [%s, B=%d]: flags after the segment filter differ' % (tag, batch), len(seg_bad), es0.numel())
    body_bad = {(int(b), int(vid)) for b, vid in bad}
    for b, vid in seg_bad:            # only where the body test already differed, or a segment vertex on a jump
        assert (int(b), int(vid)) in body_bad or touches_surface(vnp[b], g['faces'], int(vid)), (b, vid)
    assert len(seg_bad) <= 8


@pytest.mark.parametrize('tag', ['small', 'ico_medium', 'full', 'full2', 'ico_full'])
@pytest.mark.parametrize('cap', [1, 2])
def test_pair_list_overflow_falls_back_to_block_major_order(tag, cap):
    """ray_tiles_kernel switches a body whose (ray, leaf) pairs do not fit the pair list (option ray_pair_cap pairs per
    query, default 16) to block-major order, walked by the same crossing kernel (ray_winding.hip: ray_tiles_kernel /
    ray_leaf_kernel).  With room for 1 or 2 pairs per query EVERY body overflows: flags, with and without the segment
    filter and for off-surface points, must be those of the default capacity."""
    batch = 5 if tag in ('full', 'full2', 'ico_full') else 9
    g, verts = _posed_batch(tag, batch, 23)
    model = make_model(g, None, True, False)
    ext_d = model.exterior_flags(verts, apply_segments=False)
    exts_d = model.exterior_flags(verts, apply_segments=True)
    work_d = model.ray_work(verts)
    rng = np.random.default_rng(3)
    q = min(500, verts.shape[1])
    ids = np.stack([np.sort(rng.choice(verts.shape[1], q, replace=False)) for _ in range(batch)])
    pts = torch.stack([verts[b][torch.tensor(ids[b], device=dev())] for b in range(batch)]) \
        + 0.004 * torch.tensor(rng.standard_normal((batch, q, 3)).astype(np.float32), device=dev())
    _, pext_d = model.winding_points(verts, pts.contiguous(), flags_only=True)
    model.set_option('ray_pair_cap', cap)
    assert model.get_option('ray_pair_cap') == cap
    ext_c = model.exterior_flags(verts, apply_segments=False)
    exts_c = model.exterior_flags(verts, apply_segments=True)
    work_c = model.ray_work(verts)
    _, pext_c = model.winding_points(verts, pts.contiguous(), flags_only=True)
    assert torch.equal(ext_c, ext_d) and torch.equal(exts_c, exts_d) and torch.equal(pext_c, pext_d)
    assert (~ext_d.bool()).sum() > 0
    # block-major order walks more elements for the same answer: proof that the other path ran
    report('pair cap %d [%s]: element steps block-major vs leaf-major' % (cap, tag), work_c['elements'], work_d['elements'])
    assert work_c['elements'] > work_d['elements']


@pytest.mark.parametrize('tag', TAGS)
def test_fused_segment_filter_matches_the_six_launch_pass(tag):
    """The segment filter behind the body test as ONE launch (segment_one_kernel, option seg_fused = 1: eight workgroups
    per (segment, body), each finishing a share of the interior vertices) against the general six-launch pass
    (seg_fused = 0): identical flags, on the fixtures and on sheared / squeezed copies with many interior vertices, at a
    batch that is not a multiple of anything."""
    batch = 6 if tag in FULL else 11
    g, verts = _posed_batch(tag, batch, 31, scale=1.3)
    model = make_model(g, None, True, False)
    assert model.get_option('seg_fused') == 1 and model.get_option('seg_fused_active') == 1
    plain = model.exterior_flags(verts, apply_segments=False)
    one = model.exterior_flags(verts, apply_segments=True)
    model.set_option('seg_fused', 0)
    six = model.exterior_flags(verts, apply_segments=True)
    model.set_option('seg_fused', 1)
    again = model.exterior_flags(verts, apply_segments=True)
    assert torch.equal(one, six) and torch.equal(again, one)
    changed = int((one != plain).sum())
    report('fused segment filter [%s]: vertices re-marked exterior by the filter' % tag, changed, plain.numel())
    assert int((plain == 0).sum()) > 0


@pytest.mark.parametrize('tag', ['medium', 'ico_medium'])
def test_fan_direction_tangent_to_a_star_face(tag):
    """w of a vertex by ray crossings = crossings of (mesh - star + closing fan) - the fan's angles / 4 pi.  When the fan's
    apex direction lies in the plane of one of the star's faces (with the opposite direction inside the face), that cone
    triangle is flat: its crossing flips by one and its solid angle jumps by 2 pi there -- the two must be signed by the
    SAME determinant, or w is off by exactly one (csrc/ray_winding.hip: cone_term).  Bodies rotated so that a chosen
    vertex sits exactly in that configuration, up to rotations of ~1e-7 rad either way."""
    g = golden(tag)
    model = make_model(g, None, False, False)
    base = g['verts'][0].astype(np.float64)
    faces = g['faces']
    u = np.array([0.8191, 0.3467, 0.4571])                       # kFanX/Y/Z of ray_winding.hip
    u /= np.linalg.norm(u)
    rng = np.random.default_rng(12)

    def rot(axis, angle):
        axis = axis / np.linalg.norm(axis)
        k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * k @ k
    bodies, targets = [], []
    for f in rng.choice(len(faces), 40, replace=False):
        v, a, b = faces[f]
        mid = (base[a] - base[v]) / np.linalg.norm(base[a] - base[v]) + (base[b] - base[v]) / np.linalg.norm(base[b] - base[v])
        mid /= np.linalg.norm(mid)
        # rotate the bisector of the face's corner at v onto -u: u then lies in the face's plane, -u inside the face
        axis = np.cross(mid, -u)
        r0 = rot(axis, np.arctan2(np.linalg.norm(axis), mid @ -u)) if np.linalg.norm(axis) > 1e-9 else np.eye(3)
        r0 = rot(u, rng.uniform(0, 2 * np.pi)) @ r0
        for eps in (0.0, 1e-7, -1e-7, 3e-7, -3e-7, 1e-6):
            r = rot(rng.standard_normal(3), eps) @ r0
            bodies.append((base - base[v]) @ r.T + base[v])
            targets.append(v)
    verts = torch.tensor(np.stack(bodies).astype(np.float32), device=dev())
    model.set_option('winding_ray', 0)
    w_s = model.exterior_flags(verts, apply_segments=False, return_details=True)[1]
    model.set_option('winding_ray', 2)
    w_r = model.exterior_flags(verts, apply_segments=False, return_details=True)[1]
    idx = torch.tensor(targets, device=dev())
    rows = torch.arange(len(targets), device=dev())
    err_t = (w_r[rows, idx] - w_s[rows, idx]).abs()
    report('fan tangent to a star face [%s]: targeted vertices with |dw| > 0.5' % tag, int((err_t > 0.5).sum()), len(targets))
    assert float(err_t.max()) < 1e-3
    err = (w_r - w_s).abs()
    assert int((err > 0.5).sum()) == 0 and float(err.max()) < 1e-3


@pytest.mark.parametrize('tag', TAGS)
def test_segment_filter_by_ray_crossings_matches_the_solid_angle_sums(tag, monkeypatch):
    """The segment test (segmentation.py:81-99) by ray crossings: w of EVERY segment vertex w.r.t. its "closed" segment
    = crossings + cone terms of the closing chain (links of the vertex's star - the boundary of the segment mesh; the
    synthetic caps leave boundary edges on the arm segments, so the chain is not just a ring) against the summed solid
    angles; flags identical wherever w is not within 1e-4 of the threshold, body flags after the filter identical."""
    g, verts = _posed_batch(tag, 4, 11)
    model = make_model(g, None, True, False)
    model.set_option('winding_ray', 0)
    ext_s, _, segw_s, sege_s = model.exterior_flags(verts, apply_segments=True, return_details=True)
    model.set_option('winding_ray', 2)
    ext_r, _, segw_r, sege_r = model.exterior_flags(verts, apply_segments=True, return_details=True)
    model.set_option('winding_ray', 1)
    ext_1 = model.exterior_flags(verts, apply_segments=True)
    segw_s, segw_r = segw_s.cpu().numpy(), segw_r.cpu().numpy()
    err = np.abs(segw_r - segw_s)
    jump = err > 0.5                       # a vertex touching another triangle of its segment: either side is legitimate
    report('segment w, ray vs solid angle: vertices on a jump [%s]' % tag, int(jump.sum()), err.size)
    assert jump.sum() <= 4
    report('segment w, ray vs solid angle: max |dw| [%s] x1e7' % tag, int(err[~jump].max() * 1e7), err.size)
    # sheared / squeezed copies of a self-penetrating body put vertices microns from foreign triangles, where the float32
    # solid-angle sum loses digits: nearly all agree to 2e-5, the worst to 1e-3 (the crossing count is exact there)
    assert np.percentile(err[~jump], 99.9) < 5e-5 and err[~jump].max() < 1e-3
    clear = (np.abs(segw_s - 0.99) > 1e-4) & ~jump
    assert np.array_equal(sege_r.cpu().numpy()[clear], sege_s.cpu().numpy()[clear])
    if not jump.any():
        assert torch.equal(ext_r, ext_s) and torch.equal(ext_1, ext_s)
    if tag != 'ico_small':                                 # (its one segment, 16 head vertices, is never entered)
        assert len(np.unique(np.round(segw_s))) >= 2      # vertices inside their own segment do occur
    # the default model takes the crossings with the segments' body faces from the body's own inside test; a model
    # built with TUCH_SEG_ASSIST=0 walks every face of the segment in the segment pass: same answers
    monkeypatch.setenv('TUCH_SEG_ASSIST', '0')      # read when the model is created, fixed afterwards
    plain = make_model(g, None, True, False)
    plain.set_option('winding_ray', 2)
    assert plain.get_option('seg_assist') == 0 and model.get_option('seg_assist') == 1
    ext_p, _, segw_p, sege_p = plain.exterior_flags(verts, apply_segments=True, return_details=True)
    assert torch.equal(sege_p, sege_r) and torch.equal(ext_p, ext_r)
    assert float((segw_p - torch.tensor(segw_r, device=segw_p.device)).abs().max()) < 2e-6


def test_ray_crossing_flags_at_rest_pose_and_axis_aligned():
    """Degenerate input: the symmetric template itself, unposed and axis aligned (many exactly equal coordinates,
    rays through edges and vertices: the tie rules decide) and a mirrored copy (orientation reversed: w = -...)."""
    from synthetic import make_body
    body = make_body(40, 40)
    from tuch_amd.ops import ContactModel
    model = ContactModel(body.faces, None, None, None, None, device=dev())
    v = torch.tensor(body.v_template, device=dev())[None]
    # the shear of the ray frame is fixed in space: also test the template rotated so that rays run along mesh symmetry
    verts = torch.cat([v, v[:, :, [2, 0, 1]], v * torch.tensor([1.0, 1.0, 0.5], device=dev())]).contiguous()
    model.set_option('winding_ray', 0)
    ext_s, w_s = model.exterior_flags(verts, apply_segments=False, return_details=True)[:2]
    model.set_option('winding_ray', 2)
    ext_r, w_r = model.exterior_flags(verts, apply_segments=False, return_details=True)[:2]
    assert float((w_r - w_s).abs().max()) < 2e-4
    assert torch.equal(ext_r, ext_s)


@pytest.mark.parametrize('tag', ['medium', 'ico_medium', 'full', 'ico_full'])
def test_ray_crossing_flags_of_points_match_the_solid_angle_sums(tag, monkeypatch):
    """Off-surface points (HD points of loss.py:297: on a face, 1 mm along its normal; plus points well inside and
    outside): integer crossing counts against the summed solid angles, ragged counts, both point orders."""
    g, verts = _posed_batch(tag, 5, 9, scale=0.6)
    model = make_model(g, None, False, False)
    rng = np.random.default_rng(2)
    faces = torch.tensor(g['faces'], device=dev())
    q = 900
    fid = torch.tensor(rng.integers(0, faces.shape[0], (5, q)), device=dev())
    bary = torch.tensor(rng.dirichlet([1, 1, 1], (5, q)).astype(np.float32), device=dev())
    tri = torch.stack([verts[b][faces[fid[b]]] for b in range(5)])                 # [5,q,3,3]
    on = (tri * bary[..., None]).sum(2)
    n = torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=2)
    n = n / n.norm(dim=2, keepdim=True)
    sign = torch.tensor(rng.choice([1.0, -1.0, 20.0, -20.0], (5, q, 1)).astype(np.float32), device=dev())
    pts = (on + 0.001 * sign * n).contiguous()                                     # 1 mm / 2 cm above / below
    counts = torch.tensor([q, q - 100, 1, 0, 517], dtype=torch.int32, device=dev())
    model.set_option('winding_ray', 0)
    w_s, ext_s = model.winding_points(verts, pts, counts)
    model.set_option('winding_ray', 1)
    _, ext_r = model.winding_points(verts, pts, counts, flags_only=True)
    model.set_option('winding_ray', 2)
    w_r, ext_2 = model.winding_points(verts, pts, counts)
    w_s, w_r = w_s.cpu().numpy(), w_r.cpu().numpy()
    assert torch.equal(ext_r, ext_2)
    assert np.array_equal(w_r, np.round(w_r))                                      # integers
    report('ray vs solid-angle w of points: max |dw| [%s] x1e6' % tag, int(np.abs(w_r - w_s).max() * 1e6), w_s.size)
    assert np.abs(w_r - w_s).max() < 1e-3
    assert torch.equal(ext_r, ext_s)
    assert len(np.unique(w_r)) >= 2                                                # inside and outside points both occur


@pytest.mark.parametrize('use_hd', [True, False])
def test_hd_gradient_is_bit_reproducible_in_deterministic_mode(use_hd):
    """Deterministic mode (the default; ops.set_deterministic): the HD branch's point gradients are summed as 64-bit fixed-point integers (LDS integer
    atomics) and gathered per vertex in a fixed order -- the gradient of contact_loss(use_hd=True) is the same BITS every
    time, and agrees with the float-atomic one to float tolerance.  use_hd=False: the plain training term's scatter
    (contact_terms_bwd_kernel<Fixed>, round 4) likewise."""
    import types
    from tuch_amd import ops
    from tuch_amd.train.loss import RegressorLoss
    from tuch_amd.utils.segmentation import BatchBodySegment
    g, gm = golden('medium'), golden_mask('medium')
    d = dev()
    batch = g['verts'].shape[0]
    face_tensor = torch.tensor(g['faces'], device=d)[None].repeat(batch, 1, 1)
    segs = gio.unpack_segments(g)
    crit = RegressorLoss(types.SimpleNamespace(contact_loss_weight=1.0), d, g['verts'].shape[1], face_tensor,
                         torch.tensor(np.where(gm, 1.0, 0.0).astype(np.float32), device=d), geothres=0.3,
                         euclthres=float(g['euclthres']), face_tensor=face_tensor, use_hd=use_hd,
                         segments=BatchBodySegment(list(segs.keys()), face_tensor[0], segs),
                         hd_regressor=(g['hd_idx'], g['hd_w']), hd_faces=g['hd_face'])
    valid = torch.tensor(g['valid_fit'], device=d)

    def grad():
        v = torch.tensor(g['verts'], device=d, requires_grad=True)
        crit.contact_loss(v, valid).backward()
        torch.cuda.synchronize()
        return v.grad.clone()
    assert ops.deterministic()                         # the default
    with ops.deterministic_mode(False):
        plain = grad()
    assert float(plain.abs().max()) > 0
    runs = [grad() for _ in range(4)]
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    assert_close(runs[0].cpu().numpy(), plain.cpu().numpy(), 1e-4, 1e-6 * float(plain.abs().max()), 'deterministic vs LDS float atomics')


@pytest.mark.parametrize('tag', SMALL)
def test_hd_branch_selection_partners_and_graph_capture(tag):
    """The fused HD branch (csrc/hd_contact.hip): the selected HD points of every body are exactly those of the
    restated reference (loss.py:278-281); an invalid body selects nothing; the whole contact_loss(use_hd=True) runs
    without host synchronisation, so it can be captured in a hipGraph, and the replay reproduces loss and gradient."""
    import types
    from tuch_amd.train.loss import RegressorLoss
    from tuch_amd.utils.segmentation import BatchBodySegment
    g, gm = golden(tag), golden_mask(tag)
    d = dev()
    batch = g['verts'].shape[0]
    face_tensor = torch.tensor(g['faces'], device=d)[None].repeat(batch, 1, 1)
    segs = gio.unpack_segments(g)
    crit = RegressorLoss(types.SimpleNamespace(contact_loss_weight=1.0), d, g['verts'].shape[1], face_tensor,
                         torch.tensor(np.where(gm, 1.0, 0.0).astype(np.float32), device=d), geothres=0.3,
                         euclthres=float(g['euclthres']), face_tensor=face_tensor, use_hd=True,
                         segments=BatchBodySegment(list(segs.keys()), face_tensor[0], segs),
                         hd_regressor=(g['hd_idx'], g['hd_w']), hd_faces=g['hd_face'])
    verts = torch.tensor(g['verts'], device=d, requires_grad=True)
    valid = torch.tensor(g['valid_fit'], device=d)
    loss = crit.contact_loss(verts, valid)
    loss.backward()
    counts, sel = crit._hd.selection(crit._hd.last_saved, batch)
    osegs = oracle_segments(g)
    for b in range(batch):
        if not g['valid_fit'][b]:
            assert counts[b] == 0
            continue
        r = oc.train_contact_body(g['verts'][b], g['faces'], gm, float(g['euclthres']), osegs, True,
                                  hd_idx=g['hd_idx'], hd_w=g['hd_w'], hd_face=g['hd_face'])
        want = np.where(r['hd_sel'])[0]
        got = np.sort(sel[b, :counts[b]])
        assert (sel[b, counts[b]:] == -1).all()
        assert np.array_equal(got, want), (b, len(got), len(want))
    # hipGraph capture of forward + backward (replays never on the NULL stream: tuch_amd/ops/_base.py:off_default_stream)
    from tuch_amd.ops import off_default_stream
    static_v = torch.tensor(g['verts'], device=d, requires_grad=True)
    with off_default_stream(d):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                static_v.grad = None
                crit.contact_loss(static_v, valid).backward()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        static_v.grad = None
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            out = crit.contact_loss(static_v, valid)
            out.backward()
        graph.replay()
        torch.cuda.synchronize()
        assert abs(out.item() - loss.item()) <= 1e-6 * abs(loss.item())
        assert torch.allclose(static_v.grad, verts.grad, rtol=1e-4, atol=1e-6 * float(verts.grad.abs().max()))
        # new vertices through the same graph
        with torch.no_grad():
            static_v.copy_(torch.tensor(g['verts'], device=d).flip(0))
        graph.replay()
    flipped = torch.tensor(g['verts'], device=d).flip(0).requires_grad_(True)
    want2 = crit.contact_loss(flipped, valid)
    assert abs(out.item() - want2.item()) <= 1e-5 * abs(want2.item()) + 1e-7


def test_hd_branch_with_a_general_sparse_regressor():
    """HD regressor rows with up to FIVE non-zeros (tuch_hd_model_create with K = 5; the reference multiplies the dense matrix,
    loss.py:285): RegressorLoss.contact_loss(use_hd=True) and its gradient against the oracle's HD branch fed with the
    same regressor as a dense matrix."""
    import types
    from tuch_amd.train.loss import RegressorLoss
    from tuch_amd.utils.segmentation import BatchBodySegment
    tag = 'medium'
    g, gm = golden(tag), golden_mask(tag)
    d = dev()
    batch, V = g['verts'].shape[0], g['verts'].shape[1]
    rng = np.random.default_rng(12)
    N = len(g['hd_face'])
    K = 5
    idx = np.zeros((N, K), np.int64)
    w = np.zeros((N, K), np.float32)
    faces = g['faces']
    # every point: a convex combination of its face's corners and of up to two vertices next to them
    nbr = {}
    for f in faces:
        for a in f:
            nbr.setdefault(int(a), set()).update(int(x) for x in f)
    for n in range(N):
        f = faces[g['hd_face'][n]]
        extra = [x for x in sorted(nbr[int(f[0])] | nbr[int(f[1])]) if x not in f][:2]
        k = 3 + (n % 3 if len(extra) >= 2 else 0)
        ids = list(f) + extra[:k - 3]
        wt = rng.dirichlet(np.ones(len(ids)) * 4.0)
        idx[n, :len(ids)] = ids
        idx[n, len(ids):] = ids[0]
        w[n, :len(ids)] = wt
    face_tensor = torch.tensor(g['faces'], device=d)[None].repeat(batch, 1, 1)
    segs = gio.unpack_segments(g)
    crit = RegressorLoss(types.SimpleNamespace(contact_loss_weight=1.0), d, V, face_tensor,
                         torch.tensor(np.where(gm, 1.0, 0.0).astype(np.float32), device=d), geothres=0.3,
                         euclthres=float(g['euclthres']), face_tensor=face_tensor, use_hd=True,
                         segments=BatchBodySegment(list(segs.keys()), face_tensor[0], segs), hd_regressor=(idx, w),
                         hd_faces=g['hd_face'])
    assert crit._hd.row_nnz == K
    valid = torch.ones(batch, dtype=torch.bool, device=d)
    v = torch.tensor(g['verts'], device=d, requires_grad=True)
    loss = crit.contact_loss(v, valid)
    loss.backward()
    osegs = oracle_segments(g)
    want, grads = [], []
    for b in range(batch):
        r = oc.train_contact_body(g['verts'][b], g['faces'], gm, float(g['euclthres']), osegs, True,
                                  hd_idx=idx, hd_w=w, hd_face=g['hd_face'])
        want.append(r['loss'])
        grads.append(r['grad'] / batch)
    assert_close(loss.item(), float(np.mean(want)), 2e-4, 0, 'HD loss with a 5-non-zero regressor')
    got = v.grad.cpu().numpy()
    for b in range(batch):
        grad_close(got[b], grads[b], 2e-5, 'general sparse HD regressor, body %d' % b, quantum=True)


def test_valid_mean_is_the_reference_division_in_one_launch():
    """loss.py:317: ``loss_contact.sum() / valid_fit.sum()`` over the per-body terms (ops.valid_mean: one launch forward, one
    backward): value within float32 summation order of torch's, gradient valid / n exactly, no valid body -> NaN."""
    from tuch_amd import ops
    DEV = dev()
    g = torch.Generator(device='cpu').manual_seed(4)
    for b, k in ((1, 1), (7, 2), (64, 2), (300, 1), (1000, 2)):
        terms = torch.rand(b, k, generator=g).to(DEV).requires_grad_(True)
        valid = (torch.rand(b, generator=g) < 0.7).to(DEV)
        valid[0] = True
        garbage = terms.detach().clone()
        garbage[~valid] = float('nan')                       # the other bodies' terms are never read into the sum
        garbage.requires_grad_(True)
        got = ops.valid_mean(garbage, ops.as_u8(valid))
        want = torch.where(valid[:, None], terms, torch.zeros_like(terms)).sum() / valid.sum()
        assert abs(float(got.detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
        (3.0 * got).backward()
        n = int(valid.sum())
        expect = (valid[:, None].float() * (3.0 / n)).expand(b, k)
        assert torch.allclose(garbage.grad, expect, rtol=1e-6, atol=0)
        assert float(garbage.grad[~valid].abs().sum()) == 0.0
    none = ops.valid_mean(torch.ones(5, 2, device=DEV), ops.as_u8(torch.zeros(5, dtype=torch.bool, device=DEV)))
    assert torch.isnan(none)
    m = torch.tensor([True, False, True], device=DEV)
    assert ops.as_u8(m).data_ptr() == m.data_ptr() and ops.as_u8(m).dtype == torch.uint8
