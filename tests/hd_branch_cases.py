"""Fixtures and the float64 restatement for the HD branch of RegressorLoss.contact_loss (csrc/hd_contact.hip and the
search of csrc/hd_search.hip), shared by tests/test_hd_branch_host.py (no GPU) and tests/test_gpu_hd_branch.py.

The branch takes the VERTEX-level results (exterior flags, masked minimum distance, validity) as arguments, so the
selection of every body is constructed here instead of coming out of a pose:

  * mesh, geodesic mask and poses: the golden `medium` bodies (1602 vertices, 3200 faces);
  * a synthetic HD regressor.  Ten FANS (all faces around a centre vertex, pairwise disjoint) carry FAN_POINTS points in
    all, every other face one point; flagging the centres of fans 0..k and nothing else selects exactly the points of
    those fans: PREFIX_COUNTS = 1, 32, 33, 64, 65 (tile edges of the search), 1023, 1024, 1025 (the chunk of the
    selection kernels and the span of the point adjoint), 2048, 2049 (the second trip of the adjoint's loop).  Fans 0 and
    1 are geodesic neighbours: bodies 0 and 1 have no admissible pair at all.  The caller's order is a fixed shuffle;
  * three row formats of the same points' faces: K = 3 (barycentric), K = 1 (a corner of the face), K = 8 (convex
    weights over the corners and vertices next to them, short rows padded with weight 0 and a valid id);
  * 13 bodies: 0..9 the prefixes, 10 valid with nothing flagged, 11 invalid with everything flagged, 12 everything.

`reference` restates loss.py:278-297 in numpy float64 from those inputs, `evaluate` loss.py:299-315 and its adjoint for
GIVEN partners and flags.  Nothing here calls the library under test."""
import functools

import numpy as np

from helpers import golden, golden_mask

TAG = 'medium'
THRESH = 0.99
FAN_POINTS = (1, 31, 1, 31, 1, 958, 1, 1, 1023, 1)
PREFIX_COUNTS = tuple(int(c) for c in np.cumsum(FAN_POINTS))      # 1 32 33 64 65 1023 1024 1025 2048 2049
# centre vertices of the fans (tests/test_hd_branch_host.py checks every condition they were chosen for): fans 0 and 1
# are geodesic neighbours (fan 0 is a pole of the mesh: 40 faces, one point); fan 5 lies where pose 1 interpenetrates
# (interior and exterior points) and fan 8 on the part it touches there, 9 mm away; the others are geodesically far from
# all of them and at least 15 cm from fans 5 and 8 in that pose
FAN_CENTRES = (0, 41, 296, 355, 448, 841, 481, 498, 913, 509)
# the golden pose of every body
BODY_POSE = (0, 1, 2, 0, 1, 1, 1, 1, 1, 1, 2, 0, 0)
BATCH = len(BODY_POSE)
EMPTY_VALID, INVALID, EVERYTHING = 10, 11, 12
KS = (1, 3, 8)
# upstream gradient of (interior sum, exterior sum) per body: non-uniform, negative for body 3, no interior part for
# body 6 (which has interior points)
GRAD_TERMS = np.array([[1.0, 1.0], [0.5, 2.0], [1.5, 0.25], [-1.0, -0.75], [2.0, 1.0], [1.0, 3.0], [0.0, 1.25],
                       [0.75, 0.5], [1.25, 2.0], [3.0, 0.5], [1.0, 1.0], [1.0, 1.0], [0.5, 1.5]], np.float32)
NO_INTERIOR_GRAD = 6
# an unflagged vertex outside the fans whose min_d2 is exactly the threshold in bodies 0..10
EQUAL_VERTEX = 1601


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def mesh():
    """(faces [F,3] int64, geomask [V,V] bool, verts [BATCH,V,3] float32, euclthres)."""
    g = golden(TAG)
    verts = np.ascontiguousarray(g['verts'][list(BODY_POSE)], np.float32)
    return g['faces'].astype(np.int64), golden_mask(TAG), _frozen(verts), float(g['euclthres'])


@functools.lru_cache(maxsize=None)
def fans():
    """Face ids of every fan, ascending."""
    faces = mesh()[0]
    return tuple(_frozen(np.where((faces == c).any(1))[0]) for c in FAN_CENTRES)


@functools.lru_cache(maxsize=None)
def layout():
    """(hd_face [N] in the caller's order, fan [N]: the fan of every point or -1, build [N]: running number of the point
    on its face): FAN_POINTS[i] points dealt round the faces of fan i, one point on every face outside the fans, then a
    fixed shuffle."""
    faces = mesh()[0]
    face, fan, num = [], [], []
    in_fan = np.zeros(len(faces), bool)
    for i, fs in enumerate(fans()):
        assert not in_fan[fs].any(), 'fans share a face'
        in_fan[fs] = True
        for k in range(FAN_POINTS[i]):
            face.append(int(fs[k % len(fs)]))
            fan.append(i)
            num.append(k // len(fs))
    for f in np.where(~in_fan)[0]:
        face.append(int(f))
        fan.append(-1)
        num.append(0)
    perm = np.random.default_rng(20).permutation(len(face))
    return _frozen(np.asarray(face, np.int64)[perm], np.asarray(fan, np.int64)[perm], np.asarray(num, np.int64)[perm])


def num_points():
    return len(layout()[0])


@functools.lru_cache(maxsize=None)
def regressor(K):
    """(hd_idx [N,K] int64, hd_w [N,K] float32, hd_face [N] int64) of the row format K."""
    faces = mesh()[0]
    hd_face, _, num = layout()
    n = len(hd_face)
    # (seeds with which no offset point comes within 2 um of a triangle in the poses it is used in:
    # test_hd_branch_host.py::test_no_offset_point_touches_the_surface)
    rng = np.random.default_rng({1: 101, 3: 103, 8: 300}[K])
    bary = rng.dirichlet([2.0, 2.0, 2.0], n)
    corners = faces[hd_face]
    if K == 3:
        idx, w = corners.copy(), bary.astype(np.float32)
    elif K == 1:
        # the points of a face go round its corners: the centre of a big fan supports a third of the fan's points
        pick = (num + np.arange(n)) % 3
        idx = corners[np.arange(n), pick][:, None].copy()
        w = np.ones((n, 1), np.float32)
    elif K == 8:
        nbr = [set() for _ in range(int(faces.max()) + 1)]
        for tri in faces:
            for a in tri:
                nbr[int(a)].update(int(x) for x in tri)
        idx = np.zeros((n, 8), np.int64)
        w = np.zeros((n, 8), np.float32)
        for p in range(n):
            tri = [int(x) for x in corners[p]]
            extra = [x for x in sorted(nbr[tri[0]] | nbr[tri[1]] | nbr[tri[2]]) if x not in tri]
            k = 3 + p % 6                                         # 3..8 non-zeros: rows with fewer are padded
            ids = tri + extra[:k - 3]
            # convex: 97 % on the face, the rest spread over the vertices next to it (the point stays well within the
            # 1 mm of the offset from its face)
            wt = 0.97 * bary[p] if len(ids) > 3 else bary[p]
            wt = np.concatenate([wt, 0.03 * rng.dirichlet(np.ones(len(ids) - 3))]) if len(ids) > 3 else wt
            idx[p, :len(ids)] = ids
            idx[p, len(ids):] = ids[p % len(ids)]                 # padding: weight 0, a valid id
            w[p, :len(ids)] = wt
    else:
        raise ValueError(K)
    return _frozen(idx, w, hd_face)


@functools.lru_cache(maxsize=None)
def inputs():
    """(exterior [B,V] uint8, min_d2 [B,V] float32, valid [B] uint8): the vertex-level inputs, CONSTRUCTED.  A vertex is
    flagged through exterior == 0 or through min_d2 one float32 step below float32(euclthres)^2; unflagged vertices with
    min_d2 == float32(euclthres)^2 exactly (the centres of the fans a prefix body leaves out, and vertex EQUAL_VERTEX in
    bodies 0..10) must not select (loss.py:278 is strict)."""
    _, _, verts, euclthres = mesh()
    v = verts.shape[1]
    e2 = eucl2(euclthres)
    below = np.nextafter(e2, np.float32(0.0))
    assert below < e2
    exterior = np.ones((BATCH, v), np.uint8)
    min_d2 = np.ones((BATCH, v), np.float32)
    valid = np.ones(BATCH, np.uint8)
    for b in range(EMPTY_VALID + 1):
        min_d2[b, EQUAL_VERTEX] = e2
        for i, c in enumerate(FAN_CENTRES):
            if b < EMPTY_VALID and i <= b:
                if i % 2 == 0:
                    exterior[b, c] = 0
                else:
                    min_d2[b, c] = below
            else:
                min_d2[b, c] = e2
    valid[INVALID] = 0
    exterior[INVALID] = 0
    min_d2[INVALID] = 0.0
    exterior[EVERYTHING, 0::2] = 0
    min_d2[EVERYTHING, 1::2] = below
    return _frozen(exterior, min_d2, valid)


def eucl2(euclthres):
    """float32(euclthres)^2 in float32: the threshold of loss.py:278 as the reference's float32 tensors compare it."""
    return np.float32(euclthres) * np.float32(euclthres)


# ------------------------------------------------------------------------------------------------ the float64 restatement
def winding_numbers(points, tris, chunk=256):
    """float64 winding numbers of points [Q,3] against triangles [F,3,3] (contact.py:79-147): sum of the solid angles
    2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|) over 4 pi."""
    points, tris = np.asarray(points, np.float64), np.asarray(tris, np.float64)
    out = np.empty(len(points))

    def some(lo):
        # coordinate by coordinate ([Q,F] arrays): the same sums as the vector form, several times faster in numpy
        p = points[lo:lo + chunk]
        ax, ay, az = (tris[None, :, 0, k] - p[:, k, None] for k in range(3))
        bx, by, bz = (tris[None, :, 1, k] - p[:, k, None] for k in range(3))
        cx, cy, cz = (tris[None, :, 2, k] - p[:, k, None] for k in range(3))
        la, lb, lc = np.sqrt(ax * ax + ay * ay + az * az), np.sqrt(bx * bx + by * by + bz * bz), np.sqrt(cx * cx + cy * cy + cz * cz)
        num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
        den = (la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (ax * cx + ay * cy + az * cz) * lb
               + (bx * cx + by * cy + bz * cz) * la)
        out[lo:lo + chunk] = np.arctan2(num, den).sum(1) / (2.0 * np.pi)

    # (the chunks are independent and numpy releases the interpreter lock: a few threads)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=4) as pool:
        list(pool.map(some, range(0, len(points), chunk)))
    return out


def reference(verts_b, faces, geomask, hd_idx, hd_w, hd_face, exterior_b, min_d2_b, valid_b, euclthres, thresh=THRESH,
              winding_cache=None):
    """loss.py:278-297 for one body in float64, from the given vertex-level inputs.  Points are listed by ascending
    caller id; a row / column of the n x n matrix is a position in that list.  Returns a dict:
      sel [n] caller ids; pts, offs [n,3]; winding [n]; exterior [n] (w <= thresh); vid [n] mask vertex;
      min_d2 [n] masked minimum per column (inf: no admissible row); argmin [n] (first row attaining it, -1: none);
      admissible [n] number of admissible rows per column.
    winding_cache: a dict {caller id: winding} of this pose and regressor, filled and reused (the points of a body
    contained in another one of the same pose are not evaluated twice)."""
    v = np.asarray(verts_b, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    hd_idx, hd_face = np.asarray(hd_idx, np.int64), np.asarray(hd_face, np.int64)
    w = np.asarray(hd_w, np.float32).astype(np.float64)
    cand = np.zeros(len(v), bool)
    if valid_b:
        cand = (np.asarray(min_d2_b, np.float32) < eucl2(euclthres)) | (np.asarray(exterior_b) == 0)      # :278
    face_sel = cand[faces].any(1)                                                                         # :279-280
    sel = np.where(face_sel[hd_face])[0]                                                                  # :281
    n = len(sel)
    pts = (v[hd_idx[sel]] * w[sel][:, :, None]).sum(1)                                                    # :285
    tri = v[faces[hd_face[sel]]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    offs = pts + 0.001 * nrm / np.linalg.norm(nrm, axis=1, keepdims=True)                                 # :295-296
    wind = np.empty(n)
    todo = np.ones(n, bool)
    if winding_cache is not None:
        for i, s in enumerate(sel):
            if int(s) in winding_cache:
                wind[i], todo[i] = winding_cache[int(s)], False
    if todo.any():
        wind[todo] = winding_numbers(offs[todo], v[faces])                                                # :297
        if winding_cache is not None:
            winding_cache.update(zip(sel[todo].tolist(), wind[todo].tolist()))
    vid = faces[hd_face[sel], 0]                                                                          # :88
    mn, arg, adm = np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for lo in range(0, n, 512):                                                                           # :288-291
        cols = slice(lo, lo + 512)
        d2 = ((pts[:, None, :] - pts[None, cols, :]) ** 2).sum(2)                     # [row, column]
        ok = geomask[vid[:, None], vid[None, cols]]                                  # geomask[vid[row]][vid[column]]
        d2 = np.where(ok, d2, np.inf)
        adm[cols] = ok.sum(0)
        mn[cols] = d2.min(0)
        arg[cols] = np.where(adm[cols] > 0, d2.argmin(0), -1)
    return dict(sel=sel, n=n, pts=pts, offs=offs, winding=wind, exterior=wind <= thresh, vid=vid, min_d2=mn, argmin=arg,
                admissible=adm)


def pair_d2(ref, rows, cols):
    """float64 squared distances of the pairs (rows[i], cols[i]) and whether the mask admits them."""
    d2 = ((ref['pts'][rows] - ref['pts'][cols]) ** 2).sum(1)
    return d2, geomask_of(ref, rows, cols)


def geomask_of(ref, rows, cols):
    return mesh()[1][ref['vid'][rows], ref['vid'][cols]]


def evaluate(ref, partner, exterior, grad_terms_b, hd_idx, hd_w, num_verts, keep=None):
    """loss.py:299-315 and its adjoint in float64 for GIVEN partners (positions in ref['sel']) and exterior flags:
    (terms [2] = (sum over interior points of tanh^2(d / 0.04), sum over exterior ones of 0.005 tanh^2(d / 0.005)),
    grad [V,3] of grad_terms_b . terms w.r.t. the vertices).  torch.norm's backward at d == 0 is taken as 0.
    keep [n] bool: only these points contribute (e.g. the exterior ones alone)."""
    n = ref['n']
    grad = np.zeros((num_verts, 3))
    if n == 0:
        return np.zeros(2), grad
    partner, exterior = np.asarray(partner, np.int64), np.asarray(exterior, bool)
    keep = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    pts = ref['pts']
    diff = pts - pts[partner]
    d = np.sqrt((diff * diff).sum(1))
    weight, scale = np.where(exterior, 0.005, 1.0), np.where(exterior, 0.005, 0.04)
    t = np.tanh(d / scale)
    value = np.where(keep, weight * t * t, 0.0)
    terms = np.array([value[~exterior].sum(), value[exterior].sum()])
    g = np.where(exterior, float(grad_terms_b[1]), float(grad_terms_b[0]))
    coef = np.zeros(n)
    pos = keep & (d > 0)
    coef[pos] = (g * 2.0 * weight * t * (1.0 - t * t) / scale)[pos] / d[pos]
    gp = np.zeros((n, 3))
    np.add.at(gp, np.arange(n), coef[:, None] * diff)
    np.add.at(gp, partner, -coef[:, None] * diff)
    idx = np.asarray(hd_idx, np.int64)[ref['sel']]
    w = np.asarray(hd_w, np.float32).astype(np.float64)[ref['sel']]
    for k in range(idx.shape[1]):
        np.add.at(grad, idx[:, k], gp * w[:, k:k + 1])
    return terms, grad


@functools.lru_cache(maxsize=None)
def fixture_reference(K):
    """reference() of the 13 bodies for the row format K, computed once (read-only)."""
    faces, gm, verts, euclthres = mesh()
    hd_idx, hd_w, hd_face = regressor(K)
    exterior, min_d2, valid = inputs()
    caches = {}
    out = []
    for b in range(BATCH):
        r = reference(verts[b], faces, gm, hd_idx, hd_w, hd_face, exterior[b], min_d2[b], valid[b], euclthres,
                      winding_cache=caches.setdefault(BODY_POSE[b], {}))
        _frozen(*(x for x in r.values() if isinstance(x, np.ndarray)))
        out.append(r)
    return tuple(out)


def supported_vertices(K, ref):
    """[V] bool: vertices with a non-zero weight in the row of a selected point."""
    hd_idx, hd_w, _ = regressor(K)
    out = np.zeros(mesh()[2].shape[1], bool)
    idx, w = hd_idx[ref['sel']], hd_w[ref['sel']]
    out[idx[w != 0]] = True
    return out


def tile_runs(mask_vertices):
    """Per tile of 32 consecutive slots: (runs of equal consecutive mask vertices, distinct mask vertices)."""
    mv = np.asarray(mask_vertices)
    runs, distinct = [], []
    for lo in range(0, len(mv), 32):
        t = mv[lo:lo + 32]
        runs.append(1 + int((t[1:] != t[:-1]).sum()))
        distinct.append(len(np.unique(t)))
    return np.asarray(runs), np.asarray(distinct)
