"""CPU: the host side of the renderer (tuch_amd/render.py, tuch_amd/utils/renderer.py, compat.install_renderer): view
matrices against the reference's composed transforms, the grid layout, the vertex -> faces lists, argument validation,
construction without a device, and the reference rasterisers of tests/render_cases.py against each other."""
import importlib
import sys

import numpy as np
import pytest
import torch

import render_cases as rc


def rotation_4x4(deg, axis):
    """trimesh.transformations.rotation_matrix(np.radians(deg), axis) for a coordinate axis."""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.eye(4)
    i, j = {'x': (1, 2), 'y': (2, 0)}[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


@pytest.mark.parametrize('name,dorot2,dorot3', [('front', False, False), ('rot2', True, False), ('rot3', False, True)])
def test_view_matrices_equal_the_composed_reference_transforms(name, dorot2, dorot3):
    """renderer.py:181-196, 236-240 in numpy: the mesh turned by R_x(180) (then R_y(60) / R_x(60)), the camera at
    (-t.x, t.y, t.z) looking down -z with y up, pyrender's pinhole (column f x / -z + cx, row cy - f y / -z)."""
    from tuch_amd.render import VIEWS
    rng = np.random.default_rng(5)
    v = rng.standard_normal((40, 3)) * 0.5
    t = np.array([0.13, -0.21, 4.2])
    f, cx, cy = 500.0, 112.0, 112.0
    mesh = rotation_4x4(180, 'x')
    if dorot2:
        mesh = rotation_4x4(60, 'y') @ mesh
    if dorot3:
        mesh = rotation_4x4(60, 'x') @ mesh
    pose = np.eye(4)
    pose[:3, 3] = t * np.array([-1.0, 1.0, 1.0])                       # camera_translation[0] *= -1
    q = (np.linalg.inv(pose) @ mesh @ np.concatenate([v, np.ones((40, 1))], 1).T).T
    want = np.stack([f * q[:, 0] / -q[:, 2] + cx, cy - f * q[:, 1] / -q[:, 2]], 1)
    got, z, ok = rc.project(v, VIEWS[name], t, f, cx, cy)
    assert ok.all() and np.allclose(z, -q[:, 2], rtol=0, atol=1e-12)
    assert np.allclose(got, want, rtol=0, atol=1e-9)
    if name == 'front':                                               # the project's own camera
        from tuch_amd.utils.geometry import perspective_projection
        uv = perspective_projection(torch.tensor(v)[None], torch.eye(3, dtype=torch.float64)[None], torch.tensor(t)[None], f,
                                    torch.tensor([[cx, cy]], dtype=torch.float64))[0].numpy()
        assert np.allclose(uv, got, rtol=0, atol=1e-9)


def test_views_are_rotations_and_names_are_checked():
    from tuch_amd.render import VIEWS, view_matrix
    for m in VIEWS.values():
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(m), 1.0)
    assert view_matrix('rot2') is VIEWS['rot2'] and view_matrix(np.eye(3)).shape == (3, 3)
    with pytest.raises(ValueError, match='unknown view'):
        view_matrix('side')
    with pytest.raises(ValueError, match='3, 3'):
        view_matrix(np.eye(4))


@pytest.mark.parametrize('n,nrow', [(8, 4), (3, 7), (5, 2), (1, 4)])
def test_grid_layout(n, nrow):
    from tuch_amd.render import image_grid
    h, w = 5, 7
    tiles = torch.arange(n * 3 * h * w, dtype=torch.float32).reshape(n, 3, h, w) + 1.0
    grid = image_grid(tiles, nrow=nrow)
    cols = min(nrow, n)
    rows = -(-n // cols)
    assert grid.shape == (3, rows * (h + 2) + 2, cols * (w + 2) + 2)
    seen = torch.zeros(grid.shape[1:], dtype=torch.bool)
    for k in range(n):
        r, c = divmod(k, cols)
        assert torch.equal(grid[:, r * (h + 2) + 2: r * (h + 2) + 2 + h, c * (w + 2) + 2: c * (w + 2) + 2 + w], tiles[k])
        seen[r * (h + 2) + 2: r * (h + 2) + 2 + h, c * (w + 2) + 2: c * (w + 2) + 2 + w] = True
    assert torch.all(grid[:, ~seen] == 0)
    try:
        from torchvision.utils import make_grid
    except Exception:
        return
    assert torch.equal(make_grid(list(tiles), nrow=nrow), grid) or n == 1   # (make_grid returns a single image unpadded)


def test_vertex_face_table():
    from tuch_amd import ops
    from synthetic import make_body
    faces = make_body(10, 12).faces
    off, ids = ops.vertex_face_table(faces, 125)                      # three vertices more than the mesh uses
    assert off.dtype == np.int32 and ids.dtype == np.int32 and off.shape == (126,) and ids.shape == (3 * len(faces),)
    assert off[0] == 0 and off[-1] == 3 * len(faces) and np.all(np.diff(off) >= 0)
    for v in range(125):
        want = np.sort(np.nonzero((faces == v).any(1))[0])
        assert np.array_equal(ids[off[v]:off[v + 1]], want), v
    twice = np.array([[0, 0, 1], [2, 1, 0]])
    off, ids = ops.vertex_face_table(twice, 3)
    assert off.tolist() == [0, 3, 5, 6] and ids.tolist() == [0, 0, 1, 0, 1, 1]
    for bad in (np.zeros((0, 3), int), np.zeros((2, 4), int), np.array([[0, 1, 3]]), np.array([[0, -1, 2]])):
        with pytest.raises(ValueError):
            ops.vertex_face_table(bad, 3)


def test_construction_needs_no_device_and_arguments_are_checked():
    from tuch_amd import _C
    from tuch_amd.render import MeshRenderer
    from tuch_amd.utils.renderer import Renderer
    faces = np.array([[0, 1, 2], [2, 1, 3]])
    r = MeshRenderer(faces, img_res=(48, 64), focal_length=300.)
    assert (r.height, r.width) == (48, 64) and r.camera_center == (32.0, 24.0)
    assert MeshRenderer(torch.tensor(faces)).camera_center == (112.0, 112.0)
    for kw in (dict(faces=np.zeros((0, 3), int)), dict(faces=faces[:, :2]), dict(faces=-faces), dict(faces=faces, img_res=0),
               dict(faces=faces, img_res=(1, 2, 3)), dict(faces=faces, focal_length=0.0)):
        with pytest.raises(ValueError):
            MeshRenderer(**kw)
    verts, cam = torch.zeros(2, 4, 3), torch.zeros(2, 3)
    with pytest.raises(_C.TuchError, match='HIP device'):             # no host fallback
        r.render(verts, cam)
    with pytest.raises(_C.TuchError, match='HIP device'):
        r.contact_colors(verts, partner=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match='verts has 3'):
        r.render(torch.zeros(1, 3, 3), cam[:1])
    with pytest.raises(ValueError):
        r.render(verts[0], cam)
    with pytest.raises(ValueError, match='exactly one'):
        r.contact_colors(verts, pairs={}, partner=torch.zeros(2, 4))
    ref = Renderer({'classes': [], 'csig': {}}, focal_length=5000, img_res=224, faces=faces)
    assert ref.camera_center == [112, 112] and ref.focal_length == 5000 and ref.faces is faces
    with pytest.raises(ValueError, match='weak_perspective'):
        Renderer(None, cam_type='weak_perspective', faces=faces)
    with pytest.raises(ValueError, match='keypoints'):
        ref.visu_smplifycontactopti([verts], cam, torch.zeros(2, 3, 224, 224), [None, None], keypoints=torch.zeros(2, 49, 3))


def test_c_abi_checks_its_arguments_without_a_device():
    from tuch_amd import _C
    L = _C.lib()
    assert L.tuch_render_workspace_bytes(64, 3, 6890, 13776, 224, 224) >= 64 * 3 * 224 * 224 * 8
    assert L.tuch_render_workspace_bytes(1, 33, 10, 10, 8, 8) == 0
    rc_ = L.tuch_render_mesh(None, None, None, None, 1, 3, 1, None, None, 1, 1.0, 0.0, 0.0, 8, 8, None, None, 0, None, None, None,
                             None, 0, None)
    assert rc_ != 0 and b'null pointer' in L.tuch_last_error()
    rc_ = L.tuch_render_mesh(None, None, None, None, 1, 3, 1, None, None, 40, 1.0, 0.0, 0.0, 8, 8, None, None, 0, None, None, None,
                             None, 0, None)
    assert rc_ != 0 and b'bad sizes' in L.tuch_last_error()
    rc_ = L.tuch_contact_vertex_colors(None, 1, 3, None, None, None, 0, None, None, 0, None, None, None, 0, None, None, 0, None)
    assert rc_ != 0 and b'null pointer' in L.tuch_last_error()


def test_install_renderer_is_opt_in():
    from tuch_amd import compat
    import tuch_amd.utils.renderer as ours
    compat.uninstall()
    try:
        compat.install()
        assert 'tuch.utils.renderer' not in sys.modules               # left to the reference checkout
        assert compat._finder.find_spec('tuch.utils.renderer') is None
        assert compat._finder.find_spec('tuch.utils.contact') is not None
        assert compat.install_renderer() == ['tuch.utils.renderer']
        assert importlib.import_module('tuch.utils.renderer') is ours
        from tuch.utils.renderer import Renderer                      # noqa: the reference's import line
        assert Renderer is ours.Renderer
        del sys.modules['tuch.utils.renderer']                        # somebody emptied sys.modules: still ours
        assert importlib.import_module('tuch.utils.renderer') is ours
        compat.uninstall()
        assert 'tuch.utils.renderer' not in sys.modules
        compat.install()                                              # the opt-in does not outlive uninstall()
        assert compat._finder.find_spec('tuch.utils.renderer') is None
    finally:
        compat.uninstall()


def test_reference_rasterisers_agree_off_the_excluded_pixels():
    """The two numpy rasterisers of render_cases.py, one with the device's snapping and integer rules and one in plain
    float64, on the smallest body: identical faces off the exclusion band, which stays under the caps of the GPU test."""
    from oracle import lbs as olbs
    from synthetic import make_body, through_pose
    from tuch_amd.render import VIEWS
    body = make_body(10, 12)
    bp, go, be = [torch.tensor(np.asarray(x, np.float32)) for x in through_pose(1, 7)]
    verts = olbs.smpl_forward(olbs.model_tensors(body), be, bp, go)[0][0].numpy().astype(np.float32)
    f = 0.8 * 64 * 5.0 / np.ptp(body.v_template, 0).max()
    for name in ('front', 'rot2'):
        ref = rc.float_raster(verts, body.faces, VIEWS[name], [0.02, -0.03, 5.0], f, 32, 32, 64, 64)
        face, depth = rc.integer_raster(verts, body.faces, VIEWS[name], [0.02, -0.03, 5.0], f, 32, 32, 64, 64)
        ex, cov = rc.excluded(ref), ref['face'] >= 0
        assert cov.sum() > 400 and ex.mean() <= 0.02 and (ex & cov).sum() <= 0.10 * cov.sum()
        assert np.array_equal(face[~ex], ref['face'][~ex])
        assert np.all((ref['image'] >= 0) & (ref['image'] <= 1)) and np.all(ref['image'][~cov] == 1.0)


def test_colour_references():
    v = np.array([[0, 0, 0], [1, 2, 4], [0.5, 1, 1], [0.25, 2, 3]], np.float32)
    mc = rc.meshcols(v)
    assert mc.tolist() == [[0, 0, 0], [255, 255, 255], [127, 127, 63], [63, 255, 191]]
    col, src = rc.contact_colors_pairs(v, [1, 2], [2, 3])
    assert src.tolist() == [[-1, -1], [1, 2], [2, 3], [2, 3]]
    assert col[0].tolist() == [230] * 3 and col[1].tolist() == [191, 191, 159] and col[2].tolist() == col[3].tolist() == [95, 191, 127]
    col, src = rc.contact_colors_regions(v, [1, 0], [('a', 'b'), ('b', 'a')], {'a': [2, 0], 'b': [3]})
    assert col[1].tolist() == [230] * 3 and col[0].tolist() == col[2].tolist() == col[3].tolist() == mc[2].tolist()
