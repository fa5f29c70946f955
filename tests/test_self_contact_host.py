"""CPU: the host side of self-contact detection -- the vertex -> regions table, constructors that must run where no
GPU is visible, the drop-in name and the exported symbol."""
import ctypes
import sys

import numpy as np
import pytest
import torch


def test_vertex_region_table():
    from tuch_amd.ops import vertex_region_table
    # regions 0 and 2 overlap in vertices 2 and 3, region 1 is empty, vertices 5 and 7 belong to no region,
    # vertex 4 is listed twice in region 2
    regions = [[3, 0, 2], [], [2, 3, 4, 4, 6]]
    off, ids = vertex_region_table(regions, 8)
    assert off.dtype == np.int32 and ids.dtype == np.int32 and off.shape == (9,)
    got = [ids[off[v]:off[v + 1]].tolist() for v in range(8)]
    assert got == [[0], [], [0, 2], [0, 2], [2], [], [2], []]
    assert off[0] == 0 and off[-1] == len(ids) == 7
    off, ids = vertex_region_table([], 3)
    assert off.tolist() == [0, 0, 0, 0] and ids.size == 0


def test_vertex_region_table_errors():
    from tuch_amd.ops import vertex_region_table
    with pytest.raises(ValueError, match='outside'):
        vertex_region_table([[0, 8]], 8)
    with pytest.raises(ValueError, match='outside'):
        vertex_region_table([[1], [-1]], 8)
    with pytest.raises(ValueError, match='128'):
        vertex_region_table([[0]] * 129, 8)
    vertex_region_table([[0]] * 128, 8)


def _small_inputs():
    rng = np.random.default_rng(0)
    geod = rng.random((12, 12)).astype(np.float32)
    geod = geod + geod.T
    faces = np.array([[0, 1, 2], [2, 3, 11]])
    contactlists = {'classes': [('a', 'b')], 'csig': {'a': [0, 1, 2], 'b': [5, 6]}}
    return geod, faces, contactlists


def test_constructors_run_without_a_device():
    from tuch_amd.contact_detect import SelfContact
    from tuch_amd.train.train_module import TUCH
    geod, faces, contactlists = _small_inputs()
    det = SelfContact(geod, regions=contactlists['csig'])
    assert (det.geothres, det.euclthres) == (0.3, 0.02)                     # configs/config.py:90-91
    assert det.num_verts == 12 and det.num_regions == 2 and det.region_names == ['a', 'b']
    det = SelfContact(geomask=torch.tensor(geod) >= 0.3, regions=[[0, 1], [], [1, 4]], euclthres=0.05)
    assert det.region_names == [0, 1, 2] and det.num_regions == 3
    assert SelfContact(geod).num_regions == 0
    with pytest.raises(ValueError):
        SelfContact()
    with pytest.raises(ValueError):
        SelfContact(geod, geomask=geod >= 0.3)
    with pytest.raises(ValueError):
        SelfContact(geod[:, :5])
    with pytest.raises(ValueError, match='outside'):
        SelfContact(geod, regions=[[12]])
    module = TUCH(contactlists=contactlists, faces=faces, geodistssmpl=torch.tensor(geod), device='cuda')
    assert callable(module.get_verts_in_contact)
    # vertices on the host: an error, not a fallback
    with pytest.raises(Exception, match='HIP device'):
        module.get_verts_in_contact(torch.zeros(1, 12, 3))
    with pytest.raises(ValueError, match='geodistssmpl'):
        TUCH(contactlists=contactlists, faces=faces, device='cuda').get_verts_in_contact(torch.zeros(1, 12, 3))


def test_evaluator_argument_exists_and_defaults_to_none():
    import inspect
    from tuch_amd.eval import Evaluator
    assert inspect.signature(Evaluator.__init__).parameters['contact'].default is None
    assert list(inspect.signature(Evaluator.add).parameters) == ['self', 'pred_vertices', 'gt_vertices', 'gt_joints',
                                                                  'contact_vertices']


def test_drop_in_name_after_install():
    import inspect
    import tuch_amd.compat as compat
    saved = {k: v for k, v in sys.modules.items() if k == 'tuch' or k.startswith('tuch.')}
    try:
        compat.install()
        from tuch.train.train_module import TUCH
        assert list(inspect.signature(TUCH.get_verts_in_contact).parameters)[:2] == ['self', 'verts']
    finally:
        for k in [k for k in sys.modules if k == 'tuch' or k.startswith('tuch.')]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_symbol_exported_and_arguments_checked():
    from tuch_amd import _C, _build
    _build.build()
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), 'tuch_self_contact')
    assert 'tuch_self_contact' in _C.exported_symbols()
    L = _C.lib()
    one = ctypes.c_void_p(256)                     # never dereferenced: every call below fails or returns before a launch
    assert L.tuch_self_contact(None, None, 0, 0, 0.02, None, None, 0, None, None, None, None, None, None) == 0   # B = 0
    assert L.tuch_self_contact(None, one, 1, 4, 0.02, None, None, 0, one, one, one, None, one, None) != 0
    assert b'null pointer' in L.tuch_last_error()
    assert L.tuch_self_contact(one, one, 1, 0, 0.02, None, None, 0, one, one, one, None, one, None) != 0
    assert b'vertex count' in L.tuch_last_error()
    assert L.tuch_self_contact(one, one, 1, 4, 0.02, one, one, 129, one, one, one, one, one, None) != 0
    assert b'regions' in L.tuch_last_error()
    assert L.tuch_self_contact(one, one, -1, 4, 0.02, None, None, 0, one, one, one, None, one, None) != 0
