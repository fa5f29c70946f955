"""The layout of the package tuch_amd/ops, read as source (ast): nothing is imported, no library is loaded.

One module per kernel family in ONE declared order; __init__ re-exports the public names and defines nothing; nobody
outside reads a private name off ``ops``."""
import ast
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'tuch_amd', 'ops')

# the declared import order: a module imports only from the ones before it
ORDER = ['_base', 'args', 'dense', 'selfcontact', 'normals_render', 'terms', 'objectives', 'mesh_fit', 'closest_point',
         'model', 'point_cloud', 'hd', 'image_crop']
MAX_LINES = 650

# what callers reach as ops.<name>: the 68 public top-level names ops.py had as one file ...
PUBLIC = """
CROP_FRAC_BITS CROP_MAX_K CROP_MAX_RES CROP_RECORD ClosestPoint CloudGrid ContactModel DeviceCropRecords FitWeights
HDModel IMAGE_TABLE KNearest MAX_CONTACT_REGIONS MAX_NEIGHBOURS MAX_RENDER_VIEWS MODE_SMPLIFY MODE_TRAIN NearestPoint
PointCloud PointNormals SCAN_RHO TransferTable VertexNormalTable as_u8 batch_pairwise_dist cached_derived
check_crop_records cloud_fit cluster_tree contact_terms contact_terms_mean contact_terms_ragged contact_vertex_colors
crop_batch crop_box crop_records deterministic deterministic_mode fit_weights gather_triangles hd_points mesh_transfer
near_encode_host off_default_stream pack_geomask pack_images region_tables render_mesh scan_fit segment_faces
self_contact set_cloud_canary set_deterministic smplify_objective smplify_small_terms smplify_stage1_objective
smplify_stage2_tail solid_angles transfer_table upload_crop_records v2v_min_masked valid_mean vertex_face_table
vertex_fit vertex_normal_table vertex_normals vertex_region_table winding_numbers
""".split()
# ... and backward_scalar, which backward_pass.py defines
FROM_OUTSIDE = {'backward_scalar': 'backward_pass'}
# the dicts of _base: changed in place, bound once, named nowhere else
STATE = {'_SIDE_STREAMS', '_STREAM_OBJECTS', '_GRAPH_STREAMS', '_TICKETS', '_DERIVED'}


def parse(path):
    with open(path) as fh:
        return ast.parse(fh.read(), path)


@pytest.fixture(scope='module')
def modules():
    files = sorted(f[:-3] for f in os.listdir(PKG) if f.endswith('.py'))
    assert files == sorted(ORDER + ['__init__']), 'the modules of tuch_amd/ops are not the declared ones'
    assert not os.path.exists(os.path.join(ROOT, 'tuch_amd', 'ops.py'))
    return {m: parse(os.path.join(PKG, m + '.py')) for m in files}


def defined(tree):
    """Top-level names a module binds itself (def, class, assignment)."""
    out = []
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            out.append(node.name)
        elif isinstance(node, (ast.Assign, ast.AnnAssign, ast.AugAssign)):
            targets = node.targets if isinstance(node, ast.Assign) else [node.target]
            out += [n.id for t in targets for n in ast.walk(t) if isinstance(n, ast.Name)]
    return out


def test_public_names_are_68():
    assert len(PUBLIC) == len(set(PUBLIC)) == 68 and not any(n.startswith('_') for n in PUBLIC)
    assert not set(PUBLIC) & set(ORDER), 'a module named like a public name would be shadowed by the re-export'


def test_init_defines_nothing_and_reexports_public_names_only(modules):
    tree = modules['__init__']
    exported = {}
    for k, node in enumerate(tree.body):
        if k == 0 and isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant):
            continue                                            # the docstring
        if isinstance(node, ast.Assign) and [getattr(t, 'id', None) for t in node.targets] == ['__all__']:
            continue
        assert isinstance(node, ast.ImportFrom) and node.level >= 1, \
            '__init__.py line %d: only relative imports (and __all__) belong here' % node.lineno
        for a in node.names:
            name = a.asname or a.name
            assert not name.startswith('_') and a.name != '*', '__init__.py exports %r' % name
            assert name not in exported, '%r is exported twice' % name
            exported[name] = (node.level, node.module)
    for name in PUBLIC:
        assert name in exported, 'ops.%s is gone' % name
    for name, module in FROM_OUTSIDE.items():
        assert exported.get(name) == (2, module)
    extra = set(exported) - set(PUBLIC) - set(FROM_OUTSIDE) - set(ORDER)
    assert not extra, 'exported beyond the public surface: %s' % sorted(extra)


def test_every_public_name_has_one_owner(modules):
    owners = {}
    for m in ORDER:
        names = defined(modules[m])
        assert len(names) == len(set(names)), '%s.py binds a name twice' % m
        for n in names:
            owners.setdefault(n, []).append(m)
    twice = {n: ms for n, ms in owners.items() if len(ms) > 1}
    assert not twice, 'defined in more than one module: %s' % twice
    reexport = {(a.asname or a.name): node.module for node in modules['__init__'].body
                if isinstance(node, ast.ImportFrom) and node.level == 1 and node.module for a in node.names}
    for name in PUBLIC:
        assert name in owners, '%s is defined in no module' % name
        assert reexport.get(name) == owners[name][0], '%s: re-exported from %s, defined in %s' % (
            name, reexport.get(name), owners[name][0])


def test_imports_follow_the_declared_order_at_module_level(modules):
    for m in ORDER:
        tree = modules[m]
        top = set(id(n) for n in tree.body)
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                assert not any(a.name.startswith('tuch_amd') for a in node.names), '%s.py line %d' % (m, node.lineno)
            if not isinstance(node, ast.ImportFrom):
                continue
            assert node.level or not (node.module or '').startswith('tuch_amd'), \
                '%s.py line %d: the package is imported relatively' % (m, node.lineno)
            if node.level == 1:
                assert id(node) in top, '%s.py line %d: an import of a sibling inside a body' % (m, node.lineno)
                siblings = [node.module.split('.')[0]] if node.module else [a.name for a in node.names]
                for s in siblings:
                    assert s in ORDER and ORDER.index(s) < ORDER.index(m), \
                        '%s.py line %d imports %s, which does not come before it' % (m, node.lineno, s)
            elif node.level == 2:
                # the rest of tuch_amd: never the package itself, by either spelling
                assert node.module != 'ops' and not (node.module or '').startswith('ops.'), '%s.py line %d' % (m, node.lineno)
                assert node.module or not any(a.name == 'ops' for a in node.names), '%s.py line %d' % (m, node.lineno)


def test_no_module_exceeds_the_size_cap(modules):
    for m in modules:
        with open(os.path.join(PKG, m + '.py')) as fh:
            n = sum(1 for _ in fh)
        assert n <= MAX_LINES, '%s.py has %d lines (cap: %d)' % (m, n, MAX_LINES)


def test_family_modules_name_the_sources_they_bind(modules):
    for m in ORDER:
        doc = ast.get_docstring(modules[m])
        assert doc, '%s.py has no docstring' % m
        if m != 'args':
            assert 'csrc/' in doc and '.hip' in doc, '%s.py does not say which csrc files it binds' % m


def test_state_is_bound_once_in_base(modules):
    assert STATE <= set(defined(modules['_base']))
    stores = [n.id for n in ast.walk(modules['_base']) if isinstance(n, ast.Name) and n.id in STATE
              and isinstance(n.ctx, (ast.Store, ast.Del))]
    assert sorted(stores) == sorted(STATE), 'bound more than once in _base.py: %s' % stores
    for m in ORDER:
        for node in ast.walk(modules[m]):
            if isinstance(node, (ast.Global, ast.Nonlocal)):
                assert not STATE & set(node.names), '%s.py rebinds %s' % (m, node.names)
            if m != '_base':
                assert not (isinstance(node, ast.Name) and node.id in STATE), '%s.py names %s' % (m, node.id)
                assert not (isinstance(node, ast.alias) and node.name in STATE), '%s.py imports %s' % (m, node.name)


# how a read of ops._name, or an import from ops, can be spelled; the parse then tells code from comments and strings
MAYBE_PRIVATE = re.compile(r'\bops\s*\.\s*_|\bops\s+import\b')


def test_nobody_reads_a_private_name_off_ops():
    hits = []
    for top in ('tuch_amd', 'tests', 'tools'):
        for folder, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if not f.endswith('.py'):
                    continue
                path = os.path.join(folder, f)
                with open(path) as fh:
                    text = fh.read()
                if not MAYBE_PRIVATE.search(text):          # (nothing to find: not worth a parse)
                    continue
                for node in ast.walk(ast.parse(text, path)):
                    if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == 'ops' \
                            and node.attr.startswith('_'):
                        hits.append('%s:%d ops.%s' % (os.path.relpath(path, ROOT), node.lineno, node.attr))
                    # the same reach spelled as an import from the package itself
                    if isinstance(node, ast.ImportFrom) and node.module in ('tuch_amd.ops', 'ops'):
                        hits += ['%s:%d from %s import %s' % (os.path.relpath(path, ROOT), node.lineno, node.module, a.name)
                                 for a in node.names if a.name.startswith('_')]
    assert not hits, hits
