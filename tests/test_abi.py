"""CPU: the C-ABI library builds, loads, and exports every symbol include/tuch_amd.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from tuch_amd import _C, _build
    _build.build()
    lib = ctypes.CDLL(_C.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'tuch_amd.h')).read()
    declared = sorted(set(re.findall(r'\b(tuch_[a-z0-9_]+)\s*\(', header)))
    assert declared, 'no declarations found'
    for name in declared:
        assert hasattr(lib, name), 'missing symbol ' + name
    # the Python binding and the header agree
    assert set(_C.exported_symbols()) <= set(declared), set(_C.exported_symbols()) - set(declared)
    assert _C.lib().tuch_abi_version() >= 1


_KINDS = {'int': 'int', 'int32_t': 'int', 'unsigned': 'unsigned', 'unsigned int': 'unsigned', 'uint32_t': 'unsigned',
          'float': 'float', 'size_t': 'size_t', 'void': 'void'}
_CTYPES = {ctypes.c_int: 'int', ctypes.c_uint: 'unsigned', ctypes.c_float: 'float', ctypes.c_size_t: 'size_t',
           ctypes.c_void_p: 'pointer', ctypes.c_char_p: 'pointer', None: 'void'}


def _c_kind(text):
    """The kind of a C parameter or return type: 'pointer', or what _KINDS calls its type (the text itself otherwise)."""
    if '*' in text or '[' in text:
        return 'pointer'
    words = [w for w in text.split() if w != 'const']
    if len(words) > 1 and words[-1] not in _KINDS:      # (the parameter's name)
        words.pop()
    return _KINDS.get(' '.join(words), ' '.join(words))


def _ctypes_kind(t):
    return 'pointer' if isinstance(t, type) and issubclass(t, ctypes._Pointer) else _CTYPES[t]


def test_binding_and_header_agree_by_position():
    """Every entry of _C._SIGNATURES against the prototype include/tuch_amd.h declares under that name: the return kind, the
    number of parameters and the kind of each (pointer, int, unsigned, float, size_t), position by position."""
    from tuch_amd import _C
    header = open(os.path.join(ROOT, 'include', 'tuch_amd.h')).read()
    header = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)
    header = re.sub(r'//[^\n]*|^\s*#[^\n]*', ' ', header, flags=re.M)
    prototypes = {}
    for ret, name, params in re.findall(r'([\w \t*]+?)\b(tuch_\w+)\s*\(([^()]*)\)\s*;', header):
        params = [] if params.strip() in ('', 'void') else params.split(',')
        prototypes[name] = (_c_kind(ret), [_c_kind(p) for p in params])
    assert len(prototypes) > 100
    unbound = sorted(set(_C._SIGNATURES) - set(prototypes))
    assert not unbound, 'bound but not declared: %s' % unbound
    for name, (res, args) in _C._SIGNATURES.items():
        bound = (_ctypes_kind(res), [_ctypes_kind(a) for a in args])
        assert bound == prototypes[name], '%s: the binding has %s, the header %s' % (name, bound, prototypes[name])


def test_error_reporting_without_gpu():
    from tuch_amd import _C
    L = _C.lib()
    rc = L.tuch_winding_numbers(None, None, 1, 1, 1, None, None, 0.99, None, 0, None)
    assert rc != 0
    assert b'null pointer' in L.tuch_last_error()
    assert L.tuch_geomask_words(6890) == 108
    assert L.tuch_winding_workspace_bytes(64, 6890, 13776) > 0
