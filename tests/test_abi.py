"""The C-ABI shared library builds, loads, and exports every symbol the
public header declares (no GPU needed — hipcc cross-compiles and host-side
entry points run anywhere)."""
import ctypes
import os
import re

from chunkflow_amd.build import build, SO_PATH


def header_symbols():
    header = os.path.join(os.path.dirname(SO_PATH), '..', 'include',
                          'chunkflow_amd.h')
    with open(header) as f:
        text = f.read()
    return sorted(set(re.findall(r'\b(cfx_\w+)\s*\(', text)))


def test_build_and_symbols():
    path = build()
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert len(syms) >= 18
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, f'missing C-ABI symbols: {missing}'


def test_python_binding_symbol_list_matches_header():
    from chunkflow_amd.hip import SYMBOLS
    assert sorted(SYMBOLS) == header_symbols()


def _header_path():
    return os.path.join(os.path.dirname(SO_PATH), '..', 'include',
                        'chunkflow_amd.h')


def _kind(decl):
    """'ptr', 'int', 'long long', 'unsigned int', 'float' or 'void' of one
    parameter declaration or return type"""
    if '*' in decl or '[' in decl:
        return 'ptr'
    words = [w for w in decl.split() if w != 'const']
    for kind in ('unsigned int', 'long long', 'int', 'float', 'void'):
        n = len(kind.split())
        if ' '.join(words[:n]) == kind and len(words) <= n + 1:
            return kind
    raise AssertionError(f'unclassified declaration: {decl!r}')


def header_prototypes():
    """{name: (return kind, [parameter kinds])} of every prototype
    `ret cfx_name(params);` in the header"""
    with open(_header_path()) as f:
        text = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    protos = {}
    for ret, name, params in re.findall(
            r'([A-Za-z_][\w \t]*?[\s*]+)(cfx_\w+)\s*\(([^()]*)\)\s*;', text):
        params = ' '.join(params.split())
        kinds = [] if params == 'void' else \
            [_kind(p.strip()) for p in params.split(',')]
        assert name not in protos, name
        protos[name] = (_kind(ret.strip()), kinds)
    return protos


def test_python_binding_signatures_match_header():
    """Every argtypes / restype entry of hip.SIGNATURES is the kind the
    header declares at that position: an argument added to the header and
    forgotten in the binding, or a pointer declared as a C int, fails
    here and not on a GPU."""
    from chunkflow_amd.hip import SIGNATURES, SYMBOLS
    kind_of = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int',
               ctypes.c_longlong: 'long long', ctypes.c_uint: 'unsigned int',
               ctypes.c_float: 'float'}
    ret_of = {ctypes.c_int: 'int', ctypes.c_void_p: 'ptr',
              ctypes.c_char_p: 'ptr', None: 'void'}
    protos = header_prototypes()
    assert len(protos) == len(SYMBOLS) == len(set(SYMBOLS))
    assert sorted(protos) == sorted(SYMBOLS)
    for name, (ret, kinds) in protos.items():
        restype, argtypes = SIGNATURES[name]
        assert ret_of[restype] == ret, name
        assert [kind_of[a] for a in argtypes] == kinds, name


def test_loaded_library_carries_the_signatures():
    from chunkflow_amd.hip import SIGNATURES, load_library
    lib = load_library()
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == list(argtypes), name


def test_version_and_error_string():
    from chunkflow_amd.hip import load_library
    lib = load_library()
    assert lib.cfx_version() >= 1
    assert isinstance(lib.cfx_last_error(), bytes)
