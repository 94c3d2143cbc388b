"""ctypes binding of libtdr_hip.so, derived at import from include/tdr.h.

The header is the only written copy of the C ABI: the `Tdr...` Structure classes, SIGNATURES and ABI_VERSION below are
computed from it, so a new entry point is a prototype there plus its wrapper (kernels.py).  The parser reads the header's
own subset of C and is strict: a statement or a type it does not know raises at import and names the text, nothing is
guessed or skipped -- a binding that loads is one whose every argument was understood.

The product path has NO fallback: if the shared library is missing or a call
fails, this module raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C textualdegremoval_amd/csrc`.
"""
import ctypes as C
import os
import re

# torch bundles its own libamdhip64; it must be the HIP runtime already resident
# when libtdr_hip.so is dlopen'ed so both share one runtime (one device context,
# one set of streams).  Loading in the other order gives two runtimes.
import torch  # noqa: F401  (import order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TDR_LIB_PATH', os.path.join(_HERE, 'libtdr_hip.so'))   # override: profiling probe builds
HEADER_PATH = os.path.normpath(os.path.join(_HERE, os.pardir, 'include', 'tdr.h'))  # as csrc/ includes it: ../../include/tdr.h

c_fp = C.c_void_p      # device pointers travel as integers
i32, i64, f32 = C.c_int, C.c_int64, C.c_float


class TdrError(RuntimeError):
    pass


_SCALARS = {'int': i32, 'int64_t': i64, 'float': f32}
_RETURNS = dict(_SCALARS, **{'const char *': C.c_char_p})
_POINTEES = {'void', 'char', 'int', 'unsigned', 'uint8_t', 'int64_t', 'float', 'double'}    # every such pointer is a c_void_p
_PY_FIELD = {'in': 'inp'}      # `in` is a Python keyword
# A parameter that points to a struct the header defines is POINTER(struct): Python fills the struct on the host and passes it
# with byref.  These point to device memory instead and travel as integers, like every other device pointer.
_DEVICE_STRUCT_PARAMS = {       # (struct, parameter name): why
    ('TdrPackJob', 'jobs_dev'): 'the job array the caller copied to the device (tdr_pack_weights_multi)',
    ('TdrStepGuard', 'guard'): "the train step's verdict lives in device memory, so captured graphs replay it",
}

_NOISE = re.compile(r'/\*.*?\*/|//[^\n]*|^#ifdef __cplusplus$.*?^#endif$', re.S | re.M)   # comments; the extern "C" brackets
_STATEMENT = re.compile(
    r'\s*(?:typedef\s+struct\s+(?P<tag>\w+)\s*\{(?P<body>[^{}]*)\}\s*(?P<alias>\w+)'
    r'|typedef\s+struct\s+(?P<otag>\w+)\s+(?P<oalias>\w+)'
    r'|(?P<ret>(?:const\s+)?\w+(?:\s*\*\s*|\s+))(?P<fn>\w+)\s*\((?P<params>[^()]*)\))\s*;')
_DECLARATION = re.compile(r'(?:const\s+)?(\w+)\b\s*(.*)', re.S)           # base type, then the comma-separated declarators
_DECLARATOR = re.compile(r'((?:\*\s*(?:const\b\s*)?)*)(\w+)')            # `*`s (each may be const), then the name


def _declaration(text, structs, opaque, is_param):
    """One C declaration (`int N, Cin`, `const void *w3, *w4`, `const float* const* src`) -> [(name, ctype)]."""
    text = text.strip()
    m = _DECLARATION.fullmatch(text)
    base, declarators = m.groups() if m else (None, '')
    out = []
    for d in declarators.split(','):
        m = _DECLARATOR.fullmatch(d.strip())
        if not m:
            raise TdrError(f'tdr.h: cannot parse the declaration {text!r}')
        stars, name = m.group(1).count('*'), m.group(2)
        if not stars and base in _SCALARS:
            t = _SCALARS[base]
        elif stars == 1 and is_param and base in structs and (base, name) not in _DEVICE_STRUCT_PARAMS:
            t = C.POINTER(structs[base])
        elif stars and (base in _POINTEES or base in structs or base in opaque):
            t = c_fp
        else:
            raise TdrError(f'tdr.h: unknown type in the declaration {text!r}')
        out.append((name, t))
    return out


def parse(text):
    """The text of a header in tdr.h's subset of C -> ({struct name: Structure class}, {function: (restype, [argtypes])})."""
    text = re.sub(r'^\s*#.*$', ' ', _NOISE.sub(' ', text), flags=re.M).strip()
    structs, opaque, signatures = {}, set(), {}
    pos = 0
    while pos < len(text):
        m = _STATEMENT.match(text, pos)
        if not m:
            raise TdrError(f'tdr.h: not a prototype, a struct typedef or an opaque typedef: {text[pos:].split(";")[0].strip()!r}')
        pos = m.end()
        if m['fn']:
            ret = ' '.join(m['ret'].replace('*', ' * ').split())
            if ret not in _RETURNS:
                raise TdrError(f'tdr.h: unknown return type {ret!r} of {m["fn"]}')
            params = [] if m['params'].strip() == 'void' else m['params'].split(',')
            signatures[m['fn']] = (_RETURNS[ret], [_declaration(p, structs, opaque, True)[0][1] for p in params])
        elif (m['tag'] or m['otag']) != (m['alias'] or m['oalias']):
            raise TdrError(f'tdr.h: struct tag and typedef name differ: {m.group().strip()!r}')
        elif m['otag']:
            opaque.add(m['otag'])
        else:
            fields = [(_PY_FIELD.get(n, n), t) for decl in m['body'].split(';') if decl.strip()
                      for n, t in _declaration(decl, structs, opaque, False)]
            structs[m['tag']] = type(m['tag'], (C.Structure,), {'_fields_': fields})
    return structs, signatures


def read_header(path):
    """-> (ABI version, structs, signatures) of the header at `path`."""
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise TdrError(f'cannot read the C-ABI header {path}: {e} -- the binding is derived from it') from e
    version = re.search(r'^#define\s+TDR_ABI_VERSION\s+(\d+)\s*$', text, re.M)
    if not version:
        raise TdrError(f'{path} has no #define TDR_ABI_VERSION')
    return (int(version.group(1)),) + parse(text)


# ABI_VERSION: csrc/tdr_error.cpp returns the same #define; SIGNATURES: name -> (restype, argtypes), every symbol the header declares;
# every struct of the header is a module attribute (TdrConvDesc, TdrPackJob, ...), fields in header order
ABI_VERSION, _STRUCTS, SIGNATURES = read_header(HEADER_PATH)
globals().update(_STRUCTS)

_lib = None


def load():
    """Load libtdr_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TdrError(f'{LIB_PATH} is missing: build it first (python -c "import __graft_entry__ as g; g.build()"). '
                       'There is no CPU fallback on the product path.')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    have = lib.tdr_version()
    if have != ABI_VERSION:
        raise TdrError(f'{LIB_PATH} exports C-ABI version {have}, this package binds version {ABI_VERSION}: a stale build would be '
                       'called with shifted arguments -- rebuild it (python -c "import __graft_entry__ as g; g.build()")')
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().tdr_last_error().decode('utf-8', 'replace')
        raise TdrError(f'{what} failed (code {rc}): {msg}')
