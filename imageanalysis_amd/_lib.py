"""ctypes loader for libiamx.so (the C ABI declared in include/iamx.h).

The product path has no CPU fallback: if the HIP library is missing, or a kernel is
asked to run without a GPU, this raises.  torch is imported first so that the HIP
runtime already mapped by torch (its bundled libamdhip64, soname libamdhip64.so.7) is
the one libiamx.so binds to -- one runtime per process, device pointers interchangeable.
"""
import contextlib
import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('IAMX_LIB') or os.path.join(_HERE, 'libiamx.so')   # IAMX_LIB: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'iamx.h')   # where csrc/iamx_common.h includes it from
_lib = None

c_void_p = ctypes.c_void_p      # callers wrap their device pointers in it


class IamxError(RuntimeError):
    pass


# the whole binding: a parameter with '*' or '[' is a pointer, every other type is one of these
_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'int64_t': ctypes.c_int64,
            'uint64_t': ctypes.c_uint64, 'double': ctypes.c_double, 'float': ctypes.c_float}
_RETURNS = dict(_SCALARS, **{'const char *': ctypes.c_char_p, 'void *': ctypes.c_void_p, 'void': None})


def _argtype(param, proto):
    if '(' in param or ')' in param:
        raise IamxError("iamx.h: %s: parameter '%s' (a function pointer?) has no ctypes rule" % (proto, param))
    if '*' in param or '[' in param:
        return ctypes.c_void_p
    words = [w for w in param.split() if w != 'const']
    if len(words) not in (1, 2) or words[0] not in _SCALARS:       # type, or type and name
        raise IamxError("iamx.h: %s: parameter '%s' has no ctypes rule" % (proto, param))
    return _SCALARS[words[0]]


def parse_header(text):
    """name -> (restype, argtypes) of every `<return type> iamx_<name>(<parameters>);` of a C header.
    Strict: a type outside the rules above, an iamx_ name in front of a '(' that is no such prototype
    and a name declared twice raise IamxError -- nothing is guessed or skipped."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    text = re.sub(r'extern\s*"C"\s*\{|^[ \t]*\}[ \t]*$', '', text, flags=re.M)
    table = {}
    for stmt in text.split(';'):
        stmt = ' '.join(stmt.split())
        m = re.fullmatch(r'([\w\s*]+?)\s*\b(iamx_\w+)\s*\((.*)\)', stmt)
        if not m:
            if re.search(r'\biamx_\w+\s*\(', stmt):
                raise IamxError("iamx.h: '%s' names an entry point but is not a prototype" % stmt)
            continue
        ret, name, params = re.sub(r'\s*\*\s*', ' *', m.group(1)).strip(), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise IamxError("iamx.h: %s: return type '%s' has no ctypes rule" % (name, ret))
        if name in table:
            raise IamxError("iamx.h: %s is declared twice" % name)
        params = [] if params == 'void' else [p.strip() for p in params.split(',')]
        table[name] = (_RETURNS[ret], [_argtype(p, name) for p in params])
    return table


def _signatures():
    if not os.path.isfile(HEADER_PATH):
        raise IamxError("%s not found: the ctypes bindings are derived from the C header" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# name -> (restype, argtypes): include/iamx.h, parsed once at import; the header is the only statement of the ABI
SIGNATURES = _signatures()


def lib():
    """Load libiamx.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (maps the HIP runtime first, see module docstring)
        if not os.path.exists(LIB_PATH):
            raise IamxError(
                "libiamx.so not found at %s -- build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` "
                "(imageanalysis_amd/csrc/build.sh); there is no CPU fallback" % LIB_PATH)
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)          # AttributeError if the ABI and the header drift apart
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().iamx_last_error()
        raise IamxError("%s failed (%d): %s" % (what or 'libiamx call', rc,
                                                msg.decode() if msg else '?'))


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise IamxError("no HIP device visible: the iamx hot path runs on an MI355X only "
                        "(no CPU fallback)")
    return torch.device('cuda', torch.cuda.current_device())


_held = threading.local()


def stream_ptr():
    held = getattr(_held, 'ptr', None)
    if held is not None:
        return held
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def hold_stream(fresh=False):
    """Inside the block stream_ptr() answers with the stream that was current on entry (per
    thread) instead of asking torch each time -- torch.cuda.current_stream() costs ~8 us, more
    than many of the kernels the TRF loop launches.  Code that switches streams inside (a graph
    capture) wraps its launches in hold_stream(fresh=True): the stream current THERE."""
    import torch
    prev = getattr(_held, 'ptr', None)
    if fresh or prev is None:
        _held.ptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        yield
    finally:
        _held.ptr = prev
