"""ctypes binding of ``libraft_hip.so`` (C ABI: include/raft_hip.h).

The prototypes and the integer constants are read from the header when this module is imported (``header_signatures``,
``header_constants``); only the struct mirrors are written out here, because Python code names their fields.

There is no CPU fallback: if the shared library cannot be loaded (and cannot be built
because hipcc is absent) importing the device path raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

_LOCK = threading.Lock()
_LIB = None
ABI_VERSION = 222     # include/raft_hip.h RAFT_HIP_VERSION: the ctypes mirrors below describe THIS revision of the structs

_COMMENT = re.compile(r'/\*.*?\*/|//[^\n]*', re.S)


def header_constants(text: str) -> dict:
    """``{name: value}`` of the integer ``#define``s and of the enumerators with a written value in the header ``text``."""
    text = _COMMENT.sub(' ', text)
    out = {m[1]: int(m[2]) for m in re.finditer(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$', text, re.M)}
    for body in re.findall(r'\benum\s*\{([^{}]*)\}', text):
        out.update((m[1], int(m[2])) for m in re.finditer(r'(\w+)\s*=\s*(-?\d+)', body))
    return out


with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'raft_hip.h')) as _f:
    _HEADER = _f.read()
_CONSTANTS = header_constants(_HEADER)


class ConvWeights(C.Structure):
    _fields_ = [('wp', C.c_void_p), ('bias', C.c_void_p), ('npad', C.c_int)]


class BasicUpdateWeights(C.Structure):
    _fields_ = [(n, ConvWeights) for n in (
        'convc1', 'convc2', 'convf1', 'convf2', 'conv',
        'gru_zr1', 'gru_q1', 'gru_zr2', 'gru_q2',
        'fh1_mask0', 'fh2', 'mask2', 'gru_ctx1', 'gru_ctx2',
        'convc2_w', 'convf2_w', 'conv_w', 'fh1_mask0_w',
        'gru_zr1_w', 'gru_q1_w', 'gru_zr2_w', 'gru_q2_w', 'fh1_w',
        'gru_zr1_w4', 'gru_q1_w4', 'gru_zr2_w4', 'gru_q2_w4', 'convc1_f', 'gru_ctx1_w4', 'gru_ctx2_w4',
        'convc2_w44', 'conv_w44', 'fh1_mask0_w44', 'fh1_w44', 'convf2_w44')]


class SmallUpdateWeights(C.Structure):
    _fields_ = [(n, ConvWeights) for n in (
        'convc1', 'convf1', 'convf2', 'conv', 'gru_zr', 'gru_q', 'fh1', 'fh2',
        'conv_w', 'gru_zr_w', 'gru_q_w', 'fh1_w')]


class EncoderWeights(C.Structure):
    _fields_ = [('c0', C.c_int), ('c1', C.c_int), ('c2', C.c_int), ('c3', C.c_int), ('cout', C.c_int),
                ('norm', C.c_int), ('conv1', ConvWeights), ('block', (ConvWeights * 3) * 6), ('conv2', ConvWeights),
                ('in_gamma', C.c_void_p * 19), ('in_beta', C.c_void_p * 19), ('block_w', (ConvWeights * 2) * 6), ('block_w44', (ConvWeights * 2) * 6)]


NORM_NONE, NORM_INSTANCE, NORM_FOLDED = (_CONSTANTS['RAFT_NORM_' + n] for n in ('NONE', 'INSTANCE', 'FOLDED'))


class State(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        'net', 'x', 'corr', 'coords1', 'flow', 'delta', 'mask', 'ws', 'ctx')]


TILE_MAX_PER_AXIS = _CONSTANTS['RAFT_TILE_MAX_PER_AXIS']
TILE_MAX_TAPS = _CONSTANTS['RAFT_TILE_MAX_TAPS']


class TileOrigins(C.Structure):
    """``RaftTileOrigins``: the tile grid of one frame size, passed by value."""
    _fields_ = [('ny', C.c_int32), ('nx', C.c_int32), ('oy', C.c_int32 * TILE_MAX_PER_AXIS), ('ox', C.c_int32 * TILE_MAX_PER_AXIS)]


class AugmentParams(C.Structure):
    """``RaftAugmentParams``: one sample's record of tf_raft_amd/augment.py (include/raft_hip.h has the field notes)."""
    _fields_ = [('inv_fx', C.c_double), ('inv_fy', C.c_double), ('fx', C.c_double), ('fy', C.c_double),
                ('hue', C.c_double * 2), ('sat', C.c_double * 2), ('val', C.c_double * 2),
                ('alpha', C.c_float * 2), ('beta', C.c_float * 2),
                ('W1', C.c_int32), ('H1', C.c_int32), ('x0', C.c_int32), ('y0', C.c_int32), ('resize', C.c_int32),
                ('flip_h', C.c_int32), ('flip_v', C.c_int32), ('color', C.c_int32 * 2), ('n_rect', C.c_int32),
                ('rect', (C.c_int32 * 4) * 2)]


class ViewParams(C.Structure):
    """``RaftViewParams``: one slice's student view (tf_raft_amd/augment.py ``StudentView``; include/raft_hip.h has the field notes)."""
    _fields_ = [('m', C.c_float * 4), ('o', C.c_float * 2), ('inv', C.c_float * 4), ('gain', C.c_float * 3), ('bias', C.c_float * 3),
                ('colour', C.c_int32)]


AUGMENT_SUM_BLOCKS = _CONSTANTS['RAFT_AUGMENT_SUM_BLOCKS']

_SCALARS = {'int': C.c_int, 'float': C.c_float, 'double': C.c_double, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64,
            'uint32_t': C.c_uint32, 'size_t': C.c_size_t}
# Structs that cross the ABI by value or as HOST pointers.  RaftAugmentParams and RaftViewParams are absent on purpose: their
# records lie in device memory, so a pointer to them travels as void* like every other device pointer.
_STRUCTS = {'raft_conv_weights': ConvWeights, 'raft_basic_update_weights': BasicUpdateWeights,
            'raft_small_update_weights': SmallUpdateWeights, 'raft_encoder_weights': EncoderWeights, 'raft_state': State,
            'RaftTileOrigins': TileOrigins}


def _ctype(text: str, decl: str):
    """The ctypes type of one C type of the header's closed vocabulary; ``decl`` is quoted when there is none."""
    base, stars = ' '.join(w for w in text.replace('*', ' ').split() if w != 'const'), text.count('*')
    if stars >= 2:                              # host arrays of pointers, the out-parameter of raft_loop_ctx_create
        return C.POINTER(C.c_void_p)
    if stars == 1:
        if base == 'char':
            return C.c_char_p
        if base == 'int64_t':                   # host arrays: level offsets, element counts
            return C.POINTER(C.c_int64)
        return C.POINTER(_STRUCTS[base]) if base in _STRUCTS else C.c_void_p
    if base in _SCALARS:
        return _SCALARS[base]
    if base in _STRUCTS:
        return _STRUCTS[base]
    raise ValueError(f'include/raft_hip.h: no ctypes type for {text.strip()!r} in the declaration {decl!r}')


_TYPED_NAME = re.compile(r'\s*(.*?[\s\*])(\w+)\s*')       # "const float *x", "int64_t raft_f": a type, then a name


def header_signatures(text: str) -> dict:
    """``{name: (restype, [argtypes])}`` of every prototype in the header ``text``, in declaration order.  A declaration that
    is no typedef, no enum and no prototype of known types raises ``ValueError``: nothing is skipped or guessed."""
    text = re.sub(r'#ifdef __cplusplus.*?#endif', ' ', _COMMENT.sub(' ', text), flags=re.S)      # the extern "C" braces
    text = re.sub(r'^[ \t]*#[^\n]*', ' ', text, flags=re.M)
    text = re.sub(r'\{[^{}]*\}', ' ', text)                                                      # struct and enum bodies
    sigs = {}
    for decl in text.split(';'):
        decl = ' '.join(decl.split())
        if not decl or decl.split()[0] in ('typedef', 'enum'):
            continue
        head, _, params = decl.partition('(')
        params = [] if params[:-1].strip() == 'void' else params[:-1].split(',')
        parts = [_TYPED_NAME.fullmatch(p) for p in [head] + params]       # "return type, name" reads like a parameter
        if not decl.endswith(')') or decl.count('(') != 1 or decl.count(')') != 1 or None in parts:
            raise ValueError(f'include/raft_hip.h: cannot split the declaration {decl!r}')
        res, *args = [_ctype(p[1], decl) for p in parts]
        sigs[parts[0][2]] = (res, args)
    return sigs


_SIGNATURES = header_signatures(_HEADER)

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib', 'libraft_hip.so')


def load_library():
    """Load and type the library.  When hipcc is available the build is refreshed first (a digest of sources + flags
    makes that a no-op for an up-to-date .so), so a stale library never meets newer struct mirrors.  When the refresh
    fails (no hipcc, read-only tree, compile error) an existing .so is used only if its build stamp (lib/build.sha256,
    shipped beside it) matches the sources on disk; a .so WITHOUT a stamp cannot be verified and is refused unless
    RAFT_ALLOW_UNVERIFIED_LIB=1; a stamp that names other sources is refused unless RAFT_ALLOW_STALE_LIB=1.
    Either way ``raft_version()`` must equal ``ABI_VERSION``."""
    global _LIB
    if _LIB is not None:                       # fast path: no lock once loaded
        return _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = library_path()
        from . import build as _build
        try:
            _build.build_library(verbose=False)
        except Exception as exc:   # noqa: BLE001
            if not os.path.exists(path):
                raise RuntimeError(
                    f'libraft_hip.so is missing at {path} and could not be built ({exc}); '
                    'the RAFT device path has no CPU fallback') from exc
            # A library exists but the refresh failed (compile error, no hipcc, read-only tree).  It may only be used
            # if it was built from exactly these sources; anything else would run old kernels under new tests.
            built = _build.built_digest()
            unknown = built is None                          # prebuilt .so without its stamp: nothing to compare
            stale = (not unknown) and built != _build.source_digest()
            if stale and os.environ.get('RAFT_ALLOW_STALE_LIB') != '1':
                raise RuntimeError(
                    f'{path} was built from different sources than the ones on disk and rebuilding failed: {exc}.  '
                    'Fix the build, or set RAFT_ALLOW_STALE_LIB=1 to load the old library knowingly') from exc
            if unknown and '1' not in (os.environ.get('RAFT_ALLOW_UNVERIFIED_LIB'), os.environ.get('RAFT_ALLOW_STALE_LIB')):
                raise RuntimeError(
                    f'{path} carries no build stamp (lib/build.sha256), so it cannot be checked against the sources on disk, and '
                    f'rebuilding failed: {exc}.  Fix the build, or set RAFT_ALLOW_UNVERIFIED_LIB=1 to load it knowingly') from exc
            import warnings
            warnings.warn(f'libraft_hip.so could not be refreshed ({exc}); loading the existing '
                          f'{"STALE " if stale else ("UNVERIFIED (no build stamp) " if unknown else "up-to-date ")}library at {path}',
                          RuntimeWarning, stacklevel=2)
        try:
            lib = C.CDLL(path)
        except OSError as exc:
            raise RuntimeError(f'cannot load {path}: {exc}; the RAFT device path has no CPU fallback') from exc
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError => symbol missing: fail loudly
            fn.restype = res
            fn.argtypes = args
        if lib.raft_augment_params_bytes() != C.sizeof(AugmentParams):
            raise RuntimeError(f'{path}: RaftAugmentParams is {lib.raft_augment_params_bytes()} bytes, its mirror {C.sizeof(AugmentParams)}')
        if lib.raft_view_params_bytes() != C.sizeof(ViewParams):
            raise RuntimeError(f'{path}: RaftViewParams is {lib.raft_view_params_bytes()} bytes, its mirror {C.sizeof(ViewParams)}')
        if lib.raft_version() != ABI_VERSION:
            raise RuntimeError(f'{path} reports ABI {lib.raft_version()}, this binding mirrors ABI {ABI_VERSION}: '
                               'rebuild the library (python -m tf_raft_amd.build --force)')
        _LIB = lib
        return lib


def set_option(name: str, value) -> None:
    """``raft_set_option``: ``value`` None = load-time (environment) state, '' = built-in default."""
    v = None if value is None else str(value).encode()
    check(load_library().raft_set_option(name.encode(), v), f'set_option {name}')


class thread_concurrency:
    """``with thread_concurrency(n):`` -- ``raft_set_thread_concurrency`` for the enclosed launches of the calling thread (n
    independent launch sequences share the device: shapes for CU-time instead of latency), restored on exit."""

    def __init__(self, n: int):
        self.n, self.prev = int(n), 1

    def __enter__(self):
        self.prev = load_library().raft_set_thread_concurrency(self.n)
        return self

    def __exit__(self, *exc):
        load_library().raft_set_thread_concurrency(self.prev)
        return False


def get_option(name: str) -> str:
    buf = C.create_string_buffer(256)
    check(load_library().raft_get_option(name.encode(), buf, 256), f'get_option {name}')
    return buf.value.decode()


def check(rc: int, what: str = '') -> None:
    """Raise on a nonzero return code: ValueError for argument errors, RuntimeError for HIP errors."""
    if rc == 0:
        return
    msg = load_library().raft_error_string(rc).decode()
    text = f'{what}: {msg} (rc={rc})' if what else f'{msg} (rc={rc})'
    if rc < 0:
        raise ValueError(text)
    raise RuntimeError(text)
