"""ctypes binding of librfn_hip.so, derived from the C header the library was built from.

`make -C recurrent-flows-msc_amd/csrc` (see __graft_entry__.build) builds the library in-tree and copies
include/rfn_hip.h next to it.  That copy is the one declaration of the ABI on the Python side: SIGNATURES (name ->
argtypes), RESTYPES (name -> restype) and CONSTANTS (the header's integer `#define RFN_*` limits) are parsed from it,
and load() sets them on every entry point, so call sites pass plain Python numbers, None and addresses and ctypes
converts (and refuses a float where the header says int).  A second build of the package carries its own copy.  Only
the descriptor structs are written out here, because their fields are assigned by name; a host test
(tests/test_binding_host.py) holds them against the header's typedefs.

The library is the ONLY compute backend of this package: if it cannot be loaded, or a tensor is not a contiguous fp32
device tensor, the call raises — there is no CPU / eager fallback.
"""
import ctypes
import functools
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librfn_hip.so")
HEADER_PATH = os.path.join(_HERE, "rfn_hip.h")   # the build's copy of include/rfn_hip.h

ABI_VERSION = 2  # rfn_abi_version() of the library this binding matches (include/rfn_hip.h)


# ---- the descriptor structs of include/rfn_hip.h (same names; the layouts are part of the ABI)
class rfn_pack_desc(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("wpk", ctypes.c_void_p), ("Cout", ctypes.c_int), ("Cin", ctypes.c_int),
                ("ks", ctypes.c_int), ("mode", ctypes.c_int)]


class rfn_po_pack_desc(ctypes.Structure):
    _fields_ = [("w1", ctypes.c_void_p), ("w2", ctypes.c_void_p), ("w3", ctypes.c_void_p), ("dst", ctypes.c_void_p),
                ("Cin", ctypes.c_int), ("C", ctypes.c_int)]


class rfn_smallmap_pack_desc(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("packed", ctypes.c_void_p), ("Cout", ctypes.c_int), ("Cin", ctypes.c_int),
                ("H", ctypes.c_int), ("W", ctypes.c_int), ("transpose", ctypes.c_int), ("pad_", ctypes.c_int)]


class rfn_adam_entry(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("n", ctypes.c_long), ("step_offset", ctypes.c_int), ("flags", ctypes.c_int)]


class rfn_sheet_row(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("step", ctypes.c_long), ("kind", ctypes.c_int), ("count", ctypes.c_int)]


STRUCTS = {s.__name__: s for s in (rfn_pack_desc, rfn_po_pack_desc, rfn_smallmap_pack_desc, rfn_adam_entry,
                                   rfn_sheet_row)}

# ---- C type -> ctypes.  Values travel as their own type; every pointer travels as an address, whatever it points to.
_VALUES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
           "rfn_stream_t": ctypes.c_void_p}
_POINTEES = {"void", "int", "float", "long long"} | set(STRUCTS)
_RETURNS = {"int": ctypes.c_int, "long": ctypes.c_long, "const char*": ctypes.c_char_p}


def _ctype(decl, fn):
    """ctypes type of one parameter declaration, e.g. `const float* const* w1`; an unknown type is an error"""
    m = re.fullmatch(r"(.*[\s*])\w+", decl)
    ty = (m.group(1) if m else decl).replace("*", " * ").split()
    if "*" in ty:
        if " ".join(w for w in ty if w not in ("const", "*")) in _POINTEES:
            return ctypes.c_void_p
    elif " ".join(ty) in _VALUES:
        return _VALUES[" ".join(ty)]
    raise RuntimeError("%s: no ctypes mapping for the C type of `%s`" % (fn, decl))


def parse_header(text):
    """(SIGNATURES, RESTYPES, CONSTANTS) of the text of rfn_hip.h: every `<type> rfn_name(args);` and every
    `#define RFN_NAME <integer>`"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sigs, res = {}, {}
    for m in re.finditer(r"^([A-Za-z_][\w \t*]*?)\s*\b(rfn_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S | re.M):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        ret = " ".join(ret.replace("*", "* ").split()).replace(" *", "*")   # `const char *` -> `const char*`
        if ret not in _RETURNS:
            raise RuntimeError("%s: no ctypes mapping for the C return type `%s`" % (name, ret))
        res[name] = _RETURNS[ret]
        sigs[name] = [] if args in ("void", "") else [_ctype(a.strip(), name) for a in args.split(",")]
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(RFN_\w+)\s+(-?\d+)\s*$", text, flags=re.M)}
    return sigs, res, consts


_NOT_BUILT = ("%s not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C "
              "recurrent-flows-msc_amd/csrc`. There is no fallback path.")


@functools.lru_cache(maxsize=None)
def _declarations(path):
    if not os.path.exists(path):
        raise RuntimeError(_NOT_BUILT % ("rfn_hip.h (the build's copy of include/rfn_hip.h)", path))
    with open(path) as f:
        return parse_header(f.read())


_DERIVED = ("SIGNATURES", "RESTYPES", "CONSTANTS")


def __getattr__(name):   # lib.SIGNATURES, lib.RESTYPES, lib.CONSTANTS: read from the header copy at first use
    if name in _DERIVED:
        return _declarations(HEADER_PATH)[_DERIVED.index(name)]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


_lib = None


def load():
    """Load librfn_hip.so (once) and set every entry point's argtypes / restype from the header copy beside it.  Raises
    RuntimeError if the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(_NOT_BUILT % ("librfn_hip.so", LIB_PATH))
    lib = ctypes.CDLL(LIB_PATH)
    lib.rfn_abi_version.restype = ctypes.c_int
    if lib.rfn_abi_version() != ABI_VERSION:
        raise RuntimeError("%s has ABI version %d, this package needs %d: rebuild the library (`make -C "
                           "recurrent-flows-msc_amd/csrc`)" % (LIB_PATH, lib.rfn_abi_version(), ABI_VERSION))
    sigs, res, _ = _declarations(HEADER_PATH)
    for name, argtypes in sigs.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.argtypes = argtypes
        fn.restype = res[name]
    _lib = lib
    return lib


# Optional in-process kernel timing (bench.py): when PROFILE is a list, every call is bracketed by HIP events recorded
# on the stream the kernel is launched on, and (name, meta, start_event, end_event) is appended.
PROFILE = None


def call(name, *args, meta=None):
    """Invoke an int-returning entry point on the current torch stream; raise on a non-zero code."""
    lib = load()
    cur = torch.cuda.current_stream()
    stream = cur.cuda_stream
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        rc = getattr(lib, name)(*args, stream)
        e1.record(cur)
        PROFILE.append((name, meta, e0, e1))
    else:
        rc = getattr(lib, name)(*args, stream)
    if rc != 0:
        raise RuntimeError("%s failed (code %d): %s" % (name, rc, lib.rfn_last_error().decode()))


def ptr_array(tensors, name="tensor"):
    """host array of device pointers (for the grouped entry points); the caller keeps the tensors alive"""
    arr = (ctypes.c_void_p * len(tensors))(*[dev(t, name, check_contiguous=False).value for t in tensors])
    return arr


def dev(t, name="tensor", check_contiguous=True):
    """Validate a device tensor for the kernels and return its pointer: fp32, on the GPU, contiguous (frames() checks
    the per-frame layout of channel-slice views itself and passes check_contiguous=False)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("rfn_hip kernels need device tensors; %s is on %s (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.float32:
        raise RuntimeError("rfn_hip kernels are fp32; %s is %s" % (name, t.dtype))
    if check_contiguous and not t.is_contiguous():
        raise RuntimeError("rfn_hip kernels need dense tensors; %s has shape %s stride %s" %
                           (name, tuple(t.shape), tuple(t.stride())))
    return ctypes.c_void_p(t.data_ptr())


def frames(t, name="tensor"):
    """(pointer, frame stride) of an [N,C,H,W] (or [N,C,HW]) tensor whose per-frame block is dense."""
    p = dev(t, name, check_contiguous=False)
    shape, stride = t.shape, t.stride()
    exp = 1
    for d in range(t.dim() - 1, 0, -1):
        if shape[d] != 1 and stride[d] != exp:
            raise RuntimeError("%s: per-frame layout must be dense NCHW, got shape %s stride %s" %
                               (name, tuple(shape), tuple(stride)))
        exp *= shape[d]
    ns = stride[0] if shape[0] > 1 else exp
    return p, int(ns)
