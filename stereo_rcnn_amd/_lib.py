"""ctypes binding of libsrcnn_hip.so (the C-ABI drop-in boundary, include/srcnn_hip.h).

The reference binds its native ops with cffi (`torch.utils.ffi`,
lib/model/nms/_ext/nms/__init__.py:2-15); cffi is not in this image, ctypes gives the
same contract.  There is NO fallback: if the HIP library is missing or fails to load,
importing any operator raises (the product path never routes through the CPU oracle).

Nothing of the header is written a second time here: at import `parse_header` reads include/srcnn_hip.h and gives this module
  * every `#define SRCNN_<NAME> <integer>` as the attribute <NAME> (FMT_F32, REC_COLS, ERR_ARG, KITTI_MAX_DET, ...),
  * one ctypes.Structure per `typedef struct` (srcnn_conv_fwd_f16x3_desc -> ConvFwdF16x3Desc), pointer fields c_void_p,
  * `_SIGNATURES` = {name: (restype, [argtypes])} over every SRCNN_API declaration.
Type rule: scalars by C type; a pointer to a declared struct is POINTER(Struct); srcnn_stream_t and every other pointer is
c_void_p (device memory: callers pass data_ptr()); a non-struct pointer that the HOST reads or writes is POINTER(pointee) --
the arguments the header names *_host, and those `_HOST_ARRAYS` lists.  What the parser does not understand raises with its text.
"""
import collections
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRCNN_LIB_PATH") or os.path.join(_HERE, "libsrcnn_hip.so")   # override: A/B builds of the library (dev)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "srcnn_hip.h")            # where csrc/build.py takes it from

c_int, c_float, c_double, c_void_p, c_size_t = (ctypes.c_int, ctypes.c_float, ctypes.c_double,
                                                ctypes.c_void_p, ctypes.c_size_t)

# Host arrays and out-parameters whose header names do not end in _host (renaming them would touch the header).
_HOST_ARRAYS = {
    "srcnn_rpn_score_levels": ("heads", "level_hw"),
    "srcnn_rpn_score_parts": ("parts", "nparts", "plane_floats", "level_hw"),
    "srcnn_proposal_workspace_layout": ("offsets",),
    "srcnn_dense_align_workspace_layout": ("offsets",),
    "srcnn_stream_create": ("stream",),
    "srcnn_stream_create_cu_mask": ("mask", "stream"),
    "srcnn_prof_read": ("conv_ms", "conv_flops", "conv_launches"),
    "srcnn_prof_read_launches": ("ms",),
}

# base type -> (ctype, or None for void; pointer levels the name itself carries); parse_header adds the header's typedefs
_BASE_TYPES = {"void": (None, 0), "int": (c_int, 0), "unsigned": (ctypes.c_uint, 0), "unsigned int": (ctypes.c_uint, 0),
               "long long": (ctypes.c_longlong, 0), "float": (c_float, 0), "double": (c_double, 0), "size_t": (c_size_t, 0),
               "char": (ctypes.c_char, 0), "signed char": (ctypes.c_byte, 0), "unsigned char": (ctypes.c_ubyte, 0)}
_DECLARATOR = r"\s*((?:\*\s*)*)([A-Za-z_]\w*)\s*(?:\[\s*(\d+)\s*\])?\s*"
_STATEMENT = r"\s*(?:typedef\s+struct\s+\w*\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)|(?P<decl>[^;{}]+?))\s*;"

Header = collections.namedtuple("Header", "constants structs signatures")


def _match(pattern, text, where, match=re.fullmatch):
    m = match(pattern, text, flags=re.S)
    if not m:
        raise ValueError("declaration does not split: %s" % where)
    return m


def _declarators(decl, types, where):
    """'const float *const *x, *y[2]' -> [(name, ctype of the base or None for void, pointer depth, array length or 0), ...]."""
    first, *rest = re.sub(r"\bconst\b", " ", decl).split(",")
    m = _match(r"\s*(\w+(?:\s+\w+)*?)\b" + _DECLARATOR, first, where)
    base = " ".join(m.group(1).split())
    if base not in types:
        raise ValueError("unknown base type %r: %s" % (base, where))
    ctype, depth = types[base]
    return [(name, ctype, depth + stars.count("*"), int(n or 0))
            for stars, name, n in [m.groups()[1:]] + [_match(_DECLARATOR, r, where).groups() for r in rest]]


def _ctype(ctype, depth, host, where):
    """The module docstring's type rule for one argument or return value."""
    if depth == 1 and isinstance(ctype, type) and issubclass(ctype, ctypes.Structure):
        return ctypes.POINTER(ctype)
    if host:
        if depth == 0 or (depth == 1 and ctype is None):
            raise ValueError("a host array must be a pointer to a sized type: %s" % where)
        return ctypes.POINTER(ctype if depth == 1 else c_void_p)
    if depth:
        return c_void_p
    if ctype is None:
        raise ValueError("a value cannot be void: %s" % where)
    return ctype


def parse_header(text, host_arrays=None):
    """What a header text declares -> Header(constants {NAME: int}, SRCNN_ stripped; structs {C name: ctypes.Structure};
    signatures {name: (restype, [argtypes])}).  host_arrays: {function: arguments typed as host arrays without a _host suffix}."""
    host_arrays = {k: list(v) for k, v in (host_arrays or {}).items()}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, structs, signatures = {}, collections.OrderedDict(), collections.OrderedDict()
    types = dict(_BASE_TYPES)

    def fresh(name, where):
        if name in constants or name in types or name in signatures:
            raise ValueError("duplicate name %r: %s" % (name, where))
        return name

    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+SRCNN_(\w+)[ \t]+(\(?[ \t]*-?\d.*?)[ \t]*$", text, flags=re.M):
        where = "#define SRCNN_%s %s" % (name, value)
        m = re.fullmatch(r"\(\s*(-?\w+)\s*\)|(-?\w+)", value)
        if not m or not re.fullmatch(r"-?(0[xX][0-9a-fA-F]+|\d+)", m.group(1) or m.group(2)):
            raise ValueError("not an integer: %s" % where)
        constants[fresh(name, where)] = int(m.group(1) or m.group(2), 0)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*$", " ", text, flags=re.S | re.M)   # extern "C" { / }
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)

    pos = 0
    while text[pos:].strip():
        m = _match(_STATEMENT, text[pos:], " ".join(text[pos:pos + 200].split()), re.match)
        pos += m.end()
        where = " ".join(m.group(0).split())
        if m.group("struct"):
            cname = fresh(m.group("struct"), where)
            *members, tail = m.group("body").split(";")
            fields = [(name, c_void_p if depth else _ctype(ctype, 0, False, where), n)
                      for s in members for name, ctype, depth, n in _declarators(s, types, "%s; in struct %s" % (" ".join(s.split()), cname))]
            if tail.strip() or len({f[0] for f in fields}) != len(fields):
                raise ValueError("declaration does not split: %s" % where)
            pyname = "".join(p.capitalize() for p in re.sub(r"^srcnn_", "", cname).split("_"))
            structs[cname] = type(pyname, (ctypes.Structure,), {"_fields_": [(name, t * n if n else t) for name, t, n in fields],
                                                                "__doc__": "struct %s (include/srcnn_hip.h)." % cname})
            types[cname] = (structs[cname], 0)
            continue
        handle = re.fullmatch(r"typedef\s+void\s*\*\s*(\w+)", m.group("decl"))
        if handle:                                  # srcnn_stream_t: void with one pointer level of its own
            types[fresh(handle.group(1), where)] = (None, 1)
            continue
        fn = _match(r"SRCNN_API\s+([^(),]+)\((.*)\)", m.group("decl"), where)
        (name, ctype, depth, n), = _declarators(fn.group(1), types, where)
        fresh(name, where)
        if (ctype, depth) == (ctypes.c_char, 1):
            restype = ctypes.c_char_p
        else:
            restype = None if (ctype, depth) == (None, 0) else _ctype(ctype, depth, False, where)
        listed = host_arrays.pop(name, [])
        argtypes = []
        for a in ([] if fn.group(2).strip() == "void" else fn.group(2).split(",")):
            (aname, ctype, depth, an), = _declarators(a, types, where)
            n += an
            host = aname in listed or aname.endswith("_host")
            if aname in listed:
                listed.remove(aname)
            argtypes.append(_ctype(ctype, depth, host, "%s in %s" % (" ".join(a.split()), where)))
        if n:
            raise ValueError("declaration does not split (an array in a signature): %s" % where)
        if listed:
            raise ValueError("the host-array table names %s, which is no argument of: %s" % (", ".join(listed), where))
        signatures[name] = (restype, argtypes)
    if host_arrays:
        raise ValueError("the host-array table names functions the header lacks: %s" % ", ".join(sorted(host_arrays)))
    return Header(constants, structs, signatures)


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError("include/srcnn_hip.h not found at %s: the ctypes binding is derived from it" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return parse_header(f.read(), _HOST_ARRAYS)


HEADER = _read_header()
globals().update(HEADER.constants)                                      # FMT_F32, REC_COLS, LOSS_ROWS_PER_WG, PREP_CONV, ...
globals().update((s.__name__, s) for s in HEADER.structs.values())      # ConvDesc, ConvBwdDesc, KittiSplit, PrepLayer, ...
_SIGNATURES = HEADER.signatures

_lib = None


def declared_symbols():
    return sorted(_SIGNATURES)


def lib():
    """Load the HIP library (once).  Raises if it is absent: no CPU/eager fallback exists."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libsrcnn_hip.so not found at %s - build it with `python -m stereo_rcnn_amd.csrc.build` "
                "(or __graft_entry__.build()). The product path has no fallback." % LIB_PATH)
        from . import streams
        streams.hip_may_start()            # the hardware-queue count HIP will start with is decided no later than here
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what="srcnn call"):
    if rc != 0:
        msg = lib().srcnn_last_error()
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda, "libsrcnn_hip operates on device memory only"
    assert t.is_contiguous(), "tensor must be contiguous"
    return t.data_ptr()


def int_array(values, ctype=c_int):
    """C array of integers for a library call."""
    values = [int(v) for v in values]
    return (ctype * len(values))(*values)


def ptr_array(tensors_or_ints):
    """C array of device pointers for a library call: tensors (their data_ptr) or addresses."""
    ptrs = [t if isinstance(t, int) else t.data_ptr() for t in tensors_or_ints]
    return (c_void_p * len(ptrs))(*ptrs)


def stream():
    """Handle of torch's current HIP stream: every launch goes where torch's allocator expects it."""
    return torch.cuda.current_stream().cuda_stream


class Workspace(object):
    """Grow-only device scratch owned by the caller side (one per device)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        nbytes = max(int(nbytes), 256)
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self.buf


_workspaces = {}
_recording_refs = None      # while a launch program records: every workspace handed out (the program keeps them alive)


def workspace(nbytes, device, key="default"):
    # one scratch buffer per (device, purpose, stream): forwards in flight on different streams never share scratch
    k = (str(device), key, torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0)
    if k not in _workspaces:
        _workspaces[k] = Workspace()
    buf = _workspaces[k].get(nbytes, device)
    if _recording_refs is not None:
        _recording_refs.append(buf)
    return buf
