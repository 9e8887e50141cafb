"""ctypes binding of libspeechclip_hip.so, DERIVED from include/speechclip_hip.h (the C ABI every C source compiles against).

Nothing of the header is typed a second time here: ``_header`` reads it once at import - the six argument structs field by field,
every prototype with its return type, the integer ``#define``s - and refuses anything it does not understand.  What stays in this
file is naming (``STRUCT_NAMES``) and loading.

There is NO fallback: if the header or the library is missing or a symbol cannot be resolved this module raises, and every op in
``speechclip_plus_amd.ops`` fails loudly.  Build with ``python -m speechclip_plus_amd.build`` (or ``__graft_entry__.build()``).
"""
import contextlib
import ctypes
import os

from . import _header
from .build import INCLUDE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SC_LIB_PATH") or os.path.join(_HERE, "csrc", "libspeechclip_hip.so")   # override: same-box A/B of two builds
HEADER_PATH = os.path.join(INCLUDE, "speechclip_hip.h")

# C struct -> the Python name of its ctypes class, in the order of sc_sizeof()'s indices.  Segments (sc_segments) is the ragged row
# layout: device tables row0 [B + 1], chunk [rows / 8][4].
STRUCT_NAMES = {"sc_gemm_args": "GemmArgs", "sc_hubert_layer_args": "HubertLayerArgs", "sc_rt_gemm_args": "RtGemmArgs",
                "sc_rt_ln_args": "RtLnArgs", "sc_rt_ln_bwd_args": "RtLnBwdArgs", "sc_segments": "Segments"}
HEADER = _header.read(HEADER_PATH, STRUCT_NAMES)
if set(HEADER.structs) != set(STRUCT_NAMES):
    raise RuntimeError(f"{HEADER_PATH} declares the structs {sorted(HEADER.structs)}, _lib.STRUCT_NAMES names {sorted(STRUCT_NAMES)}")
GemmArgs, HubertLayerArgs, RtGemmArgs, RtLnArgs, RtLnBwdArgs, Segments = STRUCTS = tuple(HEADER.structs[c] for c in STRUCT_NAMES)
DEFINES = HEADER.defines            # the header's integer #defines: SC_SEG_ROWS, SC_ATTN_SLACK, SC_CONV0_NSTAT, SC_WS_*, SC_SUPCON_MAX_LOGIT_BYTES
# name -> argtypes of the functions that return int / int32_t (a status, or a small count); the others (sc_last_error, sc_sizeof,
# sc_workspace_bytes, sc_infonce_workspace_floats, sc_supcon_workspace_floats, sc_hash32) are bound from HEADER.functions like these, with
# their own restype
SIGNATURES = {name: argtypes for name, (restype, argtypes) in HEADER.functions.items() if restype is ctypes.c_int32}
# The cross-batch queue's three entry points (csrc/infonce_queue.hip) stand in a header of their own, read by the same reader and
# bound by the same loop: speechclip_hip.h and the tables above are as they were before them.
QUEUE_HEADER_PATH = os.path.join(INCLUDE, "speechclip_hip_queue.h")
QUEUE_HEADER = _header.read(QUEUE_HEADER_PATH)
if QUEUE_HEADER.structs or QUEUE_HEADER.defines or set(QUEUE_HEADER.functions) & set(HEADER.functions):
    raise RuntimeError(f"{QUEUE_HEADER_PATH} declares prototypes only, none of them {HEADER_PATH}'s")
# So do the pairwise sigmoid loss's three (csrc/sigmoid_loss.hip): the same reader, the same loop, the other two headers as they were.
SIGMOID_HEADER_PATH = os.path.join(INCLUDE, "speechclip_hip_sigmoid.h")
SIGMOID_HEADER = _header.read(SIGMOID_HEADER_PATH)
if SIGMOID_HEADER.structs or SIGMOID_HEADER.defines or set(SIGMOID_HEADER.functions) & (set(HEADER.functions) | set(QUEUE_HEADER.functions)):
    raise RuntimeError(f"{SIGMOID_HEADER_PATH} declares prototypes only, none of them another header's")

DIAG_LIB_PATH = os.path.join(_HERE, "csrc", "libspeechclip_hip_diag.so")
GELU_EXACT_LIB_PATH = os.path.join(_HERE, "csrc", "libspeechclip_hip_gelu_exact.so")   # checker build (build.py), tests only
_LIB = None
_DIAG = None
_VARIANTS = {}


def lib() -> ctypes.CDLL:
    """The product library."""
    global _LIB
    if _LIB is None:
        _LIB = _load(LIB_PATH)
    return _LIB


@contextlib.contextmanager
def using_library(path: str):
    """Tests / A-B tools only: route every op through another build of the SAME ABI (e.g. GELU_EXACT_LIB_PATH) inside the block, in one
    process, so two builds see identical inputs.  The libraries hold no state the ops share (weight copies live in torch tensors)."""
    global _LIB
    if path not in _VARIANTS:
        _VARIANTS[path] = _load(path)
    prev, _LIB = lib(), _VARIANTS[path]
    try:
        yield _LIB
    finally:
        _LIB = prev


def diag_lib() -> ctypes.CDLL:
    """libspeechclip_hip_diag.so: the same ABI built with SC_DIAG_BUILD - additionally the timing-only / stamped kernels (GEMM tile ids
    32 / 34, the attention section stamps) and the opt-in LayerNorm-folded GEMMs.  Loaded by tools/, bench.py's in-kernel clock probe
    and the SC_FUSED_LN experiment; the product path (lib()) cannot reach those kernels."""
    global _DIAG
    if _DIAG is None:
        _DIAG = _load(DIAG_LIB_PATH)
        if _DIAG.sc_is_diag_build() != 1:
            raise RuntimeError(f"{DIAG_LIB_PATH} is not a diagnostics build")
    return _DIAG


def _load(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP extension is not built (python -m speechclip_plus_amd.build). "
            "speechclip_plus_amd has no CPU / eager fallback.")
    cdll = ctypes.CDLL(path)
    for name, (restype, argtypes) in (list(HEADER.functions.items()) + list(QUEUE_HEADER.functions.items())
                                      + list(SIGMOID_HEADER.functions.items())):
        fn = getattr(cdll, name)            # AttributeError if the symbol is missing: loud
        fn.argtypes = argtypes
        fn.restype = restype
    for what, cls in enumerate(STRUCTS):
        if cdll.sc_sizeof(what) != ctypes.sizeof(cls):
            raise RuntimeError(f"{cls.__name__}: the header's struct has {ctypes.sizeof(cls)} bytes, the library's {cdll.sc_sizeof(what)} "
                               f"({path} was built from another {HEADER_PATH}: a stale .so)")
    return cdll


def check(rc: int, what: str = "", library=None) -> None:
    if rc != 0:
        raise RuntimeError(f"libspeechclip_hip {what} failed ({rc}): {(library or lib()).sc_last_error().decode()}")
