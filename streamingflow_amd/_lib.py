"""ctypes binding of libsfnative.so (C ABI: include/sfnative.h).

The header is the only place a prototype or a public constant is written: `SIGNATURES` and every `SF_*` name below are read from
it at import (_header.py), so the binding cannot drift from the contract.  What stays by hand are the `Structure` classes, whose
field names the Python code uses and whose sizes `lib()` proves against the library (sf_abi_check).  Arguments: scalars by their C
type, a pointer to a public struct as POINTER(its class), every other pointer or array as c_void_p.

The library is the product: there is no CPU or PyTorch fallback.  `lib()` raises if the shared
object is missing or does not export every symbol the header declares.
"""
import ctypes as C
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SF_LIB_PATH") or os.path.join(_HERE, "libsfnative.so")   # SF_LIB_PATH: experiment builds only

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int32)

_PROTOS, CONSTANTS, _STRUCT_NAMES = _header.read()
globals().update(CONSTANTS)      # SF_OK, SF_ERR_*, SF_ABI_VERSION, SF_COEF_STRIDE, SF_PROF_KEYS, SF_*_PLAN_INTS, SF_PANOPTIC_*, ... under their header names


def _family(prefix):
    return {k[len(prefix):].lower(): v for k, v in CONSTANTS.items() if k.startswith(prefix)}


PACK_TRANSPOSED, PACK_FOLD_DUP, PACK_INTERLEAVE, PACK_BF16X3, PACK_WINOGRAD = (
    CONSTANTS["SF_PACK_" + n] for n in ("TRANSPOSED", "FOLD_DUP", "INTERLEAVE", "BF16X3", "WINOGRAD"))
ACT = _family("SF_ACT_")            # {"none": 0, "lrelu": 1, ...}
SOLVER = _family("SF_SOLVER_")      # {"euler": 0, "midpoint": 1, "rk4": 2}
OP_JUMP, OP_STEP = CONSTANTS["SF_OP_JUMP"], CONSTANTS["SF_OP_STEP"]


class ConvW(C.Structure):
    _fields_ = [("w", C.c_void_p), ("scale", C.c_void_p), ("bias", C.c_void_p),
                ("cout", C.c_int32), ("cout_pad", C.c_int32), ("c0", C.c_int32), ("c1", C.c_int32),
                ("cin_pad", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32), ("dil", C.c_int32),
                ("stride", C.c_int32), ("pad", C.c_int32), ("act", C.c_int32), ("reserved", C.c_int32), ("w_bf16x3", C.c_void_p), ("w_wino", C.c_void_p)]


class GruW(C.Structure):
    _fields_ = [("gates", ConvW), ("cand", ConvW), ("decoder", ConvW)]


class DualW(C.Structure):
    _fields_ = [("gates1", ConvW), ("cand1", ConvW), ("gates2", ConvW), ("cand2", ConvW), ("dec2", ConvW),
                ("tg7", ConvW), ("tgproj", ConvW), ("tg1", ConvW), ("tg3", ConvW),
                ("w_logit", C.c_void_p), ("C", C.c_int32), ("gates1_x", ConvW), ("gates1_s", ConvW)]


class BottleW(C.Structure):
    _fields_ = [("c7", ConvW), ("c1", ConvW), ("c3", ConvW), ("proj", ConvW)]


class ResW(C.Structure):
    _fields_ = [("conv1", ConvW), ("conv2", ConvW), ("proj", ConvW)]


class PModelW(C.Structure):
    _fields_ = [("rb0", ResW), ("rb1", ResW), ("se0_fc0", C.c_void_p), ("se0_fc2", C.c_void_p),
                ("se1_fc0", C.c_void_p), ("se1_fc2", C.c_void_p), ("last", ConvW), ("C", C.c_int32)]


class EncoderW(C.Structure):
    _fields_ = [("blocks", ResW * 5), ("last", ConvW), ("C", C.c_int32), ("F", C.c_int32)]


class DecoderW(C.Structure):
    _fields_ = [("first", ConvW), ("blocks", ResW * 5), ("last0", ConvW), ("last1", ConvW),
                ("C", C.c_int32), ("F", C.c_int32)]


class ConvNextW(C.Structure):
    _fields_ = [("dw_w", C.c_void_p), ("dw_b", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p),
                ("pw1", ConvW), ("pw2", ConvW), ("C", C.c_int32)]


class DeepLabW(C.Structure):
    _fields_ = [("branch", ConvW * 4), ("pool_w", C.c_void_p), ("pool_scale", C.c_void_p),
                ("pool_bias", C.c_void_p), ("proj_pool_w", C.c_void_p), ("project", ConvW),
                ("conv3", ConvW), ("cls", ConvW), ("C", C.c_int32), ("hid", C.c_int32)]


class BottleneckW(C.Structure):
    _fields_ = [("down", ConvW), ("conv", ConvW), ("up", ConvW), ("proj", ConvW), ("downsample", C.c_int32)]


# the two structs of include/sfnative_effnet.h (the EfficientNet trunk's extension header): passed as `const void*`, guarded by
# SF_EFFNET_ABI_VERSION / sf_effnet_abi_sizeof (EFFNET_STRUCTS below, checked by lib())
class MBConvW(C.Structure):
    _fields_ = [("expand", ConvW), ("project", ConvW), ("dw_w", C.c_void_p), ("dw_scale", C.c_void_p), ("dw_bias", C.c_void_p),
                ("se_reduce_w", C.c_void_p), ("se_reduce_b", C.c_void_p), ("se_expand_w", C.c_void_p), ("se_expand_b", C.c_void_p),
                ("cin", C.c_int32), ("cexp", C.c_int32), ("cout", C.c_int32), ("cse", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32),
                ("pad_t", C.c_int32), ("pad_l", C.c_int32), ("pad_b", C.c_int32), ("pad_r", C.c_int32), ("skip", C.c_int32),
                ("reserved", C.c_int32)]


class EffNetW(C.Structure):
    _fields_ = [("stem_w", C.c_void_p), ("stem_scale", C.c_void_p), ("stem_bias", C.c_void_p), ("blocks", C.POINTER(MBConvW)),
                ("c_stem", C.c_int32), ("n_blocks", C.c_int32), ("pad_t", C.c_int32), ("pad_l", C.c_int32), ("pad_b", C.c_int32),
                ("pad_r", C.c_int32), ("index", C.c_int32), ("reserved", C.c_int32)]


EFFNET_STRUCTS = (MBConvW, EffNetW)      # in SF_EFFNET_STRUCT_* order

STRUCTS = {"sf_conv_w": ConvW, "sf_gru_w": GruW, "sf_dual_w": DualW, "sf_res_w": ResW, "sf_pmodel_w": PModelW, "sf_encoder_w": EncoderW,
           "sf_decoder_w": DecoderW, "sf_convnext_w": ConvNextW, "sf_deeplab_w": DeepLabW, "sf_bottleneck_w": BottleneckW, "sf_bottle_w": BottleW}
assert set(STRUCTS) == set(_STRUCT_NAMES), set(STRUCTS) ^ set(_STRUCT_NAMES)
# in the header's SF_STRUCT_* order (SF_STRUCT_CONV_W = 0 is sf_conv_w): what lib() hands to sf_abi_check
_ids = _family("SF_STRUCT_")
ABI_STRUCTS = tuple(STRUCTS["sf_" + k] for k in sorted(_ids, key=_ids.get) if k != "count")
assert len(ABI_STRUCTS) == _ids["count"]

_sz = C.c_size_t
CTYPES = {"int": C.c_int, "long": C.c_long, "size_t": _sz, "float": C.c_float, "double": C.c_double, "const char*": C.c_char_p}


def ctype(t):
    """The ctypes class of a C type as _header spells it: a pointer to a public struct is typed, any other pointer is c_void_p, which
    takes what the callers pass (ctypes arrays, byref(), data_as() pointers, data_ptr() integers, None)."""
    if t in CTYPES:
        return CTYPES[t]
    struct = STRUCTS.get(t.replace("const ", "")[:-1])
    return C.POINTER(struct) if struct else C.c_void_p


# name -> (restype, argtypes); every function include/sfnative.h declares
SIGNATURES = {name: (ctype(ret), [ctype(a) for a in args]) for name, (ret, args) in _PROTOS.items()}

# kernel key = KEY_NAMES key * 8 + epilogue.  Keys 0..15 are the tiled conv kernels: beside each name the rows of the tile table (csrc/sf_launch.h:
# TILES) that report it — the table's key column is the authority; DESIGN.md 4.2 lists the launches reported under another tile's name
KEY_NAMES = {
    0: "S16x64k4",            # TILE_S16x64K4
    1: "L64x64",              # TILE_L64x64
    2: "LN64x128",            # TILE_LN64x128
    3: "direct16px",          # TILE_DIRECT16
    4: "T64x64splitK",        # TILE_SPLIT64x64
    5: "dmaLN128x64",         # TILE_DMA_LN128x64
    6: "L64x128",             # retired name: no row reports this key
    7: "L128x128w4",          # retired name
    8: "L64x128w8",           # retired name
    9: "L128x128w8",          # TILE_L128x128
    10: "dma128x128w8",       # TILE_DMA128x128 (SE-scaled launches: the 64x64 SCALE instantiation runs)
    11: "dma64x64",           # TILE_DMA64x64, and reported as it: TILE_DMA32x128 (narrow layers), TILE_DMA32x32 (one latent), TILE_DMA64x128W4 (SF_NARROW=7)
    12: "dma64x128w8",        # TILE_DMA64x128, TILE_DMA64x256 (SE-scaled launches: the 64x64 SCALE instantiation runs)
    13: "dmaLN64x128",        # TILE_DMA_LN64x128
    14: "sp64x32",            # the small-P kernel (conv_sp.hip)
    15: "dmaT64x64splitK",    # TILE_DMA_SPLIT64x64
    16: "wino128x32t",        # the Winograd kernel (conv_wino.hip): 16 + form
    17: "wino64x64t",
    18: "wino64x32t2",
    19: "wino64x32t2dil",
    20: "mlp64-256-64",       # convnext_mlp.hip
}
KERNEL_NAMES = {c * 8 + e: (f"convnext_mlp<{cn[3:]},gelu+residual>" if cn.startswith("mlp") else f"conv_wino<{cn[4:]},{en}>" if cn.startswith("wino") else f"conv_glds<{cn[3:]},{en}>" if cn.startswith("dma") else f"conv_sp<{cn[2:]},{en}>" if cn.startswith("sp") else f"conv_igemm<{cn},{en}>")
                for c, cn in KEY_NAMES.items()
                for e, en in enumerate(("affine", "blend", "ln_gelu", "trust", "sample"))}

_LIB = None


def lib():
    """Load (once) and return the ctypes handle; raises RuntimeError when the HIP library is absent."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m streamingflow_amd.build` "
                "(hipcc --offload-arch=gfx950). streamingflow_amd has no CPU fallback.")
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)     # AttributeError => missing export
            fn.restype, fn.argtypes = res, args
        # ABI guard: this binding's struct layouts against the ones the library was compiled with
        sizes = (_sz * len(ABI_STRUCTS))(*[C.sizeof(t) for t in ABI_STRUCTS])
        if h.sf_abi_check(SF_ABI_VERSION, sizes, len(ABI_STRUCTS)) != 0:
            theirs = [h.sf_abi_sizeof(i) for i in range(len(ABI_STRUCTS))]
            raise RuntimeError(f"{LIB_PATH}: ABI mismatch (library ABI {h.sf_abi_version()}, sizes {theirs}; binding ABI "
                               f"{SF_ABI_VERSION}, sizes {list(sizes)}): rebuild with `python -m streamingflow_amd.build`")
        if h.sf_effnet_abi_version() != SF_EFFNET_ABI_VERSION or [h.sf_effnet_abi_sizeof(i) for i in range(len(EFFNET_STRUCTS))] != [C.sizeof(t) for t in EFFNET_STRUCTS]:
            raise RuntimeError(f"{LIB_PATH}: ABI mismatch of the EfficientNet trunk structs (include/sfnative_effnet.h): rebuild with `python -m streamingflow_amd.build`")
        _LIB = h
    return _LIB


def check(status, what=""):
    if status != 0:
        msg = lib().sf_status_string(status).decode()
        raise RuntimeError(f"libsfnative {what}: {msg} ({status})")
