"""CPU: the layout guard of the EfficientNet trunk's structs (include/sfnative_effnet.h: sf_mbconv_w, sf_effnet_w) as the header (compiled
by gcc), the library and the ctypes binding see them — the pattern of tests/test_cabi.py.  They live in an extension header under
SF_EFFNET_ABI_VERSION / sf_effnet_abi_sizeof: the struct set and SF_ABI_VERSION of sfnative.h, which tests/test_cabi.py pins, are what
they were."""
import ctypes
import os
import subprocess

import pytest

from util import ROOT


def test_extension_guard_header_library_binding_agree(tmp_path):
    from streamingflow_amd import _lib
    lib = _lib.lib()
    assert _lib.SF_EFFNET_ABI_VERSION == lib.sf_effnet_abi_version() == 1
    assert (_lib.SF_EFFNET_STRUCT_MBCONV_W, _lib.SF_EFFNET_STRUCT_EFFNET_W, _lib.SF_EFFNET_STRUCT_COUNT) == (0, 1, 2)
    assert _lib.EFFNET_STRUCTS == (_lib.MBConvW, _lib.EffNetW)
    # the main header's guard does not know them: its struct set and version are unchanged
    assert lib.sf_abi_version() == _lib.SF_ABI_VERSION and lib.sf_abi_sizeof(_lib.SF_STRUCT_COUNT) == 0
    assert not {"sf_mbconv_w", "sf_effnet_w"} & set(_lib.STRUCTS)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sfnative_effnet.h"\nint main(void) {\n'
                   '  printf("%d %zu %zu %zu %zu %zu\\n", SF_EFFNET_ABI_VERSION, sizeof(sf_mbconv_w), sizeof(sf_effnet_w), offsetof(sf_mbconv_w, dw_w),\n'
                   '         offsetof(sf_mbconv_w, cin), offsetof(sf_effnet_w, c_stem));\n'
                   '  return SF_EFFNET_STRUCT_COUNT == 2 ? 0 : 1;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    ver, mb, eff, off_dw, off_cin, off_stem = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ver == _lib.SF_EFFNET_ABI_VERSION
    assert mb == lib.sf_effnet_abi_sizeof(0) == ctypes.sizeof(_lib.MBConvW) == 2 * ctypes.sizeof(_lib.ConvW) + 7 * 8 + 12 * 4
    assert eff == lib.sf_effnet_abi_sizeof(1) == ctypes.sizeof(_lib.EffNetW) == 4 * 8 + 8 * 4
    assert (off_dw, off_cin, off_stem) == (_lib.MBConvW.dw_w.offset, _lib.MBConvW.cin.offset, _lib.EffNetW.c_stem.offset)
    assert lib.sf_effnet_abi_sizeof(2) == 0 and lib.sf_effnet_abi_sizeof(-1) == 0


def test_header_handshake_runs_against_the_library(tmp_path):
    """sf_effnet_abi_check_header(), compiled by gcc from the extension header and linked with the library, returns SF_OK."""
    from streamingflow_amd import _lib
    src = tmp_path / "shake.c"
    src.write_text('#include "sfnative_effnet.h"\nint main(void) { return sf_effnet_abi_check_header() == SF_OK ? 0 : 1; }\n')
    exe = tmp_path / "shake"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_a_binding_with_a_stale_trunk_struct_is_refused_at_load():
    from streamingflow_amd import _lib
    _lib.lib()
    real, _lib._LIB = _lib._LIB, None
    old = _lib.EFFNET_STRUCTS

    class StaleMBConvW(ctypes.Structure):
        _fields_ = _lib.MBConvW._fields_[:-2]
    try:
        _lib.EFFNET_STRUCTS = (StaleMBConvW, old[1])
        with pytest.raises(RuntimeError, match="ABI mismatch"):
            _lib.lib()
    finally:
        _lib.EFFNET_STRUCTS, _lib._LIB = old, real
    assert _lib.lib() is real


def test_trunk_entry_points_are_bound_from_the_header():
    from streamingflow_amd import _lib
    i, v, z = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["sf_effnet_trunk_ws_bytes"] == (z, [v, i, i, i])
    assert _lib.SIGNATURES["sf_effnet_trunk_fwd"] == (i, [v, v, i, v, v, i, i, i, v, z, v])
    assert _lib.SIGNATURES["sf_mbconv_fwd"] == (i, [v, v, v, i, i, i, v, z, v])
    assert _lib.SIGNATURES["sf_effnet_pointwise_fwd"] == (i, [ctypes.POINTER(_lib.ConvW), v, v, v, v, i, i, i, v])
    assert _lib.SIGNATURES["sf_effnet_abi_sizeof"] == (z, [i])
