"""CPU: the C-ABI library loads and exports every symbol that include/manet_hip.h declares
(no compute calls -- there is no GPU here)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def built_lib():
    so = os.path.join(ROOT, "cvpr2020_manet_amd", "libmanet_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cvpr2020_manet_amd", "csrc")])
    return so


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "manet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(manet_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    for s in ["manet_global_match", "manet_bank_prepare", "manet_global_match_prepared",
              "manet_local_match_f32", "manet_local_dist_f32", "manet_correlation_forward_f32",
              "manet_normalize_merge_f32", "manet_last_error_string"]:
        assert s in syms


def test_library_exports_every_declared_symbol(built_lib):
    from cvpr2020_manet_amd import _lib
    lib = _lib.load()  # binds every entry of SIGNATURES; raises if one is missing
    syms = declared_symbols()
    assert sorted(_lib.SIGNATURES) == syms, "ctypes table and header are out of sync"
    for s in syms:
        assert hasattr(lib, s)
    assert b"gfx950" in lib.manet_version()


def test_argument_validation_without_a_gpu(built_lib):
    """pure host-side checks of the ABI: size queries and error reporting need no device"""
    import ctypes
    from cvpr2020_manet_amd import _lib
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    assert lib.manet_global_match_workspace_bytes(25680, 128400, 100, 2, 1, _lib.COMPUTE_F32, ctypes.byref(n)) == 0
    assert 50e6 < n.value < 200e6  # packed bank (128400 x 104 floats) + packed queries + keys
    assert lib.manet_global_match_workspace_bytes(10, 10, 1000, 2, 1, 0, ctypes.byref(n)) == -1
    assert b"C=1000" in lib.manet_last_error_string()
    assert lib.manet_local_workspace_bytes(120, 214, 100, 13, 1, ctypes.byref(n)) == -1
    oc, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert lib.manet_correlation_out_dims(20, 30, 4, 1, 4, 1, 1, ctypes.byref(oc), ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oc.value, oh.value, ow.value) == (81, 20, 30)


# the global_match_* / frame_prepare_* kernels of the library: one build, one set
MATCH_KERNELS = sorted(
    ["frame_prepare_kernel<%s, %s>" % (t, v) for t in ("float", "unsigned short") for v in ("false", "true")] +
    ["global_match_f32_kernel<%d, %s>" % (ks, form) for ks in (16, 50, 52, 64)
     for form in ("1, true, false", "1, true, true", "8, false, false")] +
    ["global_match_f32_pipe_kernel<%d, %s>" % (ks, r) for ks in (16, 50, 52, 64) for r in ("false", "true")] +
    ["global_match_bf16_wide_kernel<%d, %s>" % (k, f) for k in (2, 7) for f in ("false", "true")] +
    ["global_match_bf16_pipe_kernel<9>"] +
    ["global_match_bf16x3_kernel<%d>" % k for k in (2, 7, 9)] +
    ["global_match_backward_kernel"])


def test_default_build_carries_no_ablation_variants(built_lib):
    """VERDICT r3 hygiene: the library compiles only the kernels the data path can reach.  The tuning keys that selected
    variant / ablation instantiations and experiment launch forms are retired and refused by name; the keys that only steer the
    shipped kernels (block map, split count, the unfused local route) work."""
    import subprocess as sp
    import sys
    code = (
        "import os, sys; os.environ['MANET_TUNING']='1'; sys.path.insert(0, %r)\n"
        "from cvpr2020_manet_amd import _lib\n"
        "lib = _lib.load()\n"
        "assert lib.manet_tune_set(0, 4) == 0 and lib.manet_tune_set(0, -2**31) == 0\n"
        "assert lib.manet_tune_set(1, 16) == 0 and lib.manet_tune_set(1, -2**31) == 0\n"
        "for k in (2, 3, 5, 6, 7, 9, 11, 12):\n"
        "    print('key', k, lib.manet_tune_set(k, 1), lib.manet_last_error_string().decode())\n" % ROOT)
    out = sp.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("key ")]
    assert len(lines) == 8
    for k, line in zip((2, 3, 5, 6, 7, 9, 11, 12), lines):
        assert line.startswith("key %d -1 " % k), line
        assert "tune key %d " % k in line and "removed" in line, line
    nm = sp.run(["nm", "-C", "--defined-only", built_lib], capture_output=True, text=True).stdout
    # none of the spilled / unreachable instantiations r3's build carried: no wide kernel at k-step 9, no 64-column frame prepare,
    # no un-pipelined k = 1 fp32 kernel, no ablation or register-staging form of the bf16 kernels
    for sym in ("global_match_bf16_wide_kernel<9", "global_match_bf16_wide_kernel<7, 4", "global_match_bf16_kernel<",
                "global_match_f32_kernel<64, 1, false", "frame_prepare_kernel<float, 64", "refine_debug_kernel"):
        assert sym not in nm, sym
    have = sorted(set(re.findall(r"__device_stub__((?:global_match_|frame_prepare_)\w+(?:<[^>]*>)?)\(", nm)))
    assert have == MATCH_KERNELS, (sorted(set(have) - set(MATCH_KERNELS)), sorted(set(MATCH_KERNELS) - set(have)))
