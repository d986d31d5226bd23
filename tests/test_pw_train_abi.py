"""CPU: the C ABI of the training 1x1 and BatchNorm + ReLU kernels (csrc/pw_train.hip) -- declared, exported, workspace
queries, argument checks that return MANET_E_INVALID before anything reaches a device, and the register / occupancy budget of
the hot kernels in the compiler's resource report (no scratch, no spill)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

NEW = ["manet_pw_forward_workspace_bytes", "manet_pw_forward_f32", "manet_pw_backward_data_f32",
       "manet_pw_backward_weight_workspace_bytes", "manet_pw_backward_weight_f32", "manet_bn_relu_workspace_bytes",
       "manet_bn_relu_forward_f32", "manet_bn_relu_backward_f32"]
E_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "cvpr2020_manet_amd", "libmanet_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cvpr2020_manet_amd", "csrc")])
    from cvpr2020_manet_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.manet_last_error_string().decode()


def test_new_symbols_are_declared_and_exported(lib):
    from cvpr2020_manet_amd import _lib
    text = open(os.path.join(ROOT, "include", "manet_hip.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES
        assert hasattr(lib, s)


def test_workspace_queries(lib):
    n = ctypes.c_size_t(0)
    # forward: W transposed for the inference kernel (256 output channels, h*w % 4 == 0), nothing otherwise
    assert lib.manet_pw_forward_workspace_bytes(3, 103, 256, 104 * 104, ctypes.byref(n)) == 0 and n.value == 103 * 256 * 4
    assert lib.manet_pw_forward_workspace_bytes(2, 3, 8, 130, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.manet_pw_forward_workspace_bytes(2, 256, 256, 130, ctypes.byref(n)) == 0 and n.value == 0
    # backward-weight: 128 x 128 slabs per (tile, slice) + 128 bias partials per (row tile, slice)
    assert lib.manet_pw_backward_weight_workspace_bytes(3, 256, 256, 120 * 214, ctypes.byref(n)) == 0
    assert 0 < n.value <= 64 << 20 and n.value % (128 * 4) == 0
    assert lib.manet_pw_backward_weight_workspace_bytes(1, 1, 1, 1, ctypes.byref(n)) == 0
    assert n.value == (128 * 128 + 128) * 4  # one chunk: one slice
    # BN + ReLU: two floats per (channel, 4096-element tile) + two per channel
    assert lib.manet_bn_relu_workspace_bytes(3, 256, 120 * 214, ctypes.byref(n)) == 0
    assert n.value == (2 * 3 * 256 * 7 + 2 * 256) * 4
    for dims in ((0, 3, 8, 130), (2, 0, 8, 130), (2, 3, 0, 130), (2, 3, 8, -1)):
        assert lib.manet_pw_forward_workspace_bytes(*dims, ctypes.byref(n)) == E_INVALID
        assert "positive" in _err(lib)
        assert lib.manet_pw_backward_weight_workspace_bytes(*dims, ctypes.byref(n)) == E_INVALID
        assert "positive" in _err(lib)
    for dims in ((0, 3, 130), (2, 0, 130), (2, 3, 0)):
        assert lib.manet_bn_relu_workspace_bytes(*dims, ctypes.byref(n)) == E_INVALID
        assert "positive" in _err(lib)
    assert lib.manet_pw_forward_workspace_bytes(2, 3, 8, 130, None) == E_INVALID
    assert lib.manet_pw_backward_weight_workspace_bytes(2, 3, 8, 130, None) == E_INVALID
    assert lib.manet_bn_relu_workspace_bytes(2, 3, 130, None) == E_INVALID
    assert "NULL" in _err(lib)


def test_argument_checks_return_invalid_without_a_device(lib):
    """every refusal happens on the host before a launch: fake (never dereferenced) pointers are enough"""
    p = ctypes.c_void_p(4096)
    n = ctypes.c_size_t(0)
    assert lib.manet_pw_forward_f32(None, 2, 3, 8, 130, p, None, p, None, 0, None) == E_INVALID
    assert "NULL" in _err(lib)
    assert lib.manet_pw_forward_f32(p, 2, 3, 0, 130, p, None, p, None, 0, None) == E_INVALID
    assert "positive" in _err(lib)
    assert lib.manet_pw_forward_f32(p, 70000, 3, 8, 130, p, None, p, None, 0, None) == E_INVALID
    assert lib.manet_pw_forward_workspace_bytes(3, 103, 256, 10816, ctypes.byref(n)) == 0
    assert lib.manet_pw_forward_f32(p, 3, 103, 256, 10816, p, p, p, p, n.value - 4, None) == E_INVALID
    assert "workspace" in _err(lib)
    assert lib.manet_pw_forward_f32(p, 3, 103, 256, 10816, p, p, p, None, n.value, None) == E_INVALID
    assert lib.manet_pw_backward_data_f32(p, 2, 3, 8, 130, None, p, None) == E_INVALID
    assert lib.manet_pw_backward_data_f32(p, 2, -3, 8, 130, p, p, None) == E_INVALID
    assert lib.manet_pw_backward_weight_workspace_bytes(2, 3, 8, 130, ctypes.byref(n)) == 0
    assert lib.manet_pw_backward_weight_f32(p, p, 2, 3, 8, 130, p, p, p, n.value - 1, None) == E_INVALID
    assert "workspace" in _err(lib)
    assert lib.manet_pw_backward_weight_f32(p, p, 2, 3, 8, 130, None, None, p, n.value, None) == E_INVALID
    assert lib.manet_pw_backward_weight_f32(p, None, 2, 3, 8, 130, p, p, p, n.value, None) == E_INVALID
    assert lib.manet_pw_backward_weight_f32(p, p, 2, 3, 8, 130, p, p, None, n.value, None) == E_INVALID
    assert lib.manet_bn_relu_workspace_bytes(2, 3, 130, ctypes.byref(n)) == 0
    f = ctypes.c_float
    fwd = lambda B, C, HW, mom, eps, train, ws, nb, x=p: lib.manet_bn_relu_forward_f32(  # noqa: E731
        x, B, C, HW, p, p, p, p, f(mom), f(eps), train, p, p, p, ws, nb, None)
    assert fwd(1, 3, 1, 0.1, 1e-5, 1, p, n.value) == E_INVALID
    assert "one value per channel" in _err(lib)
    assert fwd(2, 3, 130, 0.1, 1e-5, 1, p, n.value - 1) == E_INVALID
    assert "workspace" in _err(lib)
    assert fwd(2, 3, 130, 0.1, 0.0, 1, p, n.value) == E_INVALID
    assert fwd(2, 3, 130, 1.5, 1e-5, 1, p, n.value) == E_INVALID
    assert "momentum" in _err(lib)
    assert fwd(2, 3, 130, 0.1, 1e-5, 1, p, n.value, x=None) == E_INVALID
    assert "NULL" in _err(lib)
    assert fwd(2, 0, 130, 0.1, 1e-5, 0, None, 0) == E_INVALID
    bwd = lambda train, gx, ws, nb, dy=p: lib.manet_bn_relu_backward_f32(  # noqa: E731
        dy, p, 2, 3, 130, p, p, p, p, train, gx, p, p, ws, nb, None)
    assert bwd(1, p, p, n.value - 1) == E_INVALID
    assert "workspace" in _err(lib)
    assert bwd(0, p, None, 0) == E_INVALID  # (d_gamma / d_beta asked for: the reduction needs the workspace)
    assert bwd(1, p, p, n.value, dy=None) == E_INVALID
    assert "NULL" in _err(lib)


def _resources():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "cvpr2020_manet_amd", "csrc", "pw_train.hip")],
                         capture_output=True, text=True, timeout=900, check=True).stdout
    rows = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if len(f) >= 7:
            rows[" ".join(f[:-6])] = [int(v) for v in f[-6:]]
    return rows


# kernel -> (max VGPR + AGPR per lane, min waves per SIMD), in the style of test_kernel_resources.HOT
HOT = {
    "pw_gemm_kernel<true>": (256, 2), "pw_gemm_kernel<false>": (256, 2),
    "pw_wgrad_kernel<true>": (256, 2), "pw_wgrad_kernel<false>": (256, 2),
    "pw_wgrad_finish_kernel": (64, 8), "pw_transpose_kernel": (64, 8),
    "bn_stats_kernel<true>": (64, 8), "bn_stats_finish_kernel": (64, 8), "bn_apply_kernel<true>": (64, 8),
    "bn_bwd_reduce_kernel<true>": (64, 8), "bn_bwd_finish_kernel": (64, 8), "bn_bwd_apply_kernel<true>": (64, 8),
    "bn_stats_kernel<false>": (64, 8), "bn_apply_kernel<false>": (64, 8), "bn_bwd_reduce_kernel<false>": (64, 8),
    "bn_bwd_apply_kernel<false>": (128, 4),
}


def test_new_kernels_keep_their_register_budget_and_use_no_scratch():
    rows = _resources()
    assert set(HOT) <= set(rows), sorted(rows)
    bad = []
    for name, (vgpr, agpr, sgpr, spill, scratch, occ) in rows.items():
        if scratch or spill:
            bad.append((name, rows[name]))
    for name, (regs, min_occ) in HOT.items():
        vgpr, agpr, sgpr, spill, scratch, occ = rows[name]
        if vgpr + max(agpr, 0) > regs or occ < min_occ:
            bad.append((name, rows[name]))
    assert not bad, bad
