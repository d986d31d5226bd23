"""CPU: the C ABI of the heads' training input (csrc/head_input_train.hip) -- declared, in the ctypes table, exported; every
argument check returns MANET_E_INVALID with a message naming the argument before anything reaches a device; the compiler's
resource report of the new kernels (no scratch, no spill) -- and the layers above: IntVOS(train_inputs=...), the cfg flag, the
ops' refusal of CPU tensors."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from test_match_train_abi import _hipcc

NEW = ["manet_head_input_forward_f32", "manet_head_input_backward_f32"]
KERNELS = ["head_input_fwd_kernel<4>", "head_input_fwd_kernel<1>", "head_input_bwd_kernel<4>", "head_input_bwd_kernel<1>"]
E_INVALID = -1
CSRC = os.path.join(ROOT, "cvpr2020_manet_amd", "csrc")


@pytest.fixture(autouse=True)
def _module_cfg_restored():
    """IntVOS(cfg, ...) installs its cfg as the module-level default of networks.IntVOS (set_cfg): put the previous one back, so
    that heads built without arguments by later tests keep the default widths"""
    from cvpr2020_manet_amd.networks import IntVOS as M
    saved = M.cfg
    yield
    M.set_cfg(saved)


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "cvpr2020_manet_amd", "libmanet_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "-C", CSRC])
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
    assert "head_input_train.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_argument_checks_return_invalid_without_a_device(lib):
    p = ctypes.c_void_p(4096)

    def fwd(**d):
        return lib.manet_head_input_forward_f32(d.get("embedding", p), 63, 9, 1, d.get("map0", p), d.get("map1", p), d.get("labels0", p),
                                                d.get("labels1", p), d.get("C", 5), d.get("h", 7), d.get("w", 9), d.get("n_ids", 3),
                                                d.get("n_maps", 2), d.get("n_planes", 1), d.get("normalize_first", 0), d.get("x", p),
                                                d.get("norm_out", p), None)

    def bwd(**d):
        return lib.manet_head_input_backward_f32(d.get("grad_x", p), d.get("norm_out", p), d.get("C", 5), d.get("h", 7), d.get("w", 9),
                                                 d.get("n_ids", 3), d.get("n_maps", 2), d.get("n_planes", 1), d.get("normalize_first", 0),
                                                 d.get("grad_embedding", p), 63, 9, 1, d.get("grad_map0", p), d.get("grad_map1", p), None)
    for call in (fwd, bwd):
        for bad in (0, -1, 129):
            assert call(C=bad) == E_INVALID and "C=%d" % bad in _err(lib)
        for bad in (0, 65, -3):
            assert call(n_ids=bad) == E_INVALID and "n_ids=%d" % bad in _err(lib)
        for bad in (-1, 3):
            assert call(n_maps=bad) == E_INVALID and "n_maps=%d" % bad in _err(lib)
        for bad in (0, 3):
            assert call(n_planes=bad) == E_INVALID and "n_planes=%d" % bad in _err(lib)
        assert call(n_maps=0, normalize_first=1) == E_INVALID and "normalize_first" in _err(lib)
        assert call(h=0) == E_INVALID and "h=0" in _err(lib)
        assert call(w=-2) == E_INVALID and "w=-2" in _err(lib)
        # 64 * (128 + 4) * 512 * 512 = 2^31 + ...: one element too many for the kernels' 31-bit row arithmetic
        assert call(C=128, n_ids=64, n_planes=2, h=512, w=512) == E_INVALID and "31 bits" in _err(lib)
    for ptr in ("embedding", "x", "labels0"):
        assert fwd(**{ptr: None}) == E_INVALID and "NULL" in _err(lib) and ptr.rstrip("0") in _err(lib), ptr
    assert fwd(map0=None) == E_INVALID and "map" in _err(lib)
    assert fwd(map1=None) == E_INVALID and "map" in _err(lib)
    assert fwd(n_planes=2, labels1=None) == E_INVALID and "labels" in _err(lib)
    assert fwd(normalize_first=1, norm_out=None) == E_INVALID and "norm_out" in _err(lib)
    assert bwd(grad_x=None) == E_INVALID and "grad_x" in _err(lib)
    assert bwd(normalize_first=1, norm_out=None) == E_INVALID and "norm_out" in _err(lib)
    # no output wanted: no work, no launch, no error
    assert bwd(grad_embedding=None, grad_map0=None, grad_map1=None) == 0
    assert bwd(n_maps=0, grad_embedding=None) == 0


def test_switch():
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    from test_intvos_module import TinyExtractor
    argv = ["--MODEL_SEMANTIC_EMBEDDING_DIM", "12", "--MODEL_HEAD_EMBEDDING_DIM", "8", "--MODEL_ASPP_OUTDIM", "6"]
    cfg = make_cfg(argv)
    assert not hasattr(cfg, "MODEL_TRAIN_INPUTS")  # the default cfg keeps the attributes it had
    plain = M.IntVOS(cfg, TinyExtractor())
    assert plain.train_inputs == "framework"
    model = M.IntVOS(cfg, TinyExtractor(), train_inputs="fused")
    assert model.train_inputs == "fused"
    assert list(model.state_dict()) == list(plain.state_dict())  # not a buffer, not in the state dict
    with pytest.raises(ValueError, match="train_inputs"):
        M.IntVOS(cfg, TinyExtractor(), train_inputs="all")
    assert M.IntVOS(make_cfg(argv + ["--MODEL_TRAIN_INPUTS", "fused"]), TinyExtractor()).train_inputs == "fused"
    cfg.MODEL_TRAIN_INPUTS = "fused"
    assert M.IntVOS(cfg, TinyExtractor()).train_inputs == "fused"
    assert M.IntVOS(cfg, TinyExtractor(), train_inputs="framework").train_inputs == "framework"
    cfg.MODEL_TRAIN_INPUTS = "hip"
    with pytest.raises(ValueError, match="train_inputs"):
        M.IntVOS(cfg, TinyExtractor())


def test_ops_refuse_cpu_tensors():
    from cvpr2020_manet_amd import ops
    from cvpr2020_manet_amd.networks import IntVOS as M
    emb = torch.rand(5, 7, 9, requires_grad=True)
    maps = [torch.rand(7, 9, 3), torch.rand(7, 9, 3)]
    lab = torch.zeros(7, 9, dtype=torch.int32)
    for nf in (False, True):
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.head_input_train(emb, maps, [lab], 3, normalize_first=nf)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.head_input_train(emb, [], [lab, lab], 3)
    head = M.DynamicSegHead(in_dim=8, embed_dim=8, train_kernels="fused")
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.dynamic_seghead_train_parts(head, emb, maps, [lab], 3)


def test_new_kernels_use_no_scratch_and_spill_nothing():
    _hipcc()  # (skips without the compiler)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(CSRC, "head_input_train.hip")],
                         capture_output=True, text=True, timeout=900, check=True).stdout
    rows = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if len(f) >= 7:
            rows[" ".join(f[:-6])] = [int(v) for v in f[-6:]]
    assert set(rows) == set(KERNELS), sorted(rows)
    bad = [(k, v) for k, v in rows.items() if v[3] or v[4]]  # VGPR spill, scratch bytes per lane
    assert not bad, bad
    for k, v in rows.items():  # streaming kernels: full occupancy
        assert v[5] >= 8, (k, v)
