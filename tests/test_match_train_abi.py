"""CPU: the C ABI of the ordered training route of the matching path (csrc/match_train.hip) -- declared, in the ctypes table,
exported; the workspace queries return the documented sizes; null pointers and n_ids / d / k out of range return MANET_E_INVALID
with a message before anything reaches a device; the compiler's resource report of the new kernels (no scratch, no spill); their
device assembly holds no floating-point atomic add of any address space -- and the switches above: ops' `deterministic=` keyword,
IntVOS(train_match=...)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

NEW = ["manet_global_match_backward_ordered_workspace_bytes", "manet_global_match_backward_ordered_f32",
       "manet_local_match_train_forward_f32", "manet_local_match_train_workspace_bytes", "manet_local_match_train_backward_f32",
       "manet_local_match_full_backward_ordered_f32"]
KERNELS = ["mt_rows_kernel", "mt_global_query_kernel", "mt_global_bank_kernel<16>", "mt_global_bank_kernel<32>", "mt_local_min_arg_kernel",
           "mt_pool_cl_kernel", "mt_local_cell_kernel", "mt_local_prev_kernel", "mt_unpool_kernel", "mt_fill_kernel", "mt_full_dv_kernel",
           "mt_full_dist_kernel"]
E_INVALID, E_WORKSPACE = -1, -2
CSRC = os.path.join(ROOT, "cvpr2020_manet_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "cvpr2020_manet_amd", "libmanet_hip.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    from cvpr2020_manet_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.manet_last_error_string().decode()


def _a256(n):
    return (n + 255) // 256 * 256


def test_new_symbols_are_declared_and_exported(lib):
    from cvpr2020_manet_amd import _lib
    text = open(os.path.join(ROOT, "include", "manet_hip.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.SIGNATURES
        assert hasattr(lib, s)


def test_workspace_queries_return_the_documented_sizes(lib):
    n = ctypes.c_size_t(0)
    # global: the query as [N][C] rows
    assert lib.manet_global_match_backward_ordered_workspace_bytes(10816, 10816, 100, 3, 1, ctypes.byref(n)) == 0
    assert n.value == _a256(10816 * 100 * 4)
    assert lib.manet_global_match_backward_ordered_workspace_bytes(25680, 128400, 100, 3, 8, ctypes.byref(n)) == 0
    assert n.value == _a256(25680 * 100 * 4)
    assert lib.manet_global_match_backward_ordered_workspace_bytes(7, 0, 3, 1, 1, ctypes.byref(n)) == 0 and n.value == 256
    # local: four pooled [cells][C] planes, the per-cell counts, lists (offset, coefficient) of `cap` entries, bitmap + counts
    for h, w, C, n_ids, d, cover in ((104, 104, 100, 3, 12, 5), (120, 214, 100, 3, 12, 5), (104, 104, 100, 5, 12, 5), (104, 104, 100, 64, 12, 5),
                                     (480, 854, 100, 3, 12, 5), (24, 30, 16, 2, 2, 5), (12, 13, 8, 2, 0, 5)):
        cells = (h // 2) * (w // 2)
        cap = min((2 * d + 1) ** 2, cover * cover * n_ids)
        want = 4 * _a256(cells * C * 4) + _a256(cells * 4) + 2 * _a256(cells * cap * 4) + 2 * _a256(cells * 20 * 4)
        assert lib.manet_local_match_train_workspace_bytes(h, w, C, n_ids, d, ctypes.byref(n)) == 0
        assert n.value == want, (h, w, C, n_ids, d, n.value, want)
    assert lib.manet_local_match_train_workspace_bytes(104, 104, 100, 3, 12, None) == E_INVALID and "NULL" in _err(lib)
    assert lib.manet_global_match_backward_ordered_workspace_bytes(5, 5, 5, 1, 1, None) == E_INVALID and "NULL" in _err(lib)


def test_argument_checks_return_invalid_without_a_device(lib):
    p = ctypes.c_void_p(4096)
    n = ctypes.c_size_t(0)

    def gq(**d):
        return lib.manet_global_match_backward_ordered_workspace_bytes(d.get("N", 100), d.get("M0", 50), d.get("C", 16), d.get("n_ids", 3),
                                                                       d.get("ranks", 1), ctypes.byref(n))

    def gb(**d):
        return lib.manet_global_match_backward_ordered_f32(d.get("query", p), 16, 1, d.get("bank", p), 16, 1, d.get("arg", p), d.get("gw", p),
                                                           d.get("N", 100), d.get("M0", 50), d.get("C", 16), d.get("n_ids", 3),
                                                           d.get("ranks", 1), d.get("gq", p), 16, 1, d.get("gk", p), 16, 1, d.get("ws", p),
                                                           d.get("ws_bytes", 1 << 20), None)
    for call in (gq, gb):
        assert call(N=0) == E_INVALID and "N=0" in _err(lib)
        assert call(M0=-1) == E_INVALID
        assert call(C=0) == E_INVALID and "C=0" in _err(lib)
        assert call(C=129) == E_INVALID and "C=129" in _err(lib)
        for bad in (0, 65):
            assert call(n_ids=bad) == E_INVALID and "n_ids=%d" % bad in _err(lib)
        for bad in (0, 9, -1):
            assert call(ranks=bad) == E_INVALID and "ranks=%d" % bad in _err(lib)
    for ptr in ("query", "bank", "arg", "gw"):
        assert gb(**{ptr: None}) == E_INVALID and "null" in _err(lib), ptr
    assert gb(gq=None, gk=None) == E_INVALID and "null" in _err(lib)
    assert gb(arg=ctypes.c_void_p(4100)) == E_INVALID and "aligned" in _err(lib)
    assert gb(ws_bytes=100 * 16 * 4 - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert gb(ws=None) == E_WORKSPACE

    def lq(**d):
        return lib.manet_local_match_train_workspace_bytes(d.get("h", 24), d.get("w", 30), d.get("C", 16), d.get("n_ids", 3), d.get("d", 4),
                                                           ctypes.byref(n))
    assert lq() == 0
    need = n.value

    def lf(**d):
        return lib.manet_local_match_train_forward_f32(d.get("prev", p), 30 * 16, 16, 1, d.get("cur", p), 30 * 16, 16, 1, d.get("labels", p),
                                                       d.get("h", 24), d.get("w", 30), d.get("C", 16), d.get("n_ids", 3), d.get("d", 4),
                                                       d.get("out", p), d.get("arg", p), d.get("vol", p), d.get("ws", p), 1 << 30, None)

    def lb(**d):
        return lib.manet_local_match_train_backward_f32(d.get("prev", p), 30 * 16, 16, 1, d.get("cur", p), 30 * 16, 16, 1, d.get("vol", p),
                                                        d.get("arg", p), d.get("g", p), d.get("h", 24), d.get("w", 30), d.get("C", 16),
                                                        d.get("n_ids", 3), d.get("d", 4), d.get("gp", p), 30 * 16, 16, 1, d.get("gc", p),
                                                        30 * 16, 16, 1, d.get("ws", p), d.get("ws_bytes", need), None)

    def lfull(**d):
        return lib.manet_local_match_full_backward_ordered_f32(d.get("prev", p), d.get("cur", p), d.get("arg", p), d.get("g", p),
                                                               d.get("h", 24), d.get("w", 30), d.get("C", 16), d.get("n_ids", 3),
                                                               d.get("d", 4), d.get("gp", p), d.get("gc", p), d.get("dv", p), None)
    for call in (lq, lf, lb, lfull):
        assert call(h=0) == E_INVALID and "h=0" in _err(lib)
        assert call(C=0) == E_INVALID
        for bad in (-1, 13):
            assert call(d=bad) == E_INVALID and "max_distance=%d" % bad in _err(lib)
        for bad in (0, 65):
            assert call(n_ids=bad) == E_INVALID and "n_ids=%d" % bad in _err(lib)
    for call in (lq, lf, lb):
        assert call(h=1) == E_INVALID and "downsample" in _err(lib)
    for call in (lq, lb, lfull):
        assert call(C=129) == E_INVALID and "C=129" in _err(lib)
    for ptr in ("prev", "cur", "labels", "out", "arg", "vol"):
        assert lf(**{ptr: None}) == E_INVALID and "null" in _err(lib), ptr
    for ptr in ("prev", "cur", "vol", "arg", "g", "ws"):
        assert lb(**{ptr: None}) == E_INVALID and "null" in _err(lib), ptr
    assert lb(gp=None, gc=None) == E_INVALID and "null" in _err(lib)
    assert lb(ws_bytes=need - 1) == E_WORKSPACE and "workspace" in _err(lib)
    for ptr in ("prev", "cur", "arg", "g", "dv"):
        assert lfull(**{ptr: None}) == E_INVALID and "null" in _err(lib), ptr
    assert lfull(gp=None, gc=None) == E_INVALID and "null" in _err(lib)


def _hipcc():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    return "/opt/rocm/bin/hipcc"


def test_new_kernels_use_no_scratch_and_spill_nothing():
    _hipcc()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(CSRC, "match_train.hip")],
                         capture_output=True, text=True, timeout=900, check=True).stdout
    rows = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if len(f) >= 7:
            rows[" ".join(f[:-6])] = [int(v) for v in f[-6:]]
    assert set(KERNELS) <= set(rows), sorted(rows)
    bad = [(k, v) for k, v in rows.items() if v[3] or v[4]]  # VGPR spill, scratch bytes per lane
    assert not bad, bad
    # the two per-cell kernels and the bank kernel keep at least two waves per SIMD, the streaming ones full occupancy
    for k in ("mt_local_cell_kernel", "mt_local_prev_kernel", "mt_global_bank_kernel<16>", "mt_global_bank_kernel<32>"):
        assert rows[k][0] + max(rows[k][1], 0) <= 128 and rows[k][5] >= 2, (k, rows[k])
    for k in ("mt_local_min_arg_kernel", "mt_global_query_kernel", "mt_pool_cl_kernel", "mt_unpool_kernel", "mt_full_dist_kernel"):
        assert rows[k][5] >= 8, (k, rows[k])


FLOAT_ATOMIC = re.compile(r"\b\w*atomic_add_f32\b|\b\w*atomic_add_f64\b|\b\w*atomic_pk_add_\w+|\bds_add_f32\b|\bds_add_rtn_f32\b|\bds_add_f64\b|"
                          r"\bds_add_rtn_f64\b|\bds_pk_add_\w+", re.I)


def test_device_assembly_of_the_new_kernels_has_no_float_atomic_add(tmp_path):
    """the Makefile's flags, device code only, to assembly: every kernel of csrc/match_train.hip is there and none of them holds a
    floating-point atomic add (global, flat, buffer or LDS; packed forms included).  Min / max and integer atomics are allowed."""
    hipcc = _hipcc()
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
             "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only"]
    asm = str(tmp_path / "match_train.s")
    subprocess.run([hipcc] + flags + [os.path.join(CSRC, "match_train.hip"), "-o", asm], check=True, capture_output=True, timeout=900)
    text = open(asm).read()
    for base in sorted({k.split("<")[0] for k in KERNELS}):
        assert re.search(r"^_Z\w*%s\w*:" % base, text, re.M), base
    code = "\n".join(line.split(";")[0] for line in text.splitlines() if not line.lstrip().startswith((".", ";")))
    hits = FLOAT_ATOMIC.findall(code)
    assert not hits, sorted(set(hits))
    # (the pattern does find what it is for: the atomic route's scatter kernels)
    assert FLOAT_ATOMIC.search("global_atomic_add_f32 v0, v[1:2], v3, off") and FLOAT_ATOMIC.search("ds_add_f32 v0, v1")
    assert FLOAT_ATOMIC.search("global_atomic_pk_add_f16 v0, v[1:2], v3, off") and not FLOAT_ATOMIC.search("ds_min_u32 v0, v1")


def test_switches():
    from cvpr2020_manet_amd import ops
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    from test_intvos_module import TinyExtractor
    cfg = make_cfg(["--MODEL_SEMANTIC_EMBEDDING_DIM", "12", "--MODEL_HEAD_EMBEDDING_DIM", "8", "--MODEL_ASPP_OUTDIM", "6"])
    plain = M.IntVOS(cfg, TinyExtractor())
    assert plain.train_match == "atomic" and M.TRAIN_MATCH == "atomic"
    model = M.IntVOS(cfg, TinyExtractor(), train_match="ordered")
    assert model.train_match == "ordered"
    assert list(model.state_dict()) == list(plain.state_dict())  # not a buffer, not in the state dict
    with pytest.raises(ValueError, match="train_match"):
        M.IntVOS(cfg, TinyExtractor(), train_match="sorted")
    cfg.MODEL_TRAIN_MATCH = "ordered"
    assert M.IntVOS(cfg, TinyExtractor()).train_match == "ordered"
    assert M.IntVOS(cfg, TinyExtractor(), train_match="atomic").train_match == "atomic"
    cfg.MODEL_TRAIN_MATCH = "fast"
    with pytest.raises(ValueError, match="train_match"):
        M.IntVOS(cfg, TinyExtractor())
    # the ops keep refusing CPU tensors, with the keyword as without it
    a = torch.rand(6, 8, 4, requires_grad=True)
    lab = torch.zeros(6, 8, dtype=torch.int32)
    for kw in ({}, {"deterministic": True}):
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.local_match(a, a, lab, 2, 2, **kw)
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.global_match(a, a, lab, 2, **kw)
    # the module-level functions take the route by keyword or from the module's TRAIN_MATCH
    with pytest.raises(ValueError, match="train_match"):
        M.local_previous_frame_nearest_neighbor_features_per_object(a, a, lab, torch.arange(2), 2, train_match="x")
