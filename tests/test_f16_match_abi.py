"""CPU: the C ABI and the Python switches of compute="f16" (MANET_COMPUTE_F16 = 4), and the register budget of its kernels.

The mode reuses the plain-bf16 mode's operand geometry -- tiles, workspaces, launch plan -- so every size query answers with
MANET_COMPUTE_BF16's number; what differs is the element type inside the images (tests/test_f16_match_gpu.py)."""
import re
import subprocess

import pytest

from cvpr2020_manet_amd import _lib, ops

CS = [20, 100, 107, 128]  # 2 k-steps, 7, and the narrow kernel's 9 on both sides of it


@pytest.mark.parametrize("C", CS)
def test_workspace_sizes_are_the_bf16_modes(C):
    for N, M0, n_ids in ((130, 120, 2), (25680, 128400, 4)):
        for args in (("manet_match_workspace_bytes", N, M0, C, n_ids, 1), ("manet_global_match_workspace_bytes", N, M0, C, n_ids, 1),
                     ("manet_bank_workspace_bytes", M0, C, n_ids), ("manet_query_pack_bytes", N, C)):
            assert _lib.query(*args, _lib.COMPUTE_F16) == _lib.query(*args, _lib.COMPUTE_BF16) > 0, args
    for h, w, d in ((13, 10, -1), (120, 214, 12)):
        assert (_lib.query("manet_frame_workspace_bytes", h, w, C, _lib.COMPUTE_F16, d)
                == _lib.query("manet_frame_workspace_bytes", h, w, C, _lib.COMPUTE_BF16, d) > 0)


def test_unknown_code_is_refused_and_the_message_lists_the_mode():
    for args in (("manet_match_workspace_bytes", 130, 120, 100, 2, 1), ("manet_bank_workspace_bytes", 120, 100, 2),
                 ("manet_query_pack_bytes", 130, 100), ("manet_frame_workspace_bytes", 13, 10, 100)):
        tail = (-1,) if args[0] == "manet_frame_workspace_bytes" else ()
        with pytest.raises(RuntimeError, match=r"compute=5 .*_F16"):
            _lib.query(*args, 5, *tail)
    with pytest.raises(RuntimeError, match="k_nn > 1 needs MANET_COMPUTE_F32"):
        _lib.query("manet_match_workspace_bytes", 130, 120, 100, 2, 2, _lib.COMPUTE_F16)


def test_python_switches():
    assert _lib.COMPUTE_F16 == 4 and ops.COMPUTE["f16"] == 4 and ops.COMPUTE["fp16"] == 4
    assert ops._image_kind(_lib.COMPUTE_F16) == _lib.COMPUTE_F16 != ops._image_kind(_lib.COMPUTE_BF16)
    assert ops._image_kind(_lib.COMPUTE_BF16_REFINE) == _lib.COMPUTE_BF16  # (unchanged)
    from test_intvos_module import TinyExtractor, tiny_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    saved = M.cfg  # (building an IntVOS installs its cfg as the module-level default)
    try:
        assert M.IntVOS(tiny_cfg(), TinyExtractor(), compute="f16").compute == "f16"
        cfg = tiny_cfg()
        cfg.MODEL_MATCH_COMPUTE = "f16"
        assert M.IntVOS(cfg, TinyExtractor()).compute == "f16"
        with pytest.raises(ValueError, match="compute="):
            M.IntVOS(tiny_cfg(), TinyExtractor(), compute="f8")
    finally:
        M.set_cfg(saved)


def test_training_in_the_mode_keeps_raising():
    import torch
    q = torch.zeros(4, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="backward exists for compute='f32'"):
        ops.global_match(torch.zeros(4, 8), q, torch.zeros(4, dtype=torch.int32), 1, compute="f16")


@pytest.fixture(scope="module")
def kernels():
    """kernel name -> the metadata the compiler wrote into the BUILT library's gfx950 code objects (registers, private segment,
    spills): what the resource remarks of tests/test_kernel_resources.py print, for the same flags (the Makefile's), read back from
    the library that runs instead of compiling the sources once more"""
    import os
    import struct
    import tempfile
    tools = "/opt/rocm/llvm/bin/"
    if not os.path.exists(tools + "llvm-readelf"):
        pytest.skip("no llvm-readelf")
    _lib.load()
    magic, out = b"__CLANG_OFFLOAD_BUNDLE__", {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([tools + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, _lib.LIB_PATH], check=True)
        blob = open(fat, "rb").read()
        for s in [m.start() for m in re.finditer(re.escape(magic), blob)]:  # one bundle per source file
            (count,) = struct.unpack_from("<Q", blob, s + len(magic))
            p = s + len(magic) + 8
            for _ in range(count):
                off, size, tl = struct.unpack_from("<QQQ", blob, p)
                triple = blob[p + 24:p + 24 + tl].decode()
                p += 24 + tl
                if "gfx950" not in triple or size == 0:
                    continue
                co = os.path.join(d, "code.o")
                open(co, "wb").write(blob[s + off:s + off + size])
                notes = subprocess.run([tools + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
                cur = {}
                for line in notes.splitlines():  # amdhsa.kernels: one map per kernel, keys in alphabetical order
                    m = re.match(r"\s*(- )?\.(\w+):\s*(\S*)", line)
                    if not m:
                        continue
                    if m.group(1) and m.group(2) == "agpr_count":  # a kernel's first key
                        cur = {}
                    cur[m.group(2)] = m.group(3).strip("'")
                    if m.group(2) == "symbol":
                        out[m.group(3).strip("'")[:-3]] = cur  # (without ".kd"; the keys behind .symbol still land in cur)
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.splitlines()
    res = {}
    for k, n in zip(out, names):
        res[re.sub(r"\(.*", "", re.sub(r"\(anonymous namespace\)::|^void ", "", n))] = {a: int(b) for a, b in out[k].items() if b.isdigit()}
    assert len(res) > 80, len(res)
    return res


def _regs(r):
    return r["vgpr_count"] + r.get("agpr_count", 0)


def test_fp16_kernels_budget(kernels):
    """the fp16 wide kernel at 7 k-steps: at most 256 VGPR + AGPR per lane, i.e. two waves per SIMD of a CU's 512 registers per
    lane (granule 8), no scratch, no spill; the 2-step and the 9-step (narrow) forms: no scratch"""
    r = kernels["f16_match_wide_kernel<7>"]
    assert _regs(r) <= 256 and 512 // ((_regs(r) + 7) // 8 * 8) >= 2, r
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    for k in ("f16_match_wide_kernel<2>", "f16_match_pipe_kernel<9>"):
        assert kernels[k]["private_segment_fixed_size"] == 0 and kernels[k]["vgpr_spill_count"] == 0, (k, kernels[k])
    # ... and the wrappers share the bf16 kernels' bodies: the same registers
    assert _regs(r) == _regs(kernels["global_match_bf16_wide_kernel<7, false>"])
    assert _regs(kernels["f16_match_pipe_kernel<9>"]) == _regs(kernels["global_match_bf16_pipe_kernel<9>"])


def test_the_library_carries_exactly_these_fp16_kernels(kernels):
    """the mode's kernels are named f16_* / *_f16_*, outside the global_match_* / frame_prepare_* families whose members
    tests/test_cabi_symbols.py lists one by one: this is THEIR list -- one wide kernel per wide k-step count, the narrow one, and
    the bank / query pack for the two storage types; frame_prepare_kernel picks the fp16 image at run time"""
    have = sorted(k for k in kernels if "f16" in k.replace("bf16", "") and re.search("match|pack_rows|frame_prepare", k))
    want = sorted(["f16_match_wide_kernel<2>", "f16_match_wide_kernel<7>", "f16_match_pipe_kernel<9>"] +
                  ["pack_rows_f16_kernel<%s, %s>" % (r, t) for r in ("64, 64", "32, 32") for t in ("float", "unsigned short")])
    assert have == want, (have, want)
