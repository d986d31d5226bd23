"""CPU: register / scratch budget of the fp16 stored-volume kernels, from the compiler's own resource report (the method of
test_kernel_resources.py).  `local_fused_f16_kernel<D, MODE>` takes a `_Float16 *`, which older demanglers leave mangled: the
kernels are found by their mangled template arguments instead of the demangled name.

Budgets are those test_kernel_resources.py pins for the fp32 siblings `local_fused_kernel<D, 1>` / `<D, 2>` (the fp16 forms share
their body, thread count and LDS plan, with half the image): no scratch and no VGPR spill at any window radius, at d = 12 and d = 4
the fp32 kernels' registers-per-lane and occupancy steps."""
import os
import re

import pytest

import test_kernel_resources as tkr


@pytest.fixture(scope="module")
def f16_kernels():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    out = {}
    for mangled, row in tkr._report("local_fused.hip").items():
        m = re.search(r"local_fused_f16_kernelILi(\d+)ELi(\d+)EE", mangled)
        if m:
            out[(int(m.group(1)), int(m.group(2)))] = row
    return out


def test_every_window_radius_has_both_f16_kernels_without_scratch(f16_kernels):
    assert sorted(f16_kernels) == [(d, mode) for d in range(13) for mode in (1, 2)], sorted(f16_kernels)
    for key, r in f16_kernels.items():
        assert r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0, (key, r)
        assert r.get("VGPRs", 0) <= 256, (key, r)


def test_f16_kernels_keep_the_register_budget_of_their_fp32_siblings(f16_kernels):
    for key in ((12, 1), (12, 2), (4, 1), (4, 2)):
        regs, occ = tkr.HOT["local_fused_kernel<%d, %d>" % key]
        r = f16_kernels[key]
        assert r.get("VGPRs", 0) + r.get("AGPRs", 0) <= regs and r.get("Occupancy [waves/SIMD]", 0) >= occ, (key, r)
