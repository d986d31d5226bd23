"""CPU: register / scratch budget of head_layer1_object_f16_kernel (head_act="f16", layer 1's per-object half in one launch), from
the compiler's own resource report -- the method of test_kernel_resources.py / test_head_f16_resources.py (the kernel takes
`_Float16 *`: found by its mangled name)."""
import os

import pytest

import test_kernel_resources as tkr

REGS, WAVES = 168, 3  # registers per lane and waves per SIMD as the compile reports them (DESIGN 3 quotes the row)


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    return [r for name, r in tkr._report("seg_head.hip").items() if "head_layer1_object_f16_kernel" in name]


def test_the_kernel_is_there_once_without_scratch_or_spill(rows):
    assert len(rows) == 1
    r = rows[0]
    assert r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs Spill", 0) == 0, r
    assert r.get("VGPRs", 0) + r.get("AGPRs", 0) <= 256, r


def test_registers_occupancy_and_lds_are_pinned(rows):
    r = rows[0]
    assert r.get("VGPRs", 0) + r.get("AGPRs", 0) <= REGS and r.get("Occupancy [waves/SIMD]", 0) >= WAVES, r
    # 256 threads = one wave per SIMD per workgroup: WAVES workgroups per CU share its 160 KiB of LDS
    assert r.get("LDS Size [bytes/block]", 0) <= 160 * 1024 // WAVES, r
