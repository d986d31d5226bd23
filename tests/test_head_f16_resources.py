"""CPU: register / scratch budget of the head_act="f16" kernels, from the compiler's own resource report (the method of
test_kernel_resources.py / test_local_volume_f16_resources.py: the kernels take `_Float16 *`, which older demanglers leave
mangled, so they are found by their mangled names)."""
import os
import re

import pytest

import test_kernel_resources as tkr

# kernel -> (registers per lane, waves per SIMD) as the compile reports them (DESIGN 3 quotes the rows)
PW = {(False, False): (159, 3), (True, False): (161, 3), (False, True): (159, 3)}  # <HEAD, OUT32>


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    dw, pw, pack = {}, {}, []
    for mangled, row in tkr._report("seg_head.hip").items():
        m = re.search(r"dwconv7x7_bn_relu_f16_kernelILb([01])EE", mangled)
        if m:
            dw[bool(int(m.group(1)))] = row
        m = re.search(r"conv1x1_f16_kernelILb([01])ELb([01])EE", mangled)
        if m:
            pw[(bool(int(m.group(1))), bool(int(m.group(2))))] = row
        if "conv1x1_f16_pack_kernel" in mangled:
            pack.append(row)
    return dw, pw, pack


def _clean(r):
    return r.get("VGPRs Spill", 0) == 0 and r.get("ScratchSize [bytes/lane]", 0) == 0 and r.get("VGPRs", 0) + r.get("AGPRs", 0) <= 256


def test_every_f16_head_kernel_is_there_without_scratch_or_spill(rows):
    dw, pw, pack = rows
    assert sorted(dw) == [False, True] and sorted(pw) == sorted(PW) and len(pack) == 1
    for r in list(dw.values()) + list(pw.values()) + pack:
        assert _clean(r), r


def test_f16_depthwise_keeps_its_fp32_siblings_occupancy(rows):
    regs, occ = tkr.HOT["dwconv7x7_bn_relu_kernel<true, false, true>"]
    for in16, r in rows[0].items():
        assert r.get("VGPRs", 0) + r.get("AGPRs", 0) <= regs and r.get("Occupancy [waves/SIMD]", 0) >= occ, (in16, r)


def test_f16_pointwise_registers_and_occupancy_are_pinned(rows):
    for key, (regs, occ) in PW.items():
        r = rows[1][key]
        assert r.get("VGPRs", 0) + r.get("AGPRs", 0) <= regs and r.get("Occupancy [waves/SIMD]", 0) >= occ, (key, r)
        assert r.get("LDS Size [bytes/block]", 0) <= 160 * 1024 // 3  # three workgroups per CU
