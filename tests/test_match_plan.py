"""CPU: the launch plan of the global-match kernels (match_plan, cvpr2020_manet_amd/csrc/global_match_common.h) -- query tiles,
split count, the `block_map` word, dynamic LDS bytes, grid -- for a table of shapes, forms and tune values, and the workspace
totals of the same shapes (ABI).  Every block map gives the same bits (tests/test_block_map.py), so a wrong plan shows only as
time on the GPU: this test is what sees it.

The header holds no kernel, so a host-only program that includes it compiles in a second or two and runs without a GPU.

EXPECTED was printed by the commit BEFORE the plan existed, from that commit's own pick_splits / block_map_arg / layouts, combined
as each entry point and launcher combined them (split count, the bank-bytes hint set in front of the launch, the tune keys read
where they were read).  It is not regenerated from the code under test: a change of a figure here is a change of a launch."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cvpr2020_manet_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# (label, N, M0, C, n_ids, k_nn, compute, form, (MANET_TUNE_SPLITS, MANET_TUNE_BLOCK_MAP, MANET_TUNE_ONE_ROUND; unset = 0, -1, 0), expected)
#   small16 / small100: the smallest banks at which the automatic map leaves 0 (S = 16 is the first count with S / 8 >= 2);
#   480p5: the 480p five-frame bank; scribble: a scribble-sized bank, the one-round case; c120: fp32 KS = 64, bf16 pipe (256 slots)
CASES = [
    ("small16 f32", 256, 4096, 16, 2, 1, "F32", "MAIN", (0, -1, 0),
     "nQT=1 T_max=66 S=16 slots=512 block_map=0x20020004 lds=18432 grid=16 bank_total=626688 match_total=35840"),
    ("small16 arg", 256, 4096, 16, 2, 1, "F32", "ARG", (0, -1, 0),
     "nQT=1 T_max=66 S=16 slots=512 block_map=0x20004 lds=18432 grid=16 bank_total=626688 match_total=39936"),
    ("small100 f32", 512, 4096, 100, 3, 1, "F32", "MAIN", (0, -1, 0),
     "nQT=2 T_max=67 S=16 slots=512 block_map=0x20010004 lds=55296 grid=32 bank_total=1870848 match_total=221184"),
    ("small100 bf16", 512, 4096, 100, 3, 1, "BF16", "MAIN", (0, -1, 0),
     "nQT=1 T_max=67 S=16 slots=512 block_map=0x20004 lds=57344 grid=16 bank_total=978944 match_total=120832"),
    ("small100 refine pre", 512, 4096, 100, 3, 1, "BF16_REFINE", "REFINE_PRE", (0, -1, 0),
     "nQT=1 T_max=12 S=8 slots=512 block_map=0x20000 lds=57344 grid=8 bank_total=4737024 match_total=1928192"),
    ("small100 refine filter", 512, 4096, 100, 3, 1, "BF16_REFINE", "REFINE_FILTER", (0, -1, 0),
     "nQT=1 T_max=67 S=16 slots=512 block_map=0x20008 lds=77824 grid=40 bank_total=4737024 match_total=1928192"),
    ("small100 refine rescue", 512, 4096, 100, 3, 1, "BF16_REFINE", "REFINE_RESCUE", (0, -1, 0),
     "nQT=2 T_max=67 S=16 slots=512 block_map=0x40000000 lds=55296 grid=32 bank_total=4737024 match_total=1928192"),
    ("small100 refine rescue exact", 512, 4096, 100, 3, 1, "BF16_REFINE", "REFINE_RESCUE_EXACT", (0, -1, 0),
     "nQT=2 T_max=67 S=16 slots=512 block_map=0x10004 lds=55296 grid=32 bank_total=4737024 match_total=1928192"),
    ("480p5 f32", 51360, 256800, 100, 3, 1, "F32", "MAIN", (0, -1, 0),
     "nQT=201 T_max=4016 S=24 slots=512 block_map=0x20000200 lds=55296 grid=4824 bank_total=112075776 match_total=22228992"),
    ("480p5 bf16", 51360, 256800, 100, 3, 1, "BF16", "MAIN", (0, -1, 0),
     "nQT=101 T_max=4016 S=48 slots=512 block_map=0x504 lds=57344 grid=4848 bank_total=58614784 match_total=12204032"),
    ("480p5 bf16x3", 51360, 256800, 100, 3, 1, "BF16X3", "MAIN", (0, -1, 0),
     "nQT=101 T_max=4016 S=48 slots=256 block_map=0x200 lds=57344 grid=4848 bank_total=116188160 match_total=23787520"),
    ("480p5 f32 k5", 51360, 256800, 100, 3, 5, "F32", "MAIN", (0, -1, 0),
     "nQT=201 T_max=4016 S=16 slots=512 block_map=0x200 lds=55296 grid=3216 bank_total=112075776 match_total=101265408"),
    ("480p5 arg", 51360, 256800, 100, 3, 1, "F32", "ARG", (0, -1, 0),
     "nQT=201 T_max=4016 S=24 slots=512 block_map=0x200 lds=55296 grid=4824 bank_total=112075776 match_total=23463936"),
    ("480p5 nth arg", 51360, 256800, 100, 3, 1, "F32", "NTH_ARG", (0, -1, 0),
     "nQT=201 T_max=4016 S=24 slots=512 block_map=0x200 lds=55296 grid=4824 bank_total=112075776 match_total=23463936"),
    ("480p5 refine pre", 51360, 256800, 100, 3, 1, "BF16_REFINE", "REFINE_PRE", (0, -1, 0),
     "nQT=101 T_max=255 S=48 slots=512 block_map=0x505 lds=57344 grid=4848 bank_total=277143552 match_total=194658304"),
    ("480p5 refine filter", 51360, 256800, 100, 3, 1, "BF16_REFINE", "REFINE_FILTER", (0, -1, 0),
     "nQT=101 T_max=4016 S=48 slots=512 block_map=0x508 lds=77824 grid=7272 bank_total=277143552 match_total=194658304"),
    ("480p5 refine rescue", 51360, 256800, 100, 3, 1, "BF16_REFINE", "REFINE_RESCUE", (0, -1, 0),
     "nQT=202 T_max=4016 S=16 slots=512 block_map=0x40000000 lds=55296 grid=3232 bank_total=277143552 match_total=194658304"),
    ("480p5 refine rescue exact", 51360, 256800, 100, 3, 1, "BF16_REFINE", "REFINE_RESCUE_EXACT", (0, -1, 0),
     "nQT=202 T_max=4016 S=24 slots=512 block_map=0x200 lds=55296 grid=4848 bank_total=277143552 match_total=194658304"),
    ("n2500 f32", 2500, 40000, 100, 5, 1, "F32", "MAIN", (0, -1, 0),
     "nQT=10 T_max=630 S=128 slots=512 block_map=0x20003305 lds=55296 grid=1280 bank_total=17584128 match_total=1126400"),
    ("n2500 bf16", 2500, 40000, 100, 5, 1, "BF16", "MAIN", (0, -1, 0),
     "nQT=5 T_max=630 S=152 slots=512 block_map=0x6605 lds=57344 grid=760 bank_total=9197568 match_total=624640"),
    ("n2500 f32 k5", 2500, 40000, 100, 5, 5, "F32", "MAIN", (0, -1, 0),
     "nQT=10 T_max=630 S=16 slots=512 block_map=0x3304 lds=55296 grid=160 bank_total=17584128 match_total=7680000"),
    ("n2500 arg", 2500, 40000, 100, 5, 1, "F32", "ARG", (0, -1, 0),
     "nQT=10 T_max=630 S=128 slots=512 block_map=0x3305 lds=55296 grid=1280 bank_total=17584128 match_total=1228800"),
    ("n2500 nth arg", 2500, 40000, 100, 5, 1, "F32", "NTH_ARG", (0, -1, 0),
     "nQT=10 T_max=630 S=128 slots=512 block_map=0x3305 lds=55296 grid=1280 bank_total=17584128 match_total=1228800"),
    ("scribble f32", 103680, 17000, 100, 2, 1, "F32", "MAIN", (0, -1, 0),
     "nQT=405 T_max=268 S=24 slots=512 block_map=0x20000105 lds=55296 grid=9720 bank_total=7480320 match_total=44375040"),
    ("scribble bf16", 103680, 17000, 100, 2, 1, "BF16", "MAIN", (0, -1, 0),
     "nQT=203 T_max=268 S=40 slots=512 block_map=0x205 lds=57344 grid=8120 bank_total=3912704 match_total=24113152"),
    ("c120 f32", 51360, 256800, 120, 3, 1, "F32", "MAIN", (0, -1, 0),
     "nQT=201 T_max=4016 S=24 slots=512 block_map=0x20000200 lds=67584 grid=4824 bank_total=136750080 match_total=27168768"),
    ("c120 bf16", 51360, 256800, 120, 3, 1, "BF16", "MAIN", (0, -1, 0),
     "nQT=101 T_max=4016 S=48 slots=256 block_map=0x200 lds=73728 grid=4848 bank_total=75064320 match_total=15513600"),
    ("c120 bf16x3", 51360, 256800, 120, 3, 1, "BF16X3", "MAIN", (0, -1, 0),
     "nQT=101 T_max=4016 S=48 slots=256 block_map=0x200 lds=73728 grid=4848 bank_total=149087232 match_total=30406656"),
    ("c120 f32 k5", 51360, 256800, 120, 3, 5, "F32", "MAIN", (0, -1, 0),
     "nQT=201 T_max=4016 S=16 slots=512 block_map=0x200 lds=67584 grid=3216 bank_total=136750080 match_total=106205184"),
    ("empty bank f32", 1000, 0, 100, 1, 1, "F32", "MAIN", (0, -1, 0),
     "nQT=4 T_max=1 S=8 slots=512 block_map=0x20008000 lds=55296 grid=32 bank_total=29696 match_total=434176"),
    ("tune splits=36 480p5 f32", 51360, 256800, 100, 3, 1, "F32", "MAIN", (36, -1, 0),
     "nQT=201 T_max=4016 S=40 slots=512 block_map=0x20000200 lds=55296 grid=8040 bank_total=112075776 match_total=22228992"),
    ("tune splits=36 480p5 arg", 51360, 256800, 100, 3, 1, "F32", "ARG", (36, -1, 0),
     "nQT=201 T_max=4016 S=24 slots=512 block_map=0x200 lds=55296 grid=4824 bank_total=112075776 match_total=23463936"),
    ("tune block_map=1 480p5 f32", 51360, 256800, 100, 3, 1, "F32", "MAIN", (0, 1, 0),
     "nQT=201 T_max=4016 S=24 slots=512 block_map=0x20000201 lds=55296 grid=4824 bank_total=112075776 match_total=22228992"),
    ("tune block_map=0 480p5 bf16", 51360, 256800, 100, 3, 1, "BF16", "MAIN", (0, 0, 0),
     "nQT=101 T_max=4016 S=48 slots=512 block_map=0x500 lds=57344 grid=4848 bank_total=58614784 match_total=12204032"),
    ("tune block_map=1 480p5 refine filter", 51360, 256800, 100, 3, 1, "BF16_REFINE", "REFINE_FILTER", (0, 1, 0),
     "nQT=101 T_max=4016 S=48 slots=512 block_map=0x501 lds=77824 grid=4848 bank_total=277143552 match_total=194658304"),
    ("tune block_map=1 480p5 refine rescue exact", 51360, 256800, 100, 3, 1, "BF16_REFINE", "REFINE_RESCUE_EXACT", (0, 1, 0),
     "nQT=202 T_max=4016 S=24 slots=512 block_map=0x201 lds=55296 grid=4848 bank_total=277143552 match_total=194658304"),
    ("tune one_round=1 scribble f32", 103680, 17000, 100, 2, 1, "F32", "MAIN", (0, -1, 1),
     "nQT=405 T_max=268 S=24 slots=512 block_map=0x105 lds=55296 grid=9720 bank_total=7480320 match_total=44375040"),
    ("tune one_round=1 scribble bf16", 103680, 17000, 100, 2, 1, "BF16", "MAIN", (0, -1, 1),
     "nQT=203 T_max=268 S=40 slots=512 block_map=0x205 lds=57344 grid=8120 bank_total=3912704 match_total=24113152"),
]

PROGRAM = """
#include <cstdio>
#include "global_match_common.h"
struct Case { const char *label; long N, M0; int C, n_ids, k_nn, compute, form; MatchTune tune; };
static const Case cases[] = {
%s};
int main()
{
    for (const Case &c : cases) {
        const MatchPlan P = match_plan(c.N, c.M0, c.C, c.n_ids, c.k_nn, c.compute, c.form, c.tune);
        printf("%%s: nQT=%%d T_max=%%ld S=%%d slots=%%d block_map=0x%%x lds=%%zu grid=%%u bank_total=%%zu match_total=%%zu\\n", c.label, P.nQT,
               P.T_max, P.S, P.slots, (unsigned)P.block_map, P.lds, P.grid, bank_layout(c.M0, c.C, c.n_ids, c.compute).total,
               match_layout(c.N, c.C, c.n_ids, c.compute, c.k_nn, c.form == MATCH_FORM_ARG || c.form == MATCH_FORM_NTH_ARG).total);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("match_plan")
    rows = "".join('    {"%s", %d, %d, %d, %d, %d, MANET_COMPUTE_%s, MATCH_FORM_%s, {%d, %d, %d}},\n' % (c[:8] + c[8]) for c in CASES)
    src = d / "match_plan.cpp"
    src.write_text(PROGRAM % rows)
    exe = str(d / "match_plan")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(src), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout
    return dict(line.split(": ", 1) for line in out.splitlines())


def test_every_plan_is_the_one_the_entry_points_computed_before_the_plan_existed(plans):
    assert sorted(plans) == sorted(c[0] for c in CASES)
    bad = [(c[0], plans[c[0]], c[9]) for c in CASES if plans[c[0]] != c[9]]
    assert not bad, "\n".join("%s:\n  got      %s\n  expected %s" % b for b in bad)


def test_anchor_plans(plans):
    """split count and map word (the ONE_ROUND_OK flag, bit 29, aside) of the shapes the benchmark and the reference driver run"""
    def s_map(label):
        f = dict(kv.split("=") for kv in plans[label].split())
        return int(f["S"]), int(f["block_map"], 16) & ~(1 << 29)
    assert s_map("small16 f32") == (16, 0x20004)
    assert s_map("480p5 f32") == (24, 0x200)
    assert s_map("480p5 bf16") == (48, 0x504)
    assert s_map("n2500 f32") == (128, 0x3305)
    assert s_map("scribble f32") == (24, 0x105)
