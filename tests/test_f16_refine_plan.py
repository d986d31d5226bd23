"""CPU: compute="f16r" (MANET_COMPUTE_F16_REFINE) is a refine mode like "bf16r" -- the fp16 images are the bf16 images' size, so for
every refine shape tests/test_match_plan.py covers, each field of the launch plan of the four refine forms and both workspace
totals are MANET_COMPUTE_BF16_REFINE's; check_common keeps that mode's limits (C <= 106, k_nn == 1) under the new mode's name; the
Python switches know the mode.

A host-only program that includes global_match_common.h, as tests/test_match_plan.py builds one (manet_set_error / manet_tune_get
live in manet_common.hip: the program brings its own)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_match_plan import CASES, CSRC, HIPCC

SHAPES = sorted({c[1:5] for c in CASES if c[6] == "BF16_REFINE"})  # (N, M0, C, n_ids)
FORMS = ("REFINE_PRE", "REFINE_FILTER", "REFINE_RESCUE", "REFINE_RESCUE_EXACT")

PROGRAM = r"""
#include <cstdarg>
#include <cstdio>
#include "global_match_common.h"
static char last_error[512];
int manet_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
    return code;
}
int manet_tune_get(int, int dflt) { return dflt; }
struct Shape { long N, M0; int C, n_ids; };
static const Shape shapes[] = {
%s};
static const int forms[] = {MATCH_FORM_REFINE_PRE, MATCH_FORM_REFINE_FILTER, MATCH_FORM_REFINE_RESCUE, MATCH_FORM_REFINE_RESCUE_EXACT};
static const int modes[] = {MANET_COMPUTE_BF16_REFINE, MANET_COMPUTE_F16_REFINE};
int main()
{
    printf("code %%d\n", MANET_COMPUTE_F16_REFINE);
    for (int m = 0; m < 2; ++m)
        for (const Shape &s : shapes) {
            for (int tb = -1; tb <= 1; tb += 2)  // MANET_TUNE_BLOCK_MAP unset / 1
                for (int f = 0; f < 4; ++f) {
                    const MatchPlan P = match_plan(s.N, s.M0, s.C, s.n_ids, 1, modes[m], forms[f], MatchTune{0, tb, 0});
                    printf("plan %%d | %%ld %%ld %%d %%d form=%%d tune=%%d | form=%%d k_nn=%%d steps=%%d nQT=%%d T_max=%%ld S=%%d slots=%%d block_map=0x%%x "
                           "lds=%%zu grid=%%u\n", m, s.N, s.M0, s.C, s.n_ids, forms[f], tb, P.form, P.k_nn, P.steps, P.nQT, P.T_max, P.S, P.slots,
                           (unsigned)P.block_map, P.lds, P.grid);
                    if (P.compute != modes[m]) return 1;  // (the one field that names the mode)
                }
            const BankLayout B = bank_layout(s.M0, s.C, s.n_ids, modes[m]);
            const MatchLayout M = match_layout(s.N, s.C, s.n_ids, modes[m], 1);
            printf("totals %%d | %%ld %%ld %%d %%d | bank=%%zu match=%%zu T_sub_max=%%ld off_rows=%%zu off_pack32=%%zu off_list=%%zu off_q32=%%zu "
                   "bucket_cap=%%ld\n", m, s.N, s.M0, s.C, s.n_ids, B.total, M.total, B.T_sub_max, B.off_rows, B.off_pack32, M.off_list,
                   M.off_q32, M.bucket_cap);
        }
    const int mode = MANET_COMPUTE_F16_REFINE;
    printf("check ok %%d\n", check_common(512, 4096, 106, 3, 1, mode));
    int rc = check_common(512, 4096, 107, 3, 1, mode);
    printf("check C107 %%d %%s\n", rc, last_error);
    rc = check_common(512, 4096, 100, 3, 2, mode);
    printf("check k2 %%d %%s\n", rc, last_error);
    return 0;
}
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    assert len(SHAPES) >= 2, SHAPES
    d = tmp_path_factory.mktemp("f16_refine_plan")
    src = d / "f16_refine_plan.cpp"
    src.write_text(PROGRAM % "".join("    {%d, %d, %d, %d},\n" % s for s in SHAPES))
    exe = str(d / "f16_refine_plan")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(src), "-o", exe], check=True, timeout=300)
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()


def test_plans_and_workspace_totals_are_the_bf16_refine_modes(report):
    for kind, per_shape in (("plan", 8), ("totals", 1)):
        rows = {m: [ln.split(" | ", 1)[1] for ln in report if ln.startswith("%s %d | " % (kind, m))] for m in (0, 1)}
        assert len(rows[0]) == per_shape * len(SHAPES) and rows[0] == rows[1], (kind, rows)


def test_check_common_keeps_the_refine_limits_under_the_modes_name(report):
    lines = {ln.split(" ", 2)[1]: ln.split(" ", 2)[2] for ln in report if ln.startswith("check ")}
    assert lines["ok"] == "0"
    assert re.match(r"-1 MANET_COMPUTE_F16_REFINE supports C <= 106", lines["C107"]), lines
    assert re.match(r"-1 k_nn > 1 needs MANET_COMPUTE_F32", lines["k2"]), lines


def test_python_switches(report):
    from cvpr2020_manet_amd import _lib, ops
    code = int([ln for ln in report if ln.startswith("code ")][0].split()[1])
    assert ops.COMPUTE["f16r"] == _lib.COMPUTE_F16_REFINE == code
    assert ops._image_kind(code) == _lib.COMPUTE_F16 and code in _lib.REFINE_MODES and _lib.COMPUTE_BF16_REFINE in _lib.REFINE_MODES
    for args in (("manet_match_workspace_bytes", 700, 3000, 100, 3, 1), ("manet_bank_workspace_bytes", 3000, 100, 3),
                 ("manet_query_pack_bytes", 700, 100)):
        assert _lib.query(*args, code) == _lib.query(*args, _lib.COMPUTE_BF16_REFINE) > 0, args
    with pytest.raises(RuntimeError, match="MANET_COMPUTE_F16_REFINE supports C <= 106"):
        _lib.query("manet_bank_workspace_bytes", 3000, 107, 3, code)
    from test_intvos_module import TinyExtractor, tiny_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    saved = M.cfg  # (building an IntVOS installs its cfg as the module-level default)
    try:
        assert M.IntVOS(tiny_cfg(), TinyExtractor(), compute="f16r").compute == "f16r"
        cfg = tiny_cfg()
        cfg.MODEL_MATCH_COMPUTE = "f16r"
        assert M.IntVOS(cfg, TinyExtractor()).compute == "f16r"
    finally:
        M.set_cfg(saved)


def test_training_in_the_mode_keeps_raising():
    import torch
    from cvpr2020_manet_amd import ops
    q = torch.zeros(4, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="backward exists for compute='f32'"):
        ops.global_match(torch.zeros(4, 8), q, torch.zeros(4, dtype=torch.int32), 1, compute="f16r")
