"""CPU: what the kernels of compute="f16r" cost in registers and scratch, from the compiler's metadata in the BUILT library (the
`kernels` fixture of tests/test_f16_match_abi.py).  The fp16 filter is a wrapper of the body the bf16 filter wraps: no more
registers and no more scratch than global_match_bf16_wide_kernel<K, true> of the same build; the mode's other kernels -- the bank's
domain scan and the fp16 threshold -- use no scratch at all."""
from test_f16_match_abi import _regs, kernels  # noqa: F401  (a module-scoped fixture)


def test_fp16_filter_costs_no_more_than_the_bf16_filter(kernels):  # noqa: F811
    for K in (2, 7):
        new, old = kernels["refine_filter_half_kernel<%d>" % K], kernels["global_match_bf16_wide_kernel<%d, true>" % K]
        assert _regs(new) <= _regs(old), (K, new, old)
        assert new["private_segment_fixed_size"] <= old["private_segment_fixed_size"], (K, new, old)
        assert new["vgpr_spill_count"] <= old["vgpr_spill_count"] and new["sgpr_spill_count"] <= old["sgpr_spill_count"], (K, new, old)
    r = kernels["refine_filter_half_kernel<7>"]
    assert 512 // ((_regs(r) + 7) // 8 * 8) >= 2, r  # two workgroups per CU, as the launch plan assumes (slots = 512)


def test_the_modes_other_kernels_use_no_scratch(kernels):  # noqa: F811
    for k in ("f16_domain_kernel", "refine_threshold_f16_kernel"):
        r = kernels[k]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (k, r)
