"""compute="f16" against the fp32 REFERENCE formula on unrounded embeddings, at full size: the structure of
test_bf16_error_bound.py (BASELINE configs[2] and [4], whole frame, fp32 embeddings handed to every mode, figures on the
normalised maps (sigmoid(d) - 0.5) * 2 the segmentation head consumes).

fp16 keeps 11 significand bits where bf16 keeps 8, so the input-rounding error is expected 8x smaller; rounding-only
simulation in fp64 (2 048 queries x 128 400 rows, C = 100): 7.6e-5 at scale 0.1 and 1.4e-4 at scale 0.3, where bf16 has 6.5e-4
and 1.2e-3.  Asserted: inside the 1e-3 bar at BOTH scales (bf16 leaves it at 0.3), and at most a quarter of bf16's error on the
same tensors -- the 8x of the three extra bits, with a factor 2 left for the maximum over 10^5..10^6 samples.

Measured on MI355X (normalised max |err|, f16 / bf16):   scale 0.1                  scale 0.3
    cfg3                                                  9.9e-5 / 7.0e-4 (7.1x)     1.5e-4 / 1.4e-3 (9.2x)
    cfg5                                                  1.0e-4 / 9.1e-4 (9.1x)     1.8e-4 / 1.7e-3 (9.2x)
(the table with raw errors and arg-min flips is in DESIGN.md 4)"""
import pytest
import torch

from test_bf16_error_bound import TOL, _inputs, _norm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


@pytest.mark.parametrize("cfg", [3, 5])
@pytest.mark.parametrize("scale", [0.1, 0.3])
def test_f16_error_vs_fp32_reference_at_full_size(ops, cfg, scale):
    q, bank, lab, n_ids = _inputs(cfg, scale)
    ref = ops.global_match(bank, q, lab, n_ids, compute="f32")  # bit-exact against the oracle (test_bf16_error_bound.py checks it here)
    refn = _norm(ref)
    errs = {}
    for mode in ("f16", "bf16"):
        got = ops.global_match(bank, q, lab, n_ids, compute=mode)
        errs[mode] = ((_norm(got) - refn).abs().max().item(), (got - ref).abs().max().item(),
                      (got.argmin(1) != ref.argmin(1)).float().mean().item())
    print("cfg%d scale %.1f: (normalised max err, raw max err, arg-min id flips) %s" % (cfg, scale, errs))
    assert errs["f16"][0] <= TOL
    assert errs["f16"][0] <= errs["bf16"][0] / 4
