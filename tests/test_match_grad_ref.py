"""CPU: tests/match_grad_ref.py -- the float64 restatements the GPU backward tests compare with -- against the reference's own
autograd (fixtures grad_tiny, grad_knn, grad_ds0), fed by the brute-force float64 selectors: the GPU tests must not trust a
reference that nothing checks.  Tolerances: the project's for these fixtures (tests/test_autograd_gpu.py).

Every case also asserts that no selection was decided by less than 1e-6 (the fixtures' selection is a float32 one: a float64
selector could legitimately differ at a near-tie, and a regenerated fixture must not hide a mismatch behind one).  Measured
here: smallest margin 1.0e-5 / 2.1e-3 for the local match with / without downsample, 5.5e-5 for the global match (k = 1) and
7.0e-5 for its k > 1 cases; largest |out error| 1.8e-7, largest |gradient error| 2.8e-7 on the six local cases."""
import numpy as np
import pytest
import torch

import match_grad_ref as R
from conftest import load_golden

RTOL, ATOL = 2e-4, 2e-6
MARGIN = 1e-6


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _global_case(ref, qry, lab, n_ids, k, weight, normalize, want_out, want_ref, want_qry):
    arg, wgt, _, margin = R.global_select64(ref, qry, lab, n_ids, k)
    print("global k=%d n_ids=%d: margin %.3e" % (k, n_ids, margin))
    assert margin > MARGIN
    r64, q64 = ref.double().requires_grad_(True), qry.double().requires_grad_(True)
    out = R.global_out64(R.rows_of(r64), R.rows_of(q64), arg, wgt)
    if want_out is not None:
        np.testing.assert_allclose(out.detach().numpy(), want_out.reshape(-1, n_ids), rtol=1e-5, atol=2e-6)
    res = (torch.sigmoid(out) - 0.5) * 2 if normalize else out
    gr, gq = torch.autograd.grad((res * t(weight).reshape(out.shape).double()).sum(), [r64, q64])
    np.testing.assert_allclose(gr.numpy(), want_ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gq.numpy(), want_qry, rtol=RTOL, atol=ATOL)
    if not normalize:  # the form the GPU tests use: the gradients of sum(out * gout) in one call
        gr2, gq2 = R.global64(ref, qry, arg, wgt, t(weight).reshape(out.shape))
        np.testing.assert_allclose(gr2.numpy(), want_ref, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(gq2.numpy(), want_qry, rtol=RTOL, atol=ATOL)


def test_global_restatement_reproduces_the_reference_autograd():
    g = load_golden("grad_tiny")
    ref, qry, lab = t(g["g_ref_chw"]), t(g["g_qry_chw"]), t(g["g_labels"])
    _global_case(ref, qry, lab, 4, 1, g["g_weight"], True, g["g_out"], g["g_grad_ref"], g["g_grad_qry"])
    _global_case(ref, qry, lab, 3, 1, g["g_weight_raw"], False, None, g["g_grad_ref_raw"], g["g_grad_qry_raw"])


@pytest.mark.parametrize("i", [0, 1, 2])
def test_global_knn_restatement_reproduces_the_reference_autograd(i):
    g = load_golden("grad_knn")
    assert int(g["n_cases"]) == 3
    ref, qry, lab = t(g["c%d_ref_chw" % i]), t(g["c%d_qry_chw" % i]), t(g["c%d_labels" % i])
    k, n_ids = int(g["c%d_k" % i]), int(g["c%d_n_obj" % i]) + 1
    arg, wgt, _, _ = R.global_select64(ref, qry, lab, n_ids, k)
    counts = np.bincount(g["c%d_labels" % i].reshape(-1), minlength=n_ids)
    assert (counts[:n_ids] < k).any()  # the padding rule is exercised: an object with fewer than k rows
    assert bool(((arg >= 0).sum(0) == t(np.minimum(counts[:n_ids], k))[None, :]).all())
    short = [o for o in range(n_ids) if 0 < counts[o] < k]
    for o in short:  # 1 / k per real neighbour, the replaced entries' share on the farthest
        total = wgt[:, :, o].sum(0)
        assert bool(torch.allclose(total, torch.ones_like(total))) and float(wgt[:, :, o].max()) > 1.0 / k
    _global_case(ref, qry, lab, n_ids, k, g["c%d_weight" % i], True, g["c%d_out" % i], g["c%d_grad_ref" % i],
                 g["c%d_grad_qry" % i])


@pytest.mark.parametrize("name,downsample", [("grad_tiny", True), ("grad_ds0", False)])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_local_restatement_reproduces_the_reference_autograd(name, downsample, i):
    g = load_golden(name)
    prev, cur, lab = t(g["l%d_prev_chw" % i]), t(g["l%d_cur_chw" % i]), t(g["l%d_labels" % i])
    d, n_ids = int(g["l%d_d" % i]), int(g["l%d_n_ids" % i])
    arg, margin = R.local_select64(prev, cur, lab, n_ids, d, downsample)
    winners = int((arg >= 0).sum())
    print("local %s case %d: %d winners of %d, margin %.3e" % (name, i, winners, arg.numel(), margin))
    assert winners > 0 and margin > MARGIN
    if not downsample:
        assert winners < arg.numel()  # both branches of the min
    p64, c64 = prev.double().requires_grad_(True), cur.double().requires_grad_(True)
    out = R.local_out64(p64, c64, arg, d, downsample)
    want_out = g["l%d_out" % i]
    np.testing.assert_allclose(out.detach().numpy().reshape(want_out.shape), want_out, rtol=1e-5, atol=2e-6)
    weight = t(g["l%d_weight" % i]).reshape(out.shape)
    gp, gc = torch.autograd.grad((out * weight.double()).sum(), [p64, c64])
    gp2, gc2 = R.local64(prev, cur, arg, weight, d, downsample)  # the form the GPU tests use
    scale = max(np.abs(g["l%d_grad_cur" % i]).max(), 1e-6)
    print("  max |out error| %.2e  max |gradient error| %.2e %.2e" % (
        np.abs(out.detach().numpy().reshape(want_out.shape) - want_out).max(),
        np.abs(gp.numpy() - g["l%d_grad_prev" % i]).max(), np.abs(gc.numpy() - g["l%d_grad_cur" % i]).max()))
    for got_p, got_c in ((gp, gc), (gp2, gc2)):
        np.testing.assert_allclose(got_p.numpy(), g["l%d_grad_prev" % i], rtol=RTOL, atol=2e-5 * scale)
        np.testing.assert_allclose(got_c.numpy(), g["l%d_grad_cur" % i], rtol=RTOL, atol=2e-5 * scale)


def test_cover_counts_of_the_small_sizes():
    """the most full-resolution positions one pooled position serves, sizes 2 .. 9 and the training sizes: what limits the
    winners of one pooled cell (and makes (7, 9) at d = 4 with one object a cover-limited case: 6 * 6 < 81)"""
    assert [R.max_cover(n // 2, n) for n in range(2, 10)] == [2, 3, 4, 5, 5, 6, 5, 6]
    assert all(R.max_cover(n // 2, n) == 5 for n in (12, 13, 40, 104, 120, 214, 480))
