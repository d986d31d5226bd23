"""the heads' BatchNorm + ReLU pairs in training on HIP kernels (csrc/pw_train.hip,
autograd.BatchNormReluFn, ops.batch_norm_relu).  Ground truth: nn.BatchNorm2d + ReLU in float64 on the CPU."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (n = 2 per channel is left out: its exact input gradient is ~eps-sized cancellation noise, in float64 too)
SHAPES = [(2, 5, 3, 1), (2, 8, 10, 13), (3, 103, 13, 17), (3, 256, 104, 104), (2, 100, 120, 214)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def _close(got, want, rtol):
    want = want.detach().cpu().double().numpy()
    scale = max(float(np.abs(want).max()), 1e-30)
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), want, rtol=rtol, atol=rtol * scale)


def _case(B, C, h, w, momentum, seed=0):
    g = torch.Generator().manual_seed(seed + B + 3 * C + h + w)
    bn = torch.nn.BatchNorm2d(C, momentum=momentum)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(C, generator=g) * 0.4 - 0.2)
        bn.running_mean.copy_(torch.rand(C, generator=g) * 0.2 - 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) * 1.5 + 0.5)
    # per-channel offsets and scales, so the statistics are not all ~(0, 1)
    x = torch.randn(B, C, h, w, generator=g) * (torch.rand(C, 1, 1, generator=g) * 3 + 0.1) \
        + torch.randn(C, 1, 1, generator=g) * 2
    go = torch.randn(B, C, h, w, generator=g)
    return bn, x, go


def _reference(bn, x, go):
    ref = copy.deepcopy(bn).double()
    x64 = x.double().requires_grad_(True)
    out = torch.relu(ref(x64))
    gx, gw, gb = torch.autograd.grad(out, [x64, ref.weight, ref.bias], go.double())
    return ref, out, gx, gw, gb


def _check(ops, bn, x, go, training):
    bn = bn.train(training)
    ref, out64, gx64, gw64, gb64 = _reference(bn, x, go)
    fast = copy.deepcopy(bn).cuda()
    xd = x.cuda().requires_grad_(True)
    out = ops.batch_norm_relu(xd, fast)
    assert out.grad_fn is not None and "BatchNormReluFn" in type(out.grad_fn).__name__
    gx, gw, gb = torch.autograd.grad(out, [xd, fast.weight, fast.bias], go.cuda())
    _close(out, out64, 1e-5)
    _close(gx, gx64, 1e-4)
    _close(gw, gw64, 1e-4)
    _close(gb, gb64, 1e-4)
    _close(fast.running_mean, ref.running_mean, 1e-6)
    _close(fast.running_var, ref.running_var, 1e-6)
    assert int(fast.num_batches_tracked) == int(ref.num_batches_tracked)


@pytest.mark.parametrize("momentum", [0.0003, 0.1])
@pytest.mark.parametrize("shape", SHAPES)
def test_training_matches_float64(ops, shape, momentum):
    bn, x, go = _case(*shape, momentum)
    _check(ops, bn, x, go, True)


@pytest.mark.parametrize("shape", SHAPES[1:4])
def test_eval_with_grad_uses_the_running_statistics(ops, shape):
    bn, x, go = _case(*shape, 0.1, seed=1)
    before = (bn.running_mean.clone(), bn.running_var.clone())
    _check(ops, bn, x, go, False)
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])


def test_a_zero_gamma_channel(ops):
    bn, x, go = _case(3, 103, 13, 17, 0.1, seed=2)
    with torch.no_grad():
        bn.weight[5] = 0.0
        bn.weight[17] = 0.0
        bn.bias[17] = 0.3  # (gamma 0, beta > 0: the output is beta, every gradient still flows into d_gamma)
    _check(ops, bn, x, go, True)


def test_without_grad_same_bits_and_running_update(ops):
    bn, x, go = _case(3, 103, 104, 104, 0.1, seed=4)
    a, b = copy.deepcopy(bn).cuda(), copy.deepcopy(bn).cuda()
    xd = x.cuda()
    with_grad = ops.batch_norm_relu(xd.clone().requires_grad_(True), a)
    with torch.no_grad():
        without = ops.batch_norm_relu(xd, b)
    assert torch.equal(with_grad.detach(), without)
    assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)


@pytest.mark.parametrize("shape", [(3, 256, 104, 104), (2, 100, 120, 214)])
def test_two_runs_are_bit_identical(ops, shape):
    bn, x, go = _case(*shape, 0.0003, seed=6)
    res = []
    for _ in range(2):
        m = copy.deepcopy(bn).cuda()
        xd = x.cuda().requires_grad_(True)
        out = ops.batch_norm_relu(xd, m)
        res.append([out.detach(), m.running_mean, m.running_var] + list(torch.autograd.grad(out, [xd, m.weight, m.bias], go.cuda())))
    for a, c in zip(res[0], res[1]):
        assert torch.equal(a, c)


def test_one_value_per_channel_raises_what_batchnorm_raises(ops):
    bn = torch.nn.BatchNorm2d(4).cuda()
    x = torch.randn(1, 4, 1, 1, device="cuda", requires_grad=True)
    with pytest.raises(ValueError) as stock:
        bn(x)
    with pytest.raises(ValueError) as ours:
        ops.batch_norm_relu(x, bn)
    assert str(ours.value) == str(stock.value)
    bn.eval()  # (eval mode takes one value per channel)
    torch.testing.assert_close(ops.batch_norm_relu(x, bn), torch.relu(bn(x)))


def test_unsupported_batchnorm_is_refused(ops):
    x = torch.randn(2, 4, 3, 3, device="cuda")
    for bn in (torch.nn.BatchNorm2d(4, affine=False), torch.nn.BatchNorm2d(4, track_running_stats=False),
               torch.nn.BatchNorm2d(4, momentum=None)):
        assert not ops.batch_norm_relu_ok(bn)
        with pytest.raises(ValueError):
            ops.batch_norm_relu(x, bn.cuda())
