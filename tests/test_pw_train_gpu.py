"""the heads' 1x1 convolutions in training on HIP kernels (csrc/pw_train.hip, autograd.PointwiseConvFn,
ops.pointwise_conv2d).  Ground truth: the same layer in float64 through F.conv2d on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, h, w): the tiny test models' head (Cout 8, 10 x 13), layer 1 (Cin 102 / 103), the 256-channel blocks on the
# inference kernel (Cout 256, h*w % 4 == 0) and off it (h*w odd), the embedding conv (Cout 100), the output-conv width (Cout 1)
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 8, 10, 13), (2, 8, 8, 10, 13), (2, 102, 256, 10, 13), (3, 103, 256, 104, 104),
          (2, 256, 100, 13, 17), (1, 256, 1, 5, 4), (2, 256, 256, 104, 104), (3, 256, 256, 120, 214)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def _close(got, want, rtol):
    want = want.detach().cpu().double().numpy()
    scale = max(float(np.abs(want).max()), 1e-30)
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), want, rtol=rtol, atol=rtol * scale)


def _case(B, Cin, Cout, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + B + 7 * Cin + 13 * Cout + h + w)
    x = torch.randn(B, Cin, h, w, generator=g)
    wt = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    b = torch.randn(Cout, generator=g)
    go = torch.randn(B, Cout, h, w, generator=g)
    return x, wt, b, go


def _reference(x, wt, b, go):
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, b))
    out = F.conv2d(x64, w64, b64)
    gx, gw, gb = torch.autograd.grad(out, [x64, w64, b64], go.double())
    return out, gx, gw, gb


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_gradients_match_float64(ops, shape):
    x, wt, b, go = _case(*shape)
    out64, gx64, gw64, gb64 = _reference(x, wt, b, go)
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, wt, b))
    out = ops.pointwise_conv2d(xd, wd, bd)
    assert out.grad_fn is not None and "PointwiseConvFn" in type(out.grad_fn).__name__
    gx, gw, gb = torch.autograd.grad(out, [xd, wd, bd], go.cuda())
    assert gw.shape == wd.shape and gb.shape == bd.shape and gx.shape == xd.shape
    _close(out, out64, 1e-5)
    _close(gx, gx64, 1e-5)
    _close(gw, gw64, 1e-4)
    _close(gb, gb64, 1e-4)
    with torch.no_grad():  # without grad: the forward kernel alone, the same bits
        assert torch.equal(ops.pointwise_conv2d(xd, wd, bd), out.detach())
    out_nb = ops.pointwise_conv2d(xd, wd)
    _close(out_nb, out64 - b.double()[None, :, None, None], 1e-5)


def test_non_contiguous_input(ops):
    x, wt, b, go = _case(2, 103, 256, 13, 17, seed=3)
    out64, gx64, gw64, gb64 = _reference(x, wt, b, go)
    base = x.permute(0, 2, 3, 1).contiguous().cuda()  # NHWC storage, NCHW view
    xd = base.permute(0, 3, 1, 2).requires_grad_(True)
    assert not xd.is_contiguous()
    wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    out = ops.pointwise_conv2d(xd, wd, bd)
    gx, gw, gb = torch.autograd.grad(out, [xd, wd, bd], go.cuda())
    _close(out, out64, 1e-5)
    _close(gx, gx64, 1e-5)
    _close(gw, gw64, 1e-4)
    _close(gb, gb64, 1e-4)


@pytest.mark.parametrize("shape", [(2, 3, 8, 10, 13), (3, 103, 256, 104, 104), (3, 256, 256, 120, 214)])
def test_two_runs_are_bit_identical(ops, shape):
    x, wt, b, go = (t.cuda() for t in _case(*shape, seed=5))
    res = []
    for _ in range(2):
        xd, wd, bd = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out = ops.pointwise_conv2d(xd, wd, bd)
        res.append((out.detach(),) + torch.autograd.grad(out, [xd, wd, bd], go))
    for a, c in zip(res[0], res[1]):
        assert torch.equal(a, c)


def _count_calls(monkeypatch):
    from cvpr2020_manet_amd import _lib
    lib = _lib.load()
    calls = {"data": 0, "weight": 0}
    for key, name in (("data", "manet_pw_backward_data_f32"), ("weight", "manet_pw_backward_weight_f32")):
        fn = getattr(lib, name)

        def wrapped(*a, _fn=fn, _key=key):
            calls[_key] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapped)
    return calls


def test_backward_launches_only_what_is_asked_for(ops, monkeypatch):
    x, wt, b, go = _case(2, 3, 8, 10, 13, seed=9)
    out64, gx64, gw64, gb64 = _reference(x, wt, b, go)
    calls = _count_calls(monkeypatch)
    wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    out = ops.pointwise_conv2d(x.cuda(), wd, bd)  # frozen input
    gw, gb = torch.autograd.grad(out, [wd, bd], go.cuda())
    assert calls == {"data": 0, "weight": 1}
    _close(gw, gw64, 1e-4)
    _close(gb, gb64, 1e-4)
    xd = x.cuda().requires_grad_(True)
    out = ops.pointwise_conv2d(xd, wt.cuda(), b.cuda())  # frozen weights
    (gx,) = torch.autograd.grad(out, [xd], go.cuda())
    assert calls == {"data": 1, "weight": 1}
    _close(gx, gx64, 1e-5)
    bd = b.cuda().requires_grad_(True)
    out = ops.pointwise_conv2d(x.cuda(), wt.cuda(), bd)  # bias only
    (gb,) = torch.autograd.grad(out, [bd], go.cuda())
    assert calls == {"data": 1, "weight": 2}
    _close(gb, gb64, 1e-4)
