"""SURVEY.md 8f rank 3, the head's half: the heads' depthwise layers in training on HIP kernels (csrc/dwconv_train.hip,
autograd.DepthwiseConvFn, ops.depthwise_conv2d, IntVOS(train_kernels=True)).  Ground truth: the same layer in float64 through
F.conv2d(groups=C) on the CPU, and the reference's own training step (tests/golden/grad_tiny.npz, grad_step_alt.npz)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_intvos_module import TinyExtractor

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 3, 5, 4), (1, 2, 3, 9), (3, 103, 13, 17), (2, 256, 104, 104), (3, 256, 120, 214)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def _close(got, want, rtol):
    want = want.detach().cpu().double().numpy()
    scale = max(float(np.abs(want).max()), 1e-30)
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), want, rtol=rtol, atol=rtol * scale)


def _case(B, C, h, w, K, seed=0):
    g = torch.Generator().manual_seed(seed + 97 * K + B + C + h + w)
    x = torch.randn(B, C, h, w, generator=g)
    wt = torch.randn(C, 1, K, K, generator=g) * 0.2
    b = torch.randn(C, generator=g)
    go = torch.randn(B, C, h, w, generator=g)
    return x, wt, b, go


def _reference(x, wt, b, go):
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, b))
    K = wt.shape[-1]
    out = F.conv2d(x64, w64, b64, padding=K // 2, groups=x.shape[1])
    gx, gw, gb = torch.autograd.grad(out, [x64, w64, b64], go.double())
    return out, gx, gw, gb


@pytest.mark.parametrize("K", [3, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_gradients_match_float64(ops, shape, K):
    x, wt, b, go = _case(*shape, K)
    out64, gx64, gw64, gb64 = _reference(x, wt, b, go)
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, wt, b))
    out = ops.depthwise_conv2d(xd, wd, bd)
    assert out.grad_fn is not None and "DepthwiseConvFn" in type(out.grad_fn).__name__
    gx, gw, gb = torch.autograd.grad(out, [xd, wd, bd], go.cuda())
    _close(out, out64, 1e-5)
    _close(gx, gx64, 1e-5)
    _close(gw, gw64, 1e-4)
    _close(gb, gb64, 1e-4)
    # without grad: the forward kernel alone, the same bits
    with torch.no_grad():
        assert torch.equal(ops.depthwise_conv2d(xd, wd, bd), out.detach())
    # no bias
    out_nb = ops.depthwise_conv2d(xd, wd)
    _close(out_nb, out64 - b.double()[None, :, None, None], 1e-5)


def test_seven_tap_forward_is_the_inference_kernel_without_bn(ops):
    x, wt, b, _ = _case(3, 103, 13, 17, 7)
    x, wt, b = x.cuda(), wt.cuda(), b.cuda()
    with torch.no_grad():
        want = ops.dwconv7x7_bn_relu(x, wt, b, relu=False)
        assert torch.equal(ops.depthwise_conv2d(x, wt, b), want)


@pytest.mark.parametrize("shape,K", [((3, 103, 13, 17), 7), ((2, 256, 104, 104), 3), ((3, 256, 120, 214), 7)])
def test_backward_weight_is_deterministic(ops, shape, K):
    x, wt, b, go = (t.cuda() for t in _case(*shape, K, seed=5))
    res = []
    for _ in range(2):
        wd, bd = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out = ops.depthwise_conv2d(x, wd, bd)
        res.append(torch.autograd.grad(out, [wd, bd], go))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def _count_calls(monkeypatch):
    from cvpr2020_manet_amd import _lib
    lib = _lib.load()
    calls = {"data": 0, "weight": 0}
    for key, name in (("data", "manet_dwconv_backward_data_f32"), ("weight", "manet_dwconv_backward_weight_f32")):
        fn = getattr(lib, name)

        def wrapped(*a, _fn=fn, _key=key):
            calls[_key] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapped)
    return calls


def test_backward_launches_only_what_is_asked_for(ops, monkeypatch):
    x, wt, b, go = _case(2, 3, 5, 4, 7, seed=9)
    out64, gx64, gw64, gb64 = _reference(x, wt, b, go)
    calls = _count_calls(monkeypatch)
    # weight only (a frozen input)
    wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    out = ops.depthwise_conv2d(x.cuda(), wd, bd)
    gw, gb = torch.autograd.grad(out, [wd, bd], go.cuda())
    assert calls == {"data": 0, "weight": 1}
    _close(gw, gw64, 1e-4)
    _close(gb, gb64, 1e-4)
    # input only (frozen weights)
    xd = x.cuda().requires_grad_(True)
    out = ops.depthwise_conv2d(xd, wt.cuda(), b.cuda())
    (gx,) = torch.autograd.grad(out, [xd], go.cuda())
    assert calls == {"data": 1, "weight": 1}
    _close(gx, gx64, 1e-5)


def _graph_nodes(t):
    seen, stack, names = set(), [t.grad_fn], []
    while stack:
        n = stack.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        names.append(n)
        stack.extend(f for f, _ in n.next_functions)
    return names


def _grouped_conv_nodes(nodes):
    return [n for n in nodes if "Convolution" in type(n).__name__ and getattr(n, "_saved_groups", 1) > 1]


def _dw_nodes(nodes):
    return [n for n in nodes if "DepthwiseConvFn" in type(n).__name__]


def _head_pair(in_dim=103, seed=1):
    from cvpr2020_manet_amd.networks import IntVOS as M
    torch.manual_seed(seed)
    head = M.DynamicSegHead(in_dim=in_dim)
    for m in head.modules():  # non-trivial BN parameters and running stats
        if isinstance(m, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1), m.running_var.uniform_(0.5, 2.0)
    return head


def test_dynamic_seghead_training_step_matches_float64(ops):
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = _head_pair()
    ref = copy.deepcopy(head).double().train()
    fast = M.use_train_kernels(copy.deepcopy(head).cuda().train())
    torch.manual_seed(2)
    x = torch.randn(2, 103, 13, 17)
    wl = torch.randn(2, 1, 13, 17)
    x64 = x.double().requires_grad_(True)
    out64 = ref(x64)
    (out64 * wl.double()).sum().backward()
    xd = x.cuda().requires_grad_(True)
    out = fast(xd)
    nodes = _graph_nodes(out)
    assert len(_dw_nodes(nodes)) == 4 and not _grouped_conv_nodes(nodes)
    (out * wl.cuda()).sum().backward()
    _close(out, out64, 1e-4)
    _close(xd.grad, x64.grad, 1e-3)
    # the framework's own fp32 step on the GPU: its rounding noise bounds the parameters whose exact gradient vanishes (a
    # conv1.bias in front of a train-mode BatchNorm: the batch mean removes it, float64 gives ~1e-13, fp32 ~1e-4)
    stock = copy.deepcopy(head).cuda().train()
    (stock(x.cuda()) * wl.cuda()).sum().backward()
    pr, pf, ps = dict(ref.named_parameters()), dict(fast.named_parameters()), dict(stock.named_parameters())
    assert set(pr) == set(pf)
    for name in pr:
        assert pf[name].grad is not None, name
        want = pr[name].grad.double()
        got = pf[name].grad.cpu().double().numpy()
        noise = float((ps[name].grad.cpu().double() - want).abs().max())
        atol = max(1e-4 * float(want.abs().max()), 8 * noise, 1e-12)
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-3, atol=atol, err_msg=name)
    br, bf = dict(ref.named_buffers()), dict(fast.named_buffers())
    for name in br:
        if br[name].is_floating_point():
            _close(bf[name], br[name], 1e-5)
        else:
            assert torch.equal(bf[name].cpu(), br[name]), name


def test_switch_off_is_the_framework_route(ops):
    head = _head_pair(seed=3).cuda().train()
    stock = copy.deepcopy(head)
    from cvpr2020_manet_amd.networks import IntVOS as M
    M.use_train_kernels(head, False)
    torch.manual_seed(4)
    x = torch.randn(2, 103, 13, 17, device="cuda")
    outs = []
    for h in (head, stock):
        xd = x.clone().requires_grad_(True)
        y = h(xd)
        nodes = _graph_nodes(y)
        assert not _dw_nodes(nodes) and len(_grouped_conv_nodes(nodes)) == 4
        y.sum().backward()
        outs.append((y.detach(), xd.grad, [p.grad for p in h.parameters()]))
    # (the framework's grouped convolution is not bit-reproducible from call to call -- its algorithm choice may change after the
    # first call -- so the values are compared at a tight tolerance; the graphs above are the route)
    for a, b in zip([outs[0][0], outs[0][1]] + outs[0][2], [outs[1][0], outs[1][1]] + outs[1][2]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6 * float(b.abs().max()))


def _tiny_model(golden, extra=()):
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    cfg = make_cfg(["--TEST_MODE", "False", "--MODEL_SEMANTIC_EMBEDDING_DIM", "12", "--MODEL_HEAD_EMBEDDING_DIM", "8",
                    "--MODEL_ASPP_OUTDIM", "6", "--MODEL_MAX_LOCAL_DISTANCE", "2"] + list(extra))
    model = M.IntVOS(cfg, TinyExtractor(), train_kernels=True)
    sd = {k[4:]: torch.from_numpy(v.copy()) for k, v in golden.items() if k.startswith("sd::")}
    model.load_state_dict(sd, strict=True)
    return model.cuda().train()


def test_extract_feature_routes_the_embedding_head(ops):
    g = load_golden("grad_tiny")
    model = _tiny_model(g)
    x = torch.from_numpy(g["t_x"].copy()).cuda()
    emb = model.extract_feature(x)
    nodes = _graph_nodes(emb)
    assert len(_dw_nodes(nodes)) == 1 and not _grouped_conv_nodes(nodes)
    # the same values as the stock module sequence
    with torch.no_grad():
        want = model.semantic_embedding(model.feature_extracter(x))
    _close(emb, want, 1e-4)


@pytest.mark.parametrize("golden,extra", [("grad_tiny", ()), ("grad_step_alt", ("--MODEL_LOCAL_DOWNSAMPLE", "False"))])
def test_training_step_with_train_kernels_matches_reference(ops, golden, extra):
    """tests/test_autograd_gpu.py's whole training steps (IntVOS.forward in train() mode + backward) with the depthwise layers on
    the HIP kernels: the reference's own logits and parameter gradients"""
    g = load_golden(golden)
    model = _tiny_model(g, extra)
    nobj = int(g["t_nobj"])
    knn = int(g["t_knn"]) if "t_knn" in g else 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dic = model.forward(dev(g["t_x"]), dev(g["t_ref_lab"]), dev(g["t_prev_lab"]), seq_names=["clip"],
                        gt_ids=torch.Tensor([nobj]), k_nearest_neighbors=knn, global_map_tmp_dic=None,
                        local_map_dics=None, interaction_num=1, start_annotated_frame=0, frame_num=[2])
    logits = dic["clip"]
    nodes = _graph_nodes(logits)
    assert len(_dw_nodes(nodes)) == 5 and not _grouped_conv_nodes(nodes)  # embedding head + the propagation head's four
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["t_logits"], rtol=1e-3, atol=1e-4)
    (logits * dev(g["t_wl"])).sum().backward()
    params = dict(model.named_parameters())
    names = g["t_grad_names"].tolist()
    assert "seperate_conv.weight" in names and "dynamic_seghead.layer1.conv1.weight" in names
    for name in names:
        want = g["t_grad::" + name]
        got = params[name].grad.cpu().numpy()
        assert np.abs(got).max() > 0
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-4 * max(np.abs(want).max(), 1e-6), err_msg=name)
