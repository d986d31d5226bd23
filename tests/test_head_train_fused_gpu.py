"""train_kernels="fused": a whole DynamicSegHead -- four blocks and the output conv, forward and backward -- behind ONE autograd node
(ops.dynamic_seghead_train, autograd.DynamicSegHeadFn, csrc/head_train.hip), deterministic end to end, and the output conv on its
own HIP kernels (ops.output_conv1x1).  Ground truth: a float64 copy of the head, the block-by-block "all" route where the two run
the same kernels, and the reference's own training step (tests/golden/grad_tiny.npz, grad_step_alt.npz).  Tolerances are those of
test_head_train_all_gpu.py / test_pw_train_gpu.py."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_dwconv_autograd_gpu import _close, _dw_nodes, _graph_nodes, _head_pair, _tiny_model

pytestmark = pytest.mark.gpu

OTHER_NODES = ("Convolution", "BatchNorm", "DepthwiseConvFn", "PointwiseConvFn", "BatchNormReluFn")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def _named(nodes, key):
    return [n for n in nodes if key in type(n).__name__]


def _framework_bn_nodes(nodes):
    return [n for n in nodes if "BatchNorm" in type(n).__name__ and "BatchNormReluFn" not in type(n).__name__]


def _assert_one_node(out):
    nodes = _graph_nodes(out)
    assert len(_named(nodes, "DynamicSegHeadFn")) == 1
    for key in OTHER_NODES:
        assert not _named(nodes, key), key


def test_the_head_is_one_node(ops):
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = M.use_train_kernels(_head_pair(seed=3).cuda().train(), "fused")
    x = torch.randn(2, 103, 13, 17, device="cuda", requires_grad=True)
    _assert_one_node(head(x))
    # a frozen input: still one node (the parameters want gradients)
    _assert_one_node(head(x.detach()))


def _float64_step(head, x, wl, eval_mode):
    ref = copy.deepcopy(head).double()
    ref = ref.eval() if eval_mode else ref.train()
    x64 = x.double().requires_grad_(True)
    out64 = ref(x64)
    (out64 * wl.double()).sum().backward()
    return ref, x64, out64


@pytest.mark.parametrize("eval_mode", [False, True])
def test_dynamic_seghead_fused_training_step_matches_float64(ops, eval_mode):
    """test_dynamic_seghead_all_training_step_matches_float64's body with "fused" -- the output conv's gradients included -- in
    train() mode and in eval() with grad enabled (running statistics used and left alone, bit for bit)"""
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = _head_pair()
    mode = (lambda m: m.eval()) if eval_mode else (lambda m: m.train())
    torch.manual_seed(2)
    x = torch.randn(2, 103, 13, 17)
    wl = torch.randn(2, 1, 13, 17)
    ref, x64, out64 = _float64_step(head, x, wl, eval_mode)
    fast = M.use_train_kernels(mode(copy.deepcopy(head).cuda()), "fused")
    before = {k: v.clone() for k, v in fast.named_buffers()}
    xd = x.cuda().requires_grad_(True)
    out = fast(xd)
    _assert_one_node(out)
    (out * wl.cuda()).sum().backward()
    _close(out, out64, 1e-4)
    _close(xd.grad, x64.grad, 1e-3)
    # the framework's own fp32 step bounds the parameters whose exact gradient vanishes (test_dwconv_autograd_gpu's bound)
    stock = mode(copy.deepcopy(head).cuda())
    (stock(x.cuda()) * wl.cuda()).sum().backward()
    pr, pf, ps = dict(ref.named_parameters()), dict(fast.named_parameters()), dict(stock.named_parameters())
    assert set(pr) == set(pf) and len(pf) == 34 and "conv.weight" in pf and "conv.bias" in pf
    for name in pr:
        assert pf[name].grad is not None, name
        want = pr[name].grad.double()
        got = pf[name].grad.cpu().double().numpy()
        noise = float((ps[name].grad.cpu().double() - want).abs().max())
        atol = max(1e-4 * float(want.abs().max()), 8 * noise, 1e-12)
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-3, atol=atol, err_msg=name)
    br, bf = dict(ref.named_buffers()), dict(fast.named_buffers())
    assert set(br) == set(bf)
    for name in br:
        if br[name].is_floating_point():
            _close(bf[name], br[name], 1e-5)
        else:
            assert torch.equal(bf[name].cpu(), br[name]), name
        if eval_mode:
            assert torch.equal(bf[name], before[name]), name


def test_frozen_input_gives_the_same_parameter_gradients(ops):
    """x.requires_grad == False (stage 2: the embedding is frozen): no gradient for x, every parameter gradient has the bits of the
    run where x wants its gradient -- and matches float64 like that run; likewise with some parameters frozen"""
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = _head_pair()
    torch.manual_seed(2)
    x = torch.randn(2, 103, 13, 17)
    wl = torch.randn(2, 1, 13, 17)
    ref, _, out64 = _float64_step(head, x, wl, False)
    grads = {}
    for want_x in (True, False):
        fast = M.use_train_kernels(copy.deepcopy(head).cuda().train(), "fused")
        xd = x.cuda().requires_grad_(want_x)
        out = fast(xd)
        (out * wl.cuda()).sum().backward()
        _close(out, out64, 1e-4)
        assert (xd.grad is not None) == want_x
        grads[want_x] = {k: p.grad for k, p in fast.named_parameters()}
    for name, g in grads[True].items():
        assert torch.equal(g, grads[False][name]), name
    # frozen parameters: no gradient for them, the same bits for the others
    fast = M.use_train_kernels(copy.deepcopy(head).cuda().train(), "fused")
    frozen = ("layer1.conv1.weight", "layer2.bn1.bias", "layer3.conv2.weight", "conv.bias")
    for name, p in fast.named_parameters():
        p.requires_grad_(name not in frozen)
    (fast(x.cuda()) * wl.cuda()).sum().backward()
    for name, p in fast.named_parameters():
        if name in frozen:
            assert p.grad is None, name
        else:
            assert torch.equal(p.grad, grads[True][name]), name


def _step(head, x, wl):
    head.zero_grad(set_to_none=True)
    xd = x.clone().requires_grad_(True)
    out = head(xd)
    (out * wl).sum().backward()
    return [out.detach(), xd.grad] + [p.grad.clone() for p in head.parameters()] + [b.clone() for b in head.buffers()]


def test_two_identical_fused_steps_are_bit_identical_end_to_end(ops):
    """the sentence test_two_identical_all_steps_are_bit_identical could not write: two identical steps of the WHOLE head, output
    conv included, give the same bits -- logits, x.grad, all 34 parameter gradients, all buffers"""
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = _head_pair(in_dim=103, seed=5)
    torch.manual_seed(6)
    x = torch.randn(3, 103, 104, 104, device="cuda")
    wl = torch.randn(3, 1, 104, 104, device="cuda")
    res = []
    for _ in range(2):
        h = M.use_train_kernels(copy.deepcopy(head).cuda().train(), "fused")
        _assert_one_node(h(x.clone().requires_grad_(True)))
        h = M.use_train_kernels(copy.deepcopy(head).cuda().train(), "fused")
        res.append(_step(h, x, wl))
    assert len(res[0]) == 2 + 34 + 8 * 3
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
        assert bool(torch.isfinite(a.float()).all())


def test_forward_agrees_with_the_all_route_where_the_kernels_are_the_same(ops):
    """one step from the same state: the seven BatchNorms in front of layer 4's bn2 see the same kernels in the same order under
    "all" and "fused", so their running statistics are equal bit for bit; the logits agree to fp32 rounding"""
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = _head_pair(in_dim=103, seed=7)
    torch.manual_seed(8)
    x = torch.randn(3, 103, 52, 60, device="cuda")
    outs, bufs = {}, {}
    for mode in ("all", "fused"):
        h = M.use_train_kernels(copy.deepcopy(head).cuda().train(), mode)
        outs[mode] = h(x.clone().requires_grad_(True)).detach()
        bufs[mode] = dict(h.named_buffers())
    n = 0
    for name, b in bufs["all"].items():
        if name.startswith("layer4.bn2."):
            if b.is_floating_point():
                _close(bufs["fused"][name], b, 1e-5)
            continue
        assert torch.equal(bufs["fused"][name], b), name
        n += 1
    assert n == 7 * 3
    _close(outs["fused"], outs["all"], 1e-4)


def _oc_case(B, C, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + B + C + h + w)
    x = torch.randn(B, C, h, w, generator=g)
    wt = torch.randn(1, C, 1, 1, generator=g) / C ** 0.5
    b = torch.randn(1, generator=g)
    go = torch.randn(B, 1, h, w, generator=g)
    return x, wt, b, go


@pytest.mark.parametrize("shape", [(2, 8, 13, 17), (3, 256, 104, 104)])
def test_output_conv_matches_float64_and_is_deterministic(ops, shape):
    x, wt, b, go = _oc_case(*shape)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, b))
    out64 = F.conv2d(x64, w64, b64)
    gx64, gw64, gb64 = torch.autograd.grad(out64, [x64, w64, b64], go.double())
    res = []
    for _ in range(2):
        xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, wt, b))
        out = ops.output_conv1x1(xd, wd, bd)
        assert out.grad_fn is not None and "OutputConvFn" in type(out.grad_fn).__name__
        gx, gw, gb = torch.autograd.grad(out, [xd, wd, bd], go.cuda())
        _close(out, out64, 1e-5)
        _close(gx, gx64, 1e-5)
        _close(gw, gw64, 1e-4)
        _close(gb, gb64, 1e-4)
        res.append((out.detach(), gx, gw, gb))
    for a, c in zip(res[0], res[1]):
        assert torch.equal(a, c)
    # without grad: the forward kernel alone, the same bits; no bias
    with torch.no_grad():
        assert torch.equal(ops.output_conv1x1(x.cuda(), wt.cuda(), b.cuda()), res[0][0])
    _close(ops.output_conv1x1(x.cuda(), wt.cuda()), out64 - b.double(), 1e-5)
    # only what is asked for: a frozen input, a frozen layer
    wd, bd = wt.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    gw, gb = torch.autograd.grad(ops.output_conv1x1(x.cuda(), wd, bd), [wd, bd], go.cuda())
    assert torch.equal(gw, res[0][2]) and torch.equal(gb, res[0][3])
    xd = x.cuda().requires_grad_(True)
    (gx,) = torch.autograd.grad(ops.output_conv1x1(xd, wt.cuda(), b.cuda()), [xd], go.cuda())
    assert torch.equal(gx, res[0][1])


def test_ineligible_layer_falls_back_block_by_block_with_the_output_conv_on_hip(ops):
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = _head_pair(seed=4)
    head.layer2.bn1.momentum = None  # cumulative moving average: the stock module
    fast = M.use_train_kernels(copy.deepcopy(head).cuda().train(), "fused")
    stock = copy.deepcopy(head).cuda().train()
    x = torch.randn(2, 103, 13, 17, device="cuda", requires_grad=True)
    y = fast(x)
    nodes = _graph_nodes(y)
    assert not _named(nodes, "DynamicSegHeadFn")
    assert len(_named(nodes, "BatchNormReluFn")) == 7 and len(_framework_bn_nodes(nodes)) == 1
    assert len(_dw_nodes(nodes)) == 4 and len(_named(nodes, "PointwiseConvFn")) == 4
    assert len(_named(nodes, "OutputConvFn")) == 1 and not _named(nodes, "Convolution")
    _close(y, stock(x), 1e-4)
    y.sum().backward()
    assert x.grad is not None and all(p.grad is not None for p in fast.parameters())


def _fused_model(golden, extra=()):
    from cvpr2020_manet_amd.networks import IntVOS as M
    model = _tiny_model(golden, extra)
    M.use_train_kernels(model, "fused")
    model.train_kernels = "fused"
    return model


def test_extract_feature_under_fused_is_the_all_route(ops):
    g = load_golden("grad_tiny")
    model = _fused_model(g)
    x = torch.from_numpy(g["t_x"].copy()).cuda()
    nodes = _graph_nodes(model.extract_feature(x))
    assert len(_dw_nodes(nodes)) == 1 and len(_named(nodes, "PointwiseConvFn")) == 1
    assert len(_named(nodes, "BatchNormReluFn")) == 2 and not _framework_bn_nodes(nodes)


@pytest.mark.parametrize("golden,extra", [("grad_tiny", ()), ("grad_step_alt", ("--MODEL_LOCAL_DOWNSAMPLE", "False"))])
def test_training_step_with_fused_matches_reference(ops, golden, extra):
    """test_training_step_with_all_matches_reference's body with train_kernels="fused": the reference's own logits and parameter
    gradients; the propagation head is one node, the embedding head goes the "all" route"""
    g = load_golden(golden)
    model = _fused_model(g, extra)
    nobj = int(g["t_nobj"])
    knn = int(g["t_knn"]) if "t_knn" in g else 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dic = model.forward(dev(g["t_x"]), dev(g["t_ref_lab"]), dev(g["t_prev_lab"]), seq_names=["clip"],
                        gt_ids=torch.Tensor([nobj]), k_nearest_neighbors=knn, global_map_tmp_dic=None,
                        local_map_dics=None, interaction_num=1, start_annotated_frame=0, frame_num=[2])
    logits = dic["clip"]
    nodes = _graph_nodes(logits)
    assert len(_named(nodes, "DynamicSegHeadFn")) == 1
    assert len(_dw_nodes(nodes)) == 1 and len(_named(nodes, "PointwiseConvFn")) == 1  # the embedding head's
    assert len(_named(nodes, "BatchNormReluFn")) == 2 and not _framework_bn_nodes(nodes)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["t_logits"], rtol=1e-3, atol=1e-4)
    (logits * dev(g["t_wl"])).sum().backward()
    params = dict(model.named_parameters())
    names = g["t_grad_names"].tolist()
    for name in names:
        want = g["t_grad::" + name]
        got = params[name].grad.cpu().numpy()
        assert np.abs(got).max() > 0
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-4 * max(np.abs(want).max(), 1e-6), err_msg=name)
