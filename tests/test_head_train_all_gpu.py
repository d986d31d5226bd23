"""SURVEY.md 8f rank 3, finished: with train_kernels="all" a head's whole training step -- depthwise, BatchNorm + ReLU and 1x1
layers of every block and of the embedding head -- runs on HIP kernels (ops.depthwise_conv2d, ops.batch_norm_relu,
ops.pointwise_conv2d); only the heads' output conv stays the framework's.  Ground truth: a float64 copy of the head and the
reference's own training step (tests/golden/grad_tiny.npz, grad_step_alt.npz)."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_dwconv_autograd_gpu import _close, _dw_nodes, _graph_nodes, _head_pair, _tiny_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def _named(nodes, key):
    return [n for n in nodes if key in type(n).__name__]


def _framework_conv_nodes(nodes):
    return _named(nodes, "Convolution")


def _framework_bn_nodes(nodes):
    return [n for n in nodes if "BatchNorm" in type(n).__name__ and "BatchNormReluFn" not in type(n).__name__]


def test_switch_values():
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = M.DynamicSegHead(in_dim=11, embed_dim=8, train_kernels="all")
    assert head.layer1._train_kernels == "all" and head.layer4._train_kernels == "all"
    for on, want in ((True, True), (False, False), ("all", "all"), ("ALL", "all"), (1, True), (0, False)):
        M.use_train_kernels(head, on)
        assert head.layer2._train_kernels == want


def test_dynamic_seghead_all_training_step_matches_float64(ops):
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = _head_pair()
    ref = copy.deepcopy(head).double().train()
    fast = M.use_train_kernels(copy.deepcopy(head).cuda().train(), "all")
    torch.manual_seed(2)
    x = torch.randn(2, 103, 13, 17)
    wl = torch.randn(2, 1, 13, 17)
    x64 = x.double().requires_grad_(True)
    out64 = ref(x64)
    (out64 * wl.double()).sum().backward()
    xd = x.cuda().requires_grad_(True)
    out = fast(xd)
    nodes = _graph_nodes(out)
    assert len(_dw_nodes(nodes)) == 4
    assert len(_named(nodes, "PointwiseConvFn")) == 4
    assert len(_named(nodes, "BatchNormReluFn")) == 8
    assert len(_framework_conv_nodes(nodes)) == 1 and not _framework_bn_nodes(nodes)  # the output conv alone
    (out * wl.cuda()).sum().backward()
    _close(out, out64, 1e-4)
    _close(xd.grad, x64.grad, 1e-3)
    # the framework's own fp32 step bounds the parameters whose exact gradient vanishes (test_dwconv_autograd_gpu's bound)
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
    assert set(br) == set(bf)
    for name in br:
        if br[name].is_floating_point():
            _close(bf[name], br[name], 1e-5)
        else:
            assert torch.equal(bf[name].cpu(), br[name]), name


def test_true_keeps_the_framework_1x1_and_batchnorm(ops):
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = M.use_train_kernels(_head_pair(seed=3).cuda().train(), True)
    x = torch.randn(2, 103, 13, 17, device="cuda", requires_grad=True)
    nodes = _graph_nodes(head(x))
    assert len(_dw_nodes(nodes)) == 4 and not _named(nodes, "PointwiseConvFn") and not _named(nodes, "BatchNormReluFn")
    assert len(_framework_conv_nodes(nodes)) == 5 and len(_framework_bn_nodes(nodes)) == 8  # 4 x conv2 + the output conv


def test_unsupported_batchnorm_falls_back_to_the_module(ops):
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = _head_pair(seed=4)
    head.layer2.bn1.momentum = None  # cumulative moving average: the stock module
    fast = M.use_train_kernels(copy.deepcopy(head).cuda().train(), "all")
    stock = copy.deepcopy(head).cuda().train()
    x = torch.randn(2, 103, 13, 17, device="cuda", requires_grad=True)
    y = fast(x)
    nodes = _graph_nodes(y)
    assert len(_named(nodes, "BatchNormReluFn")) == 7 and len(_framework_bn_nodes(nodes)) == 1
    _close(y, stock(x), 1e-4)
    assert int(fast.layer2.bn1.num_batches_tracked) == 1
    _close(fast.layer2.bn1.running_mean, stock.layer2.bn1.running_mean, 1e-5)


def _step(blocks, x, wl):
    blocks.zero_grad(set_to_none=True)
    out = blocks(x)
    (out * wl).sum().backward()
    return [out.detach()] + [p.grad.clone() for p in blocks.parameters()] + [b.clone() for b in blocks.buffers()]


def test_two_identical_all_steps_are_bit_identical(ops):
    """every kernel of the "all" route is deterministic: two identical steps of a head's four blocks give the same bits --
    outputs, every parameter gradient, running statistics.  (The head's output conv, the framework's, is left out: its
    backward is not bit-reproducible from call to call, and every gradient upstream would inherit that.)"""
    from cvpr2020_manet_amd.networks import IntVOS as M
    head = _head_pair(in_dim=103, seed=5)
    torch.manual_seed(6)
    x = torch.randn(3, 103, 104, 104, device="cuda")
    wl = torch.randn(3, 256, 104, 104, device="cuda")
    res = []
    for _ in range(2):
        h = M.use_train_kernels(copy.deepcopy(head).cuda().train(), "all")
        blocks = torch.nn.Sequential(h.layer1, h.layer2, h.layer3, h.layer4)
        res.append(_step(blocks, x, wl))
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)


def _all_model(golden, extra=()):
    from cvpr2020_manet_amd.networks import IntVOS as M
    model = _tiny_model(golden, extra)
    M.use_train_kernels(model, "all")
    model.train_kernels = "all"
    return model


def test_extract_feature_all_routes_the_embedding_head(ops):
    g = load_golden("grad_tiny")
    model = _all_model(g)
    x = torch.from_numpy(g["t_x"].copy()).cuda()
    emb = model.extract_feature(x)
    nodes = _graph_nodes(emb)
    assert len(_dw_nodes(nodes)) == 1 and len(_named(nodes, "PointwiseConvFn")) == 1
    assert len(_named(nodes, "BatchNormReluFn")) == 2 and not _framework_bn_nodes(nodes)


def test_intvos_constructor_takes_all():
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    from test_intvos_module import TinyExtractor
    cfg = make_cfg(["--MODEL_SEMANTIC_EMBEDDING_DIM", "12", "--MODEL_HEAD_EMBEDDING_DIM", "8", "--MODEL_ASPP_OUTDIM", "6"])
    model = M.IntVOS(cfg, TinyExtractor(), train_kernels="all")
    assert model.train_kernels == "all" and model.dynamic_seghead.layer3._train_kernels == "all"
    assert M.IntVOS(cfg, TinyExtractor(), train_kernels=True).train_kernels is True
    assert M.IntVOS(cfg, TinyExtractor()).train_kernels is False


@pytest.mark.parametrize("golden,extra", [("grad_tiny", ()), ("grad_step_alt", ("--MODEL_LOCAL_DOWNSAMPLE", "False"))])
def test_training_step_with_all_matches_reference(ops, golden, extra):
    """the whole IntVOS.forward training step + backward with train_kernels="all": the reference's own logits and parameter
    gradients, at test_training_step_with_train_kernels_matches_reference's tolerances"""
    g = load_golden(golden)
    model = _all_model(g, extra)
    nobj = int(g["t_nobj"])
    knn = int(g["t_knn"]) if "t_knn" in g else 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dic = model.forward(dev(g["t_x"]), dev(g["t_ref_lab"]), dev(g["t_prev_lab"]), seq_names=["clip"],
                        gt_ids=torch.Tensor([nobj]), k_nearest_neighbors=knn, global_map_tmp_dic=None,
                        local_map_dics=None, interaction_num=1, start_annotated_frame=0, frame_num=[2])
    logits = dic["clip"]
    nodes = _graph_nodes(logits)
    assert len(_dw_nodes(nodes)) == 5 and len(_named(nodes, "PointwiseConvFn")) == 5
    assert len(_named(nodes, "BatchNormReluFn")) == 10 and not _framework_bn_nodes(nodes)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["t_logits"], rtol=1e-3, atol=1e-4)
    (logits * dev(g["t_wl"])).sum().backward()
    params = dict(model.named_parameters())
    names = g["t_grad_names"].tolist()
    for name in names:
        want = g["t_grad::" + name]
        got = params[name].grad.cpu().numpy()
        assert np.abs(got).max() > 0
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-4 * max(np.abs(want).max(), 1e-6), err_msg=name)
