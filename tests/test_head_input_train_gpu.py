"""train_inputs="fused": the heads' input in training assembled by one launch and one autograd node (ops.head_input_train,
autograd.HeadInputFn, csrc/head_input_train.hip), and the assembly + a whole DynamicSegHead as ONE node
(ops.dynamic_seghead_train_parts, autograd.DynamicSegHeadPartsFn).  Ground truth: the framework composition the module runs
otherwise (repeat, permute, label compare, cat -- bit for bit, forward and backward: the backward's inputs are small integers, so
every sum is exact in fp32), the float64 derivative of (sigmoid(d) - 0.5) * 2 with the framework's own fp32 autograd as the
yardstick, the two-node route the one-node route must equal bit for bit, and the reference's own training step
(tests/golden/grad_tiny.npz)."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_intvos_module import TinyExtractor

pytestmark = pytest.mark.gpu

# (C, h, w, n_ids): below one wave, a multiple of 4, odd, across a 256-thread block; 64 objects once
CASES = [(1, 2, 2, 1), (5, 7, 9, 3), (12, 16, 16, 2), (12, 17, 19, 11), (5, 7, 9, 64), (5, 16, 16, 3), (1, 17, 19, 2), (12, 2, 2, 11)]
LAYOUTS = ("contiguous", "batch_slice", "hwc")


@pytest.fixture(autouse=True)
def _module_cfg_restored():
    """IntVOS(cfg, ...) installs its cfg as the module-level default of networks.IntVOS (set_cfg): put the previous one back, so
    that heads built without arguments by later tests keep the default widths"""
    from cvpr2020_manet_amd.networks import IntVOS as M
    saved = M.cfg
    yield
    M.set_cfg(saved)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def _gen(*key):
    return torch.Generator().manual_seed(1000 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def _embedding(C, h, w, layout, g):
    """a [C, h, w] fp32 tensor on the GPU in one of the layouts the module meets, no grad yet"""
    if layout == "contiguous":
        return torch.randn(C, h, w, generator=g).cuda()
    if layout == "batch_slice":
        return torch.randn(3, C, h, w, generator=g).cuda()[1]
    return torch.randn(h, w, C, generator=g).cuda().permute(2, 0, 1)  # HWC storage


def _labels(h, w, n_ids, g):
    """labels 0..n_ids-1 with the values that mark no object among them: -1, n_ids, 255"""
    lab = torch.randint(0, n_ids, (h, w, 1), generator=g, dtype=torch.int32)
    flat = lab.view(-1)
    for i, v in enumerate((-1, n_ids, 255)):
        flat[(i * 5 + 1) % flat.numel()] = v
    return lab.cuda()


def _compose(emb, maps, planes, n_ids, normalize_first=False):
    """the module's framework route (IntVOS.py:663-671, :741-758)"""
    C, h, w = emb.shape
    ids = torch.arange(0, n_ids, dtype=torch.int32, device=emb.device)
    parts = [emb.unsqueeze(0).repeat((n_ids, 1, 1, 1))]
    for j, m in enumerate(maps):
        m = m.view(1, h, w, n_ids, 1)
        if normalize_first and j == 0:
            m = (torch.sigmoid(m) - 0.5) * 2
        parts.append(m.squeeze(0).permute(2, 3, 0, 1))
    for lab in planes:
        parts.append((lab.view(h, w, 1).float() == ids.float()).unsqueeze(-1).permute(2, 3, 0, 1).float())
    return torch.cat(parts, 1)


@pytest.mark.parametrize("C,h,w,n_ids", CASES)
def test_forward_bits(ops, C, h, w, n_ids):
    g = _gen(C, h, w, n_ids)
    emb = _embedding(C, h, w, "contiguous", g)
    maps = [torch.rand(h, w, n_ids, generator=g).cuda() for _ in range(2)]
    lab, lab2 = _labels(h, w, n_ids, g), _labels(h, w, n_ids, g)
    for m, pl in ((maps, [lab]), ([], [lab, lab2]), (maps, [lab, lab2]), ([], [lab])):
        x = ops.head_input_train(emb, m, pl, n_ids)
        assert x.shape == (n_ids, C + len(m) + len(pl), h, w) and x.is_contiguous() and x.grad_fn is None
        assert torch.equal(x, _compose(emb, m, pl, n_ids))
    # the first interaction's second plane (IntVOS.py:756-758: object 0's channel 1, the others 0) is an all-zero label plane
    first = torch.zeros(n_ids, 1, h, w, device="cuda")
    first[0] = 1.0
    x = ops.head_input_train(emb, [], [lab, torch.zeros_like(lab)], n_ids)
    assert torch.equal(x[:, C + 1:], first) and torch.equal(x[:, :C + 1], _compose(emb, [], [lab], n_ids))
    # the maps may come in the match ops' view shapes
    x = ops.head_input_train(emb, [maps[0].view(1, h, w, n_ids, 1), maps[1].view(h * w, n_ids)], [lab.view(-1)], n_ids)
    assert torch.equal(x, _compose(emb, maps, [lab], n_ids))
    # normalize_first: the inference epilogue's bits, an absent object's 1e20 included
    d = torch.rand(h, w, n_ids, generator=g) * 12
    d.view(-1)[0] = 1e20
    d.view(-1)[-1] = 0.0
    d = d.cuda()
    x = ops.head_input_train(emb, [d, maps[1]], [lab], n_ids, normalize_first=True)
    want = ops.normalize_merge_(d.clone(), None, normalize=True)
    assert torch.equal(x[:, C], want.permute(2, 0, 1))
    assert torch.equal(x[:, :C], _compose(emb, [], [lab], n_ids)[:, :C])
    assert torch.equal(x[:, C + 1:], _compose(emb, [maps[1]], [lab], n_ids)[:, C:])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C,h,w,n_ids", CASES)
def test_backward_exact(ops, C, h, w, n_ids, layout):
    """grad_x of integers in [-8, 8]: a sum over at most 64 objects is exact in fp32 whatever its order, so the embedding's
    gradient and the maps' equal torch autograd through the framework composition bit for bit"""
    g = _gen(C, h, w, n_ids, 7)
    emb = _embedding(C, h, w, layout, g)
    maps = [torch.rand(h, w, n_ids, generator=g).cuda().view(1, h, w, n_ids, 1) for _ in range(2)]
    lab = _labels(h, w, n_ids, g)
    gx = torch.randint(-8, 9, (n_ids, C + 3, h, w), generator=g).float().cuda()
    leaves = [t.detach().requires_grad_(True) for t in [emb] + maps]
    assert leaves[0].stride() == emb.stride()
    want = torch.autograd.grad(_compose(leaves[0], leaves[1:], [lab], n_ids), leaves, gx)
    x = ops.head_input_train(leaves[0], leaves[1:], [lab], n_ids)
    assert "HeadInputFn" in type(x.grad_fn).__name__
    got = torch.autograd.grad(x, leaves, gx)
    for a, b, leaf in zip(got, want, leaves):
        assert a.shape == leaf.shape and torch.equal(a, b)
    # the embedding's gradient comes back in the embedding's own layout
    assert got[0].stride() == leaves[0].stride()
    # no maps, two planes (the interaction head's input): the embedding's gradient alone
    e = emb.detach().requires_grad_(True)
    gx2 = gx[:, :C + 2].contiguous()
    (ge,) = torch.autograd.grad(ops.head_input_train(e, [], [lab, lab], n_ids), [e], gx2)
    assert torch.equal(ge, gx2[:, :C].sum(0))


def test_backward_of_the_normalisation(ops):
    """d -> (sigmoid(d) - 0.5) * 2 inside the assembly: the gradient against the float64 composition through torch autograd,
    measured as max |error| / |grad_x|; the yardstick is torch's own fp32 autograd on the same inputs against the same float64
    result, and the op may be at most twice as far off (both are a handful of fp32 roundings of the same function; the factor
    covers the different formula, 0.5 (1 - y)(1 + y) in the saved y).  On the CPU, with the library's forward formula, both come
    to 1.8e-7.  A distance of 1e20 (an object absent from the bank) gives exactly 0."""
    g = _gen(3)
    d = torch.cat([torch.rand(200000, generator=g) * 12, torch.rand(50000, generator=g) * 30, torch.tensor([0.0, 30.0, 1e20])])
    n_ids, h, w, C = 13, 1, 19231, 1  # 13 * 19231 = 250003 values
    assert d.numel() == n_ids * h * w
    d = d.cuda().view(h, w, n_ids)
    gm = torch.randn(h, w, n_ids, generator=g).cuda()
    d64 = d.double().requires_grad_(True)
    (want,) = torch.autograd.grad((torch.sigmoid(d64) - 0.5) * 2, [d64], gm.double())
    d32 = d.clone().requires_grad_(True)
    (yard,) = torch.autograd.grad((torch.sigmoid(d32) - 0.5) * 2, [d32], gm)
    emb = torch.zeros(C, h, w, device="cuda")
    lab = torch.zeros(h, w, dtype=torch.int32, device="cuda")
    dm = d.clone().requires_grad_(True)
    x = ops.head_input_train(emb, [dm], [lab], n_ids, normalize_first=True)
    gx = torch.zeros_like(x)
    gx[:, C] = gm.permute(2, 0, 1)
    (got,) = torch.autograd.grad(x, [dm], gx)
    err_yard = float(((yard.double() - want).abs() / gm.double().abs()).max())
    err_op = float(((got.double() - want).abs() / gm.double().abs()).max())
    print("normalisation backward: max |error| / |grad_x|: op %.3e, torch fp32 autograd %.3e" % (err_op, err_yard))
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(x).all())
    assert float(got.view(-1)[-1]) == 0.0 and float(x.detach()[n_ids - 1, C, 0, w - 1]) == 1.0
    assert err_op <= 2 * err_yard, (err_op, err_yard)


def test_gradients_nobody_asked_for(ops):
    C, h, w, n_ids = 5, 7, 9, 3
    g = _gen(C, h, w, n_ids, 11)
    emb = _embedding(C, h, w, "contiguous", g)
    maps = [torch.rand(h, w, n_ids, generator=g).cuda() * 6 for _ in range(2)]
    lab = _labels(h, w, n_ids, g)
    gx = torch.randint(-8, 9, (n_ids, C + 3, h, w), generator=g).float().cuda()

    def run(need_emb, need_maps, normalize_first=True):
        e = emb.clone().requires_grad_(need_emb)
        m = [t.clone().requires_grad_(need_maps) for t in maps]
        x = ops.head_input_train(e, m, [lab], n_ids, normalize_first=normalize_first)
        if x.grad_fn is not None:
            x.backward(gx)
        return x, e.grad, [t.grad for t in m]
    x, ge, gm = run(True, True)
    x1, ge1, gm1 = run(False, True)  # a frozen embedding
    assert ge1 is None and all(torch.equal(a, b) for a, b in zip(gm1, gm)) and torch.equal(x1, x)
    x2, ge2, gm2 = run(True, False)  # frozen maps
    assert torch.equal(ge2, ge) and gm2 == [None, None] and torch.equal(x2, x)
    x3, ge3, gm3 = run(False, False)  # nothing to differentiate: no node
    assert x3.grad_fn is None and ge3 is None and gm3 == [None, None] and torch.equal(x3, x)
    with torch.no_grad():
        assert ops.head_input_train(emb.clone().requires_grad_(True), maps, [lab], n_ids, normalize_first=True).grad_fn is None
    # only the second map differentiated
    m1 = maps[1].clone().requires_grad_(True)
    (g1,) = torch.autograd.grad(ops.head_input_train(emb, [maps[0], m1], [lab], n_ids, normalize_first=True), [m1], gx)
    assert torch.equal(g1, gm[1]) and torch.equal(g1, gx[:, C + 1].permute(1, 2, 0))
    assert torch.equal(ge, gx[:, :C].sum(0))


def _tiny_head(in_dim, seed=1):
    from cvpr2020_manet_amd.networks import IntVOS as M
    torch.manual_seed(seed)
    head = M.DynamicSegHead(in_dim=in_dim, embed_dim=8)
    for m in head.modules():  # non-trivial BN parameters and running statistics
        if isinstance(m, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.uniform_(0.5, 1.5), m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.1, 0.1), m.running_var.uniform_(0.5, 2.0)
    return M.use_train_kernels(head.cuda().train(), "fused")


@pytest.mark.parametrize("frozen_inputs", [False, True])
def test_one_node_equals_the_two_node_route(ops, frozen_inputs):
    """ops.dynamic_seghead_train_parts against ops.dynamic_seghead_train(head, ops.head_input_train(...)): the same kernels in
    the same order -- logits, every parameter gradient, the embedding's and the maps' gradients and the running statistics are
    the same bits, on a second run too"""
    C, h, w, n_ids = 12, 7, 9, 3
    g = _gen(C, h, w, n_ids, 13)
    emb = _embedding(C, h, w, "batch_slice", g)
    maps = [torch.rand(h, w, n_ids, generator=g).cuda() * 6 for _ in range(2)]
    maps[0].view(-1)[4] = 1e20
    lab = _labels(h, w, n_ids, g)
    wl = torch.randn(n_ids, 1, h, w, generator=g).cuda()
    head = _tiny_head(C + 3)

    def step(one_node):
        hd = copy.deepcopy(head)
        e = emb.detach().requires_grad_(not frozen_inputs)
        m = [t.clone().requires_grad_(not frozen_inputs) for t in maps]
        if one_node:
            out = ops.dynamic_seghead_train_parts(hd, e, m, [lab], n_ids, normalize_first=True)
            assert "DynamicSegHeadPartsFn" in type(out.grad_fn).__name__
        else:
            out = ops.dynamic_seghead_train(hd, ops.head_input_train(e, m, [lab], n_ids, normalize_first=True))
        (out * wl).sum().backward()
        assert all(p.grad is not None for p in hd.parameters())
        if frozen_inputs:
            assert e.grad is None and m[0].grad is None and m[1].grad is None
            inputs = []
        else:
            assert e.grad.stride() == e.stride()
            inputs = [e.grad, m[0].grad, m[1].grad]
        return [out.detach()] + inputs + [p.grad for p in hd.parameters()] + [b.clone() for b in hd.buffers()]
    two, one, again = step(False), step(True), step(True)
    assert len(one) == len(two) == 1 + (0 if frozen_inputs else 3) + 34 + 8 * 3
    for a, b, c in zip(one, two, again):
        assert torch.equal(a, b) and torch.equal(a, c)
        assert bool(torch.isfinite(a.float()).all())
    assert int(one[-1]) == 1  # num_batches_tracked counted once


def _library_node_names():
    from cvpr2020_manet_amd import autograd as A
    return {name + "Backward" for name, obj in vars(A).items()
            if isinstance(obj, type) and issubclass(obj, torch.autograd.Function) and obj is not torch.autograd.Function}


def _nodes_behind_the_matches(t):
    """the graph from `t` down to -- and including -- the match nodes and the embedding head's nodes, not beyond them"""
    stops = ("Match", "BatchNormReluFn", "PointwiseConvFn", "DepthwiseConvFn")
    seen, stack, nodes = set(), [t.grad_fn], []
    while stack:
        n = stack.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        nodes.append(n)
        if not any(s in type(n).__name__ for s in stops):
            stack.extend(f for f, _ in n.next_functions)
    return nodes, stops


def _module_step(golden, train_inputs):
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    cfg = make_cfg(["--TEST_MODE", "False", "--MODEL_SEMANTIC_EMBEDDING_DIM", "12", "--MODEL_HEAD_EMBEDDING_DIM", "8",
                    "--MODEL_ASPP_OUTDIM", "6", "--MODEL_MAX_LOCAL_DISTANCE", "2"])
    model = M.IntVOS(cfg, TinyExtractor(), train_kernels="fused", train_match="ordered", train_inputs=train_inputs)
    sd = {k[4:]: torch.from_numpy(v.copy()) for k, v in golden.items() if k.startswith("sd::")}
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    nobj = int(golden["t_nobj"])
    dic = model.forward(dev(golden["t_x"]), dev(golden["t_ref_lab"]), dev(golden["t_prev_lab"]), seq_names=["clip"],
                        gt_ids=torch.Tensor([nobj]), k_nearest_neighbors=1, global_map_tmp_dic=None,
                        local_map_dics=None, interaction_num=1, start_annotated_frame=0, frame_num=[2])
    logits = dic["clip"]
    nodes, stops = _nodes_behind_the_matches(logits)
    (logits * dev(golden["t_wl"])).sum().backward()
    return logits.detach().cpu().numpy(), {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}, nodes, stops


def test_module_training_step(ops):
    """IntVOS(train_kernels="fused", train_match="ordered", train_inputs="fused") in train(): the reference's own logits and
    parameter gradients (test_autograd_gpu.py::test_training_step_through_forward_matches_reference's set-up and tolerances), ONE
    node of this library between the match nodes and the logits and none of the glue's framework nodes; "framework" gives
    today's graph and the same gradients"""
    g = load_golden("grad_tiny")
    lib = _library_node_names()
    glue = ("CatBackward", "RepeatBackward", "SigmoidBackward")
    res = {}
    for mode in ("fused", "framework"):
        logits, grads, nodes, stops = _module_step(g, mode)
        names = [type(n).__name__ for n in nodes]
        between = [n for n in names if n in lib and not any(s in n for s in stops)]
        assert any("GlobalMatchOrderedFn" in n for n in names) and any("LocalMatchOrderedFn" in n for n in names), names
        if mode == "fused":
            assert between == ["DynamicSegHeadPartsFnBackward"], names
            for key in glue:
                assert not [n for n in names if n.startswith(key)], (key, names)
        else:
            assert between == ["DynamicSegHeadFnBackward"], names
            for key in glue:
                assert [n for n in names if n.startswith(key)], (key, names)
        np.testing.assert_allclose(logits, g["t_logits"], rtol=1e-3, atol=1e-4)
        for name in g["t_grad_names"].tolist():
            want = g["t_grad::" + name]
            assert np.abs(grads[name]).max() > 0
            np.testing.assert_allclose(grads[name], want, rtol=2e-3, atol=2e-4 * max(np.abs(want).max(), 1e-6), err_msg=name)
        res[mode] = (logits, grads)
    np.testing.assert_allclose(res["fused"][0], res["framework"][0], rtol=1e-3, atol=1e-4)
    for name in g["t_grad_names"].tolist():
        want = res["framework"][1][name]
        np.testing.assert_allclose(res["fused"][1][name], want, rtol=2e-3, atol=2e-4 * max(np.abs(want).max(), 1e-6), err_msg=name)


@pytest.mark.parametrize("first_inter", [True, False])
def test_interaction_head_with_a_frozen_embedding(ops, first_inter):
    """int_seghead under grad with a frozen embedding (the stage-2 shape): no normalisation is involved and the assembled input
    is the same bits, so logits and every head parameter gradient equal the framework route's bit for bit"""
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    cfg = make_cfg(["--TEST_MODE", "False", "--MODEL_SEMANTIC_EMBEDDING_DIM", "12", "--MODEL_HEAD_EMBEDDING_DIM", "8",
                    "--MODEL_ASPP_OUTDIM", "6", "--MODEL_MAX_LOCAL_DISTANCE", "2"])
    torch.manual_seed(5)
    base = M.IntVOS(cfg, TinyExtractor(), train_kernels="fused").cuda().train()
    g = _gen(17)
    h, w, nobj = 8, 10, 2
    emb = torch.relu(torch.randn(1, 12, h, w, generator=g)).cuda()
    scribble = torch.randint(-1, nobj + 1, (1, 1, 4 * h, 4 * w), generator=g).float().cuda()
    prev_round = torch.randint(0, nobj + 1, (1, 1, 4 * h, 4 * w), generator=g).float().cuda()
    wl = torch.randn(1, nobj + 1, h, w, generator=g).cuda()
    res = {}
    for mode in ("fused", "framework"):
        model = copy.deepcopy(base)
        model.train_inputs = mode
        logits = model.int_seghead(ref_frame_embedding=emb, ref_scribble_label=scribble,
                                   prev_round_label=None if first_inter else prev_round, global_map_tmp_dic={},
                                   local_map_dics=None, interaction_num=1 if first_inter else 2, seq_names=["clip"],
                                   gt_ids=torch.Tensor([nobj]), frame_num=[0], first_inter=first_inter)["clip"]
        names = [type(n).__name__ for n in _nodes_behind_the_matches(logits)[0]]
        assert ("DynamicSegHeadPartsFnBackward" in names) == (mode == "fused"), names
        assert ("DynamicSegHeadFnBackward" in names) == (mode == "framework"), names
        (logits * wl).sum().backward()
        grads = {k: p.grad for k, p in model.inter_seghead.named_parameters()}
        assert len(grads) == 34 and all(v is not None for v in grads.values())
        res[mode] = (logits.detach(), grads)
    assert torch.equal(res["fused"][0], res["framework"][0])
    for name, v in res["fused"][1].items():
        assert torch.equal(v, res["framework"][1][name]), name
