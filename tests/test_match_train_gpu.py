"""GPU: the ordered (atomic-free) training route of the matching path -- ops.global_match / ops.local_match(deterministic=True),
IntVOS(train_match="ordered"), csrc/match_train.hip.

  * forward: the same bits as the default route and as the no-grad inference kernel, the same recorded selection;
  * gradients: the reference's own autograd (fixtures grad_tiny, grad_knn, grad_ds0) at tests/test_autograd_gpu.py's tolerances;
    at the training size against a float64 restatement that takes the selection from the op's recorded `arg`, the ordered route
    held to within 2x of the default (atomic) route's error measured on the same inputs;
  * five backward calls from the same inputs give the same bits (i.i.d. inputs and a collision-heavy case);
  * a whole IntVOS training step with train_kernels="fused", train_match="ordered" and the fused loss is bit-reproducible behind
    the encoder; a frozen operand gets None and leaves the other gradient's bits alone."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from match_grad_ref import global64 as _global64, local64 as _local64
from test_intvos_module import TinyExtractor

pytestmark = pytest.mark.gpu
RTOL, ATOL = 2e-4, 2e-6  # tests/test_autograd_gpu.py's
C, D = 100, 12
SIZES = [(104, 104), (120, 214)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.requires_grad_(True) if grad else t


def blobs(h, w, n_ids, g):
    cy, cx = torch.rand(n_ids, generator=g) * h, torch.rand(n_ids, generator=g) * w
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    return ((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2).argmin(0).to(torch.int32)


def iid(h, w, n_ids, seed, c=C):
    """relu(randn) * 0.1 embeddings (C-major, as the head writes them) with blob labels"""
    g = torch.Generator().manual_seed(seed)
    ref, prev, cur = [(torch.relu(torch.randn(c, h, w, generator=g)) * 0.1).cuda() for _ in range(3)]
    return ref, prev, cur, blobs(h, w, n_ids, g).cuda(), blobs(h, w, n_ids, g).cuda()


def colliding(h, w, n_ids, seed):
    """every query nearest to ONE bank row per object; one label over the whole previous frame, whose pixels are near-copies of
    one vector (the window minimum collides on few cells)"""
    g = torch.Generator().manual_seed(seed)
    base = torch.relu(torch.randn(C, 1, 1, generator=g)) * 0.1
    cur = (base + 0.003 * torch.randn(C, h, w, generator=g)).cuda()
    ref = (base + 1.0 + torch.rand(C, h, w, generator=g))
    lab = blobs(h, w, n_ids, g)
    for o in range(n_ids):
        ys, xs = torch.nonzero(lab == o, as_tuple=True)
        ref[:, ys[len(ys) // 2], xs[len(xs) // 2]] = base[:, 0, 0] + 0.001 * o
    prev = (base + 0.003 * torch.randn(C, h, w, generator=g))
    prev[:, h // 2, w // 2] = base[:, 0, 0]
    return ref.cuda(), prev.cuda(), cur, lab.cuda(), torch.ones(h, w, dtype=torch.int32).cuda()


def hwc(t):
    return t.permute(1, 2, 0)


def saved(out, dtype=torch.int32):
    return [t for t in out.grad_fn.saved_tensors if t.dtype == dtype]


def rel_err(got, want64):
    return float((got.double() - want64).abs().max() / want64.abs().max())


# ----------------------------------------------------------------------------------------------------------------- forward

def _local_forward_case(ops, prev, cur, lab, n_ids, d):
    from cvpr2020_manet_amd.autograd import LocalMatchFn, LocalMatchOrderedFn
    p, c = prev.clone().requires_grad_(True), cur.clone().requires_grad_(True)
    a = ops.local_match(hwc(p), hwc(c), lab, n_ids, d)
    b = ops.local_match(hwc(p), hwc(c), lab, n_ids, d, deterministic=True)
    assert type(a.grad_fn).__name__.startswith(LocalMatchFn.__name__ + "Backward")
    assert type(b.grad_fn).__name__.startswith(LocalMatchOrderedFn.__name__ + "Backward")
    with torch.no_grad():
        plain = ops.local_match(hwc(prev), hwc(cur), lab, n_ids, d, deterministic=True)
    assert torch.equal(b.detach(), a.detach()) and torch.equal(b.detach(), plain)
    assert torch.equal(saved(b)[0], saved(a)[0])  # the recorded winning offsets
    assert torch.equal(saved(b, torch.float32)[-1], saved(a, torch.float32)[-1])  # and the volume kept for the backward
    return saved(b)[0]


@pytest.mark.parametrize("d", [0, 2, 12])
@pytest.mark.parametrize("size", SIZES)
def test_local_forward_is_bit_equal_at_the_training_sizes(ops, size, d):
    h, w = size
    for n_ids, seed in ((3, 1), (5, 2)):
        _, prev, cur, _, lab = iid(h, w, n_ids, seed)
        arg = _local_forward_case(ops, prev, cur, lab, n_ids, d)
        assert int((arg >= 0).sum()) > 0
    _, prev, cur, _, lab = colliding(h, w, 3, 3)
    _local_forward_case(ops, prev, cur, lab, 3, d)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_local_forward_is_bit_equal_at_the_golden_sizes(ops, i):
    g = load_golden("grad_tiny")
    prev, cur = dev(g["l%d_prev_chw" % i]), dev(g["l%d_cur_chw" % i])
    lab, d, n_ids = dev(g["l%d_labels" % i]), int(g["l%d_d" % i]), int(g["l%d_n_ids" % i])
    _local_forward_case(ops, prev, cur, lab, n_ids, d)
    # many ids (more than one pass of the kernel's four)
    lab9 = torch.randint(0, 9, lab.shape, device="cuda", dtype=torch.int32, generator=torch.Generator(device="cuda").manual_seed(i))
    _local_forward_case(ops, prev, cur, lab9, 9, d)


# ------------------------------------------------------------------------------------- gradients: the reference's own autograd

def test_global_fixture_gradients_through_the_ordered_route(ops):
    g = load_golden("grad_tiny")
    ref, qry = dev(g["g_ref_chw"], True), dev(g["g_qry_chw"], True)
    lab = dev(g["g_labels"])
    out = ops.global_match(hwc(ref), hwc(qry), lab, 4, normalize=True, deterministic=True)
    with torch.no_grad():
        assert torch.equal(out.detach(), ops.global_match(hwc(ref), hwc(qry), lab, 4, normalize=True))
    w = dev(g["g_weight"]).reshape(out.shape)
    gr, gq = torch.autograd.grad((out * w).sum(), [ref, qry])
    np.testing.assert_allclose(gr.cpu().numpy(), g["g_grad_ref"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gq.cpu().numpy(), g["g_grad_qry"], rtol=RTOL, atol=ATOL)
    out = ops.global_match(hwc(ref), hwc(qry), lab, 3, deterministic=True)
    w = dev(g["g_weight_raw"]).reshape(out.shape)
    gr, gq = torch.autograd.grad((out * w).sum(), [ref, qry])
    np.testing.assert_allclose(gr.cpu().numpy(), g["g_grad_ref_raw"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(gq.cpu().numpy(), g["g_grad_qry_raw"], rtol=RTOL, atol=ATOL)


def test_global_knn_fixture_gradients_through_the_ordered_route(ops):
    g = load_golden("grad_knn")
    for i in range(int(g["n_cases"])):
        ref, qry = dev(g["c%d_ref_chw" % i], True), dev(g["c%d_qry_chw" % i], True)
        lab, k, n_ids = dev(g["c%d_labels" % i]), int(g["c%d_k" % i]), int(g["c%d_n_obj" % i]) + 1
        out = ops.global_match(hwc(ref), hwc(qry), lab, n_ids, k_nearest_neighbors=k, deterministic=True)
        np.testing.assert_allclose(out.detach().cpu().numpy(), g["c%d_out" % i].reshape(-1, n_ids), rtol=2e-5, atol=2e-6)
        w = dev(g["c%d_weight" % i]).reshape(out.shape)
        norm = (torch.sigmoid(out) - 0.5) * 2
        gr, gq = torch.autograd.grad((norm * w).sum(), [ref, qry])
        np.testing.assert_allclose(gr.cpu().numpy(), g["c%d_grad_ref" % i], rtol=RTOL, atol=ATOL, err_msg="case %d ref" % i)
        np.testing.assert_allclose(gq.cpu().numpy(), g["c%d_grad_qry" % i], rtol=RTOL, atol=ATOL, err_msg="case %d qry" % i)


@pytest.mark.parametrize("name,downsample", [("grad_tiny", True), ("grad_ds0", False)])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_local_fixture_gradients_through_the_ordered_route(ops, name, downsample, i):
    g = load_golden(name)
    prev, cur = dev(g["l%d_prev_chw" % i], True), dev(g["l%d_cur_chw" % i], True)
    lab, d, n_ids = dev(g["l%d_labels" % i]), int(g["l%d_d" % i]), int(g["l%d_n_ids" % i])
    out = ops.local_match(hwc(prev), hwc(cur), lab, n_ids, d, downsample=downsample, deterministic=True)
    np.testing.assert_allclose(out.detach().cpu().numpy().reshape(g["l%d_out" % i].shape), g["l%d_out" % i], rtol=1e-5, atol=2e-6)
    w = dev(g["l%d_weight" % i]).reshape(out.shape)
    gp, gc = torch.autograd.grad((out * w).sum(), [prev, cur])
    scale = max(np.abs(g["l%d_grad_cur" % i]).max(), 1e-6)
    np.testing.assert_allclose(gp.cpu().numpy(), g["l%d_grad_prev" % i], rtol=RTOL, atol=2e-5 * scale)
    np.testing.assert_allclose(gc.cpu().numpy(), g["l%d_grad_cur" % i], rtol=RTOL, atol=2e-5 * scale)


# -------------------------------------------------------------------------------- gradients at the training size: float64

# (_global64 / _local64: the float64 restatements on the op's recorded selection, tests/match_grad_ref.py)


def _both_routes(fn):
    return fn({}), fn({"deterministic": True})


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_global_gradients_at_training_size_against_float64(ops, size, k):
    """error = max |grad - grad64| / max |grad64| per tensor, both routes on the same inputs; the ordered route within 2x of the
    atomic one.  Measured on the MI355X, bank gradient atomic / ordered (the atomic figure changes from run to run; three runs):
    [100,104,104] k = 1: 4.0e-7 ... 6.0e-7 / 4.3e-7, k = 3: 3.6e-7 ... 8.6e-7 / 4.6e-7; [100,120,214] k = 1: 5.8e-7 ... 9.6e-7 /
    5.4e-7, k = 3: 2.5e-7 ... 3.1e-7 / 3.2e-7; query gradient 7.2e-8 ... 1.0e-7, the same figure on both routes.  (With ONE chain
    over all ranks instead of a sum per rank the ordered bank gradient stood at 1.1e-6 and 7.4e-7 for k = 3, 3x the atomic route's
    per-rank sums: the kernel now keeps a sum per rank and joins them in ascending rank.)"""
    h, w = size
    ref, _, cur, lab, _ = iid(h, w, 3, 10 + k)
    gout = torch.randn(h * w, 3, generator=torch.Generator().manual_seed(5)).cuda()
    errs = {}
    for name, kw in (("atomic", {}), ("ordered", {"deterministic": True})):
        r, q = ref.clone().requires_grad_(True), cur.clone().requires_grad_(True)
        out = ops.global_match(hwc(r), hwc(q), lab, 3, k_nearest_neighbors=k, **kw)
        arg = saved(out)[0]
        if k == 1:
            arg, wgt = arg[None], torch.ones_like(out)[None]
        else:
            wgt = [t for t in saved(out, torch.float32) if t.shape == arg.shape][0]
        gr, gq = torch.autograd.grad(out, [r, q], gout)
        wr, wq = _global64(ref, cur, arg, wgt, gout)
        errs[name] = (rel_err(gr, wr), rel_err(gq, wq))
    print("global %s k=%d: atomic (bank, query) %.3e %.3e   ordered %.3e %.3e" % ((size, k) + errs["atomic"] + errs["ordered"]))
    for a, o in zip(errs["atomic"], errs["ordered"]):
        assert o <= 2 * a, errs


@pytest.mark.parametrize("downsample", [True, False])
@pytest.mark.parametrize("size", SIZES)
def test_local_gradients_at_training_size_against_float64(ops, size, downsample):
    """as above for the local match (d = 12, 3 ids), with and without downsample.  Measured on the MI355X, (previous, current)
    frame, atomic / ordered: [100,104,104] downsample 4.98e-7, 2.44e-7 / 4.98e-7, 2.44e-7, no downsample 1.82e-7, 7.5e-8 / the same;
    [100,120,214] downsample 2.91e-7, 1.74e-7 / 3.07e-7, 1.74e-7, no downsample 2.68e-7, 7.8e-8 / the same."""
    h, w = size
    _, prev, cur, _, lab = iid(h, w, 3, 20)
    if not downsample:  # raw distances compete with the constant 1.0: closer embeddings, so that pixels do have winners
        prev, cur = prev * 0.5, cur * 0.5
    gout = torch.randn(h, w, 3, generator=torch.Generator().manual_seed(6)).cuda()
    errs = {}
    for name, kw in (("atomic", {}), ("ordered", {"deterministic": True})):
        p, c = prev.clone().requires_grad_(True), cur.clone().requires_grad_(True)
        out = ops.local_match(hwc(p), hwc(c), lab, 3, D, downsample=downsample, **kw)
        arg = saved(out)[0]
        assert int((arg >= 0).sum()) > h * w // 4
        gp, gc = torch.autograd.grad(out, [p, c], gout)
        wp, wc = _local64(prev, cur, arg, gout, D, downsample)
        errs[name] = (rel_err(gp, wp), rel_err(gc, wc))
    print("local %s downsample=%s: atomic (prev, cur) %.3e %.3e   ordered %.3e %.3e" % ((size, downsample) + errs["atomic"] + errs["ordered"]))
    for a, o in zip(errs["atomic"], errs["ordered"]):
        assert o <= 2 * a, errs


# ------------------------------------------------------------------------------------------------------- reproducibility

@pytest.mark.parametrize("case", ["iid", "colliding"])
@pytest.mark.parametrize("k", [1, 3])
def test_global_backward_is_bit_reproducible(ops, case, k):
    ref, _, cur, lab, _ = (iid if case == "iid" else colliding)(104, 104, 3, 30)
    gout = torch.randn(104 * 104, 3, generator=torch.Generator().manual_seed(7)).cuda()
    runs = []
    for _ in range(5):
        r, q = ref.clone().requires_grad_(True), cur.clone().requires_grad_(True)
        out = ops.global_match(hwc(r), hwc(q), lab, 3, k_nearest_neighbors=k, deterministic=True)
        arg = saved(out)[0].reshape(-1, 104 * 104, 3)[0]
        runs.append(torch.autograd.grad(out, [r, q], gout))
    if case == "colliding":  # one bank row per object collects (nearly) every query
        assert all(int(torch.bincount(arg[:, o].long()).max()) > 104 * 104 * 0.9 for o in range(3))
    assert float(runs[0][0].abs().max()) > 0 and float(runs[0][1].abs().max()) > 0
    for gr, gq in runs[1:]:
        assert torch.equal(gr, runs[0][0]) and torch.equal(gq, runs[0][1])


@pytest.mark.parametrize("case", ["iid", "colliding"])
@pytest.mark.parametrize("downsample", [True, False])
def test_local_backward_is_bit_reproducible(ops, case, downsample):
    _, prev, cur, _, lab = (iid if case == "iid" else colliding)(104, 104, 3, 31)
    if case == "iid" and not downsample:
        prev, cur = prev * 0.5, cur * 0.5
    gout = torch.randn(104, 104, 3, generator=torch.Generator().manual_seed(8)).cuda()
    runs = []
    for _ in range(5):
        p, c = prev.clone().requires_grad_(True), cur.clone().requires_grad_(True)
        out = ops.local_match(hwc(p), hwc(c), lab, 3, D, downsample=downsample, deterministic=True)
        winners = int((saved(out)[0] >= 0).sum())
        runs.append(torch.autograd.grad(out, [p, c], gout))
    assert winners > 1000
    assert float(runs[0][0].abs().max()) > 0 and float(runs[0][1].abs().max()) > 0
    for gp, gc in runs[1:]:
        assert torch.equal(gp, runs[0][0]) and torch.equal(gc, runs[0][1])


# ------------------------------------------------------------------------------------------------------- frozen operand

@pytest.mark.parametrize("downsample", [True, False])
def test_frozen_previous_frame_gets_none_and_the_current_frame_the_same_bits(ops, downsample):
    from cvpr2020_manet_amd.autograd import LocalMatchFullOrderedFn, LocalMatchOrderedFn
    _, prev, cur, _, lab = iid(52, 60, 3, 40)
    prev, cur = prev * 0.5, cur * 0.5
    gout = torch.randn(52, 60, 3, generator=torch.Generator().manual_seed(9)).cuda()
    p, c = prev.clone().requires_grad_(True), cur.clone().requires_grad_(True)
    gp2, gc2 = torch.autograd.grad(ops.local_match(hwc(p), hwc(c), lab, 3, 4, downsample=downsample, deterministic=True), [p, c], gout)
    assert float(gp2.abs().max()) > 0
    fn = LocalMatchOrderedFn if downsample else LocalMatchFullOrderedFn
    for frozen in (0, 1):
        a = prev.clone().requires_grad_(frozen != 0)
        b = cur.clone().requires_grad_(frozen != 1)
        out = fn.apply(hwc(a), hwc(b), lab.reshape(-1), 3, 4)
        grads = out.grad_fn.apply(gout)  # the node's own return values: None for the frozen operand
        assert grads[frozen] is None and grads[1 - frozen] is not None
        (got,) = torch.autograd.grad(ops.local_match(hwc(a), hwc(b), lab, 3, 4, downsample=downsample, deterministic=True),
                                     [b if frozen == 0 else a], gout)
        assert torch.equal(got, gc2 if frozen == 0 else gp2)


def test_frozen_bank_gets_no_gradient_and_the_query_the_same_bits(ops):
    ref, _, cur, lab, _ = iid(52, 60, 3, 41)
    gout = torch.randn(52 * 60, 3, generator=torch.Generator().manual_seed(10)).cuda()
    for k in (1, 3):
        r, q = ref.clone().requires_grad_(True), cur.clone().requires_grad_(True)
        gr2, gq2 = torch.autograd.grad(ops.global_match(hwc(r), hwc(q), lab, 3, k_nearest_neighbors=k, deterministic=True), [r, q], gout)
        q1 = cur.clone().requires_grad_(True)
        (gq,) = torch.autograd.grad(ops.global_match(hwc(ref), hwc(q1), lab, 3, k_nearest_neighbors=k, deterministic=True), [q1], gout)
        r1 = ref.clone().requires_grad_(True)
        (gr,) = torch.autograd.grad(ops.global_match(hwc(r1), hwc(cur), lab, 3, k_nearest_neighbors=k, deterministic=True), [r1], gout)
        assert torch.equal(gq, gq2) and torch.equal(gr, gr2) and float(gr.abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------- whole step

def _model(g, train_match, extra=()):
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    cfg = make_cfg(["--TEST_MODE", "False", "--MODEL_SEMANTIC_EMBEDDING_DIM", "12", "--MODEL_HEAD_EMBEDDING_DIM", "8",
                    "--MODEL_ASPP_OUTDIM", "6", "--MODEL_MAX_LOCAL_DISTANCE", "2"] + list(extra))
    model = M.IntVOS(cfg, TinyExtractor(), train_kernels="fused", train_match=train_match)
    sd = {k[4:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("sd::")}
    model.load_state_dict(sd, strict=True)
    return model.cuda().train()


def _step(g, model, knn=1):
    nobj = int(g["t_nobj"])
    return model.forward(dev(g["t_x"]), dev(g["t_ref_lab"]), dev(g["t_prev_lab"]), seq_names=["clip"], gt_ids=torch.Tensor([nobj]),
                         k_nearest_neighbors=knn, global_map_tmp_dic=None, local_map_dics=None, interaction_num=1,
                         start_annotated_frame=0, frame_num=[2])["clip"]


def test_whole_training_step_is_bit_reproducible_behind_the_encoder(ops):
    """IntVOS.forward in train() with train_kernels="fused", train_match="ordered" and the fused loss (size=(H, W)): two runs from
    the same state dict give the same bits at the extractor's output (what the embedding head receives) and for every parameter
    of the embedding head and the propagation head.  (The extractor's own convolution is the framework's: outside the claim.)"""
    from cvpr2020_manet_amd.networks.loss import Added_CrossEntropyLoss
    g = load_golden("grad_tiny")
    H, W = g["t_x"].shape[2:]
    nobj = int(g["t_nobj"])
    labels = torch.randint(0, nobj + 1, (1, H, W), generator=torch.Generator().manual_seed(3)).cuda()
    runs = []
    for _ in range(2):
        model = _model(g, "ordered")
        feats = []
        def keep(_module, _inputs, output):
            output.retain_grad()
            feats.append(output)
        hook = model.feature_extracter.register_forward_hook(keep)
        logits = _step(g, model)
        loss = Added_CrossEntropyLoss(0.15, 0)({"clip": logits}, {"clip": labels}, 0, size=(H, W))
        names = {type(n).__name__ for n in _nodes(loss)}
        assert any(n.startswith("UpsampledCrossEntropyTopKFn") for n in names) and any(n.startswith("DynamicSegHeadFn") for n in names)
        assert any(n.startswith("LocalMatchOrderedFn") for n in names) and any(n.startswith("GlobalMatchOrderedFn") for n in names)
        assert not any(n.startswith(("LocalMatchFnB", "GlobalMatchFnB", "GlobalMatchTopkFnB", "LocalMatchFullFnB")) for n in names), names
        loss.backward()
        hook.remove()
        grads = {"extractor output": feats[0].grad.clone(), "loss": loss.detach().clone()}
        for head in ("semantic_embedding", "dynamic_seghead"):  # (the embedding head's modules are aliased: ask the head itself)
            for name, p in getattr(model, head).named_parameters():
                grads[head + "." + name] = p.grad.clone()
        runs.append(grads)
    assert float(runs[0]["extractor output"].abs().max()) > 0
    assert sum(k.startswith("semantic_embedding.") for k in runs[0]) == 8 and sum(k.startswith("dynamic_seghead.") for k in runs[0]) == 34
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name


def _nodes(t):
    seen, stack = set(), [t.grad_fn]
    while stack:
        n = stack.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        stack.extend(f for f, _ in n.next_functions)
    return seen


@pytest.mark.parametrize("golden,extra", [("grad_tiny", ()), ("grad_step_alt", ("--MODEL_LOCAL_DOWNSAMPLE", "False"))])
def test_training_step_through_the_ordered_route_matches_reference(ops, golden, extra):
    """tests/test_autograd_gpu.py's training step (the reference's own logits and parameter gradients, that test's tolerances)
    with train_match="ordered"; grad_step_alt: k = 3 and no downsample through the ordered route as well"""
    g = load_golden(golden)
    model = _model(g, "ordered", extra)
    logits = _step(g, model, int(g["t_knn"]) if "t_knn" in g else 1)
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["t_logits"], rtol=1e-3, atol=1e-4)
    (logits * dev(g["t_wl"])).sum().backward()
    params = dict(model.named_parameters())
    for name in g["t_grad_names"].tolist():
        want = g["t_grad::" + name]
        got = params[name].grad.cpu().numpy()
        assert np.abs(got).max() > 0
        np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-4 * max(np.abs(want).max(), 1e-6), err_msg=name)
