"""head_act="f16" on the GPU: fp16 activations between the stages of a DynamicSegHead (DESIGN 4 states the contract).

  depthwise stage   rn16(min(relu(fmaf(acc + bias, scale1, shift1)), 65504)), acc the fp32 kernel's fmaf chain: bit for bit the
                    fp32 kernel's output saturated and rounded;
  1x1 stage         exact fp16 x fp16 products, fp32 accumulation in the MFMA's own order, fp32 epilogue, one rounding at the
                    store: bounded against float64 by one fp16 spacing plus the worst case of an fp32 sum in ANY order;
  whole head        against an emulation of the contract composed from framework ops, margin 2 (see test 5);
  module            memo, prepare_head_terms, mode switches, and the fall-back of ineligible shapes to the fp32 route's bits.

Per-kernel inputs are fp16 values already and hold no fp16 subnormals (test 4 adds them on purpose)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
U32 = 2.0 ** -23  # per-operation relative error allowed to an fp32 sum (twice the unit roundoff: any order, fused or not)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def h16(a, keep_subnormals=False):
    """a -> the fp16 values nearest to it, as float32; magnitudes below fp16's smallest normal become 0 first unless kept"""
    a = np.asarray(a, np.float32).copy()
    if not keep_subnormals:
        a[np.abs(a) < F16_MIN_NORMAL] = 0.0
    return a.astype(np.float16).astype(np.float32)


def rn16(a64):
    """float64 -> min(., 65504) rounded to nearest-even fp16 (numpy rounds a float64 to half directly: one rounding)"""
    return np.minimum(a64, F16_MAX).astype(np.float16)


def spacing16(m):
    """one fp16 spacing at magnitude m (float64 array)"""
    e = np.floor(np.log2(np.maximum(m, F16_MIN_NORMAL)))
    return 2.0 ** (e - 10)


# ---- 1. depthwise: the fp32 kernel's bits, saturated and rounded

DW_SHAPES = [(1, 3, 61, 66), (3, 5, 9, 14), (2, 4, 130, 72), (2, 3, 60, 64), (3, 2, 121, 130), (2, 3, 121, 86), (3, 256, 24, 36)]
_dw_cache = {}


def dw_case(shape):
    """(x fp16-exact fp32, weight, bias, scale, shift) on the GPU: made once per shape, shared, never written to"""
    if shape not in _dw_cache:
        B, C, h, w = shape
        rng = np.random.default_rng(B * 1000 + C * 100 + h + w)
        x = h16(rng.standard_normal(shape) * 0.7)
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()
        _dw_cache[shape] = (t(x), t(rng.standard_normal((C, 1, 7, 7)) * 0.2), t(rng.standard_normal(C) * 0.1),
                            t(rng.uniform(0.5, 1.5, C)), t(rng.standard_normal(C) * 0.1))
    return _dw_cache[shape]


@pytest.mark.parametrize("in16", [False, True], ids=["in_f32", "in_f16"])
@pytest.mark.parametrize("shape", DW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_depthwise_is_the_fp32_kernel_saturated_and_rounded(ops, shape, in16):
    x, wt, bias, scale, shift = dw_case(shape)
    want = ops.dwconv7x7_bn_relu(x, wt, bias, scale=scale, shift=shift).clamp(max=F16_MAX).half()
    got = ops.dwconv7x7_bn_relu_f16(x.half() if in16 else x, wt, bias, scale=scale, shift=shift)
    assert got.dtype == torch.float16 and got.shape == x.shape
    assert (want > 0).float().mean() > 0.2  # (the case exercises both sides of the ReLU)
    assert torch.equal(got, want), "max |diff| %g" % (got.float() - want.float()).abs().max().item()


# ---- 2. saturation and NaN

def test_depthwise_saturates_at_65504_and_keeps_a_nan(ops):
    x, wt, bias, scale, shift = dw_case((2, 3, 60, 64))
    big = ops.dwconv7x7_bn_relu_f16(x, wt, bias, scale=scale * 3e5, shift=shift)
    f32 = ops.dwconv7x7_bn_relu(x, wt, bias, scale=scale * 3e5, shift=shift)
    assert (f32 > F16_MAX).float().mean() > 0.05  # outputs beyond the fp16 range exist ...
    assert torch.isfinite(big).all() and torch.equal(big[f32 > F16_MAX], torch.full_like(big[f32 > F16_MAX], F16_MAX))
    for in16 in (False, True):
        xn = x.clone()
        xn[1, 2, 30, 40] = float("nan")
        out = ops.dwconv7x7_bn_relu_f16(xn.half() if in16 else xn, wt, bias, scale=scale, shift=shift)
        assert torch.isnan(out[1, 2, 30, 40])
        bad = torch.isnan(out)
        bad[1, 2, 27:34, 37:44] = False  # the 7 x 7 outputs that read the pixel may be NaN; nothing else
        assert not bad.any()


# ---- 3. the 1x1 against float64

def pw_case(cin, B, hw, seed=0):
    """fp16-exact activation [B, cin, h, w] (post-ReLU-like: non-negative), fp16-exact weight w2t [cin, 256], fp32 b2 / add /
    output-layer weights"""
    h, w = hw
    rng = np.random.default_rng(seed + cin * 7 + B * 3 + h * w)
    x = h16(np.maximum(rng.standard_normal((B, cin, h, w)), 0) * 0.5)
    w2t = h16(rng.standard_normal((cin, 256)) * (0.5 / np.sqrt(cin)))
    b2 = (rng.standard_normal(256) * 0.2).astype(np.float32)
    add = (rng.standard_normal((256, h, w)) * 0.3).astype(np.float32)
    hw_ = (rng.standard_normal(256) * 0.1).astype(np.float32)
    hb = np.float32(0.05)
    return x, w2t, b2, add, hw_, hb


def pw_reference(x, w2t, b2, add):
    """(float64 value before the ReLU, S = sum |w||x| + |b2| + |add|) by the framework's float64 convolution"""
    X, W = torch.from_numpy(x).double(), torch.from_numpy(w2t).double().t().reshape(256, -1, 1, 1)
    v = F.conv2d(X, W, torch.from_numpy(b2).double())
    S = F.conv2d(X.abs(), W.abs(), torch.from_numpy(b2).double().abs())
    if add is not None:
        v, S = v + torch.from_numpy(add).double(), S + torch.from_numpy(add).double().abs()
    return v.numpy(), S.numpy()


PW_GRIDS = [(10, 12), (12, 16), (24, 36)]  # h*w = 120 (a lone partial tile of 128), 192 (1.5 tiles), 864 (6.75 tiles)


@pytest.mark.parametrize("form", ["relu", "add_relu", "logits"])
@pytest.mark.parametrize("hw", PW_GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cin", [3, 100, 256])
def test_pointwise_against_float64(ops, cin, B, hw, form):
    x, w2t, b2, add, hw_, hb = pw_case(cin, B, hw)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()
    weight = ops.HalfWeight(t(w2t))
    v64, S = pw_reference(x, w2t, b2, add if form == "add_relu" else None)
    if form == "logits":
        got = ops.conv1x1_f16(t(x).half(), weight, t(b2), head_weight=t(hw_).reshape(1, 256, 1, 1), head_bias=t([hb]))
        assert got.dtype == torch.float32 and got.shape == (B, 1) + hw
        want = (np.maximum(v64, 0) * hw_.astype(np.float64)[None, :, None, None]).sum(1, keepdims=True) + float(hb)
        S2 = (S * np.abs(hw_.astype(np.float64))[None, :, None, None]).sum(1, keepdims=True) + abs(float(hb))
        err, bound = np.abs(got.cpu().numpy().astype(np.float64) - want), (cin + 258) * U32 * S2
        print("cin %d B %d %dx%d logits: max err %.3g, max err / bound %.3g" % (cin, B, hw[0], hw[1], err.max(), (err / bound).max()))
        assert np.all(err <= bound)
        return
    got = ops.conv1x1_f16(t(x).half(), weight, t(b2), relu_out=True, add=t(add) if form == "add_relu" else None)
    assert got.dtype == torch.float16 and got.shape == (B, 256) + hw
    want = rn16(np.maximum(v64, 0))
    g64, w64 = got.cpu().numpy().astype(np.float64), want.astype(np.float64)
    err, bound = np.abs(g64 - w64), spacing16(np.maximum(np.abs(g64), np.abs(w64))) + (cin + 2) * U32 * S
    differ = float((g64 != w64).mean())
    print("cin %d B %d %dx%d %s: max err %.3g, max err / bound %.3g, outputs that differ from rn16(float64) %.4f %%"
          % (cin, B, hw[0], hw[1], form, err.max(), (err / bound).max(), 100 * differ))
    assert np.all(err <= bound)
    assert differ <= 0.01  # a rounding-mode bug (truncation, double rounding through another grid) moves far more than 1 %


def test_pointwise_saturates_at_65504_and_keeps_a_nan(ops):
    x, w2t, b2, add, _, _ = pw_case(100, 2, (12, 16), seed=5)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()
    weight = ops.HalfWeight(t(w2t))
    # (powers of two keep the operands fp16 values: activations up to ~1e4, weights up to ~30, sums of +-1e5)
    big = ops.conv1x1_f16(t(x * 2.0 ** 12).half(), ops.HalfWeight(t(w2t * 2.0 ** 7)), t(b2), relu_out=True, add=t(add))
    v64, _ = pw_reference(x * 2.0 ** 12, w2t * 2.0 ** 7, b2, add)
    over = torch.from_numpy(v64 > F16_MAX * 1.01).cuda()
    assert over.float().mean() > 0.05
    assert torch.isfinite(big).all() and torch.equal(big[over], torch.full_like(big[over], F16_MAX))
    xn = x.copy()
    xn[1, 7, 5, 9] = np.nan
    for kw in ({}, {"add": t(add)}):
        out = ops.conv1x1_f16(t(xn).half(), weight, t(b2), relu_out=True, **kw)
        assert torch.isnan(out[1, :, 5, 9]).all()
        bad = torch.isnan(out)
        bad[1, :, 5, 9] = False
        assert not bad.any()


# ---- 4. fp16 subnormal operands

def test_pointwise_subnormal_elements_move_an_output_by_at_most_their_products(ops):
    """5 % of the activation elements are fp16 subnormals (multiples of 2^-24 below 2^-14).  Whether the matrix pipe keeps or
    flushes such operands is the hardware's: an output may lose at most the products in which a subnormal takes part, sum |w||x|
    over those elements.  The bound is built from the inputs, so it holds either way; the behaviour seen is printed."""
    cin, B, hw = 100, 2, (12, 16)
    x, w2t, b2, _, _, _ = pw_case(cin, B, hw, seed=9)
    rng = np.random.default_rng(9)
    m = rng.random(x.shape) < 0.05
    x[m] = (rng.integers(1, 1024, size=int(m.sum())) * 2.0 ** -24).astype(np.float32)
    assert np.array_equal(h16(x, keep_subnormals=True), x)
    sub = (x != 0) & (x < F16_MIN_NORMAL)
    assert 0.03 < sub.mean() < 0.07
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()
    weight = ops.HalfWeight(t(w2t))
    got = ops.conv1x1_f16(t(x).half(), weight, t(b2), relu_out=True).cpu().numpy().astype(np.float64)
    v64, S = pw_reference(x, w2t, b2, None)
    _, slack = pw_reference(x * sub, w2t, np.zeros_like(b2), None)  # sum |w||x| over the subnormal elements
    want = rn16(np.maximum(v64, 0)).astype(np.float64)
    base = spacing16(np.maximum(np.abs(got), np.abs(want))) + (cin + 2) * U32 * S
    err = np.abs(got - want)
    print("max err %.3g, max allowed %.3g, max allowed without the subnormal term %.3g" % (err.max(), (base + slack).max(), base.max()))
    assert np.all(err <= base + slack)
    # which behaviour: one subnormal activation 2^-15 against a weight of 2048: kept -> 2^-4, flushed -> 0
    xx, ww = np.zeros((1, 1, 2, 4), np.float32), np.zeros((1, 256), np.float32)
    xx[:], ww[:] = 2.0 ** -15, 2048.0
    out = ops.conv1x1_f16(t(xx).half(), ops.HalfWeight(t(ww)), t(np.zeros(256)), relu_out=True)
    v = float(out[0, 0, 0, 0])
    print("fp16 subnormal operand in v_mfma_f32_32x32x16_f16: 2^-15 * 2048 = %.6f (kept: 0.0625, flushed: 0) -> %s"
          % (v, "kept" if v == 0.0625 else "flushed"))
    assert v in (0.0625, 0.0)


# ---- 5. the whole head against the contract

def _make_head(seed, act="f16"):
    """a DynamicSegHead of default size (103 -> 256 -> 256 -> 256 -> 256 -> 1) with non-trivial BatchNorm statistics"""
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    M.set_cfg(make_cfg([]))
    torch.manual_seed(seed)
    head = M.DynamicSegHead()
    g = torch.Generator().manual_seed(seed + 1)
    for m in head.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5, generator=g)
            m.bias.data.normal_(0.0, 0.1, generator=g)
            m.running_mean.normal_(0.0, 0.1, generator=g)
            m.running_var.uniform_(0.5, 1.5, generator=g)
    head = head.cuda().eval()
    return M.use_head_act(head, act), M


def _emulate(head, x):
    """the contract composed from framework ops in fp32 on the CPU: every stored activation through
    min(., 65504) -> half -> float, the folded 1x1 weight rounded once to half, layer 4's ReLU and the output conv in fp32"""
    from cvpr2020_manet_amd import ops
    r16 = lambda t: t.clamp(max=F16_MAX).half().float()
    layers = [head.layer1, head.layer2, head.layer3, head.layer4]
    for i, blk in enumerate(layers):
        scale1, shift1 = ops.fold_bn(blk.bn1)
        scale2, shift2 = ops.fold_bn(blk.bn2)
        acc = F.conv2d(x, blk.conv1.weight, None, padding=3, groups=x.shape[1])
        y = r16(torch.relu(torch.addcmul(shift1[None, :, None, None], acc + blk.conv1.bias[None, :, None, None], scale1[None, :, None, None])))
        w16 = (blk.conv2.weight * scale2[:, None, None, None]).half().float()
        z = torch.relu(F.conv2d(y, w16, blk.conv2.bias * scale2 + shift2))
        if i == 3:
            return F.conv2d(z, head.conv.weight, head.conv.bias)
        x = r16(z)


@pytest.mark.parametrize("grid", [(24, 36), (20, 72)], ids=lambda g: "%dx%d" % g)
def test_whole_head_stays_within_twice_the_contracts_own_error(grid):
    """f16 route vs today's fp32 route, against what an emulation of the contract loses.  Factor 2: two correct implementations
    of the contract differ where an fp32 sum falls on an fp16 rounding boundary, and that flip propagates through the layers
    (fp32 sums against float64 sums in the emulation: 0.31 of the emulation's own error, measured on the CPU)."""
    h, w = grid
    head, M = _make_head(3)
    torch.manual_seed(h * w)
    emb = torch.relu(torch.randn(1, 100, h, w)) * 0.3
    per = torch.rand(3, 3, h, w)
    per[:, 2] = (per[:, 2] > 0.5).float()
    with torch.no_grad():
        assert head._f16_ok(h, w, 100)
        got = head.forward_shared(emb.cuda(), per.cuda())
        M.use_head_act(head, "f32")
        ref = head.forward_shared(emb.cuda(), per.cuda())
        emul = _emulate(head.cpu().float(), torch.cat((emb.repeat(3, 1, 1, 1), per), 1))
    assert got.dtype == torch.float32 and got.shape == ref.shape == (3, 1, h, w)
    d, e = (got - ref).cpu().double(), (emul - ref.cpu()).double()
    print("grid %dx%d: max |logit| %.3g; f16 route vs fp32 route: max %.3g rms %.3g; emulation vs fp32 route: max %.3g rms %.3g"
          % (h, w, ref.abs().max().item(), d.abs().max().item(), d.pow(2).mean().sqrt().item(), e.abs().max().item(),
             e.pow(2).mean().sqrt().item()))
    assert e.abs().max() > 0 and not torch.equal(got, ref)  # (the mode is really on)
    assert d.abs().max() <= 2 * e.abs().max()
    assert d.pow(2).mean().sqrt() <= 2 * e.pow(2).mean().sqrt()


# ---- 6. the module

def _clip_model(dev, **kw):
    from examples import propagate_clip as pc
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks.IntVOS import IntVOS
    torch.manual_seed(0)  # (the same weights for every model of the test)
    cfg = make_cfg(["--TEST_MODE", "True"])
    model = IntVOS(cfg, pc.StandInEncoder(cfg.MODEL_ASPP_OUTDIM), **kw).to(dev).eval()
    g = torch.Generator().manual_seed(11)
    for m in list(model.dynamic_seghead.modules()) + list(model.inter_seghead.modules()):
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g).mul_(0.1).to(dev))
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g).add_(0.5).to(dev))
    return cfg, model


def _clip_inputs(dev):
    h, w, H, W = 24, 36, 96, 144
    g = torch.Generator().manual_seed(5)
    emb = (torch.relu(torch.randn(4, 100, h, w, generator=g)) * 0.3).to(dev)
    scribs = []
    for r in range(2):
        s = torch.full((1, 1, h, w), -1.0)
        s[0, 0, 3 + r:6 + r, 4:20] = 0
        s[0, 0, 12:15, 8 + r:30] = 1
        s[0, 0, 18:21, 20:33 - r] = 2
        scribs.append(s.to(dev))
    return emb, scribs, (H, W)


def _two_rounds(model, emb, scribs, size, calls=None):
    """int_seghead on the annotated frame, prop_seghead along the clip, twice (memories carried over); returns every logit
    tensor in call order.  calls: a list that receives (shared, per_object, logits) of every propagation-head call"""
    SEQ, gt, out = "clip", torch.Tensor([3]), []
    up = lambda x: torch.argmax(F.interpolate(x, size=size, mode="bilinear", align_corners=True), dim=1)
    head = model.dynamic_seghead
    if calls is not None:
        inner = head.forward_shared

        def spy(shared, per_object, memo=None):
            y = inner(shared, per_object, memo=memo)
            calls.append((shared.clone(), per_object.clone(), y.clone()))
            return y
        head.forward_shared = spy
    try:
        with torch.no_grad():
            gmap, lmaps, prev_round = {}, ({}, {}), None
            for r, start in enumerate((1, 2)):
                ref = emb[start:start + 1]
                tmp, lmaps = model.int_seghead(ref_frame_embedding=ref, ref_scribble_label=scribs[r], prev_round_label=prev_round,
                                               global_map_tmp_dic=gmap, local_map_dics=lmaps, interaction_num=r + 1, seq_names=[SEQ],
                                               gt_ids=gt, frame_num=[start], first_inter=r == 0)
                out.append(tmp[SEQ])
                prev_label, prev_emb = up(tmp[SEQ]).unsqueeze(0), ref
                prev_round = up(tmp[SEQ]).float().unsqueeze(0)
                for ii in range(start + 1, 4):
                    tmp, gmap, lmaps = model.prop_seghead(ref, prev_emb, emb[ii:ii + 1], scribs[r], prev_label,
                                                          normalize_nearest_neighbor_distances=True, use_local_map=True,
                                                          seq_names=[SEQ], gt_ids=gt, k_nearest_neighbors=1, global_map_tmp_dic=gmap,
                                                          local_map_dics=lmaps, interaction_num=r + 1, start_annotated_frame=start,
                                                          frame_num=[ii], dynamic_seghead=head)
                    out.append(tmp[SEQ])
                    prev_label, prev_emb = up(tmp[SEQ]).unsqueeze(0), emb[ii:ii + 1]
    finally:
        if calls is not None:
            del head.forward_shared
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_module_runs_the_f16_route_with_memo_prepare_and_mode_switches():
    dev = torch.device("cuda", 0)
    emb, scribs, size = _clip_inputs(dev)
    cfg, model = _clip_model(dev, head_act="f16")
    assert model.head_act == "f16"
    calls = []
    got = _two_rounds(model, emb, scribs, size, calls=calls)
    assert len(got) == 5 and len(calls) == 3  # rounds: int + frames 2, 3; int + frame 3
    # the logits are the head-level f16 route's, and not the fp32 route's
    from cvpr2020_manet_amd.networks import IntVOS as M
    with torch.no_grad():
        for shared, per_object, y in calls:
            assert model.dynamic_seghead._f16_ok(24, 36, 100)
            assert torch.equal(model.dynamic_seghead.forward_shared(shared, per_object), y)
    _, plain = _clip_model(dev)
    assert plain.head_act == "f32"
    want32 = _two_rounds(plain, emb, scribs, size)
    assert not _same(got, want32)
    # round 2 met frame 3's memoised term: the same bits as a model that never keeps one
    _, nocache = _clip_model(dev, head_act="f16", cache_frames=False)
    assert _same(_two_rounds(nocache, emb, scribs, size), got)
    # prepare_head_terms stores the f16 route's term for every cached frame, and the logits do not move
    _, prepared = _clip_model(dev, head_act="f16")
    with torch.no_grad():
        embp = prepared.prepare_clip(emb)
        assert prepared.prepare_head_terms(embp) == 4
    assert _same(_two_rounds(prepared, embp, scribs, size), got)
    # mode switches: each mode gives exactly a fresh model's logits -- no term crosses modes
    model.head_act = "f32"
    assert model.head_act == "f32" and _same(_two_rounds(model, emb, scribs, size), want32)
    model.head_act = "f16"
    assert _same(_two_rounds(model, emb, scribs, size), got)
    with pytest.raises(ValueError):
        model.head_act = "f8"


# ---- 7. fall-back: an ineligible head or grid takes the fp32 route, bit for bit

def test_ineligible_heads_and_grids_fall_back_to_the_fp32_routes_bits():
    from conftest import load_golden
    from test_intvos_module import build_model, run_script
    dev = torch.device("cuda", 0)
    g = load_golden("e2e_tiny")  # a narrow head (not 256 channels) on a grid of width 13: never eligible
    want = run_script(build_model(g, dev), g, dev)
    got = run_script(build_model(g, dev, head_act="f16"), g, dev)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # a 256-channel head at an odd width
    head, M = _make_head(4)
    torch.manual_seed(0)
    emb, per = (torch.relu(torch.randn(1, 100, 24, 35)) * 0.3).cuda(), torch.rand(3, 3, 24, 35).cuda()
    with torch.no_grad():
        assert not head._f16_ok(24, 35, 100) and head._f16_ok(24, 36, 100)
        a = head.forward_shared(emb, per)
        x = torch.cat((emb.repeat(3, 1, 1, 1), per), 1)
        a2 = head(x)
        M.use_head_act(head, "f32")
        assert torch.equal(head.forward_shared(emb, per), a) and torch.equal(head(x), a2)
