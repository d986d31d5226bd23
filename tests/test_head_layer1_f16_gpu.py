"""head_act="f16", layer 1's per-object half in one launch (ops.head_layer1_object_f16) on the GPU.

The contract is exact: the output equals, bit for bit, what the two launches it replaces compute,

    ops.conv1x1_f16(ops.dwconv7x7_bn_relu_f16(per_object, ...), HalfWeight(w2t_object), b2, relu_out=True, add=term)

-- the same fp32 fmaf chains, one rounding to fp16, the same fp16 MFMA on a zero accumulator, the same fp32 epilogue and store.
Nothing here is a tolerance.  Grids (a workgroup owns 64 consecutive pixels of the flattened plane):
  (1, 8), (4, 2)  the smallest legal planes: every tap is border;
  (7, 8)          shorter than the 7 x 7 window;
  (10, 12)        120 pixels: a full tile and a partial one;
  (13, 24)        an odd row count;
  (24, 36)        the module tests' grid, 13.5 tiles;
  (32, 214)       the 480p row width: tiles start at every column phase, 107 tiles."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F16_MAX = 65504.0
GRIDS = [(1, 8), (4, 2), (7, 8), (10, 12), (13, 24), (24, 36), (32, 214)]
OBJECTS = (1, 2, 3, 5)
CHANNELS = (1, 2, 3, 4)
N_MAX, CP_MAX = max(OBJECTS), max(CHANNELS)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


_cases = {}


def case(grid):
    """the inputs of a grid, made once on the GPU, shared, never written to: signed random planes [5, 4, h, w] (a case takes the
    first n objects and Cp channels and makes its last channel, from two channels up, a 0/1 plane), depthwise parameters of four
    channels, w2t [4, 256], b2, term [1, 256, h, w]"""
    if grid not in _cases:
        h, w = grid
        rng = np.random.default_rng(1000 * h + w)
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda()
        _cases[grid] = dict(planes=t(rng.standard_normal((N_MAX, CP_MAX, h, w)) * 0.7), dw=t(rng.standard_normal((CP_MAX, 1, 7, 7)) * 0.2),
                            bias=t(rng.standard_normal(CP_MAX) * 0.1), scale=t(rng.uniform(0.5, 1.5, CP_MAX)),
                            shift=t(rng.standard_normal(CP_MAX) * 0.1), w2t=t(rng.standard_normal((CP_MAX, 256)) * 0.5),
                            b2=t(rng.standard_normal(256) * 0.2), term=t(rng.standard_normal((1, 256, h, w)) * 0.3))
    return _cases[grid]


def per_object(c, n, cp):
    per = c["planes"][:n, :cp].clone()
    if cp >= 2:
        per[:, cp - 1] = (per[:, cp - 1] > 0).float()
    return per


def both(ops, c, per, cp, term, scale=None, relu_out=True):
    """(the depthwise planes, the two-launch composition, the fused op) on the same inputs"""
    scale = c["scale"][:cp] if scale is None else scale
    weight = ops.HalfWeight(c["w2t"][:cp])
    d = ops.dwconv7x7_bn_relu_f16(per, c["dw"][:cp], c["bias"][:cp], scale=scale, shift=c["shift"][:cp])
    want = ops.conv1x1_f16(d, weight, c["b2"], relu_out=relu_out, add=term)
    got = ops.head_layer1_object_f16(per, c["dw"][:cp], c["bias"][:cp], scale, c["shift"][:cp], weight, c["b2"], term=term,
                                     relu_out=relu_out)
    return d, want, got


# ---- 1. bit-equality with the composition

@pytest.mark.parametrize("with_term", [True, False], ids=["term", "no_term"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
def test_fused_op_equals_the_two_launch_composition_bit_for_bit(ops, grid, with_term):
    c = case(grid)
    pos = tot = 0
    for n in OBJECTS:
        for cp in CHANNELS:
            per = per_object(c, n, cp)
            d, want, got = both(ops, c, per, cp, c["term"] if with_term else None)
            assert got.dtype == torch.float16 and got.shape == (n, 256) + grid
            assert torch.equal(got, want), "n=%d Cp=%d: %d of %d outputs differ, max |diff| %g" % (
                n, cp, int((got != want).sum()), got.numel(), (got.float() - want.float()).abs().max().item())
            pos, tot = pos + int((d > 0).sum()), tot + d.numel()
    print("grid %dx%d: %.1f %% of the %d depthwise outputs are positive" % (grid[0], grid[1], 100.0 * pos / tot, tot))
    assert 0.2 < pos / tot < 0.8  # (both sides of the ReLU)


def test_fused_op_without_the_output_relu_and_without_bias_or_bn(ops):
    """relu_out = 0 and the NULL forms of dw_bias / scale / shift (0 / 1 / 0), against the composition"""
    c = case((13, 24))
    per, weight = per_object(c, 3, 3), ops.HalfWeight(c["w2t"][:3])
    _, want, got = both(ops, c, per, 3, c["term"], relu_out=False)
    assert (want < 0).any() and torch.equal(got, want)
    d = ops.dwconv7x7_bn_relu_f16(per, c["dw"][:3])
    want = ops.conv1x1_f16(d, weight, c["b2"], relu_out=True, add=c["term"])
    assert torch.equal(ops.head_layer1_object_f16(per, c["dw"][:3], None, None, None, weight, c["b2"], term=c["term"]), want)


# ---- 2. saturation and NaN

def test_fused_op_saturates_at_65504_and_keeps_a_nan_as_the_composition_does(ops):
    c = case((24, 36))
    per, weight = per_object(c, 3, 3), ops.HalfWeight(c["w2t"][:3])
    big = c["scale"][:3] * 3e5
    d, want, got = both(ops, c, per, 3, c["term"], scale=big)
    unrounded = ops.conv1x1_f16(d, weight, c["b2"], relu_out=True, add=c["term"], out_f32=True)
    assert (d == F16_MAX).float().mean() > 0.05 and (unrounded > F16_MAX).float().mean() > 0.05  # outputs beyond 65504 exist ...
    assert torch.isfinite(got).all() and torch.equal(got, want)  # ... and are stored as 65504
    assert torch.equal(got[unrounded > F16_MAX], torch.full_like(got[unrounded > F16_MAX], F16_MAX))
    for ch in range(3):
        pern = per.clone()
        pern[1, ch, 10, 20] = float("nan")
        for term in (c["term"], None):
            _, want, got = both(ops, c, pern, 3, term)
            bad = torch.isnan(got)
            assert torch.equal(bad, torch.isnan(want))
            region = torch.zeros_like(bad)
            region[1, :, 7:14, 17:24] = True  # the 7 x 7 outputs of that object that read the pixel, every channel
            assert torch.equal(bad, region)
            assert torch.equal(got[~bad], want[~bad])


# ---- 3. the module

def _head(seed, in_dim):
    """a 256-channel DynamicSegHead of `in_dim` input channels under head_act="f16", with non-trivial BatchNorm statistics"""
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M
    M.set_cfg(make_cfg([]))
    torch.manual_seed(seed)
    head = M.DynamicSegHead(in_dim=in_dim)
    g = torch.Generator().manual_seed(seed + 1)
    for m in head.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5, generator=g)
            m.bias.data.normal_(0.0, 0.1, generator=g)
            m.running_mean.normal_(0.0, 0.1, generator=g)
            m.running_var.uniform_(0.5, 1.5, generator=g)
    return M.use_head_act(head.cuda().eval(), "f16"), M


@pytest.mark.parametrize("cp", [3, 2], ids=["propagation_head_Cp3", "interaction_head_Cp2"])
def test_module_takes_the_fused_op_once_per_call_and_keeps_the_two_launch_bits(ops, monkeypatch, cp):
    h, w, cs = 24, 36, 100
    head, M = _head(7 + cp, cs + cp)
    torch.manual_seed(cp)
    emb = (torch.relu(torch.randn(1, cs, h, w)) * 0.3).cuda()
    per = torch.rand(3, cp, h, w)
    per[:, cp - 1] = (per[:, cp - 1] > 0.5).float()
    per = per.cuda()
    fused, calls = ops.head_layer1_object_f16, []

    def counted(*a, **kw):
        calls.append(1)
        return fused(*a, **kw)

    def two_launches(per_object, dw_weight, dw_bias, scale, shift, weight, b2, term=None, relu_out=True):
        calls.append(2)
        d = ops.dwconv7x7_bn_relu_f16(per_object, dw_weight, dw_bias, scale=scale, shift=shift)
        return ops.conv1x1_f16(d, weight, b2, relu_out=relu_out, add=term)

    with torch.no_grad():
        assert head._f16_ok(h, w, cs)
        monkeypatch.setattr(ops, "head_layer1_object_f16", counted)
        got = head.forward_shared(emb, per)
        assert calls == [1] and got.dtype == torch.float32 and got.shape == (3, 1, h, w)
        memo = {}
        first = head.forward_shared(emb, per, memo=memo)
        assert memo.get("term") is not None
        again = head.forward_shared(emb, per, memo=memo)  # the memoised term: the same bits
        assert calls == [1, 1, 1] and torch.equal(first, got) and torch.equal(again, got)
        monkeypatch.setattr(ops, "head_layer1_object_f16", two_launches)
        assert torch.equal(head.forward_shared(emb, per), got) and calls[-1] == 2
        # the fp32 route is another result (the mode is really on), and an ineligible grid takes it unchanged
        monkeypatch.setattr(ops, "head_layer1_object_f16", counted)
        del calls[:]
        emb_odd, per_odd = emb[..., :35].contiguous(), per[..., :35].contiguous()
        assert not head._f16_ok(h, 35, cs)
        odd = head.forward_shared(emb_odd, per_odd)
        assert calls == []
        M.use_head_act(head, "f32")
        assert torch.equal(head.forward_shared(emb_odd, per_odd), odd)
        assert not torch.equal(head.forward_shared(emb, per), got) and calls == []
