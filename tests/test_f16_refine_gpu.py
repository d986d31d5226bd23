"""MANET_COMPUTE_F16_REFINE ("f16r"): fp16 filter + exact fp32 re-rank.  The result must EQUAL compute="f32" bit for bit on EVERY
input -- inside fp16's domain, across its edge (|row|^2 > 65504: the fp16 image holds NaN, fp32 a value), with infinities, NaNs and
fp16-subnormal elements -- so every comparison here is torch.equal (NaN-aware where NaNs are expected) against compute="f32" on
the same tensors; nothing has a tolerance.  The shapes and adversarial banks are tests/test_bf16_refine.py's; two tests see to
it that the filter really filters (a build that rescues everything would pass every equality) and that it filters better than
bf16 on an encoder's embeddings, which is what the mode is for."""
import os
import sys

import pytest
import torch

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def _case(seed, N, M, C, n_ids, scale=0.2, unlabelled=0.0, dtype=torch.float32):
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = (torch.relu(torch.randn(N, C, generator=g, device="cuda")) * scale).to(dtype)
    k = (torch.relu(torch.randn(M, C, generator=g, device="cuda")) * scale).to(dtype)
    lab = torch.randint(0, n_ids, (M,), generator=g, device="cuda", dtype=torch.int32)
    if unlabelled > 0:
        lab[torch.rand(M, generator=g, device="cuda") < unlabelled] = -1
    return q, k, lab


def _same_with_nans(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(torch.where(na, torch.zeros_like(a), a),
                                                          torch.where(nb, torch.zeros_like(b), b)))


def _match(ops, k, q, lab, n_ids):
    """(f16r result, f32 result, the f16r match's statistics) with the adaptive policy off"""
    bank = ops.PreparedBank(k, lab, n_ids, compute="f16r")
    got = bank.match(q, adaptive=False)
    return got, ops.global_match(k, q, lab, n_ids, compute="f32"), bank.refine_stats_full()


SHAPES = [(700, 3000, 100, 3), (1, 64, 100, 1), (257, 65, 16, 2), (3000, 20000, 100, 5), (512, 5000, 106, 4), (900, 900, 7, 2)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("scale", [0.1, 0.5, 3.0, 30.0, 40.0])
def test_bit_equal_to_the_fp32_kernel_and_the_filter_really_runs(ops, shape, scale):
    """relu(randn) * scale: at C = 100, scales 30 and 40 put |row|^2 at 45 000 +- 10 000 and 80 000 +- 18 000 -- mixtures of rows
    inside and outside fp16's domain on both sides.  Inside the domain (scales <= 3) nothing may be rescued: every pair's
    arg-min row is a listed candidate."""
    N, M, C, n_ids = shape
    q, k, lab = _case(N + M, N, M, C, n_ids, scale)
    got, want, st = _match(ops, k, q, lab, n_ids)
    assert torch.equal(got, want)
    assert torch.equal(ops.global_match(k, q, lab, n_ids, compute="f16r"), want)  # (the one-call route)
    print("scale %g %s: %.2f rows per pair, rescued %d / %d" % (scale, shape, st["candidate_rows_per_pair"], st["rescued_tiles"],
                                                                st["query_tiles"]))
    if scale <= 3.0:
        assert st["rescued_tiles"] == 0 and st["list_overflowed"] == 0 and st["candidate_rows"] >= N * n_ids, st


@pytest.mark.parametrize("where", ["bank_row_in_prepass_sample", "bank_row_outside_sample", "query_row", "bank_inf_element",
                                   "query_inf_element"])
def test_rows_outside_fp16s_domain_take_the_exact_route(ops, where):
    """a finite row with |row|^2 = 160 000 x its old value (far beyond 65504), or one +inf element: the fp16 image has NaN for
    it, fp32 has a distance.  A bank row concerns every query (every tile is rescued), a query row its own tile."""
    N, M, C, n_ids = 700, 9000, 100, 3
    q, k, lab = _case(77, N, M, C, n_ids, 0.2)
    if where == "bank_row_in_prepass_sample":
        k[int(torch.nonzero(lab == 1)[0])] *= 400.0      # first row of object 1: tile 0 of the object, always sampled
    if where == "bank_row_outside_sample":
        k[int(torch.nonzero(lab == 1)[200])] *= 400.0    # a row of the object's 4th tile: not in the 1-in-8 sample
    if where == "query_row":
        q[123] *= 400.0
    if where == "bank_inf_element":
        k[int(torch.nonzero(lab == 2)[70]), 5] = float("inf")
    if where == "query_inf_element":
        q[300, 9] = float("inf")
    got, want, st = _match(ops, k, q, lab, n_ids)
    assert _same_with_nans(got, want)
    if where in ("query_row", "query_inf_element"):
        assert st["rescued_tiles"] == 1, st
    else:  # every 256-query tile that holds a query (the padded fourth one holds none)
        assert st["rescued_tiles"] == (N + 255) // 256 == 3 and st["query_tiles"] == 4, st
    if where in ("bank_row_in_prepass_sample", "bank_row_outside_sample", "query_row"):
        assert not bool(torch.isnan(want).any())  # (fp32 has finite distances for all of these: nothing here is a NaN test)
    mem_a, mem_b = torch.full((N, n_ids), 0.4, device="cuda"), torch.full((N, n_ids), 0.4, device="cuda")
    a = ops.global_match(k, q, lab, n_ids, compute="f32", normalize=True, mem=mem_a)
    b = ops.global_match(k, q, lab, n_ids, compute="f16r", normalize=True, mem=mem_b)
    assert _same_with_nans(a, b) and _same_with_nans(mem_a, mem_b)


@pytest.mark.parametrize("where", ["bank_row_in_prepass_sample", "bank_row_outside_sample", "query_row", "both"])
def test_nan_embeddings_propagate_like_the_fp32_kernel(ops, where):
    N, M, C, n_ids = 700, 9000, 100, 3
    q, k, lab = _case(77, N, M, C, n_ids, 0.2)
    if where in ("bank_row_in_prepass_sample", "both"):
        k[int(torch.nonzero(lab == 1)[0])] = float("nan")
    if where == "bank_row_outside_sample":
        k[int(torch.nonzero(lab == 1)[200])] = float("nan")
    if where in ("query_row", "both"):
        q[123, 7] = float("nan")
    got, want, st = _match(ops, k, q, lab, n_ids)
    assert _same_with_nans(got, want)
    assert st["rescued_tiles"] == 0, st  # (bf16r's semantics: a NaN row settles its pairs, nothing is rescued for it)
    if where != "query_row":
        assert bool(torch.isnan(got[:, 1]).all()) and not bool(torch.isnan(got[:123, 0]).any())
    if where in ("query_row", "both"):
        assert bool(torch.isnan(got[123]).all())
    mem_a, mem_b = torch.full((N, n_ids), 0.4, device="cuda"), torch.full((N, n_ids), 0.4, device="cuda")
    a = ops.global_match(k, q, lab, n_ids, compute="f32", normalize=True, mem=mem_a)
    b = ops.global_match(k, q, lab, n_ids, compute="f16r", normalize=True, mem=mem_b)
    assert _same_with_nans(a, b) and _same_with_nans(mem_a, mem_b)


@pytest.mark.parametrize("scale", [0.1, 0.0005])
def test_fp16_subnormal_elements(ops, scale):
    """5 % of the elements nonzero below 2^-14 (fp16 subnormals: the matrix pipe may keep or flush them, the threshold pays for
    either), and a band of rows -- bank and query -- whose EVERY element is below 2^-14, norms below 2^-6 (the scaled norm
    pieces drop up to 2^-28 there).  scale 0.0005: every embedding at that size."""
    N, M, C, n_ids = 700, 6000, 100, 3
    q, k, lab = _case(31, N, M, C, n_ids, scale)
    g = torch.Generator(device="cuda").manual_seed(32)
    for t in (q, k):
        tiny = (torch.rand(t.shape, generator=g, device="cuda") + 0.01) * 2.0 ** -14 * 0.99
        sign = torch.where(torch.rand(t.shape, generator=g, device="cuda") < 0.5, -1.0, 1.0)
        m = torch.rand(t.shape, generator=g, device="cuda") < 0.05
        t[m] = (tiny * sign)[m]
    k[1000:1400] = (torch.rand(400, C, generator=g, device="cuda") + 0.01) * 2.0 ** -14 * 0.99
    q[200:300] = (torch.rand(100, C, generator=g, device="cuda") + 0.01) * 2.0 ** -14 * 0.99
    assert float(k[1000:1400].pow(2).sum(1).max()) < 2.0 ** -6
    got, want, st = _match(ops, k, q, lab, n_ids)
    assert torch.equal(got, want)
    print("subnormals, scale %g: %.2f rows per pair, rescued %d / %d" % (scale, st["candidate_rows_per_pair"], st["rescued_tiles"],
                                                                        st["query_tiles"]))
    assert st["rescued_tiles"] == 0 and st["candidate_rows"] >= N * n_ids, st


def test_scribble_banks_empty_objects_and_the_fused_epilogue(ops):
    N, M, C, n_ids = 1500, 6000, 100, 5
    q, k, lab = _case(5, N, M, C, n_ids, 0.2, unlabelled=0.9)
    lab[lab == 3] = -1  # object 3 has no row at all -> the padding distance 1e20 -> 1.0 after normalisation
    mem_a, mem_b = torch.full((N, n_ids), 0.4, device="cuda"), torch.full((N, n_ids), 0.4, device="cuda")
    want = ops.global_match(k, q, lab, n_ids, compute="f32", normalize=True, mem=mem_a)
    got = ops.global_match(k, q, lab, n_ids, compute="f16r", normalize=True, mem=mem_b)
    assert torch.equal(got, want) and torch.equal(mem_a, mem_b)
    raw = ops.global_match(k, q, lab, n_ids, compute="f16r")
    assert torch.equal(raw, ops.global_match(k, q, lab, n_ids, compute="f32")) and bool((raw[:, 3] == 1e20).all())
    lab[:] = -1  # an all-unlabelled bank
    assert bool((ops.global_match(k, q, lab, n_ids, compute="f16r") == 1e20).all())


def test_prepared_bank_frames_and_2_byte_storage(ops):
    C, h, w, n_ids = 100, 40, 50, 3
    g = torch.Generator(device="cuda").manual_seed(8)
    emb = torch.relu(torch.randn(3, C, h, w, generator=g, device="cuda")) * 0.3
    lab = torch.randint(-1, n_ids, (2 * h * w,), generator=g, device="cuda", dtype=torch.int32)
    for storage in (torch.float32, torch.bfloat16):
        e = emb.to(storage)
        bank_rows = e[:2].permute(0, 2, 3, 1).reshape(-1, C)  # a stacked 2-frame bank
        want = ops.PreparedBank(bank_rows, lab, n_ids, compute="f32").match(e[2].permute(1, 2, 0))
        bank = ops.PreparedBank(bank_rows, lab, n_ids, compute="f16r")
        assert torch.equal(bank.match(e[2].permute(1, 2, 0)), want)
        for prep in ("f16r", "f16"):  # a frame prepared for plain fp16 carries the same operand image
            assert torch.equal(bank.match(ops.prepare_frames(e[2], compute=prep, max_distance=4)), want)
            assert torch.equal(bank.match(ops.PackedQuery(e[2].permute(1, 2, 0), compute=prep)), want)
        cands, over = bank.refine_stats()
        assert over == 0 and h * w <= cands < 16 * h * w * n_ids
        with pytest.raises(ValueError, match="packed for"):  # (a bf16 image is not an fp16 image)
            bank.match(ops.PackedQuery(e[2].permute(1, 2, 0), compute="bf16r"))


def test_adversarial_duplicate_rows_dense_blocks_and_beyond(ops):
    """tests/test_bf16_refine.py's banks of 40 / 2 200 / 11 000 copies of six rows, with the statistics it asserts"""
    N, C, n_ids = 300, 100, 2
    g = torch.Generator(device="cuda").manual_seed(21)
    q = torch.relu(torch.randn(N, C, generator=g, device="cuda")) * 0.2
    base = torch.relu(torch.randn(6, C, generator=g, device="cuda")) * 0.2
    for copies, rescued in ((40, False), (2200, False), (11000, True)):
        k = base.repeat(copies, 1)
        lab = (torch.arange(6 * copies, device="cuda") % 6 < 3).to(torch.int32)
        got, want, st = _match(ops, k, q, lab, n_ids)
        assert torch.equal(got, want)
        assert st["candidate_rows"] > 0
        if rescued:
            assert st["list_overflowed"] == 1 and st["rescued_tiles"] == st["query_tiles"] > 0
        else:
            assert st["list_overflowed"] == 0 and st["rescued_tiles"] == 0


def test_partly_degenerate_embeddings_rescue_only_their_blocks(ops):
    """tests/test_bf16_refine.py's band of identical embeddings, with the statistics it asserts"""
    H, W, n_ids = 40, 64, 2
    g = torch.Generator(device="cuda").manual_seed(9)
    q = torch.relu(torch.randn(100, H, W, generator=g, device="cuda")) * 0.2
    const = torch.relu(torch.randn(100, generator=g, device="cuda")) * 0.2
    q[:, 10:20, :] = const[:, None, None]
    for frames, rescued in ((1, False), (16, True)):
        ref = torch.relu(torch.randn(frames, 100, H, W, generator=g, device="cuda")) * 0.2
        ref[0, :, 5:30, :] = (const * 1.001)[:, None, None]
        ref[1:] = (const * 1.001)[None, :, None, None]
        lab = torch.randint(0, n_ids, (frames * H * W,), generator=g, device="cuda", dtype=torch.int32)
        got, want, st = _match(ops, ref.permute(0, 2, 3, 1).reshape(-1, 100), q.permute(1, 2, 0), lab, n_ids)
        assert torch.equal(got, want)
        if rescued:  # queries 640 .. 1279 are the band: tiles 2, 3, 4 of the 10
            assert st["list_overflowed"] == 1 and 0 < st["rescued_tiles"] <= 4 and st["query_tiles"] == 10
        else:
            assert st["list_overflowed"] == 0 and st["rescued_tiles"] == 0


def test_spatially_smooth_embeddings_do_not_overflow(ops):
    import torch.nn.functional as F
    H, W, T, n_ids = 60, 107, 4, 3
    g = torch.Generator(device="cuda").manual_seed(8)
    for coarse, noise in ((8, 0.1), (16, 0.0)):
        base = torch.randn(1, 100, H // coarse + 2, W // coarse + 2, generator=g, device="cuda")
        frames = []
        for i in range(T + 1):
            f = F.interpolate(base + 0.05 * i * torch.randn(base.shape, generator=g, device="cuda"), size=(H, W),
                              mode="bilinear", align_corners=True)[0]
            frames.append(torch.relu(f + noise * torch.randn(100, H, W, generator=g, device="cuda")) * 0.1)
        bank_rows = torch.stack(frames[:T]).permute(0, 2, 3, 1).reshape(-1, 100)
        lab = torch.randint(0, n_ids, (T * H * W,), generator=g, device="cuda", dtype=torch.int32)
        got, want, st = _match(ops, bank_rows, frames[T].permute(1, 2, 0), lab, n_ids)
        assert torch.equal(got, want)
        print("smooth, coarse %d: %.2f rows per pair" % (coarse, st["candidate_rows_per_pair"]))
        assert st["list_overflowed"] == 0 and st["rescued_tiles"] == 0 and st["candidate_rows_per_pair"] < 16.0


@pytest.mark.parametrize("C", [4, 7, 16, 26, 30, 50, 99, 101, 106])
@pytest.mark.parametrize("storage", [torch.float32, torch.bfloat16])
def test_channel_counts_and_ragged_sizes(ops, C, storage):
    """both filter instantiations (2 and 7 k-steps), channel counts on both sides of a 16-byte unit, the norm slots in their own
    unit or sharing one with channels; near-duplicate rows so that whole blocks qualify (dense entries)"""
    N, n_ids = 333, 3
    g = torch.Generator(device="cuda").manual_seed(1000 + C)
    base = torch.relu(torch.randn(5, C, generator=g, device="cuda")) * 0.3 + 0.05
    M = 5 * 131  # 655 rows: objects end inside tiles
    k = (base.repeat(131, 1) + 2e-4 * torch.randn(M, C, generator=g, device="cuda")).to(storage)
    lab = (torch.arange(M, device="cuda") % n_ids).to(torch.int32)
    q = (base[torch.randint(0, 5, (N,), generator=g, device="cuda")] + 2e-4 * torch.randn(N, C, generator=g, device="cuda")).to(storage)
    got, want, st = _match(ops, k, q, lab, n_ids)
    assert torch.equal(got, want), (C, storage)
    assert st["rescued_tiles"] == 0 and st["candidate_rows"] >= N * n_ids, st


@pytest.fixture(scope="module")
def encoder_embeddings():
    """two frames of the example's stand-in encoder at 240 x 428 -> [2, C, 60, 107] (what the issue's CPU simulation used)"""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import propagate_clip as pc
    from cvpr2020_manet_amd.networks import IntVOS as M
    saved = M.cfg
    try:
        dev = torch.device("cuda:0")
        cfg, model = pc.build_model(dev)
        emb = pc.synthetic_clip(model, dev, 2, 240, 428, 3)
    finally:
        M.set_cfg(saved)
    return emb.float().contiguous()


def test_it_filters_better_than_bf16_on_an_encoders_embeddings(ops, encoder_embeddings):
    """the bank is frame 0 with 3 random ids, the queries are frame 1: correlated embeddings, where bf16r keeps tens of rows per
    pair.  f16r must keep at most HALF of bf16r's candidate rows per pair on the same tensors (the threshold's leading term is
    8x smaller; the real pre-pass and tightening schedule take their share).  If bf16r overflowed its lists its figure is a
    lower bound, which only makes the comparison harder for it to lose."""
    emb = encoder_embeddings
    C, h, w = emb.shape[1:]
    g = torch.Generator(device="cuda").manual_seed(3)
    lab = torch.randint(0, 3, (h * w,), generator=g, device="cuda", dtype=torch.int32)
    k, q = emb[0].permute(1, 2, 0).reshape(-1, C), emb[1].permute(1, 2, 0)
    want = ops.global_match(k, q, lab, 3, compute="f32")
    st = {}
    for mode in ("bf16r", "f16r"):
        bank = ops.PreparedBank(k, lab, 3, compute=mode)
        assert torch.equal(bank.match(q, adaptive=False), want), mode
        st[mode] = bank.refine_stats_full()
        print("%s: %.2f candidate rows per pair, rescued %d / %d, overflowed %d" % (
            mode, st[mode]["candidate_rows_per_pair"], st[mode]["rescued_tiles"], st[mode]["query_tiles"], st[mode]["list_overflowed"]))
    assert st["f16r"]["rescued_tiles"] == 0 and st["f16r"]["list_overflowed"] == 0, st
    assert st["f16r"]["candidate_rows_per_pair"] <= 0.5 * st["bf16r"]["candidate_rows_per_pair"], st


@pytest.fixture
def module_cfg_restored():
    """building an IntVOS installs its cfg as the module-level default of networks.IntVOS: put the previous one back"""
    from cvpr2020_manet_amd.networks import IntVOS as M
    saved = M.cfg
    yield
    M.set_cfg(saved)


def test_end_to_end_through_the_module(module_cfg_restored):
    """IntVOS(cfg, fe, compute="f16r") against the compute="f32" model: global maps, local maps and logits are EQUAL"""
    from test_intvos_module import build_model, run_script
    g = load_golden("e2e_tiny")
    model = build_model(g, "cuda", compute="f16r")
    assert model.compute == "f16r"
    a, b = run_script(build_model(g, "cuda", compute="f32"), g, "cuda"), run_script(model, g, "cuda")
    for key in ("gmap_round1", "gmap_round2", "lmap_tmp", "lmap_dist", "int_logits", "prop1_logits_2", "prop1_logits_3", "int2_logits",
                "prop2_logits_3", "forward_logits"):
        assert torch.equal(a[key], b[key]), key


def test_errors_are_loud(ops):
    q, k, lab = _case(1, 100, 500, 120, 2)  # C = 120 needs the narrow kernel: not offered in this mode
    with pytest.raises(RuntimeError, match="MANET_COMPUTE_F16_REFINE supports C <= 106"):
        ops.global_match(k, q, lab, 2, compute="f16r")
    q, k, lab = _case(1, 100, 500, 100, 2)
    with pytest.raises(RuntimeError, match="k_nn"):
        ops.global_match(k, q, lab, 2, compute="f16r", k_nearest_neighbors=2)
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.PreparedBank(k, lab, 2, compute="f16r").match(q.clone().requires_grad_(True))


def test_fuzz_structured_banks(ops):
    """tools/fuzz_bf16r.py with compute="f16r": its mixture of structured banks plus the domain-edge scales 30 and 40"""
    from tools import fuzz_bf16r
    assert fuzz_bf16r.run(150, 20200614, verbose=False, compute="f16r") == 0
