"""compute="f16" (MANET_COMPUTE_F16) of the global match on the GPU: v_mfma_f32_32x32x16_f16 on embeddings rounded to fp16.

The mode IS the reference formula d = |q~|^2 + |k~|^2 - 2 q~.k~ on x~ = fp32(fp16(x)), norms in fp32 from the rounded values,
products exact, fp32 accumulation inside the MFMA.  On inputs that are fp16 values already it therefore differs from the fp32
kernel (and from the oracle) by the accumulation order alone: the tolerance of the bf16 mode's test of the same statement
(test_gpu_global.BF16_RTOL / BF16_ATOL), for the same reason.  The error against UNROUNDED embeddings at full size is
test_f16_error_bound.py's."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_global import BF16_ATOL, BF16_RTOL, _case, chw_view, dev

pytestmark = pytest.mark.gpu

RTOL, ATOL = BF16_RTOL, BF16_ATOL  # 1e-5, 3e-6: accumulation order only
F16_MIN_NORMAL = 2.0 ** -14
PAD = np.float32(1e20)


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


def hwc(chw):
    return np.ascontiguousarray(np.transpose(chw, (1, 2, 0)))


def _want(oracle, q, k, lab, n_ids):
    return oracle.global_match(hwc(k), hwc(q), lab, 1, n_ids=n_ids).reshape(-1, n_ids)


def _exact_case(seed, h, w, hr, wr, C, n_ids, scale, unlabeled_frac=0.0):
    q, k, lab = _case(seed, h, w, hr, wr, C, n_ids, unlabeled_frac=unlabeled_frac, scale=scale)
    return h16(q), h16(k), lab


def _spread_norms(seed):
    """rows whose squared norms span 0.02 .. 0.5 (the norm slots' pieces change scale across that range)"""
    q, k, lab = _case(seed, 16, 12, 16, 12, 100, 2, unlabeled_frac=0.0, scale=0.1)
    rng = np.random.default_rng(seed)
    for a in (q, k):
        target = rng.uniform(0.02, 0.5, size=a.shape[1:]).astype(np.float32)
        a *= np.sqrt(target / np.maximum((a * a).sum(0), 1e-12))[None]
    q, k = h16(q), h16(k)
    n2 = np.concatenate([(q * q).sum(0).ravel(), (k * k).sum(0).ravel()])
    assert n2.min() < 0.03 and n2.max() > 0.45
    return q, k, lab


def _empty_id_case(seed):
    q, k, lab = _exact_case(seed, 24, 32, 48, 32, 100, 3, 0.3, unlabeled_frac=0.3)
    lab[lab == 1] = -1  # object 1 has no rows; ~30 % of the labels were -1 already
    assert (lab == -1).mean() > 0.3 and (lab == 0).any() and (lab == 2).any()
    return q, k, lab


# name -> (inputs, n_ids).  h x w query, bank, C, ids, scale
CASES = {
    "two_k_steps_C20": lambda: (_exact_case(101, 13, 10, 12, 10, 20, 2, 0.1), 2),
    "C100_empty_id": lambda: (_empty_id_case(102), 3),
    "C106_wide": lambda: (_exact_case(103, 16, 16, 16, 16, 106, 3, 0.2), 3),
    "C107_narrow": lambda: (_exact_case(104, 16, 16, 16, 16, 107, 3, 0.5), 3),
    "C128": lambda: (_exact_case(105, 16, 16, 16, 16, 128, 3, 0.1), 3),
    "N513_M65": lambda: (_exact_case(106, 27, 19, 13, 5, 100, 2, 0.4), 2),  # one past the 512-query and the 64-row tile
    "norms_0.02_to_0.5": lambda: (_spread_norms(107), 2),
}
_cache = {}


def case(name, oracle):
    """(q, k, lab, n_ids, oracle result on the fp16-exact inputs): made once, shared, never written to"""
    if name not in _cache:
        (q, k, lab), n_ids = CASES[name]()
        want = _want(oracle, q, k, lab, n_ids)
        _cache[name] = (q, k, lab, n_ids, want)
    return _cache[name]


# ---- 1. against the fp32 kernel and the oracle on identical values

@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_fp32_arithmetic_on_fp16_exact_inputs(ops, oracle, name):
    q, k, lab, n_ids, want = case(name, oracle)
    assert not np.any((np.abs(q) < F16_MIN_NORMAL) & (q != 0)) and not np.any((np.abs(k) < F16_MIN_NORMAL) & (k != 0))
    got = ops.global_match(chw_view(k), chw_view(q), dev(lab), n_ids, compute="f16").cpu().numpy()
    f32 = ops.global_match(chw_view(k), chw_view(q), dev(lab), n_ids, compute="f32").cpu().numpy()
    print("%s: max |f16 - f32| %.3g, max |f16 - oracle| %.3g" % (name, np.abs(got - f32).max(), np.abs(got - want).max()))
    np.testing.assert_allclose(got, f32, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    if name == "C100_empty_id":
        assert np.all(got[:, 1] == PAD) and np.all(got[:, [0, 2]] < 1e3)  # the padding of an id without rows: exactly 1e20


# ---- 2. every route gives the same bits

@pytest.mark.parametrize("shape", [(100, 24, 32, 4), (37, 9, 15, -1), (107, 10, 14, 2)])  # even w, odd w (generic staging), C > 106
def test_routes_agree_bit_for_bit(ops, shape):
    C, h, w, d = shape
    rng = np.random.default_rng(C)
    e = torch.from_numpy((np.maximum(rng.standard_normal((2, C, h, w)), 0) * 0.3).astype(np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(-1, 3, size=(h * w,)).astype(np.int32)).cuda()
    q_chw, k_chw = e[0], e[1]
    q_view, k_view = q_chw.permute(1, 2, 0), k_chw.permute(1, 2, 0)  # C-major storage seen as [h, w, C]
    base = ops.global_match(k_view, q_view, lab, 3, compute="f16")
    bank = ops.PreparedBank(k_view.contiguous(), lab, 3, compute="f16")  # row-major bank
    outs = {
        "bank.match(view)": bank.match(q_view),
        "bank.match(row-major)": bank.match(q_view.contiguous()),
        "bank.match(PackedQuery)": bank.match(ops.PackedQuery(q_view, compute="f16")),
        "bank.match(PreparedFrame)": bank.match(ops.prepare_frames(q_chw, compute="f16", max_distance=d)),
        "bank.match(PreparedFrame of a strided view)": bank.match(
            ops.prepare_frames(q_view.contiguous().permute(2, 0, 1), compute="f16", max_distance=d)),
    }
    # through the embedding layer's epilogue: relu(x * 1 + 0) is x (the inputs are >= 0)
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    emb, frames = ops.embed_finish(e[0:1], one, zero, relu=True, emb_dtype=torch.float32, compute="f16", max_distance=d)
    assert torch.equal(emb[0], q_chw)
    outs["bank.match(embed_finish frame)"] = bank.match(frames[0])
    for name, o in outs.items():
        assert torch.equal(o, base), name
    # bf16-stored embeddings are rounded from their fp32 value: the same bits as fp32 storage of those values
    qb, kb = q_view.bfloat16(), k_view.bfloat16()
    want = ops.global_match(kb.float(), qb.float(), lab, 3, compute="f16")
    assert torch.equal(ops.global_match(kb, qb, lab, 3, compute="f16"), want)
    bank_b = ops.PreparedBank(kb, lab, 3, compute="f16")
    assert torch.equal(bank_b.match(ops.prepare_frames(q_chw.bfloat16(), compute="f16", max_distance=d)), want)
    emb_b, frames_b = ops.embed_finish(e[0:1], one, zero, relu=True, emb_dtype=torch.bfloat16, compute="f16", max_distance=d)
    assert torch.equal(emb_b[0], q_chw.bfloat16()) and torch.equal(bank_b.match(frames_b[0]), want)
    if d >= 0:  # the frame's other operand, the pooled plane of the local match, does not depend on the arithmetic mode
        f16f = ops.prepare_frames(e, compute="f16", max_distance=d)
        f32f = ops.prepare_frames(e, compute="f32", max_distance=d)
        plab = lab.clamp(min=0)
        assert torch.equal(ops.local_match_frames(f16f[1], f16f[0], plab, 3), ops.local_match_frames(f32f[1], f32f[0], plab, 3))


def test_an_operand_packed_for_another_kind_is_refused(ops):
    q, k, lab = _case(7, 8, 8, 8, 8, 100, 2)
    bank16 = ops.PreparedBank(chw_view(k), dev(lab), 2, compute="f16")
    bankbf = ops.PreparedBank(chw_view(k), dev(lab), 2, compute="bf16")
    for kind, bank in (("bf16", bank16), ("bf16r", bank16), ("f32", bank16), ("f16", bankbf)):
        with pytest.raises(ValueError, match="packed for"):
            bank.match(ops.prepare_frames(dev(q), compute=kind))
        with pytest.raises(ValueError, match="packed for"):
            bank.match(ops.PackedQuery(chw_view(q), compute=kind))
    assert bank16.match(ops.PackedQuery(chw_view(q), compute="fp16")).shape == (64, 2)  # "fp16" is the same mode


# ---- 3. epilogue

def test_fused_normalise_and_merge_equal_the_separate_operations(ops):
    q, k, lab = _case(31, 20, 24, 20, 24, 100, 3, scale=0.3)
    q2 = _case(32, 20, 24, 20, 24, 100, 3, scale=0.3)[0]
    rng = np.random.default_rng(3)
    mem0 = torch.from_numpy(rng.random((20 * 24, 3)).astype(np.float32)).cuda()
    mem, mem_ref = mem0.clone(), mem0.clone()
    for qq in (q, q2):  # two successive merges into the same stored map
        fused = ops.global_match(chw_view(k), chw_view(qq), dev(lab), 3, compute="f16", normalize=True, mem=mem)
        raw = ops.global_match(chw_view(k), chw_view(qq), dev(lab), 3, compute="f16")
        sep = ops.normalize_merge_(raw.clone(), mem_ref, normalize=True)
        assert torch.equal(fused, sep) and torch.equal(mem, mem_ref) and torch.equal(fused, mem)
        assert torch.equal(ops.global_match(chw_view(k), chw_view(qq), dev(lab), 3, compute="f16", normalize=True),
                           ops.normalize_merge_(raw.clone(), None, normalize=True))
    assert not torch.equal(mem, mem0)


# ---- 4. determinism

def test_runs_and_bank_row_order_give_the_same_bits(ops):
    q, k, lab = _case(41, 30, 40, 60, 40, 100, 4, scale=0.3)
    rows, labs = chw_view(k).reshape(-1, 100), dev(lab).reshape(-1)
    a = ops.global_match(rows, chw_view(q), labs, 4, compute="f16")
    assert torch.equal(ops.global_match(rows, chw_view(q), labs, 4, compute="f16"), a)
    perm = torch.from_numpy(np.random.default_rng(4).permutation(rows.shape[0])).cuda()
    assert torch.equal(ops.global_match(rows[perm], chw_view(q), labs[perm], 4, compute="f16"), a)


# ---- 5. domain

def test_a_bank_row_outside_fp16_makes_its_objects_column_nan(ops, oracle):
    """one element 300 (|k|^2 > 65504), then an infinity: NaN in that object's column for every query -- never a plausible
    distance -- and every other column still the reference's"""
    q, k0, lab, n_ids, want = case("C106_wide", oracle)  # 3 ids, every one with rows
    assert all((lab == o).any() for o in range(n_ids))
    row = np.argwhere(lab[:, :, 0] == 2)[3]
    for bad in (300.0, np.inf):
        k = k0.copy()
        k[5, row[0], row[1]] = bad
        got = ops.global_match(chw_view(k), chw_view(q), dev(lab), n_ids, compute="f16").cpu().numpy()
        assert np.all(np.isnan(got[:, 2])), bad
        np.testing.assert_allclose(got[:, :2], want[:, :2], rtol=RTOL, atol=ATOL)


def test_a_query_row_outside_fp16_is_nan_for_every_id(ops, oracle):
    """one query element 40 000 (|2 q| > 65504), then one whose square overflows fp32: that query is NaN for ALL of its ids, every
    other entry of the map still matches the reference; no bank row is outside the domain here"""
    q0, k, lab, n_ids, want = case("C106_wide", oracle)
    assert all((lab == o).any() for o in range(n_ids))
    for bad, (y, x) in ((40000.0, (4, 9)), (3e30, (0, 0))):
        q = q0.copy()
        q[7, y, x] = bad
        nq = y * q.shape[2] + x
        got = ops.global_match(chw_view(k), chw_view(q), dev(lab), n_ids, compute="f16").cpu().numpy()
        assert np.all(np.isnan(got[nq])), (bad, got[nq])
        others = np.ones(got.shape[0], bool)
        others[nq] = False
        assert not np.isnan(got[others]).any()
        np.testing.assert_allclose(got[others], want[others], rtol=RTOL, atol=ATOL)
    # through a prepared frame (the per-frame route packs the query with another kernel)
    q = q0.copy()
    q[7, 4, 9] = 40000.0
    bank = ops.PreparedBank(chw_view(k), dev(lab), n_ids, compute="f16")
    got = bank.match(ops.prepare_frames(dev(q), compute="f16")).cpu().numpy()
    assert np.all(np.isnan(got[4 * 16 + 9])) and np.isnan(got).sum() == n_ids


def test_nan_inputs_propagate_as_in_bf16(ops, oracle):
    q, k, lab, n_ids, want = case("C100_empty_id", oracle)
    q, k = q.copy(), k.copy()
    row = np.argwhere(lab[:, :, 0] == 0)[0]
    k[3, row[0], row[1]] = np.nan
    q[2, 1, 1] = np.nan
    got = ops.global_match(chw_view(k), chw_view(q), dev(lab), n_ids, compute="f16").cpu().numpy()
    bf = ops.global_match(chw_view(k), chw_view(q), dev(lab), n_ids, compute="bf16").cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(bf))
    assert np.all(np.isnan(got[:, 0])) and np.all(np.isnan(got[33, [0, 2]]))
    ok = ~np.isnan(got)
    np.testing.assert_allclose(got[ok], want[ok], rtol=RTOL, atol=ATOL)


# ---- 6. fp16-subnormal elements

def test_subnormal_elements_move_a_distance_by_at_most_their_products(ops, oracle):
    """5 % of the elements are fp16 subnormals (multiples of 2^-24 below 2^-14).  Whether the matrix pipe keeps or flushes such
    operands is the hardware's choice: per (query, row) pair the distance may lose at most the products in which a subnormal takes
    part, 2 sum_c |q~_c| |k~_c| over those channels, plus the subnormal channels' share of the two norms.  The bound is computed
    from the inputs, so it holds either way; the behaviour seen is printed (DESIGN 4 records it)."""
    h, w, C, n_ids = 16, 16, 100, 2
    q, k, lab = _case(61, h, w, h, w, C, n_ids, unlabeled_frac=0.0, scale=0.3)
    q, k = h16(q), h16(k)
    rng = np.random.default_rng(61)
    for a in (q, k):
        m = rng.random(a.shape) < 0.05
        a[m] = (rng.integers(1, 1024, size=int(m.sum())) * 2.0 ** -24).astype(np.float32)
    assert np.array_equal(h16(q, keep_subnormals=True), q) and np.array_equal(h16(k, keep_subnormals=True), k)
    Q, K, L = hwc(q).reshape(-1, C).astype(np.float64), hwc(k).reshape(-1, C).astype(np.float64), lab.reshape(-1)
    sq, sk = (Q != 0) & (Q < F16_MIN_NORMAL), (K != 0) & (K < F16_MIN_NORMAL)
    assert 0.03 < sq.mean() < 0.07 and 0.03 < sk.mean() < 0.07
    # sum over the channels where either side is subnormal = (q on its subnormals).k + q.(k on its subnormals) - both
    cross = (Q * sq) @ K.T + Q @ (K * sk).T - (Q * sq) @ (K * sk).T
    slack = 2.0 * cross + ((Q * sq) ** 2).sum(1)[:, None] + ((K * sk) ** 2).sum(1)[None, :]
    want = _want(oracle, q, k, lab, n_ids)  # fp32 arithmetic keeps every subnormal fp16 value: it is a normal fp32 number
    got = ops.global_match(chw_view(k), chw_view(q), dev(lab), n_ids, compute="f16").cpu().numpy()
    for o in range(n_ids):  # |min_m a - min_m b| <= max_m |a - b|
        bound = ATOL + RTOL * np.abs(want[:, o]) + slack[:, L == o].max(1)
        err = np.abs(got[:, o].astype(np.float64) - want[:, o])
        print("object %d: max err %.3g, max allowed %.3g, max err without the subnormal term %.3g"
              % (o, err.max(), bound.max(), (ATOL + RTOL * np.abs(want[:, o])).max()))
        assert np.all(err <= bound)
    # which behaviour: one subnormal query element against a bank element of 16 -- kept: d moves by 2 * 2^-15 * 16 = 2^-10
    qq, kk = np.zeros((C, 1, 1), np.float32), np.zeros((C, 1, 1), np.float32)
    qq[0], kk[0], qq[1], kk[1] = 2.0 ** -15, 16.0, 1.0, 1.0
    d = ops.global_match(chw_view(kk), chw_view(qq), dev(np.zeros((1, 1, 1), np.int32)), 1, compute="f16").item()
    flushed = (1.0 + 2.0 ** -30) + (1.0 + 256.0) - 2.0
    kept = flushed - 2.0 ** -10
    print("fp16 subnormal operand in v_mfma_f32_32x32x16_f16: d = %.6f (kept: %.6f, flushed: %.6f) -> %s"
          % (d, kept, flushed, "kept" if abs(d - kept) < abs(d - flushed) else "flushed"))
    assert min(abs(d - kept), abs(d - flushed)) < 1e-4


# ---- 7. refusals

def test_top_k_and_autograd_are_refused(ops):
    q, k, lab = _case(71, 8, 8, 8, 8, 100, 2, unlabeled_frac=0.0)
    with pytest.raises(RuntimeError, match="k_nn > 1 needs"):
        ops.global_match(chw_view(k), chw_view(q), dev(lab), 2, k_nearest_neighbors=2, compute="f16")
    with pytest.raises(RuntimeError, match="k_nn > 1 needs"):
        ops.PreparedBank(chw_view(k), dev(lab), 2, compute="f16").match(chw_view(q), k_nearest_neighbors=2)
    qg = chw_view(q).clone().requires_grad_(True)
    for mode in ("f16", "bf16"):  # as the other non-fp32 modes
        with pytest.raises(RuntimeError, match="backward exists for compute='f32'"):
            ops.global_match(chw_view(k), qg, dev(lab), 2, compute=mode)
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.PreparedBank(chw_view(k), dev(lab), 2, compute="f16").match(qg)


# ---- 9. through the module

@pytest.fixture
def module_cfg_restored():
    """building an IntVOS installs its cfg as the module-level default of networks.IntVOS: put the previous one back"""
    from cvpr2020_manet_amd.networks import IntVOS as M
    saved = M.cfg
    yield
    M.set_cfg(saved)


def test_end_to_end_f16_through_the_module(module_cfg_restored):
    """IntVOS(cfg, fe, compute="f16") on fp32-stored embeddings against the compute="f32" model on the same GPU: global maps
    within the 1e-3 bar, local maps bit-equal (the local match does not use the mode), and no logit further from the fp32
    model's than the compute="bf16" model's."""
    from test_intvos_module import build_model, run_script
    g = load_golden("e2e_tiny")
    outs = {c: run_script(build_model(g, "cuda", compute=c), g, "cuda") for c in ("f32", "f16", "bf16")}
    assert build_model(g, "cuda", compute="f16").compute == "f16"
    for key in ("gmap_round1", "gmap_round2"):
        err = (outs["f16"][key] - outs["f32"][key]).abs().max().item()
        print("%s: max |f16 - f32| %.3g (bf16: %.3g)" % (key, err, (outs["bf16"][key] - outs["f32"][key]).abs().max().item()))
        assert err <= 1e-3, (key, err)
    for key in ("lmap_tmp", "lmap_dist"):
        assert torch.equal(outs["f16"][key], outs["f32"][key]), key
    for key in ("int_logits", "prop1_logits_2", "prop1_logits_3", "int2_logits", "prop2_logits_3", "forward_logits"):
        e16 = (outs["f16"][key] - outs["f32"][key]).abs().max().item()
        ebf = (outs["bf16"][key] - outs["f32"][key]).abs().max().item()
        print("%s: max logit error f16 %.3g, bf16 %.3g (max |logit| %.3g)" % (key, e16, ebf, outs["f32"][key].abs().max().item()))
        assert e16 <= ebf, (key, e16, ebf)
