"""GPU: the half-precision (fp16) storage type of the stored local-match volumes (opt-in; ops.local_volumes(..., dtype=torch.float16),
IntVOS(local_volume_dtype="f16")).

Contract (include/manet_hip.h).  Phase 1 runs the fp32 arithmetic up to and including the normalisation, then rounds every distance
ONCE to IEEE half, to nearest even, subnormals kept; the tail widens the taps to fp32 exactly and evaluates the fp32 tail's
expression in the same association.  Hence

  * the TIE: the tail on an fp16 volume == the fp32 tail on the fp32 volume rounded to half and widened again, bit for bit -- this
    pins the conversion and the expression without constraining the image layout;
  * the BOUND: stored values lie in [0, 1], round-to-nearest half has a relative error <= 2^-11 on normal numbers (absolute
    <= 2^-12 below 1.0, <= 2^-25 below 6.1e-5), the bilinear sample is a convex combination of four taps and the masked minimum is
    1-Lipschitz, so |out_f16 - out_f32| <= min(2^-12, 2^-11 * out_f32) and an entry that is 1.0 stays exactly 1.0.  Against the CPU
    oracle the fp32 route's own distance to it (RTOL, ATOL of tests/test_gpu_local.py) comes on top."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 2e-6  # the fp32 route's distance to the oracle (tests/test_gpu_local.py)
F16 = torch.float16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cvpr2020_manet_amd import ops as o
    return o


def assert_tie(ops, v16, v32, frame, lab, n_ids, what):
    """the fp16 tail == the fp32 tail on the rounded fp32 volume, with a fresh and with a pre-set output"""
    assert v16.dtype == F16 and v32.dtype == torch.float32
    want = ops.local_match_volume(v32.half().float(), frame, lab, n_ids)
    got = ops.local_match_volume(v16, frame, lab, n_ids)
    assert torch.equal(got, want), what
    pre = torch.ones((frame.h, frame.w, n_ids), dtype=torch.float32, device="cuda")
    got2 = ops.local_match_volume(v16, frame, lab, n_ids, out=pre, out_is_preset=True)
    assert torch.equal(got2, want), what
    return got


def assert_bound(got, ref, what):
    """|got - ref| <= min(2^-12, 2^-11 |ref|) + (RTOL |ref| + ATOL); 1.0 stays 1.0"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    bound = np.minimum(2.0 ** -12, 2.0 ** -11 * np.abs(ref)) + (RTOL * np.abs(ref) + ATOL)
    print("%s: max |f16 - ref| = %.3e (bound there %.3e), mean %.3e" % (what, err.max(), bound.flat[err.argmax()], err.mean()))
    assert (err <= bound).all(), (what, float(err.max()), float((err - bound).max()))
    assert (got[ref == 1.0] == 1.0).all(), what


CASES = ((58, 53, 71, 11, torch.float32), (7, 9, 100, 2, torch.float32), (33, 30, 54, 3, torch.bfloat16))
PAIRS = [(0, 1), (1, 2), (2, 3), (3, 2), (2, 1), (1, 0), (2, 2)]  # forwards, backwards, a frame against itself


def _case(ops, rng, C, h, w, n_ids, dtype, d):
    embs = torch.from_numpy((np.maximum(rng.standard_normal((4, C, h, w)), 0) * 0.2).astype(np.float32)).cuda().to(dtype)
    labs = torch.from_numpy(rng.integers(-1, n_ids + 1, size=(4, h, w)).astype(np.int32)).cuda()
    frames = ops.prepare_frames(embs, compute="f32", max_distance=d)
    prevs, curs = [frames[a] for a, _ in PAIRS], [frames[b] for _, b in PAIRS]
    return embs, labs, frames, prevs, curs


@pytest.mark.parametrize("d", range(13))
def test_f16_tail_equals_the_f32_tail_on_the_rounded_volume(ops, d):
    """every instantiation d = 0..12, ragged grids, more ids than one per-pixel pass holds, fp32 and 2-byte embeddings, seven pairs"""
    rng = np.random.default_rng(6200 + d)
    for (C, h, w, n_ids, dtype) in CASES:
        embs, labs, frames, prevs, curs = _case(ops, rng, C, h, w, n_ids, dtype, d)
        v32 = ops.local_volumes(prevs, curs)
        v16 = ops.local_volumes(prevs, curs, dtype=F16)
        assert v16.dtype == F16 and v16.is_contiguous()
        assert v16.shape[0] == len(PAIRS) and v16.shape[1] * 2 == ops.local_volume_bytes(h, w, d, F16)
        # ... and into a caller's tensor: the same bytes
        mine = torch.empty_like(v16)
        assert ops.local_volumes(prevs, curs, out=mine, dtype=F16) is mine
        for i, (a, b) in enumerate(PAIRS):
            got = assert_tie(ops, v16[i], v32[i], frames[b], labs[a], n_ids, (d, C, a, b))
            assert torch.equal(ops.local_match_volume(mine[i], frames[b], labs[a], n_ids), got)
        with pytest.raises(ValueError):
            ops.local_match_volume(v16[0][:-8], frames[1], labs[0], n_ids)      # a wrong size for that dtype
        with pytest.raises(ValueError):
            ops.local_match_volume(v32[0].half(), frames[1], labs[0], n_ids)    # the fp32 image's size as halves
        with pytest.raises(ValueError):
            ops.local_volumes(prevs, curs, out=torch.empty_like(v32), dtype=F16)


@pytest.mark.parametrize("d", range(13))
def test_f16_route_against_the_cpu_oracle(ops, oracle, d):
    rng = np.random.default_rng(6200 + d)
    for (C, h, w, n_ids, dtype) in CASES:
        embs, labs, frames, prevs, curs = _case(ops, rng, C, h, w, n_ids, dtype, d)
        a, b = PAIRS[0]
        v16 = ops.local_volumes(prevs[:1], curs[:1], dtype=F16)
        got = ops.local_match_volume(v16[0], frames[b], labs[a], n_ids).cpu().numpy()
        e = embs.float().cpu().numpy()
        ref = oracle.local_match(np.transpose(e[a], (1, 2, 0)), np.transpose(e[b], (1, 2, 0)),
                                 labs[a].cpu().numpy().reshape(h, w, 1), n_ids, d, downsample=True).reshape(h, w, n_ids)
        assert_bound(got, ref, "oracle d=%d C=%d %dx%d" % (d, C, h, w))


@pytest.mark.parametrize("hw", [(120, 214), (180, 320)])
def test_f16_volume_is_half_the_bytes_plus_one_piece(ops, hw):
    h, w = hw
    for d in range(13):
        b32, b16 = ops.local_volume_bytes(h, w, d), ops.local_volume_bytes(h, w, d, F16)
        assert b16 <= b32 / 2 + 1024 and b16 % 16 == 0, (h, w, d, b32, b16)
        assert ops.local_volume_bytes(h, w, d, torch.float32) == b32
    with pytest.raises(ValueError):
        ops.local_volume_bytes(h, w, 12, torch.bfloat16)
    embs = torch.relu(torch.randn(2, 8, h, w, device="cuda")) * 0.1
    frames = ops.prepare_frames(embs, compute="f32", max_distance=12)
    v16 = ops.local_volumes([frames[0]], [frames[1]], dtype=F16)
    assert v16.dtype == F16 and v16.numel() * 2 == ops.local_volume_bytes(h, w, 12, F16)


def test_f16_volumes_more_pairs_than_one_launch(ops):
    """70 frame pairs = three launches of the batched phase-1 kernel; the labels change between uses of a volume"""
    torch.manual_seed(66)
    C, h, w, d, n_ids = 24, 22, 38, 12, 3
    embs = torch.relu(torch.randn(36, C, h, w, device="cuda")) * 0.2
    frames = ops.prepare_frames(embs, compute="f32", max_distance=d)
    pairs = [(t - 1, t) for t in range(1, 36)] + [(t + 1, t) for t in range(35)]
    prevs, curs = [frames[a] for a, _ in pairs], [frames[b] for _, b in pairs]
    v32 = ops.local_volumes(prevs, curs)
    v16 = ops.local_volumes(prevs, curs, dtype=F16)
    for i in (0, 31, 32, 63, 64, 69):
        a, b = pairs[i]
        alone = ops.local_volumes([frames[a]], [frames[b]], dtype=F16)
        for rnd in range(2):
            lab = torch.randint(0, n_ids, (h, w), dtype=torch.int32, device="cuda")
            got = assert_tie(ops, v16[i], v32[i], frames[b], lab, n_ids, (i, rnd))
            assert torch.equal(ops.local_match_volume(alone[0], frames[b], lab, n_ids), got)


def test_f16_volume_full_size_480p(ops):
    """120x214, C = 100, d = 12, 3 ids: 12.9 MB per pair"""
    torch.manual_seed(20200614 + 2)
    C, h, w, d, n_ids = 100, 120, 214, 12, 3
    embs = torch.relu(torch.randn(2, C, h, w, device="cuda")) * 0.1
    lab = torch.randint(0, n_ids, (h, w), dtype=torch.int32, device="cuda")
    frames = ops.prepare_frames(embs, compute="f32", max_distance=d)
    v32 = ops.local_volumes([frames[0]], [frames[1]])
    v16 = ops.local_volumes([frames[0]], [frames[1]], dtype=F16)
    assert v16.numel() * 2 == ops.local_volume_bytes(h, w, d, F16) <= (240 * 107520 + 1024) // 2 + 1024
    got = assert_tie(ops, v16[0], v32[0], frames[1], lab, n_ids, "480p")
    assert_bound(got.cpu().numpy(), ops.local_match_frames(frames[0], frames[1], lab, n_ids).cpu().numpy(), "480p d=12")


@pytest.mark.parametrize("d,n_ids", [(4, 6), (12, 6), (12, 11)])
def test_f16_volume_full_size_720p_grid(ops, d, n_ids):
    """180x320, C = 100 on 2-byte embeddings, labels outside [0, n_ids), a constant region (the single-label fast path)"""
    torch.manual_seed(20200614 + 5 + d)
    C, h, w = 100, 180, 320
    embs = (torch.relu(torch.randn(3, C, h, w, device="cuda")) * 0.1).to(torch.bfloat16)
    lab = torch.randint(-1, n_ids + 1, (h, w), dtype=torch.int32, device="cuda")
    lab[40:120, 60:200] = 1
    frames = ops.prepare_frames(embs, compute="bf16", max_distance=d)
    pairs = [(0, 1), (1, 2), (2, 1), (1, 0)]
    prevs, curs = [frames[a] for a, _ in pairs], [frames[b] for _, b in pairs]
    v32 = ops.local_volumes(prevs, curs)
    v16 = ops.local_volumes(prevs, curs, dtype=F16)
    for i, (a, b) in enumerate(pairs):
        got = assert_tie(ops, v16[i], v32[i], frames[b], lab, n_ids, (d, n_ids, a, b))
        assert_bound(got.cpu().numpy(), ops.local_match_frames(frames[a], frames[b], lab, n_ids).cpu().numpy(),
                     "720p d=%d ids=%d pair %d" % (d, n_ids, i))


def test_module_f16_volumes_global_maps_equal_local_maps_within_the_bound():
    """Two IntVOS instances with the same weights, local_volume_dtype "f32" and "f16", on one 8-frame clip: two interaction rounds
    of prop_seghead with the memory dicts, both models fed the SAME previous-frame labels (the logits behind the head are not
    asserted: nothing in the project derives a bound for them).  The global maps are bit-equal, every stored local map is within
    the bound, the cache charges real bytes, and assigning another storage type drops the cached volumes."""
    from examples import propagate_clip as pc
    from cvpr2020_manet_amd import ops
    dev = torch.device("cuda", 0)
    F_, H, W, nobj = 8, 240, 428, 2
    cfg32, m32 = pc.build_model(dev, None, None, None)
    cfg16, m16 = pc.build_model(dev, None, None, None, local_volume_dtype="F16")  # (case-insensitive)
    m16.load_state_dict(m32.state_dict())
    assert m32.local_volume_dtype == "f32" and m16.local_volume_dtype == "f16"
    assert not any("volume" in k for k in m16.state_dict())
    d = cfg32.MODEL_MAX_LOCAL_DISTANCE
    with torch.no_grad():
        emb = pc.synthetic_clip(m32, dev, F_, H, W, nobj, packed=False)
        eh, ew = emb.shape[-2:]
        scribble = pc.make_scribble(dev, eh, ew, nobj)
        bank_label = pc.rough_ROI(scribble)
        gt = torch.Tensor([nobj])
        g = torch.Generator(device=dev).manual_seed(5)
        start = F_ // 2
        results = []
        for model in (m32, m16):
            e = model.prepare_clip(emb)
            n = model.prepare_local_volumes(e)
            assert n == 2 * (F_ - 1)
            per = ops.local_volume_bytes(eh, ew, d, torch.float32 if model is m32 else F16)
            assert model.local_volume_bytes_cached() == n * per
            assert all(v[0].dtype == (torch.float32 if model is m32 else F16) for v in model._vol_cache.values())
            gmap, lmaps = {}, ({}, {})
            g.manual_seed(5)
            for rnd in (1, 2):
                ann = start if rnd == 1 else 1
                for order in (range(ann + 1, F_), range(ann - 1, -1, -1)):
                    prev_emb = e[ann:ann + 1]
                    for ii in order:
                        # mask-like labels (blocks of one id), the same for both models
                        small = torch.randint(0, nobj + 1, (1, 1, 6, 9), generator=g, device=dev).float()
                        prev_label = torch.nn.functional.interpolate(small, size=(H, W), mode="nearest").long()
                        cur = e[ii:ii + 1]
                        _, gmap, lmaps = model.prop_seghead(e[ann:ann + 1], prev_emb, cur, bank_label if rnd == 1 else scribble,
                                                            prev_label, normalize_nearest_neighbor_distances=True,
                                                            use_local_map=True, seq_names=[pc.SEQ], gt_ids=gt,
                                                            k_nearest_neighbors=cfg32.KNNS, global_map_tmp_dic=gmap,
                                                            local_map_dics=lmaps, interaction_num=rnd,
                                                            start_annotated_frame=ann, frame_num=[ii],
                                                            dynamic_seghead=model.dynamic_seghead)
                        prev_emb = cur
            results.append((gmap[pc.SEQ][:F_].clone(), lmaps[0][pc.SEQ][:F_, :2].clone()))
    (g32, l32), (g16, l16) = results
    assert torch.equal(g32, g16)
    assert float(l32[start + 1, 0].max()) > 0.0 and float(l32[start + 1, 0].min()) < 1.0  # (the maps were really written)
    assert_bound(l16.cpu().numpy(), l32.cpu().numpy(), "module local maps")
    assert not torch.equal(l16, l32)  # (the f16 model really ran on rounded volumes)
    n16 = m16.local_volume_bytes_cached()
    m16.local_volume_dtype = "f16"  # the same value: nothing dropped
    assert m16.local_volume_bytes_cached() == n16 > 0
    m16.local_volume_dtype = "f32"
    assert m16.local_volume_bytes_cached() == 0 and len(m16._vol_cache) == 0 and m16.local_volume_dtype == "f32"
    with pytest.raises(ValueError):
        m16.local_volume_dtype = "bf16"
