#!/usr/bin/env python3
"""Headline benchmark: propagated frames/s of MANet's matching path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: launched by torch.distributed.run, one rank per GPU, RCCL)

A "step" is one propagated frame: global nearest-neighbour match of the current frame against the
T-frame memory bank with the fused normalise + min-aggregation (IntVOS.py:609-622) and the local
(2d+1)^2 window match against the previous frame (IntVOS.py:629-631), embeddings already resident
in HBM (they come out of the encoder on the GPU; test.py:149-154).  Workload = BASELINE.json
configs[1]: 480p grid 120x214, C=100, 5-frame fully labelled bank (M = 128 400, the worst case
after rough_ROI), 1 object (+ background = 2 ids), fp32.

Timed region (exactly K steps + the clip's one-off work): the bank exchange (N > 1), ONE sort/pack
of the memory bank (it is the same for every frame of the propagation loop, test.py:237-259 -- what
the drop-in module does through its PreparedBank cache), then K frames, each = frame prepare
(query operand image + pooled plane from ONE read of the new embedding) + global match + fused
epilogue + local match (fused window kernel on the two prepared frames).  `--one-shot` re-sorts / re-packs the bank every frame through
the one-shot API instead (r1's definition; the reference recomputes everything per frame) -- the headline line carries that number
too (`value_one_shot`).  `--prepacked` takes the per-frame operands as given (prepared when the
embeddings were produced).

A plain run (the command above) sets up, warms up, times the K steps and prints the line: the headline with its `roofline` /
`local_stage` figures, which come from the library's HIP events inside the timed steps.  `--dump-outputs DIR` writes what the
last timed step returned (global map, merged global memory row, local map) as DIR/<name>.npy; the inputs are seeded, so
two builds run with the same arguments compare output for output.  Everything below that needs runs of its own is behind
`--full`.

With `--full` the ONE JSON line also carries, at N = 1, the other single-GPU BASELINE configs as `also` legs
(configs[2] = cfg3 and configs[4] = cfg5, bf16 arithmetic on 2-byte embeddings): ms per step, the
dominant kernel's HIP-event time and roofline fraction, and their error against the fp32 oracle;
`headline_exact_mode` (the headline workload through compute="bf16r": the fp32 bits at bf16 cost);
`robustness` (cfg2 shape on i.i.d. / video-like / smooth / flat embeddings x f32 / bf16 / bf16r: what
the distribution-dependent modes cost and err on each); `e2e` (the end-to-end propagated frame of
examples/propagate_clip.py -- matching + segmentation head + mask step -- eager, HIP-graph replay and
with the round's two directions on two HIP streams, for the fp32 and the split-bf16 head).

Multi-GPU: `python bench.py --gpus N` starts its own N ranks (one process per GPU, RCCL); frames of
the clip are sharded, K per rank (weak scaling; `--scaling strong`: a fixed 64-frame clip, BASELINE
configs[3]); the timed region contains the single RCCL all-gather that distributes the memory bank +
halo frame, and the line echoes what the collective saw (`collective`: backend, world, slab bytes,
all-gather ms).
"""
import argparse
import ctypes
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# dmabuf IPC only on these hosts: RCCL's device-buffer exchange between the ranks of a node fails without it
# (hipIpcGetMemHandle: invalid argument).  Set before the HIP runtime loads, also when a launcher started this rank.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# HIP streams share 4 hardware queues by default, dealt round-robin: two streams of a process may land on ONE queue and then
# run in order -- the two-stream round of the `e2e` block (examples/propagate_clip.py) gained its 21 % for the 1st and 3rd pair
# of streams a process created and nothing for the 2nd; with 8 queues every pair runs side by side.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

C = 100
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA peak (same guide)
HBM_PEAK_GBS = 8000.0

# BASELINE.json configs (index = --cfg): grid, bank frames, ids, local window (config.py:50 default = 12)
CONFIGS = {
    2: dict(H=120, W=214, T=5, n_ids=2, d=12),   # configs[1], the headline
    3: dict(H=120, W=214, T=5, n_ids=4, d=4),    # configs[2]
    5: dict(H=180, W=320, T=10, n_ids=6, d=4),   # configs[4]
}
MAIN_KERNEL = {"f32": "global_match_f32_pipe_kernel<50>", "bf16": "global_match_bf16_wide_kernel<7, 0>",
               "bf16x3": "global_match_bf16_kernel<7, true, 1, true>", "bf16r": "global_match_bf16_wide_kernel<7, 0> + refine"}


_CLIP_CACHE = {}


def _synthetic_scene(kind, n_frames, H, W, n_ids, scale, device, seed):
    """tools/synth_clip.make_clip, cached per (kind, shape, scale): the robustness legs run three arithmetic modes on one clip"""
    from tools import synth_clip
    key = (kind, n_frames, H, W, n_ids, float(scale), str(device), seed)
    if key not in _CLIP_CACHE:
        _CLIP_CACHE.clear()  # one clip at a time (130 MB at 480p)
        _CLIP_CACHE[key] = synth_clip.make_clip(kind, n_frames, C, H, W, n_ids, scale=scale, device=device, seed=seed)
    return _CLIP_CACHE[key]


class Workload:
    """One BASELINE config: synthetic clip of this rank, memory bank, previous-frame labels.

    The resident QUERY frames (cycled over by the timed steps) and the T BANK frames are different frames: no timed
    query is its own bank row (r3 cycled over 8 frames of which 5 were bank members -- exact zero-distance duplicates,
    the cheapest case for the bf16 filter of compute="bf16r").
    data = "iid" (SURVEY 8d's distribution, the headline) | "video" | "smooth" (tools/synth_clip.py: spatially smooth,
    temporally redundant, label-coherent clips -- bank frames interleaved in time with the query frames)."""

    def __init__(self, cfg, compute, emb, device, rank=0, world=1, n_local=8, keep_f32=False, data="iid", scale=0.1):
        c = CONFIGS[cfg]
        self.cfg, self.compute, self.emb, self.data, self.scale = cfg, compute, emb, data, scale
        self.H, self.W, self.T, self.n_ids, self.d = c["H"], c["W"], c["T"], c["n_ids"], c["d"]
        self.device, self.rank, self.world = device, rank, world
        self.emb_dtype = torch.bfloat16 if emb == "bf16" else torch.float32
        self.n_local = n_local
        self.F_total = world * n_local
        T, F_total = self.T, self.F_total
        # which clip frames are the annotated ones (who ships what in the N-rank exchange): spread over the clip
        bank_frames = sorted({int(round(i * (F_total - 1) / max(T - 1, 1))) for i in range(T)})
        f = 0
        while len(bank_frames) < T:  # tiny clips: the bank still holds T distinct (synthetic) frames
            if f not in bank_frames:
                bank_frames.append(f)
            f += 1
        self.bank_frames = sorted(bank_frames)[:T]
        # resident query frames, cycled: 8 x 10.3 MB (fp32, 480p), at least T + 2
        n_res = min(max(n_local, 1), max(8, T + 2))
        if data == "iid":
            gen = torch.Generator(device=device).manual_seed(20200614 + 2 + 1000 * rank)
            f32 = [torch.relu(torch.randn(C, self.H, self.W, generator=gen, device=device)) * scale for _ in range(n_res)]
            bank_f32 = {}
            for fb in self.bank_frames:  # the same on every rank
                g = torch.Generator(device=device).manual_seed(977 + fb)
                bank_f32[fb] = torch.relu(torch.randn(C, self.H, self.W, generator=g, device=device)) * scale
            lab_gen = torch.Generator(device=device).manual_seed(20200614 + 2)
            self.bank_labels = {fb: torch.randint(0, self.n_ids, (self.H, self.W), generator=lab_gen, device=device,
                                                  dtype=torch.int32) for fb in self.bank_frames}
            self.prev_labs = [self.blob_labels(s) for s in range(8)]
        else:
            if world != 1:
                raise SystemExit("bench.py --data %s: single-GPU legs only" % data)
            n_clip = T + n_res
            emb_c, lab_c = _synthetic_scene(data, n_clip, self.H, self.W, self.n_ids, scale, device, 20200614 + cfg)
            pos = sorted({int(round(i * (n_clip - 1) / max(T - 1, 1))) for i in range(T)})
            qpos = [i for i in range(n_clip) if i not in pos][:n_res]
            f32 = [emb_c[i] for i in qpos]
            bank_f32 = {fb: emb_c[pos[j]] for j, fb in enumerate(self.bank_frames)}
            self.bank_labels = {fb: lab_c[pos[j]].contiguous() for j, fb in enumerate(self.bank_frames)}
            # the previous frame's mask of query j = the blob labels of the clip frame before it
            self.prev_labs = [lab_c[max(qpos[j % len(qpos)] - 1, 0)].contiguous() for j in range(8)]
        # C-major embeddings as extract_feature produces them (post-ReLU), stored in the producer's type
        self.local_emb = torch.stack([f.to(self.emb_dtype) for f in f32]).contiguous()
        self.bank_emb = {fb: e.to(self.emb_dtype).contiguous() for fb, e in bank_f32.items()}
        self.f32_frames = f32 if keep_f32 else None  # the values before storage rounding (parity of the bf16 legs)
        self.bank_f32 = bank_f32 if keep_f32 else None
        self.gmap = torch.ones(104, self.H * self.W, self.n_ids, device=device)  # IntVOS.py:617

    def blob_labels(self, shift):
        """previous-frame labels: one rectangle per object, nearest-resized grid resolution"""
        H, W = self.H, self.W
        lab = torch.zeros(H, W, dtype=torch.int32, device=self.device)
        for o in range(1, self.n_ids):
            y0 = (15 * o + 3 * shift) % (H - 50)
            x0 = (40 * o + 5 * shift) % (W - 80)
            lab[y0:y0 + 45, x0:x0 + 70] = o
        return lab

    def frame_emb(self, i):  # embedding of local frame i (cycled over the resident ones)
        return self.local_emb[i % self.local_emb.shape[0]]

    def frame_f32(self, i):
        return self.f32_frames[i % len(self.f32_frames)]

    def probe_frame(self):
        """the resident frame the parity figures are taken on (no resident frame is one of the bank's: a frame of the bank
        would match itself at distance 0, which says nothing about the arithmetic)"""
        return 0

    def local_bytes(self):
        """algorithmic bytes of the local stage: both embeddings read once + labels + the [h,w,n_ids] result"""
        return 2.0 * (2 if self.emb == "bf16" else 4) * C * self.H * self.W + 4.0 * self.H * self.W * (1 + self.n_ids)

    def describe_short(self, args):
        return ("BASELINE configs[%d]: grid %dx%d, C=%d, %d-frame fully-labelled bank (M=%d), %d ids, %s arithmetic on %s-stored %s "
                "embeddings; step = frame prepare + global match + fused normalise/min-merge + local match d=%d; bank %s"
                % (self.cfg - 1, self.H, self.W, C, self.T, self.T * self.H * self.W, self.n_ids, self.compute, self.emb, self.data,
                   self.d, "re-packed per frame" if args.one_shot else "sorted/packed once per clip, timed"))

    def describe(self, args):
        M = self.T * self.H * self.W
        return ("BASELINE configs[%d]: %s embeddings, grid %dx%d, C=%d, %d-frame fully-labelled bank (M=%d), %d ids, %s arithmetic, "
                "%s-stored embeddings; step = frame prepare (query operand + pooled plane, one read of the embedding)%s + global match + fused "
                "normalise/min-merge + local match d=%d; bank %s"
                % (self.cfg - 1, {"iid": "i.i.d. relu(randn)*%g" % self.scale}.get(self.data, "%s-like (tools/synth_clip.py, scale %g)"
                                                                                       % (self.data, self.scale)),
                   self.H, self.W, C, self.T, M, self.n_ids, self.compute, self.emb,
                   " (done by the producer, untimed)" if args.prepacked else "", self.d,
                   "re-sorted/re-packed every frame (one-shot API)" if args.one_shot else
                   "sorted/packed once per clip inside the timed region"))


def run_leg(wl, K, Wm, args, lib, use_dist=False, one_shot=False, prepacked=False, overlap=False,
            ownership="block", spin_up_s=0.0):
    """Warm-up + the timed region of one workload on this rank.  Returns a dict of raw measurements."""
    from cvpr2020_manet_amd import _lib, clip_parallel, ops
    device = wl.device
    my_start, _ = clip_parallel.shard_frames(wl.F_total, wl.world, wl.rank)
    side = torch.cuda.Stream(device=device) if overlap else None
    timing = {"collective": None}

    def build_bank(timed):
        """every rank gets the full bank (+ halo): ONE all-gather over RCCL when world > 1"""
        if use_dist:
            n_local = wl.n_local
            if n_local <= wl.local_emb.shape[0]:
                owned = wl.local_emb[:n_local]
            else:
                # K > 8: frames are cycled; materialise only what the exchange reads
                class _View:
                    shape = (n_local, C, wl.H, wl.W)
                    device = wl.local_emb.device
                    dtype = wl.local_emb.dtype

                    def __getitem__(self, i):
                        return wl.frame_emb(i if i >= 0 else n_local + i)
                owned = _View()
            # the annotated frames' embeddings are their own synthetic frames (never one of the timed queries): the rank
            # that ships bank frame f -- the owner of its block, or rank j % world (round robin) -- hands it over here
            slots_, table_ = clip_parallel.bank_slots(wl.bank_frames, wl.F_total, wl.world, ownership)
            extra = {f: wl.bank_emb[f] for (r_, s_, f) in table_ if r_ == wl.rank}
            labels = {f: wl.bank_labels[f] for f in wl.bank_frames}
            bank_emb, bank_lab, halo = clip_parallel.exchange_bank_and_halo(
                owned, my_start, wl.bank_frames, labels, wl.F_total, ownership=ownership, extra_embeddings=extra,
                timing=True)
            if timed:
                timing["collective"] = dict(clip_parallel.LAST_EXCHANGE)
        else:
            bank_emb = torch.stack([wl.bank_emb[f] for f in wl.bank_frames])
            bank_lab = torch.stack([wl.bank_labels[f] for f in wl.bank_frames])
            halo = None
        # stacked T-frame bank as the API expects it: rows = pixels of all frames (IntVOS.py:203-204)
        bank_rows = bank_emb.permute(0, 2, 3, 1).reshape(-1, C)
        return bank_rows, bank_lab.reshape(-1), halo

    prepared_all = None
    if prepacked:  # the producer's job: every resident frame prepared when its embedding was produced
        prepared_all = ops.prepare_frames(wl.local_emb, compute=wl.compute, max_distance=wl.d)

    def prepare(bank_rows, bank_lab, old=None):
        """the clip's one-off: sort + pack the memory bank (None in --one-shot mode); a new clip takes over the previous
        bank's workspace, as the drop-in module does between interaction rounds"""
        return None if one_shot else ops.PreparedBank(bank_rows, bank_lab, wl.n_ids, compute=wl.compute, reuse=old)

    preset = wl.d >= 11  # the fused local kernel of wide windows wants `out` pre-set to 1.0: rides in the prepare launch
    state = {"prev": None}

    def first_prev(halo):
        """the frame before this rank's first one, prepared once per clip (its plane is all the local match needs)"""
        if one_shot:
            return
        if prepared_all is not None and halo is None:
            state["prev"] = prepared_all[0]
        else:
            state["prev"] = ops.prepare_frames(halo if halo is not None else wl.frame_emb(0), compute=wl.compute,
                                               max_distance=wl.d)

    def step(i, bank, bank_rows, bank_lab, halo):
        cur = wl.frame_emb(i)
        if bank is None:  # --one-shot: the stateless per-call API, everything recomputed per frame (r1's step)
            prev = wl.frame_emb(i - 1) if i > 0 else (halo if halo is not None else wl.frame_emb(0))
            g = ops.global_match(bank_rows, cur.permute(1, 2, 0), bank_lab, wl.n_ids, normalize=True,
                                 mem=wl.gmap[i % 104], compute=wl.compute)
            l = ops.local_match(prev.permute(1, 2, 0), cur.permute(1, 2, 0), wl.prev_labs[i % 8], wl.n_ids, wl.d)
            return g, l
        l_out = torch.empty((wl.H, wl.W, wl.n_ids), dtype=torch.float32, device=device)
        if prepared_all is not None:
            fcur, have_preset = prepared_all[i % len(prepared_all)], False
        else:  # ONE read of the new embedding: query operand image + pooled plane (+ the pre-set of l_out)
            fcur = ops.prepare_frames(cur, compute=wl.compute, max_distance=wl.d, preset=l_out if preset else None)
            have_preset = preset
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side):
                l = ops.local_match_frames(state["prev"], fcur, wl.prev_labs[i % 8], wl.n_ids, out=l_out,
                                           out_is_preset=have_preset)
        g = bank.match(fcur, normalize=True, mem=wl.gmap[i % 104])
        if side is None:
            l = ops.local_match_frames(state["prev"], fcur, wl.prev_labs[i % 8], wl.n_ids, out=l_out,
                                       out_is_preset=have_preset)
        else:  # the side stream's reads end before this stream recycles the previous frame's operands
            torch.cuda.current_stream(device).wait_stream(side)
        state["prev"] = fcur
        return g, l

    def barrier():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # warm-up (untimed)
    if side is not None:
        side.wait_stream(torch.cuda.current_stream(device))  # the synthetic frames were produced on the main stream
    bank_rows, bank_lab, halo = build_bank(False)
    bank = prepare(bank_rows, bank_lab)
    # ... twice: the timed region rebuilds the bank while the previous clip's tensors are still alive, so only the THIRD
    # build finds its blocks in the caching allocator's free lists (a first-time hipMalloc of 2 x 51 MB inside the timed
    # region cost one `also` leg 28 ms on a fresh box: 1.44 instead of 0.75 ms per step)
    first_prev(halo)
    bank_rows, bank_lab, halo = build_bank(False)
    bank = prepare(bank_rows, bank_lab, bank)
    first_prev(halo)
    for i in range(Wm):
        step(i, bank, bank_rows, bank_lab, halo)
    # (the short extra legs run right behind seconds of CPU-oracle work, during which the idle GPU drops its clocks: a
    # 30 ms timed region then ran at half speed on some boxes -- keep warming up until the GPU has been busy for spin_up_s)
    t_spin = time.perf_counter()
    while spin_up_s > 0.0 and time.perf_counter() - t_spin < spin_up_s:
        for i in range(Wm):
            step(i, bank, bank_rows, bank_lab, halo)
        torch.cuda.synchronize()
    barrier()

    # timed: the bank exchange + the bank's one-off sort/pack + exactly K frames
    _lib.check(lib.manet_profile_begin(K + 1), "manet_profile_begin")
    barrier()
    t0 = time.perf_counter()
    bank_rows, bank_lab, halo = build_bank(True)
    bank = prepare(bank_rows, bank_lab, bank)
    first_prev(halo)
    for i in range(K - 1):
        step(i, bank, bank_rows, bank_lab, halo)
    last = step(K - 1, bank, bank_rows, bank_lab, halo)  # (kept: what the caller of the last step receives)
    barrier()
    elapsed = time.perf_counter() - t0
    if bank is not None:
        bank.last_match_forced_exact_timed = getattr(bank, "last_match_forced_exact", False)
    ms, lms = (ctypes.c_float * K)(), (ctypes.c_float * K)()
    nrec, nloc = ctypes.c_int(0), ctypes.c_int(0)
    pms, npr = (ctypes.c_float * (K + 1))(), ctypes.c_int(0)
    _lib.check(lib.manet_profile_read(2, pms, K + 1, ctypes.byref(npr)), "manet_profile_read")
    prep_ms = float(np.mean([pms[i] for i in range(npr.value)])) if npr.value else None
    _lib.check(lib.manet_profile_end2(ms, K, ctypes.byref(nrec), lms, K, ctypes.byref(nloc)), "manet_profile_end2")
    kern_ms = float(np.mean([ms[i] for i in range(nrec.value)])) if nrec.value else float("nan")
    local_ms = float(np.mean([lms[i] for i in range(nloc.value)])) if nloc.value else float("nan")
    return {"elapsed": elapsed, "kern_ms": kern_ms, "local_ms": local_ms, "prep_ms": prep_ms, "bank_rows": bank_rows,
            "bank_lab": bank_lab, "collective": timing["collective"], "bank": bank,
            "outputs": {"global_map": last[0], "global_memory": wl.gmap[(K - 1) % 104], "local_map": last[1]}}


def roofline_blocks(wl, kern_ms, local_ms, overlap=False, prep_ms=None):
    N, M = wl.H * wl.W, wl.T * wl.H * wl.W
    flops = 2.0 * N * M * C  # algorithmic flops of one launch
    achieved = flops / (kern_ms * 1e-3) / 1e12
    peak = FP32_MFMA_PEAK_TFLOPS if wl.compute == "f32" else BF16_MFMA_PEAK_TFLOPS
    traffic, traffic_src = read_traffic(wl.cfg, wl.compute)
    roof = {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
            "traffic": traffic, "traffic_source": traffic_src, "kernel": MAIN_KERNEL[wl.compute], "kernel_ms": kern_ms,
            "algorithmic_flops_per_launch": flops}
    b = wl.local_bytes()
    # the HBM-bound stage of the path.  DEFINITION: `algorithmic_bytes` = both embeddings read once +
    # labels + the [h,w,n_ids] result (SURVEY 8d's formula); `stage_ms` = EVERY launch that moves those bytes = the fused
    # window/min kernel (`window_kernel_ms`, HIP events) + the frame prepare launch (`frame_prepare_ms`), which is the one
    # that reads the embedding and writes the pooled plane the window kernel consumes -- it also writes the global match's
    # query operand, so the stage is charged conservatively.  (r3 divided the same bytes by the window kernel alone.)
    local = None
    if not overlap:
        stage_ms = local_ms + (prep_ms or 0.0)
        local = {"bound": "hbm", "achieved": b / (stage_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "frac": b / (stage_ms * 1e-3) / (HBM_PEAK_GBS * 1e9), "stage_ms": stage_ms,
                 "window_kernel_ms": local_ms, "frame_prepare_ms": prep_ms, "algorithmic_bytes": b,
                 "max_distance": wl.d,
                 # the stage's arithmetic against the fp32 VECTOR peak (3 C P^2 h' w' + 2 h w P^2 n_ids flop): at the
                 # reference's default d = 12 the stage is VALU-bound (AI 58 flop/B), not HBM-bound -- both fractions are given
                 "valu": (lambda fl: {"algorithmic_flops": fl, "achieved": fl / (local_ms * 1e-3) / 1e12, "peak": FP32_MFMA_PEAK_TFLOPS,
                                      "unit": "TFLOP/s (window kernel alone)", "frac": fl / (local_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS})(
                     3.0 * C * (2 * wl.d + 1) ** 2 * (wl.H // 2) * (wl.W // 2) + 2.0 * wl.H * wl.W * (2 * wl.d + 1) ** 2 * wl.n_ids),
                 "launches": "frame prepare (one read of the embedding -> pooled plane + query operand image) + fused "
                             "window/min kernel" if prep_ms is not None else "pooling pass + fused kernel (one-shot API)"}
    return roof, local


def stored_volume_block(wl, lib, reps=4):
    """r6: the local stage split at its label boundary.  Phase 1 -- the window distances, which depend on the two
    embeddings only -- for a batch of frame pairs in one launch (`manet_local_volume_frames`), torch events around the call; phase 2
    -- label gather + masked minimum on a stored volume, what a propagated frame runs from a clip's second round on -- by the
    library's own HIP events on the launch's stream (channel 1 brackets `manet_local_match_volume`), over ROTATING pairs: every
    pair of a clip has its own volume, so phase 2 always streams a volume nobody touched since it was written.  Its roofline is
    HBM: algorithmic bytes = the volume as stored + labels + result."""
    from cvpr2020_manet_amd import _lib, ops
    n_fr = int(wl.local_emb.shape[0])
    if n_fr < 2 or wl.d < 0:
        return None
    frames = ops.prepare_frames(wl.local_emb, compute=wl.compute, max_distance=wl.d)
    pairs = [(i, i + 1) for i in range(n_fr - 1)] + [(i + 1, i) for i in range(n_fr - 1)]
    prevs, curs = [frames[a] for a, _ in pairs], [frames[b] for _, b in pairs]
    vols = ops.local_volumes(prevs, curs)
    torch.cuda.synchronize()
    t1 = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.local_volumes(prevs, curs, out=vols)
        e1.record()
        torch.cuda.synchronize()
        t1.append(e0.elapsed_time(e1) * 1e3 / len(pairs))
    out = torch.ones((wl.H, wl.W, wl.n_ids), dtype=torch.float32, device=wl.device)
    n = reps * len(pairs)
    for i in range(len(pairs)):  # warm-up
        ops.local_match_volume(vols[i], curs[i], wl.prev_labs[i % len(wl.prev_labs)], wl.n_ids, out=out)
    torch.cuda.synchronize()
    _lib.check(lib.manet_profile_begin(n + 1), "manet_profile_begin")
    for r in range(reps):
        for i in range(len(pairs)):
            # (`out` pre-set to 1.0 outside the bracket, as inside prop_seghead: there the pre-set rides in frame_begin's launch)
            out.fill_(1.0)
            ops.local_match_volume(vols[i], curs[i], wl.prev_labs[(i + r) % len(wl.prev_labs)], wl.n_ids, out=out, out_is_preset=True)
    torch.cuda.synchronize()
    ms, lms = (ctypes.c_float * n)(), (ctypes.c_float * n)()
    nrec, nloc = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(lib.manet_profile_end2(ms, n, ctypes.byref(nrec), lms, n, ctypes.byref(nloc)), "manet_profile_end2")
    p2_us = float(np.mean([lms[i] for i in range(nloc.value)])) * 1e3 if nloc.value else float("nan")
    vol_bytes = float(vols.shape[1] * 4)
    b2 = vol_bytes + 4.0 * wl.H * wl.W * (1 + wl.n_ids)
    return {"pairs": len(pairs), "volume_bytes_per_pair": vol_bytes,
            "phase1_us_per_pair_batched": float(min(t1)), "phase2_us_per_frame": p2_us,
            "phase2": {"bound": "hbm", "algorithmic_bytes": b2, "achieved": b2 / (p2_us * 1e-6) / 1e9, "peak": HBM_PEAK_GBS,
                       "unit": "GB/s", "frac": b2 / (p2_us * 1e-6) / (HBM_PEAK_GBS * 1e9)},
            "note": "phase 2 (+ the 1.0 pre-set launch for d >= 11, which rides in frame_begin inside prop_seghead) is what the "
                    "sequential chain runs per frame once a clip's volumes are stored (IntVOS.prepare_local_volumes)"}


def _sha(path):
    try:
        return hashlib.sha256(open(path, "rb").read()).hexdigest()[:12]
    except OSError:
        return None


def read_traffic(cfg, compute):
    """HBM/fabric bytes of the dominant kernel: PMC counters cannot be read from inside the run, so the figure comes
    from the tracked rocprofv3 --pmc capture of THIS command line (profiles/traffic_cfg*.json records where and when
    it was measured, and the hash of the kernel source it was measured on: `stale` says whether that still is the
    source of the library that ran here)."""
    tp = os.path.join(ROOT, "profiles", "traffic_cfg%d_%s.json" % (cfg, compute))
    if not os.path.exists(tp):
        return None, None
    try:
        tj = json.load(open(tp))
    except Exception:
        return None, None
    src = {k: tj.get(k) for k in ("source", "captured_at", "kernel", "kernel_source_sha")}
    now = _sha(os.path.join(ROOT, "cvpr2020_manet_amd", "csrc", "global_match.hip"))
    src["stale"] = None if tj.get("kernel_source_sha") is None else (tj.get("kernel_source_sha") != now)
    return tj.get("hbm_bytes_per_launch"), src


def oracle_sample(wl, bank_rows_f32, bank_lab, cur_f32, budget_s, quant_bf16=False, nq_cap=None):
    """The CPU oracle's global match on a time-bounded sample of query pixels (cost is linear in them) against the
    FULL bank.  Returns (raw distances [nq, n_ids], nq, seconds per repetition, repetitions)."""
    from oracle import oracle as orc
    cores = os.cpu_count() or 1
    N = wl.H * wl.W
    qry = cur_f32.permute(1, 2, 0).reshape(-1, C).cpu().numpy()
    ref3 = bank_rows_f32.cpu().numpy().reshape(-1, 1, C)
    lab = bank_lab.cpu().numpy().reshape(-1, 1, 1)
    last = {}

    def run(nq):
        q = np.ascontiguousarray(qry[:nq]).reshape(nq, 1, C)
        t0 = time.perf_counter()
        last["raw"] = orc.global_match(ref3, q, lab, 1, n_ids=wl.n_ids, test_mode=True, quant_bf16=quant_bf16)
        return time.perf_counter() - t0

    probe_n = min(N, 8 * cores)
    per_q = run(probe_n) / probe_n
    nq = int(min(N, max(probe_n, budget_s / per_q)))
    nq -= nq % (8 * cores)
    nq = min(N, max(nq, probe_n))
    if nq_cap:
        nq = min(nq, nq_cap)
    reps = int(max(1, min(30, round(budget_s / max(per_q * nq, 1e-3)))))
    t = sum(run(nq) for _ in range(reps)) / reps
    return last["raw"].reshape(nq, wl.n_ids), nq, t, reps


def cpu_baseline(wl, bank_rows, bank_lab, gpu_global=None, gpu_local=None):
    """The CPU oracle (a C port of the reference path, kind="port": OpenMP over query blocks, the distance loop
    vectorised across bank rows with AVX-512/AVX2 FMA -- same fmaf chains, bit-identical to the scalar form) on
    the host cores, on a bounded sample of the same frame: a subset of query pixels against the FULL bank for the
    global match (cost is linear in query pixels), the whole frame for the local match.  ~10-30 s.
    The oracle's outputs double as the parity check of the metric ("mask max-abs-err vs ref"): when the
    GPU results of the same frame are passed in, their max abs deviation is returned as well."""
    from oracle import oracle as orc
    cores = os.cpu_count() or 1
    N = wl.H * wl.W
    p = wl.probe_frame()
    cur, prev = wl.frame_emb(p).float(), wl.frame_emb(p + 1).float()  # (bf16-stored embeddings widen exactly)
    raw, nq, t_glob, reps = oracle_sample(wl, bank_rows.float(), bank_lab, cur, 10.0)
    qry = cur.permute(1, 2, 0).cpu().numpy()
    t0 = time.perf_counter()
    lreps = 0
    while True:
        loc = orc.local_match(prev.permute(1, 2, 0).cpu().numpy(), qry, wl.prev_labs[0].cpu().numpy(), wl.n_ids, wl.d)
        lreps += 1
        if time.perf_counter() - t0 > 3.0 or lreps >= 10:
            break
    t_loc = (time.perf_counter() - t0) / lreps
    frame_s = t_glob / nq * N + t_loc
    # the same global match in the reference's own shape on the host's BLAS (oracle.global_match_blas: torch's CPU GEMM per query
    # chunk, d materialised, masked min per object) -- VERDICT r3 weak #6: whichever form is faster is the baseline
    blas = None
    try:
        import torch as _t
        _t.set_num_threads(cores)
        nb = int(min(N, 2048))
        ref_np, lab_np = bank_rows.float().cpu().numpy(), bank_lab.cpu().numpy()
        q_np = np.ascontiguousarray(qry.reshape(-1, C)[:nb])
        orc.global_match_blas(ref_np, q_np[:256], lab_np, wl.n_ids)  # warm-up
        t0 = time.perf_counter()
        got_b = orc.global_match_blas(ref_np, q_np, lab_np, wl.n_ids)
        t_b = time.perf_counter() - t0
        blas = {"frames_per_s": 1.0 / (t_b / nb * N + t_loc), "query_pixels": nb, "seconds": t_b,
                "max_abs_dev_from_the_fused_port": float(np.abs(got_b - raw[:nb]).max())}
    except Exception as e:  # (a baseline, never a reason for the line to fail)
        blas = {"error": str(e)[:200]}
    fused_fps = 1.0 / frame_s
    best = max(fused_fps, blas.get("frames_per_s", 0.0))
    res = {"value": best, "unit": "frames/s", "cores": cores, "kind": "port",
           "sample_short": "global: %d of %d query px x full %d-row bank, %dx%.2fs; local d=%d whole frame %dx%.2fs; C port, %d thr"
                           % (nq, N, bank_rows.shape[0], reps, t_glob, wl.d, lreps, t_loc, cores),
           "forms": {"fused_c_port_frames_per_s": fused_fps, "blas_port": blas,
                     "reported": "blas_port" if best > fused_fps else "fused_c_port"},
           "sample": "global match: %d of %d query pixels x full %d-row bank, %d repetition(s), %.2f s each (scaled "
                     "linearly to the frame); local match d=%d: whole frame, %d repetition(s), %.2f s each; "
                     "oracle/manet_oracle.c, OpenMP on %d threads, distance loop vectorised across bank rows "
                     "(AVX-512/AVX2 FMA, bit-identical to the scalar chains)"
                     % (nq, N, bank_rows.shape[0], reps, t_glob, wl.d, lreps, t_loc, cores)}
    parity = None
    if gpu_global is not None:
        want, _ = orc.normalize_merge(raw, None, normalize=True)
        got = gpu_global.cpu().numpy()[:nq]
        parity = {"global_map_max_abs_err": float(np.abs(got - want).max()), "global_pixels_checked": int(nq),
                  "local_map_max_abs_err": float(np.abs(gpu_local.cpu().numpy() - loc.reshape(wl.H, wl.W, wl.n_ids)).max()),
                  "reference": "CPU oracle (pinned to reference vectors), same frame, normalised maps"}
    return res, parity


def err_stats(got_norm, want_norm):
    """max / mean abs error of the normalised maps and the fraction of pixels whose arg-min object id differs"""
    e = np.abs(got_norm - want_norm)
    flips = float(np.mean(np.argmin(got_norm, axis=1) != np.argmin(want_norm, axis=1)))
    return float(e.max()), float(e.mean()), flips


def bf16_parity(wl, bank_rows, bank_lab, budget_s=4.0):
    """north_star's bar for the bf16 configs is 'within 1e-3 of the reference PyTorch path on the same inputs'.  Two
    readings of 'same inputs', both measured here against the fp32 oracle on a sample of one non-bank frame's pixels x the FULL bank:
      stored    the inputs are the 2-byte embeddings the producer stored (what this leg's kernels read): the oracle runs
                the reference's fp32 formula on exactly those values (widened) -- bf16 products of bf16 values are exact,
                only the accumulation order differs
      unrounded the inputs are the fp32 embeddings BEFORE storage rounding; the GPU paths round them to bf16 themselves
                (compute='bf16'), split them hi+lo (compute='bf16x3'), or filter in bf16 and re-rank in fp32
                (compute='bf16r', bit-exact by construction) -- this is the figure a caller with fp32 embeddings sees
    Figures are on the normalised maps (sigmoid(d)-0.5)*2 in [0,1] (SURVEY 7 'hard parts'); flips = fraction of sampled
    pixels whose arg-min object id differs from the oracle's."""
    from cvpr2020_manet_amd import ops
    from oracle import oracle as orc
    out = {"reference": "CPU oracle, fp32 formula (pinned to reference vectors); sample of a non-bank frame x full bank",
           "tolerance": 1e-3}
    p = wl.probe_frame()
    cur_st = wl.frame_emb(p)
    # -- stored inputs
    raw, nq, _, _ = oracle_sample(wl, bank_rows.float(), bank_lab, cur_st.float(), budget_s)
    want, _ = orc.normalize_merge(raw, None, normalize=True)
    g = ops.global_match(bank_rows, cur_st.permute(1, 2, 0), bank_lab, wl.n_ids, normalize=True, compute=wl.compute)
    mx, mean, flips = err_stats(g.cpu().numpy()[:nq], want)
    out["pixels_checked"] = int(nq)
    out["stored_inputs"] = {"compute": wl.compute, "err_vs_fp32_oracle_normalised_max": mx,
                            "err_vs_fp32_oracle_normalised_mean": mean, "argmin_id_flip_fraction": flips}
    # -- unrounded fp32 inputs
    if wl.f32_frames is not None:
        bank_f32 = torch.stack([wl.bank_f32[f] for f in wl.bank_frames]).permute(0, 2, 3, 1).reshape(-1, C)
        cur_f32 = wl.frame_f32(p)
        raw, nq2, _, _ = oracle_sample(wl, bank_f32, bank_lab, cur_f32, budget_s, nq_cap=nq)
        want, _ = orc.normalize_merge(raw, None, normalize=True)
        un = {}
        modes = ["bf16", "bf16x3"] + (["bf16r"] if "bf16r" in ops.COMPUTE else [])
        for mode in modes:
            g = ops.global_match(bank_f32, cur_f32.permute(1, 2, 0), bank_lab, wl.n_ids, normalize=True, compute=mode)
            mx, mean, flips = err_stats(g.cpu().numpy()[:nq2], want)
            un[mode] = {"err_vs_fp32_oracle_normalised_max": mx, "err_vs_fp32_oracle_normalised_mean": mean,
                        "argmin_id_flip_fraction": flips}
        out["unrounded_fp32_inputs"] = un
        out["meets_1e-3"] = {m: bool(v["err_vs_fp32_oracle_normalised_max"] <= 1e-3) for m, v in un.items()}
        # the same frames with the embeddings three times as large (scale 0.3 instead of SURVEY 8d's 0.1), plain
        # bf16 against the fp32 KERNEL (bit-exact against the oracle) on the whole frame: where plain bf16 leaves the 1e-3 bar
        b3, c3 = bank_f32 * 3.0, (cur_f32 * 3.0).permute(1, 2, 0)
        g32 = ops.global_match(b3, c3, bank_lab, wl.n_ids, normalize=True, compute="f32")
        gb = ops.global_match(b3, c3, bank_lab, wl.n_ids, normalize=True, compute="bf16")
        out["plain_bf16_err_scale_0.3"] = float((g32 - gb).abs().max().item())
        del b3, c3, g32, gb
    return out


def also_leg(cfg, compute, device, lib, args):
    """A GPU-only leg of another single-GPU BASELINE config (a few steps) + its parity figures."""
    wl = Workload(cfg, compute, "bf16" if compute != "f32" else "f32", device, n_local=CONFIGS[cfg]["T"] + 2, keep_f32=True)
    K, Wm = args.also_steps, 6
    r = run_leg(wl, K, Wm, args, lib, spin_up_s=0.2)
    roof, local = roofline_blocks(wl, r["kern_ms"], r["local_ms"], prep_ms=r["prep_ms"])
    leg = {"workload": wl.describe(args), "cfg": cfg, "dtype": compute, "steps": K, "warmup": Wm,
           "value": K / r["elapsed"], "unit": "frames/s", "ms_per_step": r["elapsed"] / K * 1e3,
           "kernel_ms": r["kern_ms"], "roofline": roof, "local_stage": local}
    if not args.no_cpu_baseline:
        from cvpr2020_manet_amd import ops
        from oracle import oracle as orc
        leg["parity"] = bf16_parity(wl, r["bank_rows"], r["bank_lab"])
        p = wl.probe_frame()
        l_chk = ops.local_match(wl.frame_emb(p + 1).permute(1, 2, 0), wl.frame_emb(p).permute(1, 2, 0), wl.prev_labs[0],
                                wl.n_ids, wl.d)
        loc = orc.local_match(wl.frame_emb(p + 1).float().permute(1, 2, 0).cpu().numpy(),
                              wl.frame_emb(p).float().permute(1, 2, 0).cpu().numpy(), wl.prev_labs[0].cpu().numpy(),
                              wl.n_ids, wl.d)
        leg["parity"]["local_map_max_abs_err"] = float(np.abs(l_chk.cpu().numpy() - loc.reshape(wl.H, wl.W, wl.n_ids)).max())
    # the mode that meets north_star's 1e-3 WHATEVER the embeddings' scale, on fp32-stored embeddings (plain bf16 meets it on
    # this benchmark's distribution only, tests/test_bf16_error_bound.py): bf16 filter + exact fp32 re-rank = the fp32
    # kernel's result bit for bit
    del wl, r
    torch.cuda.empty_cache()
    leg["exact_mode"] = exact_leg(cfg, device, lib, args)
    # the leg LEADS with the tolerance-safe figure.  north_star's bar is 1e-3; plain bf16 meets it at SURVEY 8d's
    # embedding scale 0.1 and not at 0.3 (`err_0.3`): `value` is the bf16r rate (the fp32 result bit for bit), the plain-bf16 rate and
    # its two errors stand beside it.  (`ms_per_step`, `kernel_ms`, `roofline`, `local_stage` describe the plain-bf16 run: the bf16
    # MFMA kernel is what those configs' rooflines are about.)
    un = ((leg.get("parity") or {}).get("unrounded_fp32_inputs") or {}).get(compute) or {}
    leg["value_plain_bf16"] = leg["value"]
    leg["value"] = leg["exact_mode"]["value"]
    leg["value_mode"] = "bf16r on f32-stored embeddings: bf16 filter + exact fp32 re-rank = the fp32 kernel's result bit for bit"
    leg["err_0.1"] = un.get("err_vs_fp32_oracle_normalised_max")
    leg["err_0.3"] = (leg.get("parity") or {}).get("plain_bf16_err_scale_0.3")
    return leg


def exact_leg(cfg, device, lib, args):
    """The same step with compute="bf16r" on fp32-stored embeddings (bf16 filter pass + exact fp32 re-rank of the rows inside
    the rounding bound), and a live check that it IS the fp32 kernel's result: both modes on the probe frame, compared bit for
    bit."""
    from cvpr2020_manet_amd import ops
    K, Wm = args.also_steps, 6  # (warm-up long enough for the caching allocator to have seen every per-step block)
    wx = Workload(cfg, "bf16r", "f32", device, n_local=CONFIGS[cfg]["T"] + 2)
    rx = run_leg(wx, K, Wm, args, lib, spin_up_s=0.2)
    st = rx["bank"].refine_stats_full()
    cands, over = st["candidate_rows"], st["list_overflowed"]
    q = wx.frame_emb(wx.probe_frame()).permute(1, 2, 0)
    same = bool(torch.equal(ops.global_match(rx["bank_rows"], q, rx["bank_lab"], wx.n_ids, compute="bf16r"),
                            ops.global_match(rx["bank_rows"], q, rx["bank_lab"], wx.n_ids, compute="f32")))
    return {"dtype": "bf16r", "embeddings": "f32-stored", "value": K / rx["elapsed"], "unit": "frames/s", "steps": K,
            "ms_per_step": rx["elapsed"] / K * 1e3, "filter_kernel_ms": rx["kern_ms"],
            "result": "the fp32 kernel's distances, bit for bit (tests/test_bf16_refine.py)",
            "bit_equal_to_f32_on_probe_frame": same,
            "candidate_rows_per_pair": cands / float(wx.H * wx.W * wx.n_ids), "candidate_list_overflowed": int(over),
            "rescued_tile_fraction": st["rescued_tile_fraction"],
            "data": "i.i.d. embeddings, uniform labels: this mode's BEST case -- `robustness` brackets it"}


def robustness_block(device, lib, args):
    """every distribution-dependent claim bracketed in the driver-run line.  cfg2 shape (480p, T=5,
    2 ids, d=12), fp32-stored embeddings, data in {iid, video, smooth, flat} (tools/synth_clip.py) x scale in {0.1, 0.3} x
    compute in {f32, bf16, bf16r}: ms per step of the same step the headline times (K steps over non-bank frames),
    error of the normalised global map of one non-bank frame against the fp32 result (the f32 kernel, itself checked
    against the CPU oracle on a pixel sample right here) and, for bf16r, the candidate rows per (query, object) pair and
    the share of 256-query tiles that went through the rescue pass (the exact fp32 kernel)."""
    from cvpr2020_manet_amd import ops
    from oracle import oracle as orc
    K, Wm = args.robust_steps, 3
    legs = []
    for data in ("iid", "video", "smooth", "flat"):
        for scale in ((0.1, 0.3) if data != "flat" else (0.1,)):
            ref_norm, oracle_ok = None, None
            for compute in ("f32", "bf16", "bf16r"):
                wl = Workload(2, compute, "f32", device, n_local=CONFIGS[2]["T"] + 2, data=data, scale=scale)
                r = run_leg(wl, K, Wm, args, lib, spin_up_s=0.05)
                leg = {"data": data, "scale": scale, "compute": compute, "ms_per_step": r["elapsed"] / K * 1e3,
                       "frames_per_s": K / r["elapsed"], "main_kernel_ms": r["kern_ms"]}
                q = wl.frame_emb(wl.probe_frame()).permute(1, 2, 0)
                # (the diagnostic match runs the filter whatever the adaptive policy decided for the timed frames)
                g = r["bank"].match(ops.prepare_frames(wl.frame_emb(wl.probe_frame()), compute=compute), normalize=True,
                                    **({"adaptive": False} if compute == "bf16r" else {}))
                if compute == "bf16r":
                    leg["timed_frames_skipped_the_filter"] = bool(getattr(r["bank"], "last_match_forced_exact_timed", False))
                    st = r["bank"].refine_stats_full()
                    leg["candidate_rows_per_pair"] = st["candidate_rows_per_pair"]
                    leg["rescued_tile_fraction"] = st["rescued_tile_fraction"]
                got = g.cpu().numpy()
                if compute == "f32":
                    ref_norm = got
                    if not args.no_cpu_baseline:  # the fp32 kernel against the CPU oracle on a pixel sample of this very frame:
                        # RAW distances, bit for bit (the normalisation's expf differs from libm's in the last place)
                        raw, nq, _, _ = oracle_sample(wl, r["bank_rows"], r["bank_lab"], wl.frame_emb(wl.probe_frame()), 0.3,
                                                      nq_cap=512)
                        g_raw = r["bank"].match(ops.prepare_frames(wl.frame_emb(wl.probe_frame()), compute=compute))
                        oracle_ok = bool(np.array_equal(g_raw.cpu().numpy()[:nq], raw))
                    leg["f32_kernel_equals_cpu_oracle_on_sample"] = oracle_ok
                    leg["err_vs_fp32_oracle_normalised_max"], leg["argmin_flip_fraction"] = 0.0, 0.0
                else:
                    mx, _, flips = err_stats(got, ref_norm)
                    leg["err_vs_fp32_oracle_normalised_max"], leg["argmin_flip_fraction"] = mx, flips
                    if compute == "bf16r":
                        leg["bit_equal_to_f32"] = bool(np.array_equal(got, ref_norm))
                legs.append(leg)
                del wl, r, g, q
                torch.cuda.empty_cache()
    _CLIP_CACHE.clear()
    torch.cuda.empty_cache()

    def pick(data, compute, key, scale=0.1):
        return next(l[key] for l in legs if l["data"] == data and l["compute"] == compute and l["scale"] == scale)
    summary = {"bf16r_frames_per_s_iid_video_smooth_flat": [pick(d, "bf16r", "frames_per_s") for d in ("iid", "video", "smooth", "flat")],
               "f32_frames_per_s": pick("iid", "f32", "frames_per_s"),
               "bf16_max_err_scale_0.1": max(pick(d, "bf16", "err_vs_fp32_oracle_normalised_max") for d in ("iid", "video", "smooth", "flat")),
               "bf16_max_err_scale_0.3": max(pick(d, "bf16", "err_vs_fp32_oracle_normalised_max", 0.3) for d in ("iid", "video", "smooth"))}
    return {"shape": "cfg2 (480p grid 120x214, T=5, 2 ids, d=12), fp32-stored embeddings, %d steps per leg over non-bank frames" % K,
            "data_kinds": "iid = relu(randn) + uniform labels (best case); video = smooth field + per-pixel detail + object "
                          "clusters, temporally adjacent bank frames, blob labels (typical); smooth = 32-pixel bilinear "
                          "fields, near-identical frames (hard: whole blocks of the bf16 filter qualify -- dense entries of the "
                          "re-rank); flat = every pixel of an object carries the same vector (the floor: every tile goes to the "
                          "exact fp32 kernel, the adaptive policy then skips the filter) -- tools/synth_clip.py",
            "reference": "normalised global map of a non-bank frame from the fp32 kernel (checked against the CPU oracle on "
                         "a 512-pixel sample per data kind, raw distances bit for bit: f32_kernel_equals_cpu_oracle_on_sample)",
            "summary": summary, "legs": legs}


def e2e_block(device, args):
    """The end-to-end propagated frame (matching + DynamicSegHead + mask step, test.py:237-259) in the driver-run line:
    examples/propagate_clip.py's loop at 480p, 2 objects; the stand-in encoder runs BEFORE the timed region (test.py:143-154
    extracts a clip's embeddings up front).  VERDICT r4 next #2: the headline `value` is on the bank the reference driver's first
    round really produces -- the scribbles after rough_ROI (test.py:229-230: every pixel outside the strokes' box is background,
    ~17 000 rows at 480p) -- with the strokes-only bank of r1-r4 (`value_scribble_bank`, ~1 000 rows) and the metric's 5-frame
    memory (`value_bank_frames_5`: five annotated frames stacked, each through rough_ROI) beside it.  Head = the exact-fp32 1x1
    kernels (the module's default); the split-bf16 forms beside it with their max |logit| deviation from the fp32 head."""
    from examples import propagate_clip as pc
    base = ["--frames", str(args.e2e_frames), "--fused-mask-step", "--rounds", "3"]  # (3 timed rounds: an eager round is 40 ms)
    out = {"workload": "examples/propagate_clip.py: %d-frame synthetic 480x854 clip (grid 120x214), 2 objects, bank = 1 annotated frame "
                       "through rough_ROI (test.py:229-230), fp32 match + exact fp32 head, d=12, int_seghead + prop_seghead + "
                       "upsample/argmax per frame; encoder untimed" % args.e2e_frames,
           "unit": "frames/s", "modes": {}, "banks": {}}
    logits = {}
    eargs = pc.parse_args(base + ["--two-streams", "--bank", "roi"])
    for pw in ("f32", "split3", "split"):
        res, clip, final = pc.run_single(eargs, device, pointwise=pw, want_graph=True, want_stages=(pw == "f32"))
        with torch.no_grad():
            lg = {}
            clip.one_round(keep_logits=lg)
        logits[pw] = lg
        out["modes"][pw] = res
        del clip
        torch.cuda.empty_cache()
    f32 = out["modes"]["f32"]
    out["bank"], out["bank_rows"] = f32["bank"], f32["bank_rows"]
    out["value"] = f32["eager_frames_per_s"]
    # r6: `value` is a round with the clip's window-distance volumes stored (model.prepare_local_volumes, once per clip: every round
    # but a sequence's first finds them, like the head's memoised layer-1 term); `value_first_round` charges that one-off call to
    # one round; `value_fused_local` is the same round with the fused local kernel of r1-r5 (no volumes)
    out["value_first_round"] = f32["first_round_frames_per_s"]
    out["local_volumes"] = f32["local_volumes"]
    out["value_graph"] = f32["graph_frames_per_s"]
    # the round's two independent halves (forwards / backwards from the annotated frame) on two HIP streams of the one GPU
    out["value_two_streams"] = f32["two_streams_frames_per_s"]
    out["two_streams_masks_equal_eager"] = bool(all(out["modes"][m]["two_streams_masks_equal_eager"] for m in out["modes"]))
    out["masks_equal_eager_graph_two_streams"] = bool(all(out["modes"][m]["two_streams_masks_equal_eager"]
                                                          and out["modes"][m]["graph_masks_equal_eager"] for m in out["modes"]))
    res, clip, final = pc.run_single(pc.parse_args(base + ["--bank", "roi", "--no-local-volumes"]), device, pointwise="f32")
    out["value_fused_local"] = res["eager_frames_per_s"]
    out["fused_local_masks_equal"] = bool(res["mask_digest"] == f32["mask_digest"])
    del clip
    torch.cuda.empty_cache()
    # the other banks, fp32 head, eager loop: the strokes alone (r1-r4's workload), the 5-frame memory, every pixel labelled
    for name, extra in (("scribble", ["--bank", "scribble"]), ("roi_T5", ["--bank", "roi", "--bank-frames", "5"]),
                        ("full_T5", ["--bank", "full", "--bank-frames", "5"])):
        res, clip, final = pc.run_single(pc.parse_args(base + extra), device, pointwise="f32")
        out["banks"][name] = {k: res[k] for k in ("bank", "bank_frames", "bank_rows", "eager_ms_per_round", "eager_frames_per_s",
                                                  "mask_digest")}
        del clip
        torch.cuda.empty_cache()
    # the same roi round with the global match through compute="bf16r" (bf16 filter + exact fp32 re-rank: the fp32 kernel's
    # distances bit for bit, so the masks must be the f32 round's) -- at this bank size the fp32 match is half the frame
    res, clip, final = pc.run_single(pc.parse_args(base + ["--bank", "roi", "--compute", "bf16r"]), device, pointwise="f32")
    out["banks"]["roi_bf16r"] = {k: res[k] for k in ("bank", "bank_frames", "bank_rows", "compute", "eager_ms_per_round",
                                                     "eager_frames_per_s", "mask_digest")}
    out["value_bf16r_match"] = res["eager_frames_per_s"]
    out["bf16r_match_masks_equal_f32"] = bool(res["mask_digest"] == f32["mask_digest"])
    del clip
    torch.cuda.empty_cache()
    # a whole interactive session as test.py runs it (8 rounds on one sequence: round 1 on the roi bank, rounds 2-8 on new strokes
    # alone -- rough_ROI applies `if first_scribble` only, test.py:229 -- with the global / local memories carried over)
    res, clip, final = pc.run_single(pc.parse_args(base + ["--bank", "roi", "--session", "8"]), device, pointwise="f32")
    out["session"] = {k: res[k] for k in ("session_rounds", "session_ms_per_round", "session_frames_per_s", "session_mask_digest",
                                          "session_repeatable")}
    out["value_session_8_rounds"] = res["session_frames_per_s"]
    del clip
    torch.cuda.empty_cache()
    out["value_scribble_bank"] = out["banks"]["scribble"]["eager_frames_per_s"]
    out["value_bank_frames_5"] = out["banks"]["roi_T5"]["eager_frames_per_s"]
    out["value_full_bank_frames_5"] = out["banks"]["full_T5"]["eager_frames_per_s"]
    # split vs f32 head on the first propagated frame (same inputs: later frames see different previous masks)
    first = min(k for k in logits["f32"] if k > args.e2e_frames // 2)
    out["split_vs_f32_head_max_abs_logit_diff"] = float((logits["split"][first] - logits["f32"][first]).abs().max().item())
    out["split3_vs_f32_head_max_abs_logit_diff"] = float((logits["split3"][first] - logits["f32"][first]).abs().max().item())
    out["split_vs_f32_head_logit_scale"] = float(logits["f32"][first].abs().max().item())
    # (no mask-agreement figure: random-init heads put the ids' logits within 1e-4 of each other on a quarter of the pixels, so
    # argmax flips there say nothing about a trained head; tests/test_seg_head.py bounds the kernel against an fp64 convolution)
    out["per_frame_stages_note"] = ("modes.f32.per_frame_stages_us: HIP-event brackets around each ops.* call of one eager round; "
                                    "they include the launch gaps of a host-bound eager loop (rocprofv3 kernel times: "
                                    "profiles/r05_e2e_per_frame_kernels.csv)")
    return out


def e2e_parallel_main(args, device, rank, world, backend):
    """`bench.py --e2e [--gpus N]`: the clip-parallel real propagation as a bench line: a fixed
    `--e2e-frames` clip (strong scaling), N ranks compute the global maps of their frame blocks, ONE collective per round to the
    chain ranks (0: forwards from the annotated frame, 1: backwards), which run local match + head + mask frame by frame
    (examples/propagate_clip.py)."""
    from examples import propagate_clip as pc
    eargs = pc.parse_args(["--frames", str(args.e2e_frames), "--fused-mask-step", "--gpus", str(world)]
                          + (["--two-streams"] if world == 1 else []))
    if world > 1:
        res = pc.run_parallel(eargs, device, rank, world)
    else:
        r1, clip, final = pc.run_single(eargs, device)
        res = {"frames": r1["frames"], "world": 1, "backend": None, "pointwise": r1["pointwise"], "compute": r1["compute"],
               "parallel_ms_per_round": r1["eager_ms_per_round"], "parallel_frames_per_s": r1["eager_frames_per_s"],
               # one GPU: the round's two directions on two HIP streams (what two chain ranks do on two GPUs)
               "two_streams_frames_per_s": r1["two_streams_frames_per_s"],
               "two_streams_masks_equal_eager": r1["two_streams_masks_equal_eager"],
               "masks_bit_equal_to_single_rank": True, "mask_digest": r1["mask_digest"], "collective": None}
    if rank != 0:
        return None
    return {"metric": "propagated frames/sec at 480p, end to end (matching + head + mask step), clip-parallel",
            "value": res["parallel_frames_per_s"], "unit": "frames/s", "n_gpus": world, "steps": res["frames"] - 1,
            "warmup": res["frames"] - 1, "ms_per_step": res["parallel_ms_per_round"] / (res["frames"] - 1),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "examples/propagate_clip.py: %d-frame 480p clip, 2 objects, 1-frame rough_ROI bank, exact fp32 "
                                   "head; ranks compute the global maps of their frame blocks, rank 0 runs the forward half of the sequential "
                                   "chain, rank 1 the backward half"
                                   % res["frames"], "clip_frames": res["frames"]},
            "collective": res.get("collective"), "e2e_parallel": res}


def _r5(x):
    """floats to 5 significant digits, recursively (the compact line is read by a driver that keeps an 8 KB tail)"""
    if isinstance(x, bool) or x is None or isinstance(x, (int, str)):
        return x
    if isinstance(x, float):
        return x if x != x or x in (float("inf"), float("-inf")) else float("%.5g" % x)
    if isinstance(x, dict):
        return {k: _r5(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r5(v) for v in x]
    return x


COMPACT_LIMIT = 4096  # bytes of the LAST stdout line (the driver could not parse a 20.6 KB line)


def compact_line(full):
    """The driver-facing line: the contract's keys + `config`, `roofline`, `cpu_baseline`, `parity`, and scalar summaries of every
    other block, <= COMPACT_LIMIT bytes.  The full blocks go to bench_full.json next to this script and to an earlier stdout
    line prefixed `#bench_full `."""
    if full is None:
        return None
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data")
    out = {k: full.get(k) for k in keep if k in full}
    cfg = dict(full.get("config") or {})
    if cfg.get("workload_short"):
        cfg["workload"] = cfg.pop("workload_short")
    elif isinstance(cfg.get("workload"), str) and len(cfg["workload"]) > 330:
        cfg["workload"] = cfg["workload"][:327] + "..."
    out["config"] = cfg
    roof = full.get("roofline")
    if roof:
        r = {k: roof.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms",
                                      "algorithmic_flops_per_launch")}
        src = roof.get("traffic_source") or {}
        r["traffic_stale"], r["traffic_kernel_source_sha"] = src.get("stale"), src.get("kernel_source_sha")
        out["roofline"] = r
    cb = full.get("cpu_baseline")
    if cb:
        smp = cb.get("sample_short") or cb.get("sample") or ""
        out["cpu_baseline"] = {"value": cb.get("value"), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                               "sample": smp if len(smp) <= 120 else smp[:117] + "..."}
    elif "cpu_baseline" in full:
        out["cpu_baseline"] = None
    if full.get("parity"):
        out["parity"] = {k: v for k, v in full["parity"].items() if k != "reference"}
    ls = full.get("local_stage")
    if ls:
        out["local_stage"] = {"frac": ls.get("frac"), "stage_ms": ls.get("stage_ms"), "window_kernel_ms": ls.get("window_kernel_ms"),
                              "frame_prepare_ms": ls.get("frame_prepare_ms"), "valu_frac": (ls.get("valu") or {}).get("frac"),
                              "max_distance": ls.get("max_distance")}
        sv = ls.get("stored_volume")
        if sv:  # r6: the stage split at its label boundary -- phase 2 is what the sequential chain runs per frame
            out["local_stage"].update({"phase1_us_per_pair": sv.get("phase1_us_per_pair_batched"),
                                       "phase2_us": sv.get("phase2_us_per_frame"), "phase2_hbm_frac": (sv.get("phase2") or {}).get("frac")})
    if "collective" in full:
        out["collective"] = full["collective"]
    if "value_one_shot" in full:
        out["value_one_shot"] = full["value_one_shot"]
    hx = full.get("headline_exact_mode")
    if hx:
        out["headline_exact_mode"] = {"dtype": hx.get("dtype"), "value": hx.get("value"),
                                      "bit_equal_to_f32": hx.get("bit_equal_to_f32_on_probe_frame")}
    if full.get("also"):
        legs = []
        for a in full["also"]:
            un = ((a.get("parity") or {}).get("unrounded_fp32_inputs") or {}).get(a.get("dtype")) or {}
            # (r5 lines: `value` was the plain-bf16 rate and `exact_value` the bf16r one; r6 leads with the tolerance-safe mode)
            plain = a.get("value_plain_bf16", a.get("value"))
            exact = (a.get("exact_mode") or {}).get("value")
            legs.append({"cfg": a.get("cfg"), "dtype": a.get("dtype"), "value": exact if exact is not None else plain,
                         "value_mode": "bf16r" if exact is not None else a.get("dtype"), "value_plain_bf16": plain,
                         "err_0.1": a.get("err_0.1", un.get("err_vs_fp32_oracle_normalised_max")), "err_0.3": a.get("err_0.3"),
                         "ms_per_step_plain_bf16": a.get("ms_per_step"),
                         "frac": (a.get("roofline") or {}).get("frac"), "kernel_ms": a.get("kernel_ms"),
                         "local_window_ms": (a.get("local_stage") or {}).get("window_kernel_ms")})
        out["also"] = legs
    rb = full.get("robustness")
    if rb and rb.get("summary"):
        s = rb["summary"]
        out["robustness"] = {"f32_fps": s.get("f32_frames_per_s"), "bf16r_fps": s.get("bf16r_frames_per_s_iid_video_smooth_flat"),
                             "bf16_err_0.1": s.get("bf16_max_err_scale_0.1"), "bf16_err_0.3": s.get("bf16_max_err_scale_0.3")}
    e = full.get("e2e")
    if e:
        ek = ("value", "value_first_round", "value_fused_local", "value_graph", "value_two_streams", "value_scribble_bank", "value_bank_frames_5",
              "value_full_bank_frames_5", "value_session_8_rounds", "value_bf16r_match", "bf16r_match_masks_equal_f32", "bank", "bank_rows",
              "masks_equal_eager_graph_two_streams")
        ce = {k: e[k] for k in ek if k in e}
        w = e.get("workload") or ""
        ce["workload"] = w if len(w) <= 200 else w[:197] + "..."
        out["e2e"] = ce
    if full.get("e2e_parallel"):
        ep = full["e2e_parallel"]
        out["e2e_parallel"] = {k: ep.get(k) for k in ("frames", "world", "backend", "parallel_frames_per_s",
                                                      "two_streams_frames_per_s", "masks_bit_equal_to_single_rank") if k in ep}
    out["full"] = "bench_full.json"
    out = _r5(out)
    # belt and braces: the line must fit whatever a later block grows to
    for drop in ("e2e_parallel", "headline_exact_mode", "value_one_shot", "robustness", "also", "e2e", "local_stage"):
        if len(json.dumps(out)) <= COMPACT_LIMIT:
            break
        out.pop(drop, None)
    return out


DUMP_LIMIT = 64 << 20  # bytes of `--dump-outputs` in all


def dump_outputs(path, outputs):
    """`--dump-outputs DIR`: the last timed step's results, whole, as float32 DIR/<name>.npy (under 5 MB at every config)"""
    arrays = {k: np.ascontiguousarray(v.detach().float().cpu().numpy()) for k, v in outputs.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT:
        raise SystemExit("bench.py --dump-outputs: %d bytes, more than the %d-byte limit" % (total, DUMP_LIMIT))
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)


def emit(line):
    """rank 0: the full line to bench_full.json and to a prefixed stdout line, then the compact line LAST"""
    try:  # RCCL writes a version banner through C stdio: flush it first so the JSON line comes last
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    full = json.dumps(line)
    try:
        with open(os.path.join(ROOT, "bench_full.json"), "w") as f:
            f.write(full + "\n")
    except OSError:
        pass
    sys.stdout.write("#bench_full " + full + "\n")
    sys.stdout.write(json.dumps(compact_line(line)) + "\n")
    sys.stdout.flush()


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` outside a launcher: start the N ranks ourselves (one process per GPU,
    torch.distributed.run, rendezvous on 127.0.0.1) and relay rank 0's JSON line.  Called BEFORE anything
    in this process touches the GPU -- a process that has initialised HIP must never exec or be the
    parent that matters; this parent only waits and passes the exit code on.  (No device-count pre-check
    here: torch.cuda.device_count() may fall through to hipGetDeviceCount on builds without amdsmi, which
    would initialise the runtime in the parent; ranks without a device fail loudly by themselves.)"""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC only on these hosts (RCCL needs it)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="measure and check beyond the headline: at N = 1 the one-shot rate, the stored-volume local stage, the "
                         "CPU baseline + parity and, for the default workload, `headline_exact_mode`, the `also` legs, "
                         "`robustness` and `e2e` (the --no-* options drop single blocks).  A plain run times the headline only")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="write what the last timed step returned (global_map, global_memory, local_map) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip every CPU-oracle leg (baseline + parity)")
    ap.add_argument("--no-also", action="store_true", help="skip the extra cfg3 / cfg5 bf16 legs of the N=1 line")
    ap.add_argument("--also-steps", type=int, default=40)
    ap.add_argument("--tune", type=str, default="", help="experiments only: key=value,... for manet_tune_set")
    ap.add_argument("--compute", type=str, default="f32", choices=["f32", "bf16", "bf16x3", "bf16r"],
                    help="arithmetic of the QK^T contraction (headline = f32, BASELINE configs[1])")
    ap.add_argument("--cfg", type=int, default=2, choices=[2, 3, 5],
                    help="BASELINE config: 2 = 480p T=5 2 ids d=12 (headline); 3 = 480p T=5 4 ids d=4; "
                         "5 = 720p T=10 6 ids d=4")
    ap.add_argument("--emb", type=str, default="auto", choices=["auto", "f32", "bf16"],
                    help="storage of the embeddings in HBM (auto: bf16 for --compute bf16, else f32)")
    ap.add_argument("--one-shot", action="store_true", help="re-sort / re-pack the bank every frame (r1's step)")
    ap.add_argument("--overlap", action="store_true",
                    help="run the local stage on a second HIP stream (the two matches are independent until the "
                         "segmentation head consumes both maps, IntVOS.py:663-671): +1.7 %% frames/s at cfg2, +2 %% at "
                         "cfg3, but the per-kernel durations then include the interference, so the default keeps one "
                         "stream and clean roofline attribution")
    ap.add_argument("--prepacked", action="store_true",
                    help="query operand images packed when the embeddings were produced (outside the timed region)")
    ap.add_argument("--scaling", type=str, default="weak", choices=["weak", "strong"],
                    help="weak: K frames per rank (the driver's contract); strong: a fixed 64-frame clip (BASELINE "
                         "configs[3]) cut into 64 / N frames per rank (--steps is ignored)")
    ap.add_argument("--data", type=str, default="iid", choices=["iid", "video", "smooth", "flat"],
                    help="embedding distribution of the main leg (tools/synth_clip.py): iid = SURVEY 8d's relu(randn) with "
                         "uniform labels (the headline); video / smooth = spatially smooth, temporally redundant, "
                         "label-coherent clips; flat = all rows of an object identical, the floor (N = 1 only).  The --full line "
                         "brackets all of them in `robustness`.")
    ap.add_argument("--scale", type=float, default=0.1, help="embedding scale (SURVEY 8d: 0.1)")
    ap.add_argument("--no-robustness", action="store_true", help="skip the `robustness` legs of the N=1 line")
    ap.add_argument("--robust-steps", type=int, default=10)
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end `e2e` block of the N=1 line")
    ap.add_argument("--e2e-frames", type=int, default=32)
    ap.add_argument("--e2e", action="store_true",
                    help="print the END-TO-END line instead (matching + head + mask step; with --gpus N the clip-parallel "
                         "propagation of examples/propagate_clip.py: strong scaling over a fixed --e2e-frames clip)")
    ap.add_argument("--bank-ownership", type=str, default="round_robin", choices=["block", "round_robin"],
                    help="who ships which bank frame in the all-gather (clip_parallel): round_robin bounds every rank's "
                         "slab at ceil(T / N) frames")
    args = ap.parse_args()
    if args.emb == "auto":
        args.emb = "bf16" if args.compute in ("bf16", "bf16r") else "f32"

    # MANET_BENCH_BACKEND=gloo: dry run of the N>1 flow on fewer GPUs than ranks (ranks share devices)
    backend = os.environ.get("MANET_BENCH_BACKEND", "nccl")
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if args.e2e and args.dump_outputs:
        raise SystemExit("bench.py --dump-outputs: the matching-path line only (not --e2e)")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # not under a launcher: become the launcher (no GPU call has happened in this process)
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the matching path has no CPU fallback")
    n_dev = torch.cuda.device_count()
    if backend == "nccl" and world > n_dev:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible (one rank per GPU over RCCL)" % (world, n_dev))
    dev_index = local_rank % n_dev
    # MANET_BENCH_FORCE_DIST=1: take the collective code path even with one rank (exercises RCCL on a 1-GPU box)
    use_dist = world > 1 or os.environ.get("MANET_BENCH_FORCE_DIST") == "1"
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        torch.cuda.set_device(dev_index)
        if backend == "nccl":
            try:
                dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
            except TypeError:  # older signature without device_id
                dist.init_process_group("nccl")
        else:
            dist.init_process_group(backend)
    device = torch.device("cuda", dev_index)
    torch.cuda.set_device(device)

    from cvpr2020_manet_amd import _lib, ops
    lib = _lib.load()
    for kv in filter(None, args.tune.split(",")):
        os.environ["MANET_TUNING"] = "1"  # experiments: the setters refuse without the opt-in
        k_, v_ = kv.split("=")
        _lib.check(lib.manet_tune_set(int(k_), int(v_)), "manet_tune_set")

    if args.e2e:
        line = e2e_parallel_main(args, device, rank, world, backend)
        if use_dist:
            dist.destroy_process_group()
        if rank == 0:
            emit(line)
        return

    K, Wm = args.steps, args.warmup
    if args.scaling == "strong":
        K = max(1, 64 // world)
    T = CONFIGS[args.cfg]["T"]
    # this rank's K frames of the clip (synthetic embeddings, resident in HBM); the clip is at least long enough to
    # contain T distinct annotated frames; only K are timed
    wl = Workload(args.cfg, args.compute, args.emb, device, rank, world, n_local=max(K, -(-T // world)), data=args.data,
                  scale=args.scale)
    r = run_leg(wl, K, Wm, args, lib, use_dist=use_dist, one_shot=args.one_shot, prepacked=args.prepacked,
                overlap=args.overlap, ownership=args.bank_ownership)
    elapsed = r["elapsed"]
    t = torch.tensor([elapsed], device=device, dtype=torch.float64)
    if use_dist:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    line = None
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, r.pop("outputs"))
        bank_rows, bank_lab = r["bank_rows"], r["bank_lab"]
        M = int(bank_rows.shape[0])
        assert M == wl.T * wl.H * wl.W, "bank must hold T distinct frames"
        roof, local = roofline_blocks(wl, r["kern_ms"], r["local_ms"], overlap=args.overlap, prep_ms=r["prep_ms"])
        line = {
            "metric": "propagated frames/sec at 480p, 5-frame memory",
            "value": world * K / elapsed,
            "unit": "frames/s",
            "n_gpus": world,
            "steps": K,
            "warmup": Wm,
            "ms_per_step": elapsed / K * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": args.compute,
            "data": "synthetic",
            "config": {"workload": wl.describe(args), "workload_short": wl.describe_short(args), "frames_per_gpu": K,
                       "clip_frames": world * K,
                       "bank_exchange": "1 RCCL all-gather in the timed region" if world > 1 else "none (1 GPU)"},
            "roofline": roof,
            "local_stage": local,
            # what the collective of the timed region saw: a real N-rank run shows world == n_gpus and backend nccl
            "collective": r["collective"] if use_dist else None,
        }
        # everything past the headline takes runs of its own: --full only
        if args.full and world == 1 and not use_dist and local is not None:
            local["stored_volume"] = stored_volume_block(wl, lib)
        if args.full and world == 1 and not args.one_shot and not use_dist:
            # r1's definition next to the headline: the bank re-sorted / re-packed every frame, one-shot API
            r1s = run_leg(wl, min(K, 10), 2, args, lib, one_shot=True)
            line["value_one_shot"] = min(K, 10) / r1s["elapsed"]
        if args.full and not args.no_cpu_baseline and world == 1:
            # the same frame once more on the GPU (fresh map, outside the timed region) for the parity figures
            p = wl.probe_frame()
            g_chk = ops.global_match(bank_rows, wl.frame_emb(p).permute(1, 2, 0), bank_lab, wl.n_ids, normalize=True,
                                     compute=args.compute)
            l_chk = ops.local_match(wl.frame_emb(p + 1).permute(1, 2, 0), wl.frame_emb(p).permute(1, 2, 0),
                                    wl.prev_labs[0], wl.n_ids, wl.d)
            # (bf16 arithmetic on bf16-stored embeddings: the oracle's fp32 formula on the same stored values)
            line["cpu_baseline"], line["parity"] = cpu_baseline(wl, bank_rows, bank_lab, g_chk, l_chk)
        elif args.full and not args.no_cpu_baseline:
            line["cpu_baseline"] = None  # measured on rank 0 at N=1 only (see the N=1 line)
        default_line = (args.full and world == 1 and not use_dist and args.cfg == 2 and args.compute == "f32"
                        and args.data == "iid")
        if default_line:
            del wl, r, bank_rows, bank_lab
            torch.cuda.empty_cache()
        if default_line and not args.no_also:
            # the headline's own workload through the exact bf16 filter + fp32 re-rank: same bits as the fp32 line above
            line["headline_exact_mode"] = exact_leg(2, device, lib, args)
            torch.cuda.empty_cache()
            line["also"] = []
            for cfg_, compute_ in ((3, "bf16"), (5, "bf16")):
                line["also"].append(also_leg(cfg_, compute_, device, lib, args))
                torch.cuda.empty_cache()
        if default_line and not args.no_robustness:
            line["robustness"] = robustness_block(device, lib, args)
        if default_line and not args.no_e2e:
            line["e2e"] = e2e_block(device, args)
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        emit(line)


if __name__ == "__main__":
    main()
