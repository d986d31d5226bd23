#!/usr/bin/env python3
"""compute="f16" against compute="bf16" / "f32": the figures bench.py's fixed --compute list cannot give.

  kernel   the main kernel of the global match (device events around the launch, profile channel 0) at BASELINE configs[2]
           (480p grid 120x214, 5-frame bank, 4 ids) and configs[4] (720p grid 180x320, 10-frame bank, 6 ids), C = 100:
           f16_match_wide_kernel<7> against global_match_bf16_wide_kernel<7, false> in ONE process, after a warm-up of both, alternating rounds of N launches each; per round the median, per mode the median and the spread of the
           round medians -- a difference inside the bf16 kernel's own round-to-round spread is no difference.
  e2e      examples/propagate_clip.py's propagated frame (--fused-mask-step, roi bank) with the same clip under f32, f16 and
           bf16: frames/s, max logit error and the share of mask pixels that differ from the f32 run.

  --refine compute="f16r" (fp16 filter + exact fp32 re-rank) against "bf16r" and "f32", the same method: per data set the three
           modes alternate in one process on the SAME tensors, a round = `launches` whole matches between two device events (a
           refine match is several launches), per mode the median and the spread of the round medians; with the candidate rows
           per pair and the rescued-tile share of both refine modes (adaptive policy off).  Shapes: cfg3 (120x214 grid, 5-frame
           bank, 4 ids) and the example's roi bank (one annotated frame labelled by rough_ROI, 3 ids) x data: i.i.d.,
           bench.py's video-like and smooth clips, the example encoder's embeddings.  Then the example's propagated frame
           (--fused-mask-step, roi bank) under f32 | bf16r | f16r: frames/s, masks compared with the f32 run's.

python3 tools/f16_match_bench.py [--out FILE.json] [--rounds 7] [--launches 40] [--skip-e2e] [--modes bf16,f16] [--refine]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from cvpr2020_manet_amd import _lib, ops  # noqa: E402

CFG = {"cfg3": (120, 214, 5, 4), "cfg5": (180, 320, 10, 6)}
MODES = ("bf16", "f16")


def kernel_ms(fn, n):
    lib = _lib.load()
    _lib.check(lib.manet_profile_begin(n), "manet_profile_begin")
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    ms = (ctypes.c_float * n)()
    k = ctypes.c_int(0)
    _lib.check(lib.manet_profile_end(ms, n, ctypes.byref(k)), "manet_profile_end")
    assert k.value == n, (k.value, n)
    return [ms[i] for i in range(n)]


def kernel_part(rounds, launches, modes=MODES):
    dev = torch.device("cuda:0")
    out = {}
    for name, (h, w, T, n_ids) in CFG.items():
        g = torch.Generator(device=dev).manual_seed(20200614)
        cur = torch.relu(torch.randn(100, h, w, generator=g, device=dev)) * 0.1
        bank = torch.relu(torch.randn(T * h * w, 100, generator=g, device=dev)) * 0.1
        lab = torch.randint(0, n_ids, (T * h * w,), generator=g, device=dev, dtype=torch.int32)
        run = {}
        for m in modes:
            pb = ops.PreparedBank(bank, lab, n_ids, compute=m)
            fr = ops.prepare_frames(cur, compute=m)
            run[m] = (lambda pb=pb, fr=fr: pb.match(fr, normalize=True))
        for _ in range(3):  # warm-up: code objects, workspaces, clocks (about a second of matrix work)
            for m in modes:
                kernel_ms(run[m], launches)
        med = {m: [] for m in modes}
        for _ in range(rounds):
            for m in modes:
                med[m].append(statistics.median(kernel_ms(run[m], launches)))
        res = {}
        for m in modes:
            res[m] = {"round_medians_us": [round(x * 1e3, 2) for x in med[m]], "median_us": round(statistics.median(med[m]) * 1e3, 2),
                      "spread_us": round((max(med[m]) - min(med[m])) * 1e3, 2)}
        if "f16" in res and "bf16" in res:
            res["f16_over_bf16"] = round(res["f16"]["median_us"] / res["bf16"]["median_us"], 4)
        res["shape"] = {"grid": [h, w], "bank_rows": T * h * w, "n_ids": n_ids, "C": 100}
        out[name] = res
        print(name, json.dumps(res), flush=True)
    return out


def e2e_part(rounds):
    import propagate_clip as pc
    dev = torch.device("cuda:0")
    out, logits, masks = {}, {}, {}
    for compute in ("f32", "f16", "bf16"):
        args = pc.parse_args(["--fused-mask-step", "--compute", compute, "--bank", "roi", "--rounds", str(rounds)])
        res, clip, final = pc.run_single(args, dev)
        keep = {}
        with torch.no_grad():
            masks[compute] = clip.one_round(keep_logits=keep)
        logits[compute] = keep
        out[compute] = {"frames_per_s": round(res["eager_frames_per_s"], 1), "ms_per_round": round(res["eager_ms_per_round"], 2),
                        "bank_rows": res["bank_rows"], "grid": res["grid"]}
        if compute != "f32":
            out[compute]["logit_max_abs_diff_vs_f32"] = max(float((keep[k] - logits["f32"][k]).abs().max()) for k in keep)
            out[compute]["mask_pixels_differing_vs_f32"] = float((masks[compute] != masks["f32"]).float().mean())
        print(compute, json.dumps(out[compute]), flush=True)
        del clip
    out["max_abs_logit_f32"] = max(float(v.abs().max()) for v in logits["f32"].values())
    return out


REFINE_MODES = ("f32", "bf16r", "f16r")


def _refine_data(dev):
    """{(shape, data): (bank rows [M, C], int32 labels [M], query [h, w, C] view, n_ids)}"""
    import bench
    import propagate_clip as pc
    h, w, T, n_ids = CFG["cfg3"]
    out = {}
    args = pc.parse_args(["--fused-mask-step"])
    cfg, model = pc.build_model(dev)
    enc = pc.synthetic_clip(model, dev, T + 1, args.height, args.width, args.objects).float().contiguous()  # [T + 1, C, 120, 214]
    assert tuple(enc.shape[2:]) == (h, w), enc.shape
    g = torch.Generator(device=dev).manual_seed(20200614)
    clips = {"iid": (torch.relu(torch.randn(T + 1, 100, h, w, generator=g, device=dev)) * 0.1,
                     torch.randint(0, n_ids, (T + 1, h, w), generator=g, device=dev, dtype=torch.int32)),
             "video": bench._synthetic_scene("video", T + 1, h, w, n_ids, 0.1, dev, 20200617),
             "smooth": None,
             "encoder": (enc, torch.randint(0, n_ids, (T + 1, h, w), generator=g, device=dev, dtype=torch.int32))}
    roi = pc.rough_ROI(pc.make_scribble(dev, h, w, args.objects)).reshape(-1).to(torch.int32)  # -1 = unlabelled, ids 0..objects
    for data in ("iid", "video", "smooth", "encoder"):
        emb, lab = clips[data] if clips[data] is not None else bench._synthetic_scene("smooth", T + 1, h, w, n_ids, 0.1, dev, 20200617)
        C = emb.shape[1]
        rows = lambda f: emb[f].permute(1, 2, 0).reshape(-1, C)  # noqa: E731
        q = emb[T // 2 + 1].permute(1, 2, 0)  # a frame from the middle of the clip; the bank: the other T
        bank = [f for f in range(T + 1) if f != T // 2 + 1]
        out[("cfg3", data)] = (torch.cat([rows(f) for f in bank]).contiguous(), torch.cat([lab[f].reshape(-1) for f in bank]).contiguous(),
                               q, n_ids)
        out[("roi", data)] = (rows(T // 2).contiguous(), roi, q, args.objects + 1)
    return out


def refine_part(rounds, launches):
    dev = torch.device("cuda:0")
    out = {}
    for (shape, data), (k, lab, q, n_ids) in _refine_data(dev).items():
        banks = {m: ops.PreparedBank(k, lab, n_ids, compute=m) for m in REFINE_MODES}
        want = banks["f32"].match(q)
        res = {"bank_rows": int((lab >= 0).sum()), "queries": q.shape[0] * q.shape[1], "n_ids": n_ids, "C": k.shape[1]}
        for m in REFINE_MODES[1:]:
            assert torch.equal(banks[m].match(q, adaptive=False), want), (shape, data, m)
            st = banks[m].refine_stats_full()
            res[m] = {"candidate_rows_per_pair": round(st["candidate_rows_per_pair"], 2),
                      "rescued_tile_fraction": round(st["rescued_tile_fraction"], 4), "list_overflowed": st["list_overflowed"]}
        res["f32"] = {}

        def timed(m):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                banks[m].match(q, normalize=True, adaptive=False)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / launches

        for m in REFINE_MODES:  # warm-up
            timed(m)
        med = {m: [] for m in REFINE_MODES}
        for _ in range(rounds):
            for m in REFINE_MODES:
                med[m].append(timed(m))
        for m in REFINE_MODES:
            res[m].update({"round_ms": [round(x, 4) for x in med[m]], "median_ms": round(statistics.median(med[m]), 4),
                           "spread_ms": round(max(med[m]) - min(med[m]), 4)})
        out["%s/%s" % (shape, data)] = res
        print(shape, data, json.dumps(res), flush=True)
        del banks
    return out


def refine_e2e_part(rounds):
    import propagate_clip as pc
    dev = torch.device("cuda:0")
    out, masks = {}, {}
    for compute in REFINE_MODES:
        args = pc.parse_args(["--fused-mask-step", "--compute", compute, "--bank", "roi", "--rounds", str(rounds)])
        res, clip, final = pc.run_single(args, dev)
        masks[compute] = final
        out[compute] = {"frames_per_s": round(res["eager_frames_per_s"], 1), "ms_per_round": round(res["eager_ms_per_round"], 2),
                        "bank_rows": res["bank_rows"], "grid": res["grid"], "mask_digest": res["mask_digest"],
                        "masks_equal_f32": bool(torch.equal(final, masks["f32"]))}
        print(compute, json.dumps(out[compute]), flush=True)
        del clip
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--refine", action="store_true", help="the f16r / bf16r / f32 comparison instead of the f16 / bf16 one")
    ap.add_argument("--modes", type=str, default=",".join(MODES), help="modes of the kernel part (bf16 alone: a library without f16)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    res = {"device": torch.cuda.get_device_name(0)}
    if args.refine:
        if not args.skip_kernel:
            res["match"] = refine_part(args.rounds, args.launches)
        if not args.skip_e2e:
            res["e2e"] = refine_e2e_part(args.e2e_rounds)
    elif not args.skip_kernel:
        res["kernel"] = kernel_part(args.rounds, args.launches, tuple(args.modes.split(",")))
    if not args.skip_e2e and not args.refine:
        res["e2e"] = e2e_part(args.e2e_rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
