#!/usr/bin/env python3
"""head_act="f16" against the fp32 head on the GPU, one process, modes alternating, warm; writes profiles/head_f16_bench.json.

  kernels     per stage at [3,256,120,214] and [2,256,120,214]: the fp32 depthwise against the f16 depthwise with both input types;
              conv1x1_mfma (manet_conv1x1_f32 and its add / fused-logits forms) and conv1x1_split against the f16 1x1 in its three
              forms; layer 1's per-object half as the two launches it was (depthwise on [n,3] + 1x1 K=3 with the term) against
              the fused kernel.  The entry points are called directly on preallocated, ROTATING buffers (a single hot activation sits in the
              memory-side cache): mean of N launches between two events, R repeats, the minimum and the maximum of the means.
  head        the whole DynamicSegHead.forward_shared (layer 1's shared term memoised) as a captured graph, replayed: f32, split, f16, and f16
              with layer 1's per-object half put back on its two launches.
  end to end  examples/propagate_clip.py's round at the roi bank, 480p, 2 objects: pointwise f32 / split / head_act f16, each under
              compute f32 and f16r; frames/s of every pass, and the f16 run's logit errors / mask flips against the fp32 head.
The encoder and head weights are stand-ins: times do not depend on them, the error figures are THIS model's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cvpr2020_manet_amd import _lib, ops  # noqa: E402
from cvpr2020_manet_amd.networks import IntVOS as M  # noqa: E402

NBUF = 6
L1_TWO = "layer 1 object half: two launches (dw [n,3] f32->f16 + 1x1 K=3 add+relu f16)"
L1_FUSED = "layer 1 object half: fused f16"


def mean_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def alternate(rows, n, repeats):
    """rows: name -> fn(i); every repeat times every row once, in turn -> name -> {"min_us", "max_us"}"""
    for fn in rows.values():
        mean_us(fn, n)
    seen = {k: [] for k in rows}
    for _ in range(repeats):
        for k, fn in rows.items():
            seen[k].append(mean_us(fn, n))
    return {k: {"min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in seen.items()}


def kernel_rows(n_ids, h, w, n, repeats):
    lib, dev, HW = _lib.load(), torch.device("cuda", 0), h * w
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(n_ids)
    x32 = [torch.relu(torch.randn(n_ids, 256, h, w, device=dev, generator=g)) * 0.5 for _ in range(NBUF)]
    x16 = [t.half() for t in x32]
    p32 = [t[:, :3].contiguous() for t in x32]  # layer 1's per-object channels
    p16 = [t.half() for t in p32]
    d16 = [torch.empty_like(t) for t in p16]  # the two-launch form's fp16 planes between its launches
    o32 = [torch.empty_like(t) for t in x32]
    o16 = [torch.empty_like(t) for t in x16]
    logit = torch.empty(n_ids, 1, h, w, device=dev)
    term = [torch.randn(256, h, w, device=dev, generator=g) for _ in range(NBUF)]
    wdw = torch.randn(256, 1, 7, 7, device=dev, generator=g) * 0.1
    vec = [torch.randn(256, device=dev, generator=g) * 0.1 for _ in range(4)]
    hw_ = torch.randn(256, device=dev, generator=g) * 0.1
    w2t, w2t3 = torch.randn(256, 256, device=dev, generator=g) * 0.05, torch.randn(3, 256, device=dev, generator=g) * 0.3
    sw, sw3, hw16, hw163 = ops.SplitWeight(w2t), ops.SplitWeight(w2t3), ops.HalfWeight(w2t), ops.HalfWeight(w2t3)
    P = lambda t: t.data_ptr()
    bias, scale, shift, b2 = (P(v) for v in vec)
    C = 256
    rows = {
        "dw f32 -> f32": lambda i: lib.manet_dwconv7x7_bn_relu_ex(P(x32[i % NBUF]), n_ids, C, h, w, P(wdw), bias, scale, shift, 1, 0, P(o32[i % NBUF]), st),
        "dw f32 -> f16": lambda i: lib.manet_dwconv7x7_bn_relu_f16(P(x32[i % NBUF]), 0, n_ids, C, h, w, P(wdw), bias, scale, shift, P(o16[i % NBUF]), st),
        "dw f16 -> f16": lambda i: lib.manet_dwconv7x7_bn_relu_f16(P(x16[i % NBUF]), 1, n_ids, C, h, w, P(wdw), bias, scale, shift, P(o16[i % NBUF]), st),
        "1x1 K=256 relu: f32 (conv1x1_mfma)": lambda i: lib.manet_conv1x1_f32(P(x32[i % NBUF]), C * HW, n_ids, C, HW, P(w2t), b2, 256, 1, P(o32[i % NBUF]), st),
        "1x1 K=256 relu: split": lambda i: lib.manet_conv1x1_x3_f32(P(x32[i % NBUF]), C * HW, n_ids, C, HW, P(sw.packed), b2, None, 256, 1, P(o32[i % NBUF]), None, None, None, st),
        "1x1 K=256 relu: f16": lambda i: lib.manet_conv1x1_f16(P(x16[i % NBUF]), C * HW, n_ids, C, HW, P(hw16.packed), b2, None, 256, 1, P(o16[i % NBUF]), 0, None, None, None, st),
        "1x1 K=3 add + relu: f32 (conv1x1_mfma)": lambda i: lib.manet_conv1x1_add_f32(P(p32[i % NBUF]), 3 * HW, n_ids, 3, HW, P(w2t3), b2, P(term[i % NBUF]), 256, 1, P(o32[i % NBUF]), st),
        "1x1 K=3 add + relu: split": lambda i: lib.manet_conv1x1_x3_f32(P(p32[i % NBUF]), 3 * HW, n_ids, 3, HW, P(sw3.packed), b2, P(term[i % NBUF]), 256, 1, P(o32[i % NBUF]), None, None, None, st),
        "1x1 K=3 add + relu: f16": lambda i: lib.manet_conv1x1_f16(P(p16[i % NBUF]), 3 * HW, n_ids, 3, HW, P(hw163.packed), b2, P(term[i % NBUF]), 256, 1, P(o16[i % NBUF]), 0, None, None, None, st),
        "1x1 K=256 -> logits: f32 (conv1x1_mfma)": lambda i: lib.manet_conv1x1_head_f32(P(x32[i % NBUF]), C * HW, n_ids, C, HW, P(w2t), b2, 256, 0, None, P(hw_), None, P(logit), st),
        "1x1 K=256 -> logits: split": lambda i: lib.manet_conv1x1_x3_f32(P(x32[i % NBUF]), C * HW, n_ids, C, HW, P(sw.packed), b2, None, 256, 0, None, P(hw_), None, P(logit), st),
        "1x1 K=256 -> logits: f16": lambda i: lib.manet_conv1x1_f16(P(x16[i % NBUF]), C * HW, n_ids, C, HW, P(hw16.packed), b2, None, 256, 0, None, 0, P(hw_), None, P(logit), st),
    }

    def two_launches(i):  # layer 1's per-object half as head_act="f16" ran it before the fused kernel
        j = i % NBUF
        return (lib.manet_dwconv7x7_bn_relu_f16(P(p32[j]), 0, n_ids, 3, h, w, P(wdw), bias, scale, shift, P(d16[j]), st)
                or lib.manet_conv1x1_f16(P(d16[j]), 3 * HW, n_ids, 3, HW, P(hw163.packed), b2, P(term[j]), 256, 1, P(o16[j]), 0, None, None, None, st))

    rows[L1_TWO] = two_launches
    rows[L1_FUSED] = lambda i: lib.manet_head_layer1_object_f16(P(p32[i % NBUF]), n_ids, 3, h, w, P(wdw), bias, scale, shift, P(hw163.packed), b2, P(term[i % NBUF]), 1, P(o16[i % NBUF]), st)
    for k, fn in rows.items():
        assert fn(0) == 0, (k, lib.manet_last_error_string())
    return alternate(rows, n, repeats)


def head_rows(n_ids, h, w, n, repeats):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    base = M.DynamicSegHead(in_dim=103, embed_dim=256).to(dev).eval()
    emb = torch.relu(torch.randn(1, 100, h, w, device=dev)) * 0.3
    per = torch.rand(n_ids, 3, h, w, device=dev)
    rows, keep = {}, []
    fused_ok = ops.head_layer1_object_f16_ok
    for name, pw, act in (("f32", "f32", "f32"), ("split", "split", "f32"), ("head_act f16", "f32", "f16"),
                          ("head_act f16, layer 1 object half as two launches", "f32", "f16")):
        ops.head_layer1_object_f16_ok = (lambda per_object: False) if "two launches" in name else fused_ok
        head = M.DynamicSegHead(in_dim=103, embed_dim=256).to(dev).eval()
        head.load_state_dict(base.state_dict())
        for m in head.modules():
            if isinstance(m, M._split_separable_conv2d):
                object.__setattr__(m, "_pw_mode", pw)
        M.use_head_act(head, act)
        memo = {}
        with torch.no_grad():
            head.forward_shared(emb, per, memo=memo)  # folds, packs, and memoises the shared term
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = head.forward_shared(emb, per, memo=memo)
        keep.append((head, memo, out))
        rows[name] = lambda i, g=graph: g.replay()
    ops.head_layer1_object_f16_ok = fused_ok
    return alternate(rows, n, repeats)


def end_to_end(frames, rounds, passes):
    from examples import propagate_clip as pc
    dev = torch.device("cuda", 0)
    out = {}
    configs = [(c, name, extra) for c in ("f32", "f16r")
               for name, extra in (("f32", []), ("split", ["--pointwise", "split"]), ("head_act f16", ["--head-act", "f16"]))]
    for p in range(passes):
        for compute, name, extra in configs:
            args = pc.parse_args(["--frames", str(frames), "--fused-mask-step", "--rounds", str(rounds), "--compute", compute] + extra)
            res, _, _ = pc.run_single(args, dev)
            row = out.setdefault("compute %s, %s" % (compute, name), {"frames_per_s": []})
            row["frames_per_s"].append(round(res["eager_frames_per_s"], 1))
            row["grid"], row["bank_rows"] = res["grid"], res["bank_rows"]
            if "head_act" in res:
                row["against_the_fp32_head"] = res["head_act"]
            torch.cuda.empty_cache()
    for row in out.values():
        row["min"], row["max"] = min(row["frames_per_s"]), max(row["frames_per_s"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50, help="launches per mean")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_f16_bench.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "launches_per_mean": a.launches, "repeats": a.repeats, "kernels_us": {}, "head_us": {}}
    for n_ids in (3, 2):
        key = "[%d,256,120,214]" % n_ids
        res["kernels_us"][key] = kernel_rows(n_ids, 120, 214, a.launches, a.repeats)
        torch.cuda.empty_cache()
        res["head_us"][key] = head_rows(n_ids, 120, 214, a.launches, a.repeats)
        torch.cuda.empty_cache()
        for sect in ("kernels_us", "head_us"):
            for k, v in res[sect][key].items():
                print("%s %-78s %7.1f .. %7.1f us" % (key, k, v["min_us"], v["max_us"]), flush=True)
    # the module takes the fused form only if it wins outright at both shapes: its largest mean below the two launches' smallest
    res["layer1_object_half_fused_accepted"] = all(v[L1_FUSED]["max_us"] < v[L1_TWO]["min_us"] for v in res["kernels_us"].values())
    print("layer 1 object half, fused form accepted:", res["layer1_object_half_fused_accepted"], flush=True)
    if not a.skip_e2e:
        res["end_to_end"] = end_to_end(a.frames, a.rounds, a.passes)
        for k, v in res["end_to_end"].items():
            print("%-32s %s frames/s %s" % (k, v["frames_per_s"], v.get("against_the_fp32_head", "")), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
