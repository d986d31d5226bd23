#!/usr/bin/env python3
"""The training loss behind the head: the framework's chain (F.interpolate bilinear align_corners=True -> cross_entropy with
ignore_index=255, reduction='none' -> torch.topk -> mean, and autograd through all of it) against the fused op of
csrc/loss_train.hip (ops.upsampled_cross_entropy_topk), forward and forward + backward, at the two training sizes and k = 15 %, 50 %
and 100 % of the pixels; then one DynamicSegHead(train_kernels="all") train step with either loss.  HIP events, warm-up, median of
repeats; the two routes alternate inside one process.
usage: python tools/loss_bench.py [--reps N] [--json FILE] [--no-head]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvpr2020_manet_amd import ops  # noqa: E402
from cvpr2020_manet_amd.networks import IntVOS as M  # noqa: E402

SHAPES = [((1, 3, 104, 104), (416, 416)), ((1, 3, 120, 214), (480, 854))]
FRACTIONS = (0.15, 0.5, 1.0)


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def framework_loss(logits, labels, size, k):
    up = F.interpolate(logits, size=size, mode="bilinear", align_corners=True)
    B, C = up.shape[:2]
    pix = F.cross_entropy(up.view(B, C, -1), labels.view(B, -1), ignore_index=255, reduction="none")
    return torch.topk(pix, k=k, dim=1)[0].mean()


def fused_loss(logits, labels, size, k):
    return ops.upsampled_cross_entropy_topk(logits, labels, size, k)


def inputs(shape, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(shape, generator=g) * 3
    labels = torch.randint(0, shape[1], (shape[0],) + size, generator=g)
    labels[torch.rand((shape[0],) + size, generator=g) < 0.05] = 255
    return logits.cuda(), labels.cuda()


def op_rows(reps):
    rows = []
    for shape, size in SHAPES:
        logits, labels = inputs(shape, size)
        x = logits.clone().requires_grad_(True)
        for frac in FRACTIONS:
            k = int(frac * size[0] * size[1])
            r = {"logits": list(shape), "size": list(size), "k": k, "fraction": frac}
            for name, fn in (("framework", framework_loss), ("hip", fused_loss)):
                def fwd():
                    with torch.no_grad():
                        fn(logits, labels, size, k)

                def fwd_bwd():
                    x.grad = None
                    fn(x, labels, size, k).backward()
                r[name + "_fwd_us"] = round(timed(fwd, reps), 1)
                r[name + "_fwd_bwd_us"] = round(timed(fwd_bwd, reps), 1)
            r["speedup_fwd_bwd"] = round(r["framework_fwd_bwd_us"] / r["hip_fwd_bwd_us"], 2)
            rows.append(r)
    return rows


def head_rows(reps):
    """a DynamicSegHead("all") train step at [3, 256, 104, 104] (two objects + background) with the loss at 416 x 416, k = 15 %"""
    torch.manual_seed(0)
    head = M.DynamicSegHead(in_dim=256, train_kernels="all").cuda().train()
    x = torch.randn(3, 256, 104, 104, device="cuda")
    size = (416, 416)
    labels = inputs((1, 3, 104, 104), size, seed=1)[1]
    k = int(0.15 * size[0] * size[1])
    r = {"shape": [3, 256, 104, 104], "size": list(size), "k": k}
    for name, fn in (("framework", framework_loss), ("hip", fused_loss)):
        def step():
            head.zero_grad(set_to_none=True)
            fn(head(x).permute(1, 0, 2, 3), labels, size, k).backward()
        r[name + "_loss_step_us"] = round(timed(step, reps), 1)

    def bare():
        head.zero_grad(set_to_none=True)
        head(x).sum().backward()
    r["sum_step_us"] = round(timed(bare, reps), 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-head", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rows = op_rows(a.reps)
    print("%-18s %-10s %8s | %9s %9s | %9s %9s | %s" % ("logits", "size", "k", "fw fwd", "fw f+b", "hip fwd", "hip f+b", "f+b speed-up (us)"))
    for r in rows:
        print("%-18s %-10s %8d | %9.1f %9.1f | %9.1f %9.1f | %.2fx" % (
            tuple(r["logits"]), "%dx%d" % tuple(r["size"]), r["k"], r["framework_fwd_us"], r["framework_fwd_bwd_us"], r["hip_fwd_us"],
            r["hip_fwd_bwd_us"], r["speedup_fwd_bwd"]))
    res = {"device": torch.cuda.get_device_name(0), "loss": rows}
    if not a.no_head:
        h = head_rows(max(10, a.reps // 2))
        print("DynamicSegHead 'all' train step %s + loss at %s, k = %d: framework loss %.1f us, HIP loss %.1f us (the step with .sum() "
              "for a loss: %.1f us)" % (tuple(h["shape"]), tuple(h["size"]), h["k"], h["framework_loss_step_us"], h["hip_loss_step_us"],
                                        h["sum_step_us"]))
        res["head_step"] = h
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
