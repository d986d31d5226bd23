#!/usr/bin/env python3
"""One stage-1-shaped training sample behind the encoder, forward + backward: global match + local match + the head's input
assembly + DynamicSegHead + the fused loss (IntVOS.prop_seghead on three frames' embeddings that are leaves requiring grad, then
ops.upsampled_cross_entropy_topk), with train_kernels="fused", train_match="ordered" and train_inputs = the route under test.
Embeddings [100, 104, 104] (the stage-1 crop) and [100, 120, 214] (480p), n_ids = 3.  The method is that of
tools/head_train_bench.py --step-only: HIP events around a step and host wall time per step, warm-up, median of --reps, a fresh
process per (shape, route); every such process runs under its own `timeout` and a non-zero exit status ends the run.
usage: python tools/train_step_bench.py [--reps N] [--routes framework,fused] [--shapes 100x104x104,100x120x214]
       python tools/train_step_bench.py --route ROUTE --shape CxHxW [--reps N]      (one process: what the driver starts)"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = "100x104x104,100x120x214"
N_IDS = 3
STEP_TIMEOUT_S = 240  # one worker: start-up, 5 + 2 * reps steps of a few milliseconds


def worker(route, shape, reps):
    import torch

    from cvpr2020_manet_amd import ops
    from cvpr2020_manet_amd.config import make_cfg
    from cvpr2020_manet_amd.networks import IntVOS as M

    class NoEncoder(torch.nn.Module):  # the sample starts behind the encoder
        def forward(self, x):
            return x

    assert torch.cuda.is_available(), "needs the MI355X"
    C, h, w = shape
    H, W = 4 * h, 4 * w
    cfg = make_cfg(["--TEST_MODE", "False", "--MODEL_SEMANTIC_EMBEDDING_DIM", str(C)])
    kw = {} if route == "framework" else {"train_inputs": route}  # (the default route needs no keyword)
    torch.manual_seed(0)
    model = M.IntVOS(cfg, NoEncoder(), train_kernels="fused", train_match="ordered", **kw).cuda().train()
    embs = [torch.relu(torch.randn(1, C, h, w, device="cuda")).requires_grad_(True) for _ in range(3)]
    ref_lab = torch.randint(0, N_IDS, (1, 1, H, W), device="cuda")
    prev_lab = torch.randint(0, N_IDS, (1, 1, H, W), device="cuda")
    target = torch.randint(0, N_IDS, (1, H, W), device="cuda")
    gt_ids = torch.Tensor([N_IDS - 1])
    k = int(0.15 * H * W)

    def step():
        model.zero_grad(set_to_none=True)
        for e in embs:
            e.grad = None
        logits = model.prop_seghead(embs[0], embs[1], embs[2], ref_lab, prev_lab, True, True, ["clip"], gt_ids, 1, None, None, 1, 0,
                                    [2], model.dynamic_seghead)["clip"]
        ops.upsampled_cross_entropy_topk(logits, target, (H, W), k).backward()

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    assert all(e.grad is not None and bool(torch.isfinite(e.grad).all()) for e in embs)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):  # host time per step: the launches queue ahead unless the host is the bound
        step()
    host_us = (time.perf_counter() - t0) / reps * 1e6
    torch.cuda.synchronize()
    print("post-encoder train sample [%d,%d,%d] n_ids=%d train_inputs=%r: %.1f us (events, median of %d), host %.1f us per step"
          % (C, h, w, N_IDS, route, statistics.median(ts), reps, host_us), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--routes", default="framework,fused")
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--route", default=None, help="run ONE route in this process (what the driver starts)")
    ap.add_argument("--shape", default=None)
    a = ap.parse_args()
    if a.route is not None:
        worker(a.route, tuple(int(v) for v in (a.shape or SHAPES.split(",")[0]).split("x")), a.reps)
        return
    for shape in a.shapes.split(","):
        for route in a.routes.split(","):
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--route", route, "--shape",
                   shape, "--reps", str(a.reps)]
            rc = subprocess.run(cmd).returncode
            if rc != 0:  # a fault, an abort or the time limit: nothing more is started on the GPU
                print("train_step_bench: %s %s ended with status %d -- stopping" % (shape, route, rc), flush=True)
                sys.exit(rc)


if __name__ == "__main__":
    main()
