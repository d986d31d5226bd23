#!/usr/bin/env python3
"""Host time of the heads' Python routing: a loop of DynamicSegHead.forward_shared at a launch-bound shape ([1,100,10,12] shared,
3 objects; the kernels are far shorter than the host's work between them), one memo, in each pointwise / head_act mode -- and the
wall time of tools/head_bench.py's loop at its default shape.  One JSON line.

python3 tools/head_routes_bench.py [--root TREE] [--iters 3000] [--head-bench 200]
  --root TREE   time the package and the tools of another checkout (a parent commit's, with its library built) instead of this one"""
import argparse
import json
import os
import runpy
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--iters", type=int, default=3000)
ap.add_argument("--head-bench", type=int, default=200)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
from cvpr2020_manet_amd.networks import IntVOS as M  # noqa: E402

out = {"root": ROOT, "iters": args.iters, "forward_shared_us": {}}
h, w, n = 10, 12, 3
torch.manual_seed(0)
with torch.no_grad():
    shared = torch.relu(torch.randn(1, 100, h, w, device="cuda")) * 0.3
    per = torch.rand(n, 3, h, w, device="cuda")
    for pointwise in ("f32", "split", "split3", False):
        for act in ("f32", "f16"):
            head = M.DynamicSegHead(in_dim=103, embed_dim=256).cuda().eval()
            for blk in head.modules():
                if isinstance(blk, M._split_separable_conv2d):
                    object.__setattr__(blk, "_pw_mode", pointwise)
            M.use_head_act(head, act)
            memo = {}
            for _ in range(300):
                head.forward_shared(shared, per, memo=memo)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                head.forward_shared(shared, per, memo=memo)
            torch.cuda.synchronize()
            out["forward_shared_us"]["%s/%s" % (pointwise, act)] = round((time.perf_counter() - t0) / args.iters * 1e6, 2)

if args.head_bench:
    tool, argv = os.path.join(ROOT, "tools", "head_bench.py"), sys.argv
    try:
        sys.argv = [tool, "20"]
        runpy.run_path(tool, run_name="__main__")  # (warm: allocations, first launches)
        sys.argv = [tool, str(args.head_bench)]
        t0 = time.perf_counter()
        runpy.run_path(tool, run_name="__main__")
        out["head_bench_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        out["head_bench_calls"] = args.head_bench
    finally:
        sys.argv = argv
print(json.dumps(out))
