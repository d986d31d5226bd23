#!/usr/bin/env python3
"""The matching path of a stage-1 training step (train_stage1.py:126-158: IntVOS.forward's global and local match with both
embeddings requiring grad, then backward): the default route (float atomics in the backward) against the ordered, atomic-free
one (ops.global_match / ops.local_match with deterministic=True, csrc/match_train.hip).  Global and local, forward and forward +
backward, at the stage-1 crop [100, 104, 104] (M0 = 10 816) with 3 and 5 ids, k = 1 and 3, d = 12, and at [100, 120, 214]; the
number of (query, object, rank) entries / (pixel, object) winners that carry gradient is printed beside the times.  HIP events,
warm-up, median of repeats; the routes alternate inside one process.
usage: python tools/match_train_bench.py [--reps N] [--routes atomic,ordered] [--json FILE]
       --package-root DIR   time the package of another checkout (it knows the routes it knows: pass --routes atomic for one
                            that predates the ordered route)
       --step               one line per shape: global + local, forward + backward, of the FIRST route only (A/B between processes)
       --trace N            N untimed steps at [100, 104, 104], 3 ids, k = 1 of the first route, for a profiler's kernel trace"""
import argparse
import json
import os
import statistics
import sys

import torch

C, D = 100, 12
CASES = [(104, 104, 3, 1), (104, 104, 3, 3), (104, 104, 5, 1), (104, 104, 5, 3), (120, 214, 3, 1)]  # h, w, n_ids, k
STEP_SHAPES = [(104, 104, 3, 1), (120, 214, 3, 1)]


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


def blobs(h, w, n_ids, g):
    """every pixel takes the id of the nearest of n_ids random centres: compact regions, all ids present"""
    cy, cx = torch.rand(n_ids, generator=g) * h, torch.rand(n_ids, generator=g) * w
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    return ((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2).argmin(0).to(torch.int32)


def inputs(h, w, n_ids, seed=0):
    g = torch.Generator().manual_seed(seed)
    emb = [(torch.relu(torch.randn(C, h, w, generator=g)) * 0.1).cuda().requires_grad_(True) for _ in range(3)]  # C-major, as the head writes
    labs = [blobs(h, w, n_ids, g).cuda() for _ in range(2)]
    gouts = [torch.randn(h * w, n_ids, generator=g).cuda(), torch.randn(h, w, n_ids, generator=g).cuda()]
    return emb, labs, gouts


def route_kw(route):
    return {"deterministic": True} if route == "ordered" else {}


def saved_arg(out):
    """the selection the op recorded for its backward (the int32 tensor its autograd node keeps)"""
    node = out.grad_fn
    while node is not None and not hasattr(node, "saved_tensors"):
        node = node.next_functions[0][0] if node.next_functions else None
    return [t for t in node.saved_tensors if t.dtype == torch.int32][0]


class Case:
    def __init__(self, ops, h, w, n_ids, k, route):
        self.ops, self.n_ids, self.k, self.kw = ops, n_ids, k, route_kw(route)
        (self.ref, self.prev, self.cur), (self.ref_lab, self.prev_lab), (self.gg, self.gl) = inputs(h, w, n_ids)

    def hwc(self, t):
        return t.permute(1, 2, 0)

    def global_fwd(self):
        return self.ops.global_match(self.hwc(self.ref), self.hwc(self.cur), self.ref_lab, self.n_ids, self.k, **self.kw)

    def local_fwd(self):
        return self.ops.local_match(self.hwc(self.prev), self.hwc(self.cur), self.prev_lab, self.n_ids, D, **self.kw)

    def zero(self):
        self.ref.grad = self.prev.grad = self.cur.grad = None

    def global_step(self):
        self.zero()
        self.global_fwd().backward(self.gg)

    def local_step(self):
        self.zero()
        self.local_fwd().backward(self.gl)

    def step(self):
        self.zero()
        torch.autograd.backward([self.global_fwd(), self.local_fwd()], [self.gg, self.gl])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--routes", default="atomic,ordered")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from cvpr2020_manet_amd import ops
    assert torch.cuda.is_available(), "needs the MI355X"
    routes = a.routes.split(",")
    if a.trace:
        case = Case(ops, 104, 104, 3, 1, routes[0])
        for _ in range(a.trace):
            case.step()
        torch.cuda.synchronize()
        print("traced %d steps of the %s route" % (a.trace, routes[0]))
        return
    if a.step:
        for h, w, n_ids, k in STEP_SHAPES:
            case = Case(ops, h, w, n_ids, k, routes[0])
            print("%s route, global + local forward + backward [%d, %d, %d], %d ids, k = %d, d = %d: %.1f us (events, median of %d)"
                  % (routes[0], C, h, w, n_ids, k, D, timed(case.step, a.reps), a.reps))
        return
    rows = []
    for h, w, n_ids, k in CASES:
        r = {"shape": [C, h, w], "n_ids": n_ids, "k": k, "d": D}
        for route in routes:
            case = Case(ops, h, w, n_ids, k, route)
            r[route + "_global_fwd_us"] = round(timed(case.global_fwd, a.reps), 1)
            r[route + "_global_fwd_bwd_us"] = round(timed(case.global_step, a.reps), 1)
            if k == 1 or (h, w, n_ids) == CASES[0][:3]:  # (the local match does not depend on k)
                r[route + "_local_fwd_us"] = round(timed(case.local_fwd, a.reps), 1)
                r[route + "_local_fwd_bwd_us"] = round(timed(case.local_step, a.reps), 1)
            garg = saved_arg(case.global_fwd())
            r["global_entries"] = int((garg >= 0).sum())
            r["global_entries_max_per_row"] = int(torch.bincount(garg[garg >= 0].long().flatten()).max())
            r["local_winners"] = int((saved_arg(case.local_fwd()) >= 0).sum())
        rows.append(r)
    print("%-16s %3s %2s | %-8s | %10s %10s | %10s %10s | %s" % ("embedding", "ids", "k", "route", "global fwd", "global f+b", "local fwd",
                                                                "local f+b", "(us)  entries (max per bank row) / winners"))
    for r in rows:
        for route in routes:
            print("%-16s %3d %2d | %-8s | %10.1f %10.1f | %10s %10s | %d (%d) / %d" % (
                tuple(r["shape"]), r["n_ids"], r["k"], route, r[route + "_global_fwd_us"], r[route + "_global_fwd_bwd_us"],
                r.get(route + "_local_fwd_us", "-"), r.get(route + "_local_fwd_bwd_us", "-"), r["global_entries"],
                r["global_entries_max_per_row"], r["local_winners"]))
    res = {"device": torch.cuda.get_device_name(0), "match_train": rows}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
