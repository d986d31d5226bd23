#!/usr/bin/env python3
"""The rest of a head block in training: the framework's 1x1 convolution (F.conv2d + autograd) and BatchNorm + ReLU
(nn.BatchNorm2d in train() mode + ReLU + autograd) against the HIP kernels of csrc/pw_train.hip, per pass, and one whole
DynamicSegHead forward + backward in train() mode for train_kernels False, True, "all" and "fused".  HIP events, warm-up, median
of repeats.  The 1x1 passes are reported as fractions of the fp32 matrix peak (157.3 TFLOP/s), the BN passes as GB/s of their
compulsory HBM traffic (forward: read x twice -- statistics, apply -- write out; backward: read x and dy twice, write dx), and
beside them the output layer fused with BatchNorm + ReLU (csrc/head_train.hip; forward: read z twice; backward: read z twice,
write grad_z).
usage: python tools/head_train_bench.py [--reps N] [--json FILE] [--step-only MODE --shape B,C,h,w [--frozen-input]]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cvpr2020_manet_amd import _lib  # noqa: E402
from cvpr2020_manet_amd.networks import IntVOS as M  # noqa: E402

SHAPES = [(3, 103, 104, 104), (3, 256, 104, 104), (3, 256, 120, 214), (6, 256, 104, 104)]
PEAK_F32 = 157.3e12


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


def pointwise(shape, reps):
    """a block's conv2 at this shape: Cin = C (103: layer 1), Cout = 256"""
    B, Cin, h, w = shape
    Cout, HW = 256, h * w
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(B, Cin, h, w, device="cuda")
    wt = torch.randn(Cout, Cin, 1, 1, device="cuda") / Cin ** 0.5
    b = torch.randn(Cout, device="cuda")
    go = torch.randn(B, Cout, h, w, device="cuda")
    out, gx = torch.empty_like(go), torch.empty_like(x)
    gw, gb = torch.empty_like(wt), torch.empty_like(b)
    n = ctypes.c_size_t(0)
    _lib.check(lib.manet_pw_forward_workspace_bytes(B, Cin, Cout, HW, ctypes.byref(n)), "ws")
    wsf = torch.empty(max(n.value, 1), dtype=torch.uint8, device="cuda")
    _lib.check(lib.manet_pw_backward_weight_workspace_bytes(B, Cin, Cout, HW, ctypes.byref(n)), "ws")
    wsw = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    r = {"shape": [B, Cin, Cout, h, w]}
    r["hip_fwd_us"] = timed(lambda: lib.manet_pw_forward_f32(x.data_ptr(), B, Cin, Cout, HW, wt.data_ptr(), b.data_ptr(), out.data_ptr(),
                                                             wsf.data_ptr(), wsf.numel(), st), reps)
    r["hip_bwd_data_us"] = timed(lambda: lib.manet_pw_backward_data_f32(go.data_ptr(), B, Cin, Cout, HW, wt.data_ptr(), gx.data_ptr(),
                                                                        st), reps)
    r["hip_bwd_weight_us"] = timed(lambda: lib.manet_pw_backward_weight_f32(x.data_ptr(), go.data_ptr(), B, Cin, Cout, HW, gw.data_ptr(),
                                                                            gb.data_ptr(), wsw.data_ptr(), wsw.numel(), st), reps)
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    with torch.no_grad():
        r["fw_fwd_us"] = timed(lambda: F.conv2d(x, wt, b), reps)
    y = F.conv2d(xr, wr, br)
    r["fw_bwd_data_us"] = timed(lambda: torch.autograd.grad(y, [xr], go, retain_graph=True), reps)
    r["fw_bwd_weight_us"] = timed(lambda: torch.autograd.grad(y, [wr, br], go, retain_graph=True), reps)
    flop = 2.0 * B * HW * Cin * Cout
    for k in ("fwd", "bwd_data", "bwd_weight"):
        r["hip_%s_peak" % k] = round(flop / (r["hip_%s_us" % k] * 1e-6) / PEAK_F32, 3)
        r["fw_%s_peak" % k] = round(flop / (r["fw_%s_us" % k] * 1e-6) / PEAK_F32, 3)
    for k in list(r):
        if k.endswith("_us"):
            r[k] = round(r[k], 1)
    return r


def bn_relu(shape, reps):
    B, C, h, w = shape
    HW = h * w
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    bn = torch.nn.BatchNorm2d(C, momentum=0.0003).cuda().train()
    x = torch.randn(shape, device="cuda")
    go = torch.randn(shape, device="cuda")
    out, gx = torch.empty_like(x), torch.empty_like(x)
    save = torch.empty(2, C, device="cuda")
    gg, gbe = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    n = ctypes.c_size_t(0)
    _lib.check(lib.manet_bn_relu_workspace_bytes(B, C, HW, ctypes.byref(n)), "ws")
    ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    f = ctypes.c_float
    r = {"shape": list(shape)}
    r["hip_fwd_us"] = timed(lambda: lib.manet_bn_relu_forward_f32(
        x.data_ptr(), B, C, HW, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
        f(bn.momentum), f(bn.eps), 1, out.data_ptr(), save[0].data_ptr(), save[1].data_ptr(), ws.data_ptr(), ws.numel(), st), reps)
    r["hip_bwd_us"] = timed(lambda: lib.manet_bn_relu_backward_f32(
        go.data_ptr(), x.data_ptr(), B, C, HW, bn.weight.data_ptr(), bn.bias.data_ptr(), save[0].data_ptr(), save[1].data_ptr(), 1,
        gx.data_ptr(), gg.data_ptr(), gbe.data_ptr(), ws.data_ptr(), ws.numel(), st), reps)
    ref = torch.nn.BatchNorm2d(C, momentum=0.0003).cuda().train()
    with torch.no_grad():
        r["fw_fwd_us"] = timed(lambda: torch.relu(ref(x)), reps)
    xr = x.clone().requires_grad_(True)
    y = torch.relu(ref(xr))
    r["fw_bwd_us"] = timed(lambda: torch.autograd.grad(y, [xr, ref.weight, ref.bias], go, retain_graph=True), reps)
    act = x.numel() * 4
    for k, passes in (("fwd", 3), ("bwd", 5)):
        r["hip_%s_GBps" % k] = round(passes * act / (r["hip_%s_us" % k] * 1e-6) / 1e9, 1)
        r["fw_%s_GBps" % k] = round(passes * act / (r["fw_%s_us" % k] * 1e-6) / 1e9, 1)
    # the same BatchNorm + ReLU with the head's output layer behind it
    wt, b1 = torch.randn(C, device="cuda") / C ** 0.5, torch.randn(1, device="cuda")
    gl, logits = torch.randn(B, HW, device="cuda"), torch.empty(B, HW, device="cuda")
    gwt, gb1 = torch.empty_like(wt), torch.empty_like(b1)
    _lib.check(lib.manet_out_conv_workspace_bytes(B, C, HW, ctypes.byref(n)), "ws")
    wso = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    r["outconv_fwd_us"] = timed(lambda: lib.manet_bn_relu_outconv_forward_f32(
        x.data_ptr(), B, C, HW, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
        f(bn.momentum), f(bn.eps), 1, wt.data_ptr(), b1.data_ptr(), logits.data_ptr(), save[0].data_ptr(), save[1].data_ptr(),
        wso.data_ptr(), wso.numel(), st), reps)
    r["outconv_bwd_us"] = timed(lambda: lib.manet_bn_relu_outconv_backward_f32(
        gl.data_ptr(), x.data_ptr(), B, C, HW, bn.weight.data_ptr(), bn.bias.data_ptr(), save[0].data_ptr(), save[1].data_ptr(), 1,
        wt.data_ptr(), gx.data_ptr(), gwt.data_ptr(), gb1.data_ptr(), gg.data_ptr(), gbe.data_ptr(), wso.data_ptr(), wso.numel(),
        st), reps)
    for k, passes in (("fwd", 2), ("bwd", 3)):
        r["outconv_%s_GBps" % k] = round(passes * act / (r["outconv_%s_us" % k] * 1e-6) / 1e9, 1)
    for k in list(r):
        if k.endswith("_us"):
            r[k] = round(r[k], 1)
    return r


def _head(mode, C):
    torch.manual_seed(0)
    return M.DynamicSegHead(in_dim=C, train_kernels=mode).cuda().train()


def head_step(shape, reps):
    """DynamicSegHead(in_dim=C) forward + backward in train() mode, for train_kernels False / True / "all" / "fused" (same
    parameters)"""
    B, C, h, w = shape
    x = torch.randn(shape, device="cuda", requires_grad=True)
    r = {"shape": list(shape)}
    for name, mode in (("framework", False), ("hip_dw", True), ("hip_all", "all"), ("hip_fused", "fused")):
        head = _head(mode, C)

        def step():
            head.zero_grad(set_to_none=True)
            head(x).sum().backward()
        r[name + "_us"] = round(timed(step, reps), 1)
    r["all_vs_dw"] = round(r["hip_dw_us"] / r["hip_all_us"], 2)
    r["fused_vs_all"] = round(r["hip_all_us"] / r["hip_fused_us"], 2)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step-only", default=None, help="False | True | all | fused: only run that head step (for a profiler)")
    ap.add_argument("--shape", default="3,256,104,104")
    ap.add_argument("--frozen-input", action="store_true", help="--step-only: x does not require grad (the reference's stage 2)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if a.step_only is not None:
        shape = tuple(int(v) for v in a.shape.split(","))
        mode = {"false": False, "true": True}.get(a.step_only.lower(), a.step_only)
        head = _head(mode, shape[1])
        x = torch.randn(shape, device="cuda", requires_grad=not a.frozen_input)

        def step():
            head.zero_grad(set_to_none=True)
            head(x).sum().backward()
        gpu_us = timed(step, a.reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):  # host time per step: the launches queue ahead unless the host is the bound
            step()
        host_us = (time.perf_counter() - t0) / a.reps * 1e6
        torch.cuda.synchronize()
        print("DynamicSegHead train step %s train_kernels=%r: %.1f us (events), host %.1f us per step" % (shape, mode, gpu_us, host_us))
        return
    pw = [pointwise(s, a.reps) for s in SHAPES]
    bn = [bn_relu(s, a.reps) for s in SHAPES]
    heads = [head_step((3, 103, 104, 104), max(5, a.reps // 3)), head_step((3, 256, 104, 104), max(5, a.reps // 3))]
    print("1x1 %-24s | %8s %8s %8s | %8s %8s %8s   (us; fraction of the fp32 matrix peak of the HIP pass)" % (
        "[B,Cin,Cout,h,w]", "fw fwd", "fw bdata", "fw bw", "hip fwd", "hip bdat", "hip bw"))
    for r in pw:
        print("    %-24s | %8.1f %8.1f %8.1f | %8.1f %8.1f %8.1f   (%.2f / %.2f / %.2f)" % (
            str(tuple(r["shape"])), r["fw_fwd_us"], r["fw_bwd_data_us"], r["fw_bwd_weight_us"], r["hip_fwd_us"],
            r["hip_bwd_data_us"], r["hip_bwd_weight_us"], r["hip_fwd_peak"], r["hip_bwd_data_peak"], r["hip_bwd_weight_peak"]))
    print("BN+ReLU %-20s | %8s %8s | %8s %8s   (us; GB/s of the HIP pass) | %8s %8s   (BN + ReLU + output conv: us; GB/s)" % (
        "[B,C,h,w]", "fw fwd", "fw bwd", "hip fwd", "hip bwd", "oc fwd", "oc bwd"))
    for r in bn:
        print("        %-20s | %8.1f %8.1f | %8.1f %8.1f   (%.0f / %.0f) | %8.1f %8.1f   (%.0f / %.0f)" % (
            str(tuple(r["shape"])), r["fw_fwd_us"], r["fw_bwd_us"], r["hip_fwd_us"], r["hip_bwd_us"], r["hip_fwd_GBps"],
            r["hip_bwd_GBps"], r["outconv_fwd_us"], r["outconv_bwd_us"], r["outconv_fwd_GBps"], r["outconv_bwd_GBps"]))
    for r in heads:
        print("DynamicSegHead train step %s: framework %.1f us, HIP depthwise %.1f us, HIP all %.1f us (%.2fx over depthwise), "
              "HIP fused %.1f us (%.2fx over all)" % (tuple(r["shape"]), r["framework_us"], r["hip_dw_us"], r["hip_all_us"],
                                                       r["all_vs_dw"], r["hip_fused_us"], r["fused_vs_all"]))
    res = {"device": torch.cuda.get_device_name(0), "pointwise": pw, "bn_relu": bn, "head_step": heads}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
