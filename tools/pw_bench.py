#!/usr/bin/env python3
"""Times ops.conv1x1_mfma at [3,256,120,214] (and layer 1's shared K=100) against the framework's GEMM.
python3 tools/pw_bench.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cvpr2020_manet_amd import ops  # noqa: E402


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


torch.manual_seed(0)
if "--dw" in sys.argv:  # the depthwise kernel
    with torch.no_grad():
        x = torch.randn(3, 256, 120, 214, device="cuda")
        wt = torch.randn(256, 1, 7, 7, device="cuda")
        sc, sh = torch.rand(256, device="cuda") + 0.5, torch.randn(256, device="cuda")
        t = timeit(lambda: ops.dwconv7x7_bn_relu(x, wt, None, scale=sc, shift=sh, relu_in=True))
        print("depthwise [3,256,120,214]: %.1f us (%.2f TB/s over in + out)" % (t, 2 * x.numel() * 4 / t / 1e6))
    sys.exit(0)
with torch.no_grad():
    for (B, cin) in ((3, 256), (2, 256), (1, 100), (3, 3)):
        x = torch.randn(B, cin, 120, 214, device="cuda")
        w2t = torch.randn(cin, 256, device="cuda") * 0.05
        b2 = torch.randn(256, device="cuda")
        w2 = w2t.t().reshape(256, cin, 1, 1).contiguous()
        t_m = timeit(lambda: ops.conv1x1_mfma(x, w2t, b2))  # (any Cin since r4)
        sw = ops.SplitWeight(w2t)
        t_s = timeit(lambda: ops.conv1x1_split(x, sw, b2))
        ref = ops.conv1x1_mfma(x, w2t, b2)
        got = ops.conv1x1_split(x, sw, b2)
        rd = torch.nn.functional.conv2d(x.double(), w2.double(), b2.double())
        print("  split-bf16 kernel %.1f us (%.2f TB/s over in + out); max |split - f64| %.3g, max |fp32 MFMA - f64| %.3g, "
              "max |framework - f64| %.3g  (|y| max %.3g)"
              % (t_s, (x.numel() + ref.numel()) * 4 / t_s / 1e6, (got.double() - rd).abs().max().item(),
                 (ref.double() - rd).abs().max().item(),
                 (torch.nn.functional.conv2d(x, w2, b2).double() - rd).abs().max().item(), rd.abs().max().item()))
        t_f = timeit(lambda: torch.nn.functional.conv2d(x, w2, b2))
        fl = 2.0 * B * 120 * 214 * cin * 256
        print("B=%d Cin=%d: MFMA kernel %.1f us (%.1f TFLOP/s = %.2f of the fp32 matrix peak), framework %.1f us"
              % (B, cin, t_m, fl / t_m / 1e6, fl / t_m / 1e6 / 157.3, t_f))
