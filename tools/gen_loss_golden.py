#!/usr/bin/env python3
"""Writes tests/golden/loss_*.npz: small cases of the reference's training loss (its networks/loss.py Added_CrossEntropyLoss behind
F.interpolate(bilinear, align_corners=True), train_stage1.py:126-153) run on the CPU in fp32 as the reference runs it -- inputs,
loss, d logits, k -- plus the float64 per-pixel losses.  Data only: the reference's module is imported from the checkout given on
the command line and nothing of it is stored.

A case is refused when the float64 gap between the k-th and the (k+1)-th largest pixel loss of a row is under 10x the per-pixel
error bound of the fused op (16 ulp at the largest |logit|): the reference's own fp32 selection would then depend on rounding.
Seeds are searched from the one given until a case passes.
usage: python tools/gen_loss_golden.py --reference /path/to/CVPR2020_MANet [--out tests/golden]"""
import argparse
import importlib.util
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (logits shape, (H, W), top_k_percent_pixels, hard_example_mining_step, step, first seed)
CASES = {
    "loss_up4": ((1, 3, 24, 24), (96, 96), 0.15, 100000, 50000, 0),
    "loss_wide": ((1, 5, 15, 27), (60, 107), 0.15, 100000, 100000, 100),
    "loss_rows": ((2, 2, 13, 17), (50, 66), 0.15, 100000, 20000, 200),
    "loss_same": ((1, 4, 32, 48), (32, 48), 0.15, 100000, 50000, 300),
    "loss_mean": ((1, 3, 24, 24), (96, 96), None, 100000, 50000, 400),
}


def pixel_bound(max_abs_logit):
    """16 ulp at the largest |logit|: 4 fused taps, one log-sum-exp and one subtraction, each a few ulp at that magnitude"""
    return 16.0 * 2.0 ** -23 * 2.0 ** math.ceil(math.log2(max_abs_logit))


def inputs(shape, size, seed):
    g = torch.Generator().manual_seed(seed)
    B, C, _, _ = shape
    logits = torch.randn(shape, generator=g) * 3
    labels = torch.randint(0, C, (B,) + tuple(size), generator=g)
    labels[torch.rand((B,) + tuple(size), generator=g) < 0.05] = 255
    labels[:, : size[0] // 8, : size[1] // 5] = 255  # and a block of them, as a void border is
    return logits, labels


def pixels64(logits, labels, size):
    up = F.interpolate(logits.double(), size=size, mode="bilinear", align_corners=True)
    return F.cross_entropy(up, labels, ignore_index=255, reduction="none").reshape(logits.shape[0], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (its networks/loss.py is imported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(a.reference, "networks", "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    for name, (shape, size, pct, mining, step, seed0) in CASES.items():
        for seed in range(seed0, seed0 + 100):
            logits, labels = inputs(shape, size, seed)
            pix = pixels64(logits, labels, size)
            n = size[0] * size[1]
            crit = ref.Added_CrossEntropyLoss(pct, mining)
            if pct is None:
                k, gap = n, float("inf")
            else:
                k = int((min(1.0, step / float(mining)) * pct + (1.0 - min(1.0, step / float(mining)))) * float(n))
                assert k < n
                s = torch.sort(pix, dim=1, descending=True)[0]
                gap = float((s[:, k - 1] - s[:, k]).min())
            bound = pixel_bound(float(logits.abs().max()))
            if gap >= 10 * bound:
                break
            print("%s: seed %d refused, gap %.3g < 10 x %.3g" % (name, seed, gap, bound))
        else:
            raise SystemExit("%s: no seed with a wide enough gap" % name)
        x = logits.clone().requires_grad_(True)
        up = F.interpolate(x, size=size, mode="bilinear", align_corners=True)  # train_stage1.py:133
        loss = crit({"seq": up}, {"seq": labels}, step)
        loss.backward()
        path = os.path.join(a.out, name + ".npz")
        np.savez_compressed(path, logits=logits.numpy(), labels=labels.numpy().astype(np.uint8), size=np.array(size, dtype=np.int64),
                            top_k_percent_pixels=np.array(-1.0 if pct is None else pct), hard_example_mining_step=np.array(mining),
                            step=np.array(step), k=np.array(k), seed=np.array(seed), gap64=np.array(gap),
                            loss=loss.detach().numpy(), dlogits=x.grad.numpy(), pixel_losses64=pix.numpy())
        print("%s: seed %d k %d / %d gap %.3g (bound %.3g) loss %.6f -> %s, %d bytes" % (
            name, seed, k, n, gap, bound, float(loss.detach()), path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
