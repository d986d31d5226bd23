"""The training criterion behind the segmentation head (reference networks/loss.py:44-81), on the fused HIP op.

`Added_CrossEntropyLoss(top_k_percent_pixels, hard_example_mining_step)` is called as the reference's is -- criterion(dic_tmp, y, step)
with {sequence: logits [B, C, H, W]} and {sequence: labels [B, H, W]} -- so train_stage1.py:74 needs only its import swapped.  For fp32
logits with at most 64 channels and int64 / int32 / uint8 labels on a HIP device every sequence's term is ONE op,
ops.upsampled_cross_entropy_topk (csrc/loss_train.hip: cross-entropy with ignore_index=255, exact selection of the k hardest pixels,
mean; deterministic forward and backward).  The extra keyword `size=(H, W)` takes the head's own low-resolution logits and folds the
caller's F.interpolate(..., mode='bilinear', align_corners=True) (train_stage1.py:133) into the same op, which then never writes the
upsampled logits.  Anything else (CPU tensors, other dtypes, more channels) runs the stock composition of framework ops."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


class Added_CrossEntropyLoss(nn.Module):
    """Cross-entropy over the hardest pixels.  top_k_percent_pixels = None: the mean over every pixel whose label is not 255.
    Otherwise the mean of the k largest per-pixel losses of each row, with k annealed from every pixel at step 0 to
    top_k_percent_pixels of them at hard_example_mining_step (0: no annealing)."""

    def __init__(self, top_k_percent_pixels=None, hard_example_mining_step=100000):
        super().__init__()
        if top_k_percent_pixels is not None:
            assert 0 < top_k_percent_pixels < 1
        self.top_k_percent_pixels = top_k_percent_pixels
        self.hard_example_mining_step = hard_example_mining_step

    def top_k_pixels(self, num_pixels, step):
        """the number of pixels kept at `step` out of `num_pixels` (None: all of them, averaged over the labelled ones)"""
        if self.top_k_percent_pixels is None:
            return None
        num_pixels = float(num_pixels)
        if self.hard_example_mining_step == 0:
            return int(self.top_k_percent_pixels * num_pixels)
        ratio = min(1.0, step / float(self.hard_example_mining_step))
        return int((ratio * self.top_k_percent_pixels + (1.0 - ratio)) * num_pixels)

    def _stock(self, logits, labels, k, size):
        if size is not None and tuple(logits.shape[2:]) != size:
            logits = F.interpolate(logits, size=size, mode="bilinear", align_corners=True)
        if k is None:
            return F.cross_entropy(logits, labels, ignore_index=255, reduction="mean")
        pixel_losses = F.cross_entropy(logits.view(-1, logits.size(1), logits.size(2) * logits.size(3)),
                                       labels.view(-1, labels.size(1) * labels.size(2)), ignore_index=255, reduction="none")
        return torch.mean(torch.topk(pixel_losses, k=k, dim=1)[0])

    def _one(self, logits, labels, step, size):
        H, W = size if size is not None else (logits.size(2), logits.size(3))
        k = self.top_k_pixels(H * W, step)
        if not ops.upsampled_cross_entropy_ok(logits, labels, (H, W)) or (k is not None and k < 1):
            return self._stock(logits, labels, k, size)
        if k is None:  # every pixel, averaged over the labelled ones: the count stays on the device
            total = ops.upsampled_cross_entropy_topk(logits, labels, (H, W), H * W, divisor=1.0)
            return total / (labels != 255).sum().to(torch.float32)
        return ops.upsampled_cross_entropy_topk(logits, labels, (H, W), k)

    def forward(self, dic_tmp, y, step, size=None):
        if size is not None:
            size = (int(size[0]), int(size[1]))
        final_loss = 0
        for seq_name in dic_tmp.keys():
            final_loss = final_loss + self._one(dic_tmp[seq_name], y[seq_name], step, size)
        return final_loss
