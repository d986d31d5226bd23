"""torch.autograd.Function wrappers of the matching path's training entry points.

The reference's matching functions are plain PyTorch, so autograd differentiates them for free and
train_stage1.py:126-156 / train_stage2.py back-propagate through IntVOS.forward.  The HIP path takes raw
pointers, so the backward is explicit:

  GlobalMatchFn   nearest_neighbor_features_per_object, k = 1 (reference IntVOS.py:160-210): torch.min sends the
                  gradient to ONE bank row per (query pixel, object) -- the forward kernel records it
                  (manet_global_match_arg_f32), the backward is a gather / scatter-add
                  (manet_global_match_backward_f32).
  GlobalMatchTopkFn  the same with k > 1 (IntVOS.py:87-94): k exact arg-min passes, a gather / scatter-add per rank.
  LocalMatchFn    local_previous_frame_nearest_neighbor_features_per_object, downsample on (:345-434): the
                  forward records the winning window offset and keeps the normalised pooled volume; the
                  backward walks min -> where -> bilinear -> sigmoid -> (x - y)^2 -> avg_pool2d in reverse.
  LocalMatchFullFn  the same with MODEL_LOCAL_DOWNSAMPLE = False (:299-313): raw full-resolution distances, no sigmoid / bilinear.
  CorrelationFn   correlation_package (correlation.py:7-45): forward + manet_correlation_backward_f32.
  DepthwiseConvFn  the heads' depthwise layers (IntVOS.py:491-493, :537) in training: forward, backward-data and
                  deterministic backward-weight kernels (csrc/dwconv_train.hip); ops.depthwise_conv2d, IntVOS(train_kernels=True).
  PointwiseConvFn  the heads' 1x1 convolutions in training: forward, backward-data and deterministic backward-weight kernels
                  (csrc/pw_train.hip); ops.pointwise_conv2d, IntVOS(train_kernels="all").
  BatchNormReluFn  the heads' BatchNorm + ReLU pairs in training (or eval with grad enabled): statistics, running buffers and
                  the backward on csrc/pw_train.hip's kernels; ops.batch_norm_relu, IntVOS(train_kernels="all").
  OutputConvFn     DynamicSegHead's output conv (IntVOS.py:516,524) in training: forward and a deterministic backward
                  (csrc/head_train.hip); ops.output_conv1x1.
  DynamicSegHeadFn  a whole DynamicSegHead's training step as one node: the existing depthwise, BatchNorm + ReLU and 1x1
                  launchers sequenced in C, the output conv fused with the BatchNorm + ReLU in front of it
                  (csrc/head_train.hip); ops.dynamic_seghead_train, IntVOS(train_kernels="fused").
  HeadInputFn      the heads' input in training (IntVOS.py:663-671, :741-758: repeat, permutes, the label compare, the cats and
                  the global map's normalisation) as one node (csrc/head_input_train.hip); ops.head_input_train,
                  IntVOS(train_inputs="fused").
  DynamicSegHeadPartsFn  HeadInputFn and DynamicSegHeadFn as one node: maps -> logits; ops.dynamic_seghead_train_parts.
  UpsampledCrossEntropyTopKFn  the loss behind the head (train_stage1.py:126-153, networks/loss.py:44-81): bilinear upsample,
                  cross-entropy, hard-pixel top-k and mean as one op, deterministic forward and backward (csrc/loss_train.hip);
                  ops.upsampled_cross_entropy_topk, networks.loss.Added_CrossEntropyLoss.

  GlobalMatchOrderedFn, GlobalMatchTopkOrderedFn, LocalMatchOrderedFn, LocalMatchFullOrderedFn  the ordered training route of
                  the four matching nodes above (csrc/match_train.hip; ops.global_match / ops.local_match(deterministic=True),
                  IntVOS(train_match="ordered")): the same forward values and selections, a backward without float atomics --
                  every sum has one owner and a fixed order, so the gradients are the same bits on every run; all k ranks of the
                  top-k backward in one call; a frozen operand gets None and costs nothing.

`ops.global_match` / `ops.local_match` / `ops.correlation_forward` route here when grad mode is on and an
embedding requires grad; normalisation and the min-merge with the stored map stay ordinary torch ops on the
result (they are element-wise and torch differentiates them).  fp32 only; anything else raises.
"""
import ctypes

import torch

from . import _lib, ops
from .ops import _bank_strides, _on, _optional, _ptr, _stream_ptr, _strided, _workspace, _ws_bytes


def _scratch(device, nbytes):
    return torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)


def _dense(t):
    """non-overlapping and dense (a permuted contiguous tensor): a new buffer can mirror its layout"""
    if t.numel() == 0:
        return False
    sizes_strides = sorted(zip(t.stride(), t.shape))
    expect = 1
    for st, sz in sizes_strides:
        if sz == 1:
            continue
        if st != expect:
            return False
        expect *= sz
    return True


def _grad_like(t, needed=True):
    """a float32 gradient buffer in `t`'s own memory order (C-major embeddings stay C-major) if `t` is dense, contiguous
    otherwise; None when the gradient is not `needed` (the frozen reference frame of fine-tuning: neither zero-filled nor
    scattered into)"""
    if not needed:
        return None
    if _dense(t):
        return torch.empty_strided(t.shape, t.stride(), dtype=torch.float32, device=t.device)
    return torch.empty(t.shape, dtype=torch.float32, device=t.device)


def _global_arg_forward(bytes_query, symbol, ref, qry, labels, n_ids, ranks=()):
    """the arg-min forward kernels -> (distances, winning bank rows), each [*ranks, N, n_ids]"""
    M0, C = ref.shape
    N = qry.shape[0]
    dev = qry.device
    ws = _scratch(dev, _lib.query(bytes_query, N, M0, C, n_ids))
    d = torch.empty((*ranks, N, n_ids), dtype=torch.float32, device=dev)
    arg = torch.empty((*ranks, N, n_ids), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.call(symbol, *_strided(qry), ref.data_ptr(), *_bank_strides(ref), labels.data_ptr(), N, M0, C, n_ids, *ranks,
                  d.data_ptr(), arg.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev))
    return d, arg


def _global_backward_call(ref, qry, arg, g, n_ids, gq, gr, ranks=None):
    """the gather / scatter-add of `g` through the recorded rows `arg` into gq / gr (None: not wanted).  ranks None: the atomic
    route, one rank (manet_global_match_backward_f32); else arg / g are [ranks, N, n_ids] and the route is the ordered one."""
    M0, C = ref.shape
    N = qry.shape[0]
    dev = qry.device
    operands = (*_strided(qry), ref.data_ptr(), *_bank_strides(ref), arg.data_ptr(), g.data_ptr(), N, M0, C, n_ids)
    grads = _optional(gq, C, 1) + (_optional(gr, C, 1) if M0 > 0 else (_ptr(gr), C, 1))
    with _on(dev):
        if ranks is None:
            _lib.call("manet_global_match_backward_f32", *operands, *grads, _stream_ptr(dev))
        else:
            ws = _workspace(dev, "global_backward_ordered",
                            _ws_bytes("manet_global_match_backward_ordered_workspace_bytes", N, M0, C, n_ids, ranks))
            _lib.call("manet_global_match_backward_ordered_f32", *operands, ranks, *grads, ws.data_ptr(), ws.numel(),
                      _stream_ptr(dev))


def _global_backward(ctx, arg, g, ranks):
    """_global_backward_call into gradients laid out like the inputs -> (grad_ref, grad_qry), None where not needed"""
    ref, qry = ctx.saved_tensors[:2]
    gr, gq = _grad_like(ref, ctx.needs_input_grad[0]), _grad_like(qry, ctx.needs_input_grad[1])
    if gr is not None or gq is not None:
        _global_backward_call(ref, qry, arg, g, ctx.n_ids, gq, gr, ranks)
    return gr, gq


class GlobalMatchFn(torch.autograd.Function):
    """out [N, n_ids] raw distances; differentiable w.r.t. reference [M0, C] and query [N, C] (any strides)."""

    @staticmethod
    def forward(ctx, ref, qry, labels, n_ids):
        out, arg = _global_arg_forward("manet_global_match_arg_workspace_bytes", "manet_global_match_arg_f32", ref, qry, labels,
                                       n_ids)
        ctx.save_for_backward(ref, qry, arg)
        ctx.n_ids = n_ids
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        return (*_global_backward(ctx, ctx.saved_tensors[2], grad_out.contiguous().float(), None), None, None)


class GlobalMatchTopkFn(torch.autograd.Function):
    """nearest_neighbor_features_per_object with k_nearest_neighbors > 1 (reference IntVOS.py:87-94): out [N, n_ids] =
    mean of the k smallest distances per (query, object), entries past the object's row count replaced by the farthest real
    neighbour.  The reference gets the gradient from autograd through topk -> where -> max -> mean: each real neighbour of rank
    j receives g / k, and the farthest real one additionally the share of every replaced entry ((k - v) g / k with v real
    neighbours; nothing at all when the object has no row: `dists * valid` multiplies the padding by zero).  Forward:
    manet_global_match_topk_arg_f32 (k exact passes of the arg-min kernel); backward: one gather / scatter-add launch per rank."""

    @staticmethod
    def forward(ctx, ref, qry, labels, n_ids, k):
        d, arg = _global_arg_forward("manet_global_match_topk_arg_workspace_bytes", "manet_global_match_topk_arg_f32", ref, qry,
                                     labels, n_ids, (k,))
        # IntVOS.py:88-94 on the k sorted distances (rank along dim 0)
        valid = d < 1e20
        masked = d * valid.float()
        pad, jstar = masked.max(dim=0, keepdim=True)
        out = torch.where(valid, d, pad.expand_as(d)).mean(dim=0)
        # per-rank weights of the incoming gradient: 1/k for a real neighbour, + (k - v)/k on the rank the padding came from
        # (times that rank's own validity: with no real neighbour the padding is 0 * d -- no gradient)
        nvalid = valid.sum(dim=0, keepdim=True)
        wgt = valid.float() / k
        extra = (k - nvalid).float() / k
        wgt.scatter_add_(0, jstar, extra * torch.gather(valid.float(), 0, jstar))
        arg = torch.where(valid, arg, torch.full_like(arg, -1))
        ctx.save_for_backward(ref, qry, arg, wgt)
        ctx.n_ids, ctx.k = n_ids, k
        return out

    @staticmethod
    def backward(ctx, grad_out):
        ref, qry, arg, wgt = ctx.saved_tensors
        need_ref, need_qry = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_ref or need_qry):
            return None, None, None, None, None
        g = grad_out.contiguous().float()
        gq_sum = gr_sum = None
        for j in range(ctx.k):  # per-rank gradients in the inputs' own memory order (as for k = 1), summed with torch
            gj = (g * wgt[j]).contiguous()
            gq, gr = _grad_like(qry, need_qry), _grad_like(ref, need_ref)
            _global_backward_call(ref, qry, arg[j], gj, ctx.n_ids, gq, gr)
            if need_qry:
                gq_sum = gq if gq_sum is None else gq_sum.add_(gq)
            if need_ref:
                gr_sum = gr if gr_sum is None else gr_sum.add_(gr)
        return gr_sum, gq_sum, None, None, None


class GlobalMatchOrderedFn(GlobalMatchFn):
    """GlobalMatchFn with the ordered backward (manet_global_match_backward_ordered_f32, ranks = 1): no float atomics, each bank
    row's gradient added by one owner in ascending (query, object) order -- the same bits on every run."""

    @staticmethod
    def backward(ctx, grad_out, _grad_arg):
        return (*_global_backward(ctx, ctx.saved_tensors[2], grad_out.contiguous().float(), 1), None, None)


class GlobalMatchTopkOrderedFn(GlobalMatchTopkFn):
    """GlobalMatchTopkFn with the ordered backward: the k ranks' rows and weighted gradients go to ONE call of
    manet_global_match_backward_ordered_f32 (the atomic route launches once per rank and sums with torch)."""

    @staticmethod
    def backward(ctx, grad_out):
        arg, wgt = ctx.saved_tensors[2:]
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None, None
        gw = (grad_out.float().unsqueeze(0) * wgt).contiguous()
        return (*_global_backward(ctx, arg.contiguous(), gw, ctx.k), None, None, None)


def _local_forward(ctx, ordered, prev, cur, labels, n_ids, max_distance):
    """LocalMatchFn / LocalMatchOrderedFn.forward: the same out / arg / volume bits from either symbol; the atomic route sizes a
    fresh scratch tensor per call, the ordered one uses the workspace cache"""
    h, w, C = cur.shape
    dev = cur.device
    P = 2 * max_distance + 1
    out = torch.empty((h, w, n_ids), dtype=torch.float32, device=dev)
    arg = torch.empty((h, w, n_ids), dtype=torch.int32, device=dev)
    vol = torch.empty((P * P, h // 2, w // 2), dtype=torch.float32, device=dev)
    with _on(dev):
        if ordered:
            ws = _workspace(dev, "local_train", _ws_bytes("manet_local_match_arg_workspace_bytes", h, w, C, max_distance))
        else:
            ws = _scratch(dev, _lib.query("manet_local_match_arg_workspace_bytes", h, w, C, max_distance))
        _lib.call("manet_local_match_train_forward_f32" if ordered else "manet_local_match_arg_f32", *_strided(prev),
                  *_strided(cur), labels.data_ptr(), h, w, C, n_ids, max_distance, out.data_ptr(), arg.data_ptr(), vol.data_ptr(),
                  ws.data_ptr(), ws.numel(), _stream_ptr(dev))
    ctx.save_for_backward(prev, cur, vol, arg)
    ctx.n_ids, ctx.max_distance = n_ids, max_distance
    return out


def _local_backward(ctx, ordered, grad_out):
    """LocalMatchFn / LocalMatchOrderedFn.backward.  The atomic route computes both gradients, wanted or not; on the ordered one
    a frozen frame gets None (a null pointer with zero strides) and no work."""
    prev, cur, vol, arg = ctx.saved_tensors
    need_prev, need_cur = ctx.needs_input_grad[:2] if ordered else (True, True)
    if not (need_prev or need_cur):
        return None, None, None, None, None
    h, w, C = cur.shape
    dev = cur.device
    g = grad_out.contiguous().float()
    gp, gc = _grad_like(prev, need_prev), _grad_like(cur, need_cur)
    with _on(dev):
        if ordered:
            ws = _workspace(dev, "local_train_backward",
                            _ws_bytes("manet_local_match_train_workspace_bytes", h, w, C, ctx.n_ids, ctx.max_distance))
        else:
            ws = _scratch(dev, _lib.query("manet_local_match_backward_workspace_bytes", h, w, C, ctx.max_distance))
        _lib.call("manet_local_match_train_backward_f32" if ordered else "manet_local_match_backward_f32", *_strided(prev),
                  *_strided(cur), vol.data_ptr(), arg.data_ptr(), g.data_ptr(), h, w, C, ctx.n_ids, ctx.max_distance,
                  *_optional(gp, 0, 0, 0), *_optional(gc, 0, 0, 0), ws.data_ptr(), ws.numel(), _stream_ptr(dev))
    return gp, gc, None, None, None


class LocalMatchFn(torch.autograd.Function):
    """out [h, w, n_ids]; differentiable w.r.t. prev and cur [h, w, C] (any strides); downsample configuration."""

    @staticmethod
    def forward(ctx, prev, cur, labels, n_ids, max_distance):
        return _local_forward(ctx, False, prev, cur, labels, n_ids, max_distance)

    @staticmethod
    def backward(ctx, grad_out):
        return _local_backward(ctx, False, grad_out)


class LocalMatchOrderedFn(LocalMatchFn):
    """LocalMatchFn's ordered route: forward manet_local_match_train_forward_f32 (the same out / arg / volume bits, the masked
    minimum spread over (2d+1) x 2 threads per pixel), backward manet_local_match_train_backward_f32 -- sparse, no float atomics,
    every pooled cell's gradient added by one owner in an order fixed by indices; a frozen frame gets None and no work."""

    @staticmethod
    def forward(ctx, prev, cur, labels, n_ids, max_distance):
        return _local_forward(ctx, True, prev, cur, labels, n_ids, max_distance)

    @staticmethod
    def backward(ctx, grad_out):
        return _local_backward(ctx, True, grad_out)


def _local_full_backward(ctx, ordered, grad_out):
    """LocalMatchFullFn / LocalMatchFullOrderedFn.backward; as in _local_backward, only the ordered route skips a frozen frame"""
    prev, cur, arg = ctx.saved_tensors
    need_prev, need_cur = ctx.needs_input_grad[:2] if ordered else (True, True)
    if not (need_prev or need_cur):
        return None, None, None, None, None
    h, w, C = cur.shape
    dev = cur.device
    P = 2 * ctx.max_distance + 1
    g = grad_out.contiguous().float()
    pc, cc = prev.permute(2, 0, 1).contiguous(), cur.permute(2, 0, 1).contiguous()  # (no copy for C-major embeddings)
    gp = torch.empty_like(pc) if need_prev else None
    gc = torch.empty_like(cc) if need_cur else None
    dv = torch.empty((P * P, h * w), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.call("manet_local_match_full_backward_ordered_f32" if ordered else "manet_local_match_full_backward_f32",
                  pc.data_ptr(), cc.data_ptr(), arg.data_ptr(), g.data_ptr(), h, w, C, ctx.n_ids, ctx.max_distance, _ptr(gp),
                  _ptr(gc), dv.data_ptr(), _stream_ptr(dev))
    return (None if gp is None else gp.permute(1, 2, 0)), (None if gc is None else gc.permute(1, 2, 0)), None, None, None


class LocalMatchFullFn(torch.autograd.Function):
    """out [h, w, n_ids] for MODEL_LOCAL_DOWNSAMPLE = False (reference IntVOS.py:299-313 + :398-432): raw full-resolution
    window distances, masked minimum against the constant 1.0; the gradient of the min flows to one window offset per (pixel,
    object) -- none where the constant wins -- and from there to x - y of the two embeddings."""

    @staticmethod
    def forward(ctx, prev, cur, labels, n_ids, max_distance):
        h, w, C = cur.shape
        dev = cur.device
        P = 2 * max_distance + 1
        out = torch.empty((h, w, n_ids), dtype=torch.float32, device=dev)
        arg = torch.empty((h, w, n_ids), dtype=torch.int32, device=dev)
        vol = torch.empty((h, w, P * P), dtype=torch.float32, device=dev)
        with _on(dev):
            _lib.call("manet_local_match_full_arg_f32", *_strided(prev), *_strided(cur), labels.data_ptr(), h, w, C, n_ids,
                      max_distance, out.data_ptr(), arg.data_ptr(), vol.data_ptr(), _stream_ptr(dev))
        ctx.save_for_backward(prev, cur, arg)
        ctx.n_ids, ctx.max_distance = n_ids, max_distance
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return _local_full_backward(ctx, False, grad_out)


class LocalMatchFullOrderedFn(LocalMatchFullFn):
    """LocalMatchFullFn (MODEL_LOCAL_DOWNSAMPLE = False) with the ordered backward: one owner per (offset, pixel) adds the
    pixel's objects in ascending order (manet_local_match_full_backward_ordered_f32); a frozen frame gets None."""

    @staticmethod
    def backward(ctx, grad_out):
        return _local_full_backward(ctx, True, grad_out)


class CorrelationFn(torch.autograd.Function):
    """correlation_package's CorrelationFunction (correlation.py:7-45) on the HIP kernels.  The output (and the gradients)
    have the inputs' dtype, as the reference's op (float / half / double: its dispatch, correlation_cuda_kernel.cu:495-541; the
    forward computes in that type exactly like the no-grad path).  The backward kernels are fp32 and fp64: half gradients are
    computed in fp32 and rounded once, double gradients in double."""

    @staticmethod
    def forward(ctx, input1, input2, pad_size, kernel_size, max_displacement, stride1, stride2):
        if input1.dtype != input2.dtype:
            raise RuntimeError("cvpr2020_manet_amd: correlation inputs must have the same dtype")
        a = input1.contiguous()
        b = input2.contiguous()
        ctx.save_for_backward(a, b)
        ctx.params = (pad_size, kernel_size, max_displacement, stride1, stride2)
        with torch.no_grad():
            return ops.correlation_forward(a, b, pad_size, kernel_size, max_displacement, stride1, stride2)

    @staticmethod
    def backward(ctx, grad_out):
        a0, b0 = ctx.saved_tensors
        wide = torch.float64 if a0.dtype == torch.float64 else torch.float32
        a, b = a0.to(wide), b0.to(wide)
        B, C, H, W = a.shape
        pad_size, kernel_size, max_displacement, stride1, stride2 = ctx.params
        g = grad_out.contiguous().to(wide)
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        with _on(a.device):
            _lib.call("manet_correlation_backward_f64" if wide == torch.float64 else "manet_correlation_backward_f32", a.data_ptr(),
                      b.data_ptr(), g.data_ptr(), B, C, H, W, pad_size, kernel_size, max_displacement, stride1, stride2,
                      ga.data_ptr(), gb.data_ptr(), _stream_ptr(a.device))
        return ga.to(a0.dtype), gb.to(b0.dtype), None, None, None, None, None


class DepthwiseConvFn(torch.autograd.Function):
    """Depthwise convolution of the heads in training (IntVOS.py:491-493 _split_separable_conv2d.conv1, :537 seperate_conv):
    F.conv2d(x, weight, bias, padding=K // 2, groups=C) with K = 3 or 7, stride 1, fp32 NCHW.  Forward
    manet_dwconv_forward_f32; backward manet_dwconv_backward_data_f32 (grad_x) and manet_dwconv_backward_weight_f32 (grad_weight
    and grad_bias, deterministic) -- each launched only when its gradient is asked for."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        wt = weight.contiguous()
        with torch.no_grad():
            out = ops._dwconv_forward(x, wt, bias)
        ctx.save_for_backward(x, wt)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, wt = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        B, C, h, w = x.shape
        K = wt.shape[-1]
        dev = x.device
        g = grad_out.contiguous().float()
        gx = gw = gb = None
        with _on(dev):
            if need_x:
                gx = torch.empty_like(x)
                _lib.call("manet_dwconv_backward_data_f32", g.data_ptr(), B, C, h, w, K, wt.data_ptr(), gx.data_ptr(),
                          _stream_ptr(dev))
            if need_w or need_b:
                ws = _scratch(dev, _lib.query("manet_dwconv_backward_weight_workspace_bytes", B, C, h, w, K))
                gw_full = torch.empty_like(wt)
                gb_full = torch.empty((C,), dtype=torch.float32, device=dev) if need_b else None
                _lib.call("manet_dwconv_backward_weight_f32", x.data_ptr(), g.data_ptr(), B, C, h, w, K, gw_full.data_ptr(),
                          _ptr(gb_full), ws.data_ptr(), ws.numel(), _stream_ptr(dev))
                gw = gw_full if need_w else None
                gb = gb_full
        return gx, gw, gb


class PointwiseConvFn(torch.autograd.Function):
    """1x1 convolution of the heads in training (IntVOS.py:244-332 _split_separable_conv2d.conv2, the embedding head's
    embedding_conv): F.conv2d(x, weight, bias) with a [Cout, Cin, 1, 1] weight, fp32 NCHW.  Forward manet_pw_forward_f32;
    backward manet_pw_backward_data_f32 (grad_x) and manet_pw_backward_weight_f32 (grad_weight and / or grad_bias,
    deterministic) -- each launched only when its gradient is asked for."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        wt = weight.detach().reshape(weight.shape[0], weight.shape[1]).contiguous()
        with torch.no_grad():
            out = ops._pw_forward(x, wt, bias)
        ctx.save_for_backward(x, wt)
        ctx.has_bias = bias is not None
        ctx.wshape = weight.shape
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, wt = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        B, Cin, h, w = x.shape
        Cout = wt.shape[0]
        dev = x.device
        g = grad_out.contiguous().float()
        gx = gw = gb = None
        with _on(dev):
            st = _stream_ptr(dev)
            if need_x:
                gx = torch.empty_like(x)
                _lib.call("manet_pw_backward_data_f32", g.data_ptr(), B, Cin, Cout, h * w, wt.data_ptr(), gx.data_ptr(), st)
            if need_w or need_b:
                nbytes = _ws_bytes("manet_pw_backward_weight_workspace_bytes", B, Cin, Cout, h * w)
                ws = _workspace(dev, "pw_backward_weight", nbytes)
                gw = torch.empty(ctx.wshape, dtype=torch.float32, device=dev) if need_w else None
                gb = torch.empty((Cout,), dtype=torch.float32, device=dev) if need_b else None
                _lib.call("manet_pw_backward_weight_f32", x.data_ptr(), g.data_ptr(), B, Cin, Cout, h * w, _ptr(gw), _ptr(gb),
                          ws.data_ptr(), nbytes, st)
        return gx, gw, gb


class BatchNormReluFn(torch.autograd.Function):
    """relu(batch_norm(x)) of the heads (IntVOS.py:244-332 bn1 -> relu1, bn2 -> relu2; the embedding head's), fp32 NCHW.
    Forward manet_bn_relu_forward_f32 (training: batch statistics, running_mean / running_var updated in place; eval: the
    running statistics); saves x and the per-channel mean / invstd it used, as the framework does.  Backward
    manet_bn_relu_backward_f32, asked only for the gradients needed (grad_x; grad_weight / grad_bias)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, training):
        x = x.contiguous()
        with torch.no_grad():
            out, save = ops._bn_relu_forward(x, weight, bias, running_mean, running_var, momentum, eps, training)
        ctx.save_for_backward(x, weight, bias, save)
        ctx.training = bool(training)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, bias, save = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        B, C, h, w = x.shape
        dev = x.device
        g = grad_out.contiguous().float()
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty((C,), dtype=torch.float32, device=dev) if need_w else None
        gb = torch.empty((C,), dtype=torch.float32, device=dev) if need_b else None
        if gx is None and gw is None and gb is None:
            return None, None, None, None, None, None, None, None
        with _on(dev):
            nbytes = _ws_bytes("manet_bn_relu_workspace_bytes", B, C, h * w)
            ws = _workspace(dev, "bn_relu", nbytes)
            _lib.call("manet_bn_relu_backward_f32", g.data_ptr(), x.data_ptr(), B, C, h * w, weight.data_ptr(), bias.data_ptr(),
                      save.data_ptr(), save.data_ptr() + 4 * C, 1 if ctx.training else 0, _ptr(gx), _ptr(gw), _ptr(gb),
                      ws.data_ptr(), nbytes, _stream_ptr(dev))
        return gx, gw, gb, None, None, None, None, None


class OutputConvFn(torch.autograd.Function):
    """DynamicSegHead's output layer in training (IntVOS.py:516,524): F.conv2d(x, weight, bias) with a [1, C, 1, 1] weight, fp32
    NCHW.  Forward manet_out_conv_forward_f32; backward manet_out_conv_backward_f32 (grad_x = weight[c] * g; grad_weight and
    grad_bias through per-tile partials added in a fixed order: deterministic), asked only for the gradients needed."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        wt = weight.detach().contiguous()
        with torch.no_grad():
            out = ops._out_conv_forward(x, wt, bias)
        ctx.save_for_backward(x, wt)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, wt = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2] and ctx.has_bias
        if not (need_x or need_w or need_b):
            return None, None, None
        B, C, h, w = x.shape
        dev = x.device
        g = grad_out.contiguous().float()
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(wt) if need_w else None
        gb = torch.empty((1,), dtype=torch.float32, device=dev) if need_b else None
        with _on(dev):
            nbytes = _ws_bytes("manet_out_conv_workspace_bytes", B, C, h * w)
            ws = _workspace(dev, "out_conv", nbytes)
            _lib.call("manet_out_conv_backward_f32", g.data_ptr(), x.data_ptr(), B, C, h * w, wt.data_ptr(), _ptr(gx), _ptr(gw),
                      _ptr(gb), ws.data_ptr(), nbytes, _stream_ptr(dev))
        return gx, gw, gb


def _head_bytes(B, Cin, Cmid, h, w, K):
    """(bytes of the saved activations, bytes of the workspace) of one head's training step"""
    return _lib.query("manet_head_train_bytes", B, Cin, Cmid, h, w, K, out=(ctypes.c_size_t,) * 2)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[_ptr(t) for t in tensors])


def _head_train_forward(ctx, head, x, params):
    """manet_head_train_forward_f32 on a contiguous x -> (logits, the saved activations, the parameters to keep); what the
    backward needs besides tensors goes onto `ctx`.  DynamicSegHeadFn and DynamicSegHeadPartsFn share it."""
    tensors = ops.dynamic_seghead_tensors(head)
    bns = ops.dynamic_seghead_bns(head)
    B, Cin, h, w = x.shape
    Cmid, K = head.conv.in_channels, head.layer1.conv1.kernel_size[0]
    dev = x.device
    saved_bytes, ws_bytes = _head_bytes(B, Cin, Cmid, h, w, K)
    saved = torch.empty(saved_bytes, dtype=torch.uint8, device=dev)
    logits = torch.empty((B, 1, h, w), dtype=torch.float32, device=dev)
    training = (ctypes.c_int * 8)(*[1 if bn.training else 0 for bn in bns])
    momentum = (ctypes.c_float * 8)(*[float(bn.momentum) for bn in bns])
    eps = (ctypes.c_float * 8)(*[float(bn.eps) for bn in bns])
    with _on(dev):
        ws = _workspace(dev, "head_train", ws_bytes)
        _lib.call("manet_head_train_forward_f32", x.data_ptr(), B, Cin, Cmid, h, w, K, _ptr_array(tensors), training, momentum,
                  eps, saved.data_ptr(), saved_bytes, ws.data_ptr(), ws_bytes, logits.data_ptr(), _stream_ptr(dev))
    # the backward reads parameters, not running statistics: those slots stay NULL there
    ctx.slots = [i for i, name in enumerate(ops.HEAD_BLOCK_TENSORS * 4 + ("conv.weight", "conv.bias")) if "running" not in name]
    ctx.present = [p is not None for p in params]
    ctx.dims = (B, Cin, Cmid, h, w, K)
    ctx.training = training
    return logits, saved, [p for p in params if p is not None]


def _head_train_backward(ctx, x, saved, kept, grad_out, need_x, need_params):
    """manet_head_train_backward_f32 -> (grad_x or None, the parameters' gradients in the order of `params`, None where not
    needed); need_params: the needs_input_grad entries of `params`.  (None, None) when no gradient at all is needed."""
    B, Cin, Cmid, h, w, K = ctx.dims
    dev = x.device
    it = iter(kept)
    params = [next(it) if present else None for present in ctx.present]
    need = [present and need_params[j] for j, present in enumerate(ctx.present)]
    if not (need_x or any(need)):
        return None, None
    g = grad_out.contiguous().float()
    gx = torch.empty_like(x) if need_x else None
    grads = [torch.empty_like(p) if n else None for p, n in zip(params, need)]
    p50, g50 = [None] * 50, [None] * 50
    for slot, p, gp in zip(ctx.slots, params, grads):
        p50[slot], g50[slot] = p, gp
    saved_bytes, ws_bytes = _head_bytes(B, Cin, Cmid, h, w, K)
    with _on(dev):
        ws = _workspace(dev, "head_train", ws_bytes)
        _lib.call("manet_head_train_backward_f32", g.data_ptr(), x.data_ptr(), B, Cin, Cmid, h, w, K, _ptr_array(p50),
                  ctx.training, saved.data_ptr(), saved_bytes, ws.data_ptr(), ws_bytes, _ptr_array(g50), _ptr(gx),
                  _stream_ptr(dev))
    return gx, grads


class DynamicSegHeadFn(torch.autograd.Function):
    """A whole DynamicSegHead (IntVOS.py:509-525: four _split_separable_conv2d blocks and conv = Conv2d(C, 1, 1)) in training as
    one node: apply(head, x, *params), params = the head's 34 parameters in the order of ops.dynamic_seghead_tensors without the
    running statistics (a missing bias: None).  Forward manet_head_train_forward_f32 -- the existing depthwise, BatchNorm + ReLU
    and 1x1 launchers sequenced in C, the output conv fused with layer 4's last BatchNorm + ReLU, running statistics updated in
    place; the activations the backward reads live in ONE tensor the context keeps.  Backward manet_head_train_backward_f32,
    told which of the 35 gradients are needed: a frozen input (train_stage2.py:57: the embedding under no_grad) skips layer 1's
    depthwise backward-data, a frozen parameter its reduction."""

    @staticmethod
    def forward(ctx, head, x, *params):
        x = x.contiguous()
        logits, saved, kept = _head_train_forward(ctx, head, x, params)
        ctx.save_for_backward(x, saved, *kept)
        return logits

    @staticmethod
    def backward(ctx, grad_out):
        x, saved, *kept = ctx.saved_tensors
        gx, grads = _head_train_backward(ctx, x, saved, kept, grad_out, ctx.needs_input_grad[1], ctx.needs_input_grad[2:])
        if grads is None:
            return (None,) * (2 + len(ctx.present))
        return (None, gx) + tuple(grads)


def _head_input_forward(ctx, embedding, maps, planes, n_ids, normalize_first):
    """manet_head_input_forward_f32 -> (x [n_ids, C + maps + planes, h, w], the normalised map 0 or None); the shapes and the
    embedding's layout the backward needs go onto `ctx`.  maps: float32 tensors of h*w*n_ids elements ([h, w, n_ids] order, any
    view shape); planes: flat int32 [h*w] (ops._head_input_operands has checked both)."""
    C, h, w = embedding.shape
    dev = embedding.device
    maps = [m.contiguous() for m in maps]
    x = torch.empty((n_ids, C + len(maps) + len(planes), h, w), dtype=torch.float32, device=dev)
    norm = torch.empty(h * w * n_ids, dtype=torch.float32, device=dev) if normalize_first else None
    with _on(dev):
        _lib.call("manet_head_input_forward_f32", *_strided(embedding), *[_ptr(m) for m in (maps + [None, None])[:2]],
                  *[_ptr(t) for t in (list(planes) + [None])[:2]], C, h, w, n_ids, len(maps), len(planes),
                  1 if normalize_first else 0, x.data_ptr(), _ptr(norm), _stream_ptr(dev))
    ctx.input_dims = (C, h, w, n_ids, len(maps), len(planes), bool(normalize_first))
    ctx.emb_layout = (embedding.shape, embedding.stride() if _dense(embedding) else None)
    ctx.map_shapes = [m.shape for m in maps]
    return x, norm


def _head_input_backward(ctx, gx, norm, need_emb, need_maps):
    """manet_head_input_backward_f32 on a contiguous gx -> (grad_embedding in the embedding's own layout, [grad_map_j]); None
    where not needed, and no launch when nothing is"""
    C, h, w, n_ids, n_maps, n_planes, normalize_first = ctx.input_dims
    dev = gx.device
    ge = None
    if need_emb:
        shape, stride = ctx.emb_layout
        ge = (torch.empty(shape, dtype=torch.float32, device=dev) if stride is None
              else torch.empty_strided(shape, stride, dtype=torch.float32, device=dev))
    gm = [torch.empty(shape, dtype=torch.float32, device=dev) if need else None for shape, need in zip(ctx.map_shapes, need_maps)]
    if ge is not None or any(m is not None for m in gm):
        with _on(dev):
            _lib.call("manet_head_input_backward_f32", gx.data_ptr(), _ptr(norm), C, h, w, n_ids, n_maps, n_planes,
                      1 if normalize_first else 0, *_optional(ge, 0, 0, 0), *[_ptr(m) for m in (gm + [None, None])[:2]],
                      _stream_ptr(dev))
    return ge, (gm + [None, None])[:2]


class HeadInputFn(torch.autograd.Function):
    """The heads' input in training (IntVOS.py:663-671, :741-758) as one node: apply(embedding, map0, map1, planes, n_ids,
    normalize_first) -> x [n_ids, C + maps + planes, h, w] = cat(embedding repeated per object, the maps permuted to [n_ids, 1, h,
    w] -- map 0 through (sigmoid(d) - 0.5) * 2 when normalize_first --, labels == object).  map0 / map1: tensors or None;
    planes: a tuple of flat int32 label planes.  Forward manet_head_input_forward_f32; backward manet_head_input_backward_f32,
    asked only for the gradients needed (embedding, map0, map1).  It keeps the normalised map 0, never x."""

    @staticmethod
    def forward(ctx, embedding, map0, map1, planes, n_ids, normalize_first):
        x, norm = _head_input_forward(ctx, embedding, [m for m in (map0, map1) if m is not None], planes, n_ids, normalize_first)
        ctx.save_for_backward(*([norm] if norm is not None else []))
        return x

    @staticmethod
    def backward(ctx, grad_x):
        norm = ctx.saved_tensors[0] if ctx.saved_tensors else None
        ge, gm = _head_input_backward(ctx, grad_x.contiguous().float(), norm, ctx.needs_input_grad[0], ctx.needs_input_grad[1:3])
        return ge, gm[0], gm[1], None, None, None


class DynamicSegHeadPartsFn(torch.autograd.Function):
    """HeadInputFn and DynamicSegHeadFn as ONE node: apply(head, embedding, map0, map1, planes, n_ids, normalize_first, *params)
    -> logits [n_ids, 1, h, w].  Forward: the assembly kernel into x, then manet_head_train_forward_f32 exactly as
    DynamicSegHeadFn calls it; backward: manet_head_train_backward_f32, then the assembly's backward on its grad_x.  With a
    frozen embedding and no differentiated map (train_stage2.py: the embedding under no_grad, the interaction head has no maps)
    nobody needs grad_x and layer 1's depthwise backward-data is skipped."""

    @staticmethod
    def forward(ctx, head, embedding, map0, map1, planes, n_ids, normalize_first, *params):
        x, norm = _head_input_forward(ctx, embedding, [m for m in (map0, map1) if m is not None], planes, n_ids, normalize_first)
        logits, saved, kept = _head_train_forward(ctx, head, x, params)
        ctx.has_norm = norm is not None
        ctx.save_for_backward(x, saved, *([norm] if norm is not None else []), *kept)
        return logits

    @staticmethod
    def backward(ctx, grad_out):
        x, saved, *kept = ctx.saved_tensors
        norm = kept.pop(0) if ctx.has_norm else None
        need_emb, need_maps = ctx.needs_input_grad[1], ctx.needs_input_grad[2:4]
        need_maps = [need and j < len(ctx.map_shapes) for j, need in enumerate(need_maps)]
        gx, grads = _head_train_backward(ctx, x, saved, kept, grad_out, need_emb or any(need_maps), ctx.needs_input_grad[7:])
        if grads is None:
            return (None,) * (7 + len(ctx.present))
        ge, gm = _head_input_backward(ctx, gx, norm, need_emb, need_maps) if gx is not None else (None, [None, None])
        return (None, ge, gm[0], gm[1], None, None, None) + tuple(grads)


class UpsampledCrossEntropyTopKFn(torch.autograd.Function):
    """The loss behind the head (train_stage1.py:126-153 + networks/loss.py:44-81: bilinear upsample, cross-entropy with
    ignore_index=255, top-k of the pixel losses, mean) as one op on csrc/loss_train.hip's kernels; ops.upsampled_cross_entropy_topk,
    networks.loss.Added_CrossEntropyLoss.  Forward manet_loss_ce_topk_forward_f32; it keeps the pixel losses and each row's
    threshold (t, n_gt, n_eq), from which manet_loss_ce_topk_backward_f32 -- launched only when `logits` wants its gradient --
    gathers d logits in a fixed order."""

    @staticmethod
    def forward(ctx, logits, labels, size, k, divisor):
        logits = logits.detach()
        with torch.no_grad():
            loss, pix, stats = ops._loss_forward(logits, labels, size, k, divisor)
        ctx.save_for_backward(logits, labels, pix, stats)
        ctx.size, ctx.k, ctx.divisor = size, k, divisor
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        logits, labels, pix, stats = ctx.saved_tensors
        dev = logits.device
        B = logits.shape[0]
        g = grad_out.detach()
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.float().contiguous()
        gl = torch.empty(logits.shape, dtype=torch.float32, device=dev)
        with _on(dev):
            _lib.call("manet_loss_ce_topk_backward_f32", *ops._loss_args(logits, labels, ctx.size), ctx.k, ctx.divisor,
                      pix.data_ptr(), stats.data_ptr(), stats.data_ptr() + 4 * B, stats.data_ptr() + 8 * B, g.data_ptr(),
                      gl.data_ptr(), _stream_ptr(dev))
        return gl, None, None, None, None
