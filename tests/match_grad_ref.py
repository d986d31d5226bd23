"""float64 restatements of the four matching operations the training route differentiates, on whatever device their inputs live
(a helper module, not a test: tests/test_match_grad_ref.py holds it to the reference's own autograd on a CPU, the GPU tests
compare the HIP backward kernels with it).

Embeddings come C-major, [C, h, w], as the heads write them; the gradients come back in that shape, in float64.

  restatements on a GIVEN selection (they gather, they do not search):
    global_out64 / global64   out[n, o] = sum_r wgt[r, n, o] |q_n - k_arg[r, n, o]|^2        (IntVOS.py:32-39, :84, :87-94)
    local_out64 / local64     downsample: pooled frames, squared distance, (sigmoid - 0.5) * 2, 1.0 outside, the four bilinear
                              taps with the op's own fp32 tap constants widened to float64    (IntVOS.py:279-296, :398-432);
                              no downsample: the raw full-resolution squared distance          (IntVOS.py:299-313)
  brute-force float64 selectors (they search; nothing of the kernels' order of evaluation in them):
    global_select64           the k smallest per (query, object) among the object's rows, -1 past the object's row count, the
                              per-rank weights of autograd.GlobalMatchTopkFn.forward
    local_select64            the masked minimum over the window against the constant 1.0, labels gathered at stride 2 and 0 outside
  both selectors also return the smallest margin by which a selection was decided: a test that compares with a float32
  selection asserts that no decision was a near-tie."""
import numpy as np
import torch

PADDING = 1e20  # WRONG_LABEL_PADDING_DISTANCE (IntVOS.py:83): the k = 1 distance to an object without rows


def hwc(t):
    return t.permute(1, 2, 0)


def rows_of(chw):
    """[C, h, w] -> [h * w, C]"""
    return hwc(chw).reshape(-1, chw.shape[0])


# ------------------------------------------------------------------------------------------------------------------ global

def pairwise64(qs, rows):
    """|q_n - k_m|^2 [N, M0] in float64 (the expanded form: exact where the inputs are small dyadic numbers)"""
    return (qs * qs).sum(1)[:, None] + (rows * rows).sum(1)[None, :] - 2.0 * (qs @ rows.t())


def global_select64(ref, qry, labels, n_ids, k):
    """-> (arg [k, N, n_ids] int64, wgt [k, N, n_ids] float64, dist [k, N, n_ids] float64 ascending along k (inf past the row
    count), margin).  margin: the smallest gap that decided a selection or the rank the padding share goes to -- between the
    k-th and the (k+1)-th row of an object with more than k rows, and between the farthest and the second-farthest real
    neighbour of an object with 2 .. k-1 rows (inf if there was nothing to decide)."""
    rows, qs = rows_of(ref.detach().double()), rows_of(qry.detach().double())
    lab = labels.reshape(-1).long()
    N, M0 = qs.shape[0], rows.shape[0]
    dist = pairwise64(qs, rows)
    arg = torch.full((k, N, n_ids), -1, dtype=torch.int64, device=qs.device)
    dsel = torch.full((k, N, n_ids), float("inf"), dtype=torch.float64, device=qs.device)
    margin = float("inf")
    kk = min(k + 1, M0)
    for o in range(n_ids):
        v = int((lab == o).sum())
        if v == 0:
            continue
        vals, idx = torch.topk(dist.masked_fill((lab != o)[None, :], float("inf")), kk, dim=1, largest=False, sorted=True)
        take = min(k, v)
        arg[:take, :, o] = idx[:, :take].t()
        dsel[:take, :, o] = vals[:, :take].t()
        if v > k:
            margin = min(margin, float((vals[:, k] - vals[:, k - 1]).min()))
        elif 2 <= v < k:
            margin = min(margin, float((vals[:, v - 1] - vals[:, v - 2]).min()))
    valid = arg >= 0
    nvalid = valid.sum(0, keepdim=True)
    wgt = valid.double() / k
    if k > 1:  # the replaced entries' share goes to the farthest real neighbour: the last valid rank (none: no weight at all)
        last = (nvalid - 1).clamp(min=0)
        extra = (k - nvalid).double() / k * (nvalid > 0).double()
        wgt.scatter_add_(0, last, extra)
    return arg, wgt, dsel, margin


def global_out64(rows, qs, arg, wgt):
    """out [N, n_ids] = sum_r wgt[r] |q_n - k_arg[r]|^2 over the ranks with a row; k = 1 (one rank) without a row: 1e20.
    rows [M0, C], qs [N, C] float64 (differentiable); arg / wgt [ranks, N, n_ids]"""
    cols = []
    for o in range(arg.shape[2]):
        acc = 0
        for r in range(arg.shape[0]):
            a = arg[r, :, o].long()
            w_ = (a >= 0).double() * wgt[r, :, o].double()
            if rows.shape[0] == 0:
                continue
            acc = acc + ((qs - rows[a.clamp(min=0)]) ** 2).sum(1) * w_
        cols.append(acc if torch.is_tensor(acc) else torch.zeros(qs.shape[0], dtype=torch.float64, device=qs.device))
    out = torch.stack(cols, 1)
    if arg.shape[0] == 1:
        out = torch.where(arg[0] >= 0, out, torch.full_like(out, PADDING))
    return out


def global64(ref, qry, arg, wgt, gout):
    """the gradients of sum(out * gout) w.r.t. ref and qry [C, ., .] on the selection `arg` [ranks, N, n_ids] with the per-rank
    weights `wgt` (ones for k = 1; what the op recorded, or global_select64's, otherwise)"""
    r64 = ref.detach().double().requires_grad_(True)
    q64 = qry.detach().double().requires_grad_(True)
    valid = ((arg >= 0) * (wgt != 0)).any(0)  # (the k = 1 padding constant carries no gradient)
    out = global_out64(rows_of(r64), rows_of(q64), arg, wgt)
    loss = (torch.where(valid, out, torch.zeros_like(out)) * gout.reshape(out.shape).double()).sum()
    if not loss.requires_grad:  # nothing selected at all
        return torch.zeros_like(r64), torch.zeros_like(q64)
    return torch.autograd.grad(loss, [r64, q64], allow_unused=False)


# ------------------------------------------------------------------------------------------------------------------- local

def taps64(n_out, n_in, device):
    """F.interpolate(bilinear, align_corners=True) source positions and weights: the constants of the op itself (float32
    scale = (in - 1) / (out - 1), src = scale * dst, i0 = trunc, l1 = src - i0, l0 = 1 - l1), widened to float64"""
    if n_out > 1:
        scale = torch.tensor(float(n_in - 1), device=device) / torch.tensor(float(n_out - 1), device=device)
    else:
        scale = torch.zeros((), device=device)
    src = scale * torch.arange(n_out, dtype=torch.float32, device=device)
    i0 = src.to(torch.int64).clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = src - i0.float()
    return i0, i1, (1.0 - l1).double(), l1.double()


def max_cover(n_in, n_out):
    """most of the n_out full-resolution positions whose taps (i0, i1) include one of the n_in pooled positions, from the tap
    constants above: what bounds the winners one pooled cell can collect"""
    i0 = taps64(n_out, n_in, "cpu")[0].numpy()
    return max(int(((i0 >= t - 1) & (i0 <= t)).sum()) for t in range(n_in))


def _selected_values64(p64, c64, ys, xs, l, d, downsample):
    """the value of window offset l[i] at pixel (ys[i], xs[i]) -- differentiable in the frames p64 (previous), c64 (current)"""
    h, w = c64.shape[1:]
    P = 2 * d + 1
    dy, dx = l // P - d, l % P - d
    if downsample:
        xp = torch.nn.functional.avg_pool2d(c64[None], 2)[0]
        yp = torch.nn.functional.avg_pool2d(p64[None], 2)[0]
        hp, wp = xp.shape[1:]
        i0, i1, ly0, ly1 = taps64(h, hp, c64.device)
        j0, j1, lx0, lx1 = taps64(w, wp, c64.device)
        val = 0
        for ti, wy in ((i0[ys], ly0[ys]), (i1[ys], ly1[ys])):
            for tj, wx in ((j0[xs], lx0[xs]), (j1[xs], lx1[xs])):
                qi, qj = ti + dy, tj + dx
                inside = (qi >= 0) & (qi < hp) & (qj >= 0) & (qj < wp)
                dist = ((xp[:, ti, tj] - yp[:, qi.clamp(0, hp - 1), qj.clamp(0, wp - 1)]) ** 2).sum(0)
                vn = torch.where(inside, (torch.sigmoid(dist) - 0.5) * 2, torch.ones_like(dist))
                val = val + wy * wx * vn
        return val
    qi, qj = ys + dy, xs + dx
    assert bool(((qi >= 0) & (qi < h) & (qj >= 0) & (qj < w)).all())  # (an outside neighbour is 1e20 away: it cannot win)
    return ((c64[:, ys, xs] - p64[:, qi, qj]) ** 2).sum(0)


def local_out64(p64, c64, arg, d, downsample):
    """out [h, w, n_ids] on the winning offsets `arg` (-1: the constant 1.0 won); p64 / c64 [C, h, w] float64"""
    ys, xs, os_ = torch.nonzero(arg >= 0, as_tuple=True)
    out = torch.ones(arg.shape, dtype=torch.float64, device=c64.device)
    if ys.numel() == 0:
        return out
    val = _selected_values64(p64, c64, ys, xs, arg[ys, xs, os_].long(), d, downsample)
    return out.index_put((ys, xs, os_), val)


def local64(prev, cur, arg, gout, d, downsample):
    """float64 restatement of the local match on the recorded winning offsets (IntVOS.py:266-313, :398-432): gathers the
    selected candidate of every (pixel, object) and does not re-run the min -> the gradients w.r.t. prev and cur"""
    p64 = prev.detach().double().requires_grad_(True)
    c64 = cur.detach().double().requires_grad_(True)
    ys, xs, os_ = torch.nonzero(arg >= 0, as_tuple=True)
    if ys.numel() == 0:
        return torch.zeros_like(p64), torch.zeros_like(c64)
    val = _selected_values64(p64, c64, ys, xs, arg[ys, xs, os_].long(), d, downsample)
    return torch.autograd.grad((val * gout[ys, xs, os_].double()).sum(), [p64, c64])


def local_select64(prev, cur, labels, n_ids, d, downsample):
    """brute force -> (arg [h, w, n_ids] int64: the first window offset that attains the minimum of where(label == o, value,
    1.0), -1 where that candidate is the constant; margin: the smallest gap between a winner and the second-best candidate
    of its (pixel, object), inf if no winner had a rival)"""
    p64, c64 = prev.detach().double(), cur.detach().double()
    C, h, w = c64.shape
    P = 2 * d + 1
    dev = c64.device
    if downsample:
        xp = torch.nn.functional.avg_pool2d(c64[None], 2)[0]
        yp = torch.nn.functional.avg_pool2d(p64[None], 2)[0]
    else:
        xp, yp = c64, p64
    hp, wp = xp.shape[1:]
    vol = torch.empty((P * P, hp, wp), dtype=torch.float64, device=dev)
    padded = torch.full((C, hp + 2 * d, wp + 2 * d), float("nan"), dtype=torch.float64, device=dev)
    padded[:, d:d + hp, d:d + wp] = yp
    for by in range(P):
        for bx in range(P):
            dist = ((xp - padded[:, by:by + hp, bx:bx + wp]) ** 2).sum(0)
            if downsample:
                vol[by * P + bx] = torch.where(torch.isnan(dist), torch.ones_like(dist), (torch.sigmoid(dist) - 0.5) * 2)
            else:
                vol[by * P + bx] = torch.where(torch.isnan(dist), torch.full_like(dist, float("inf")), dist)
    if downsample:
        i0, i1, ly0, ly1 = taps64(h, hp, dev)
        j0, j1, lx0, lx1 = taps64(w, wp, dev)
        rows = vol[:, i0] * ly0[None, :, None] + vol[:, i1] * ly1[None, :, None]
        vol = rows[:, :, j0] * lx0[None, None, :] + rows[:, :, j1] * lx1[None, None, :]
    lab = torch.zeros((h + 4 * d, w + 4 * d), dtype=torch.int64, device=dev)  # (the reference pads the labels with 0)
    lab[2 * d:2 * d + h, 2 * d:2 * d + w] = labels.reshape(h, w).long()
    offs = torch.stack([lab[2 * by:2 * by + h, 2 * bx:2 * bx + w] for by in range(P) for bx in range(P)])  # [PP, h, w]
    arg = torch.empty((h, w, n_ids), dtype=torch.int64, device=dev)
    margin = float("inf")
    for o in range(n_ids):
        hit = offs == o
        cand = torch.where(hit, vol, torch.ones_like(vol))
        best, l = cand.min(0)
        l = (cand == best[None]).to(torch.uint8).argmax(0)  # the first offset among equals
        won = torch.gather(hit, 0, l[None])[0]
        arg[:, :, o] = torch.where(won, l, torch.full_like(l, -1))
        if P * P > 1 and bool(won.any()):
            second = torch.topk(cand, 2, dim=0, largest=False).values[1]
            margin = min(margin, float((second - best)[won].min()))
    return arg, margin


def to_numpy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
