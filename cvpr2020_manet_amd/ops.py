"""torch-tensor front-end of the C ABI (include/manet_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; every function
below hands raw device pointers, element strides and that stream to libmanet_hip.so.  All inputs
must live on a HIP device -- there is deliberately no CPU path (a silent fallback would void the
parity claims); CPU tensors raise.
"""
import ctypes
import functools

import torch

from . import _lib

# "bf16r": bf16 filter + exact fp32 re-rank (MANET_COMPUTE_BF16_REFINE): MANET_COMPUTE_F32's result bit for bit, ~1.4x bf16's cost
# "f16": fp16 MFMA on embeddings rounded to fp16 (MANET_COMPUTE_F16): bf16's cost, an input-rounding error 8x smaller; values with
# |row|^2 > 65504 are outside its domain and give NaN (include/manet_hip.h)
# "f16r": fp16 filter + exact fp32 re-rank (MANET_COMPUTE_F16_REFINE): bf16r with the filter in fp16 -- MANET_COMPUTE_F32's result bit for
# bit on every input (rows outside fp16's domain go through the exact fp32 kernel), a threshold 8x tighter than bf16's
COMPUTE = {"f32": _lib.COMPUTE_F32, "fp32": _lib.COMPUTE_F32, "bf16": _lib.COMPUTE_BF16,
           "bf16x3": _lib.COMPUTE_BF16X3, "bf16r": _lib.COMPUTE_BF16_REFINE, "f16": _lib.COMPUTE_F16, "fp16": _lib.COMPUTE_F16,
           "f16r": _lib.COMPUTE_F16_REFINE}
_REFINE_NAME = {_lib.COMPUTE_BF16_REFINE: "bf16r", _lib.COMPUTE_F16_REFINE: "f16r"}


def _image_kind(compute_code):
    """operand images depend on the arithmetic only through this: bf16r packs exactly as bf16, f16r exactly as f16; f16 is a kind
    of its own (the bf16 image's layout and size with fp16 elements: nothing but this comparison tells the two apart)"""
    if compute_code == _lib.COMPUTE_F16_REFINE:
        return _lib.COMPUTE_F16
    return _lib.COMPUTE_BF16 if compute_code == _lib.COMPUTE_BF16_REFINE else compute_code

_ws_cache = {}


def _need_gpu(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("cvpr2020_manet_amd: %s must be a tensor on a HIP device "
                           "(the matching path has no CPU fallback)" % name)


def _refuse_autograd(what, *tensors):
    """The HIP ops below hand raw pointers to the C ABI and return tensors without a grad_fn.  The
    reference's functions are differentiable (train_stage1.py:126-156 back-propagates through them), so
    silently detaching would train the heads with zero gradient through the match maps: raise instead.
    Ops that do have a backward (`global_match`, `local_match`, `correlation_forward`) route through their
    torch.autograd.Function in cvpr2020_manet_amd.autograd instead of coming here."""
    if not torch.is_grad_enabled():
        return
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise RuntimeError("cvpr2020_manet_amd.ops.%s: an input requires grad, but this op has no "
                               "backward -- call it under torch.no_grad() or detach the input "
                               "(gradients would otherwise be dropped silently)" % what)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _global_match_autograd(reference_embeddings, query_embeddings, reference_labels, n_ids, k_nearest_neighbors,
                           compute, normalize, mem, deterministic=False):
    """Training route of global_match (train_stage1.py:126-156 back-propagates through it): the arg-min forward +
    explicit backward of autograd.GlobalMatchFn; normalisation (IntVOS.py:611-612) and the min-merge with the
    stored map (:620-622, the stored copy detached as in the reference) are ordinary differentiable torch ops."""
    from .autograd import GlobalMatchFn, GlobalMatchTopkFn, GlobalMatchOrderedFn, GlobalMatchTopkOrderedFn
    if deterministic:  # the ordered backward (csrc/match_train.hip): no float atomics, the same gradient bits on every run
        GlobalMatchFn, GlobalMatchTopkFn = GlobalMatchOrderedFn, GlobalMatchTopkOrderedFn
    if COMPUTE[compute] != _lib.COMPUTE_F32 or not 1 <= k_nearest_neighbors <= 8:
        raise RuntimeError("cvpr2020_manet_amd.ops.global_match: the backward exists for compute='f32' and "
                           "k_nearest_neighbors 1..8 only (got k=%d, compute=%r)" % (k_nearest_neighbors, compute))
    ref, qry, lab = _match_operands(reference_embeddings, query_embeddings, reference_labels, k_nearest_neighbors)
    ref, qry = ref.float(), qry.float()  # (a differentiable widening if the embeddings are stored in bf16)
    if k_nearest_neighbors > 1:
        out = GlobalMatchTopkFn.apply(ref, qry, lab, n_ids, int(k_nearest_neighbors))
    else:
        out, _ = GlobalMatchFn.apply(ref, qry, lab, n_ids)
    if normalize:
        out = (torch.sigmoid(out) - 0.5) * 2
    if mem is not None:
        m = mem.view_as(out)
        out = torch.where(out <= m, out, m)
        with torch.no_grad():
            m.copy_(out)
    return out


def _stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


class _NoSwitch:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(device):
    """`with _on(dev):` replaces `with torch.cuda.device(dev):`, minus the guard object when `dev` already is the current
    device (the usual case: ~4 us of host time per call, 20 calls per propagated frame -- the eager loop is host-bound)"""
    return _NO_SWITCH if torch.cuda.current_device() == device.index else torch.cuda.device(device)


def _workspace(device, tag, nbytes):
    """Per (device, stream, tag) scratch tensor, grown on demand (torch allocator = plumbing)."""
    key = (device.index, _stream_ptr(device), tag)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def _armed_workspace(device, tag, nbytes):
    """Like _workspace, but the tensor is created FILLED with 0xff bytes and is only ever handed to calls that keep it so
    (MANET_EPI_KEYS_ARMED: the match keys are re-armed by the epilogue that reads them) -- no per-call fill launch."""
    key = (device.index, _stream_ptr(device), tag)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.full((int(nbytes * 1.25) + 1024,), 0xff, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def _emb(t):
    """embeddings are consumed in the producer's storage: float32, or bfloat16 (2-byte reads end to end,
    SURVEY.md 8f rank 4); anything else is widened to float32"""
    return t if t.dtype in (torch.float32, torch.bfloat16) else t.float()


def _emb_code(t):
    return _lib.EMB_BF16 if t.dtype == torch.bfloat16 else _lib.EMB_F32


def _flat(t, name):
    """[..., C] -> ([rows, C] view, rows, C); like the reference's .view(-1, C) (IntVOS.py:203-204)
    but a non-viewable input is copied instead of raising."""
    _need_gpu(t, name)
    t = _emb(t)
    t2 = t.reshape(-1, t.shape[-1])
    return t2, t2.shape[0], t2.shape[1]


def _labels(t, name, count):
    """flat contiguous int32 labels, one per pixel: `count` of them"""
    _need_gpu(t, name)
    lab = t.reshape(-1).to(torch.int32).contiguous()
    if lab.numel() != count:
        raise ValueError("%s has %d entries for %d pixels" % (name, lab.numel(), count))
    return lab


def _match_operands(reference_embeddings, query_embeddings, reference_labels, k_nearest_neighbors):
    """the global match's operands, flattened and validated -> (ref [M0, C], qry [N, C], int32 labels [M0])"""
    ref, M0, C = _flat(reference_embeddings, "reference_embeddings")
    qry, _, C2 = _flat(query_embeddings, "query_embeddings")
    if C != C2:
        raise ValueError("embedding_dim mismatch: %d vs %d" % (C, C2))
    lab = _labels(reference_labels, "reference_labels", M0)
    if k_nearest_neighbors > 1 and M0 < k_nearest_neighbors:
        raise RuntimeError("selected index k out of range")  # what torch.topk raises (IntVOS.py:87)
    return ref, qry, lab


def _mem_ptr(mem, count):
    """pointer of the optional stored map the epilogue merges into (None: null); `count` contiguous float32 on the GPU"""
    if mem is None:
        return None
    _need_gpu(mem, "mem")
    if mem.dtype != torch.float32 or not mem.is_contiguous() or mem.numel() != count:
        raise ValueError("mem must be a contiguous float32 tensor of %d elements" % count)
    return mem.data_ptr()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _strided(t):
    """(pointer, *element strides): how the C ABI takes a tensor of any strides"""
    return (t.data_ptr(), *t.stride())


def _bank_strides(ref):
    """element strides of a [M0, C] bank; an empty bank goes as (C, 1)"""
    return ref.stride() if ref.shape[0] > 0 else (ref.shape[1], 1)


def _optional(t, *placeholder):
    """_strided(t) of an output that may not be wanted: None goes as a null pointer with the `placeholder` strides"""
    return (None, *placeholder) if t is None else (t.data_ptr(), *t.stride())


def global_match(reference_embeddings, query_embeddings, reference_labels, n_ids, k_nearest_neighbors=1,
                 compute="f32", normalize=False, mem=None, deterministic=False):
    """nearest_neighbor_features_per_object on the HIP path (IntVOS.py:160-210), optionally with the
    fused normalise (IntVOS.py:611-612) and min-merge into `mem` (IntVOS.py:620-622, in place).

    Returns float32 [N, n_ids] (N = number of query pixels), raw or normalised distances.
    deterministic=True: when the call is differentiated, the backward is the ordered, atomic-free one (the same gradient bits
    on every run); forward values are the same either way.
    """
    if _wants_grad(reference_embeddings, query_embeddings, mem):
        return _global_match_autograd(reference_embeddings, query_embeddings, reference_labels, n_ids,
                                      k_nearest_neighbors, compute, normalize, mem, deterministic)
    ref, qry, lab = _match_operands(reference_embeddings, query_embeddings, reference_labels, k_nearest_neighbors)
    (M0, C), N = ref.shape, qry.shape[0]
    dev = qry.device
    cmp_ = COMPUTE[compute]
    ws = _workspace(dev, "global", _lib.query("manet_global_match_workspace_bytes", N, M0, C, n_ids, k_nearest_neighbors, cmp_))
    out = torch.empty((N, n_ids), dtype=torch.float32, device=dev)
    mem_ptr = _mem_ptr(mem, N * n_ids)
    flags = _lib.EPI_NORMALIZE if normalize else 0
    with _on(dev):
        _lib.call("manet_global_match_ex", qry.data_ptr(), _emb_code(qry), *qry.stride(), ref.data_ptr(), _emb_code(ref),
                  *_bank_strides(ref), lab.data_ptr(), N, M0, C, n_ids, k_nearest_neighbors, cmp_, out.data_ptr(), mem_ptr,
                  flags, ws.data_ptr(), ws.numel(), _stream_ptr(dev))
    return out


_PROBE_POOL = {"block": None, "next": 0}


def _probe_slot():
    """Two pinned int32 the adaptive probe kernel of compute="bf16r" writes through a raw pointer.  Slots of ONE pinned block
    that lives as long as the process (a per-bank pin_memory() tensor could go back to torch's pinned allocator
    with a device write still in flight -- the allocator knows nothing of it); handed out round robin, 1024 of them."""
    if _PROBE_POOL["block"] is None:
        _PROBE_POOL["block"] = torch.zeros(1024, 2, dtype=torch.int32).pin_memory()
    i = _PROBE_POOL["next"]
    _PROBE_POOL["next"] = (i + 1) % 1024
    return _PROBE_POOL["block"][i]


class PreparedBank:
    """A memory bank sorted by object id and packed for the MFMA loop, reusable across frames
    (test.py:237-259 matches every frame of a clip against the same annotated frame)."""

    def __init__(self, reference_embeddings, reference_labels, n_ids, compute="f32", reuse=None):
        """reuse: a PreparedBank that is no longer needed -- its workspace is taken over when it is large enough (a new
        interaction round re-prepares a bank of the same size: no 50-100 MB allocation per round)"""
        _refuse_autograd("PreparedBank", reference_embeddings)
        ref, M0, C = _flat(reference_embeddings, "reference_embeddings")
        lab = _labels(reference_labels, "reference_labels", M0)
        self.M0, self.C, self.n_ids, self.compute = M0, C, n_ids, COMPUTE[compute]
        self.device = ref.device
        nbytes = _lib.query("manet_bank_workspace_bytes", M0, C, n_ids, self.compute)  # (reads a tuning knob: asked per bank)
        if getattr(reuse, "_adapt", None) is not None:
            self._adapt = reuse._adapt  # (what the previous bank of this clip learnt about its embeddings carries over)
        old = getattr(reuse, "ws", None)
        if old is not None and old.device == self.device and old.numel() >= nbytes:
            self.ws, reuse.ws = old, None
        else:
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with _on(self.device):
            _lib.call("manet_bank_prepare_ex", ref.data_ptr(), _emb_code(ref), *_bank_strides(ref), lab.data_ptr(), M0, C, n_ids,
                      self.compute, self.ws.data_ptr(), self.ws.numel(), _stream_ptr(self.device))

    # compute="bf16r" / "f16r", adaptive policy: a frame whose filter pass sent more than this share of its query tiles to the rescue
    # pass (the exact fp32 kernel) cost the filter AND most of the fp32 kernel; the next ADAPT_FRAMES frames then skip the
    # filter (MANET_EPI_REFINE_EXACT: the same bits at the fp32 path's cost), after which one frame probes the filter again.
    # (The rescue launch is dealt to the rescued tiles only: a share r costs ~r of the fp32 kernel, so filtering pays below
    # r ~ 1 - filter / fp32 kernel ~ 0.85 at cfg2 shape; r3's all-or-nothing rescue had the switch at one half.)
    ADAPT_SHARE, ADAPT_FRAMES, ADAPT_PROBE_EVERY = 0.8, 16, 4

    def match(self, query_embeddings, k_nearest_neighbors=1, normalize=False, mem=None, out=None, adaptive=True):
        """query_embeddings: [..., C] float32 / bfloat16 tensor, or a PackedQuery (operand image made once,
        e.g. for every frame of a clip right after extract_feature: no per-frame pack pass).
        adaptive (compute="bf16r" / "f16r" only): let the previous frames' rescue share decide whether this frame runs the filter at
        all (see ADAPT_SHARE); the result is the fp32 kernel's bit for bit either way.  The share arrives by an asynchronous copy
        and is read a frame late -- no synchronisation; nothing adapts inside a HIP-graph capture."""
        armed, raw = False, None
        if isinstance(query_embeddings, (PackedQuery, PreparedFrame)):
            pq = query_embeddings
            if pq.C != self.C or _image_kind(pq.compute) != _image_kind(self.compute):
                raise ValueError("the query operand was packed for C=%d compute=%d, bank has C=%d compute=%d"
                                 % (pq.C, pq.compute, self.C, self.compute))
            _refuse_autograd("PreparedBank.match", mem)
            qry, N, C, q_code, q_s0, q_s1 = pq.image, pq.N, pq.C, _lib.EMB_PACKED, 0, 0
            armed = k_nearest_neighbors == 1 and self.compute not in _lib.REFINE_MODES
            if self.compute in _lib.REFINE_MODES:  # the exact re-rank reads the query as stored
                if pq.raw is None:
                    raise ValueError("compute=%r needs the embedding the operand image was made from (still alive)"
                                     % _REFINE_NAME[self.compute])
                raw, _, _ = _flat(pq.raw, "query_embeddings")
        else:
            _refuse_autograd("PreparedBank.match", query_embeddings, mem)
            qry, N, C = _flat(query_embeddings, "query_embeddings")
            q_code, q_s0, q_s1 = _emb_code(qry), qry.stride(0), qry.stride(1)
        if C != self.C:
            raise ValueError("embedding_dim mismatch: %d vs %d" % (C, self.C))
        if k_nearest_neighbors > 1 and self.M0 < k_nearest_neighbors:
            raise RuntimeError("selected index k out of range")
        dev = qry.device if isinstance(qry, torch.Tensor) else self.device
        nbytes = _lib.query("manet_match_workspace_bytes", N, self.M0, C, self.n_ids, k_nearest_neighbors, self.compute)
        ws = _armed_workspace(dev, "match_armed", nbytes) if armed else _workspace(dev, "match", nbytes)
        if out is None:
            out = torch.empty((N, self.n_ids), dtype=torch.float32, device=dev)
        mem_ptr = _mem_ptr(mem, N * self.n_ids)
        flags = (_lib.EPI_NORMALIZE if normalize else 0) | (_lib.EPI_KEYS_ARMED if armed else 0)
        self._last = (ws, N)  # (refine_stats)
        refine = self.compute in _lib.REFINE_MODES
        adapt = refine and adaptive and not torch.cuda.is_current_stream_capturing()
        forced = False
        if adapt:
            ad = self.__dict__.setdefault("_adapt", {"host": None, "event": None, "left": 0, "seen": 0})
            if ad["event"] is not None and ad["event"].query():  # the share of a frame or two ago has arrived
                rescued, tiles = int(ad["host"][0]), int(ad["host"][1])
                ad["event"] = None
                if tiles > 0 and rescued > self.ADAPT_SHARE * tiles:
                    ad["left"] = self.ADAPT_FRAMES
            forced = ad["left"] > 0
            if forced:
                ad["left"] -= 1
                flags |= _lib.EPI_REFINE_EXACT
        self.last_match_forced_exact = forced
        if adapt and not forced:
            ad["seen"] = ad.get("seen", 0) + 1
        try:
            with _on(dev):
                if raw is not None:
                    mode = _lib.EPI_REFINE_F16 if self.compute == _lib.COMPUTE_F16_REFINE else 0
                    _lib.call("manet_global_match_refine", raw.data_ptr(), _emb_code(raw), *raw.stride(), qry.data_ptr(),
                              self.ws.data_ptr(), N, self.M0, C, self.n_ids, out.data_ptr(), mem_ptr, flags | mode, ws.data_ptr(),
                              ws.numel(), _stream_ptr(dev))
                else:
                    _lib.call("manet_global_match_prepared_ex", qry.data_ptr(), q_code, q_s0, q_s1, self.ws.data_ptr(), N, self.M0,
                              C, self.n_ids, k_nearest_neighbors, self.compute, out.data_ptr(), mem_ptr, flags, ws.data_ptr(),
                              ws.numel(), _stream_ptr(dev))
        except RuntimeError:
            if armed:
                # the armed workspace is only all-0xff again once the finish kernel has run: after a failed call nothing is
                # known about it -- drop it, the next armed call fills a fresh one
                _ws_cache.pop((dev.index, _stream_ptr(dev), "match_armed"), None)
            raise
        if adapt and not forced and ad["event"] is None and (ad["seen"] - 1) % self.ADAPT_PROBE_EVERY == 0:
            # this frame's rescue share: one tiny launch counts it straight into pinned host memory (device-visible), an event
            # says when it is there -- looked at by a later call, never waited for.  Every ADAPT_PROBE_EVERY-th filtered frame
            # only: a probe costs ~10 us of stream time, and what the share says changes with the clip, not with the frame.
            if ad["host"] is None:
                ad["host"] = _probe_slot()
            with _on(dev):
                _lib.call("manet_global_match_refine_rescued_async", ws.data_ptr(), N, C, self.n_ids, ad["host"].data_ptr(),
                          _stream_ptr(dev))
            ad["event"] = torch.cuda.Event()
            ad["event"].record(torch.cuda.current_stream(dev))  # (the stream the launches above went to: _stream_ptr(dev))
        return out

    def refine_stats(self):
        """compute='bf16r' / 'f16r': (candidate rows the filter pass appended, 1 if the candidate list overflowed and every pair
        scanned its object's rows instead) of the LAST match() on this bank; synchronises."""
        if self.compute not in _lib.REFINE_MODES or getattr(self, "_last", None) is None:
            raise RuntimeError("refine_stats: no compute='bf16r' / 'f16r' match has run on this bank")
        ws, N = self._last
        torch.cuda.current_stream(ws.device).synchronize()  # (the C call copies on the null stream, which torch's side streams do not block)
        return _lib.query("manet_global_match_refine_stats", ws.data_ptr(), N, self.C, self.n_ids, out=(ctypes.c_int64,) * 2)

    def refine_stats_full(self):
        """compute='bf16r' / 'f16r', the LAST match() on this bank (synchronises): dict with the candidate rows the filter pass
        listed, the overflow flag, and how many of the frame's 256-query tiles went through the rescue pass (the exact fp32
        kernel) -- `rescued_tile_fraction` is the distribution-dependent part of this mode's cost.  (The figures live in the
        stream-shared match workspace: read them before another such match runs on this stream.)"""
        if self.compute not in _lib.REFINE_MODES or getattr(self, "_last", None) is None:
            raise RuntimeError("refine_stats: no compute='bf16r' / 'f16r' match has run on this bank")
        ws, N = self._last
        torch.cuda.current_stream(ws.device).synchronize()  # (as refine_stats)
        s4 = (ctypes.c_int64 * 4)()
        _lib.call("manet_global_match_refine_stats2", ws.data_ptr(), N, self.C, self.n_ids, s4)
        return {"candidate_rows": int(s4[0]), "candidate_rows_per_pair": s4[0] / float(N * self.n_ids),
                "list_overflowed": int(s4[1]), "rescued_tiles": int(s4[2]), "query_tiles": int(s4[3]),
                "rescued_tile_fraction": s4[2] / float(max(1, s4[3]))}


class PackedQuery:
    """The query operand image of ONE frame (manet_query_pack): made once per frame of a clip -- the reference
    computes all embeddings of a clip up front (test.py:143-154) -- and matched against any number of banks /
    interaction rounds without a per-frame pack pass."""

    def __init__(self, query_embeddings, compute="f32"):
        _refuse_autograd("PackedQuery", query_embeddings)
        qry, N, C = _flat(query_embeddings, "query_embeddings")
        self.N, self.C, self.compute = N, C, COMPUTE[compute]
        self.image = torch.empty(_lib.query("manet_query_pack_bytes", N, C, self.compute), dtype=torch.uint8, device=qry.device)
        with _on(qry.device):
            _lib.call("manet_query_pack", qry.data_ptr(), _emb_code(qry), *qry.stride(), N, C, self.compute,
                      self.image.data_ptr(), self.image.numel(), _stream_ptr(qry.device))
        self.device = qry.device
        self.raw = query_embeddings  # (compute="bf16r" / "f16r": the exact re-rank reads the embedding itself)


class PreparedFrame:
    """The per-frame operands of ONE frame (manet_frame_prepare): the query operand image of the global match and, when
    `max_distance` >= 0, the padded 2x2-pooled plane (+ tile table) of the local match -- made from one read of the
    embedding, once per frame: a propagated frame then needs no pack pass and no pooling pass, and the previous frame's
    embedding is not read at all (its plane was made when it was the current frame, test.py:259)."""

    def __init__(self, ws, h, w, C, compute, max_distance, keep=None, raw=None):
        self.ws, self.h, self.w, self.C, self.compute, self.max_distance = ws, h, w, C, compute, max_distance
        self.raw = raw  # the [C, h, w] embedding as an [h, w, C] view (compute="bf16r" / "f16r" re-rank from it)
        self.N = h * w
        self.image = ws  # the operand image sits at the start of the frame workspace (a MANET_EMB_PACKED query)
        self.device = ws.device
        self.keep = keep  # whatever must stay alive with this object (the identity-keyed caches key on storage pointers)


def frame_workspace_bytes(h, w, C, compute="f32", max_distance=-1):
    return _lib.query("manet_frame_workspace_bytes", h, w, C, COMPUTE[compute], max_distance)


def prepare_frames(embeddings, compute="f32", max_distance=-1, preset=None, preset_value=1.0):
    """manet_frame_prepare on `embeddings` = [C, h, w] (one frame) or [B, C, h, w] (extract_feature's batch,
    IntVOS.py:578-581) in float32 / bfloat16 storage, any strides: ONE launch for the whole batch.  Returns a
    PreparedFrame (one frame) or a list of them.  `preset`: an optional contiguous float32 tensor set to `preset_value`
    by the same launch (the next local match's `out`, see local_match_frames)."""
    _need_gpu(embeddings, "embeddings")
    _refuse_autograd("prepare_frames", embeddings)
    emb = _emb(embeddings)
    single = emb.dim() == 3
    if single:
        emb = emb.unsqueeze(0)
    if emb.dim() != 4:
        raise ValueError("embeddings must be [C, h, w] or [B, C, h, w]")
    B, C, h, w = emb.shape
    if B == 0:
        return []
    cmp_ = COMPUTE[compute]
    per = frame_workspace_bytes(h, w, C, compute, max_distance)
    ws = torch.empty((B, per), dtype=torch.uint8, device=emb.device)
    fill_ptr, fill_words, fill_bits = None, 0, 0
    if preset is not None:
        _need_gpu(preset, "preset")
        if preset.dtype != torch.float32 or not preset.is_contiguous():
            raise ValueError("preset must be a contiguous float32 tensor")
        import struct
        fill_ptr, fill_words = preset.data_ptr(), preset.numel()
        fill_bits = struct.unpack("<I", struct.pack("<f", float(preset_value)))[0]
    with _on(emb.device):
        _lib.call("manet_frame_prepare", emb.data_ptr(), _emb_code(emb), emb.stride(0), emb.stride(2), emb.stride(3),
                  emb.stride(1), B, h, w, C, cmp_, max_distance, ws.data_ptr(), per, fill_ptr, fill_words, fill_bits,
                  _stream_ptr(emb.device))
    frames = [PreparedFrame(ws[i], h, w, C, cmp_, max_distance, raw=emb[i].permute(1, 2, 0)) for i in range(B)]
    return frames[0] if single else frames


def embed_finish(conv_out, scale, shift, relu=True, emb_dtype=torch.float32, compute="f32", max_distance=-1):
    """manet_embed_finish: the embedding layer's epilogue fused with the frame prepare (IntVOS.py:537-543, :578-581).
    conv_out [B, C, h, w] float32 = embedding_conv's raw output; scale / shift [C] = eval-mode bn2 folded (ops.fold_bn).
    ONE launch -> (embedding [B, C, h, w] in emb_dtype = relu(conv_out * scale + shift), list of PreparedFrames made from the
    embedding as stored -- bit-identical to prepare_frames(embedding))."""
    _need_gpu(conv_out, "conv_out")
    _refuse_autograd("embed_finish", conv_out, scale, shift)
    if conv_out.dim() != 4 or conv_out.dtype != torch.float32:
        raise ValueError("conv_out must be float32 [B, C, h, w]")
    B, C, h, w = conv_out.shape
    if emb_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("emb_dtype must be torch.float32 or torch.bfloat16")
    scale, shift = scale.detach().float().contiguous(), shift.detach().float().contiguous()
    if scale.numel() != C or shift.numel() != C:
        raise ValueError("scale / shift must have C elements")
    cmp_ = COMPUTE[compute]
    emb = torch.empty((B, C, h, w), dtype=emb_dtype, device=conv_out.device)
    if B == 0:
        return emb, []
    per = frame_workspace_bytes(h, w, C, compute, max_distance)
    ws = torch.empty((B, per), dtype=torch.uint8, device=conv_out.device)
    with _on(conv_out.device):
        _lib.call("manet_embed_finish", conv_out.data_ptr(), conv_out.stride(0), conv_out.stride(2), conv_out.stride(3),
                  conv_out.stride(1), scale.data_ptr(), shift.data_ptr(), int(bool(relu)), emb.data_ptr(), _emb_code(emb), B, h, w,
                  C, cmp_, max_distance, ws.data_ptr(), per, _stream_ptr(conv_out.device))
    frames = [PreparedFrame(ws[i], h, w, C, cmp_, max_distance, raw=emb[i].permute(1, 2, 0)) for i in range(B)]
    return emb, frames


def local_match_frames(prev_frame, cur_frame, prev_frame_labels, n_ids, out=None, out_is_preset=False):
    """local_previous_frame_nearest_neighbor_features_per_object (IntVOS.py:345-434, downsample configuration) on two
    PreparedFrames: the fused window / min kernel alone -> [h, w, n_ids]; bit-identical to local_match on the
    embeddings the frames were prepared from."""
    a, b = prev_frame, cur_frame
    if (a.h, a.w, a.C, _image_kind(a.compute), a.max_distance) != (b.h, b.w, b.C, _image_kind(b.compute), b.max_distance):
        raise ValueError("the two frames were prepared for different shapes / arithmetic / window radius")
    if b.max_distance < 0:
        raise ValueError("the frames were prepared without a pooled plane (max_distance < 0)")
    return _local_match_tail("manet_local_match_frames", a.ws, b, prev_frame_labels, n_ids, out, out_is_preset)


def _local_match_tail(symbol, source, b, prev_frame_labels, n_ids, out, out_is_preset):
    """the masked minimum of the local match over `source` (the previous PreparedFrame's workspace, or a stored volume) and the
    current PreparedFrame `b` -> [h, w, n_ids], into `out` if given"""
    lab =_labels(prev_frame_labels, "prev_frame_labels", b.h * b.w)
    if out is None:
        out = torch.empty((b.h, b.w, n_ids), dtype=torch.float32, device=b.device)
        out_is_preset = False
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != b.h * b.w * n_ids:
        raise ValueError("out must be a contiguous float32 tensor of h*w*n_ids elements")
    with _on(b.device):
        _lib.call(symbol, source.data_ptr(), b.ws.data_ptr(), lab.data_ptr(), b.h, b.w, b.C, b.compute, n_ids, b.max_distance,
                  out.data_ptr(), int(bool(out_is_preset)), _stream_ptr(b.device))
    return out.view(b.h, b.w, n_ids)


_VOLUME_SUFFIX = {torch.float32: "", torch.float16: "_f16"}


def _volume_suffix(dtype):
    try:
        return _VOLUME_SUFFIX[dtype]
    except KeyError:
        raise ValueError("stored volumes are torch.float32 or torch.float16, not %r" % (dtype,)) from None


def local_volume_bytes(h, w, max_distance, dtype=torch.float32):
    """bytes of one frame pair's stored window-distance volume (manet_local_volume_bytes; torch.float16: the half-precision
    storage type, manet_local_volume_bytes_f16 -- at most half the fp32 bytes plus one 1 KiB piece)"""
    return _lib.query("manet_local_volume_bytes" + _volume_suffix(dtype), h, w, max_distance)


def local_volumes(prev_frames, cur_frames, out=None, dtype=torch.float32):
    """The label-independent half of the local match (IntVOS.py:266-296: pooled frames -> (2d+1)^2 window distances ->
    (sigmoid - 0.5) * 2) for a BATCH of frame pairs (prev_frames[i], cur_frames[i]) -- lists of PreparedFrames of one geometry --
    in ceil(n / 32) launches.  Returns a `dtype` tensor [n, elements per volume]; row i feeds local_match_volume.  `out`: an
    optional contiguous tensor of that dtype and shape to write into.  dtype=torch.float16 (opt-in): the fp32 arithmetic, then
    every distance rounded once to half (to nearest even) -- half the bytes; local_match_volume on such a row stays within
    min(2^-12, 2^-11 * value) of the float32 route."""
    sfx = _volume_suffix(dtype)
    n = len(cur_frames)
    if len(prev_frames) != n:
        raise ValueError("prev_frames and cur_frames must pair up")
    if n == 0:
        return torch.empty((0, 0), dtype=dtype)
    b = cur_frames[0]
    for a in list(prev_frames) + list(cur_frames):
        if (a.h, a.w, a.C, _image_kind(a.compute), a.max_distance, a.device) != (b.h, b.w, b.C, _image_kind(b.compute),
                                                                               b.max_distance, b.device):
            raise ValueError("the frames were prepared for different shapes / arithmetic / window radius / devices")
    if b.max_distance < 0:
        raise ValueError("the frames were prepared without a pooled plane (max_distance < 0)")
    es = 4 if dtype == torch.float32 else 2
    per = local_volume_bytes(b.h, b.w, b.max_distance, dtype) // es
    if out is None:
        out = torch.empty((n, per), dtype=dtype, device=b.device)
    elif out.dtype != dtype or not out.is_contiguous() or tuple(out.shape) != (n, per) or out.device != b.device:
        raise ValueError("out must be a contiguous %s [%d, %d] tensor on the frames' device"
                         % (str(dtype).replace("torch.", ""), n, per))
    arr = ctypes.c_void_p * n
    pv = arr(*[f.ws.data_ptr() for f in prev_frames])
    cv = arr(*[f.ws.data_ptr() for f in cur_frames])
    vv = arr(*[out[i].data_ptr() for i in range(n)])
    with _on(b.device):
        _lib.call("manet_local_volume_frames" + sfx, pv, cv, vv, n, b.h, b.w, b.C, b.compute, b.max_distance, _stream_ptr(b.device))
    return out


def local_match_volume(volume, cur_frame, prev_frame_labels, n_ids, out=None, out_is_preset=False):
    """The label-dependent tail of the local match (IntVOS.py:398-432) on a stored volume (one row of local_volumes) -> [h, w,
    n_ids]; on a float32 row bit-identical to local_match_frames(prev_frame, cur_frame, ...) on the pair the volume was made
    from, on a float16 row (dispatch on volume.dtype) bit-identical to this function on the float32 row rounded to half."""
    b = cur_frame
    if b.max_distance < 0:
        raise ValueError("the frame was prepared without a pooled plane (max_distance < 0)")
    if (volume.dtype not in _VOLUME_SUFFIX or not volume.is_contiguous() or volume.device != b.device
            or volume.numel() * volume.element_size() != local_volume_bytes(b.h, b.w, b.max_distance, volume.dtype)):
        raise ValueError("volume must be one contiguous float32 (or float16) row of local_volumes() for this frame geometry")
    return _local_match_tail("manet_local_match_volume" + _VOLUME_SUFFIX[volume.dtype], volume, b, prev_frame_labels, n_ids, out,
                             out_is_preset)


def normalize_merge_(x, mem=None, normalize=True):
    """In place: x = (sigmoid(x)-0.5)*2 if normalize; if mem: x = mem = min(x, mem)
    (IntVOS.py:611-612, :620-622, :718-723)."""
    _refuse_autograd("normalize_merge_", x, mem)
    _need_gpu(x, "x")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("x must be contiguous float32")
    mem_ptr = _mem_ptr(mem, x.numel())
    with _on(x.device):
        _lib.call("manet_normalize_merge_f32", x.data_ptr(), mem_ptr, x.numel(), int(bool(normalize)), _stream_ptr(x.device))
    return x


def _hwc(t, name, allow_bf16=False):
    _need_gpu(t, name)
    if t.dim() != 3:
        raise ValueError("%s must be [height, width, embedding_dim]" % name)
    if allow_bf16 and t.dtype == torch.bfloat16:
        return t
    return t if t.dtype == torch.float32 else t.float()


def local_dist(x, y, max_distance, downsample=True):
    """local_pairwise_distances2(x=query, y=prev) (IntVOS.py:266-315) -> [h, w, (2d+1)^2]."""
    _refuse_autograd("local_dist", x, y)
    x = _hwc(x, "x")
    y = _hwc(y, "y")
    h, w, C = x.shape
    if tuple(y.shape) != (h, w, C):
        raise ValueError("x and y must have the same shape")
    dev = x.device
    P = 2 * max_distance + 1
    ws = _workspace(dev, "local", _lib.query("manet_local_workspace_bytes", h, w, C, max_distance, int(bool(downsample))))
    out = torch.empty((h, w, P * P), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.call("manet_local_dist_f32", *_strided(x), *_strided(y), h, w, C, max_distance, int(bool(downsample)),
                  out.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev))
    return out


def local_match(prev_frame_embedding, query_embedding, prev_frame_labels, n_ids, max_distance=12,
                downsample=True, deterministic=False):
    """local_previous_frame_nearest_neighbor_features_per_object (IntVOS.py:345-434) -> [h, w, n_ids].
    deterministic=True: when the call is differentiated, the ordered training route (csrc/match_train.hip): the same forward
    bits, a sparse backward without float atomics (the same gradient bits on every run)."""
    grad = _wants_grad(prev_frame_embedding, query_embedding)
    both_bf16 = (not grad and prev_frame_embedding.dtype == torch.bfloat16 and query_embedding.dtype == torch.bfloat16
                 and downsample)  # 2-byte embeddings are read as they are by the pooling pass (the training route is fp32)
    prev = _hwc(prev_frame_embedding, "prev_frame_embedding", both_bf16)
    cur = _hwc(query_embedding, "query_embedding", both_bf16)
    h, w, C = cur.shape
    if tuple(prev.shape) != (h, w, C):
        raise ValueError("prev_frame_embedding and query_embedding must have the same shape")
    lab = _labels(prev_frame_labels, "prev_frame_labels", h * w)
    if grad:
        from .autograd import LocalMatchFn, LocalMatchFullFn, LocalMatchOrderedFn, LocalMatchFullOrderedFn
        if deterministic:
            LocalMatchFn, LocalMatchFullFn = LocalMatchOrderedFn, LocalMatchFullOrderedFn
        return (LocalMatchFn if downsample else LocalMatchFullFn).apply(prev, cur, lab, n_ids, max_distance)
    dev = cur.device
    ws = _workspace(dev, "local", _lib.query("manet_local_workspace_bytes", h, w, C, max_distance, int(bool(downsample))))
    out = torch.empty((h, w, n_ids), dtype=torch.float32, device=dev)
    with _on(dev):
        _lib.call("manet_local_match_ex", *_strided(prev), *_strided(cur), _emb_code(cur), lab.data_ptr(), h, w, C, n_ids,
                  max_distance, int(bool(downsample)), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev))
    return out


def correlation_out_dims(H, W, pad_size, kernel_size, max_displacement, stride1, stride2):
    return _lib.query("manet_correlation_out_dims", H, W, pad_size, kernel_size, max_displacement, stride1, stride2,
                      out=(ctypes.c_int,) * 3)


def correlation_forward(input1, input2, pad_size, kernel_size, max_displacement, stride1, stride2):
    """correlation_cuda.forward (correlation_cuda.cc:10-87) -> [B, (2r+1)^2, outH, outW] in the inputs' dtype
    (float32 / float16 / float64; anything else is computed in float32)."""
    _need_gpu(input1, "input1")
    _need_gpu(input2, "input2")
    if _wants_grad(input1, input2):
        from .autograd import CorrelationFn
        return CorrelationFn.apply(input1, input2, pad_size, kernel_size, max_displacement, stride1, stride2)
    # the reference's forward dispatches float / double / half (correlation_cuda_kernel.cu:386-415)
    code = {torch.float32: 0, torch.float16: 1, torch.float64: 2}.get(input1.dtype)
    if code is None or input2.dtype != input1.dtype:
        input1, input2, code = input1.float(), input2.float(), 0
    a = input1.contiguous()
    b = input2.contiguous()
    if a.dim() != 4 or a.shape != b.shape:
        raise ValueError("input1 and input2 must be [B, C, H, W] of the same shape")
    B, C, H, W = a.shape
    oc, oh, ow = correlation_out_dims(H, W, pad_size, kernel_size, max_displacement, stride1, stride2)
    out = torch.empty((B, oc, oh, ow), dtype=a.dtype, device=a.device)
    with _on(a.device):
        _lib.call("manet_correlation_forward", a.data_ptr(), b.data_ptr(), code, B, C, H, W, pad_size, kernel_size,
                  max_displacement, stride1, stride2, out.data_ptr(), _stream_ptr(a.device))
    return out


def upsample_argmax(logits, size, want_small=True):
    """The mask step of the reference's driver in one launch:
    bilinear(align_corners) upsample of `logits` [1, n_ids, h, w] to `size`=(H, W) + argmax over ids
    (test.py:253-255) -> int64 [1, H, W]; and that mask nearest-resized back to (h, w) as the next
    frame's previous-frame label (IntVOS.py:598-599) -> int32 [1, 1, h, w] (None if not wanted)."""
    _need_gpu(logits, "logits")
    # integer outputs (argmax): nothing to differentiate, same as the reference's torch.argmax
    if logits.dim() != 4 or logits.shape[0] != 1:
        raise ValueError("logits must be [1, n_ids, h, w]")
    lg = logits.float().contiguous()
    _, n_ids, h, w = lg.shape
    H, W = int(size[0]), int(size[1])
    mask = torch.empty((1, H, W), dtype=torch.int64, device=lg.device)
    small = torch.empty((1, 1, h, w), dtype=torch.int32, device=lg.device) if want_small else None
    with _on(lg.device):
        _lib.call("manet_upsample_argmax", lg.data_ptr(), n_ids, h, w, H, W, mask.data_ptr(), _ptr(small), _stream_ptr(lg.device))
    return mask, small


def label_resize_nearest(mask, size):
    """F.interpolate(mask.float(), size=(h, w), mode='nearest').int() (IntVOS.py:598-599) in one launch.
    mask: integer [1, 1, H, W] (or [1, H, W] / [H, W]) -> int32 [1, 1, h, w]."""
    _need_gpu(mask, "mask")
    if mask.is_floating_point() or mask.numel() != mask.shape[-1] * mask.shape[-2]:
        raise ValueError("mask must be ONE integer image [.., H, W]")
    m = mask.to(torch.int64).contiguous()
    H, W = int(m.shape[-2]), int(m.shape[-1])
    h, w = int(size[0]), int(size[1])
    out = torch.empty((1, 1, h, w), dtype=torch.int32, device=m.device)
    with _on(m.device):
        _lib.call("manet_label_resize_nearest", m.data_ptr(), H, W, h, w, out.data_ptr(), _stream_ptr(m.device))
    return out


def frame_begin(mask, size, fill=None, fill_value=1.0, scalar_dst=None, scalar_value=0.0):
    """label_resize_nearest(mask, size) plus up to two small device writes in the SAME launch (manet_frame_begin): `fill` (a
    contiguous float32 tensor) := fill_value -- the local map's slot pre-set for the wide windows -- and the one-element float32
    tensor `scalar_dst` := scalar_value -- the frame's distance weight in the caller's table (IntVOS.py:641).  Each was a ~5 us
    launch of its own in a propagated frame.  Returns the int32 [1, 1, h, w] label."""
    _need_gpu(mask, "mask")
    if mask.is_floating_point() or mask.numel() != mask.shape[-1] * mask.shape[-2]:
        raise ValueError("mask must be ONE integer image [.., H, W]")
    m = mask.to(torch.int64).contiguous()
    H, W = int(m.shape[-2]), int(m.shape[-1])
    h, w = int(size[0]), int(size[1])
    for name, t, n in (("fill", fill, None), ("scalar_dst", scalar_dst, 1)):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != m.device or (n is not None and t.numel() != n)):
            raise ValueError("%s must be a contiguous float32 tensor on the mask's device%s" % (name, "" if n is None else " with one element"))
    out = torch.empty((1, 1, h, w), dtype=torch.int32, device=m.device)
    with _on(m.device):
        _lib.call("manet_frame_begin", m.data_ptr(), H, W, h, w, out.data_ptr(), _ptr(fill), 0 if fill is None else fill.numel(),
                  float(fill_value), _ptr(scalar_dst), float(scalar_value), _stream_ptr(m.device))
    return out


def head_layer1_object(global_map, local_map, labels, n_ids, size, dw_weight, dw_bias, bn_scale, bn_shift, w2t_object, b2, term,
                       relu_out=True):
    """DynamicSegHead layer 1, per-object half, in one launch (manet_head_layer1_object_f32): the per-object input channels
    (IntVOS.py:663-669) -> depthwise 7x7 + bn1 + relu1 -> 1x1 (3 -> 256, bn2 folded) + `term` (the shared-embedding half,
    [1, 256, h, w]) [+ relu2] -> [n_ids, 256, h, w].  The same bits as head_inputs + dwconv7x7_bn_relu + conv1x1_mfma(add=term)."""
    _refuse_autograd("head_layer1_object", global_map, local_map, term)
    _need_gpu(global_map, "global_map")
    h, w = int(size[0]), int(size[1])
    lab = labels.to(torch.int32).contiguous()
    g, l = global_map.contiguous(), local_map.contiguous()
    if g.dtype != torch.float32 or l.dtype != torch.float32 or g.numel() != h * w * n_ids or l.numel() != h * w * n_ids \
            or lab.numel() != h * w:
        raise ValueError("global_map / local_map must hold h*w*n_ids float32 values, labels h*w integers")
    wd = dw_weight.detach().float().contiguous()
    if wd.numel() != 3 * 49 or tuple(w2t_object.shape) != (3, PW_COUT) or term.numel() != PW_COUT * h * w:
        raise ValueError("the fused layer takes three per-object channels, 7x7 taps, %d output channels" % PW_COUT)
    opt = lambda t: None if t is None else t.detach().float().contiguous()  # noqa: E731
    db, sc, sh = opt(dw_bias), opt(bn_scale), opt(bn_shift)
    w2, bb, tm = w2t_object.contiguous(), b2.contiguous(), term.contiguous()
    for name, t in (("local_map", l), ("labels", lab), ("dw_weight", wd), ("dw_bias", db), ("bn_scale", sc), ("bn_shift", sh),
                    ("w2t_object", w2), ("b2", bb), ("term", tm)):
        if t is not None and t.device != g.device:
            raise ValueError("%s is on %s, global_map on %s" % (name, t.device, g.device))
    if w2.dtype != torch.float32 or bb.dtype != torch.float32 or tm.dtype != torch.float32 or bb.numel() != PW_COUT:
        raise ValueError("w2t_object [3, %d], b2 [%d] and term must be float32" % (PW_COUT, PW_COUT))
    if n_ids < 1:
        raise ValueError("n_ids must be positive")
    out = torch.empty((n_ids, PW_COUT, h, w), dtype=torch.float32, device=g.device)
    with _on(g.device):
        _lib.call("manet_head_layer1_object_f32", g.data_ptr(), l.data_ptr(), lab.data_ptr(), h, w, n_ids, wd.data_ptr(), _ptr(db),
                  _ptr(sc), _ptr(sh), w2.data_ptr(), bb.data_ptr(), tm.data_ptr(), int(bool(relu_out)), out.data_ptr(),
                  _stream_ptr(g.device))
    return out


def head_inputs(global_map, local_map, labels, n_ids, size):
    """The per-object channels of the head's input (IntVOS.py:663-669) in one launch:
    [n_ids, 3, h, w] = (global map of o, local map of o, labels == o), size = (h, w); global_map / local_map hold
    h*w*n_ids elements laid out [h, w, n_ids] (any view shape), labels h*w integers."""
    _refuse_autograd("head_inputs", global_map, local_map)
    _need_gpu(global_map, "global_map")
    lab = labels.to(torch.int32).contiguous()
    h, w = int(size[0]), int(size[1])
    if lab.numel() != h * w or global_map.numel() != h * w * n_ids or local_map.numel() != h * w * n_ids:
        raise ValueError("global_map / local_map must hold h*w*n_ids elements as [h, w, n_ids], labels h*w")
    g, l = global_map.float().contiguous(), local_map.float().contiguous()
    out = torch.empty((n_ids, 3, h, w), dtype=torch.float32, device=g.device)
    with _on(g.device):
        _lib.call("manet_head_inputs_f32", g.data_ptr(), l.data_ptr(), lab.data_ptr(), h * w, n_ids, out.data_ptr(),
                  _stream_ptr(g.device))
    return out


def fold_bn(bn):
    """eval-mode BatchNorm as per-channel (scale, shift): y = x * scale + shift"""
    inv = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
    g = bn.weight.detach().float() if bn.weight is not None else torch.ones_like(inv)
    b = bn.bias.detach().float() if bn.bias is not None else torch.zeros_like(inv)
    scale = g * inv
    return scale, b - bn.running_mean.detach().float() * scale


def dwconv7x7_bn_relu(x, weight, bias=None, bn=None, relu=True, scale=None, shift=None, relu_in=False):
    """Depthwise 7x7 conv (padding 3) + bias + eval-mode BatchNorm + ReLU in one HIP kernel
    (IntVOS.py:491-493,500-502: conv1 -> bn1 -> relu1 of _split_separable_conv2d).
    x [B, C, h, w] fp32; weight [C, 1, 7, 7]; bn: an nn.BatchNorm2d in eval mode, or explicit per-channel
    `scale` / `shift` (fold_bn), or neither.  relu_in: read the input through max(x, 0) (the preceding block's
    relu2 folded into this pass)."""
    _refuse_autograd("dwconv7x7_bn_relu", x, weight, bias, scale, shift)  # callers use it under no_grad only
    _need_gpu(x, "x")
    x = x.float().contiguous()
    B, C, h, w = x.shape
    if tuple(weight.shape) != (C, 1, 7, 7):
        raise ValueError("weight must be [C, 1, 7, 7]")
    wt = weight.detach().float().contiguous()
    if bn is not None:
        scale, shift = fold_bn(bn)
    if scale is not None:
        scale, shift = scale.float().contiguous(), shift.float().contiguous()
    bz = None if bias is None else bias.detach().float().contiguous()
    out = torch.empty_like(x)
    with _on(x.device):
        _lib.call("manet_dwconv7x7_bn_relu_ex", x.data_ptr(), B, C, h, w, wt.data_ptr(), _ptr(bz), _ptr(scale), _ptr(shift),
                  int(bool(relu)), int(bool(relu_in)), out.data_ptr(), _stream_ptr(x.device))
    return out


def _dwconv_check(x, weight, bias):
    _need_gpu(x, "x")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("x must be a float32 [B, C, h, w] tensor")
    C = x.shape[1]
    if weight.dim() != 4 or weight.shape[0] != C or weight.shape[1] != 1 or weight.shape[2] != weight.shape[3] \
            or weight.shape[2] not in (3, 7) or weight.dtype != torch.float32:
        raise ValueError("weight must be a float32 [C, 1, K, K] tensor with K = 3 or 7 (got %s for C = %d)"
                         % (tuple(weight.shape), C))
    if bias is not None and (bias.numel() != C or bias.dtype != torch.float32):
        raise ValueError("bias must be a float32 [C] tensor")
    return int(weight.shape[2])


def _dwconv_forward(x, weight, bias):
    """conv + bias on the HIP kernel (manet_dwconv_forward_f32); x, weight contiguous, no autograd"""
    B, C, h, w = x.shape
    K = int(weight.shape[2])
    bz = None if bias is None else bias.detach().contiguous()
    out = torch.empty_like(x)
    with _on(x.device):
        _lib.call("manet_dwconv_forward_f32", x.data_ptr(), B, C, h, w, K, weight.detach().data_ptr(), _ptr(bz), out.data_ptr(),
                  _stream_ptr(x.device))
    return out


def depthwise_conv2d(x, weight, bias=None):
    """F.conv2d(x, weight, bias, padding=K // 2, groups=C) on HIP kernels, differentiable: the heads' depthwise layers in
    training (IntVOS.py:491-493 _split_separable_conv2d.conv1, 7x7; :537 seperate_conv, 3x3).  x [B, C, h, w] fp32 on the GPU,
    weight [C, 1, K, K] with K = 3 or 7, bias [C] or None.  With grad wanted the op is autograd.DepthwiseConvFn (forward
    kernel; backward-data / backward-weight kernels), otherwise the forward kernel alone."""
    _dwconv_check(x, weight, bias)
    if _wants_grad(x, weight, bias):
        from .autograd import DepthwiseConvFn
        return DepthwiseConvFn.apply(x, weight, bias)
    return _dwconv_forward(x.contiguous(), weight.contiguous(), bias)


def _pw_check(x, weight, bias):
    _need_gpu(x, "x")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("x must be a float32 [B, Cin, h, w] tensor")
    Cin = x.shape[1]
    if weight.dim() != 4 or weight.shape[1] != Cin or weight.shape[2:] != (1, 1) or weight.dtype != torch.float32:
        raise ValueError("weight must be a float32 [Cout, Cin, 1, 1] tensor (got %s for Cin = %d)" % (tuple(weight.shape), Cin))
    if bias is not None and (bias.numel() != weight.shape[0] or bias.dtype != torch.float32):
        raise ValueError("bias must be a float32 [Cout] tensor")


@functools.lru_cache(maxsize=256)
def _ws_bytes(query, *dims):
    """_lib.query remembered per shape -- only for the workspace queries that are a function of the shape alone (no tuning knob)"""
    return _lib.query(query, *dims)


def _pw_forward(x, weight, bias):
    """W x + bias on the HIP kernels (manet_pw_forward_f32); x, weight contiguous, no autograd"""
    B, Cin, h, w = x.shape
    Cout = int(weight.shape[0])
    bz = None if bias is None else bias.detach().contiguous()
    out = torch.empty((B, Cout, h, w), dtype=torch.float32, device=x.device)
    nbytes = _ws_bytes("manet_pw_forward_workspace_bytes", B, Cin, Cout, h * w)
    with _on(x.device):
        ws = _workspace(x.device, "pw_forward", nbytes) if nbytes else None
        _lib.call("manet_pw_forward_f32", x.data_ptr(), B, Cin, Cout, h * w, weight.detach().data_ptr(), _ptr(bz), out.data_ptr(),
                  _ptr(ws), nbytes, _stream_ptr(x.device))
    return out


def pointwise_conv2d(x, weight, bias=None):
    """F.conv2d(x, weight, bias) for a 1x1 kernel on HIP kernels, differentiable: the heads' 1x1 convolutions in training
    (IntVOS.py:244-332 _split_separable_conv2d.conv2, the embedding head's embedding_conv).  x [B, Cin, h, w] fp32 on the GPU
    (any strides), weight [Cout, Cin, 1, 1], bias [Cout] or None.  With grad wanted the op is autograd.PointwiseConvFn (forward
    kernel; backward-data / backward-weight kernels), otherwise the forward kernel alone."""
    _pw_check(x, weight, bias)
    if _wants_grad(x, weight, bias):
        from .autograd import PointwiseConvFn
        return PointwiseConvFn.apply(x, weight, bias)
    return _pw_forward(x.contiguous(), weight.contiguous(), bias)


def batch_norm_relu_ok(bn):
    """bn is a BatchNorm2d batch_norm_relu takes: affine, tracking running statistics, a numeric momentum"""
    return (isinstance(bn, torch.nn.BatchNorm2d) and bn.affine and bn.track_running_stats and bn.momentum is not None
            and bn.running_mean is not None and bn.running_var is not None)


def _bn_relu_forward(x, weight, bias, running_mean, running_var, momentum, eps, training):
    """(out, save) of relu(batch_norm(x)) on the HIP kernels (manet_bn_relu_forward_f32), save [2, C] = the mean and invstd
    used; x contiguous"""
    B, C, h, w = x.shape
    dev = x.device
    out = torch.empty_like(x)
    save = torch.empty((2, C), dtype=torch.float32, device=dev)
    nbytes = _ws_bytes("manet_bn_relu_workspace_bytes", B, C, h * w)
    with _on(dev):
        ws = _workspace(dev, "bn_relu", nbytes)
        sp = save.data_ptr()
        _lib.call("manet_bn_relu_forward_f32", x.data_ptr(), B, C, h * w, weight.data_ptr(), bias.data_ptr(),
                  running_mean.data_ptr(), running_var.data_ptr(), float(momentum), float(eps), 1 if training else 0,
                  out.data_ptr(), sp, sp + 4 * C, ws.data_ptr(), nbytes, _stream_ptr(dev))
    return out, save


def batch_norm_relu(x, bn):
    """relu(bn(x)) on HIP kernels, differentiable: the heads' BatchNorm + ReLU pairs in training (IntVOS.py:244-332 bn1 -> relu1,
    bn2 -> relu2; the embedding head's).  x [B, C, h, w] fp32 on the GPU; bn an nn.BatchNorm2d with affine parameters, running
    statistics and a numeric momentum (batch_norm_relu_ok) whose parameters and buffers are fp32 on x's device.  bn.training
    selects batch statistics -- running_mean / running_var / num_batches_tracked updated as nn.BatchNorm2d does -- or the
    running ones.  With grad wanted the op is autograd.BatchNormReluFn, otherwise the forward kernels alone."""
    _need_gpu(x, "x")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("x must be a float32 [B, C, h, w] tensor")
    if not batch_norm_relu_ok(bn):
        raise ValueError("batch_norm_relu needs an affine BatchNorm2d with running statistics and a numeric momentum")
    C = x.shape[1]
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
        if t.numel() != C or t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous():
            raise ValueError("bn's parameters and running statistics must be contiguous fp32 [C] tensors on x's device")
    if bn.training:
        size = x.shape[0] * x.shape[2] * x.shape[3]
        if size == 1:  # nn.BatchNorm2d's own check (F.batch_norm -> _verify_batch_size)
            raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(x.size()))
        bn.num_batches_tracked.add_(1)
    if _wants_grad(x, bn.weight, bn.bias):
        from .autograd import BatchNormReluFn
        return BatchNormReluFn.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, bn.training)
    return _bn_relu_forward(x.contiguous(), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps,
                            bn.training)[0]


PW_COUT = 256  # output channels the MFMA 1x1 kernel is built for (the reference's MODEL_HEAD_EMBEDDING_DIM, config.py:48)


def fold_pointwise(conv2, bn2):
    """(w2t, b2) for conv1x1_mfma: conv2's [Cout, Cin, 1, 1] weight transposed to [Cin, Cout] with eval-mode bn2 folded
    in, and the folded bias [Cout]."""
    scale2, shift2 = fold_bn(bn2)
    w = conv2.weight.detach().float().reshape(conv2.out_channels, conv2.in_channels) * scale2[:, None]
    b2 = (conv2.bias.detach().float() * scale2 + shift2) if conv2.bias is not None else shift2
    return w.t().contiguous(), b2.contiguous()


def conv1x1_mfma_ok(x, cout):
    """shapes the MFMA 1x1 kernel takes: 256 output channels, any Cin, h*w a multiple of 4 (16-byte LDS-DMA rows)"""
    return (cout == PW_COUT and x.dim() == 4 and x.shape[1] >= 1 and (x.shape[2] * x.shape[3]) % 4 == 0
            and x.shape[2] * x.shape[3] >= 4)


def conv1x1_mfma(x, w2t, b2, relu_out=False, head_weight=None, head_bias=None, add=None):
    """conv2 -> bn2 [-> relu2] of a _split_separable_conv2d block (IntVOS.py:494,503-505) as an fp32-MFMA contraction fed by
    LDS-DMA (manet_conv1x1_f32).  x [B, Cin, h, w] fp32; w2t [Cin, 256], b2 [256] from fold_pointwise -> [B, 256, h, w].
    head_weight [1, 256, 1, 1] (+ head_bias [1]): DynamicSegHead's output layer Conv2d(256, 1, 1)(relu(.)) (IntVOS.py:519,525)
    fused into the epilogue -- returns [B, 1, h, w], the 256-channel activation is never written.
    add [256, h, w] / [1, 256, h, w] fp32: added to every batch entry before relu_out (layer1's shared-embedding half)."""
    return _conv1x1("conv1x1_mfma", x, w2t, b2, relu_out, add, head_weight, head_bias)


class SplitWeight:
    """A 1x1 layer's folded weight packed for conv1x1_split (manet_conv1x1_x3_pack / _x6_pack): the MFMA A-operand image of
    its bf16 pieces -- pieces=2: hi + lo (16 significand bits, three products per pair), pieces=3: hi + mid + lo (24 bits,
    six products: fp32-class).  `cin` input channels, PW_COUT output channels."""

    def __init__(self, w2t, pieces=2):
        lib = _lib.load()
        _need_gpu(w2t, "w2t")
        if pieces not in (2, 3):
            raise ValueError("pieces must be 2 or 3")
        w2t = w2t.detach().float().contiguous()
        if w2t.dim() != 2 or w2t.shape[1] != PW_COUT:
            raise ValueError("w2t must be [Cin, %d] (ops.fold_pointwise)" % PW_COUT)
        self.cin, self.pieces = int(w2t.shape[0]), int(pieces)
        nbytes, pack = ((lib.manet_conv1x1_x6_weight_bytes, lib.manet_conv1x1_x6_pack) if pieces == 3
                        else (lib.manet_conv1x1_x3_weight_bytes, lib.manet_conv1x1_x3_pack))
        self.packed = torch.empty(int(nbytes(self.cin)), dtype=torch.uint8, device=w2t.device)  # (returns the size, not a code)
        with _on(w2t.device):
            _lib.call(pack, w2t.data_ptr(), self.cin, PW_COUT, self.packed.data_ptr(), _stream_ptr(w2t.device))


def conv1x1_split_ok(x, cout):
    """shapes the split-bf16 1x1 kernel takes: 256 output channels, any Cin, h*w a multiple of 4"""
    return cout == PW_COUT and x.dim() == 4 and (x.shape[2] * x.shape[3]) % 4 == 0 and x.shape[2] * x.shape[3] >= 4


def conv1x1_split(x, weight, b2, relu_out=False, add=None, head_weight=None, head_bias=None):
    """conv2 -> bn2 [-> relu2] of a _split_separable_conv2d block (IntVOS.py:494,503-505) in split-bf16 arithmetic
    (manet_conv1x1_x3_f32: fp32 factors as hi + lo bf16 pieces, fp32 accumulation; <= 2^-16 relative per product; with a
    three-piece SplitWeight manet_conv1x1_x6_f32: hi + mid + lo, six products, ~2^-23 per product -- fp32-class).
    x [B, Cin, h, w] fp32; weight a SplitWeight; b2 [256] -> [B, 256, h, w].
    add [1, 256, h, w] (or [256, h, w]): added to every batch entry before relu_out -- layer1's shared-embedding half.
    head_weight / head_bias: DynamicSegHead's output layer fused (see conv1x1_mfma) -> [B, 1, h, w]."""
    return _conv1x1("conv1x1_split", x, weight, b2, relu_out, add, head_weight, head_bias)


F16_MAX = 65504.0  # the largest finite fp16: where the f16 head's stores saturate


def dwconv7x7_bn_relu_f16(x, weight, bias=None, bn=None, scale=None, shift=None):
    """dwconv7x7_bn_relu (relu on) with the output stored as fp16 (manet_dwconv7x7_bn_relu_f16; head_act="f16"): the same fp32
    fmaf chain on the input widened to fp32, then rn16(min(., 65504)) -- the fp32 kernel's result saturated and rounded once
    (a NaN stays a NaN).  x [B, C, h, w] fp32 (layer 1) or fp16 (layers 2-4), w even -> [B, C, h, w] fp16."""
    _refuse_autograd("dwconv7x7_bn_relu_f16", x, weight, bias, scale, shift)
    _need_gpu(x, "x")
    if x.dtype != torch.float16:
        x = x.float()
    x = x.contiguous()
    B, C, h, w = x.shape
    if tuple(weight.shape) != (C, 1, 7, 7):
        raise ValueError("weight must be [C, 1, 7, 7]")
    wt = weight.detach().float().contiguous()
    if bn is not None:
        scale, shift = fold_bn(bn)
    if scale is not None:
        scale, shift = scale.float().contiguous(), shift.float().contiguous()
    bz = None if bias is None else bias.detach().float().contiguous()
    out = torch.empty((B, C, h, w), dtype=torch.float16, device=x.device)
    with _on(x.device):
        _lib.call("manet_dwconv7x7_bn_relu_f16", x.data_ptr(), int(x.dtype == torch.float16), B, C, h, w, wt.data_ptr(), _ptr(bz),
                  _ptr(scale), _ptr(shift), out.data_ptr(), _stream_ptr(x.device))
    return out


class HalfWeight:
    """A 1x1 layer's folded weight rounded once to fp16 and packed for conv1x1_f16 (manet_conv1x1_f16_pack): the MFMA operand
    image, 8 KiB per 16 input channels.  `cin` input channels, PW_COUT output channels.  The caller checks that the folded
    weights are finite in fp16 (networks/IntVOS.py: a block whose weights are not is ineligible)."""

    def __init__(self, w2t):
        lib = _lib.load()
        _need_gpu(w2t, "w2t")
        w2t = w2t.detach().float().contiguous()
        if w2t.dim() != 2 or w2t.shape[1] != PW_COUT:
            raise ValueError("w2t must be [Cin, %d] (ops.fold_pointwise)" % PW_COUT)
        self.cin = int(w2t.shape[0])
        self.packed = torch.empty(int(lib.manet_conv1x1_f16_weight_bytes(self.cin)), dtype=torch.uint8, device=w2t.device)
        with _on(w2t.device):
            _lib.call("manet_conv1x1_f16_pack", w2t.data_ptr(), self.cin, PW_COUT, self.packed.data_ptr(), _stream_ptr(w2t.device))


def conv1x1_f16_ok(x, cout):
    """shapes the fp16 1x1 kernel takes: 256 output channels, any Cin, h*w a multiple of 8 (16-byte LDS-DMA rows of halves)"""
    return cout == PW_COUT and x.dim() == 4 and x.shape[1] >= 1 and (x.shape[2] * x.shape[3]) % 8 == 0 and x.shape[2] * x.shape[3] >= 8


def conv1x1_f16(x, weight, b2, relu_out=False, add=None, head_weight=None, head_bias=None, out_f32=False):
    """conv2 -> bn2 [-> relu2] of a _split_separable_conv2d block on fp16 activations (manet_conv1x1_f16; head_act="f16"): exact
    fp16 x fp16 products on the fp16 MFMA with fp32 accumulation, an fp32 epilogue (+ b2, + add, ReLU) and one rounding at the
    store, rn16(min(., 65504)).  x [B, Cin, h, w] fp16; weight a HalfWeight; b2 [256] fp32 -> [B, 256, h, w] fp16.
    add [1, 256, h, w] (or [256, h, w]) fp32: added unrounded to every batch entry before relu_out (layer 1's shared half).
    head_weight / head_bias: DynamicSegHead's output layer fused in fp32 (see conv1x1_mfma) -> [B, 1, h, w] fp32.
    out_f32: the result leaves as fp32, unrounded -- layer 1's shared-half term, which a later call takes as `add`."""
    return _conv1x1("conv1x1_f16", x, weight, b2, relu_out, add, head_weight, head_bias, out_f32)


def _conv1x1(name, x, weight, b2, relu_out, add, head_weight, head_bias, out_f32=False):
    """The one body of conv1x1_mfma / conv1x1_split / conv1x1_f16 (`name` says which): refuses autograd, checks and normalises
    the operands, allocates the output and makes the call.  What differs between the three is spelled out where it differs: the
    input's type (f16 takes fp16 as it is, the others convert to fp32), the weight (a checked fp32 [Cin, 256] tensor or a packed
    image), `add` (mfma refuses one that is not fp32 on x's device, the others convert) and the symbol with its argument order."""
    mfma, f16 = name == "conv1x1_mfma", name == "conv1x1_f16"
    _refuse_autograd(name, x, weight, b2, add, head_weight, head_bias)
    _need_gpu(x, "x")
    if not mfma and not isinstance(weight, HalfWeight if f16 else SplitWeight):
        raise TypeError("weight must be an ops.%s" % ("HalfWeight" if f16 else "SplitWeight"))
    if f16 and x.dtype != torch.float16:
        raise ValueError("x must be fp16 (the f16 depthwise kernel's output)")
    x = x.contiguous() if f16 else x.float().contiguous()
    B, cin, h, w = x.shape
    if mfma:
        if tuple(weight.shape) != (cin, PW_COUT) or b2.numel() != PW_COUT:
            raise ValueError("w2t must be [%d, %d] (ops.fold_pointwise), b2 [%d]" % (cin, PW_COUT, PW_COUT))
        wt = weight.detach().float().contiguous()
    else:
        if cin != weight.cin or b2.numel() != PW_COUT:
            raise ValueError("x has %d channels, the packed weight %d; b2 must be [%d]" % (cin, weight.cin, PW_COUT))
        wt = weight.packed
    if not _CONV1X1_OK[name](x, PW_COUT):
        raise ValueError("%s needs h*w to be a multiple of %d" % (name, 8 if f16 else 4))
    b2 = b2.detach().float().contiguous()
    if add is not None:
        if head_weight is not None:
            raise ValueError("add and the fused output layer are exclusive")
        if add.numel() != PW_COUT * h * w or (mfma and (add.dtype != torch.float32 or add.device != x.device)):
            raise ValueError("add must be [%d, h, w] fp32 on x's device" % PW_COUT if mfma else "add must be [1, %d, h, w]" % PW_COUT)
        add = add.contiguous() if mfma else add.detach().float().contiguous()
    hw = hb = hout = out = None
    if head_weight is not None:
        if head_weight.numel() != PW_COUT:
            raise ValueError("head_weight must be [1, %d, 1, 1]" % PW_COUT)
        hw = head_weight.detach().float().contiguous()
        hb = None if head_bias is None else head_bias.detach().float().contiguous()
        hout = torch.empty((B, 1, h, w), dtype=torch.float32, device=x.device)
    else:
        out = torch.empty((B, PW_COUT, h, w), dtype=torch.float16 if f16 and not out_f32 else torch.float32, device=x.device)
    relu = int(bool(relu_out))
    with _on(x.device):
        head = (x.data_ptr(), cin * h * w, B, cin, h * w, wt.data_ptr(), b2.data_ptr())  # (how every one of the symbols begins)
        stream = _stream_ptr(x.device)
        if f16:
            _lib.call("manet_conv1x1_f16", *head, _ptr(add), PW_COUT, relu, _ptr(out), int(bool(out_f32)), _ptr(hw), _ptr(hb),
                      _ptr(hout), stream)
        elif not mfma:  # (the weight's packing decides the symbol)
            _lib.call("manet_conv1x1_x6_f32" if weight.pieces == 3 else "manet_conv1x1_x3_f32", *head, _ptr(add), PW_COUT, relu,
                      _ptr(out), _ptr(hw), _ptr(hb), _ptr(hout), stream)
        elif add is not None:
            _lib.call("manet_conv1x1_add_f32", *head, add.data_ptr(), PW_COUT, relu, out.data_ptr(), stream)
        elif hw is not None:
            _lib.call("manet_conv1x1_head_f32", *head, PW_COUT, 0, None, hw.data_ptr(), _ptr(hb), hout.data_ptr(), stream)
        else:
            _lib.call("manet_conv1x1_f32", *head, PW_COUT, relu, out.data_ptr(), stream)
    return out if hout is None else hout


_CONV1X1_OK = {"conv1x1_mfma": conv1x1_mfma_ok, "conv1x1_split": conv1x1_split_ok, "conv1x1_f16": conv1x1_f16_ok}


def _conv1x1_of(weight):
    """the typed wrapper's name for a kernel weight: an fp32 [Cin, 256] tensor, a SplitWeight or a HalfWeight"""
    if isinstance(weight, torch.Tensor) and weight.dtype == torch.float32:
        return "conv1x1_mfma"
    if isinstance(weight, (SplitWeight, HalfWeight)):
        return "conv1x1_f16" if isinstance(weight, HalfWeight) else "conv1x1_split"
    raise TypeError("weight must be an fp32 [Cin, %d] tensor, an ops.SplitWeight or an ops.HalfWeight" % PW_COUT)


def conv1x1_ok(x, weight, cout=PW_COUT):
    """the kernel of `weight`'s type takes x's shape (conv1x1_mfma_ok / conv1x1_split_ok / conv1x1_f16_ok)"""
    return _CONV1X1_OK[_conv1x1_of(weight)](x, cout)


def conv1x1(x, weight, b2, relu_out=False, add=None, head_weight=None, head_bias=None, out_f32=False):
    """The 256-channel 1x1 stage on the kernel of `weight`'s type: an fp32 [Cin, 256] tensor -> conv1x1_mfma, a SplitWeight ->
    conv1x1_split, a HalfWeight -> conv1x1_f16 (x fp16; the only one that takes out_f32).  Anything else is a TypeError."""
    name = _conv1x1_of(weight)
    if out_f32 and name != "conv1x1_f16":
        raise ValueError("out_f32 is the f16 kernel's (an ops.HalfWeight)")
    return _conv1x1(name, x, weight, b2, relu_out, add, head_weight, head_bias, out_f32)


L1_F16_MAX_CP = 4  # per-object channels head_layer1_object_f16 takes (they share one k block of the MFMA)


def head_layer1_object_f16_ok(per_object):
    """shapes the fused per-object half of layer 1 takes: 1..4 per-object channels, w even, h*w a multiple of 8"""
    if per_object.dim() != 4:
        return False
    n, cp, h, w = per_object.shape
    return n >= 1 and 1 <= cp <= L1_F16_MAX_CP and w % 2 == 0 and (h * w) % 8 == 0 and h * w >= 8


def head_layer1_object_f16(per_object, dw_weight, dw_bias, scale, shift, weight, b2, term=None, relu_out=True):
    """DynamicSegHead layer 1, the per-object half under head_act="f16", in ONE launch (manet_head_layer1_object_f16): the bits
    of conv1x1_f16(dwconv7x7_bn_relu_f16(per_object, dw_weight, dw_bias, scale=scale, shift=shift), weight, b2,
    relu_out=relu_out, add=term) -- the same fp32 fmaf chains, one rounding to fp16, the same fp16 MFMA on a zero accumulator, the
    same fp32 epilogue and store -- without the [n, Cp, h, w] fp16 planes in between and with the term read once, not once per
    object.  per_object [n, Cp, h, w] fp32, Cp <= 4; dw_weight [Cp, 1, 7, 7]; dw_bias / scale / shift [Cp] or None; weight a
    HalfWeight of Cp input channels; b2 [256]; term [1, 256, h, w] (or [256, h, w]) fp32 or None -> [n, 256, h, w] fp16."""
    if not isinstance(weight, HalfWeight):
        raise TypeError("weight must be an ops.HalfWeight")
    _refuse_autograd("head_layer1_object_f16", per_object, dw_weight, dw_bias, scale, shift, b2, term)
    _need_gpu(per_object, "per_object")
    x = per_object.float().contiguous()
    if not head_layer1_object_f16_ok(x):
        raise ValueError("head_layer1_object_f16 needs [n, Cp <= %d, h, w] with w even and h*w a multiple of 8" % L1_F16_MAX_CP)
    n, cp, h, w = x.shape
    if tuple(dw_weight.shape) != (cp, 1, 7, 7):
        raise ValueError("dw_weight must be [Cp, 1, 7, 7]")
    if cp != weight.cin or b2.numel() != PW_COUT:
        raise ValueError("per_object has %d channels, the packed weight %d; b2 must be [%d]" % (cp, weight.cin, PW_COUT))
    wt = dw_weight.detach().float().contiguous()
    bz, scale, shift = [None if t is None else t.detach().float().contiguous() for t in (dw_bias, scale, shift)]
    if any(t is not None and t.numel() != cp for t in (bz, scale, shift)):
        raise ValueError("dw_bias / scale / shift must be [Cp]")
    b2 = b2.detach().float().contiguous()
    if term is not None:
        if term.numel() != PW_COUT * h * w:
            raise ValueError("term must be [1, %d, h, w]" % PW_COUT)
        term = term.detach().float().contiguous()
    out = torch.empty((n, PW_COUT, h, w), dtype=torch.float16, device=x.device)
    with _on(x.device):
        _lib.call("manet_head_layer1_object_f16", x.data_ptr(), n, cp, h, w, wt.data_ptr(), _ptr(bz), _ptr(scale), _ptr(shift),
                  weight.packed.data_ptr(), b2.data_ptr(), _ptr(term), int(bool(relu_out)), out.data_ptr(), _stream_ptr(x.device))
    return out


def relu_conv1x1_c1(x, weight, bias=None, relu_in=True):
    """DynamicSegHead's output layer in one pass over the activation (IntVOS.py:519,525): Conv2d(C, 1, 1) applied to
    max(x, 0) (relu_in) or to x.  x [B, C, h, w] fp32, weight [1, C, 1, 1], bias [1] or None -> [B, 1, h, w]."""
    _refuse_autograd("relu_conv1x1_c1", x, weight, bias)
    _need_gpu(x, "x")
    x = x.float().contiguous()
    B, C, h, w = x.shape
    if weight.numel() != C:
        raise ValueError("weight must be [1, C, 1, 1]")
    wt = weight.detach().float().contiguous()
    bz = None if bias is None else bias.detach().float().contiguous()
    out = torch.empty((B, 1, h, w), dtype=torch.float32, device=x.device)
    with _on(x.device):
        _lib.call("manet_relu_conv1x1_c1_f32", x.data_ptr(), B, C, h * w, wt.data_ptr(), _ptr(bz), int(bool(relu_in)),
                  out.data_ptr(), _stream_ptr(x.device))
    return out


def _out_conv_check(x, weight, bias):
    _need_gpu(x, "x")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("x must be a float32 [B, C, h, w] tensor")
    C = x.shape[1]
    if weight.dim() != 4 or tuple(weight.shape) != (1, C, 1, 1) or weight.dtype != torch.float32:
        raise ValueError("weight must be a float32 [1, C, 1, 1] tensor (got %s for C = %d)" % (tuple(weight.shape), C))
    if bias is not None and (bias.numel() != 1 or bias.dtype != torch.float32):
        raise ValueError("bias must be a float32 [1] tensor")


def _out_conv_forward(x, weight, bias):
    """bias + sum_c weight[c] x[:, c] on the HIP kernel (manet_out_conv_forward_f32); x, weight contiguous, no autograd"""
    B, C, h, w = x.shape
    bz = None if bias is None else bias.detach().contiguous()
    out = torch.empty((B, 1, h, w), dtype=torch.float32, device=x.device)
    with _on(x.device):
        _lib.call("manet_out_conv_forward_f32", x.data_ptr(), B, C, h * w, weight.detach().data_ptr(), _ptr(bz), out.data_ptr(),
                  _stream_ptr(x.device))
    return out


def output_conv1x1(x, weight, bias=None):
    """F.conv2d(x, weight, bias) for a [1, C, 1, 1] weight on HIP kernels, differentiable and deterministic: DynamicSegHead's
    output layer (IntVOS.py:516,524) in training.  x [B, C, h, w] fp32 on the GPU, bias [1] or None.  With grad wanted the op is
    autograd.OutputConvFn (forward kernel; one fixed-order reduction and one apply kernel backward), otherwise the forward kernel
    alone."""
    _out_conv_check(x, weight, bias)
    if _wants_grad(x, weight, bias):
        from .autograd import OutputConvFn
        return OutputConvFn.apply(x, weight, bias)
    return _out_conv_forward(x.contiguous(), weight.contiguous(), bias)


HEAD_BLOCK_TENSORS = ("conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var",
                      "conv2.weight", "conv2.bias", "bn2.weight", "bn2.bias", "bn2.running_mean", "bn2.running_var")


def dynamic_seghead_tensors(head):
    """the head's parameters and running statistics in the order of the C ABI's `params` (MANET_HEAD_PARAMS = 50 entries: twelve
    per block, HEAD_BLOCK_TENSORS, then conv.weight, conv.bias); a missing bias is None"""
    out = []
    for blk in (head.layer1, head.layer2, head.layer3, head.layer4):
        for name in HEAD_BLOCK_TENSORS:
            mod, attr = name.split(".")
            out.append(getattr(getattr(blk, mod), attr))
    return out + [head.conv.weight, head.conv.bias]


def dynamic_seghead_bns(head):
    """the head's eight BatchNorms in forward order"""
    return [bn for blk in (head.layer1, head.layer2, head.layer3, head.layer4) for bn in (blk.bn1, blk.bn2)]


def _head_train_params(head, shape):
    """what both one-node routes of a DynamicSegHead do in front of their autograd Function: F.batch_norm's batch-size check
    for an input of `shape` [B, C, h, w], and the 34 parameters in the order of dynamic_seghead_tensors without the running
    statistics (a missing bias: None)"""
    if any(bn.training for bn in dynamic_seghead_bns(head)) and shape[0] * shape[2] * shape[3] == 1:  # (_verify_batch_size)
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(torch.Size(shape)))
    tensors = dynamic_seghead_tensors(head)
    return [t for t, name in zip(tensors, HEAD_BLOCK_TENSORS * 4 + ("conv.weight", "conv.bias")) if "running" not in name]


def _head_train_count(head):
    """... and behind it: num_batches_tracked of the BatchNorms in training, as nn.BatchNorm2d.forward counts"""
    counters = [bn.num_batches_tracked for bn in dynamic_seghead_bns(head) if bn.training and bn.num_batches_tracked is not None]
    if counters:
        torch._foreach_add_(counters, 1)  # (one launch for the eight, not eight)


def dynamic_seghead_train(head, x):
    """head(x) for a DynamicSegHead (IntVOS.py:509-525) in training, as ONE differentiable op on HIP kernels: the four blocks
    and the output conv, forward and backward, sequenced in C (manet_head_train_forward_f32 / _backward_f32;
    autograd.DynamicSegHeadFn), the output conv fused with layer 4's last BatchNorm + ReLU.  x [B, Cin, h, w] fp32 on the GPU.
    Gradients for x and the head's 34 parameters -- only those that require one; the eight BatchNorms' running_mean /
    running_var / num_batches_tracked updated as nn.BatchNorm2d does, each BatchNorm's own .training selecting batch or running
    statistics.  Deterministic: the same bits for the same inputs.  The caller (DynamicSegHead.forward under
    train_kernels="fused") has checked every layer's eligibility (IntVOS._train_fused_ok)."""
    _need_gpu(x, "x")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("x must be a float32 [B, C, h, w] tensor")
    from .autograd import DynamicSegHeadFn
    out = DynamicSegHeadFn.apply(head, x, *_head_train_params(head, x.shape))
    _head_train_count(head)
    return out


def _head_input_operands(embedding, maps, label_planes, n_ids):
    """the assembly's operands, validated -> (embedding [C, h, w] fp32, [map0, map1] padded with None, tuple of flat int32 planes)"""
    _need_gpu(embedding, "embedding")
    if embedding.dim() != 3 or embedding.dtype != torch.float32:
        raise ValueError("embedding must be a float32 [C, h, w] tensor (a 2-byte embedding is widened by the caller)")
    C, h, w = embedding.shape
    maps, label_planes = list(maps), list(label_planes)
    if len(maps) > 2 or not 1 <= len(label_planes) <= 2:
        raise ValueError("the head input takes 0..2 maps and 1..2 label planes (got %d and %d)" % (len(maps), len(label_planes)))
    for j, m in enumerate(maps):
        _need_gpu(m, "maps[%d]" % j)
        if m.dtype != torch.float32 or m.numel() != h * w * n_ids or m.device != embedding.device:
            raise ValueError("maps[%d] must hold h*w*n_ids float32 values as [h, w, n_ids] on the embedding's device" % j)
    planes = tuple(_labels(t, "label_planes[%d]" % l, h * w) for l, t in enumerate(label_planes))
    return embedding, (maps + [None, None])[:2], planes


def head_input_train(embedding, maps, label_planes, n_ids, normalize_first=False):
    """The head's input in training (IntVOS.py:663-671, :741-758) in one launch and one autograd node (autograd.HeadInputFn,
    csrc/head_input_train.hip): x [n_ids, C + len(maps) + len(label_planes), h, w] = cat(embedding.unsqueeze(0).repeat(n_ids, 1,
    1, 1), each map permuted to [n_ids, 1, h, w], (labels == object).float() per plane).  embedding [C, h, w] fp32, any strides;
    maps: 0..2 float32 tensors of h*w*n_ids elements laid out [h, w, n_ids] (any view shape, as the match ops return them);
    label_planes: 1..2 integer tensors of h*w labels (a label outside 0..n_ids-1 marks no object).  normalize_first: maps[0]
    holds raw distances and goes through (sigmoid(d) - 0.5) * 2 on the way (ops.global_match(normalize=False) in front of it:
    the inference epilogue's bits).  Differentiable w.r.t. the embedding and the maps; only the gradients that are needed are
    computed."""
    emb, (map0, map1), planes = _head_input_operands(embedding, maps, label_planes, n_ids)
    from .autograd import HeadInputFn
    return HeadInputFn.apply(emb, map0, map1, planes, int(n_ids), bool(normalize_first))


def dynamic_seghead_train_parts(head, embedding, maps, label_planes, n_ids, normalize_first=False):
    """dynamic_seghead_train(head, head_input_train(embedding, maps, label_planes, n_ids, normalize_first)) as ONE autograd node
    (autograd.DynamicSegHeadPartsFn): the same kernels in the same order, hence the same bits -- logits [n_ids, 1, h, w], the
    head's parameter gradients, running statistics and num_batches_tracked, and the gradients of the embedding and the maps.
    With a frozen embedding and no differentiated map the head's input gradient is not computed at all.  The caller has checked
    the head's eligibility for the assembled input (IntVOS._train_fused_ok)."""
    emb, (map0, map1), planes = _head_input_operands(embedding, maps, label_planes, n_ids)
    C, h, w = emb.shape
    n_maps = (map0 is not None) + (map1 is not None)
    params = _head_train_params(head, (int(n_ids), C + n_maps + len(planes), h, w))
    from .autograd import DynamicSegHeadPartsFn
    out = DynamicSegHeadPartsFn.apply(head, emb, map0, map1, planes, int(n_ids), bool(normalize_first), *params)
    _head_train_count(head)
    return out


_LOSS_LABEL_DTYPES = (torch.int64, torch.int32, torch.uint8)
LOSS_MAX_CHANNELS = 64  # MANET_MAX_IDS


def upsampled_cross_entropy_ok(logits, labels, size=None):
    """the fused loss takes these: fp32 [B, C <= 64, h, w] logits and int64 / int32 / uint8 [B, H, W] labels on one HIP device, with
    (H, W) = `size` (default: the logits' own) no smaller than (h, w)"""
    if not (isinstance(logits, torch.Tensor) and isinstance(labels, torch.Tensor) and logits.is_cuda and labels.is_cuda):
        return False
    if logits.device != labels.device or logits.dtype != torch.float32 or labels.dtype not in _LOSS_LABEL_DTYPES:
        return False
    if logits.dim() != 4 or labels.dim() != 3 or logits.numel() == 0 or not 1 <= logits.shape[1] <= LOSS_MAX_CHANNELS:
        return False
    H, W = (int(size[0]), int(size[1])) if size is not None else (logits.shape[2], logits.shape[3])
    return (tuple(labels.shape) == (logits.shape[0], H, W) and logits.shape[2] <= H <= 16384 and logits.shape[3] <= W <= 16384)


def _loss_args(logits, labels, size):
    """the leading arguments every manet_loss_ce_* call shares: pointers, element strides, label element size, dimensions"""
    if not upsampled_cross_entropy_ok(logits, labels, size):
        _need_gpu(logits, "logits")
        _need_gpu(labels, "labels")
        raise ValueError("upsampled cross-entropy: logits must be float32 [B, C <= %d, h, w], labels int64 / int32 / uint8 [B, H, W] with "
                         "(H, W) = size >= (h, w) on the same device (got %s %s, %s %s, size %s)"
                         % (LOSS_MAX_CHANNELS, tuple(logits.shape), logits.dtype, tuple(labels.shape), labels.dtype, size))
    B, C, h, w = logits.shape
    H, W = int(size[0]), int(size[1])
    return (*_strided(logits), labels.data_ptr(), labels.element_size(), *labels.stride(), B, C, h, w, H, W)


def upsampled_cross_entropy_pixels(logits, labels, size):
    """F.cross_entropy(F.interpolate(logits, size, mode='bilinear', align_corners=True), labels, ignore_index=255,
    reduction='none') as [B, H*W], in one launch that never writes the upsampled logits (manet_loss_ce_pixels_f32).  No backward:
    the differentiable op is upsampled_cross_entropy_topk."""
    _refuse_autograd("upsampled_cross_entropy_pixels", logits)
    logits, labels = logits.detach(), labels.detach()
    args = _loss_args(logits, labels, size)
    out = torch.empty((logits.shape[0], int(size[0]) * int(size[1])), dtype=torch.float32, device=logits.device)
    with _on(logits.device):
        _lib.call("manet_loss_ce_pixels_f32", *args, out.data_ptr(), _stream_ptr(logits.device))
    return out


def _loss_forward(logits, labels, size, k, divisor):
    """manet_loss_ce_topk_forward_f32 -> (loss [], pixel_losses [B, H*W], stats int32 [3, B] = (bits of t, n_gt, n_eq))"""
    args = _loss_args(logits, labels, size)
    dev = logits.device
    B, H, W = logits.shape[0], int(size[0]), int(size[1])
    pix = torch.empty((B, H * W), dtype=torch.float32, device=dev)
    stats = torch.empty((3, B), dtype=torch.int32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    nbytes = _ws_bytes("manet_loss_ce_topk_workspace_bytes", B, H, W)
    with _on(dev):
        ws = _workspace(dev, "loss_ce_topk", nbytes)
        _lib.call("manet_loss_ce_topk_forward_f32", *args, int(k), float(divisor), pix.data_ptr(), loss.data_ptr(), stats.data_ptr(),
                  stats.data_ptr() + 4 * B, stats.data_ptr() + 8 * B, ws.data_ptr(), nbytes, _stream_ptr(dev))
    return loss, pix, stats


def upsampled_cross_entropy_topk(logits, labels, size, k, divisor=None, return_stats=False):
    """The training loss behind the head as one differentiable op (train_stage1.py:126-153 + networks/loss.py:44-81):
    mean(topk(cross_entropy(interpolate(logits, size, bilinear, align_corners=True), labels, ignore_index=255, 'none'), k, dim=1)).
    logits [B, C, h, w] fp32 (any strides), labels [B, H, W] int64 / int32 / uint8, size = (H, W), 1 <= k <= H * W; the sum of the
    selected losses is divided by `divisor` (default B * k: the reference's mean).  Returns a scalar.  With grad wanted for
    `logits` the op is autograd.UpsampledCrossEntropyTopKFn, otherwise the forward kernels alone.  Ties at the k-th loss share the
    remaining weight equally; see include/manet_hip.h.
    return_stats (no autograd): (loss, pixel_losses [B, H*W], t [B] = each row's k-th largest loss, n_gt [B] = #{loss > t},
    n_eq [B] = #{loss == t})."""
    k = int(k)
    if divisor is None:
        divisor = float(logits.shape[0] * k)
    if return_stats:
        _refuse_autograd("upsampled_cross_entropy_topk(return_stats=True)", logits)
        loss, pix, stats = _loss_forward(logits.detach(), labels, size, k, divisor)
        return loss, pix, stats[0].view(torch.float32), stats[1], stats[2]
    if _wants_grad(logits):
        from .autograd import UpsampledCrossEntropyTopKFn
        return UpsampledCrossEntropyTopKFn.apply(logits, labels, (int(size[0]), int(size[1])), k, float(divisor))
    return _loss_forward(logits.detach(), labels, size, k, divisor)[0]
