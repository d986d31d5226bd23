// The training loss behind the segmentation head, in one op -- what train_stage1.py:126-153 + networks/loss.py:44-81 run as a chain
// of framework calls:
//   F.interpolate(logits [B,C,h,w], (H,W), 'bilinear', align_corners=True) -> CrossEntropyLoss(ignore_index=255, reduction='none')
//   -> torch.topk(pixel_losses [B,H*W], k) -> mean, and the backward of all four.
// fp32.  The upsampled [B,C,H,W] logits and their gradient are never written, nothing is sorted, and no floating-point sum depends on
// an arrival order: the result and the gradient are the same bits for the same shape, every run.
//
//   loss_pixels_kernel     one thread per output pixel (8 pixels per thread, 2048 per workgroup): the 4 bilinear taps applied to every
//                          channel in registers, two sweeps over the channels (maximum, then sum of exponentials; the taps are
//                          re-read from L1 rather than kept in an array, so any C runs without scratch), loss = logsumexp - target.
//                          Labels outside 0..C-1 give loss 0.  The same launch counts the losses' top 11 bits into the row's first
//                          histogram (LDS counters, then one integer atomic per non-empty bin per workgroup).
//   loss_select_kernel<P>  radix select of the k-th largest loss of a row.  Losses are >= 0 (or the canonical NaN 0x7fc00000), so their
//                          bit patterns order as unsigned integers.  Digits of 11, 11 and 10 bits: pass P re-reads the finished
//                          histograms (every workgroup finds the earlier digits for itself: 2048 counters, a suffix scan in LDS) and
//                          counts digit P of the keys that match the prefix.  Integer atomics only: the counts do not depend on order.
//   loss_sum_kernel        finds the last digit -> t (the k-th largest loss, exact), n_gt = #{loss > t}, n_eq = #{loss == t}; per
//                          workgroup the sum of the losses > t, in double, in a fixed order, to a workspace slot.
//   loss_finish_kernel     one workgroup: adds each row's slots in ascending order, loss = sum_b (S_b + (k - n_gt_b) t_b) / divisor.
//   loss_backward_kernel<G>  d logits[b][c][y][x]: a group of G lanes (64, 16 or 1, by the size of the covering window) owns one
//                          low-resolution position, walks the high-resolution pixels whose taps touch it in a fixed order, recomputes
//                          softmax - onehot from the kept pixel loss (logsumexp = loss + target logit) and adds weight * tap
//                          coefficient * that through a fixed butterfly.  A gather: no atomics, no [B,C,H,W] intermediate.
//
// Source index: the real value dst * (in - 1) / (out - 1) that F.interpolate means, taken in integer arithmetic (quotient = lower tap,
// remainder / (out - 1) = its weight, correctly rounded) instead of aten's fp32 scale * dst, whose rounding moves a weight by up to
// 1e-5 at these sizes: the per-pixel loss stays within 16 ulp of the float64 composition.
#include "manet_common.h"

namespace {

constexpr int LT = 256;           // threads per workgroup, every kernel here
constexpr int LPB = 2048;         // pixels (keys) per workgroup of the pixel / select / sum kernels: 8 per thread
constexpr int LBINS = 2048;       // counters per histogram (11-bit digits; the last digit uses 1024 of them)
constexpr unsigned LNAN = 0x7fc00000u;

struct Tap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Tap tap_of(int dst, int in_size, int out_size)
{
    Tap t;
    if (in_size <= 1 || out_size <= 1) {
        t.i0 = t.i1 = 0;
        t.l0 = 1.0f;
        t.l1 = 0.0f;
        return t;
    }
    const unsigned den = (unsigned)(out_size - 1), num = (unsigned)dst * (unsigned)(in_size - 1);
    const unsigned a = num / den, r = num - a * den;
    t.i0 = (int)a;
    t.i1 = (int)a + ((int)a < in_size - 1 ? 1 : 0);
    t.l1 = (float)r / (float)den;
    t.l0 = (float)(den - r) / (float)den;
    return t;
}

// the 4 taps' element offsets inside one channel plane
struct Taps {
    long o00, o01, o10, o11;
    float ly0, ly1, lx0, lx1;
};
__device__ __forceinline__ Taps taps_of(const Tap &ty, const Tap &tx, long sy, long sx)
{
    Taps t;
    t.o00 = ty.i0 * sy + tx.i0 * sx;
    t.o01 = ty.i0 * sy + tx.i1 * sx;
    t.o10 = ty.i1 * sy + tx.i0 * sx;
    t.o11 = ty.i1 * sy + tx.i1 * sx;
    t.ly0 = ty.l0, t.ly1 = ty.l1, t.lx0 = tx.l0, t.lx1 = tx.l1;
    return t;
}
__device__ __forceinline__ float tap_value(const float *__restrict__ p, const Taps &t)
{
    const float r0 = fmaf(t.lx1, p[t.o01], t.lx0 * p[t.o00]);
    const float r1 = fmaf(t.lx1, p[t.o11], t.lx0 * p[t.o10]);
    return fmaf(t.ly1, r1, t.ly0 * r0);
}

__device__ __forceinline__ long long label_at(const void *__restrict__ labels, int elem, long off)
{
    if (elem == 8) return ((const long long *)labels)[off];
    if (elem == 4) return ((const int *)labels)[off];
    return ((const unsigned char *)labels)[off];
}

struct LossArgs {
    const float *logits;
    long l_sb, l_sc, l_sy, l_sx;
    const void *labels;
    int label_elem;
    long y_sb, y_sy, y_sx;
    int B, C, h, w, H, W;
};

__device__ __forceinline__ float pixel_loss(const LossArgs &a, int b, int Y, int X)
{
    const long long lab = label_at(a.labels, a.label_elem, b * a.y_sb + Y * a.y_sy + X * a.y_sx);
    if ((unsigned long long)lab >= (unsigned long long)a.C) return 0.0f;  // 255 (ignore_index) and anything else outside 0..C-1
    const Taps t = taps_of(tap_of(Y, a.h, a.H), tap_of(X, a.w, a.W), a.l_sy, a.l_sx);
    const float *p = a.logits + b * a.l_sb;
    float m = -INFINITY, vt = 0.0f;
    for (int c = 0; c < a.C; ++c) {
        const float v = tap_value(p + c * a.l_sc, t);
        m = (v > m || v != v) ? v : m;  // a NaN sticks
        if (c == (int)lab) vt = v;
    }
    float s = 0.0f;
    for (int c = 0; c < a.C; ++c) s += expf(tap_value(p + c * a.l_sc, t) - m);
    const float loss = (m + logf(s)) - vt;  // s >= 1, so logsumexp >= m >= vt: never negative
    return loss != loss ? __uint_as_float(LNAN) : loss;
}

__global__ __launch_bounds__(LT) void loss_pixels_kernel(LossArgs a, float *__restrict__ losses, unsigned *__restrict__ hist)
{
    __shared__ unsigned sh[LBINS];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long n = (long)a.H * a.W, base = (long)blockIdx.x * LPB;
    if (hist) {
        for (int i = tid; i < LBINS; i += LT) sh[i] = 0;
        __syncthreads();
    }
    for (int j = 0; j < LPB / LT; ++j) {
        const long i = base + j * LT + tid;
        if (i >= n) break;
        const int Y = (int)(i / a.W), X = (int)(i - (long)Y * a.W);
        const float loss = pixel_loss(a, b, Y, X);
        losses[b * n + i] = loss;
        if (hist) atomicAdd(&sh[__float_as_uint(loss) >> 21], 1u);
    }
    if (hist) {
        __syncthreads();
        unsigned *dst = hist + (long)b * 3 * LBINS;
        for (int i = tid; i < LBINS; i += LT)
            if (sh[i]) atomicAdd(&dst[i], sh[i]);
    }
}

// The bin that holds the k-th largest key of a finished histogram, counting from the top: `digit`, the number of keys in higher bins
// (`above` < k <= above + count) and the bin's own count.  All LT threads call it and all get the answer.  sh: LT + 3 words.
__device__ __forceinline__ void find_bin(const unsigned *__restrict__ hist, unsigned k, unsigned *sh, unsigned &digit, unsigned &above,
                                         unsigned &count)
{
    const int tid = threadIdx.x;
    unsigned c[LBINS / LT], own = 0;
#pragma unroll
    for (int j = 0; j < LBINS / LT; ++j) {
        c[j] = hist[tid * (LBINS / LT) + j];
        own += c[j];
    }
    sh[tid] = own;
    __syncthreads();
    for (int off = 1; off < LT; off <<= 1) {  // inclusive suffix sums
        const unsigned v = tid + off < LT ? sh[tid + off] : 0u;
        __syncthreads();
        sh[tid] += v;
        __syncthreads();
    }
    unsigned acc = sh[tid] - own;
    if (acc < k && k <= acc + own) {  // exactly one thread, as 1 <= k <= the histogram's total
#pragma unroll
        for (int j = LBINS / LT - 1; j >= 0; --j) {
            if (k > acc && k <= acc + c[j]) {
                sh[LT] = (unsigned)(tid * (LBINS / LT) + j);
                sh[LT + 1] = acc;
                sh[LT + 2] = c[j];
            }
            acc += c[j];
        }
    }
    __syncthreads();
    digit = sh[LT], above = sh[LT + 1], count = sh[LT + 2];
    __syncthreads();
}

template <int PASS>  // 2: counts bits 20..10 of the keys whose bits 31..21 match; 3: bits 9..0 of those whose bits 31..10 match
__global__ __launch_bounds__(LT) void loss_select_kernel(const unsigned *__restrict__ keys, long n, unsigned k,
                                                         unsigned *__restrict__ hist)
{
    __shared__ unsigned sh[LBINS];
    __shared__ unsigned fb[LT + 3];
    const int tid = threadIdx.x, b = blockIdx.y;
    unsigned *hb = hist + (long)b * 3 * LBINS;
    unsigned d, above, cnt, prefix;
    find_bin(hb, k, fb, d, above, cnt);
    prefix = d;
    if (PASS == 3) {
        find_bin(hb + LBINS, k - above, fb, d, above, cnt);
        prefix = (prefix << 11) | d;
    }
    for (int i = tid; i < LBINS; i += LT) sh[i] = 0;
    __syncthreads();
    const long base = (long)blockIdx.x * LPB;
    for (int j = 0; j < LPB / LT; ++j) {
        const long i = base + j * LT + tid;
        if (i >= n) break;
        const unsigned key = keys[b * n + i];
        if (PASS == 2) {
            if ((key >> 21) == prefix) atomicAdd(&sh[(key >> 10) & 2047u], 1u);
        } else {
            if ((key >> 10) == prefix) atomicAdd(&sh[key & 1023u], 1u);
        }
    }
    __syncthreads();
    unsigned *dst = hb + (PASS - 1) * LBINS;
    for (int i = tid; i < LBINS; i += LT)
        if (sh[i]) atomicAdd(&dst[i], sh[i]);
}

// fixed-order sum of one double per thread over the workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = LT / 2; off > 0; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(LT) void loss_sum_kernel(const unsigned *__restrict__ keys, long n, unsigned k,
                                                      const unsigned *__restrict__ hist, double *__restrict__ partial, int nblk,
                                                      float *__restrict__ t_out, int *__restrict__ n_gt_out, int *__restrict__ n_eq_out)
{
    __shared__ unsigned fb[LT + 3];
    __shared__ double red[LT];
    const int tid = threadIdx.x, b = blockIdx.y;
    const unsigned *hb = hist + (long)b * 3 * LBINS;
    unsigned d1, d2, d3, a1, a2, a3, cnt;
    find_bin(hb, k, fb, d1, a1, cnt);
    find_bin(hb + LBINS, k - a1, fb, d2, a2, cnt);
    find_bin(hb + 2 * LBINS, k - a1 - a2, fb, d3, a3, cnt);
    const unsigned t = (d1 << 21) | (d2 << 10) | d3;
    if (blockIdx.x == 0 && tid == 0) {
        t_out[b] = __uint_as_float(t);
        n_gt_out[b] = (int)(a1 + a2 + a3);
        n_eq_out[b] = (int)cnt;
    }
    const long base = (long)blockIdx.x * LPB;
    double s = 0.0;
    for (int j = 0; j < LPB / LT; ++j) {
        const long i = base + j * LT + tid;
        if (i >= n) break;
        const unsigned key = keys[b * n + i];
        if (key > t) s += (double)__uint_as_float(key);
    }
    s = block_sum(s, red);
    if (tid == 0) partial[(long)b * nblk + blockIdx.x] = s;
}

__global__ __launch_bounds__(LT) void loss_finish_kernel(const double *__restrict__ partial, int nblk, int B, unsigned k, float divisor,
                                                         const float *__restrict__ t, const int *__restrict__ n_gt,
                                                         float *__restrict__ loss_out)
{
    __shared__ double red[LT];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double s = 0.0;
        for (int i = tid; i < nblk; i += LT) s += partial[(long)b * nblk + i];
        s = block_sum(s, red);
        __syncthreads();
        total += s + (double)(k - (unsigned)n_gt[b]) * (double)t[b];
    }
    if (tid == 0) *loss_out = (float)(total / (double)divisor);
}

// The high-resolution indices whose taps touch low-resolution index y with a non-zero weight: lower tap y, or lower tap y - 1 with a
// remainder (H == h: the pixel itself and nothing else).
__device__ __forceinline__ void cover(int y, int in_size, int out_size, int &lo, int &cnt)
{
    if (in_size <= 1 || out_size <= 1) {
        lo = 0, cnt = out_size;
        return;
    }
    const long den = in_size - 1, o = out_size - 1;
    long first = y > 0 ? ((long)(y - 1) * o) / den + 1 : 0;        // smallest Y with Y * den > (y - 1) * o
    long last = ((long)(y + 1) * o + den - 1) / den - 1;           // largest Y with Y * den < (y + 1) * o
    if (last > o) last = o;
    lo = (int)first, cnt = (int)(last - first + 1);
}

template <int G>
__global__ __launch_bounds__(LT) void loss_backward_kernel(LossArgs a, unsigned k, float divisor, const unsigned *__restrict__ keys,
                                                           const float *__restrict__ t_in, const int *__restrict__ n_gt_in,
                                                           const int *__restrict__ n_eq_in, const float *__restrict__ grad_out,
                                                           float *__restrict__ grad_logits)
{
    const long e = ((long)blockIdx.x * LT + threadIdx.x) / G;  // low-resolution position (b, y, x)
    const int sub = threadIdx.x % G;
    const long plane = (long)a.h * a.w;
    if (e >= a.B * plane) return;  // whole groups leave together: LT % G == 0
    const int b = (int)(e / plane), y = (int)((e - b * plane) / a.w), x = (int)(e - b * plane - (long)y * a.w);
    const unsigned t = __float_as_uint(t_in[b]);
    const int n_gt = n_gt_in[b], n_eq = n_eq_in[b];
    const float w_eq = (float)((double)(k - (unsigned)n_gt) / (double)n_eq);
    const float scale = grad_out[0] / divisor;
    const long n = (long)a.H * a.W;
    int Y0, ny, X0, nx;
    cover(y, a.h, a.H, Y0, ny);
    cover(x, a.w, a.W, X0, nx);
    const int win = ny * nx;
    float *out = grad_logits + ((long)b * a.C * a.h + y) * a.w + x;
    const float *p = a.logits + b * a.l_sb;
    for (int i0 = 0; i0 < win; i0 += G) {
        const int i = i0 + sub;
        float wgt = 0.0f, lse = 0.0f;
        int lab = -1;
        Taps tp = {};
        if (i < win) {
            const int Y = Y0 + i / nx, X = X0 + i % nx;
            const unsigned key = keys[b * n + (long)Y * a.W + X];
            const long long l = label_at(a.labels, a.label_elem, b * a.y_sb + Y * a.y_sy + X * a.y_sx);
            const float sel = key > t ? 1.0f : (key == t ? w_eq : 0.0f);
            if (sel != 0.0f && (unsigned long long)l < (unsigned long long)a.C) {
                const Tap ty = tap_of(Y, a.h, a.H), tx = tap_of(X, a.w, a.W);
                const float cy = (ty.i0 == y ? ty.l0 : 0.0f) + (ty.i1 == y ? ty.l1 : 0.0f);
                const float cx = (tx.i0 == x ? tx.l0 : 0.0f) + (tx.i1 == x ? tx.l1 : 0.0f);
                tp = taps_of(ty, tx, a.l_sy, a.l_sx);
                lab = (int)l;
                wgt = sel * (cy * cx);
                lse = __uint_as_float(key) + tap_value(p + lab * a.l_sc, tp);
            }
        }
        for (int c = 0; c < a.C; ++c) {
            float g = 0.0f;
            if (wgt != 0.0f) g = wgt * (expf(tap_value(p + c * a.l_sc, tp) - lse) - (c == lab ? 1.0f : 0.0f));
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) g += __shfl_xor(g, off, G);
            if (sub == 0) {
                float *dst = out + (long)c * plane;
                *dst = (i0 == 0 ? 0.0f : *dst) + g * scale;
            }
        }
    }
}

int loss_check(const char *fn, int B, int C, int h, int w, int H, int W)
{
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
        return manet_set_error(MANET_E_INVALID, "%s: dimensions must be positive (B=%d C=%d h=%d w=%d H=%d W=%d)", fn, B, C, h, w, H, W);
    if (C > MANET_MAX_IDS) return manet_set_error(MANET_E_INVALID, "%s: C=%d > %d channels", fn, C, MANET_MAX_IDS);
    if (H < h || W < w) return manet_set_error(MANET_E_INVALID, "%s: the op upsamples: (H, W)=(%d, %d) < (h, w)=(%d, %d)", fn, H, W, h, w);
    if (H > 16384 || W > 16384 || B > 65535) return manet_set_error(MANET_E_INVALID, "%s: H, W <= 16384 and B <= 65535", fn);
    return MANET_OK;
}
int loss_check_labels(const char *fn, int elem)
{
    if (elem != 8 && elem != 4 && elem != 1)
        return manet_set_error(MANET_E_INVALID, "%s: labels are int64, int32 or uint8 (element size %d)", fn, elem);
    return MANET_OK;
}
int loss_check_k(const char *fn, int64_t k, int H, int W)
{
    if (k < 1 || k > (int64_t)H * W) return manet_set_error(MANET_E_INVALID, "%s: k=%lld outside 1..H*W=%lld", fn, (long long)k, (long long)H * W);
    return MANET_OK;
}
inline int loss_blocks(int H, int W) { return (int)(((long)H * W + LPB - 1) / LPB); }
inline size_t loss_hist_bytes(int B) { return manet_align_up((size_t)B * 3 * LBINS * sizeof(unsigned), 256); }
inline size_t loss_ws_bytes(int B, int H, int W) { return loss_hist_bytes(B) + (size_t)B * loss_blocks(H, W) * sizeof(double); }

}  // namespace

extern "C" int manet_loss_ce_topk_workspace_bytes(int B, int H, int W, size_t *bytes)
{
    if (B <= 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384 || B > 65535)
        return manet_set_error(MANET_E_INVALID, "manet_loss_ce_topk_workspace_bytes: dimensions must be positive, H, W <= 16384, B <= 65535");
    if (!bytes) return manet_set_error(MANET_E_INVALID, "manet_loss_ce_topk_workspace_bytes: NULL pointer");
    *bytes = loss_ws_bytes(B, H, W);
    return MANET_OK;
}

extern "C" int manet_loss_ce_pixels_f32(const float *logits, int64_t l_sb, int64_t l_sc, int64_t l_sy, int64_t l_sx, const void *labels,
                                        int label_elem_size, int64_t y_sb, int64_t y_sy, int64_t y_sx, int B, int C, int h, int w, int H,
                                        int W, float *pixel_losses, manet_stream_t stream)
{
    const char *fn = "manet_loss_ce_pixels_f32";
    int rc = loss_check(fn, B, C, h, w, H, W);
    if (!rc) rc = loss_check_labels(fn, label_elem_size);
    if (rc) return rc;
    if (!logits || !labels || !pixel_losses) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer", fn);
    LossArgs a = {logits, (long)l_sb, (long)l_sc, (long)l_sy, (long)l_sx, labels, label_elem_size, (long)y_sb, (long)y_sy, (long)y_sx,
                  B, C, h, w, H, W};
    hipLaunchKernelGGL(loss_pixels_kernel, dim3(loss_blocks(H, W), B), dim3(LT), 0, (hipStream_t)stream, a, pixel_losses, (unsigned *)nullptr);
    return manet_check_launch(fn);
}

extern "C" int manet_loss_ce_topk_forward_f32(const float *logits, int64_t l_sb, int64_t l_sc, int64_t l_sy, int64_t l_sx,
                                              const void *labels, int label_elem_size, int64_t y_sb, int64_t y_sy, int64_t y_sx, int B,
                                              int C, int h, int w, int H, int W, int64_t k, float divisor, float *pixel_losses,
                                              float *loss_out, float *t_out, int32_t *n_gt_out, int32_t *n_eq_out, void *ws,
                                              size_t ws_bytes, manet_stream_t stream)
{
    const char *fn = "manet_loss_ce_topk_forward_f32";
    int rc = loss_check(fn, B, C, h, w, H, W);
    if (!rc) rc = loss_check_labels(fn, label_elem_size);
    if (!rc) rc = loss_check_k(fn, k, H, W);
    if (rc) return rc;
    if (!logits || !labels || !pixel_losses || !loss_out || !t_out || !n_gt_out || !n_eq_out || !ws)
        return manet_set_error(MANET_E_INVALID, "%s: NULL pointer", fn);
    if (ws_bytes < loss_ws_bytes(B, H, W))
        return manet_set_error(MANET_E_INVALID, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, loss_ws_bytes(B, H, W));
    hipStream_t st = (hipStream_t)stream;
    unsigned *hist = (unsigned *)ws;
    double *partial = (double *)((char *)ws + loss_hist_bytes(B));
    const int nblk = loss_blocks(H, W);
    const long n = (long)H * W;
    const dim3 grid(nblk, B);
    LossArgs a = {logits, (long)l_sb, (long)l_sc, (long)l_sy, (long)l_sx, labels, label_elem_size, (long)y_sb, (long)y_sy, (long)y_sx,
                  B, C, h, w, H, W};
    if (hipMemsetAsync(hist, 0, (size_t)B * 3 * LBINS * sizeof(unsigned), st) != hipSuccess) return manet_check_launch(fn);
    hipLaunchKernelGGL(loss_pixels_kernel, grid, dim3(LT), 0, st, a, pixel_losses, hist);
    hipLaunchKernelGGL(loss_select_kernel<2>, grid, dim3(LT), 0, st, (const unsigned *)pixel_losses, n, (unsigned)k, hist);
    hipLaunchKernelGGL(loss_select_kernel<3>, grid, dim3(LT), 0, st, (const unsigned *)pixel_losses, n, (unsigned)k, hist);
    hipLaunchKernelGGL(loss_sum_kernel, grid, dim3(LT), 0, st, (const unsigned *)pixel_losses, n, (unsigned)k, (const unsigned *)hist,
                       partial, nblk, t_out, (int *)n_gt_out, (int *)n_eq_out);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(LT), 0, st, (const double *)partial, nblk, B, (unsigned)k, divisor,
                       (const float *)t_out, (const int *)n_gt_out, loss_out);
    return manet_check_launch(fn);
}

extern "C" int manet_loss_ce_topk_backward_f32(const float *logits, int64_t l_sb, int64_t l_sc, int64_t l_sy, int64_t l_sx,
                                               const void *labels, int label_elem_size, int64_t y_sb, int64_t y_sy, int64_t y_sx, int B,
                                               int C, int h, int w, int H, int W, int64_t k, float divisor, const float *pixel_losses,
                                               const float *t, const int32_t *n_gt, const int32_t *n_eq, const float *grad_out,
                                               float *grad_logits, manet_stream_t stream)
{
    const char *fn = "manet_loss_ce_topk_backward_f32";
    int rc = loss_check(fn, B, C, h, w, H, W);
    if (!rc) rc = loss_check_labels(fn, label_elem_size);
    if (!rc) rc = loss_check_k(fn, k, H, W);
    if (rc) return rc;
    if (!logits || !labels || !pixel_losses || !t || !n_gt || !n_eq || !grad_out || !grad_logits)
        return manet_set_error(MANET_E_INVALID, "%s: NULL pointer", fn);
    LossArgs a = {logits, (long)l_sb, (long)l_sc, (long)l_sy, (long)l_sx, labels, label_elem_size, (long)y_sb, (long)y_sy, (long)y_sx,
                  B, C, h, w, H, W};
    // lanes per low-resolution position, by the covering window of about (2 H/h + 1) x (2 W/w + 1) pixels
    const long win = (2L * ((H + h - 1) / h) + 1) * (2L * ((W + w - 1) / w) + 1);
    const long elems = (long)B * h * w;
    hipStream_t st = (hipStream_t)stream;
    const unsigned *keys = (const unsigned *)pixel_losses;
    if (H == h && W == w)  // every position is covered by its own pixel alone
        hipLaunchKernelGGL(loss_backward_kernel<1>, dim3((unsigned)((elems + LT - 1) / LT)), dim3(LT), 0, st, a, (unsigned)k, divisor, keys, t,
                           (const int *)n_gt, (const int *)n_eq, grad_out, grad_logits);
    else if (win <= 32)
        hipLaunchKernelGGL(loss_backward_kernel<16>, dim3((unsigned)((elems * 16 + LT - 1) / LT)), dim3(LT), 0, st, a, (unsigned)k, divisor,
                           keys, t, (const int *)n_gt, (const int *)n_eq, grad_out, grad_logits);
    else
        hipLaunchKernelGGL(loss_backward_kernel<64>, dim3((unsigned)((elems * 64 + LT - 1) / LT)), dim3(LT), 0, st, a, (unsigned)k, divisor,
                           keys, t, (const int *)n_gt, (const int *)n_eq, grad_out, grad_logits);
    return manet_check_launch(fn);
}
