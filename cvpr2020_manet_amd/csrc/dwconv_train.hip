// Depthwise convolution for TRAINING: forward, backward-data and backward-weight (+ bias) -- SURVEY.md 8f rank 3, the head's
// half: autograd through the depthwise layers of the heads, so that a training step (train_stage1.py:126-158) runs them on
// gfx950 kernels instead of the framework's grouped convolution.  The layers:
//   _split_separable_conv2d.conv1 (IntVOS.py:491-493): Conv2d(C, C, 7, padding 3, groups C), four per DynamicSegHead;
//   seperate_conv                 (IntVOS.py:537):     Conv2d(C, C, 3, padding 1, groups C), the embedding head.
// fp32, NCHW contiguous, stride 1, padding r = K / 2, K in {3, 7}, any B, C, h, w >= 1 (h or w < K included).
//
//   forward        out[b][c][y][x]    = bias[c] + sum_{ty,tx} w[c][ty][tx] * in[b][c][y+ty-r][x+tx-r]
//   backward-data  grad_in[b][c][y][x] = sum_{ty,tx} w[c][ty][tx] * grad_out[b][c][y-ty+r][x-tx+r]
//                                     = the forward's correlation of grad_out with the filter rotated by 180 degrees
//   backward-weight grad_w[c][ty][tx] = sum_{b,y,x} grad_out[b][c][y][x] * in[b][c][y+ty-r][x+tx-r],  grad_b[c] = sum grad_out[b][c]
// (zero padding everywhere).  The 7x7 forward is seg_head.hip's manet_dwconv7x7_bn_relu_ex without BN / ReLU: (conv + bias) * 1 + 0,
// exact.  Everything else is here:
//  * dw_corr_kernel<K, FLIP>: a workgroup owns one 128 x 32 output tile of one (b, c) plane; the input tile with its r-pixel halo is
//    staged in LDS (all loads of a thread issued first, from clamped addresses, zeros selected afterwards); a thread owns 4 rows x 4
//    columns and reads each of its 4 + K - 1 input rows as aligned ds_read_b128 once, for up to 4 x 4 x K fmaf.  Tap order per
//    output: ty outer, tx inner, one fmaf chain from zero, then + bias.  FLIP reads w[K*K-1-t] (backward-data).
//  * dw_wgrad_kernel<K>: 64 x 64 tiles; a workgroup owns (tile, channel, batch slice) and walks the slice's items, a thread keeps
//    K*K + 1 running sums over its 16 pixels, the next item's input loads in flight under the current item's arithmetic.  The
//    256 threads' sums meet in LDS in a fixed order and go to a workspace slot per (channel, tile, slice); dw_wgrad_finish_kernel
//    adds the slots of a channel in ascending order.  No atomics: the result depends on the shape alone, bit for bit.
// Blocks are mapped XCD-aware as in seg_head.hip's depthwise kernel: all tiles of a plane on one XCD (block L runs on XCD L % 8),
// so the halo lines two neighbouring tiles share are hits in that XCD's L2.
#include "manet_common.h"

namespace {

// TX_: tile columns; 256 threads of 4 x 4 outputs: TX_ / 4 column groups x 1024 / TX_ row groups.  The correlation uses 128 x 32
// tiles (480p's 214 columns: 7 tiles, 5 % idle; 64 x 64 tiles idled 20 % of their columns), the weight gradient 64 x 64 ones (its
// workgroups walk the batch, and 8 tiles x 256 channels keep every item in one workgroup at 480p)
template <int K, int TX_>
struct DwTrain {
    static constexpr int R = K / 2;
    static constexpr int TX = TX_, RY = 4, CG = TX / 4, TY = RY * (256 / CG);
    static constexpr int HY = TY + 2 * R, HX = TX + 2 * R;        // staged tile (with halo)
    static constexpr int NV = (4 + K - 1 + 3) / 4;                // b128 reads per window row (4 outputs + K - 1 halo columns)
    static constexpr int LW = (4 * (CG - 1) + 4 * NV > HX ? 4 * (CG - 1) + 4 * NV : (HX + 3) / 4 * 4);  // LDS row pitch (floats)
    static constexpr int NS = (HY * HX + 255) / 256;              // staged elements per thread
    static constexpr int NT = K * K + 1;                          // backward-weight sums per thread (taps + bias)
    static constexpr int RP = 260, RCH = 16;                      // reduction: row pitch (4 x 65 floats), taps per round
    static constexpr int LDS = (HY * LW > RCH * RP ? HY * LW : RCH * RP);
};

template <typename T>
__device__ __forceinline__ void dw_stage_issue(float (&v)[T::NS], const float *__restrict__ src, int h, int w, int x0, int y0)
{
#pragma unroll
    for (int s = 0; s < T::NS; ++s) {
        const int i = threadIdx.x + 256 * s;
        const int p = i / T::HX, q = i - p * T::HX;
        const int yc = min(max(y0 - T::R + p, 0), h - 1), xc = min(max(x0 - T::R + q, 0), w - 1);
        v[s] = src[yc * w + xc];  // (clamped: always inside the plane; the padding is selected in dw_stage_store)
    }
}

template <typename T>
__device__ __forceinline__ void dw_stage_store(float *__restrict__ tile, const float (&v)[T::NS], int h, int w, int x0, int y0)
{
#pragma unroll
    for (int s = 0; s < T::NS; ++s) {
        const int i = threadIdx.x + 256 * s;
        const int p = i / T::HX, q = i - p * T::HX;
        const int yy = y0 - T::R + p, xx = x0 - T::R + q;
        const bool ok = yy >= 0 && yy < h && xx >= 0 && xx < w;
        if (i < T::HY * T::HX) tile[p * T::LW + q] = ok ? v[s] : 0.0f;
    }
}

// LDS-only barrier (no wait for outstanding global stores / loads)
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// window of a thread's input row: LDS columns 4 tg .. 4 tg + 4 NV - 1
template <typename T>
__device__ __forceinline__ void dw_window(float (&win)[4 * T::NV], const float *__restrict__ row)
{
#pragma unroll
    for (int i = 0; i < T::NV; ++i) {
        const f32x4 u = *(const f32x4 *)(row + 4 * i);
        win[4 * i] = u[0], win[4 * i + 1] = u[1], win[4 * i + 2] = u[2], win[4 * i + 3] = u[3];
    }
}

template <int K, bool FLIP>
__global__ __launch_bounds__(256) void dw_corr_kernel(const float *__restrict__ in, int P, int C, int h, int w,
                                                      const float *__restrict__ weight, const float *__restrict__ bias,
                                                      float *__restrict__ out, int ntx, int ntile, int vec)
{
    using T = DwTrain<K, 32>;
    const int xcd_ = blockIdx.x & 7, j_ = blockIdx.x >> 3;
    const int tile_ = j_ % ntile, plane = (j_ / ntile) * 8 + xcd_;
    if (plane >= P) return;
    __shared__ __attribute__((aligned(16))) float tile[T::LDS];
    const int c = plane % C;
    const int x0 = (tile_ % ntx) * T::TX, y0 = (tile_ / ntx) * T::TY;
    const long base = (long)plane * h * w;
    float v[T::NS];
    dw_stage_issue<T>(v, in + base, h, w, x0, y0);
    dw_stage_store<T>(tile, v, h, w, x0, y0);
    lds_barrier();

    const float *wk = weight + (long)c * K * K;
    float wr[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wr[t] = wk[FLIP ? K * K - 1 - t : t];
    const int tid = threadIdx.x, t = tid / T::CG, tg = tid - t * T::CG;
    float acc[T::RY][4];
#pragma unroll
    for (int r = 0; r < T::RY; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = 0.0f;
#pragma unroll
    for (int ir = 0; ir < T::RY + K - 1; ++ir) {
        float win[4 * T::NV];
        dw_window<T>(win, tile + (T::RY * t + ir) * T::LW + 4 * tg);
#pragma unroll
        for (int r = 0; r < T::RY; ++r) {
            const int ky = ir - r;
            if (ky < 0 || ky >= K) continue;
#pragma unroll
            for (int kx = 0; kx < K; ++kx)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[r][j] = fmaf(win[j + kx], wr[ky * K + kx], acc[r][j]);
        }
    }
    const float bc = bias ? bias[c] : 0.0f;
    const int x = x0 + 4 * tg;
#pragma unroll
    for (int r = 0; r < T::RY; ++r) {
        const int y = y0 + T::RY * t + r;
        if (y >= h) break;
        float *dst = out + base + (long)y * w + x;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = bias ? acc[r][j] + bc : acc[r][j];
        if (vec && x + 3 < w) {  // w even, plane 8-byte aligned
            *(f32x2 *)dst = f32x2{o[0], o[1]};
            *(f32x2 *)(dst + 2) = f32x2{o[2], o[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < w) dst[j] = o[j];
        }
    }
}

template <int K>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const float *__restrict__ in, const float *__restrict__ gout, int B, int C,
                                                       int h, int w, int ntx, int ntile, int nbs, float *__restrict__ ws)
{
    using T = DwTrain<K, 64>;
    const int xcd_ = blockIdx.x & 7, j_ = blockIdx.x >> 3;
    const int tile_ = j_ % ntile, z = (j_ / ntile) * 8 + xcd_;
    if (z >= C * nbs) return;
    __shared__ __attribute__((aligned(16))) float tile[T::LDS];
    __shared__ float red2[4 * T::RCH];
    const int c = z / nbs, bs = z - c * nbs;
    const int b_first = (int)((long)bs * B / nbs), b_end = (int)((long)(bs + 1) * B / nbs);
    const int x0 = (tile_ % ntx) * T::TX, y0 = (tile_ / ntx) * T::TY;
    const long plane = (long)h * w;
    const int tid = threadIdx.x, t = tid / T::CG, tg = tid - t * T::CG;
    const int x = x0 + 4 * tg;
    float acc[T::NT];
#pragma unroll
    for (int k = 0; k < T::NT; ++k) acc[k] = 0.0f;
    float v[T::NS];
    dw_stage_issue<T>(v, in + ((long)b_first * C + c) * plane, h, w, x0, y0);
    for (int b = b_first; b < b_end; ++b) {
        // this thread's grad_out pixels (clamped loads, zero outside the image)
        const float *gsrc = gout + ((long)b * C + c) * plane;
        float g[T::RY][4];
#pragma unroll
        for (int r = 0; r < T::RY; ++r) {
            const int y = y0 + T::RY * t + r, yc = min(y, h - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) g[r][j] = gsrc[yc * w + min(x + j, w - 1)];
        }
#pragma unroll
        for (int r = 0; r < T::RY; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (y0 + T::RY * t + r >= h || x + j >= w) g[r][j] = 0.0f;
        dw_stage_store<T>(tile, v, h, w, x0, y0);
        lds_barrier();
        if (b + 1 < b_end) dw_stage_issue<T>(v, in + ((long)(b + 1) * C + c) * plane, h, w, x0, y0);  // under this item's arithmetic
#pragma unroll
        for (int ir = 0; ir < T::RY + K - 1; ++ir) {
            float win[4 * T::NV];
            dw_window<T>(win, tile + (T::RY * t + ir) * T::LW + 4 * tg);
#pragma unroll
            for (int r = 0; r < T::RY; ++r) {
                const int ty = ir - r;
                if (ty < 0 || ty >= K) continue;
#pragma unroll
                for (int tx = 0; tx < K; ++tx)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[ty * K + tx] = fmaf(g[r][j], win[j + tx], acc[ty * K + tx]);
            }
        }
#pragma unroll
        for (int r = 0; r < T::RY; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[K * K] += g[r][j];
        lds_barrier();  // (the next item's staging overwrites the tile)
    }
    // the workgroup's sums, in a fixed order: thread tid's value of tap k at red[k][tid / 64][tid % 64] (rows of 4 x 65 floats: the 64
    // readers -- 16 taps x 4 quarters -- hit 64 distinct banks); a reader adds its quarter's 64 values in ascending order, one
    // thread per tap adds the four quarters
    float *red = tile;
    float *dst = ws + ((long)c * ntile * nbs + (long)tile_ * nbs + bs) * T::NT;
#pragma unroll
    for (int t0 = 0; t0 < T::NT; t0 += T::RCH) {
#pragma unroll
        for (int k = 0; k < T::RCH; ++k)
            if (t0 + k < T::NT) red[k * T::RP + (tid >> 6) * 65 + (tid & 63)] = acc[t0 + k];
        lds_barrier();
        if (tid < 4 * T::RCH) {
            const int tap = tid >> 2, qd = tid & 3;
            float s = 0.0f;
            if (t0 + tap < T::NT) {
                const float *src = red + tap * T::RP + qd * 65;
                for (int i = 0; i < 64; ++i) s += src[i];
            }
            red2[tid] = s;
        }
        lds_barrier();
        if (tid < T::RCH && t0 + tid < T::NT)
            dst[t0 + tid] = (red2[4 * tid] + red2[4 * tid + 1]) + (red2[4 * tid + 2] + red2[4 * tid + 3]);
        lds_barrier();  // (the next round overwrites red / red2)
    }
}

// grad_w[c][k] / grad_b[c] = sum over the channel's workspace slots, ascending
template <int K>
__global__ __launch_bounds__(256) void dw_wgrad_finish_kernel(const float *__restrict__ ws, int C, int nslot, float *__restrict__ grad_w,
                                                              float *__restrict__ grad_b)
{
    constexpr int NT = K * K + 1;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)C * NT) return;
    const int c = (int)(i / NT), k = (int)(i - (long)c * NT);
    const float *src = ws + (long)c * nslot * NT + k;
    float s = 0.0f;
    for (int n = 0; n < nslot; ++n) s += src[(long)n * NT];
    if (k < K * K) grad_w[(long)c * K * K + k] = s;
    else if (grad_b) grad_b[c] = s;
}

struct WgradGeom {
    int ntx, ntile, nbs;
    long nblocks, slots;  // workgroups of dw_wgrad_kernel; workspace slots (each K*K + 1 floats)
};

// batch slices: enough (tile, channel, slice) workgroups for the chip (~8 per CU) without splitting an item; a function of the
// shape alone, so the summation order -- and the bits -- are too
WgradGeom wgrad_geom(int B, int C, int h, int w)
{
    using T = DwTrain<3, 64>;  // (the same tiles for both K)
    WgradGeom g;
    g.ntx = (w + T::TX - 1) / T::TX;
    g.ntile = g.ntx * ((h + T::TY - 1) / T::TY);
    const long per = (long)g.ntile * C;
    long nbs = (2048 + per - 1) / per;
    g.nbs = (int)(nbs < 1 ? 1 : nbs > B ? B : nbs);
    g.nblocks = 8L * g.ntile * (((long)C * g.nbs + 7) / 8);
    g.slots = per * g.nbs;
    return g;
}

template <int K, bool FLIP>
int launch_corr(const float *in, int B, int C, int h, int w, const float *weight, const float *bias, float *out, hipStream_t st)
{
    using T = DwTrain<K, 32>;
    const int ntx = (w + T::TX - 1) / T::TX, ntile = ntx * ((h + T::TY - 1) / T::TY);
    const long P = (long)B * C;
    const long nblocks = 8L * ntile * ((P + 7) / 8);
    if (P > 0x7fffffffL || nblocks > 0x7fffffffL) return manet_set_error(MANET_E_INVALID, "too many tiles for one launch");
    const int vec = (w % 2 == 0 && ((size_t)out & 7) == 0) ? 1 : 0;
    hipLaunchKernelGGL((dw_corr_kernel<K, FLIP>), dim3((unsigned)nblocks), dim3(256), 0, st, in, (int)P, C, h, w, weight, bias, out,
                       ntx, ntile, vec);
    return MANET_OK;
}

int check_dims(const char *what, int B, int C, int h, int w, int K)
{
    if (K != 3 && K != 7) return manet_set_error(MANET_E_INVALID, "%s: K=%d (3 or 7)", what, K);
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0)
        return manet_set_error(MANET_E_INVALID, "%s: sizes must be positive (B=%d C=%d h=%d w=%d)", what, B, C, h, w);
    if ((long)h * w > 0x7fffffffL) return manet_set_error(MANET_E_INVALID, "%s: h*w must fit in 31 bits", what);
    return MANET_OK;
}

}  // namespace

extern "C" int manet_dwconv_forward_f32(const float *in, int B, int C, int h, int w, int K, const float *weight, const float *bias,
                                        float *out, manet_stream_t stream)
{
    int rc = check_dims("manet_dwconv_forward_f32", B, C, h, w, K);
    if (rc) return rc;
    if (!in || !weight || !out) return manet_set_error(MANET_E_INVALID, "manet_dwconv_forward_f32: NULL pointer");
    if (K == 7 && (long)B * C <= 65535)  // the inference kernel without BN / ReLU: (conv + bias) * 1 + 0
        return manet_dwconv7x7_bn_relu_ex(in, B, C, h, w, weight, bias, nullptr, nullptr, 0, 0, out, stream);
    rc = K == 7 ? launch_corr<7, false>(in, B, C, h, w, weight, bias, out, (hipStream_t)stream)
                : launch_corr<3, false>(in, B, C, h, w, weight, bias, out, (hipStream_t)stream);
    return rc ? rc : manet_check_launch("manet_dwconv_forward_f32");
}

extern "C" int manet_dwconv_backward_data_f32(const float *grad_out, int B, int C, int h, int w, int K, const float *weight,
                                              float *grad_in, manet_stream_t stream)
{
    int rc = check_dims("manet_dwconv_backward_data_f32", B, C, h, w, K);
    if (rc) return rc;
    if (!grad_out || !weight || !grad_in) return manet_set_error(MANET_E_INVALID, "manet_dwconv_backward_data_f32: NULL pointer");
    rc = K == 7 ? launch_corr<7, true>(grad_out, B, C, h, w, weight, nullptr, grad_in, (hipStream_t)stream)
                : launch_corr<3, true>(grad_out, B, C, h, w, weight, nullptr, grad_in, (hipStream_t)stream);
    return rc ? rc : manet_check_launch("manet_dwconv_backward_data_f32");
}

extern "C" int manet_dwconv_backward_weight_workspace_bytes(int B, int C, int h, int w, int K, size_t *bytes)
{
    int rc = check_dims("manet_dwconv_backward_weight_workspace_bytes", B, C, h, w, K);
    if (rc) return rc;
    if (!bytes) return manet_set_error(MANET_E_INVALID, "manet_dwconv_backward_weight_workspace_bytes: NULL pointer");
    const WgradGeom g = wgrad_geom(B, C, h, w);
    *bytes = (size_t)g.slots * (size_t)(K * K + 1) * sizeof(float);
    return MANET_OK;
}

extern "C" int manet_dwconv_backward_weight_f32(const float *in, const float *grad_out, int B, int C, int h, int w, int K,
                                                float *grad_weight, float *grad_bias, void *ws, size_t ws_bytes,
                                                manet_stream_t stream)
{
    int rc = check_dims("manet_dwconv_backward_weight_f32", B, C, h, w, K);
    if (rc) return rc;
    if (!in || !grad_out || !grad_weight || !ws)
        return manet_set_error(MANET_E_INVALID, "manet_dwconv_backward_weight_f32: NULL pointer");
    const WgradGeom g = wgrad_geom(B, C, h, w);
    const size_t need = (size_t)g.slots * (size_t)(K * K + 1) * sizeof(float);
    if (ws_bytes < need)
        return manet_set_error(MANET_E_INVALID, "manet_dwconv_backward_weight_f32: workspace of %zu bytes, %zu needed", ws_bytes, need);
    if (g.nblocks > 0x7fffffffL) return manet_set_error(MANET_E_INVALID, "manet_dwconv_backward_weight_f32: too many tiles");
    const hipStream_t st = (hipStream_t)stream;
    const long nfin = ((long)C * (K * K + 1) + 255) / 256;
    const int nslot = g.ntile * g.nbs;
    if (K == 7) {
        hipLaunchKernelGGL(dw_wgrad_kernel<7>, dim3((unsigned)g.nblocks), dim3(256), 0, st, in, grad_out, B, C, h, w, g.ntx, g.ntile,
                           g.nbs, (float *)ws);
        hipLaunchKernelGGL(dw_wgrad_finish_kernel<7>, dim3((unsigned)nfin), dim3(256), 0, st, (const float *)ws, C, nslot, grad_weight,
                           grad_bias);
    } else {
        hipLaunchKernelGGL(dw_wgrad_kernel<3>, dim3((unsigned)g.nblocks), dim3(256), 0, st, in, grad_out, B, C, h, w, g.ntx, g.ntile,
                           g.nbs, (float *)ws);
        hipLaunchKernelGGL(dw_wgrad_finish_kernel<3>, dim3((unsigned)nfin), dim3(256), 0, st, (const float *)ws, C, nslot, grad_weight,
                           grad_bias);
    }
    return manet_check_launch("manet_dwconv_backward_weight_f32");
}
