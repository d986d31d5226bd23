// The rest of a head block's TRAINING step -- SURVEY.md 8f rank 3, finishing what dwconv_train.hip began: the 1x1 convolution
// (forward, backward-data, backward-weight + bias) and BatchNorm + ReLU (training / eval forward, backward) of every
// _split_separable_conv2d (IntVOS.py:244-332: bn1 -> relu1 -> conv2 -> bn2 -> relu2) and of the embedding head's tail
// (bn1, relu1, embedding_conv, bn2, relu2).  fp32, NCHW contiguous, stride 1.  No atomics anywhere: every reduction writes
// per-tile partials to a workspace and a second launch adds them in a fixed order, so the bits depend on the shape alone.
//
// Pointwise convolution, on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation):
//   forward          out[b][co][p] = bias[co] + sum_ci W[co][ci] * x[b][ci][p]
//   backward-data    gx[b][ci][p]  = sum_co W[co][ci] * g[b][co][p]          (the same contraction, W read transposed)
//   backward-weight  gW[co][ci]    = sum_{b,p} g[b][co][p] * x[b][ci][p],  gb[co] = sum_{b,p} g[b][co][p]
//  * 256 output channels with h*w % 4 == 0 (the 256-channel blocks; backward-data of every block but layer 1): seg_head.hip's
//    manet_conv1x1_f32, the inference kernel (0.73 of the fp32 matrix peak), with W transposed into the workspace (forward) or W
//    as it is (backward-data: W [Cout][Cin] is already the [K][256] operand) and a zero bias.
//  * anything else: pw_gemm_kernel, 128 x 128 output tiles, 4 waves of 64 x 64 (2 x 2 accumulator blocks: the four independent
//    chains the fp32 pipe needs), 16-channel k-chunks staged through LDS from registers loaded one chunk ahead.  Rows past
//    Cout / Cin and pixels past h*w are zeros in LDS; only real outputs are stored.
//  * backward-weight: pw_wgrad_kernel, 128 x 128 tiles of gW with K = B*h*w split into slices of 32-pixel chunks; a workgroup
//    owns (tile, slice) and writes its 128 x 128 partial (and, in the first Cin tile, the 128 bias partials) to a workspace
//    slab; pw_wgrad_finish_kernel adds a tile's slabs in ascending slice order.  Both operands run along K contiguously, so the
//    MFMA's k index is mapped to pixels by a fixed permutation (step 4q + r, lane half h -> pixel 8q + 4h + r) that lets
//    every lane read its A and B values as ds_read_b128.
//
// BatchNorm + ReLU (memory-bound; tiles of 4096 elements of one (b, c) plane):
//   training forward  per-tile (count, mean, M2) -> bn_stats_finish_kernel merges a channel's tiles in ascending order (Chan's
//                     formula, in double) -> mean, invstd = 1 / sqrt(var + eps), running_mean / running_var updated as
//                     nn.BatchNorm2d does (momentum, unbiased n / (n - 1) variance) -> bn_apply_kernel:
//                     out = max((x - mean) * invstd * gamma + beta, 0)
//   eval forward      mean / invstd from the running statistics, nothing updated, the same apply kernel
//   backward          g = dy * [out > 0], the mask recomputed from x with the forward's own arithmetic (bn_pre):
//                     d_beta = sum g, d_gamma = sum g * xhat (bn_bwd_reduce_kernel + bn_bwd_finish_kernel, fixed order);
//                     dx = gamma * invstd * (g - d_beta / n - xhat * d_gamma / n) in training, gamma * invstd * g in eval.
#include "manet_common.h"

namespace {

#include "bn_train.h"  // ld4, the BatchNorm tile loads, bn_pre, block_sum, the statistics kernels

// ------------------------------------------------------------------------------------------------------------------------
// pointwise convolution

constexpr int GT = 128;        // pw_gemm / pw_wgrad tile: 128 x 128 outputs, 256 threads
constexpr int GKC = 16;        // pw_gemm: input channels per k-chunk
constexpr int GAP = GKC + 4;   // pw_gemm: A tile row pitch (floats; b128 reads of 16 lanes hit 64 distinct banks)
constexpr int GBP = GT + 4;    // pw_gemm: B tile row pitch
constexpr int WKC = 32;        // pw_wgrad: pixels per k-chunk
constexpr int WP = WKC + 4;    // pw_wgrad: tile row pitch

// A[i][k] = w[i * Cin + k] (forward) or w[k * M + i] (wtrans: backward-data, W [K][M]); B[k][j] = in[b][k][j]; M outputs rows
template <bool VEC>
__global__ __launch_bounds__(256, 2) void pw_gemm_kernel(const float *__restrict__ in, int K, int M, int HW,
                                                         const float *__restrict__ w, int wtrans, const float *__restrict__ bias,
                                                         float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float As[GT * GAP];
    __shared__ __attribute__((aligned(16))) float Bs[GKC * GBP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * GT, m0 = blockIdx.y * GT, b = blockIdx.z;
    const float *src = in + (long)b * K * HW;
    const int nch = (K + GKC - 1) / GKC;
    float ra[8];
    float rb[8];
    auto load = [&](int c) __attribute__((always_inline)) {
        const int k0 = c * GKC;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int e = tid + 256 * r;
            const int i = wtrans ? (e & (GT - 1)) : (e >> 4), k = wtrans ? (e >> 7) : (e & (GKC - 1));
            const bool ok = m0 + i < M && k0 + k < K;
            ra[r] = ok ? (wtrans ? w[(long)(k0 + k) * M + m0 + i] : w[(long)(m0 + i) * K + k0 + k]) : 0.0f;
        }
        if constexpr (VEC) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int e = tid + 256 * r, k = e >> 5, j = (e & 31) * 4;
                f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (k0 + k < K && p0 + j < HW) v = ld4(src + (long)(k0 + k) * HW + p0 + j);  // (HW % 4 == 0: all four or none)
                rb[4 * r] = v[0], rb[4 * r + 1] = v[1], rb[4 * r + 2] = v[2], rb[4 * r + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int e = tid + 256 * r, k = e >> 7, j = e & (GT - 1);
                rb[r] = (k0 + k < K && p0 + j < HW) ? src[(long)(k0 + k) * HW + p0 + j] : 0.0f;
            }
        }
    };
    auto store = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int e = tid + 256 * r;
            const int i = wtrans ? (e & (GT - 1)) : (e >> 4), k = wtrans ? (e >> 7) : (e & (GKC - 1));
            As[i * GAP + k] = ra[r];
        }
        if constexpr (VEC) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int e = tid + 256 * r, k = e >> 5, j = (e & 31) * 4;
                *(f32x4 *)&Bs[k * GBP + j] = f32x4{rb[4 * r], rb[4 * r + 1], rb[4 * r + 2], rb[4 * r + 3]};
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int e = tid + 256 * r;
                Bs[(e >> 7) * GBP + (e & (GT - 1))] = rb[r];
            }
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    const int mw = (wave & 1) * 64, nw = (wave >> 1) * 64;
    const int li = lane & 31, h = lane >> 5;
    load(0);
    for (int c = 0; c < nch; ++c) {
        store();
        __syncthreads();
        if (c + 1 < nch) load(c + 1);  // (in flight under this chunk's MFMAs)
        // k-step 4q + r of lane half h is input channel 8q + 4h + r of the chunk
#pragma unroll
        for (int q = 0; q < GKC / 8; ++q) {
            const f32x4 a0 = ld4(&As[(mw + li) * GAP + 8 * q + 4 * h]);
            const f32x4 a1 = ld4(&As[(mw + 32 + li) * GAP + 8 * q + 4 * h]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *brow = &Bs[(8 * q + 4 * h + r) * GBP + nw + li];
                const float b0 = brow[0], b1 = brow[32];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[r], b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[r], b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[r], b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[r], b1, acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();  // (the next store overwrites the tiles)
    }
    // C/D layout: column = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel)
    float *dst = out + (long)b * M * HW;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int p = p0 + nw + 32 * nb + li;
        if (p >= HW) continue;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + mw + 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (m < M) dst[(long)m * HW + p] = bias ? acc[mb][nb][r] + bias[m] : acc[mb][nb][r];
            }
    }
}

// W [Cout][Cin] -> W^T [Cin][Cout] (the inference kernel's weight operand)
__global__ __launch_bounds__(256) void pw_transpose_kernel(const float *__restrict__ w, int Cout, int Cin, float *__restrict__ wt)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Cout * Cin) return;
    const int ci = (int)(i / Cout), co = (int)(i - (long)ci * Cout);
    wt[i] = w[(long)co * Cin + ci];
}

// one (128 x 128 tile of gW, K slice) per workgroup; A = g rows (output channels), B = x rows (input channels), k = pixels
template <bool VEC>
__global__ __launch_bounds__(256, 2) void pw_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ g, int Cin, int Cout,
                                                          int HW, int npc, long nchunk, int ntn, int nsl, float *__restrict__ ws,
                                                          float *__restrict__ wsb)
{
    __shared__ __attribute__((aligned(16))) float Gs[GT * WP];
    __shared__ __attribute__((aligned(16))) float Xs[GT * WP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x % nsl, tile = blockIdx.x / nsl;
    const int tm = tile / ntn, tn = tile - tm * ntn;
    const int m0 = tm * GT, n0 = tn * GT;
    const long c_begin = nchunk * s / nsl, c_end = nchunk * (s + 1) / nsl;
    float rg[16], rx[16];
    auto load = [&](long cc) __attribute__((always_inline)) {
        const int b = (int)(cc / npc), pc = (int)(cc - (long)b * npc) * WKC;
        const float *gb = g + (long)b * Cout * HW, *xb = x + (long)b * Cin * HW;
        if constexpr (VEC) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = tid + 256 * r, row = e >> 3, j = pc + (e & 7) * 4;
                f32x4 u = {0.0f, 0.0f, 0.0f, 0.0f}, v = {0.0f, 0.0f, 0.0f, 0.0f};
                if (j < HW) {  // (HW % 4 == 0: all four or none)
                    if (m0 + row < Cout) u = ld4(gb + (long)(m0 + row) * HW + j);
                    if (n0 + row < Cin) v = ld4(xb + (long)(n0 + row) * HW + j);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) rg[4 * r + t] = u[t], rx[4 * r + t] = v[t];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int e = tid + 256 * r, row = e >> 5, j = pc + (e & 31);
                rg[r] = (j < HW && m0 + row < Cout) ? gb[(long)(m0 + row) * HW + j] : 0.0f;
                rx[r] = (j < HW && n0 + row < Cin) ? xb[(long)(n0 + row) * HW + j] : 0.0f;
            }
        }
    };
    auto store = [&]() __attribute__((always_inline)) {
        if constexpr (VEC) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = tid + 256 * r, o = (e >> 3) * WP + (e & 7) * 4;
                *(f32x4 *)&Gs[o] = f32x4{rg[4 * r], rg[4 * r + 1], rg[4 * r + 2], rg[4 * r + 3]};
                *(f32x4 *)&Xs[o] = f32x4{rx[4 * r], rx[4 * r + 1], rx[4 * r + 2], rx[4 * r + 3]};
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int e = tid + 256 * r, o = (e >> 5) * WP + (e & 31);
                Gs[o] = rg[r], Xs[o] = rx[r];
            }
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    float bacc = 0.0f;  // bias partial of row tid (tid < 128, first Cin tile only)
    const bool do_bias = tn == 0 && tid < GT;
    const int mw = (wave & 1) * 64, nw = (wave >> 1) * 64;
    const int li = lane & 31, h = lane >> 5;
    if (c_begin < c_end) load(c_begin);
    for (long cc = c_begin; cc < c_end; ++cc) {
        store();
        __syncthreads();
        if (cc + 1 < c_end) load(cc + 1);
        if (do_bias) {
#pragma unroll
            for (int q = 0; q < WKC / 4; ++q) {
                const f32x4 v = ld4(&Gs[tid * WP + 4 * q]);
                bacc = (((bacc + v[0]) + v[1]) + v[2]) + v[3];
            }
        }
        // k-step 4q + r of lane half h is pixel 8q + 4h + r of the chunk
#pragma unroll
        for (int q = 0; q < WKC / 8; ++q) {
            const f32x4 a0 = ld4(&Gs[(mw + li) * WP + 8 * q + 4 * h]);
            const f32x4 a1 = ld4(&Gs[(mw + 32 + li) * WP + 8 * q + 4 * h]);
            const f32x4 b0 = ld4(&Xs[(nw + li) * WP + 8 * q + 4 * h]);
            const f32x4 b1 = ld4(&Xs[(nw + 32 + li) * WP + 8 * q + 4 * h]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[r], b0[r], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[r], b1[r], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[r], b0[r], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[r], b1[r], acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // the slab: [128 rows (output channel)][128 columns (input channel)], every entry written (zeros past Cout / Cin)
    float *slab = ws + ((long)tile * nsl + s) * (GT * GT);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = mw + 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * h, j = nw + 32 * nb + li;
                slab[i * GT + j] = acc[mb][nb][r];
            }
    if (do_bias) wsb[((long)tm * nsl + s) * GT + tid] = bacc;
}

// gW[co][ci] / gb[co] = the tile's slabs added in a fixed order: a workgroup owns 32 outputs (consecutive ci of one co, or 32
// consecutive bias entries); its 8 thread groups each add a contiguous eighth of the slices in ascending order (loads 8 at a
// time, adds in order), then group 0 adds the 8 partial sums in ascending order.  (One thread per output walking every slice
// serially waited on one load at a time: 128-256 dependent loads, longer than the main kernel.)
constexpr int FO = 32, FG = 8;
__global__ __launch_bounds__(256) void pw_wgrad_finish_kernel(const float *__restrict__ ws, const float *__restrict__ wsb, int Cin,
                                                              int Cout, int ntn, int nsl, int nwblk, float *__restrict__ gw,
                                                              float *__restrict__ gb)
{
    __shared__ float red[FG][FO];
    const int o = threadIdx.x & (FO - 1), grp = threadIdx.x >> 5;
    const int cpr = (Cin + FO - 1) / FO;  // workgroups per row of gW
    const float *src;
    long stride;
    bool ok;
    float *dst;
    if ((int)blockIdx.x < nwblk) {  // gW row co, columns ci0 .. ci0 + 31
        const int co = blockIdx.x / cpr, ci = (blockIdx.x - co * cpr) * FO + o;
        ok = ci < Cin;
        const int tile = (co / GT) * ntn + (ok ? ci : 0) / GT;
        src = ws + (long)tile * nsl * (GT * GT) + (co % GT) * GT + (ok ? ci : 0) % GT;
        stride = GT * GT;
        dst = ok ? gw + (long)co * Cin + ci : nullptr;
    } else {  // bias entries co0 .. co0 + 31
        const int co = ((int)blockIdx.x - nwblk) * FO + o;
        ok = co < Cout;
        src = wsb + (long)((ok ? co : 0) / GT) * nsl * GT + (ok ? co : 0) % GT;
        stride = GT;
        dst = ok ? gb + co : nullptr;
    }
    const int n0 = (int)((long)nsl * grp / FG), n1 = (int)((long)nsl * (grp + 1) / FG);
    float s = 0.0f;
    for (int n = n0; n < n1; n += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (n + u < n1) ? src[(long)(n + u) * stride] : 0.0f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (n + u < n1) s += v[u];
    }
    red[grp][o] = s;
    __syncthreads();
    if (grp == 0 && ok) {
        float t = red[0][o];
#pragma unroll
        for (int g = 1; g < FG; ++g) t += red[g][o];
        *dst = t;
    }
}

struct WgradGeom {
    int npc, ntm, ntn, nsl;
    long nchunk;
};

// K slices: about two workgroups per CU over the chip, never more than the chunks; a function of the shape alone, so the
// summation order -- and the bits -- are too
WgradGeom wgrad_geom(int B, int Cin, int Cout, int HW)
{
    WgradGeom g;
    g.npc = (HW + WKC - 1) / WKC;
    g.nchunk = (long)B * g.npc;
    g.ntm = (Cout + GT - 1) / GT;
    g.ntn = (Cin + GT - 1) / GT;
    const long tiles = (long)g.ntm * g.ntn;
    long nsl = (512 + tiles - 1) / tiles;
    if (nsl > g.nchunk) nsl = g.nchunk;
    g.nsl = (int)(nsl < 1 ? 1 : nsl);
    return g;
}

size_t wgrad_ws_bytes(const WgradGeom &g)
{
    return ((size_t)g.ntm * g.ntn * g.nsl * GT * GT + (size_t)g.ntm * g.nsl * GT) * sizeof(float);
}

int pw_check(const char *what, int B, int Cin, int Cout, int HW)
{
    if (B <= 0 || Cin <= 0 || Cout <= 0 || HW <= 0)
        return manet_set_error(MANET_E_INVALID, "%s: sizes must be positive (B=%d Cin=%d Cout=%d HW=%d)", what, B, Cin, Cout, HW);
    if (B > 65535) return manet_set_error(MANET_E_INVALID, "%s: B=%d (at most 65535)", what, B);
    return MANET_OK;
}

// the inference 1x1 kernel applies: 256 output channels, 16-byte rows (seg_head.hip's contract)
bool pw_fast(int Cout, int HW, const void *in, const void *w)
{
    return Cout == 256 && HW % 4 == 0 && ((size_t)in & 15) == 0 && ((size_t)w & 15) == 0;
}

__device__ float pw_zero_bias[256];  // (zero-initialised: backward-data's bias on the inference kernel)

const float *zero_bias()
{
    static const float *cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!cache[dev]) {
        void *p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(pw_zero_bias)) != hipSuccess) return nullptr;
        cache[dev] = (const float *)p;
    }
    return cache[dev];
}

int launch_gemm(const float *in, int B, int K, int M, int HW, const float *w, int wtrans, const float *bias, float *out, hipStream_t st)
{
    const dim3 grid((unsigned)((HW + GT - 1) / GT), (unsigned)((M + GT - 1) / GT), (unsigned)B);
    if ((long)grid.y > 65535) return manet_set_error(MANET_E_INVALID, "too many output channels (%d)", M);
    if (HW % 4 == 0 && ((size_t)in & 15) == 0)
        hipLaunchKernelGGL(pw_gemm_kernel<true>, grid, dim3(256), 0, st, in, K, M, HW, w, wtrans, bias, out);
    else
        hipLaunchKernelGGL(pw_gemm_kernel<false>, grid, dim3(256), 0, st, in, K, M, HW, w, wtrans, bias, out);
    return MANET_OK;
}

// ------------------------------------------------------------------------------------------------------------------------
// BatchNorm + ReLU

template <bool VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float *__restrict__ x, int C, int HW, int ntp, const float *__restrict__ mean,
                                                       const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, float *__restrict__ out)
{
    const int tile = blockIdx.x % ntp, plane = blockIdx.x / ntp, c = plane % C;
    const int t0 = tile * BT;
    float v[16];
    const long base = (long)plane * HW;
    bn_load<VEC>(v, x + base, t0, HW);
    const float m = mean[c], is = invstd[c], g = gamma[c], bb = beta[c];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = fmaxf(bn_pre(v[r], m, is, g, bb), 0.0f);
    if constexpr (VEC) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = t0 + 4 * threadIdx.x + 1024 * r;
            if (o < HW) *(f32x4 *)(out + base + o) = f32x4{v[4 * r], v[4 * r + 1], v[4 * r + 2], v[4 * r + 3]};
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = t0 + threadIdx.x + 256 * r;
            if (o < HW) out[base + o] = v[r];
        }
    }
}

// per tile: sum g and sum g * xhat, g = dy * [pre > 0]
template <bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float *__restrict__ dy, const float *__restrict__ x, int B, int C,
                                                            int HW, int ntp, const float *__restrict__ mean,
                                                            const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, float *__restrict__ ws)
{
    __shared__ float red[4];
    const int tile = blockIdx.x % ntp, plane = blockIdx.x / ntp;
    const int b = plane / C, c = plane - b * C;
    const int t0 = tile * BT;
    const long base = (long)plane * HW;
    float xv[16], gv[16];
    bn_load<VEC>(xv, x + base, t0, HW);
    bn_load<VEC>(gv, dy + base, t0, HW);
    const float m = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
    float sg = 0.0f, sgx = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float g = bn_pre(xv[r], m, is, ga, be) > 0.0f ? gv[r] : 0.0f;  // (padding: dy = 0)
        sg += g;
        sgx = fmaf(g, (xv[r] - m) * is, sgx);
    }
    sg = block_sum(sg, red);
    sgx = block_sum(sgx, red);
    if (threadIdx.x == 0) {
        float *dst = ws + 2 * (((long)c * B + b) * ntp + tile);
        dst[0] = sg, dst[1] = sgx;
    }
}

// per channel: d_beta, d_gamma (tiles ascending); coef = {d_beta / n, d_gamma / n} for the apply
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const float *__restrict__ ws, int B, int C, int ntp, float inv_n,
                                                            float *__restrict__ grad_gamma, float *__restrict__ grad_beta,
                                                            float *__restrict__ coef)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float *src = ws + 2L * c * B * ntp;
    float sg = 0.0f, sgx = 0.0f;
    const int nt = B * ntp;
    for (int i0 = 0; i0 < nt; i0 += 8) {  // (ascending; the loads of 8 in flight together)
        f32x2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = i0 + u < nt ? *(const f32x2 *)(src + 2 * (i0 + u)) : f32x2{0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u < nt) sg += v[u][0], sgx += v[u][1];
    }
    if (grad_beta) grad_beta[c] = sg;
    if (grad_gamma) grad_gamma[c] = sgx;
    coef[2 * c] = sg * inv_n, coef[2 * c + 1] = sgx * inv_n;
}

template <bool VEC>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float *__restrict__ dy, const float *__restrict__ x, int C, int HW, int ntp,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           const float *__restrict__ coef, float *__restrict__ dx)
{
    const int tile = blockIdx.x % ntp, plane = blockIdx.x / ntp, c = plane % C;
    const int t0 = tile * BT;
    const long base = (long)plane * HW;
    float xv[16], gv[16];
    bn_load<VEC>(xv, x + base, t0, HW);
    bn_load<VEC>(gv, dy + base, t0, HW);
    const float m = mean[c], is = invstd[c], ga = gamma[c], be = beta[c], k = ga * is;
    const float cb = coef ? coef[2 * c] : 0.0f, cg = coef ? coef[2 * c + 1] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float g = bn_pre(xv[r], m, is, ga, be) > 0.0f ? gv[r] : 0.0f;
        gv[r] = coef ? k * ((g - cb) - (xv[r] - m) * is * cg) : k * g;
    }
    if constexpr (VEC) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = t0 + 4 * threadIdx.x + 1024 * r;
            if (o < HW) *(f32x4 *)(dx + base + o) = f32x4{gv[4 * r], gv[4 * r + 1], gv[4 * r + 2], gv[4 * r + 3]};
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = t0 + threadIdx.x + 256 * r;
            if (o < HW) dx[base + o] = gv[r];
        }
    }
}

int bn_check(const char *what, int B, int C, int HW)
{
    if (B <= 0 || C <= 0 || HW <= 0)
        return manet_set_error(MANET_E_INVALID, "%s: sizes must be positive (B=%d C=%d HW=%d)", what, B, C, HW);
    const long ntp = (HW + BT - 1) / BT;
    if ((long)B * C * ntp > 0x7fffffffL) return manet_set_error(MANET_E_INVALID, "%s: too many tiles", what);
    return MANET_OK;
}

size_t bn_ws_bytes(int B, int C, int HW)
{
    const long ntp = (HW + BT - 1) / BT;
    return ((size_t)2 * B * C * ntp + (size_t)2 * C) * sizeof(float);
}

bool bn_vec(int HW, const void *a, const void *b, const void *c)
{
    return HW % 4 == 0 && ((size_t)a & 15) == 0 && ((size_t)b & 15) == 0 && ((size_t)c & 15) == 0;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// C ABI

extern "C" int manet_pw_forward_workspace_bytes(int B, int Cin, int Cout, int HW, size_t *bytes)
{
    int rc = pw_check("manet_pw_forward_workspace_bytes", B, Cin, Cout, HW);
    if (rc) return rc;
    if (!bytes) return manet_set_error(MANET_E_INVALID, "manet_pw_forward_workspace_bytes: NULL pointer");
    *bytes = (Cout == 256 && HW % 4 == 0) ? (size_t)Cin * Cout * sizeof(float) : 0;
    return MANET_OK;
}

extern "C" int manet_pw_forward_f32(const float *in, int B, int Cin, int Cout, int HW, const float *weight, const float *bias,
                                    float *out, void *ws, size_t ws_bytes, manet_stream_t stream)
{
    int rc = pw_check("manet_pw_forward_f32", B, Cin, Cout, HW);
    if (rc) return rc;
    if (!in || !weight || !out) return manet_set_error(MANET_E_INVALID, "manet_pw_forward_f32: NULL pointer");
    const size_t need = (Cout == 256 && HW % 4 == 0) ? (size_t)Cin * Cout * sizeof(float) : 0;
    if (need && (!ws || ws_bytes < need))
        return manet_set_error(MANET_E_INVALID, "manet_pw_forward_f32: workspace of %zu bytes, %zu needed", ws ? ws_bytes : 0, need);
    const hipStream_t st = (hipStream_t)stream;
    if (need && pw_fast(Cout, HW, in, ws) && (bias || zero_bias())) {
        hipLaunchKernelGGL(pw_transpose_kernel, dim3((unsigned)(((long)Cin * Cout + 255) / 256)), dim3(256), 0, st, weight, Cout, Cin,
                           (float *)ws);
        rc = manet_check_launch("manet_pw_forward_f32 (transpose)");
        if (rc) return rc;
        return manet_conv1x1_f32(in, (int64_t)Cin * HW, B, Cin, HW, (const float *)ws, bias ? bias : zero_bias(), Cout, 0, out, stream);
    }
    rc = launch_gemm(in, B, Cin, Cout, HW, weight, 0, bias, out, st);
    return rc ? rc : manet_check_launch("manet_pw_forward_f32");
}

extern "C" int manet_pw_backward_data_f32(const float *grad_out, int B, int Cin, int Cout, int HW, const float *weight, float *grad_in,
                                          manet_stream_t stream)
{
    int rc = pw_check("manet_pw_backward_data_f32", B, Cin, Cout, HW);
    if (rc) return rc;
    if (!grad_out || !weight || !grad_in) return manet_set_error(MANET_E_INVALID, "manet_pw_backward_data_f32: NULL pointer");
    // W [Cout][Cin] is the [K][256] weight operand of the inference kernel when Cin = 256
    if (pw_fast(Cin, HW, grad_out, weight) && zero_bias())
        return manet_conv1x1_f32(grad_out, (int64_t)Cout * HW, B, Cout, HW, weight, zero_bias(), Cin, 0, grad_in, stream);
    rc = launch_gemm(grad_out, B, Cout, Cin, HW, weight, 1, nullptr, grad_in, (hipStream_t)stream);
    return rc ? rc : manet_check_launch("manet_pw_backward_data_f32");
}

extern "C" int manet_pw_backward_weight_workspace_bytes(int B, int Cin, int Cout, int HW, size_t *bytes)
{
    int rc = pw_check("manet_pw_backward_weight_workspace_bytes", B, Cin, Cout, HW);
    if (rc) return rc;
    if (!bytes) return manet_set_error(MANET_E_INVALID, "manet_pw_backward_weight_workspace_bytes: NULL pointer");
    *bytes = wgrad_ws_bytes(wgrad_geom(B, Cin, Cout, HW));
    return MANET_OK;
}

extern "C" int manet_pw_backward_weight_f32(const float *in, const float *grad_out, int B, int Cin, int Cout, int HW, float *grad_weight,
                                            float *grad_bias, void *ws, size_t ws_bytes, manet_stream_t stream)
{
    int rc = pw_check("manet_pw_backward_weight_f32", B, Cin, Cout, HW);
    if (rc) return rc;
    if (!in || !grad_out || !ws || (!grad_weight && !grad_bias))
        return manet_set_error(MANET_E_INVALID, "manet_pw_backward_weight_f32: NULL pointer");
    const WgradGeom g = wgrad_geom(B, Cin, Cout, HW);
    const size_t need = wgrad_ws_bytes(g);
    if (ws_bytes < need)
        return manet_set_error(MANET_E_INVALID, "manet_pw_backward_weight_f32: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const long nblocks = (long)g.ntm * g.ntn * g.nsl;
    if (nblocks > 0x7fffffffL) return manet_set_error(MANET_E_INVALID, "manet_pw_backward_weight_f32: too many tiles");
    const hipStream_t st = (hipStream_t)stream;
    float *slabs = (float *)ws, *bslabs = slabs + (size_t)g.ntm * g.ntn * g.nsl * GT * GT;
    if (HW % 4 == 0 && ((size_t)in & 15) == 0 && ((size_t)grad_out & 15) == 0)
        hipLaunchKernelGGL(pw_wgrad_kernel<true>, dim3((unsigned)nblocks), dim3(256), 0, st, in, grad_out, Cin, Cout, HW, g.npc, g.nchunk,
                           g.ntn, g.nsl, slabs, bslabs);
    else
        hipLaunchKernelGGL(pw_wgrad_kernel<false>, dim3((unsigned)nblocks), dim3(256), 0, st, in, grad_out, Cin, Cout, HW, g.npc,
                           g.nchunk, g.ntn, g.nsl, slabs, bslabs);
    const long nwblk = grad_weight ? (long)Cout * ((Cin + FO - 1) / FO) : 0, nbblk = grad_bias ? (Cout + FO - 1) / FO : 0;
    if (nwblk + nbblk > 0x7fffffffL) return manet_set_error(MANET_E_INVALID, "manet_pw_backward_weight_f32: too many outputs");
    hipLaunchKernelGGL(pw_wgrad_finish_kernel, dim3((unsigned)(nwblk + nbblk)), dim3(256), 0, st, (const float *)slabs,
                       (const float *)bslabs, Cin, Cout, g.ntn, g.nsl, (int)nwblk, grad_weight, grad_bias);
    return manet_check_launch("manet_pw_backward_weight_f32");
}

extern "C" int manet_bn_relu_workspace_bytes(int B, int C, int HW, size_t *bytes)
{
    int rc = bn_check("manet_bn_relu_workspace_bytes", B, C, HW);
    if (rc) return rc;
    if (!bytes) return manet_set_error(MANET_E_INVALID, "manet_bn_relu_workspace_bytes: NULL pointer");
    *bytes = bn_ws_bytes(B, C, HW);
    return MANET_OK;
}

extern "C" int manet_bn_relu_forward_f32(const float *in, int B, int C, int HW, const float *gamma, const float *beta,
                                         float *running_mean, float *running_var, float momentum, float eps, int training, float *out,
                                         float *save_mean, float *save_invstd, void *ws, size_t ws_bytes, manet_stream_t stream)
{
    int rc = bn_check("manet_bn_relu_forward_f32", B, C, HW);
    if (rc) return rc;
    if (!in || !gamma || !beta || !out || !save_mean || !save_invstd || (!training && (!running_mean || !running_var)))
        return manet_set_error(MANET_E_INVALID, "manet_bn_relu_forward_f32: NULL pointer");
    if (training && (long)B * HW < 2)
        return manet_set_error(MANET_E_INVALID, "manet_bn_relu_forward_f32: one value per channel in training (B=%d HW=%d)", B, HW);
    if (!(eps > 0.0f) || !(momentum >= 0.0f && momentum <= 1.0f))
        return manet_set_error(MANET_E_INVALID, "manet_bn_relu_forward_f32: eps=%g momentum=%g", (double)eps, (double)momentum);
    const size_t need = bn_ws_bytes(B, C, HW);
    if (training && (!ws || ws_bytes < need))
        return manet_set_error(MANET_E_INVALID, "manet_bn_relu_forward_f32: workspace of %zu bytes, %zu needed", ws ? ws_bytes : 0, need);
    const hipStream_t st = (hipStream_t)stream;
    const int ntp = (HW + BT - 1) / BT;
    const unsigned nb = (unsigned)((long)B * C * ntp), nc = (unsigned)((C + 255) / 256);
    const bool vec = bn_vec(HW, in, out, in);
    if (training) {
        if (vec) hipLaunchKernelGGL(bn_stats_kernel<true>, dim3(nb), dim3(256), 0, st, in, B, C, HW, ntp, (float *)ws);
        else hipLaunchKernelGGL(bn_stats_kernel<false>, dim3(nb), dim3(256), 0, st, in, B, C, HW, ntp, (float *)ws);
        hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(nc), dim3(256), 0, st, (const float *)ws, B, C, HW, ntp, eps, momentum,
                           running_mean, running_var, save_mean, save_invstd);
    } else {
        hipLaunchKernelGGL(bn_eval_stats_kernel, dim3(nc), dim3(256), 0, st, (const float *)running_mean, (const float *)running_var, C,
                           eps, save_mean, save_invstd);
    }
    if (vec)
        hipLaunchKernelGGL(bn_apply_kernel<true>, dim3(nb), dim3(256), 0, st, in, C, HW, ntp, save_mean, save_invstd, gamma, beta, out);
    else
        hipLaunchKernelGGL(bn_apply_kernel<false>, dim3(nb), dim3(256), 0, st, in, C, HW, ntp, save_mean, save_invstd, gamma, beta, out);
    return manet_check_launch("manet_bn_relu_forward_f32");
}

extern "C" int manet_bn_relu_backward_f32(const float *grad_out, const float *in, int B, int C, int HW, const float *gamma,
                                          const float *beta, const float *save_mean, const float *save_invstd, int training,
                                          float *grad_in, float *grad_gamma, float *grad_beta, void *ws, size_t ws_bytes,
                                          manet_stream_t stream)
{
    int rc = bn_check("manet_bn_relu_backward_f32", B, C, HW);
    if (rc) return rc;
    if (!grad_out || !in || !gamma || !beta || !save_mean || !save_invstd)
        return manet_set_error(MANET_E_INVALID, "manet_bn_relu_backward_f32: NULL pointer");
    const bool reduce = grad_gamma || grad_beta || (training && grad_in);
    const size_t need = bn_ws_bytes(B, C, HW);
    if (reduce && (!ws || ws_bytes < need))
        return manet_set_error(MANET_E_INVALID, "manet_bn_relu_backward_f32: workspace of %zu bytes, %zu needed", ws ? ws_bytes : 0, need);
    const hipStream_t st = (hipStream_t)stream;
    const int ntp = (HW + BT - 1) / BT;
    const unsigned nb = (unsigned)((long)B * C * ntp), nc = (unsigned)((C + 255) / 256);
    const bool vec = bn_vec(HW, grad_out, in, grad_in ? (const void *)grad_in : (const void *)in);
    float *coef = reduce ? (float *)ws + (size_t)2 * B * C * ntp : nullptr;
    if (reduce) {
        if (vec)
            hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, dim3(nb), dim3(256), 0, st, grad_out, in, B, C, HW, ntp, save_mean, save_invstd,
                               gamma, beta, (float *)ws);
        else
            hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, dim3(nb), dim3(256), 0, st, grad_out, in, B, C, HW, ntp, save_mean,
                               save_invstd, gamma, beta, (float *)ws);
        hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(nc), dim3(256), 0, st, (const float *)ws, B, C, ntp, (float)(1.0 / ((double)B * HW)),
                           grad_gamma, grad_beta, coef);
    }
    if (grad_in) {
        const float *cf = training ? coef : nullptr;
        if (vec)
            hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(nb), dim3(256), 0, st, grad_out, in, C, HW, ntp, save_mean, save_invstd,
                               gamma, beta, cf, grad_in);
        else
            hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(nb), dim3(256), 0, st, grad_out, in, C, HW, ntp, save_mean, save_invstd,
                               gamma, beta, cf, grad_in);
    }
    return manet_check_launch("manet_bn_relu_backward_f32");
}
