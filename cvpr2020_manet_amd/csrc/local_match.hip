// Local (2d+1)^2 window matching against the previous frame, MI355X (gfx950): the unfused kernels of the reference formula.
//
// Replaces networks/IntVOS.py:266-315 (local_pairwise_distances2) and :345-434
// (local_previous_frame_nearest_neighbor_features_per_object; USE_CORRELATION_COST=False,
// MODEL_UNFOLD=True -- the live configuration, IntVOS.py:15-16).
//
// HBM-bound at small windows (d=4: ~7 flop/B), VALU-bound at the reference's default d=12 (SURVEY.md
// 8d): the point is to read each embedding once, coalesced along x out of the caller's C-major
// planes, and never to build the reference's [1,C,h',w',(2d+1)^2] unfold tensor (1.6 GB at d=12).
// The live configuration (downsample on) runs csrc/local_fused.hip; these kernels serve the stand-alone distance API, downsample off,
// the unfused route (MANET_TUNE_LOCAL_UNFUSED) and training (csrc/local_train.hip).  csrc/local_geom.h: tile geometry (ld_*), shared code.
//   pool2x2_kernel      both frames -> [C][h'][w'] planes (2x2 mean; floor sizes)
//   local_dist_kernel<D> workgroup = rows x 16 columns of the (pooled) grid; the previous frame's halo
//                       tile goes through LDS in channel stages, a thread slides a 2-column window over
//                       one window row: 2 x (2d+1) running sums over C of (x - y)^2, direct form as the
//                       reference (no |x|^2+|y|^2-2xy cancellation); out-of-image neighbours are the
//                       reference's 1e20 padding -> inf -> 1.0 after normalisation
//   local_min_kernel    64 full-resolution pixels x 8 waves: bilinear (align_corners) sample of the
//                       pooled, normalised volume + stride-2 label gather + masked min per object;
//                       waves split the window rows, partial minima meet in LDS
//   local_upsample_kernel  only for the stand-alone local_pairwise_distances2 API
#include "manet_common.h"
#include "local_geom.h"

namespace {

// (window width P = 2d+1 <= 2*MANET_MAX_LOCAL_DISTANCE+1 = 25)
// IntVOS.py:282-284  F.avg_pool2d(x, (2,2), (2,2)): window summed row-major, times 1/4 (exact)
__global__ void pool2x2_kernel(const float *__restrict__ a, long a_sy, long a_sx, long a_sc,
                               const float *__restrict__ b, long b_sy, long b_sx, long b_sc, int C, int hp,
                               int wp, float *__restrict__ ap, float *__restrict__ bp)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long plane = (long)hp * wp;
    if (i >= plane * C) return;
    int c = (int)(i / plane);
    int rem = (int)(i - (long)c * plane);
    int py = rem / wp, px = rem - py * wp;
    const float *p = a + (2L * py) * a_sy + (2L * px) * a_sx + (long)c * a_sc;
    const float *q = b + (2L * py) * b_sy + (2L * px) * b_sx + (long)c * b_sc;
    ap[i] = (((p[0] + p[a_sx]) + p[a_sy]) + p[a_sy + a_sx]) * 0.25f;
    bp[i] = (((q[0] + q[b_sx]) + q[b_sy]) + q[b_sy + b_sx]) * 0.25f;
}

// IntVOS.py:288-294 (pooled grid, normalised) and :300-313 (full grid, raw).
// x = current/query frame, y = previous frame, both [H][W][C] with element strides.
// pooled_out != 0: out[l][H][W] = (sigmoid(dist)-0.5)*2 ; else out[H][W][P*P] = dist.
//
// Workgroup = RY grid rows x 16 columns, all P*P offsets.  Thread = (row ry, window row dy, pair of
// columns): 2 x P running sums in registers.  Per chunk of LD_CC channels the y halo tile
// [(RY+2d) rows][16+2d cols] (out-of-image = the reference's 1e20 padding, IntVOS.py:287, so
// (x-1e20)^2 = inf needs no bounds logic in the inner loop) and the x tile are staged in LDS with
// row-contiguous global reads; a thread then slides its 2+2d wide window over the P offsets out
// of registers: (2+2d)/2 ds_read_b64 feed 2*P sub+fma pairs.  Channels are accumulated in ascending
// order with fmaf -- the same arithmetic as the oracle.
template <int D>  // window radius: compile-time so the 2 x P accumulators unroll without predicates
__global__ __launch_bounds__(256, 2) void local_dist_kernel(const float *__restrict__ x, long x_sy, long x_sx,
                                                            long x_sc, const float *__restrict__ y, long y_sy,
                                                            long y_sx, long y_sc, int H, int W, int C,
                                                            int pooled_out, float *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int d = D;
    constexpr int P = 2 * d + 1;
    constexpr int MAXP = P;  // arrays are exactly P wide
    constexpr int RY = ld_ry(D), LD_CC = ld_cc(D), LD_NJ = ld_nj(D);
    constexpr int RYH = RY + 2 * d;  // halo rows
    constexpr int CW = ld_cw(D);
    constexpr int yplane = RYH * CW, xplane = RY * LD_TX;
    const int buf_floats = LD_CC * (yplane + xplane);  // one stage: ys [LD_CC][RYH][CW] then xs [LD_CC][RY][16]
    float *smem = (float *)smem_raw;
    const int tid = threadIdx.x;
    const int px0 = blockIdx.x * LD_TX, py0 = blockIdx.y * RY;

    // staging map, fixed for the whole kernel: this thread's LD_NJ elements of the halo plane and its
    // one element of the x plane (global offsets without the channel term; -1 = outside the image)
    long yoff[LD_NJ];
    int ylds[LD_NJ];
#pragma unroll
    for (int j = 0; j < LD_NJ; ++j) {
        int e = tid + 256 * j;
        ylds[j] = (e < yplane) ? e : -1;
        int r = e / CW, col = e - r * CW;
        int yy = py0 - d + r, xx = px0 - d + col;
        yoff[j] = (e < yplane && yy >= 0 && yy < H && xx >= 0 && xx < W) ? ((long)yy * y_sy + (long)xx * y_sx) : -1;
    }
    long xoff = -1;
    const bool has_x = tid < xplane;
    if (has_x) {
        int r = tid / LD_TX, col = tid - r * LD_TX;
        if (py0 + r < H && px0 + col < W) xoff = (long)(py0 + r) * x_sy + (long)(px0 + col) * x_sx;
    }
    float ry_[LD_CC][LD_NJ], rx_[LD_CC];
    auto load_regs = [&](int c0) {  // all loads of a stage issued back to back
#pragma unroll
        for (int c = 0; c < LD_CC; ++c) {
            const bool cin = (c0 + c) < C;
#pragma unroll
            for (int j = 0; j < LD_NJ; ++j)
                ry_[c][j] = (cin && yoff[j] >= 0) ? y[yoff[j] + (long)(c0 + c) * y_sc] : (cin ? 1e20f : 0.0f);
            rx_[c] = (cin && xoff >= 0) ? x[xoff + (long)(c0 + c) * x_sc] : 0.0f;
        }
    };
    auto store_lds = [&](int buf) {
        float *ys = smem + (long)buf * buf_floats;
        float *xs = ys + LD_CC * yplane;
#pragma unroll
        for (int c = 0; c < LD_CC; ++c) {
#pragma unroll
            for (int j = 0; j < LD_NJ; ++j)
                if (ylds[j] >= 0) ys[c * yplane + ylds[j]] = ry_[c][j];
            if (has_x) xs[c * xplane + tid] = rx_[c];
        }
    };

    // thread -> (ry, dy, g): g = column pair
    const int g = tid & 7;
    const int dy = (tid >> 3) % P;
    const int ry = (tid >> 3) / P;
    const bool active = ry < RY;
    float acc0[MAXP], acc1[MAXP];
#pragma unroll
    for (int i = 0; i < MAXP; ++i) acc0[i] = acc1[i] = 0.0f;

    load_regs(0);
    store_lds(0);
    __syncthreads();
    int buf = 0;
    for (int c0 = 0; c0 < C; c0 += LD_CC, buf ^= 1) {
        const bool more = (c0 + LD_CC) < C;
        if (more) load_regs(c0 + LD_CC);  // next stage's global loads fly under this stage's math
        if (active) {
            const float *ys = smem + (long)buf * buf_floats;
            const float *xs = ys + LD_CC * yplane;
#pragma unroll 2
            for (int c = 0; c < LD_CC; ++c) {  // channels beyond C were staged as x = y = 0 (adds 0) / 1e20 (already inf)
                const float *yrow = ys + c * yplane + (ry + dy) * CW + 2 * g;
                const float2 xv = *(const float2 *)(xs + c * xplane + ry * LD_TX + 2 * g);
                float win[MAXP + 1];
#pragma unroll
                for (int i = 0; i < (MAXP + 1) / 2; ++i) {
                    if (2 * i < P + 1) {
                        float2 t = *(const float2 *)(yrow + 2 * i);
                        win[2 * i] = t.x;
                        win[2 * i + 1] = t.y;
                    }
                }
#pragma unroll
                for (int dx = 0; dx < MAXP; ++dx) {
                    if (dx < P) {
                        float d0 = xv.x - win[dx];
                        float d1 = xv.y - win[dx + 1];
                        acc0[dx] = fmaf(d0, d0, acc0[dx]);
                        acc1[dx] = fmaf(d1, d1, acc1[dx]);
                    }
                }
            }
        }
        if (more) store_lds(buf ^ 1);
        __syncthreads();
    }
    if (!active) return;
    const int py = py0 + ry, pxa = px0 + 2 * g;
    if (py >= H) return;
#pragma unroll
    for (int dx = 0; dx < MAXP; ++dx) {
        if (dx < P) {
            const int l = dy * P + dx;
            if (pooled_out) {
                float *o = out + ((long)l * H + py) * W + pxa;
                if (pxa < W) o[0] = manet_normalize_dist_local(acc0[dx]);
                if (pxa + 1 < W) o[1] = manet_normalize_dist_local(acc1[dx]);
            } else {
                if (pxa < W) out[((long)py * W + pxa) * (P * P) + l] = acc0[dx];
                if (pxa + 1 < W) out[((long)py * W + pxa + 1) * (P * P) + l] = acc1[dx];
            }
        }
    }
}

// IntVOS.py:398-408 (label unfold, stride 2, zero padding) + :428-432 (where / min).
// pooled != 0: dvol = [P*P][hp][wp] normalised pooled volume, sampled bilinearly at (y, x);
// pooled == 0: dvol = [h][w][P*P] full-resolution raw distances.
// Workgroup = 64 consecutive pixels x LM_WAVES waves; wave k takes window rows by = k, k+LM_WAVES, ..
// (lanes run along x, so tap and label loads are row segments); partial minima meet in LDS.
constexpr int NI = 8;        // object ids per pass
constexpr int LM_WAVES = 8;  // waves per workgroup
__global__ __launch_bounds__(64 * LM_WAVES) void local_min_kernel(const float *__restrict__ dvol, int pooled,
                                                                  const int *__restrict__ labels, int h, int w,
                                                                  int hp, int wp, int d, int n_ids,
                                                                  float *__restrict__ out)
{
    __shared__ float red[LM_WAVES][NI][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 64 + lane;
    const bool valid = i < (long)h * w;
    const int y = valid ? (int)(i / w) : 0, x = valid ? (int)(i - (long)y * w) : 0;
    const int P = 2 * d + 1;
    Bilin cy = {0, 0, 0.f, 0.f}, cx = {0, 0, 0.f, 0.f};
    if (pooled) {
        cy = bilin_coeff(y, hp, h);
        cx = bilin_coeff(x, wp, w);
    }
    const long plane = (long)hp * wp;
    for (int o0 = 0; o0 < n_ids; o0 += NI) {
        float m[NI];
#pragma unroll
        for (int k = 0; k < NI; ++k) m[k] = INFINITY;
        if (valid) {
            for (int by = wave; by < P; by += LM_WAVES) {
                const int yy = y + 2 * (by - d);
                const bool yin = (yy >= 0 && yy < h);
#pragma unroll 5
                for (int bx = 0; bx < P; ++bx) {
                    const int xx = x + 2 * (bx - d);
                    const int lab = (yin && xx >= 0 && xx < w) ? labels[(long)yy * w + xx] : 0;
                    const int l = by * P + bx;
                    const float v = pooled ? bilin_sample(dvol + (long)l * plane, wp, cy, cx) : dvol[i * (P * P) + l];
#pragma unroll
                    for (int k = 0; k < NI; ++k) m[k] = fminf(m[k], (lab == o0 + k) ? v : 1.0f);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NI; ++k) red[wave][k][lane] = m[k];
        __syncthreads();
        if (wave == 0 && valid) {
#pragma unroll
            for (int k = 0; k < NI; ++k) {
                float r = red[0][k][lane];
#pragma unroll
                for (int ww = 1; ww < LM_WAVES; ++ww) r = fminf(r, red[ww][k][lane]);
                if (o0 + k < n_ids) out[i * n_ids + o0 + k] = r;
            }
        }
        __syncthreads();
    }
}

// IntVOS.py:295-296: the resized volume itself, [h][w][P*P]
__global__ void local_upsample_kernel(const float *__restrict__ dvol, int h, int w, int hp, int wp, int PP,
                                      float *__restrict__ out)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)h * w * PP) return;
    int l = (int)(i % PP);
    long pix = i / PP;
    int y = (int)(pix / w), x = (int)(pix - (long)y * w);
    Bilin cy = bilin_coeff(y, hp, h), cx = bilin_coeff(x, wp, w);
    out[i] = bilin_sample(dvol + (long)l * hp * wp, wp, cy, cx);
}

// enqueue pooling (if any) + the distance volume into the workspace; returns the volume pointer
float *enqueue_volume(const float *cur, int64_t c_sy, int64_t c_sx, int64_t c_sc, const float *prev,
                      int64_t p_sy, int64_t p_sx, int64_t p_sc, int h, int w, int C, int d, int downsample,
                      char *ws, const LocalLayout &L, hipStream_t st)
{
    float *vol = (float *)(ws + L.off_vol);
    if (downsample)
        manet_local_pooled_volume(cur, (long)c_sy, (long)c_sx, (long)c_sc, prev, (long)p_sy, (long)p_sx, (long)p_sc, C, L.hp, L.wp, d,
                                  (float *)(ws + L.off_ap), (float *)(ws + L.off_bp), vol, st);
    else
        manet_local_launch_dist(d, st, cur, (long)c_sy, (long)c_sx, (long)c_sc, prev, (long)p_sy, (long)p_sx, (long)p_sc, h, w, C,
                                0, vol);
    return vol;
}

}  // namespace

void manet_local_launch_dist(int d, hipStream_t st, const float *x, long x_sy, long x_sx, long x_sc, const float *y, long y_sy,
                             long y_sx, long y_sc, int H, int W, int C, int pooled_out, float *out)
{
    const DistLaunch DL = dist_launch(H, W, d);
    for_window(d, [&](auto dc) {
        hipLaunchKernelGGL(local_dist_kernel<decltype(dc)::value>, DL.grid, dim3(256), DL.lds, st, x, x_sy, x_sx, x_sc, y, y_sy, y_sx,
                           y_sc, H, W, C, pooled_out, out);
    });
}

void manet_local_pooled_volume(const float *cur, long c_sy, long c_sx, long c_sc, const float *prev, long p_sy, long p_sx, long p_sc,
                               int C, int hp, int wp, int d, float *ap, float *bp, float *vol, hipStream_t st)
{
    const long plane = (long)hp * wp, n = plane * C;
    hipLaunchKernelGGL(pool2x2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cur, c_sy, c_sx, c_sc, prev, p_sy, p_sx,
                       p_sc, C, hp, wp, ap, bp);
    if (vol) manet_local_launch_dist(d, st, (const float *)ap, (long)wp, 1L, plane, (const float *)bp, (long)wp, 1L, plane, hp, wp, C, 1, vol);
}

extern "C" {

int manet_local_workspace_bytes(int h, int w, int C, int max_distance, int downsample, size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = check_local(h, w, C, max_distance, downsample);
    if (rc) return rc;
    *bytes = local_layout(h, w, C, max_distance, downsample).total;
    return MANET_OK;
}

int manet_local_dist_f32(const float *cur, int64_t c_sy, int64_t c_sx, int64_t c_sc, const float *prev,
                         int64_t p_sy, int64_t p_sx, int64_t p_sc, int h, int w, int C, int max_distance,
                         int downsample, float *out, void *workspace, size_t workspace_bytes,
                         manet_stream_t stream)
{
    int rc = check_local(h, w, C, max_distance, downsample);
    if (rc) return rc;
    if (!cur || !prev || !out) return manet_set_error(MANET_E_INVALID, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int d = max_distance;
    if (!downsample) {  // the volume is the result: write it straight into out
        manet_local_launch_dist(d, st, cur, (long)c_sy, (long)c_sx, (long)c_sc, prev, (long)p_sy, (long)p_sx, (long)p_sc, h, w, C,
                                0, out);
        return manet_check_launch("manet_local_dist_f32");
    }
    LocalLayout L = local_layout(h, w, C, d, downsample);
    if (!workspace || workspace_bytes < L.total)
        return manet_set_error(MANET_E_WORKSPACE, "local workspace %zu < %zu bytes", workspace_bytes, L.total);
    float *vol = enqueue_volume(cur, c_sy, c_sx, c_sc, prev, p_sy, p_sx, p_sc, h, w, C, d, 1, (char *)workspace, L, st);
    long n = (long)h * w * L.PP;
    hipLaunchKernelGGL(local_upsample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       (const float *)vol, h, w, L.hp, L.wp, L.PP, out);
    return manet_check_launch("manet_local_dist_f32");
}

int manet_local_match_f32(const float *prev, int64_t p_sy, int64_t p_sx, int64_t p_sc, const float *cur,
                          int64_t c_sy, int64_t c_sx, int64_t c_sc, const int32_t *prev_labels, int h, int w,
                          int C, int n_ids, int max_distance, int downsample, float *out, void *workspace,
                          size_t workspace_bytes, manet_stream_t stream)
{
    return manet_local_match_ex(prev, p_sy, p_sx, p_sc, cur, c_sy, c_sx, c_sc, MANET_EMB_F32, prev_labels, h, w, C, n_ids,
                                max_distance, downsample, out, workspace, workspace_bytes, stream);
}

int manet_local_match_ex(const void *prev_v, int64_t p_sy, int64_t p_sx, int64_t p_sc, const void *cur_v, int64_t c_sy,
                         int64_t c_sx, int64_t c_sc, int emb_dtype, const int32_t *prev_labels, int h, int w, int C,
                         int n_ids, int max_distance, int downsample, float *out, void *workspace, size_t workspace_bytes,
                         manet_stream_t stream)
{
    const float *prev = (const float *)prev_v, *cur = (const float *)cur_v;  // (typed below)
    int rc = check_local(h, w, C, max_distance, downsample);
    if (rc) return rc;
    if (emb_dtype != MANET_EMB_F32 && emb_dtype != MANET_EMB_BF16)
        return manet_set_error(MANET_E_INVALID, "embedding dtype %d (MANET_EMB_F32 / MANET_EMB_BF16)", emb_dtype);
    if (emb_dtype == MANET_EMB_BF16 && (!downsample || manet_tune_get(MANET_TUNE_LOCAL_UNFUSED, 0)))
        return manet_set_error(MANET_E_INVALID, "bf16 embeddings: the downsample configuration (fused path) only");
    if ((rc = check_ids(n_ids))) return rc;
    if (!cur || !prev || !prev_labels || !out) return manet_set_error(MANET_E_INVALID, "null pointer");
    LocalLayout L = local_layout(h, w, C, max_distance, downsample);
    if (!workspace || workspace_bytes < L.total)
        return manet_set_error(MANET_E_WORKSPACE, "local workspace %zu < %zu bytes", workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    if (downsample && !manet_tune_get(MANET_TUNE_LOCAL_UNFUSED, 0)) {  // the live configuration: pooling pass + fused kernel
        manet_profile_record(st, true, 1);
        manet_local_launch_fused(max_distance, st, cur_v, (long)c_sy, (long)c_sx, (long)c_sc, prev_v, (long)p_sy, (long)p_sx,
                                 (long)p_sc, emb_dtype, prev_labels, h, w, C, n_ids, out, (float *)((char *)workspace + L.off_ap),
                                 (int *)((char *)workspace + L.off_vol));
        manet_profile_record(st, false, 1);
        return manet_check_launch("manet_local_match_f32");
    }
    // IntVOS.py:370: local_pairwise_distances2(query_embedding, prev_frame_embedding)
    float *vol = enqueue_volume(cur, c_sy, c_sx, c_sc, prev, p_sy, p_sx, p_sc, h, w, C, max_distance, downsample,
                                (char *)workspace, L, st);
    long n = (long)h * w;
    hipLaunchKernelGGL(local_min_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64 * LM_WAVES), 0, st,
                       (const float *)vol, downsample ? 1 : 0, prev_labels, h, w, L.hp, L.wp, max_distance, n_ids, out);
    return manet_check_launch("manet_local_match_f32");
}

}  // extern "C"
