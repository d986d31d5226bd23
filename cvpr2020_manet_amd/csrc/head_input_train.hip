// The heads' input in TRAINING, assembled by one launch and taken apart by one (networks/IntVOS.py prop_seghead / int_seghead,
// reference IntVOS.py:663-671, :741-758): what the framework composes from sigmoid / sub / mul, three permutes, a label
// compare, two cats and embedding.unsqueeze(0).repeat(n, 1, 1, 1) -- a dozen launches and as many autograd nodes.
//
//   forward   x [n_ids][C + n_maps + n_planes][h*w]:
//               c <  C                     embedding[c][p]                      (any strides; read once, written n_ids times)
//               C <= c < C + n_maps        map_j[p * n_ids + o]                 (map 0 through manet_normalize_dist when
//                                          normalize_first: the inference epilogue's function, so the same bits; that value
//                                          also goes to norm_out [h*w*n_ids] for the backward, which never needs x)
//               C + n_maps <= c            labels_l[p] == o ? 1 : 0             (a label outside 0..n_ids-1: zeros)
//   backward  g_embedding[c][p] = ((gx[0][c][p] + gx[1][c][p]) + gx[2][c][p]) + ...   one owner per element, ascending objects,
//                                          written with the gradient buffer's own strides
//             g_map_j[p * n_ids + o] = gx[o][C + j][p]  (* 0.5 (1 - y)(1 + y) for the normalised map 0, y from norm_out: the
//                                          derivative of (sigmoid(d) - 0.5) * 2; y == 1 -- an object absent from the bank,
//                                          d = 1e20 -- gives exactly 0)
//             a NULL output is not wanted and its rows are not launched.
//
// Both are bandwidth-bound.  A workgroup owns 256 lanes of one channel row (blockIdx.y) and walks the objects; lanes run along
// p.  VEC: 16-byte accesses, four pixels per lane, when h*w is a multiple of 4, the planes are contiguous and every pointer is
// 16-byte aligned; otherwise one pixel per lane with the strides as given.  No workspace, no atomics.
#include "manet_common.h"

namespace {

constexpr int HI_THREADS = 256;

template <int V>
__device__ __forceinline__ void hi_store(float *dst, const float (&v)[V])
{
    if constexpr (V == 4) {
        f32x4 t = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4 *>(dst) = t;
    } else {
        dst[0] = v[0];
    }
}

template <int V>
__device__ __forceinline__ void hi_load(const float *src, float (&v)[V])
{
    if constexpr (V == 4) {
        f32x4 t = *reinterpret_cast<const f32x4 *>(src);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = src[0];
    }
}

// V = 4: the embedding's planes are contiguous (element (c, p) at c * es_c + p); V = 1: any strides
template <int V>
__global__ __launch_bounds__(HI_THREADS) void head_input_fwd_kernel(const float *__restrict__ emb, long es_c, long es_h, long es_w,
                                                                     const float *__restrict__ map0, const float *__restrict__ map1,
                                                                     const int *__restrict__ lab0, const int *__restrict__ lab1, int C,
                                                                     int w, int HW, int n_ids, int n_maps, int n_planes,
                                                                     int normalize_first, float *__restrict__ x,
                                                                     float *__restrict__ norm_out)
{
    const int c = blockIdx.y;
    const int p = (blockIdx.x * HI_THREADS + threadIdx.x) * V;
    if (p >= HW) return;
    const size_t ostride = (size_t)(C + n_maps + n_planes) * HW;
    float *dst = x + (size_t)c * HW + p;
    float v[V];
    if (c < C) {
        if constexpr (V == 4)
            hi_load<4>(emb + c * es_c + p, v);
        else
            v[0] = emb[c * es_c + (long)(p / w) * es_h + (long)(p % w) * es_w];
        for (int o = 0; o < n_ids; ++o) hi_store<V>(dst + o * ostride, v);
    } else if (c < C + n_maps) {
        const float *m = c == C ? map0 : map1;
        const bool norm = normalize_first && c == C;
        for (int o = 0; o < n_ids; ++o) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const size_t i = (size_t)(p + k) * n_ids + o;
                float t = m[i];
                if (norm) {
                    t = manet_normalize_dist(t);
                    norm_out[i] = t;
                }
                v[k] = t;
            }
            hi_store<V>(dst + o * ostride, v);
        }
    } else {
        const int *lab = (c == C + n_maps ? lab0 : lab1) + p;
        int l[V];
#pragma unroll
        for (int k = 0; k < V; ++k) l[k] = lab[k];
        for (int o = 0; o < n_ids; ++o) {
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = l[k] == o ? 1.0f : 0.0f;
            hi_store<V>(dst + o * ostride, v);
        }
    }
}

// rows c0 .. c0 + gridDim.y - 1 of the C + n_maps differentiable channels; the label channels have no gradient
template <int V>
__global__ __launch_bounds__(HI_THREADS) void head_input_bwd_kernel(const float *__restrict__ gx, const float *__restrict__ ysaved,
                                                                     int C, int c0, int w, int HW, int n_ids, int Ctot,
                                                                     int normalize_first, float *__restrict__ g_emb, long gs_c,
                                                                     long gs_h, long gs_w, float *__restrict__ g_map0,
                                                                     float *__restrict__ g_map1)
{
    const int c = c0 + blockIdx.y;
    const int p = (blockIdx.x * HI_THREADS + threadIdx.x) * V;
    if (p >= HW) return;
    const size_t ostride = (size_t)Ctot * HW;
    const float *src = gx + (size_t)c * HW + p;
    float v[V];
    if (c < C) {
        float acc[V];
        hi_load<V>(src, acc);
        for (int o = 1; o < n_ids; ++o) {
            hi_load<V>(src + o * ostride, v);
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] += v[k];
        }
        if constexpr (V == 4)
            hi_store<4>(g_emb + c * gs_c + p, acc);
        else
            g_emb[c * gs_c + (long)(p / w) * gs_h + (long)(p % w) * gs_w] = acc[0];
    } else {
        float *gm = c == C ? g_map0 : g_map1;
        if (!gm) return;
        const bool norm = normalize_first && c == C;
        for (int o = 0; o < n_ids; ++o) {
            hi_load<V>(src + o * ostride, v);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const size_t i = (size_t)(p + k) * n_ids + o;
                float g = v[k];
                if (norm) {
                    const float y = ysaved[i];
                    g *= 0.5f * ((1.0f - y) * (1.0f + y));
                }
                gm[i] = g;
            }
        }
    }
}

bool hi_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// element (c, y, x) of a [C][h][w] tensor with these strides sits at c * s_c + (y * w + x), every plane 16-byte aligned
bool hi_planes(const void *base, int C, int h, int w, long s_c, long s_h, long s_w)
{
    return hi_al16(base) && (C == 1 || s_c % 4 == 0) && (w == 1 || s_w == 1) && (h == 1 || s_h == w);
}

int hi_check(const char *what, int C, int h, int w, int n_ids, int n_maps, int n_planes, int normalize_first)
{
    if (C < 1 || C > MANET_MAX_C) return manet_set_error(MANET_E_INVALID, "%s: C=%d (1..%d)", what, C, MANET_MAX_C);
    if (h <= 0 || w <= 0) return manet_set_error(MANET_E_INVALID, "%s: sizes must be positive (h=%d w=%d)", what, h, w);
    if (n_ids < 1 || n_ids > MANET_MAX_IDS) return manet_set_error(MANET_E_INVALID, "%s: n_ids=%d (1..%d)", what, n_ids, MANET_MAX_IDS);
    if (n_maps < 0 || n_maps > 2) return manet_set_error(MANET_E_INVALID, "%s: n_maps=%d (0..2)", what, n_maps);
    if (n_planes < 1 || n_planes > 2) return manet_set_error(MANET_E_INVALID, "%s: n_planes=%d (1 or 2)", what, n_planes);
    if (normalize_first && n_maps == 0) return manet_set_error(MANET_E_INVALID, "%s: normalize_first without a map (n_maps=0)", what);
    if ((long)n_ids * (C + n_maps + n_planes) * h * w > 0x7fffffffL)
        return manet_set_error(MANET_E_INVALID, "%s: n_ids * channels * h * w must fit in 31 bits", what);
    return MANET_OK;
}

}  // namespace

extern "C" int manet_head_input_forward_f32(const float *embedding, int64_t es_c, int64_t es_h, int64_t es_w, const float *map0,
                                            const float *map1, const int32_t *labels0, const int32_t *labels1, int C, int h, int w,
                                            int n_ids, int n_maps, int n_planes, int normalize_first, float *x, float *norm_out,
                                            manet_stream_t stream)
{
    const char *what = "manet_head_input_forward_f32";
    if (int rc = hi_check(what, C, h, w, n_ids, n_maps, n_planes, normalize_first)) return rc;
    if (!embedding) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer (embedding)", what);
    if (!x) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer (x)", what);
    if ((n_maps > 0 && !map0) || (n_maps > 1 && !map1)) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer (map)", what);
    if (!labels0 || (n_planes > 1 && !labels1)) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer (labels)", what);
    if (normalize_first && !norm_out) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer (norm_out)", what);
    const int HW = h * w;
    const bool vec = HW % 4 == 0 && hi_al16(x) && hi_planes(embedding, C, h, w, (long)es_c, (long)es_h, (long)es_w);
    const int per = HI_THREADS * (vec ? 4 : 1);
    const dim3 grid((unsigned)((HW + per - 1) / per), (unsigned)(C + n_maps + n_planes));
    hipLaunchKernelGGL(vec ? head_input_fwd_kernel<4> : head_input_fwd_kernel<1>, grid, dim3(HI_THREADS), 0, (hipStream_t)stream,
                       embedding, (long)es_c, (long)es_h, (long)es_w, map0, map1, (const int *)labels0, (const int *)labels1, C, w, HW,
                       n_ids, n_maps, n_planes, normalize_first ? 1 : 0, x, norm_out);
    return manet_check_launch(what);
}

extern "C" int manet_head_input_backward_f32(const float *grad_x, const float *norm_out, int C, int h, int w, int n_ids, int n_maps,
                                             int n_planes, int normalize_first, float *grad_embedding, int64_t gs_c, int64_t gs_h,
                                             int64_t gs_w, float *grad_map0, float *grad_map1, manet_stream_t stream)
{
    const char *what = "manet_head_input_backward_f32";
    if (int rc = hi_check(what, C, h, w, n_ids, n_maps, n_planes, normalize_first)) return rc;
    if (!grad_x) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer (grad_x)", what);
    if (n_maps < 2) grad_map1 = nullptr;
    if (n_maps < 1) grad_map0 = nullptr;
    if (normalize_first && grad_map0 && !norm_out) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer (norm_out)", what);
    const bool maps = grad_map0 || grad_map1;
    if (!grad_embedding && !maps) return MANET_OK;  // nothing is wanted: no work
    const int HW = h * w;
    const int c0 = grad_embedding ? 0 : C;
    const int rows = (grad_embedding ? C : 0) + (maps ? n_maps : 0);
    const bool vec = HW % 4 == 0 && hi_al16(grad_x) &&
                     (!grad_embedding || hi_planes(grad_embedding, C, h, w, (long)gs_c, (long)gs_h, (long)gs_w));
    const int per = HI_THREADS * (vec ? 4 : 1);
    const dim3 grid((unsigned)((HW + per - 1) / per), (unsigned)rows);
    hipLaunchKernelGGL(vec ? head_input_bwd_kernel<4> : head_input_bwd_kernel<1>, grid, dim3(HI_THREADS), 0, (hipStream_t)stream,
                       grad_x, norm_out, C, c0, w, HW, n_ids, C + n_maps + n_planes, normalize_first ? 1 : 0, grad_embedding, (long)gs_c,
                       (long)gs_h, (long)gs_w, grad_map0, grad_map1);
    return manet_check_launch(what);
}
