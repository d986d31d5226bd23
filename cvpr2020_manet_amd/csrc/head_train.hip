// A whole DynamicSegHead TRAINING step behind two calls (networks/IntVOS.py:443-476, reference IntVOS.py:509-525: four
// _split_separable_conv2d blocks and conv = Conv2d(Cmid, 1, 1)), and the output layer's own kernels.
//
// Output layer, fused with the BatchNorm + ReLU in front of it (layer 4 ends conv2 -> bn2 -> relu2; conv reads that once):
//   forward   z [B][C][HW] (layer 4's conv2 output) -> statistics exactly as manet_bn_relu_forward_f32 (bn_train.h's kernels)
//             -> logits[b][p] = bias + sum_c w[c] * max(bn(z)[b][c][p], 0).  The activation is never written.
//             oc_fwd_kernel: a workgroup owns 256 pixels (64 lanes x float4) of one batch item and one GROUP of channels, its
//             4 waves split the group, 8 independent 16-byte loads in flight per lane, the waves meet in LDS
//             ((w0 + w1) + (w2 + w3)).  With one group the logits are written directly; with G > 1 (few pixels: 129 workgroups
//             at [3,256,104,104] would leave half the chip idle) each group writes a partial plane to the workspace and
//             oc_fwd_finish_kernel adds them in ascending order.  G is a function of the shape alone.
//   backward  a = max(bn(z), 0) recomputed with the forward's arithmetic (bn_pre), g' = w[c] * g * [a > 0]:
//             oc_bwd_reduce_kernel   per (b, c, 4096-element tile): sum g a, sum g [a > 0], sum g [a > 0] xhat, sum g
//             oc_bwd_finish_kernel   per channel, tiles ascending: grad_w = sum g a, grad_beta = w sum g [a > 0],
//                                    grad_gamma = w sum g [a > 0] xhat, grad_bias = channel 0's sum g
//             oc_bwd_apply_kernel    grad_z = gamma invstd (g' - grad_beta / n - xhat grad_gamma / n)   (eval: gamma invstd g')
//             The rank-one gradient of the activation, w[c] g[b][p], is never written either.
//   The same three backward kernels without the BatchNorm (BN = false: a = x, g' = w g) are the standalone output conv's
//   backward; its forward is seg_head.hip's relu_conv1x1_c1_kernel with relu_in = 0.
// No atomics: partials per (channel, tile) in the workspace, a second launch adds them in a fixed order.
//
// The head: manet_head_train_forward_f32 / _backward_f32 call the EXISTING launchers (manet_dwconv_*, manet_bn_relu_*,
// manet_pw_*) in the order the block-by-block route does, and the fused output kernels at the end / start; the saved
// activations and every workspace are carved out of two caller-provided buffers (head_layout).  Every argument is checked
// before the first launch.
#include "manet_common.h"

namespace {

#include "bn_train.h"  // ld4, BT, bn_pre, bn_load, bn_off, block_sum, the statistics kernels

// ------------------------------------------------------------------------------------------------------------------------
// output layer: forward

constexpr int OC_PX = 256;  // pixels per workgroup: 64 lanes x float4

// channel groups: enough workgroups for the chip (about 4 per CU), at least 32 channels (8 per wave) per group
int oc_groups(int B, int C, int HW)
{
    const long nwg = (long)B * ((HW + OC_PX - 1) / OC_PX);
    int G = 1;
    while (G < 8 && nwg * G < 1024 && C / (2 * G) >= 32) G *= 2;
    return G;
}

// dst[(grp * B + b) * HW + p] = (bias) + sum over the group's channels of w[c] * max(bn_pre(z[b][c][p]), 0)
__global__ __launch_bounds__(256) void oc_fwd_kernel(const float *__restrict__ z, int C, int HW, int cpg, int vec_ok,
                                                     const float *__restrict__ mean, const float *__restrict__ invstd,
                                                     const float *__restrict__ gamma, const float *__restrict__ beta,
                                                     const float *__restrict__ weight, const float *__restrict__ bias,
                                                     float *__restrict__ dst)
{
    __shared__ f32x4 part[4][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = blockIdx.y, b = blockIdx.z, B = gridDim.z;
    const int p0 = ((int)blockIdx.x * 64 + lane) * 4;
    const float *src = z + (long)b * C * HW;
    const int g0 = grp * cpg, g1 = min(g0 + cpg, C);
    const int cper = (g1 - g0 + 3) / 4, c0 = g0 + wave * cper, c1 = min(c0 + cper, g1);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (vec_ok) {  // (HW % 4 == 0, 16-byte aligned planes: p0 < HW means all four)
        if (p0 < HW) {
            int c = c0;
            for (; c + 8 <= c1; c += 8) {
                f32x4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = ld4(src + (long)(c + u) * HW + p0);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float m = mean[c + u], is = invstd[c + u], ga = gamma[c + u], be = beta[c + u], wv = weight[c + u];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(fmaxf(bn_pre(v[u][j], m, is, ga, be), 0.0f), wv, acc[j]);
                }
            }
            for (; c < c1; ++c) {
                const f32x4 v = ld4(src + (long)c * HW + p0);
                const float m = mean[c], is = invstd[c], ga = gamma[c], be = beta[c], wv = weight[c];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(fmaxf(bn_pre(v[j], m, is, ga, be), 0.0f), wv, acc[j]);
            }
        }
    } else {
        for (int c = c0; c < c1; ++c) {
            const float m = mean[c], is = invstd[c], ga = gamma[c], be = beta[c], wv = weight[c];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p0 + j < HW) acc[j] = fmaf(fmaxf(bn_pre(src[(long)c * HW + p0 + j], m, is, ga, be), 0.0f), wv, acc[j]);
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave != 0 || p0 >= HW) return;
    const float bz = bias ? bias[0] : 0.0f;
    const f32x4 s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    float *o = dst + ((long)grp * B + b) * HW + p0;
    if (vec_ok) {
        *(f32x4 *)o = f32x4{s[0] + bz, s[1] + bz, s[2] + bz, s[3] + bz};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < HW) o[j] = s[j] + bz;
    }
}

// logits[i] = bias + the G partial planes, groups ascending
__global__ __launch_bounds__(256) void oc_fwd_finish_kernel(const float *__restrict__ part, int G, long n, const float *__restrict__ bias,
                                                            float *__restrict__ logits)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int g = 1; g < G; ++g) s += part[(long)g * n + i];
    logits[i] = s + (bias ? bias[0] : 0.0f);
}

// ------------------------------------------------------------------------------------------------------------------------
// output layer: backward (BN = true: behind BatchNorm + ReLU, x = z; BN = false: the plain output conv)

// per tile of plane (b, c): {sum g a, sum g [a > 0], sum g [a > 0] xhat, sum g}
template <bool VEC, bool BN>
__global__ __launch_bounds__(256) void oc_bwd_reduce_kernel(const float *__restrict__ g, const float *__restrict__ x, int B, int C,
                                                            int HW, int ntp, const float *__restrict__ mean,
                                                            const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, f32x4 *__restrict__ ws)
{
    __shared__ float red[4];
    const int tile = blockIdx.x % ntp, plane = blockIdx.x / ntp;
    const int b = plane / C, c = plane - b * C;
    const int t0 = tile * BT;
    float xv[16], gv[16];
    bn_load<VEC>(xv, x + (long)plane * HW, t0, HW);
    bn_load<VEC>(gv, g + (long)b * HW, t0, HW);  // (padding: g = 0)
    float sga = 0.0f, sg = 0.0f, sgx = 0.0f, sb = 0.0f;
    if constexpr (BN) {
        const float m = mean[c], is = invstd[c], ga = gamma[c], be = beta[c];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pre = bn_pre(xv[r], m, is, ga, be);
            const float gm = pre > 0.0f ? gv[r] : 0.0f;
            sga = fmaf(gm, pre, sga);
            sg += gm;
            sgx = fmaf(gm, (xv[r] - m) * is, sgx);
            sb += gv[r];
        }
        sg = block_sum(sg, red);
        sgx = block_sum(sgx, red);
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sga = fmaf(gv[r], xv[r], sga);
            sb += gv[r];
        }
    }
    sga = block_sum(sga, red);
    if (c == 0) sb = block_sum(sb, red);  // (uniform over the workgroup)
    if (threadIdx.x == 0) ws[((long)c * B + b) * ntp + tile] = f32x4{sga, sg, sgx, sb};
}

// per channel (tiles ascending): the parameter gradients; coef = {grad_beta / n, grad_gamma / n} for the apply
__global__ __launch_bounds__(256) void oc_bwd_finish_kernel(const f32x4 *__restrict__ ws, int B, int C, int ntp, float inv_n,
                                                            const float *__restrict__ weight, float *__restrict__ grad_weight,
                                                            float *__restrict__ grad_bias, float *__restrict__ grad_gamma,
                                                            float *__restrict__ grad_beta, float *__restrict__ coef)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const f32x4 *src = ws + (long)c * B * ntp;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    const int nt = B * ntp;
    for (int i0 = 0; i0 < nt; i0 += 8) {  // (ascending; the loads of 8 in flight together)
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = i0 + u < nt ? src[i0 + u] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u < nt) s += v[u];
    }
    const float wv = weight[c], gbeta = wv * s[1], ggamma = wv * s[2];
    if (grad_weight) grad_weight[c] = s[0];
    if (grad_bias && c == 0) grad_bias[0] = s[3];
    if (grad_beta) grad_beta[c] = gbeta;
    if (grad_gamma) grad_gamma[c] = ggamma;
    if (coef) coef[2 * c] = gbeta * inv_n, coef[2 * c + 1] = ggamma * inv_n;
}

template <bool VEC, bool BN>
__global__ __launch_bounds__(256) void oc_bwd_apply_kernel(const float *__restrict__ g, const float *__restrict__ x, int C, int HW, int ntp,
                                                           const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           const float *__restrict__ weight, const float *__restrict__ coef,
                                                           float *__restrict__ dx)
{
    const int tile = blockIdx.x % ntp, plane = blockIdx.x / ntp;
    const int b = plane / C, c = plane - b * C;
    const int t0 = tile * BT;
    const long base = (long)plane * HW;
    float gv[16];
    bn_load<VEC>(gv, g + (long)b * HW, t0, HW);
    const float wv = weight[c];
    if constexpr (BN) {
        float xv[16];
        bn_load<VEC>(xv, x + base, t0, HW);
        const float m = mean[c], is = invstd[c], ga = gamma[c], be = beta[c], k = ga * is;
        const float cb = coef ? coef[2 * c] : 0.0f, cg = coef ? coef[2 * c + 1] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float gp = bn_pre(xv[r], m, is, ga, be) > 0.0f ? wv * gv[r] : 0.0f;
            gv[r] = coef ? k * ((gp - cb) - (xv[r] - m) * is * cg) : k * gp;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) gv[r] = wv * gv[r];
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

int oc_check(const char *what, int B, int C, int HW)
{
    if (B <= 0 || C <= 0 || HW <= 0) return manet_set_error(MANET_E_INVALID, "%s: sizes must be positive (B=%d C=%d HW=%d)", what, B, C, HW);
    if (B > 65535) return manet_set_error(MANET_E_INVALID, "%s: B=%d (at most 65535)", what, B);
    const long ntp = (HW + BT - 1) / BT;
    if ((long)B * C * ntp > 0x7fffffffL) return manet_set_error(MANET_E_INVALID, "%s: too many tiles", what);
    return MANET_OK;
}

// forward: [2 B C ntp floats: tile statistics][G B HW floats: partial logits, G > 1];  backward: [4 B C ntp][2 C: coef]
size_t oc_stats_floats(int B, int C, int HW) { return manet_align_up((size_t)2 * B * C * ((HW + BT - 1) / BT), 4); }

size_t oc_ws_bytes(int B, int C, int HW)
{
    const int G = oc_groups(B, C, HW);
    const size_t fwd = oc_stats_floats(B, C, HW) + (G > 1 ? (size_t)G * B * HW : 0);
    const size_t bwd = (size_t)4 * B * C * ((HW + BT - 1) / BT) + (size_t)2 * C;
    return (fwd > bwd ? fwd : bwd) * sizeof(float);
}

bool al16(const void *p) { return ((size_t)p & 15) == 0; }

template <bool BN>
void oc_launch_backward(const float *g, const float *x, int B, int C, int HW, const float *gamma, const float *beta, const float *mean,
                        const float *invstd, const float *weight, const float *coef_or_null, bool reduce, float *dx, float *gw, float *gb,
                        float *ggamma, float *gbeta, float *coef, f32x4 *tiles, hipStream_t st)
{
    const int ntp = (HW + BT - 1) / BT;
    const unsigned nb = (unsigned)((long)B * C * ntp), nc = (unsigned)((C + 255) / 256);
    const bool vec = HW % 4 == 0 && al16(g) && (!x || al16(x)) && (!dx || al16(dx));
    if (reduce) {
        if (vec) hipLaunchKernelGGL((oc_bwd_reduce_kernel<true, BN>), dim3(nb), dim3(256), 0, st, g, x, B, C, HW, ntp, mean, invstd, gamma, beta, tiles);
        else hipLaunchKernelGGL((oc_bwd_reduce_kernel<false, BN>), dim3(nb), dim3(256), 0, st, g, x, B, C, HW, ntp, mean, invstd, gamma, beta, tiles);
        hipLaunchKernelGGL(oc_bwd_finish_kernel, dim3(nc), dim3(256), 0, st, (const f32x4 *)tiles, B, C, ntp, (float)(1.0 / ((double)B * HW)),
                           weight, gw, gb, ggamma, gbeta, coef);
    }
    if (dx) {
        if (vec) hipLaunchKernelGGL((oc_bwd_apply_kernel<true, BN>), dim3(nb), dim3(256), 0, st, g, x, C, HW, ntp, mean, invstd, gamma, beta, weight, coef_or_null, dx);
        else hipLaunchKernelGGL((oc_bwd_apply_kernel<false, BN>), dim3(nb), dim3(256), 0, st, g, x, C, HW, ntp, mean, invstd, gamma, beta, weight, coef_or_null, dx);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// the head's two buffers

constexpr int NBLK = 4, PPB = 12, NPAR = NBLK * PPB + 2;  // MANET_HEAD_PARAMS
enum { P_W1 = 0, P_B1, P_G1, P_BE1, P_RM1, P_RV1, P_W2, P_B2, P_G2, P_BE2, P_RM2, P_RV2 };

struct HeadLayout {
    // `saved` (floats from its start): per block the depthwise output d, a1 = relu(bn1(d)), the conv2 output z, the block's
    // output (blocks 1-3: the next block's input), and the statistics the two BatchNorms used ([mean C][invstd C] each)
    size_t d[NBLK], a1[NBLK], z[NBLK], out[NBLK], st1[NBLK], st2[NBLK], saved_bytes;
    // `ws`: the launchers' scratch (one region, sized for the largest), a dummy depthwise grad_weight, two gradient buffers
    size_t scratch, scratch_bytes, dummy, ga, gb, ws_bytes;
};

size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

int head_check(const char *what, int B, int Cin, int Cmid, int h, int w, int K)
{
    if (K != 3 && K != 7) return manet_set_error(MANET_E_INVALID, "%s: K=%d (3 or 7)", what, K);
    if (B <= 0 || Cin <= 0 || Cmid <= 0 || h <= 0 || w <= 0)
        return manet_set_error(MANET_E_INVALID, "%s: sizes must be positive (B=%d Cin=%d Cmid=%d h=%d w=%d)", what, B, Cin, Cmid, h, w);
    if (B > 65535 || Cin > 65535 || Cmid > 65535)
        return manet_set_error(MANET_E_INVALID, "%s: B=%d Cin=%d Cmid=%d (at most 65535 each)", what, B, Cin, Cmid);
    // every launcher's tile count fits one launch: at most one workgroup per (plane, pixel)
    const long cmax = Cin > Cmid ? Cin : Cmid;
    if ((long)h * w > 0x7fffffffL / ((long)B * cmax + 8))
        return manet_set_error(MANET_E_INVALID, "%s: B * C * h * w must fit in 31 bits", what);
    return MANET_OK;
}

HeadLayout head_layout(int B, int Cin, int Cmid, int h, int w, int K)
{
    HeadLayout L;
    const size_t HW = (size_t)h * w, A = 64;  // pieces aligned to 64 floats (256 bytes)
    size_t o = 0, scratch = 0, n = 0;
    for (int i = 0; i < NBLK; ++i) {
        const int ci = i ? Cmid : Cin;
        L.d[i] = o, o += manet_align_up((size_t)B * ci * HW, A);
        L.a1[i] = o, o += manet_align_up((size_t)B * ci * HW, A);
        L.z[i] = o, o += manet_align_up((size_t)B * Cmid * HW, A);
        L.out[i] = o;
        if (i + 1 < NBLK) o += manet_align_up((size_t)B * Cmid * HW, A);  // (layer 4's is never written)
        L.st1[i] = o, o += manet_align_up((size_t)2 * ci, A);
        L.st2[i] = o, o += manet_align_up((size_t)2 * Cmid, A);
        manet_dwconv_backward_weight_workspace_bytes(B, ci, h, w, K, &n), scratch = max_sz(scratch, n);
        manet_pw_forward_workspace_bytes(B, ci, Cmid, (int)HW, &n), scratch = max_sz(scratch, n);
        manet_pw_backward_weight_workspace_bytes(B, ci, Cmid, (int)HW, &n), scratch = max_sz(scratch, n);
        manet_bn_relu_workspace_bytes(B, ci, (int)HW, &n), scratch = max_sz(scratch, n);
    }
    manet_bn_relu_workspace_bytes(B, Cmid, (int)HW, &n), scratch = max_sz(scratch, n);
    scratch = max_sz(scratch, oc_ws_bytes(B, Cmid, (int)HW));
    L.saved_bytes = o * sizeof(float);
    const size_t cmax = Cin > Cmid ? Cin : Cmid;
    o = 0;
    L.scratch = o, L.scratch_bytes = scratch, o += manet_align_up((scratch + 3) / 4, A);
    L.dummy = o, o += manet_align_up(cmax * K * K, A);
    L.ga = o, o += manet_align_up((size_t)B * cmax * HW, A);
    L.gb = o, o += manet_align_up((size_t)B * cmax * HW, A);
    L.ws_bytes = o * sizeof(float);
    return L;
}

int head_buffers(const char *what, const HeadLayout &L, const void *saved, size_t saved_bytes, const void *ws, size_t ws_bytes)
{
    if (!saved || saved_bytes < L.saved_bytes)
        return manet_set_error(MANET_E_INVALID, "%s: saved buffer of %zu bytes, %zu needed", what, saved ? saved_bytes : 0, L.saved_bytes);
    if (!ws || ws_bytes < L.ws_bytes)
        return manet_set_error(MANET_E_INVALID, "%s: workspace of %zu bytes, %zu needed", what, ws ? ws_bytes : 0, L.ws_bytes);
    if (!al16(saved) || !al16(ws)) return manet_set_error(MANET_E_INVALID, "%s: saved and workspace must be 16-byte aligned", what);
    return MANET_OK;
}

int head_params(const char *what, float *const *params, bool stats)
{
    if (!params) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer (params)", what);
    for (int i = 0; i < NPAR; ++i) {
        const int k = i < NBLK * PPB ? i % PPB : (i == NBLK * PPB ? P_W1 : P_B1);
        const bool optional = k == P_B1 || k == P_B2 || (!stats && (k == P_RM1 || k == P_RV1 || k == P_RM2 || k == P_RV2));
        if (!params[i] && !optional) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer (params[%d])", what, i);
    }
    return MANET_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// C ABI: the output layer

extern "C" int manet_out_conv_workspace_bytes(int B, int C, int HW, size_t *bytes)
{
    int rc = oc_check("manet_out_conv_workspace_bytes", B, C, HW);
    if (rc) return rc;
    if (!bytes) return manet_set_error(MANET_E_INVALID, "manet_out_conv_workspace_bytes: NULL pointer");
    *bytes = oc_ws_bytes(B, C, HW);
    return MANET_OK;
}

extern "C" int manet_bn_relu_outconv_forward_f32(const float *z, int B, int C, int HW, const float *gamma, const float *beta,
                                                 float *running_mean, float *running_var, float momentum, float eps, int training,
                                                 const float *weight, const float *bias, float *logits, float *save_mean,
                                                 float *save_invstd, void *ws, size_t ws_bytes, manet_stream_t stream)
{
    const char *what = "manet_bn_relu_outconv_forward_f32";
    int rc = oc_check(what, B, C, HW);
    if (rc) return rc;
    if (!z || !gamma || !beta || !weight || !logits || !save_mean || !save_invstd || (!training && (!running_mean || !running_var)))
        return manet_set_error(MANET_E_INVALID, "%s: NULL pointer", what);
    if (training && (long)B * HW < 2)
        return manet_set_error(MANET_E_INVALID, "%s: one value per channel in training (B=%d HW=%d)", what, B, HW);
    if (!(eps > 0.0f) || !(momentum >= 0.0f && momentum <= 1.0f))
        return manet_set_error(MANET_E_INVALID, "%s: eps=%g momentum=%g", what, (double)eps, (double)momentum);
    const int G = oc_groups(B, C, HW);
    const size_t need = oc_ws_bytes(B, C, HW);
    if ((training || G > 1) && (!ws || ws_bytes < need || !al16(ws)))
        return manet_set_error(MANET_E_INVALID, "%s: workspace of %zu bytes, %zu needed (16-byte aligned)", what, ws ? ws_bytes : 0, need);
    const hipStream_t st = (hipStream_t)stream;
    const int ntp = (HW + BT - 1) / BT;
    const unsigned nb = (unsigned)((long)B * C * ntp), nc = (unsigned)((C + 255) / 256);
    float *tiles = (float *)ws, *part = G > 1 ? (float *)ws + oc_stats_floats(B, C, HW) : nullptr;
    if (training) {
        if (HW % 4 == 0 && al16(z)) hipLaunchKernelGGL(bn_stats_kernel<true>, dim3(nb), dim3(256), 0, st, z, B, C, HW, ntp, tiles);
        else hipLaunchKernelGGL(bn_stats_kernel<false>, dim3(nb), dim3(256), 0, st, z, B, C, HW, ntp, tiles);
        hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(nc), dim3(256), 0, st, (const float *)tiles, B, C, HW, ntp, eps, momentum,
                           running_mean, running_var, save_mean, save_invstd);
    } else {
        hipLaunchKernelGGL(bn_eval_stats_kernel, dim3(nc), dim3(256), 0, st, (const float *)running_mean, (const float *)running_var, C,
                           eps, save_mean, save_invstd);
    }
    const int cpg = (C + G - 1) / G;
    const int vec = (HW % 4 == 0 && al16(z) && al16(logits)) ? 1 : 0;
    hipLaunchKernelGGL(oc_fwd_kernel, dim3((unsigned)((HW + OC_PX - 1) / OC_PX), (unsigned)G, (unsigned)B), dim3(256), 0, st, z, C, HW, cpg,
                       vec, (const float *)save_mean, (const float *)save_invstd, gamma, beta, weight, G > 1 ? nullptr : bias,
                       G > 1 ? part : logits);
    if (G > 1) {
        const long n = (long)B * HW;
        hipLaunchKernelGGL(oc_fwd_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float *)part, G, n, bias, logits);
    }
    return manet_check_launch(what);
}

extern "C" int manet_bn_relu_outconv_backward_f32(const float *grad_logits, const float *z, int B, int C, int HW, const float *gamma,
                                                  const float *beta, const float *save_mean, const float *save_invstd, int training,
                                                  const float *weight, float *grad_z, float *grad_weight, float *grad_bias,
                                                  float *grad_gamma, float *grad_beta, void *ws, size_t ws_bytes, manet_stream_t stream)
{
    const char *what = "manet_bn_relu_outconv_backward_f32";
    int rc = oc_check(what, B, C, HW);
    if (rc) return rc;
    if (!grad_logits || !z || !gamma || !beta || !save_mean || !save_invstd || !weight)
        return manet_set_error(MANET_E_INVALID, "%s: NULL pointer", what);
    const bool reduce = grad_weight || grad_bias || grad_gamma || grad_beta || (training && grad_z);
    const size_t need = oc_ws_bytes(B, C, HW);
    if (reduce && (!ws || ws_bytes < need || !al16(ws)))
        return manet_set_error(MANET_E_INVALID, "%s: workspace of %zu bytes, %zu needed (16-byte aligned)", what, ws ? ws_bytes : 0, need);
    float *coef = reduce ? (float *)ws + (size_t)4 * B * C * ((HW + BT - 1) / BT) : nullptr;
    oc_launch_backward<true>(grad_logits, z, B, C, HW, gamma, beta, save_mean, save_invstd, weight, training ? coef : nullptr, reduce, grad_z,
                             grad_weight, grad_bias, grad_gamma, grad_beta, coef, (f32x4 *)ws, (hipStream_t)stream);
    return manet_check_launch(what);
}

extern "C" int manet_out_conv_forward_f32(const float *in, int B, int C, int HW, const float *weight, const float *bias, float *out,
                                          manet_stream_t stream)
{
    int rc = oc_check("manet_out_conv_forward_f32", B, C, HW);
    if (rc) return rc;
    if (!in || !weight || !out) return manet_set_error(MANET_E_INVALID, "manet_out_conv_forward_f32: NULL pointer");
    return manet_relu_conv1x1_c1_f32(in, B, C, HW, weight, bias, 0, out, stream);
}

extern "C" int manet_out_conv_backward_f32(const float *grad_out, const float *in, int B, int C, int HW, const float *weight,
                                           float *grad_in, float *grad_weight, float *grad_bias, void *ws, size_t ws_bytes,
                                           manet_stream_t stream)
{
    const char *what = "manet_out_conv_backward_f32";
    int rc = oc_check(what, B, C, HW);
    if (rc) return rc;
    const bool reduce = grad_weight || grad_bias;
    if (!grad_out || !weight || (reduce && !in)) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer", what);
    const size_t need = oc_ws_bytes(B, C, HW);
    if (reduce && (!ws || ws_bytes < need || !al16(ws)))
        return manet_set_error(MANET_E_INVALID, "%s: workspace of %zu bytes, %zu needed (16-byte aligned)", what, ws ? ws_bytes : 0, need);
    oc_launch_backward<false>(grad_out, in, B, C, HW, nullptr, nullptr, nullptr, nullptr, weight, nullptr, reduce, grad_in, grad_weight,
                              grad_bias, nullptr, nullptr, nullptr, (f32x4 *)ws, (hipStream_t)stream);
    return manet_check_launch(what);
}

// ---------------------------------------------------------------------------------------------------------------------------
// C ABI: the head

extern "C" int manet_head_train_bytes(int B, int Cin, int Cmid, int h, int w, int K, size_t *saved_bytes, size_t *ws_bytes)
{
    int rc = head_check("manet_head_train_bytes", B, Cin, Cmid, h, w, K);
    if (rc) return rc;
    if (!saved_bytes || !ws_bytes) return manet_set_error(MANET_E_INVALID, "manet_head_train_bytes: NULL pointer");
    const HeadLayout L = head_layout(B, Cin, Cmid, h, w, K);
    *saved_bytes = L.saved_bytes, *ws_bytes = L.ws_bytes;
    return MANET_OK;
}

#define HEAD_TRY(call)     \
    do {                   \
        rc = (call);       \
        if (rc) return rc; \
    } while (0)

extern "C" int manet_head_train_forward_f32(const float *x, int B, int Cin, int Cmid, int h, int w, int K, float *const *params,
                                            const int *training, const float *momentum, const float *eps, void *saved,
                                            size_t saved_bytes, void *ws, size_t ws_bytes, float *logits, manet_stream_t stream)
{
    const char *what = "manet_head_train_forward_f32";
    int rc = head_check(what, B, Cin, Cmid, h, w, K);
    if (rc) return rc;
    if (!x || !training || !momentum || !eps || !logits) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer", what);
    HEAD_TRY(head_params(what, params, true));
    const int HW = h * w;
    for (int i = 0; i < 2 * NBLK; ++i) {
        if (training[i] && (long)B * HW < 2)
            return manet_set_error(MANET_E_INVALID, "%s: one value per channel in training (B=%d h*w=%d)", what, B, HW);
        if (!(eps[i] > 0.0f) || !(momentum[i] >= 0.0f && momentum[i] <= 1.0f))
            return manet_set_error(MANET_E_INVALID, "%s: BatchNorm %d: eps=%g momentum=%g", what, i, (double)eps[i], (double)momentum[i]);
    }
    const HeadLayout L = head_layout(B, Cin, Cmid, h, w, K);
    HEAD_TRY(head_buffers(what, L, saved, saved_bytes, ws, ws_bytes));
    float *S = (float *)saved, *W = (float *)ws;
    void *scratch = W + L.scratch;
    const float *in = x;
    for (int i = 0; i < NBLK; ++i) {
        float *const *p = params + i * PPB;
        const int ci = i ? Cmid : Cin;
        float *d = S + L.d[i], *a1 = S + L.a1[i], *z = S + L.z[i], *st1 = S + L.st1[i], *st2 = S + L.st2[i];
        HEAD_TRY(manet_dwconv_forward_f32(in, B, ci, h, w, K, p[P_W1], p[P_B1], d, stream));
        HEAD_TRY(manet_bn_relu_forward_f32(d, B, ci, HW, p[P_G1], p[P_BE1], p[P_RM1], p[P_RV1], momentum[2 * i], eps[2 * i], training[2 * i],
                                           a1, st1, st1 + ci, scratch, L.scratch_bytes, stream));
        HEAD_TRY(manet_pw_forward_f32(a1, B, ci, Cmid, HW, p[P_W2], p[P_B2], z, scratch, L.scratch_bytes, stream));
        if (i + 1 < NBLK) {
            float *out = S + L.out[i];
            HEAD_TRY(manet_bn_relu_forward_f32(z, B, Cmid, HW, p[P_G2], p[P_BE2], p[P_RM2], p[P_RV2], momentum[2 * i + 1], eps[2 * i + 1],
                                               training[2 * i + 1], out, st2, st2 + Cmid, scratch, L.scratch_bytes, stream));
            in = out;
        } else {
            HEAD_TRY(manet_bn_relu_outconv_forward_f32(z, B, Cmid, HW, p[P_G2], p[P_BE2], p[P_RM2], p[P_RV2], momentum[2 * i + 1],
                                                       eps[2 * i + 1], training[2 * i + 1], params[NBLK * PPB], params[NBLK * PPB + 1],
                                                       logits, st2, st2 + Cmid, scratch, L.scratch_bytes, stream));
        }
    }
    return MANET_OK;
}

extern "C" int manet_head_train_backward_f32(const float *grad_logits, const float *x, int B, int Cin, int Cmid, int h, int w, int K,
                                             float *const *params, const int *training, const void *saved, size_t saved_bytes, void *ws,
                                             size_t ws_bytes, float *const *grads, float *grad_x, manet_stream_t stream)
{
    const char *what = "manet_head_train_backward_f32";
    int rc = head_check(what, B, Cin, Cmid, h, w, K);
    if (rc) return rc;
    if (!grad_logits || !x || !training || !grads) return manet_set_error(MANET_E_INVALID, "%s: NULL pointer", what);
    HEAD_TRY(head_params(what, params, false));
    const HeadLayout L = head_layout(B, Cin, Cmid, h, w, K);
    HEAD_TRY(head_buffers(what, L, saved, saved_bytes, ws, ws_bytes));
    const float *S = (const float *)saved;
    float *W = (float *)ws;
    void *scratch = W + L.scratch;
    float *ga = W + L.ga, *gb = W + L.gb, *dummy = W + L.dummy;
    const int HW = h * w;
    auto wanted = [&](int lo, int hi) {  // a parameter gradient asked for among grads[lo .. hi)
        for (int j = lo; j < hi; ++j) {
            const int k = j % PPB;
            const bool stat = j < NBLK * PPB && (k == P_RM1 || k == P_RV1 || k == P_RM2 || k == P_RV2);
            if (grads[j] && !stat) return true;
        }
        return false;
    };
    // the gradient of a block's output arrives in gb (layer 4: grad_logits, through the fused kernels); ga and gb alternate.
    // Each stage runs only if something in front of it wants a gradient.
    for (int i = NBLK - 1; i >= 0; --i) {
        float *const *p = params + i * PPB, *const *q = grads + i * PPB;
        const int ci = i ? Cmid : Cin;
        const float *in = i ? S + L.out[i - 1] : x, *d = S + L.d[i], *a1 = S + L.a1[i], *z = S + L.z[i];
        const float *st1 = S + L.st1[i], *st2 = S + L.st2[i];
        const bool need_in = grad_x || wanted(0, i * PPB);           // the gradient of the block's input
        const bool need_d = need_in || q[P_W1] || q[P_B1];           // ... of the depthwise output d
        const bool need_a1 = need_d || q[P_G1] || q[P_BE1];          // ... of a1 = relu(bn1(d))
        const bool need_z = need_a1 || q[P_W2] || q[P_B2];           // ... of the conv2 output z
        if (i == NBLK - 1) {
            HEAD_TRY(manet_bn_relu_outconv_backward_f32(grad_logits, z, B, Cmid, HW, p[P_G2], p[P_BE2], st2, st2 + Cmid, training[2 * i + 1],
                                                        params[NBLK * PPB], need_z ? ga : nullptr, grads[NBLK * PPB],
                                                        grads[NBLK * PPB + 1], q[P_G2], q[P_BE2], scratch, L.scratch_bytes, stream));
        } else if (need_z || q[P_G2] || q[P_BE2]) {
            HEAD_TRY(manet_bn_relu_backward_f32(gb, z, B, Cmid, HW, p[P_G2], p[P_BE2], st2, st2 + Cmid, training[2 * i + 1],
                                                need_z ? ga : nullptr, q[P_G2], q[P_BE2], scratch, L.scratch_bytes, stream));
        }
        if (!need_z) break;
        if (q[P_W2] || q[P_B2])
            HEAD_TRY(manet_pw_backward_weight_f32(a1, ga, B, ci, Cmid, HW, q[P_W2], q[P_B2], scratch, L.scratch_bytes, stream));
        if (!need_a1) break;
        HEAD_TRY(manet_pw_backward_data_f32(ga, B, ci, Cmid, HW, p[P_W2], gb, stream));
        HEAD_TRY(manet_bn_relu_backward_f32(gb, d, B, ci, HW, p[P_G1], p[P_BE1], st1, st1 + ci, training[2 * i], need_d ? ga : nullptr, q[P_G1],
                                            q[P_BE1], scratch, L.scratch_bytes, stream));
        if (!need_d) break;
        if (q[P_W1] || q[P_B1])  // (the launcher wants a grad_weight: a dummy when only the bias is asked for)
            HEAD_TRY(manet_dwconv_backward_weight_f32(in, ga, B, ci, h, w, K, q[P_W1] ? q[P_W1] : dummy, q[P_B1], scratch, L.scratch_bytes,
                                                      stream));
        if (!need_in) break;
        HEAD_TRY(manet_dwconv_backward_data_f32(ga, B, ci, h, w, K, p[P_W1], i ? gb : grad_x, stream));
    }
    return MANET_OK;
}
