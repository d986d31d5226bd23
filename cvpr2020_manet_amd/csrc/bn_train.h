// BatchNorm statistics over tiles of one (b, c) plane, shared by pw_train.hip (BatchNorm + ReLU) and head_train.hip (BatchNorm +
// ReLU + the head's output layer): the tile loads, the pre-activation both directions recompute bit for bit, the fixed-order
// workgroup sum, and the statistics kernels (per-tile (mean, M2) -> Chan's merge in double, tiles ascending -> mean, invstd and
// the running buffers updated as nn.BatchNorm2d does; or mean / invstd from the running statistics in eval).  Included inside
// each file's anonymous namespace: every translation unit carries its own copies of the kernels.
#pragma once

__device__ __forceinline__ f32x4 ld4(const float *p) { return *(const f32x4 *)p; }

constexpr int BT = 4096;  // elements per tile: 256 threads x 16

// the pre-activation, one rounding per op (the backward's mask is this, recomputed bit for bit)
__device__ __forceinline__ float bn_pre(float x, float mean, float invstd, float gamma, float beta)
{
    return (x - mean) * invstd * gamma + beta;
}

// a tile's 16 values per thread: element o of the plane for thread slot r (o < n; others 0 and not counted)
template <bool VEC>
__device__ __forceinline__ void bn_load(float (&v)[16], const float *__restrict__ src, int t0, int n)
{
    if constexpr (VEC) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = t0 + 4 * threadIdx.x + 1024 * r;
            f32x4 u = {0.0f, 0.0f, 0.0f, 0.0f};
            if (o < n) u = ld4(src + o);  // (n % 4 == 0)
            v[4 * r] = u[0], v[4 * r + 1] = u[1], v[4 * r + 2] = u[2], v[4 * r + 3] = u[3];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = t0 + threadIdx.x + 256 * r;
            v[r] = o < n ? src[o] : 0.0f;
        }
    }
}

template <bool VEC>
__device__ __forceinline__ int bn_off(int r)
{
    return VEC ? 4 * (int)threadIdx.x + 1024 * (r >> 2) + (r & 3) : (int)threadIdx.x + 256 * r;
}

// sum of one value per thread in a fixed order (lane butterflies, then the four waves); the result reaches every thread
__device__ __forceinline__ float block_sum(float v, float *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();  // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// per tile: (mean, M2) of its elements
template <bool VEC>
__global__ __launch_bounds__(256) void bn_stats_kernel(const float *__restrict__ x, int B, int C, int HW, int ntp, float *__restrict__ ws)
{
    __shared__ float red[4];
    const int tile = blockIdx.x % ntp, plane = blockIdx.x / ntp;
    const int b = plane / C, c = plane - b * C;
    const int t0 = tile * BT, cnt = min(BT, HW - t0);
    float v[16];
    bn_load<VEC>(v, x + (long)plane * HW, t0, HW);
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s += v[r];
    const float mean = block_sum(s, red) / (float)cnt;
    float m2 = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float d = v[r] - mean;
        if (t0 + bn_off<VEC>(r) < HW) m2 = fmaf(d, d, m2);
    }
    m2 = block_sum(m2, red);
    if (threadIdx.x == 0) {
        float *dst = ws + 2 * (((long)c * B + b) * ntp + tile);
        dst[0] = mean, dst[1] = m2;
    }
}

// per channel: merge the tiles (b ascending, tile ascending), statistics and running buffers
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const float *__restrict__ ws, int B, int C, int HW, int ntp, float eps,
                                                              float momentum, float *__restrict__ running_mean,
                                                              float *__restrict__ running_var, float *__restrict__ save_mean,
                                                              float *__restrict__ save_invstd)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float *src = ws + 2L * c * B * ntp;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    const int nt = B * ntp;
    for (int i0 = 0; i0 < nt; i0 += 8) {  // (tiles in ascending order; the loads of 8 in flight together)
        f32x2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = i0 + u < nt ? *(const f32x2 *)(src + 2 * (i0 + u)) : f32x2{0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (i0 + u >= nt) break;
            const int t = (i0 + u) % ntp;
            const double nb = (double)min(BT, HW - t * BT), mb = v[u][0], qb = v[u][1];
            const double nn = n + nb, d = mb - mean;
            mean += d * (nb / nn);
            m2 += qb + d * d * (n * nb / nn);
            n = nn;
        }
    }
    const double var = m2 / n;
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) running_mean[c] = momentum * (float)mean + (1.0f - momentum) * running_mean[c];
    if (running_var) running_var[c] = momentum * (float)(var * n / (n - 1.0)) + (1.0f - momentum) * running_var[c];
}

__global__ __launch_bounds__(256) void bn_eval_stats_kernel(const float *__restrict__ running_mean, const float *__restrict__ running_var,
                                                            int C, float eps, float *__restrict__ save_mean, float *__restrict__ save_invstd)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    save_mean[c] = running_mean[c];
    save_invstd[c] = 1.0f / sqrtf(running_var[c] + eps);
}
