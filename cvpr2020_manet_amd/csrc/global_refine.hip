// Global nearest-neighbour matching, MANET_COMPUTE_BF16_REFINE and MANET_COMPUTE_F16_REFINE.  The threshold, re-rank and statistics kernels live here; the
// pre-pass, the filter and the rescue are forms of the main kernels, launched through launch_match (csrc/global_match.hip).
//
// MANET_COMPUTE_BF16_REFINE: fp32-exact minima at bf16 cost (VERDICT r2 "next" #4).
//   IntVOS.py:81-85 is a MINIMUM over the bank, so any filter that keeps the true arg-min row may discard the rest:
//   1. pre-pass  : the plain bf16 kernel over every REFINE_SUB-th bank tile -> U(n,o), a bf16 distance of SOME row, i.e. an
//                  upper bound (to within the rounding bound E) of the minimum;
//   2. threshold : thr(n,o) = U + 2 E(n,o), E from |q_n|, max |k| and U (below): every row m with fp32 distance
//                  <= the fp32 minimum has bf16 distance <= thr;
//   3. filter    : the bf16 wide kernel over the WHOLE bank (FILTER form) appends the rows with bf16 distance <= thr to the
//                  pair's candidate list (REFINE_CAP slots);
//   4. re-rank   : the candidates are re-evaluated in the reference's fp32 arithmetic -- the oracle's fmaf chains, from
//                  the fp32 copy of the sorted bank -- and reduced; a pair whose list overflowed scans its object's rows
//                  instead.  The result is the fp32 kernel's, bit for bit.
// The bound: with u = 2^-9 (bf16 round-to-nearest), q~ = bf16(q), k~ = bf16(k), e = (q~ - q) - (k~ - k), |e| <= u (|q| + |k|):
//   | |q~ - k~|^2 - |q - k|^2 | = | 2 (q - k).e + |e|^2 | <= 2 u s sqrt(d) + u^2 s^2,   s = |q| + max |k|,  d = |q - k|^2
// plus the fp32 accumulation error of either evaluation (a = 8 (C + 8) 2^-24 s^2, generous).  For the two rows that matter
// (the pre-pass's best row and the true arg-min) d <= U + E0 + a with the crude E0 = (2u + u^2) s^2 + a, hence
//   E = 2 u s sqrt(max(U, 0) + E0 + a) + u^2 s^2 + a   bounds both, and thr = U + 2 E (x 1.05 against the bound's own rounding).
//
// MANET_COMPUTE_F16_REFINE: the same five steps with the pre-pass and the filter in fp16 arithmetic on the fp16 images (the
// re-rank, the rescue and the statistics are shared).  Its bound, with u = 2^-11 (fp16 round-to-nearest) -- the threshold's leading
// term 2 u s sqrt(U) is 8x bf16's true one (bf16's u is 2^-8; the 2^-9 above is carried by the crude s and the 2.1):
//   Elements.  x~ = fp16(x).  A NORMAL x~ has |x~ - x| <= u |x|.  An x~ that is zero or subnormal has |x~ - x| <= 2^-25.  The
//   matrix pipe may keep a nonzero subnormal operand or flush it to zero (the project leaves that open): the operand it USES, x^,
//   then differs from x by less than 2^-14.  (The query image holds -2 q~, a subnormal of which comes from a subnormal q~.)
//   With n_q = the number of nonzero subnormal elements of the rounded query row, n_k = the maximum of that count over the bank's
//   in-domain rows, and e = (q^ - q) - (k^ - k):
//     |e| <= u (|q| + |k|) + 2^-14 (sqrt(n_q) + sqrt(n_k)) + 2^-24 sqrt(C)                                   =: eps
//   Distances.  The MFMA chain gives |q~|^2 + |k~|^2 - 2 q^.k^: the norm slots hold the norms of the ROUNDED rows, flushed or
//   not.  q~ = q^ + f_q with f_q the flushed elements (disjoint support, |f_q|^2 <= 2^-28 n_q), so this is
//     |q^ - k^|^2 + |f_q|^2 + |f_k|^2,   and   |q^ - k^|^2 - |q - k|^2 = 2 (q - k).e + |e|^2:
//     | d~ - d | <= 2 sqrt(d) eps + eps^2 + 2^-28 (n_q + n_k) + 2 * 2^-28 + a <= 2 sqrt(d) eps + 2 eps^2 + 2^-27 + a
//   (2^-28 (n_q + n_k) <= eps^2; 2^-28 per side: what the scaled norm pieces drop of a norm below 2^-5, global_match_common.h;
//   a = 8 (C + 8) 2^-24 s^2 as above, the fp32 accumulation of either evaluation).  s = |q| + max |k| >= sqrt(d) gives the crude
//   E0 = 2 s eps + 2 eps^2 + 2^-27 + a, and, as above, for the two rows that matter
//     E = 2 eps sqrt(max(U, 0) + E0 + a) + 2 eps^2 + 2^-27 + a,   thr = U + 2 E (x 1.05).
//   |q|, |k| come from the images' norms of the rounded rows: |x| <= (|x~| + 2^-25 sqrt(C)) / (1 - u), so
//   s <= 1.001 (|q~| + max |k~|) + 2^-24 sqrt(C).
// Rows outside fp16's domain (NaN in the image's first norm slot; fp32 has a value for them): see refine_threshold_f16_kernel.
#include "global_match_common.h"

namespace {

// |q~_n|^2 out of the bf16 query image: the three bf16 pieces in k slots C+3 .. C+5 (see Geom)
__device__ __forceinline__ float query_norm_from_image(const char *qimg, long qblk_bytes, long n, int C)
{
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int k = C + 3 + i, u = 2 * (k >> 4) + ((k >> 3) & 1), e = k & 7;
        const unsigned short b = *(const unsigned short *)(qimg + (n >> 5) * qblk_bytes + ((long)u * QB + (n & 31)) * 16 + e * 2);
        s += bf2f(b);  // hi + mid + lo: exact in fp32
    }
    return s;
}

__global__ void refine_threshold_kernel(const unsigned *__restrict__ keys, const char *__restrict__ qimg, long qblk_bytes,
                                        int C, const int *__restrict__ meta, long N, long N_pad, int n_ids,
                                        unsigned *__restrict__ thr, float *__restrict__ slack, unsigned *__restrict__ keys2,
                                        unsigned long long *__restrict__ stats, unsigned *__restrict__ bcnt)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) stats[0] = stats[1] = 0ull;
    if (i <= 2 * (N_pad / QB)) bcnt[i] = 0u;  // (entries appended, dense entries appended, number of tiles to rescue)
    if (i >= (long)n_ids * N_pad) return;
    const long n = i % N_pad;
    const int o = (int)(i / N_pad);
    unsigned k2 = 0xffffffffu;  // "no row": the exact distances meet here by atomicMin
    const unsigned k = keys[i];
    float t = -INFINITY, sl = 0.0f;  // no row of this object anywhere: no candidates, the result is the padding distance
    if (k != 0xffffffffu && n < N) {
        const float U = float_of(k);
        const float u = 0.001953125f;  // 2^-9
        const float qn2 = query_norm_from_image(qimg, qblk_bytes, n, C);
        // NaN embeddings: a NaN in the query row, or in any row of this object, makes every distance of the pair's
        // minimum NaN in MANET_COMPUTE_F32 (min3p propagates it): the pair's exact key is NaN's (0, it wins every atomicMin) --
        // no threshold is meaningful for it, and none is needed
        if (qn2 != qn2 || meta[META_NAN + o]) k2 = 0u;
        const float qn = sqrtf(fmaxf(qn2, 0.0f)) * 1.004f;  // |q| <= |q~| / (1 - u)
        const float kn = sqrtf(__uint_as_float((unsigned)meta[META_KMAX])) * 1.0001f;
        const float s = qn + kn, s2 = s * s;
        const float a = 8.0f * (float)(C + 8) * 5.9604645e-8f * s2;
        const float E0 = (2.0f * u + u * u) * s2 + a;
        const float E = 2.0f * u * s * sqrtf(fmaxf(U, 0.0f) + E0 + a) + u * u * s2 + a;
        sl = 2.1f * E;
        t = U + sl;  // (NaN stays NaN: no candidates; such a pair's result was settled above)
    }
    keys2[i] = k2;
    thr[i] = key_of(t);  // as an order-preserving key: the filter pass's workgroups tighten it by atomicMin
    slack[i] = sl;       // ... to (smallest bf16 distance they met) + slack: E only shrinks with U
}

// MANET_COMPUTE_F16_REFINE's form of the kernel above: one thread per QUERY (it reads its row of the fp16 image once: the scaled
// norm pieces, the subnormal count, NaN and infinity elements), a loop over the objects.  256 threads = eight 32-query blocks, a
// half-wave per block, so the block's counter is written ONCE, by its first lane, with the "incomplete" mark (bit 31: the
// rescue pass -- the exact fp32 kernel -- takes the block's 256-query tile) already in it when the filter may not speak for the
// block: a query of it lies outside fp16's domain (finite with a norm slot of NaN, or an infinity: fp32 has distances for it), or a
// bank row does (META_F16_OOD: every block, the filter pass returns at once).  Distances of such rows are NaN in fp16: the
// pre-pass's U of their pairs is NaN and their thresholds admit nothing, which no longer matters.  A NaN QUERY element settles
// the pixel as in bf16r (every distance of the row is NaN in fp32 too).
__global__ __launch_bounds__(256) void refine_threshold_f16_kernel(const unsigned *__restrict__ keys, const char *__restrict__ qimg,
                                                                   long qblk_bytes, int units, int C, const int *__restrict__ meta,
                                                                   long N, long N_pad, int n_ids, unsigned *__restrict__ thr,
                                                                   float *__restrict__ slack, unsigned *__restrict__ keys2,
                                                                   unsigned long long *__restrict__ stats,
                                                                   unsigned *__restrict__ bcnt)
{
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (the grid covers N_pad exactly: a multiple of 512)
    if (n == 0) stats[0] = stats[1] = 0ull;
    const long nb = N_pad / QB;
    if (n >= nb && n <= 2 * nb) bcnt[n] = 0u;  // (dense entries appended, number of tiles to rescue; nb < 2 nb + 1 <= N_pad)
    const char *row = qimg + (n >> 5) * qblk_bytes + (n & 31) * 16;  // unit u of this query: row + u * QB * 16
    auto elem = [&](int k) {
        const int u = 2 * (k >> 4) + ((k >> 3) & 1);
        return (unsigned)*(const unsigned short *)(row + (long)u * QB * 16 + (k & 7) * 2);
    };
    int sub = 0;
    bool has_nan = false, has_inf = false;
    for (int u = 0; u < units; ++u) {
        const uint4 v = *(const uint4 *)(row + (long)u * QB * 16);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        const int k0 = 16 * (u >> 1) + 8 * (u & 1);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned b = (w[e >> 1] >> (16 * (e & 1))) & 0x7fffu;  // |-2 q~|
            const bool in = k0 + e < C;
            sub += (in && b != 0u && b < 0x0800u) ? 1 : 0;  // q~ nonzero and below 2^-14
            has_nan = has_nan || (in && b > 0x7c00u);
            has_inf = has_inf || (in && b == 0x7c00u);
        }
    }
    const unsigned p0 = elem(C + 3);
    const bool slot_nan = (p0 & 0x7fffu) > 0x7c00u;
    const float qn2 = h2f(p0) + h2f(elem(C + 4)) * (1.0f / 2048.0f) + h2f(elem(C + 5)) * (1.0f / 16384.0f);
    const bool bank_ood = meta[META_F16_OOD] != 0;
    const bool exact = n < N && (bank_ood || (!has_nan && (has_inf || slot_nan)));
    const bool mark = (__ballot(exact) >> (threadIdx.x & 32) & 0xffffffffull) != 0ull;  // this 32-query block's lanes
    if ((n & 31) == 0) bcnt[n >> 5] = mark ? 0x80000000u : 0u;
    const float u = 4.8828125e-4f;  // 2^-11
    const float tiny = 6.1035156e-5f * (sqrtf((float)sub) + sqrtf((float)meta[META_F16_SUBN])) + 5.9604645e-8f * sqrtf((float)C);
    const float kn = sqrtf(__uint_as_float((unsigned)meta[META_F16_KMAX]));
    const float s = 1.001f * (sqrtf(fmaxf(qn2, 0.0f)) + kn) + 5.9604645e-8f * sqrtf((float)C), s2 = s * s;
    const float eps = u * s + tiny;
    const float a = 8.0f * (float)(C + 8) * 5.9604645e-8f * s2;
    const float fix = 2.0f * eps * eps + 7.4505806e-9f + a;  // 2 eps^2 + 2^-27 + a
    const float E0 = 2.0f * s * eps + fix;
    for (int o = 0; o < n_ids; ++o) {
        const long i = (long)o * N_pad + n;
        unsigned k2 = 0xffffffffu;  // "no row": the exact distances meet here by atomicMin
        const unsigned k = keys[i];
        float t = -INFINITY, sl = 0.0f;  // no row of this object anywhere: no candidates, the result is the padding distance
        if (k != 0xffffffffu && n < N) {
            const float U = float_of(k);
            if (has_nan || meta[META_NAN + o]) k2 = 0u;  // (as in refine_threshold_kernel)
            const float E = 2.0f * eps * sqrtf(fmaxf(U, 0.0f) + E0 + a) + fix;
            sl = 2.1f * E;
            t = exact ? -INFINITY : U + sl;  // (NaN stays NaN: no candidates)
        }
        keys2[i] = k2;
        thr[i] = key_of(t);
        slack[i] = sl;
    }
}

// MANET_EPI_REFINE_EXACT: no filter at all -- every 32-query block is marked incomplete, so the re-rank launch only writes the
// fp32 query images and the rescue pass (the exact fp32 kernel) takes every tile: the fp32 path's cost + ~0.03 ms, for callers
// that KNOW (ops.PreparedBank: from the previous frame's rescue share) that the bf16 pass cannot tell these embeddings apart
__global__ void refine_force_kernel(long N_pad, int n_ids, unsigned *__restrict__ keys2, unsigned long long *__restrict__ stats,
                                    unsigned *__restrict__ bcnt)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        stats[0] = 0ull;
        stats[1] = 1ull;
    }
    if (i < N_pad / QB) bcnt[i] = 0x80000000u;
    if (i == 0) bcnt[2 * (N_pad / QB)] = 0u;  // (the re-rank launch lists the tiles to rescue: all of them)
    if (i < (long)n_ids * N_pad) keys2[i] = 0xffffffffu;
}

// how many 256-query tiles of the last filter pass went through the rescue pass -> out2 = {rescued, tiles} (device memory: the
// caller copies it out asynchronously and reads it a frame later)
__global__ void refine_rescued_kernel(const unsigned *__restrict__ bcnt, long tiles, long bucket_cap, int *__restrict__ out2)
{
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int mine = 0;
    for (long t = threadIdx.x; t < tiles; t += blockDim.x) {
        bool need = false;
        for (int i = 0; i < QT / QB; ++i) {
            const unsigned raw = bcnt[t * (QT / QB) + i];
            need = need || (raw >> 31) || (long)raw > bucket_cap;
        }
        mine += need ? 1 : 0;
    }
    atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        out2[0] = cnt;
        out2[1] = (int)tiles;
    }
}

// exact re-rank: one workgroup per bucket of the candidate list (= 32 neighbouring queries, every object), one thread per
// candidate {pair, bank slot}: the reference's fp32 distance (the oracle's fmaf chains, IntVOS.py:32-39) of that (query,
// bank row), reduced per pair by atomicMin on the order-preserving key; the usual finish kernel decodes the keys.
// The block's 32 query vectors are read ONCE, coalesced, into LDS as [channel][query] (same query: broadcast, different
// queries: different banks) -- with a flat list in emission order a wave's candidates spread over a filter workgroup's 512
// queries, so each of the 100 query loads touched ~14 cache lines: measured, the query gather cost as much as the bank-row
// gather (48 us each of the kernel's 87 at cfg3 shape; tools/ history in DESIGN.md 3.2b).  A lane's bank row is read 32
// channels per round, all eight 16-byte loads issued together: one 128-byte line's worth, crossing L2 -> L1 once.
template <typename SRC>
__global__ __launch_bounds__(256) void refine_rerank_kernel(const SRC *__restrict__ q, long q_sn, long q_sc,
                                                            const float *__restrict__ rows, const float *__restrict__ norms,
                                                            const uint2 *__restrict__ list, unsigned *__restrict__ bcnt,
                                                            long bucket_cap, long N, long N_pad, int C,
                                                            unsigned *__restrict__ keys2, unsigned long long *__restrict__ stats,
                                                            char *__restrict__ q32, int units32, long qblk_bytes32)
{
    extern __shared__ __attribute__((aligned(16))) char rr_smem[];
    float *qs = (float *)rr_smem;  // [C][QB]
    const long b = blockIdx.x;
    const unsigned raw = bcnt[b], have = raw & 0x7fffffffu;  // (bit 31: a block's hits were not listed, see emit)
    const int cnt = (long)have < bucket_cap ? (int)have : (int)bucket_cap;
    const int tid = threadIdx.x;
    if (((long)have > bucket_cap || (raw >> 31)) && tid == 0) stats[1] = 1ull;  // (statistics; the rescue pass looks at bcnt itself)
    // the rescue pass (the exact fp32 kernel) takes every 256-query tile that holds an incomplete bucket: the blocks of such
    // a tile also write their fp32 operand image here, where the block's queries are in LDS anyway (a separate pack launch
    // cost 5 us per healthy frame)
    bool rescue = false;
    {
        const long t0 = b / (QT / QB) * (QT / QB);
        for (int i = 0; i < QT / QB; ++i) {
            const unsigned r2 = bcnt[t0 + i];
            rescue = rescue || (r2 >> 31) || (long)r2 > bucket_cap;
        }
    }
    // this workgroup's share of the bucket: entries z, z + zn, ... -- zn of the launch's REFINE_RZ workgroups per bucket take
    // part: one per 512 entries, a dense entry (a 32 x 32 x C matrix tile for one wave) counted as 64 listed rows.  (All four on
    // every bucket: 4 x the query-block loads and a quarter of the work each -- +8 us of the re-rank on video-like data, where a
    // bucket holds ~320 rows; one: -45 us on smooth data, where the longest bucket is the launch's time.)
    const int z = blockIdx.y;
    int zn = (int)(((long)cnt + 64l * (long)bcnt[N_pad / QB + b] + 511) / 512);
    zn = zn < 1 ? 1 : (zn > REFINE_RZ ? REFINE_RZ : zn);
    if (rescue && tid == 0 && z == 0 && b % (QT / QB) == 0) {  // the tile's first block lists it for the rescue launch
        unsigned *rs = bcnt + 2 * (N_pad / QB);
        rs[1 + atomicAdd(&rs[0], 1u)] = (unsigned)(b / (QT / QB));
    }
    if (z > 0 && (rescue || z >= zn)) return;  // (a rescued tile's candidates are moot; its image is written by z == 0)
    if (cnt == 0 && !rescue) return;
    __shared__ int dense_n;
    __shared__ int dense_at[REFINE_DENSE_CAP];
    if (tid == 0) dense_n = 0;
    for (int idx = tid; idx < QB * C; idx += 256) {
        long n = b * QB + (idx & (QB - 1));
        n = n < N ? n : N - 1;  // (padding queries have no candidates)
        qs[idx] = emb_load(q + n * q_sn, (long)(idx / QB) * q_sc);
    }
    __syncthreads();
    if (rescue) {  // (block-uniform; z == 0) the block's image as pack_rows_kernel<32,32> writes it for MANET_COMPUTE_F32
        char *out0 = q32 + b * qblk_bytes32;
        for (int item = tid; item < units32 * QB; item += 256) {
            const int r = item & (QB - 1), u = item / QB;
            const int k0 = 8 * (u >> 1) + (u & 1);  // image_unit_f32: k0, k0 + 2, k0 + 4, k0 + 6
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (k0 + 2 * e < C) ? qs[(k0 + 2 * e) * QB + r] : 0.0f;
            *(f32x4 *)(out0 + ((long)u * QB + r) * 16) = v;
        }
        if (tid < QB) {
            float nrm = 0.0f;
            for (int k = 0; k < C; ++k) nrm = fmaf(qs[k * QB + tid], qs[k * QB + tid], nrm);
            *(float *)(out0 + (long)units32 * QB * 16 + tid * 4) = nrm;
        }
        return;  // (the rescue pass evaluates every pair of this tile: its candidates are moot)
    }
    for (int i = z + zn * tid; i < cnt; i += zn * 256) {
        const uint2 e = list[b * bucket_cap + i];
        if (e.y & REFINE_DENSE_BIT) {  // a dense block: the whole workgroup evaluates it below
            if (!rescue) {             // (a tile that is rescued anyway gets every distance from the fp32 kernel)
                const int at = atomicAdd(&dense_n, 1);
                if (at < REFINE_DENSE_CAP) dense_at[at] = i;  // (more than the cap: the filter pass marked the bucket incomplete)
            }
            continue;
        }
        const float *x = qs + (int)((e.x % (unsigned long)N_pad) & (QB - 1));
        const float *kr = rows + (long)e.y * C;
        float xs = 0.0f, mm = 0.0f;
        int k = 0;
        for (; (C & 3) == 0 && k + 32 <= C; k += 32) {
            f32x4 y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = *(const f32x4 *)(kr + k + 4 * j);  // (rows are 16-byte aligned: C % 4 == 0)
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const float xv = x[(k + j) * QB];
                xs = fmaf(xv, xv, xs);
                mm = fmaf(xv, y[j >> 2][j & 3], mm);
            }
        }
        for (; k < C; ++k) {
            const float xv = x[k * QB];
            xs = fmaf(xv, xv, xs);
            mm = fmaf(xv, kr[k], mm);
        }
        atomicMin(keys2 + e.x, key_of(fmaf(-2.0f, mm, xs + norms[e.y])));  // IntVOS.py:39
    }
    __syncthreads();
    // dense entries: 32 bank rows x this block's 32 queries each -- exactly one 32 x 32 tile of the fp32 matrix pipe: a WAVE
    // per entry, A = the 32 bank rows (lane = row, read from the fp32 copy of the bank), B = the block's queries from LDS,
    // ceil(C / 2) v_mfma_f32_32x32x2_f32 in k order -- the fp32 kernel's own chain for these pairs, hence its bits.  (First
    // form: VALU, a thread per (query, 4 rows): 1.4 us per entry per workgroup, a quarter of the CU's rate.)
    const int nd = dense_n < REFINE_DENSE_CAP ? dense_n : REFINE_DENSE_CAP;
    if (nd > 0) {
        const int lane = tid & 63, w = tid >> 6, l31 = lane & 31, hh = lane >> 5;
        const float *x = qs + l31;
        float xs = 0.0f;
        for (int k = 0; k < C; ++k) xs = fmaf(x[k * QB], x[k * QB], xs);
        for (int d = w; d < nd; d += 4) {
            const uint2 e = list[b * bucket_cap + dense_at[d]];
            const long slot0 = (long)(e.y & ~REFINE_DENSE_BIT);
            const float *kr = rows + (slot0 + l31) * C;
            f32x16 acc = {0};
            if ((C & 3) == 0) {
                // batches of five 16-byte loads = ten k-steps, two batches in flight: the loads of batch i + 1 are issued before
                // the MFMAs of batch i (a lone wave has nothing else to hide a row load behind: the first form -- load, wait,
                // ten MFMAs, five times per entry -- spent most of an entry waiting)
                f32x4 ya[5], yb[5];
                auto load5 = [&](f32x4 (&y)[5], int k0) __attribute__((always_inline)) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) y[j] = (k0 + 4 * j < C) ? *(const f32x4 *)(kr + k0 + 4 * j) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                };
                auto mfma5 = [&](const f32x4 (&y)[5], int k0) __attribute__((always_inline)) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        if (k0 + 4 * j < C) {  // (wave-uniform)
                            const int k = k0 + 4 * j + hh;  // this half's k of the step: even lanes' half 2s, the other 2s + 1
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(hh ? y[j][1] : y[j][0], x[k * QB], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(hh ? y[j][3] : y[j][2], x[(k + 2) * QB], acc, 0, 0, 0);
                        }
                    }
                };
                load5(ya, 0);
                for (int k0 = 0; k0 < C; k0 += 40) {
                    if (k0 + 20 < C) load5(yb, k0 + 20);
                    mfma5(ya, k0);
                    if (k0 + 40 < C) load5(ya, k0 + 40);
                    if (k0 + 20 < C) mfma5(yb, k0 + 20);
                }
            } else {
                for (int k0 = 0; k0 < C; k0 += 2) {
                    const int k = k0 + hh;
                    const bool ok = k < C;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? kr[k] : 0.0f, ok ? x[k * QB] : 0.0f, acc, 0, 0, 0);
                }
            }
            // C/D layout: column = lane & 31 (query), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (bank row of the pass)
            unsigned best = 0xffffffffu;
#pragma unroll
            for (int tq = 0; tq < 4; ++tq) {
                const f32x4 nv = *(const f32x4 *)(norms + slot0 + 8 * tq + 4 * hh);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned kd = key_of(fmaf(-2.0f, acc[4 * tq + i], xs + nv[i]));  // IntVOS.py:39
                    best = kd < best ? kd : best;
                }
            }
            const unsigned other = (unsigned)__shfl_xor((int)best, 32);
            best = other < best ? other : best;
            if (hh == 0) atomicMin(keys2 + e.x + l31, best);  // (e.x = the pair of the block's first query)
        }
    }
}

}  // namespace

// MANET_COMPUTE_BF16_REFINE on a prepared bank (see the header comment).  `qimg` = the query's bf16 operand
// image (made by the caller of this function), `qraw` = the same query as stored (fp32 / bf16, element strides).
int run_refine(int compute, const char *qimg, const void *qraw, int q_dtype, long q_sn, long q_sc, const char *bws,
               const BankLayout &BL, char *mws, const MatchLayout &ML, long N, int64_t M0, int C, int n_ids, float *out, float *mem,
               int flags, hipStream_t st)
{
    const int *meta = (const int *)(bws + BL.off_meta), *sub_meta = (const int *)(bws + BL.off_sub_meta);
    unsigned *keys = (unsigned *)(mws + ML.off_keys), *keys2 = (unsigned *)(mws + ML.off_keys2);
    unsigned *thr = (unsigned *)(mws + ML.off_thr);
    float *slack = (float *)(mws + ML.off_slack);
    uint2 *list = (uint2 *)(mws + ML.off_list);
    unsigned long long *stats = (unsigned long long *)(mws + ML.off_stats);
    unsigned *bcnt = (unsigned *)(mws + ML.off_bcnt);
    const bool force_exact = (flags & MANET_EPI_REFINE_EXACT) != 0;
    flags &= ~MANET_EPI_REFINE_EXACT;
    const long pairs = (long)n_ids * ML.N_pad;
    const MatchTune tune = match_tune();
    auto plan = [&](int form) { return match_plan(N, M0, C, n_ids, 1, compute, form, tune); };
    MatchArgs A = {qimg, bws + BL.off_sub_pack, sub_meta, n_ids, ML.N_pad, keys, nullptr, thr, slack, stats, list, ML.bucket_cap, bcnt};
    if (force_exact) {
        hipLaunchKernelGGL(refine_force_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, ML.N_pad, n_ids, keys2, stats,
                           bcnt);
    } else {
        // 1. pre-pass over the sub-sampled bank -> keys = U
        launch_match(plan(MATCH_FORM_REFINE_PRE), A, st);
        // 2. thresholds; exact keys and counters reset
        if (compute == MANET_COMPUTE_F16_REFINE)
            hipLaunchKernelGGL(refine_threshold_f16_kernel, dim3((unsigned)(ML.N_pad / 256)), dim3(256), 0, st, (const unsigned *)keys,
                               qimg, (long)ML.qblk_bytes, ML.G.units, C, meta, N, ML.N_pad, n_ids, thr, slack, keys2, stats, bcnt);
        else
            hipLaunchKernelGGL(refine_threshold_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, (const unsigned *)keys,
                               qimg, (long)ML.qblk_bytes, C, meta, N, ML.N_pad, n_ids, thr, slack, keys2, stats, bcnt);
        // 3. filter pass over the whole bank -> candidate list
        A.bpack = bws + BL.off_pack;
        A.meta = meta;
        launch_match(plan(MATCH_FORM_REFINE_FILTER), A, st);
    }
    // 4. exact re-rank of the candidates
    const float *rows = (const float *)(bws + BL.off_rows), *norms = (const float *)(bws + BL.off_norms);
    const dim3 rgrid((unsigned)(ML.N_pad / QB), REFINE_RZ);
    const size_t rlds = (size_t)QB * C * sizeof(float);
    const Geom G32 = BL.G32;
    char *q32 = mws + ML.off_q32;
    if (q_dtype == MANET_EMB_F32)
        hipLaunchKernelGGL(refine_rerank_kernel<float>, rgrid, dim3(256), rlds, st, (const float *)qraw, q_sn, q_sc, rows, norms,
                           (const uint2 *)list, bcnt, ML.bucket_cap, N, ML.N_pad, C, keys2, stats, q32, G32.units,
                           (long)G32.qblk_bytes);
    else
        hipLaunchKernelGGL(refine_rerank_kernel<unsigned short>, rgrid, dim3(256), rlds, st, (const unsigned short *)qraw, q_sn, q_sc,
                           rows, norms, (const uint2 *)list, bcnt, ML.bucket_cap, N, ML.N_pad, C, keys2, stats, q32,
                           G32.units, (long)G32.qblk_bytes);
    // 5. rescue: the 256-query tiles that hold a 32-query block whose bucket is incomplete (a block's hits were not listed,
    //    or the bucket overflowed) go through the exact fp32 kernel against the whole bank -- their fp32 operand image was
    //    written by the re-rank launch above; the minima meet the re-rank's by atomicMin on keys2
    A.qpack = q32;
    A.bpack = bws + BL.off_pack32;
    A.meta = meta;
    A.keys = keys2;
    if (force_exact) manet_profile_record(st, true, 0);
    launch_match(plan(force_exact ? MATCH_FORM_REFINE_RESCUE_EXACT : MATCH_FORM_REFINE_RESCUE), A, st);
    if (force_exact) manet_profile_record(st, false, 0);
    launch_global_finish(keys2, N, ML.N_pad, n_ids, flags & ~MANET_EPI_KEYS_ARMED, out, mem, N * n_ids, st);
    return manet_check_launch("manet_global_match (filter + fp32 re-rank)");
}

// what both statistics readers share: checks, the layout, and blocking copies of the last filter pass's two counters
// {candidates appended, list overflowed} and -- bcnt != nullptr -- of the N_pad / 32 bucket counts (malloc'ed: the caller frees)
static int read_refine_stats(const void *match_ws, int64_t N, int C, int n_ids, MatchLayout &ML, int64_t (&h)[2], unsigned **bcnt)
{
    if (!match_ws) return manet_set_error(MANET_E_INVALID, "null pointer");
    int rc = check_common(N, 0, C, n_ids, 1, MANET_COMPUTE_BF16_REFINE);
    if (rc) return rc;
    ML = match_layout(N, C, n_ids, MANET_COMPUTE_BF16_REFINE, 1);
    const size_t nb = (size_t)(ML.N_pad / QB) * sizeof(unsigned);
    if (bcnt && !(*bcnt = (unsigned *)malloc(nb))) return manet_set_error(MANET_E_INVALID, "out of host memory");
    unsigned long long u[2] = {0, 0};
    if (hipMemcpy(u, (const char *)match_ws + ML.off_stats, sizeof(u), hipMemcpyDeviceToHost) != hipSuccess ||
        (bcnt && hipMemcpy(*bcnt, (const char *)match_ws + ML.off_bcnt, nb, hipMemcpyDeviceToHost) != hipSuccess)) {
        if (bcnt) free(*bcnt);
        return manet_set_error(MANET_E_LAUNCH, "reading the statistics failed");
    }
    h[0] = (int64_t)u[0];
    h[1] = (int64_t)u[1];
    return MANET_OK;
}

extern "C" {

int manet_global_match_refine(const void *query, int emb_dtype, int64_t q_stride_n, int64_t q_stride_c,
                              const void *query_image, const void *bank_ws, int64_t N, int64_t M0, int C, int n_ids,
                              float *out, float *mem_inout, int epilogue_flags, void *match_ws, size_t match_ws_bytes,
                              manet_stream_t stream)
{
    const int compute = (epilogue_flags & MANET_EPI_REFINE_F16) ? MANET_COMPUTE_F16_REFINE : MANET_COMPUTE_BF16_REFINE;
    epilogue_flags &= ~MANET_EPI_REFINE_F16;
    int rc = check_common(N, M0, C, n_ids, 1, compute);
    if (rc) return rc;
    if (!query || !bank_ws || !out || !match_ws) return manet_set_error(MANET_E_INVALID, "null pointer");
    if (emb_dtype != MANET_EMB_F32 && emb_dtype != MANET_EMB_BF16)
        return manet_set_error(MANET_E_INVALID, "embedding dtype %d (MANET_EMB_F32 / MANET_EMB_BF16)", emb_dtype);
    if (!query_image)  // no image at hand: the general entry point packs one
        return manet_global_match_prepared_ex(query, emb_dtype, q_stride_n, q_stride_c, bank_ws, N, M0, C, n_ids, 1, compute, out,
                                              mem_inout, epilogue_flags, match_ws, match_ws_bytes, stream);
    BankLayout BL = bank_layout(M0, C, n_ids, compute);
    MatchLayout ML = match_layout(N, C, n_ids, compute, 1);
    if (match_ws_bytes < ML.total)
        return manet_set_error(MANET_E_WORKSPACE, "match workspace %zu < %zu bytes", match_ws_bytes, ML.total);
    hipStream_t st = (hipStream_t)stream;
    fill32((char *)match_ws + ML.off_keys, 0xffffffffu, (size_t)n_ids * ML.N_pad, st);
    return run_refine(compute, (const char *)query_image, query, emb_dtype, (long)q_stride_n, (long)q_stride_c, (const char *)bank_ws, BL,
                      (char *)match_ws, ML, (long)N, M0, C, n_ids, out, mem_inout, epilogue_flags & ~MANET_EPI_KEYS_ARMED, st);
}

int manet_global_match_refine_stats(const void *match_ws, int64_t N, int C, int n_ids, int64_t *candidates,
                                    int64_t *list_overflowed)
{
    MatchLayout ML;
    int64_t h[2];
    int rc = read_refine_stats(match_ws, N, C, n_ids, ML, h, nullptr);
    if (rc) return rc;
    if (candidates) *candidates = h[0];
    if (list_overflowed) *list_overflowed = h[1];
    return MANET_OK;
}

int manet_global_match_refine_rescued_async(const void *match_ws, int64_t N, int C, int n_ids, int32_t *out2_device,
                                            manet_stream_t stream)
{
    if (!match_ws || !out2_device) return manet_set_error(MANET_E_INVALID, "null pointer");
    int rc = check_common(N, 0, C, n_ids, 1, MANET_COMPUTE_BF16_REFINE);
    if (rc) return rc;
    MatchLayout ML = match_layout(N, C, n_ids, MANET_COMPUTE_BF16_REFINE, 1);
    hipLaunchKernelGGL(refine_rescued_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned *)((const char *)match_ws + ML.off_bcnt), (long)(ML.N_pad / QT), (long)ML.bucket_cap, out2_device);
    return manet_check_launch("manet_global_match_refine_rescued_async");
}

int manet_global_match_refine_stats2(const void *match_ws, int64_t N, int C, int n_ids, int64_t *stats4)
{
    if (!stats4) return manet_set_error(MANET_E_INVALID, "null pointer");
    MatchLayout ML;
    int64_t h[2];
    unsigned *bc = nullptr;
    int rc = read_refine_stats(match_ws, N, C, n_ids, ML, h, &bc);
    if (rc) return rc;
    // a 256-query tile goes through the rescue pass (the exact fp32 kernel) iff one of its eight 32-query blocks has an
    // incomplete bucket -- the same test global_match_f32_pipe_kernel<KS, RESCUE> makes
    long rescued = 0;
    const long tiles = ML.N_pad / QT;
    for (long t = 0; t < tiles; ++t) {
        bool need = false;
        for (int i = 0; i < QT / QB; ++i) {
            const unsigned raw = bc[t * (QT / QB) + i];
            need = need || (raw >> 31) || (long)raw > ML.bucket_cap;
        }
        rescued += need ? 1 : 0;
    }
    free(bc);
    stats4[0] = (int64_t)h[0];
    stats4[1] = (int64_t)h[1];
    stats4[2] = (int64_t)rescued;
    stats4[3] = (int64_t)tiles;
    return MANET_OK;
}

}  // extern "C"
