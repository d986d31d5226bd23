// Global nearest-neighbour matching for MI355X (gfx950): the match itself.
//
// Replaces networks/IntVOS.py:160-210 (nearest_neighbor_features_per_object) and its helpers
// (:23-40 pairwise distances, :62-97 masked min, :100-109 pixel selection, :113-157 chunk loop)
// plus, as a fused epilogue, :611-612 (normalise) and :615-622 (min-aggregation with the stored
// per-frame global map).
//
// Design (see DESIGN.md for the numbers):
//   * The N x M distance matrix is never materialised.  d(n,m) = (|q_n|^2 + |k_m|^2) - 2 q_n.k_m
//     is produced tile by tile on the matrix cores and reduced to a running minimum in registers.
//   * The contraction runs on v_mfma_f32_32x32x2_f32 with the operands SWAPPED (A = bank rows,
//     B = query pixels): an accumulator register then holds one query column and 16 bank rows, so
//     the reduction over the bank is lane-local (one v_min per element) and only the two 32-lane
//     halves have to be combined at the end (one cross-lane shuffle per object).
//   * the operands come packed from csrc/global_prepare.hip: bank rows sorted by object id, so every 64-row bank tile
//     belongs to one object, in the exact LDS image the MFMA loop wants (Geom, csrc/global_match_common.h); a tile is
//     staged one tile-step ahead, double buffered, one barrier per tile.
//   * arithmetic modes: fp32 MFMA (exact), bf16 MFMA on rounded embeddings, fp16 MFMA on rounded embeddings (the bf16
//     kernels' body on v_mfma_f32_32x32x16_f16: 11 significand bits instead of 8 at the same cost), and split-bf16
//     (hi+lo, three MFMAs: fp32-class accuracy); top-k (k_nn 2..8) as a variant of the fp32 kernel.  A fourth, the bf16
//     filter + exact fp32 re-rank (csrc/global_refine.hip), borrows the wide bf16 kernel and the pipelined fp32 kernel.
//   * the 64 queries x C operand of a wave lives in registers for the whole kernel.
//   * grid = (256-query tiles) x (S bank splits), split index tied to blockIdx % 8 so that the
//     workgroups of one XCD stream the same bank range through that XCD's L2.  Splits combine by
//     atomicMin on order-preserving integer keys; a last tiny kernel decodes, normalises and
//     min-merges with the stored map.  How a launch is cut is decided in one place: match_plan (the common header).
//
// Numerics of the fp32 path: the MFMA is a k-ascending fmaf chain from 0, d = fmaf(-2, mm, xs+ys);
// min is exact -- so the result is bit-identical to oracle/manet_oracle.c.
#include "global_match_common.h"

namespace {

// block -> (query tile, bank split, tile range [t0, t1)); false = nothing to do.
// Big banks: S splits chosen on the host (pick_splits), split index tied to the XCD (block b runs on XCD b % 8 --
// observed, used for speed only): the blocks of one XCD that are resident together stream the same bank range
// through that XCD's L2.
// Small banks (T < S tiles: a scribble-sized memory, the reference's normal case, test.py:170-176): the host cannot know
// T without a sync (it only knows the upper bound M0 / 64), and S splits of at most one tile each would make every
// workgroup load its 256-query operand for a single tile.  The kernel re-decides: S' = clamp(small_S, 1, T) splits with
// small_S = resident workgroup slots / query tiles -- one full round of workgroups, whole tiles each -- and a flat
// block -> (tile, split) map (such a bank fits every XCD's L2 anyway).  The minimum is order-independent: same bits.
// `block_map`: bits 0-7 = tuning (0: XCD-aware, 1: tile fastest, 2: split fastest, 4..7: XCD-aware with 2..5 splits
// fastest), bits 8.. = small_S.
__device__ __forceinline__ bool split_of_block(int b, int nQT, int S, int T, int block_map, int &qt, int &s, int &t0,
                                               int &t1)
{
    const int bm = block_map & 0xff, small_S = (block_map >> 8) & BLOCK_MAP_SMALL_S_MASK;
    bool one_round = T < S && small_S > 0;
    if (!one_round && (block_map & ONE_ROUND_OK) && small_S > 0 && small_S < S) {
        // r5.  The host sizes S from the bank's UPPER-bound tile count (it cannot know how many rows are labelled without a
        // sync) for many rounds of short splits; a workgroup's fixed cost (query operand, pipeline fill, closing atomics) is
        // worth ~0.6 tile-times after the overlap of two workgroups per CU.  With the REAL tile count: cost of the host's
        // choice = its rounds over the 512 slots (a last round at most half full counts half, as in pick_splits) x (tiles per
        // split + 0.6) against ONE round of small_S = floor(512 / query tiles) long splits.  The reference driver's first-round
        // bank (rough_ROI: ~17 000 rows = 268 tiles at 480p) ran 48 splits of 5.6 tiles: 673 us; one round of 5 x 54: 633.
        // Banks above ~600 tiles keep the host's choice (a tie there, and the XCD-aware map).  Same bits either way.
        const float rounds = (float)nQT * (float)S / 512.0f;
        const float whole = floorf(rounds), frac = rounds - whole;
        const float last = frac <= 0.0f ? 0.0f : (frac <= 0.5f ? 0.5f : 1.0f);
        const float cost_host = (whole + last) * ((float)T / (float)S + 0.6f);
        const float cost_one = ceilf((float)T / (float)small_S) + 0.6f;
        one_round = cost_one < 0.97f * cost_host;
    }
    if (one_round) {
        const int S2 = small_S < T ? small_S : T;
        qt = b % nQT;
        s = b / nQT;
        if (s >= S2) return false;
        t0 = (int)((long)s * T / S2);
        t1 = (int)((long)(s + 1) * T / S2);
        return t0 < t1;
    }
    if (bm == 0 || bm == 3) {
        const int xcd = b & 7;
        const int idx = b >> 3;
        qt = idx % nQT;
        s = xcd + 8 * (idx / nQT);
        // bm == 3 (the FILTER pass of MANET_COMPUTE_BF16_REFINE; S is a multiple of 8): XCD x walks the CONTIGUOUS splits
        // x S/8 .. (x+1) S/8 - 1 one after the other instead of x, x + 8, ...: at any time the eight resident splits are
        // spread over the whole bank, i.e. over all objects, so most of an object's splits start after earlier ones of the
        // same object have published their tightened thresholds
        if (bm == 3 && (S & 7) == 0) s = xcd * (S >> 3) + idx / nQT;
    } else if (bm >= 4 && bm <= 7 && (S & 7) == 0) {
        // XCD-aware with PB splits fastest: the workgroups of an XCD that are resident together cover 64 / PB query tiles x
        // PB of the XCD's splits -- a query operand is loaded by PB workgroups at about the same time (one L2 miss, PB - 1
        // hits) at the price of PB splits streaming through the L2 side by side
        const int PB = bm - 2, S8 = S >> 3;
        const int xcd = b & 7, idx = b >> 3;
        const int g = idx / (nQT * PB), r = idx - g * (nQT * PB);
        const int pbg = (S8 - g * PB) < PB ? (S8 - g * PB) : PB;
        if (pbg <= 0) return false;
        qt = r / pbg;
        s = xcd + 8 * (g * PB + (r - qt * pbg));
        if (qt >= nQT) return false;
    } else if (bm == 1) {
        qt = b % nQT;
        s = b / nQT;
    } else {
        s = b % S;
        qt = b / S;
    }
    t0 = (int)((long)s * T / S);
    t1 = (int)((long)(s + 1) * T / S);
    return t0 < t1;
}

// bm == 3's map with a TAPERED tail (the FILTER pass only): each XCD's LAST split is cut into FILTER_TAIL_CUTS pieces.  The
// listing behind the filter's tests is a few per cent of all wave cycles but sits in a few workgroups -- on video-like data a
// (query tile, split) that holds the tile's image region of a bank frame lists thousands of rows and runs twice as long as its
// neighbours (measured: listing 3.9 % of the wave cycles, up to 45 % of one wave's) -- and whatever such a workgroup adds in
// the launch's LAST round is the launch's tail: shorter last workgroups, a shorter tail.
__device__ __forceinline__ bool tapered_split_of_block(int b, int nQT, int S, int T, int &qt, int &s, int &t0, int &t1)
{
    const int xcd = b & 7, idx = b >> 3, S8 = S >> 3;
    const int full = nQT * (S8 - 1);
    int cut = 0, cuts = 1;
    if (idx < full) {
        qt = idx % nQT;
        s = xcd * S8 + idx / nQT;
    } else {
        const int r = idx - full;
        cut = r / nQT;
        cuts = FILTER_TAIL_CUTS;
        if (cut >= FILTER_TAIL_CUTS) return false;
        qt = r - cut * nQT;
        s = xcd * S8 + S8 - 1;
    }
    const int a = (int)((long)s * T / S), e = (int)((long)(s + 1) * T / S);
    t0 = a + (int)((long)cut * (e - a) / cuts);
    t1 = a + (int)((long)(cut + 1) * (e - a) / cuts);
    return t0 < t1;
}


// ---------------------------------------------------------------------------------------------
// main kernel, fp32: one workgroup = 256 queries x one bank split
// sorted insert of d into the ascending list m[0..K-1] (drops the largest)
template <int K>
__device__ __forceinline__ void topk_insert(float (&m)[K], float d)
{
#pragma unroll
    for (int j = 0; j < K; ++j) {
        float lo = fminf(m[j], d);
        d = fmaxf(m[j], d);
        m[j] = lo;
    }
}

// KNN = 1: masked minimum (IntVOS.py:84-85), splits meet through atomicMin on `keys`.
// KNN = 8: the MANET_MAX_KNN smallest distances per (query, object) for the top-k path
//          (IntVOS.py:87-94); every split writes its sorted list to `topk` [S][n_ids][N_pad][8].
// ARG (with KNN = 1): also track WHICH bank row attains the minimum (training: the gradient of torch.min flows to
//          that row only, IntVOS.py:84); splits meet through a 64-bit atomicMin on (distance key << 32 | bank slot)
//          in `keys64` -- equal distances resolve to the smallest slot, i.e. the first row in the sorted bank.
// (KS = 64 -- C in 105..128 -- with the top-k lists or the arg-min slots does not fit 256 VGPRs: those two forms take one
// workgroup per CU instead of spilling)
// NTH (with ARG, r5 -- the training path of k_nearest_neighbors > 1, IntVOS.py:87-94): the minimum is taken over the (distance
//          key, bank slot) pairs STRICTLY ABOVE a per-(object, query) bound -- `keys` then points at the previous pass's 64-bit
//          pairs -- so pass j of k yields the j-th nearest row and its slot, exactly, ties ordered by slot.
template <int KS, int KNN, bool ARG = false, bool NTH = false>
__global__ __launch_bounds__(256, ((KS == 64 && (KNN > 1 || ARG)) || NTH) ? 1 : 2) void global_match_f32_kernel(const char *__restrict__ qpack,
                                                                  const char *__restrict__ bpack,
                                                                  const int *__restrict__ meta,
                                                                  int n_ids, int nQT, int S,
                                                                  long N_pad,
                                                                  unsigned *__restrict__ keys,
                                                                  float *__restrict__ topk, int block_map)
{
    static_assert(!ARG || KNN == 1, "arg-min tracking is the k = 1 path");
    static_assert(!NTH || ARG, "the bounded form is a variant of the arg-min form");
    unsigned long long *keys64 = (unsigned long long *)topk;  // ARG: the top-k region holds the 64-bit pairs
    const unsigned long long *bound64 = (const unsigned long long *)keys;  // NTH: the previous pass's pairs
    constexpr int NG = (KS + 3) / 4;
    constexpr size_t TILE_BYTES = bank_tile_bytes(NG);
    constexpr size_t QBLK_BYTES = query_block_bytes(NG);
    extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 x TILE_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int h = lane >> 5;

    // XCD-aware mapping: block b runs on XCD b % 8 (observed, used for speed only).  All blocks
    // of one XCD that are resident together share a bank split -> the split streams through L2.
    int qt, s, t0, t1;
    const int T = meta[META_T];
    if (!split_of_block(blockIdx.x, nQT, S, T, block_map, qt, s, t0, t1)) return;

    // Tile staging through registers (issue the global loads a whole tile-step early, write them to
    // LDS after the next barrier).  global_load_lds would save the VGPR round trip, but hipcc cannot
    // tell the DMA's LDS destination from the ds_reads of the other buffer and drains vmcnt(0) in
    // front of the first ds_read of every tile, which serialises the prefetch.
    constexpr int NV = (int)(TILE_BYTES / 16);    // 16-byte vectors per tile
    constexpr int NLD = (NV + 255) / 256;         // per thread
    u32x4 R[NLD];
#define MANET_GLOAD(R_, t_)                                                                \
    {                                                                                      \
        const u32x4 *g_ = (const u32x4 *)(bpack + (size_t)(t_) * TILE_BYTES);              \
        _Pragma("unroll") for (int i_ = 0; i_ < NLD; ++i_)                                 \
        {                                                                                  \
            const int idx_ = i_ * NTHR + tid;                                              \
            R_[i_] = g_[idx_ < NV ? idx_ : NV - 1]; /* clamped: always a valid address */  \
        }                                                                                  \
    }
#define MANET_LSTORE(R_, slot_)                                                            \
    {                                                                                      \
        u32x4 *l_ = (u32x4 *)(smem + (size_t)(slot_) * TILE_BYTES);                        \
        _Pragma("unroll") for (int i_ = 0; i_ < NLD; ++i_)                                 \
            if (i_ * NTHR + tid < NV) l_[i_ * NTHR + tid] = R_[i_];                        \
    }
    constexpr int NTHR = 256;
    MANET_GLOAD(R, t0);

    // this wave's 2 x 32 queries, resident in registers for the whole kernel (B operand:
    // lane holds q[j = lane&31][k = 8g + 2jj + (lane>>5)])
    f32x4 q0[NG], q1[NG];
    float xs0, xs1;
    {
        const char *qb0 = qpack + (size_t)(qt * (QT / QB) + wave * 2) * QBLK_BYTES;
        const char *qb1 = qb0 + QBLK_BYTES;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            q0[g] = *(const f32x4 *)(qb0 + ((size_t)(g * 2 + h) * QB + l31) * 16);
            q1[g] = *(const f32x4 *)(qb1 + ((size_t)(g * 2 + h) * QB + l31) * 16);
        }
        xs0 = *(const float *)(qb0 + (size_t)NG * 2 * QB * 16 + l31 * 4);
        xs1 = *(const float *)(qb1 + (size_t)NG * 2 * QB * 16 + l31 * 4);
    }
    const long qbase = (long)qt * QT + wave * 64 + l31;

    int o = 0;
    while (meta[META_SEG + o + 1] <= t0) ++o;  // object owning tile t0
    int seg_end = meta[META_SEG + o + 1];
    float m0[KNN], m1[KNN];
    int a0 = -1, a1 = -1;  // ARG: bank slot (without the lane's +4h) of the running minimum, -1 = none yet
    unsigned long long B0 = ~0ull, B1 = ~0ull, lo0 = 0, lo1 = 0;  // NTH: running minimum pairs, and the bounds they must exceed
    auto reset = [&]() {
#pragma unroll
        for (int j = 0; j < KNN; ++j) m0[j] = m1[j] = (KNN == 1) ? MANET_WRONG_LABEL_PADDING_DISTANCE : INFINITY;
        a0 = a1 = -1;
        B0 = B1 = ~0ull;
    };
    auto load_bounds = [&](int obj) {
        if (NTH) {
            lo0 = bound64[(size_t)obj * N_pad + qbase];
            lo1 = bound64[(size_t)obj * N_pad + qbase + 32];
        }
    };
    reset();
    load_bounds(o);

    auto flush = [&](int obj) {
        if (ARG) {
            unsigned long long k0 = ((unsigned long long)key_of(m0[0]) << 32) | (unsigned)(a0 < 0 ? -1 : a0 + 4 * h);
            unsigned long long k1 = ((unsigned long long)key_of(m1[0]) << 32) | (unsigned)(a1 < 0 ? -1 : a1 + 4 * h);
            if (NTH) {
                k0 = B0;
                k1 = B1;
            }
            const unsigned long long o0 = __shfl_xor(k0, 32), o1 = __shfl_xor(k1, 32);
            k0 = k0 < o0 ? k0 : o0;
            k1 = k1 < o1 ? k1 : o1;
            if (h == 0) {
                atomicMin(keys64 + (size_t)obj * N_pad + qbase, k0);
                atomicMin(keys64 + (size_t)obj * N_pad + qbase + 32, k1);
            }
        } else if (KNN == 1) {
            float a = min3p(m0[0], m0[0], __shfl_xor(m0[0], 32));
            float c = min3p(m1[0], m1[0], __shfl_xor(m1[0], 32));
            if (h == 0) {
                atomicMin(keys + (size_t)obj * N_pad + qbase, key_of(a));
                atomicMin(keys + (size_t)obj * N_pad + qbase + 32, key_of(c));
            }
        } else {
            // merge the other half-wave's list into ours, then the lower half writes the split's list
            float o0[KNN], o1[KNN];
#pragma unroll
            for (int j = 0; j < KNN; ++j) {
                o0[j] = __shfl_xor(m0[j], 32);
                o1[j] = __shfl_xor(m1[j], 32);
            }
#pragma unroll
            for (int j = 0; j < KNN; ++j) {
                topk_insert<KNN>(m0, o0[j]);
                topk_insert<KNN>(m1, o1[j]);
            }
            if (h == 0) {
                float *p0 = topk + (((size_t)s * n_ids + obj) * N_pad + qbase) * KNN;
                float *p1 = p0 + (size_t)32 * KNN;
#pragma unroll
                for (int j = 0; j < KNN; ++j) {
                    p0[j] = m0[j];
                    p1[j] = m1[j];
                }
            }
        }
    };

    MANET_LSTORE(R, 0);
    if (t0 + 1 < t1) MANET_GLOAD(R, t0 + 1);
    for (int t = t0; t < t1; ++t) {
        const int buf = (t - t0) & 1;
        __syncthreads();  // tile t is visible in buffer buf; buffer buf^1 (tile t-1) is free
        if (t + 1 < t1) {
            MANET_LSTORE(R, buf ^ 1);                 // tile t+1, loaded during the previous step
            if (t + 2 < t1) MANET_GLOAD(R, t + 2);    // in flight during this step's MFMAs
        }
        if (t >= seg_end) {  // wave-uniform: crossed into the next object's rows
            flush(o);
            reset();
            do { ++o; seg_end = meta[META_SEG + o + 1]; } while (t >= seg_end);
            load_bounds(o);
        }
        const char *tb = smem + (size_t)buf * TILE_BYTES;
        const f32x4 *A = (const f32x4 *)tb;
        f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            f32x4 a0 = A[(g * 2 + h) * BT + l31];
            f32x4 a1 = A[(g * 2 + h) * BT + 32 + l31];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (g * 4 + j < KS) {  // compile-time: k-steps beyond C are all-zero, skip them
                    c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], q0[g][j], c00, 0, 0, 0);
                    c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], q1[g][j], c01, 0, 0, 0);
                    c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], q0[g][j], c10, 0, 0, 0);
                    c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], q1[g][j], c11, 0, 0, 0);
                }
            }
        }
        // epilogue: register r of block rb holds bank row rb*32 + (r&3) + 8*(r>>2) + 4*h
        const float *ysl = (const float *)(tb + (size_t)NG * 2 * BT * 16);
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) {
            f32x4 y0 = *(const f32x4 *)(ysl + 8 * tq + 4 * h);
            f32x4 y1 = *(const f32x4 *)(ysl + 32 + 8 * tq + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 4 * tq + i;
                const float d00 = fmaf(-2.0f, c00[r], xs0 + y0[i]);  // IntVOS.py:39
                const float d01 = fmaf(-2.0f, c01[r], xs1 + y0[i]);
                const float d10 = fmaf(-2.0f, c10[r], xs0 + y1[i]);
                const float d11 = fmaf(-2.0f, c11[r], xs1 + y1[i]);
                if (NTH) {  // the smallest (distance key, slot) pair above the bound; a NaN (key 0) never qualifies
                    const unsigned slot = (unsigned)(t * BT + (r & 3) + 8 * (r >> 2) + 4 * h);
                    const unsigned long long k00 = ((unsigned long long)key_of(d00) << 32) | slot;
                    const unsigned long long k10 = ((unsigned long long)key_of(d10) << 32) | (slot + 32u);
                    const unsigned long long k01 = ((unsigned long long)key_of(d01) << 32) | slot;
                    const unsigned long long k11 = ((unsigned long long)key_of(d11) << 32) | (slot + 32u);
                    if (k00 > lo0 && k00 < B0) B0 = k00;
                    if (k10 > lo0 && k10 < B0) B0 = k10;
                    if (k01 > lo1 && k01 < B1) B1 = k01;
                    if (k11 > lo1 && k11 < B1) B1 = k11;
                } else if (ARG) {  // strict <: the first row in bank order wins a tie; a NaN never wins
                    const int slot = t * BT + (r & 3) + 8 * (r >> 2);
                    if (d00 < m0[0]) { m0[0] = d00; a0 = slot; }
                    if (d10 < m0[0]) { m0[0] = d10; a0 = slot + 32; }
                    if (d01 < m1[0]) { m1[0] = d01; a1 = slot; }
                    if (d11 < m1[0]) { m1[0] = d11; a1 = slot + 32; }
                } else if (KNN == 1) {  // NaN-propagating, like torch.min (IntVOS.py:84)
                    m0[0] = min3p(m0[0], d00, d10);
                    m1[0] = min3p(m1[0], d01, d11);
                } else {
                    topk_insert<KNN>(m0, d00);
                    topk_insert<KNN>(m0, d10);
                    topk_insert<KNN>(m1, d01);
                    topk_insert<KNN>(m1, d11);
                }
            }
        }
    }
    flush(o);
}

// ---------------------------------------------------------------------------------------------
// Half-tile pipelined form of the fp32 kernel (k = 1, the shipped headline path).  Same decomposition, operand
// images and arithmetic as global_match_f32_kernel<KS, 1> -- every accumulator is the same k-ascending fmaf chain,
// d = fmaf(-2, mm, xs + ys): bit-identical results -- but the tile is computed as two phases of 100 MFMAs:
//   phase A  rows  0-31 (c00, c01)   while the VALU reduces rows 32-63 of the PREVIOUS tile (c10, c11 still hold
//                                     them; their |k|^2 were copied to 16 registers before the buffer was recycled)
//   phase B  rows 32-63 (c10, c11)   while the VALU reduces rows 0-31 of this tile
// r2 PMC of the un-pipelined kernel: matrix pipe 90 % busy -- the two co-resident workgroups of a CU run in
// lockstep, so their ~1.3 k-cycle epilogues (add, fma, min per element) coincide and the pipe idles for exactly
// that share of a 12.8 k-cycle tile.  Here a wave's MFMA stream never stops for an epilogue.
// Staging by asm LDS-DMA (see lds_dma16): it frees the 28 staging VGPRs the 16 carried |k|^2 need, and removes
// the ds_write pass; one raw s_barrier per tile.
// RESCUE (MANET_COMPUTE_BF16_REFINE): the same kernel as the exact fall-back of the bf16 filter -- a workgroup returns at
// once unless one of its query tile's eight 32-query blocks has an incomplete candidate bucket (bit 31 or a count past
// the capacity); the minima meet the re-rank's by atomicMin on the same keys (the same fp32 chains: the same bits).
template <int KS, bool RESCUE = false>
__global__ __launch_bounds__(256, 2) void global_match_f32_pipe_kernel(const char *__restrict__ qpack,
                                                                       const char *__restrict__ bpack,
                                                                       const int *__restrict__ meta, int n_ids,
                                                                       int nQT, int S, long N_pad,
                                                                       unsigned *__restrict__ keys, int block_map,
                                                                       const unsigned *__restrict__ bcnt = nullptr,
                                                                       long bucket_cap = 0)
{
    constexpr int NG = (KS + 3) / 4;
    constexpr size_t TILE_BYTES = bank_tile_bytes(NG);  // whole KiB
    constexpr size_t QBLK_BYTES = query_block_bytes(NG);
    constexpr int PIECES = (int)(TILE_BYTES / 1024);
    constexpr int NW = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 x TILE_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int h = lane >> 5;

    int qt, s, t0, t1;
    const int T = meta[META_T];
    if (RESCUE && (block_map & RESCUE_LISTED)) {
        // the tiles to rescue were listed by the re-rank launch (rs = {count, tile ids}, behind bcnt's two halves): the
        // launch's workgroups are dealt to THOSE tiles, with as many bank splits each as the grid allows -- a frame with a
        // handful of incomplete tiles spreads them over the whole chip instead of leaving each to 16 workgroups (r4: 1.5 ms
        // for 4 of 102 tiles at cfg2 size, the time one workgroup needs for a 16th of the bank)
        const unsigned *rs = bcnt + 2 * (N_pad >> 5);
        const int nr = (int)rs[0];
        if (nr <= 0) return;
        // splits per tile: whole rounds of the chip's 512 workgroup slots (a workgroup's fixed cost -- its 106 KB query
        // operand, the pipeline fill, the closing atomics -- is worth ~6 tiles of matrix work: few long workgroups beat many
        // short ones; 4 tiles of 102 at cfg2 size: 390 us with 404 splits of 5 tiles, 3.2 rounds)
        int Sd = (block_map >> 8) & BLOCK_MAP_RESCUE_MASK;  // (a forced count; the shipped launch passes 0: the choice below)
        if (Sd > 0) {
            const int most_grid = (int)gridDim.x / nr;
            Sd = Sd > most_grid ? most_grid : Sd;
            Sd = Sd < 1 ? 1 : Sd;
        } else {
            const int most_grid = (int)gridDim.x / nr, most_t = T / 8 > 1 ? T / 8 : 1;
            const int most = most_grid < most_t ? most_grid : most_t;
            long best = -1;
            for (int r = 1; r <= 4; ++r) {
                int c = (512 * r) / nr;
                c = c < 1 ? 1 : (c > most ? most : c);
                const long rounds = ((long)nr * c + 511) / 512;
                const long cost = rounds * ((long)(T + c - 1) / c + 6);
                if (best < 0 || cost < best) { best = cost; Sd = c; }
            }
        }
        if ((int)blockIdx.x >= nr * Sd) return;
        s = (int)blockIdx.x / nr;
        qt = (int)rs[1 + ((int)blockIdx.x - s * nr)];
        t0 = (int)((long)s * T / Sd);
        t1 = (int)((long)(s + 1) * T / Sd);
        if (t0 >= t1) return;
    } else {
        if (!split_of_block(blockIdx.x, nQT, S, T, block_map, qt, s, t0, t1)) return;
        if (RESCUE) {
            bool need = false;
            for (int i = 0; i < QT / QB; ++i) {
                const unsigned raw = bcnt[(long)qt * (QT / QB) + i];
                need = need || (raw >> 31) || (long)raw > bucket_cap;
            }
            if (!need) return;  // (wave-uniform: every lane read the same eight counters)
        }
    }

    const unsigned smem_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)smem);
    auto stage_dma = [&](int t, int slot) __attribute__((always_inline)) {
        const char *g = bpack + (size_t)t * TILE_BYTES + (size_t)lane * 16;
        const unsigned l = smem_base + (unsigned)slot * (unsigned)TILE_BYTES;
#pragma unroll
        for (int i = 0; i < (PIECES + NW - 1) / NW; ++i) {
            const int pc = wave + i * NW;  // wave-uniform
            if (pc < PIECES) lds_dma16(g + (size_t)pc * 1024, l + (unsigned)pc * 1024u);
        }
    };
    stage_dma(t0, 0);

    f32x4 q0[NG], q1[NG];
    float xs0, xs1;
    {
        const char *qb0 = qpack + (size_t)(qt * (QT / QB) + wave * 2) * QBLK_BYTES;
        const char *qb1 = qb0 + QBLK_BYTES;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            q0[g] = *(const f32x4 *)(qb0 + ((size_t)(g * 2 + h) * QB + l31) * 16);
            q1[g] = *(const f32x4 *)(qb1 + ((size_t)(g * 2 + h) * QB + l31) * 16);
        }
        xs0 = *(const float *)(qb0 + (size_t)NG * 2 * QB * 16 + l31 * 4);
        xs1 = *(const float *)(qb1 + (size_t)NG * 2 * QB * 16 + l31 * 4);
    }
    const long qbase = (long)qt * QT + wave * 64 + l31;
    // the compiler waits for the query operand HERE (its counted vmcnt waits must not sink into the tile loop,
    // where they would drain the LDS-DMA it does not know about)
#pragma unroll
    for (int g = 0; g < NG; ++g) asm volatile("" : "+v"(q0[g]), "+v"(q1[g]));
    asm volatile("" : "+v"(xs0), "+v"(xs1));

    int o = 0;
    while (meta[META_SEG + o + 1] <= t0) ++o;  // object owning tile t0
    int seg_end = meta[META_SEG + o + 1];
    float m0a, m0b, m1a, m1b;  // two running minima per query block: short dependency chains
    m0a = m0b = m1a = m1b = MANET_WRONG_LABEL_PADDING_DISTANCE;
    auto flush = [&](int obj) {
        const float v0 = min3p(m0a, m0b, m0b), v1 = min3p(m1a, m1b, m1b);
        const float a = min3p(v0, v0, __shfl_xor(v0, 32));
        const float c = min3p(v1, v1, __shfl_xor(v1, 32));
        if (h == 0) {
            atomicMin(keys + (size_t)obj * N_pad + qbase, key_of(a));
            atomicMin(keys + (size_t)obj * N_pad + qbase + 32, key_of(c));
        }
    };

    // pending = rows 32-63 of the previous tile: still in c10 / c11, their |k|^2 in yp[]; "nothing pending" is
    // expressed by values that cannot win (c = 0, |k|^2 = 1e20 -> d = 1e20)
    f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
    float yp[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) yp[r] = MANET_WRONG_LABEL_PADDING_DISTANCE;
    // the reference's d = (xs + ys) - 2 mm with its two roundings (IntVOS.py:39), then the running minimum
#define MANET_REDUCE(ca_, cb_, y_, r_)                                                             \
    {                                                                                              \
        const float da_ = fmaf(-2.0f, ca_[r_], xs0 + (y_));                                        \
        const float db_ = fmaf(-2.0f, cb_[r_], xs1 + (y_));                                        \
        if ((r_) & 1) {                                                                            \
            m0b = min3p(m0b, da_, da_);                                                            \
            m1b = min3p(m1b, db_, db_);                                                            \
        } else {                                                                                   \
            m0a = min3p(m0a, da_, da_);                                                            \
            m1a = min3p(m1a, db_, db_);                                                            \
        }                                                                                          \
    }
    auto settle = [&]() __attribute__((always_inline)) {  // reduce what is pending, serially (object boundary, end)
#pragma unroll
        for (int r = 0; r < 16; ++r) MANET_REDUCE(c10, c11, yp[r], r);
#pragma unroll
        for (int r = 0; r < 16; ++r) yp[r] = MANET_WRONG_LABEL_PADDING_DISTANCE;
        c10 = f32x16{0};
        c11 = f32x16{0};
    };

    for (int t = t0; t < t1; ++t) {
        const int buf = (t - t0) & 1;
        // this wave's pieces of tile t have landed (issued one tile ago); the barrier publishes the tile and tells
        // us that every wave is done with the other buffer (tile t-1: fragments consumed, |k|^2 copied to yp)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + 1 < t1) stage_dma(t + 1, buf ^ 1);  // in flight during this tile's 200 MFMAs
        if (t >= seg_end) {  // wave-uniform: crossed into the next object's rows
            settle();
            flush(o);
            m0a = m0b = m1a = m1b = MANET_WRONG_LABEL_PADDING_DISTANCE;
            do { ++o; seg_end = meta[META_SEG + o + 1]; } while (t >= seg_end);
        }
        const char *tb = smem + (size_t)buf * TILE_BYTES;
        const f32x4 *A = (const f32x4 *)tb;
        const float *ysl = (const float *)(tb + (size_t)NG * 2 * BT * 16);
        // ---- phase A: rows 0-31 of tile t on the matrix pipe, rows 32-63 of tile t-1 on the VALU
        c00 = f32x16{0};
        c01 = f32x16{0};
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const f32x4 a0 = A[(g * 2 + h) * BT + l31];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (g * 4 + j < KS) {  // compile-time: k-steps beyond C are all-zero, skip them
                    c00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], q0[g][j], c00, 0, 0, 0);
                    c01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], q1[g][j], c01, 0, 0, 0);
                }
            }
            // the 16 pending registers spread over the NG fragment groups
#pragma unroll
            for (int r = (g * 16) / NG; r < ((g + 1) * 16) / NG; ++r) MANET_REDUCE(c10, c11, yp[r], r);
        }
        // |k|^2 of rows 32-63 of THIS tile, for the next tile's phase A (register r = row 32 + (r&3) + 8(r>>2) + 4h)
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) {
            const f32x4 y1 = *(const f32x4 *)(ysl + 32 + 8 * tq + 4 * h);
#pragma unroll
            for (int i = 0; i < 4; ++i) yp[4 * tq + i] = y1[i];
        }
        // ---- phase B: rows 32-63 of tile t on the matrix pipe, rows 0-31 of tile t on the VALU
        c10 = f32x16{0};
        c11 = f32x16{0};
        f32x4 y0v[4];
#pragma unroll
        for (int tq = 0; tq < 4; ++tq) y0v[tq] = *(const f32x4 *)(ysl + 8 * tq + 4 * h);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const f32x4 a1 = A[(g * 2 + h) * BT + 32 + l31];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (g * 4 + j < KS) {
                    c10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], q0[g][j], c10, 0, 0, 0);
                    c11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], q1[g][j], c11, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = (g * 16) / NG; r < ((g + 1) * 16) / NG; ++r) MANET_REDUCE(c00, c01, y0v[r >> 2][r & 3], r);
        }
    }
    settle();
#undef MANET_REDUCE
    flush(o);
}

// ---------------------------------------------------------------------------------------------
// the bf16 MFMA of the three bf16 kernels below (macros: the device code is what it was with the text in each kernel)
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
#define MANET_BF(x) __builtin_bit_cast(bf16x8_t, x)
#define MANET_MFMA(a_, b_, c_) c_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(MANET_BF(a_), MANET_BF(b_), c_, 0, 0, 0)
// The two plain kernels (one MFMA per 16 k) are templates on the ELEMENT of their operand images: bf16 (MANET_COMPUTE_BF16) or
// fp16 (MANET_COMPUTE_F16, v_mfma_f32_32x32x16_f16: the same operand shape, 8 two-byte elements per lane).  Everything else --
// tiles, staging, schedule, the minimum -- is one __device__ body per kernel; each element has thin __global__ wrappers of its own
// (global_match_bf16_wide_kernel / _pipe_kernel, f16_match_wide_kernel / _pipe_kernel).
struct ElemBF16 {};
struct ElemF16 {};
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
#define MANET_HF(x) __builtin_bit_cast(f16x8_t, x)
#define MANET_MFMA_E(a_, b_, c_)                                                                               \
    {                                                                                                          \
        if constexpr (std::is_same<E, ElemF16>::value)                                                         \
            c_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(MANET_HF(a_), MANET_HF(b_), c_, 0, 0, 0);              \
        else                                                                                                   \
            c_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(MANET_BF(a_), MANET_BF(b_), c_, 0, 0, 0);             \
    }

// ---------------------------------------------------------------------------------------------
// main kernel, split-bf16 operands (MANET_COMPUTE_BF16X3): one workgroup = 512 queries x one bank
// split, 8 waves.  Same decomposition as the f32 kernel (swapped operands, object-pure 64-row tiles,
// lane-local running min, atomicMin across splits); the contraction is v_mfma_f32_32x32x16_bf16 with fp32
// accumulation of hi*hi + hi*lo + lo*hi with x = hi + lo, hi = bf16(x), lo = bf16(x - hi): the dropped
// lo*lo term is <= 2^-16 relative, i.e. fp32-class distances at 3/16 of the f32 MFMA cost.
// The operand images carry -2q and both squared norms (see Geom), so an accumulator element IS
// d(n, m) = |q|^2 + |k|^2 - 2 q.k when the k loop ends: the epilogue is ONE v_minimum3_f32 per two
// elements (r1: add + fma + min per element = 6x the VALU work, 0.32 of 0.68 ms).
// Staging: one tile per step, double buffered in LDS by asm LDS-DMA (no VGPR round trip, no ds_write pass,
// the loads of step s+1 fly during the whole of step s).
template <int KSB>
__global__ __launch_bounds__(512, 1) void global_match_bf16x3_kernel(const char *__restrict__ qpack,
                                                                     const char *__restrict__ bpack,
                                                                     const int *__restrict__ meta, int n_ids,
                                                                     int nQT, int S, long N_pad,
                                                                     unsigned *__restrict__ keys, int block_map)
{
    constexpr int NW = 8;
    constexpr int UNITS = 4 * KSB;
    constexpr int LO = 2 * KSB;  // first unit of the lo image
    constexpr size_t TILE_BYTES = bank_tile_bytes_u(UNITS, false);  // = UNITS KiB
    constexpr size_t QBLK_BYTES = query_block_bytes_u(UNITS, false);
    constexpr int QTB = NW * 64;
    static_assert(TILE_BYTES == (size_t)UNITS * 1024, "a bf16 tile is a whole number of 1 KiB DMA pieces");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 x TILE_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int h = lane >> 5;

    int qt, s, t0, t1;
    const int T = meta[META_T];
    if (!split_of_block(blockIdx.x, nQT, S, T, block_map, qt, s, t0, t1)) return;

    // ---- staging of one tile: UNITS 1 KiB pieces, dealt to the waves ---------------------------------
    const unsigned smem_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)smem);
    auto stage_dma = [&](int t, int slot) __attribute__((always_inline)) {
        const int np = ((t1 - t) < 1 ? (t1 - t) : 1) * UNITS;  // (<= 0 behind the split's end: nothing staged)
        const char *g = bpack + (size_t)t * TILE_BYTES + (size_t)lane * 16;
        const unsigned l = smem_base + (unsigned)slot * (unsigned)TILE_BYTES;
#pragma unroll
        for (int i = 0; i < (UNITS + NW - 1) / NW; ++i) {
            const int pc = wave + i * NW;  // wave-uniform
            if (pc < np) lds_dma16(g + (size_t)pc * 1024, l + (unsigned)pc * 1024u);
        }
    };
    stage_dma(t0, 0);

    // B operand: lane holds (-2q | norm slots)[j = lane&31][k = 16s + 8*(lane>>5) + 0..7] for its two blocks, hi and lo image
    u32x4 q0[KSB], q1[KSB], q0l[KSB], q1l[KSB];
    {
        const char *qb0 = qpack + (size_t)(qt * (QTB / QB) + wave * 2) * QBLK_BYTES;
        const char *qb1 = qb0 + QBLK_BYTES;
#pragma unroll
        for (int k = 0; k < KSB; ++k) {
            q0[k] = *(const u32x4 *)(qb0 + ((size_t)(k * 2 + h) * QB + l31) * 16);
            q1[k] = *(const u32x4 *)(qb1 + ((size_t)(k * 2 + h) * QB + l31) * 16);
            q0l[k] = *(const u32x4 *)(qb0 + ((size_t)(LO + k * 2 + h) * QB + l31) * 16);
            q1l[k] = *(const u32x4 *)(qb1 + ((size_t)(LO + k * 2 + h) * QB + l31) * 16);
        }
    }
    const long qbase = (long)qt * QTB + wave * 64 + l31;
    // Make the compiler wait for the query operand HERE.  Otherwise its counted vmcnt waits for these
    // loads sink into the tile loop (down to vmcnt(0)), where they would also drain the asm LDS-DMA of the
    // next step that the compiler does not know about.
#pragma unroll
    for (int k = 0; k < KSB; ++k) {
        asm volatile("" : "+v"(q0[k]), "+v"(q1[k]));
        asm volatile("" : "+v"(q0l[k]), "+v"(q1l[k]));
    }

    int o = 0;
    while (meta[META_SEG + o + 1] <= t0) ++o;
    int seg_end = meta[META_SEG + o + 1];
    // two running minima per query block (even / odd accumulator registers): short dependency chains
    float m0a, m0b, m1a, m1b;
    m0a = m0b = m1a = m1b = MANET_WRONG_LABEL_PADDING_DISTANCE;
    auto flush = [&](int obj) {
        float a = min3p(m0a, m0b, __shfl_xor(min3p(m0a, m0b, m0b), 32));
        float c = min3p(m1a, m1b, __shfl_xor(min3p(m1a, m1b, m1b), 32));
        if (h == 0) {
            atomicMin(keys + (size_t)obj * N_pad + qbase, key_of(a));
            atomicMin(keys + (size_t)obj * N_pad + qbase + 32, key_of(c));
        }
    };
    // one 64-row tile: 12 x KSB MFMAs from zero accumulators, then the running minimum
    auto tile = [&](const char *tb) __attribute__((always_inline)) {
        const u32x4 *A = (const u32x4 *)tb;
        f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};
#pragma unroll
        for (int k = 0; k < KSB; ++k) {
            u32x4 a0 = A[(k * 2 + h) * BT + l31];
            u32x4 a1 = A[(k * 2 + h) * BT + 32 + l31];
            u32x4 a0l = A[(LO + k * 2 + h) * BT + l31];
            u32x4 a1l = A[(LO + k * 2 + h) * BT + 32 + l31];
            MANET_MFMA(a0, q0[k], c00);
            MANET_MFMA(a1, q0[k], c10);
            MANET_MFMA(a0, q1[k], c01);
            MANET_MFMA(a1, q1[k], c11);
            MANET_MFMA(a0, q0l[k], c00);
            MANET_MFMA(a1, q0l[k], c10);
            MANET_MFMA(a0, q1l[k], c01);
            MANET_MFMA(a1, q1l[k], c11);
            MANET_MFMA(a0l, q0[k], c00);
            MANET_MFMA(a1l, q0[k], c10);
            MANET_MFMA(a0l, q1[k], c01);
            MANET_MFMA(a1l, q1[k], c11);
        }
        // accumulator register r of block rb = bank row rb*32 + (r&3) + 8*(r>>2) + 4*h; all of them belong
        // to the same object, so the reduction over rows is register-wise
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            m0a = min3p(m0a, c00[r], c10[r]);
            m0b = min3p(m0b, c00[r + 1], c10[r + 1]);
            m1a = min3p(m1a, c01[r], c11[r]);
            m1b = min3p(m1b, c01[r + 1], c11[r + 1]);
        }
    };
    auto next_object = [&](int t) __attribute__((always_inline)) {
        if (t >= seg_end) {  // wave-uniform: tile t starts another object's rows
            flush(o);
            m0a = m0b = m1a = m1b = MANET_WRONG_LABEL_PADDING_DISTANCE;
            do { ++o; seg_end = meta[META_SEG + o + 1]; } while (t >= seg_end);
        }
    };
    int buf = 0;
    for (int t = t0; t < t1; ++t, buf ^= 1) {
        // this wave's pieces of the tile have landed; the barrier then publishes everybody's pieces
        // and tells us that every wave is done reading the other buffer (the previous tile)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + 1 < t1) stage_dma(t + 1, buf ^ 1);  // in flight during the whole step
        next_object(t);
        tile(smem + (size_t)buf * TILE_BYTES);
    }
    flush(o);
}

// ---------------------------------------------------------------------------------------------
// Software-pipelined form of the plain-bf16 kernel (the shipped one for MANET_COMPUTE_BF16).
// Same decomposition as global_match_bf16x3_kernel, one MFMA per 16 k on embeddings rounded to bf16 (7 instead of
// 50 MFMAs per block at C = 100) and two tiles per step; what differs is WHEN
// things are issued, so that the matrix pipe never waits for LDS (r2 PMC of the kernel above: pipe 67 %
// busy, waves parked 37 % of their cycles on s_waitcnt -- the A-fragment reads right behind every barrier):
//   * a step = 2 tiles (A, B); fragment registers F[k] are bound to k-step k: as soon as the four MFMAs of
//     (tile, k) have been issued, F[k] is refilled with the NEXT tile's k-step -- every ds_read_b128 is in
//     flight for a whole tile (~7 x 128 matrix cycles) before its MFMA needs it;
//   * the step's barrier sits BETWEEN tile A and tile B.  By then tile B's fragments are already in
//     registers, so the barrier (a) publishes the next step's buffer, whose first fragments tile B's k-steps
//     prefetch, and (b) frees the current buffer for the LDS-DMA of the step after next.  No fragment read
//     ever follows a barrier directly; two LDS buffers suffice.
// (A 3-deep LDS ring with counted vmcnt(N) waits -- the DMA two steps ahead -- was measured slower, 0.529 vs
// 0.498 ms, and removed: DMA latency is not the stall.)
template <int KSB, typename E>
__device__ __forceinline__ void plain_pipe_body(const char *__restrict__ qpack, const char *__restrict__ bpack,
                                   const int *__restrict__ meta, int n_ids, int nQT, int S, long N_pad,
                                   unsigned *__restrict__ keys, int block_map)
{
    constexpr int NW = 8, TPS = 2;
    constexpr int UNITS = 2 * KSB;
    constexpr size_t TILE_BYTES = bank_tile_bytes_u(UNITS, false);  // = UNITS KiB
    constexpr size_t QBLK_BYTES = query_block_bytes_u(UNITS, false);
    constexpr size_t STEP_BYTES = TILE_BYTES * TPS;
    constexpr int QTB = NW * 64;
    constexpr int NBUF = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];  // NBUF x STEP_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31;
    const int h = lane >> 5;

    int qt, s, t0, t1;
    const int T = meta[META_T];
    if (!split_of_block(blockIdx.x, nQT, S, T, block_map, qt, s, t0, t1)) return;

    constexpr int PIECES = UNITS * TPS;  // 1 KiB pieces per step
    const unsigned smem_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)smem);
    auto stage_dma = [&](int t, int slot) __attribute__((always_inline)) {
        const int np = ((t1 - t) < TPS ? (t1 - t) : TPS) * UNITS;  // the split's last step may be short
        const char *g = bpack + (size_t)t * TILE_BYTES + (size_t)lane * 16;
        const unsigned l = smem_base + (unsigned)slot * (unsigned)STEP_BYTES;
#pragma unroll
        for (int i = 0; i < (PIECES + NW - 1) / NW; ++i) {
            const int pc = wave + i * NW;  // wave-uniform
            if (pc < np) lds_dma16(g + (size_t)pc * 1024, l + (unsigned)pc * 1024u);
        }
    };
    stage_dma(t0, 0);
    if (t0 + TPS < t1) stage_dma(t0 + TPS, 1);

    u32x4 q0[KSB], q1[KSB];
    {
        const char *qb0 = qpack + (size_t)(qt * (QTB / QB) + wave * 2) * QBLK_BYTES;
        const char *qb1 = qb0 + QBLK_BYTES;
#pragma unroll
        for (int k = 0; k < KSB; ++k) {
            q0[k] = *(const u32x4 *)(qb0 + ((size_t)(k * 2 + h) * QB + l31) * 16);
            q1[k] = *(const u32x4 *)(qb1 + ((size_t)(k * 2 + h) * QB + l31) * 16);
        }
    }
    const long qbase = (long)qt * QTB + wave * 64 + l31;
#pragma unroll
    for (int k = 0; k < KSB; ++k) asm volatile("" : "+v"(q0[k]), "+v"(q1[k]));  // compiler waits for q here

    int o = 0;
    while (meta[META_SEG + o + 1] <= t0) ++o;
    int seg_end = meta[META_SEG + o + 1];
    float m0a, m0b, m1a, m1b;
    m0a = m0b = m1a = m1b = MANET_WRONG_LABEL_PADDING_DISTANCE;
    auto flush = [&](int obj) {
        float a = min3p(m0a, m0b, __shfl_xor(min3p(m0a, m0b, m0b), 32));
        float c = min3p(m1a, m1b, __shfl_xor(min3p(m1a, m1b, m1b), 32));
        if (h == 0) {
            atomicMin(keys + (size_t)obj * N_pad + qbase, key_of(a));
            atomicMin(keys + (size_t)obj * N_pad + qbase + 32, key_of(c));
        }
    };
    auto next_object = [&](int t) __attribute__((always_inline)) {
        if (t >= seg_end) {  // wave-uniform: tile t starts another object's rows
            flush(o);
            m0a = m0b = m1a = m1b = MANET_WRONG_LABEL_PADDING_DISTANCE;
            do { ++o; seg_end = meta[META_SEG + o + 1]; } while (t >= seg_end);
        }
    };
    // this lane's fragment offset inside a tile image: unit (2k + h), rows l31 and 32 + l31
    const unsigned frag_off = (unsigned)((h * BT + l31) * 16);
    u32x4 F0[KSB], F1[KSB];
#define MANET_LOADF(k_, tile_base_)                                                                \
    {                                                                                              \
        const char *f_ = (tile_base_) + frag_off + (size_t)(k_) * (2 * BT * 16);                   \
        F0[k_] = *(const u32x4 *)f_;                                                               \
        F1[k_] = *(const u32x4 *)(f_ + 32 * 16);                                                   \
    }
    // one tile: MFMAs of k-step k from F[k], then F[k] <- k-step k of the tile at `next_base`
#define MANET_TILE(next_base_)                                                                     \
    {                                                                                              \
        f32x16 c00 = {0}, c01 = {0}, c10 = {0}, c11 = {0};                                         \
        _Pragma("unroll") for (int k = 0; k < KSB; ++k)                                            \
        {                                                                                          \
            MANET_MFMA_E(F0[k], q0[k], c00);                                                         \
            MANET_MFMA_E(F1[k], q0[k], c10);                                                         \
            MANET_MFMA_E(F0[k], q1[k], c01);                                                         \
            MANET_MFMA_E(F1[k], q1[k], c11);                                                         \
            MANET_LOADF(k, next_base_);                                                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); /* 4 MFMA  */                       \
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0); /* 2 DS read: the refill, right behind them */ \
        }                                                                                          \
        _Pragma("unroll") for (int r = 0; r < 16; r += 2)                                          \
        {                                                                                          \
            m0a = min3p(m0a, c00[r], c10[r]);                                                      \
            m0b = min3p(m0b, c00[r + 1], c10[r + 1]);                                              \
            m1a = min3p(m1a, c01[r], c11[r]);                                                      \
            m1b = min3p(m1b, c01[r + 1], c11[r + 1]);                                              \
        }                                                                                          \
    }

    // prologue: steps 0 and 1 in flight; publish step 0, fetch tile A's fragments
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < KSB; ++k) MANET_LOADF(k, smem);

    int buf = 0;
    for (int t = t0; t < t1; t += TPS, buf ^= 1) {
        const char *cur = smem + (size_t)buf * STEP_BYTES;
        const char *nxt = smem + (size_t)(buf ^ 1) * STEP_BYTES;
        // ---- tile A (its fragments are in F; refill F with tile B of the same buffer)
        next_object(t);
        MANET_TILE(cur + TILE_BYTES);
        // ---- mid-step: everything of this buffer is in registers now.  This wave's pieces of the next step have
        // landed (issued one step ago); the barrier publishes the next step's buffer and frees this one for the
        // step after next.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of `cur` have returned
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + NBUF * TPS < t1) stage_dma(t + NBUF * TPS, buf);
        // ---- tile B (refill F with tile A of the next step's buffer; a stale read if there is none)
        if (t + 1 < t1) {
            next_object(t + 1);
            MANET_TILE(nxt);
        }
    }
#undef MANET_TILE
#undef MANET_LOADF
    flush(o);
}
template <int KSB>
__global__ __launch_bounds__(512, 1) __attribute__((amdgpu_waves_per_eu(2, 2)))
void global_match_bf16_pipe_kernel(const char *__restrict__ qpack, const char *__restrict__ bpack,
                                   const int *__restrict__ meta, int n_ids, int nQT, int S, long N_pad,
                                   unsigned *__restrict__ keys, int block_map)
{
    plain_pipe_body<KSB, ElemBF16>(qpack, bpack, meta, n_ids, nQT, S, N_pad, keys, block_map);
}
// MANET_COMPUTE_F16, C > 106.  (The fp16 kernels are named f16_*: the library's global_match_* kernels are the set they were.)
template <int KSB>
__global__ __launch_bounds__(512, 1) __attribute__((amdgpu_waves_per_eu(2, 2)))
void f16_match_pipe_kernel(const char *__restrict__ qpack, const char *__restrict__ bpack, const int *__restrict__ meta, int n_ids,
                           int nQT, int S, long N_pad, unsigned *__restrict__ keys, int block_map)
{
    plain_pipe_body<KSB, ElemF16>(qpack, bpack, meta, n_ids, nQT, S, N_pad, keys, block_map);
}

// ---------------------------------------------------------------------------------------------
// "Wide" form of the pipelined plain-bf16 kernel: 4 waves per workgroup, each wave owns 128 queries (four
// 32-query blocks, 112 VGPRs of -2q operand) and walks the bank in PASSES of 32 rows: 4 x KSB MFMAs per pass,
// four independent accumulators, one A fragment per k-step (7 ds_read_b128 per 28 MFMAs -- half the LDS
// fragment traffic of the 64 x 64 wave tile).  Same 512 queries per workgroup and the same packed images as
// the other bf16 kernels, but TWO workgroups per CU (256 threads, <= 256 VGPRs): their barriers are
// independent, and the prologue / flush of one overlaps the matrix work of the other.
//   step = 2 tiles = 4 passes; fragments F[k] bound to k, refilled with the next pass's k-step right behind
//   the MFMAs that consumed them; the step's barrier sits before the LAST pass (its fragments are already in
//   registers): it publishes the next step's buffer and frees the current one for the LDS-DMA of step + 2.
// FILTER (MANET_COMPUTE_BF16_REFINE, second pass): instead of reducing to a minimum, every bank row whose bf16 distance is
// within the query's threshold thr[object][query] is appended to the flat candidate list {pair, bank slot} (stats[0] = its
// fill count; an entry that does not fit raises stats[1]).  A pass's 16 distances per lane are first reduced to their minimum --
// the same eight v_minimum3 the plain kernel spends -- and only a wave in which some lane's minimum passes its threshold
// takes the slow path that looks at the individual rows.
template <int KSB, bool FILTER, typename E>
__device__ __forceinline__ void plain_wide_body(const char *__restrict__ qpack,
                                                                        const char *__restrict__ bpack,
                                                                        const int *__restrict__ meta, int n_ids,
                                                                        int nQT, int S, long N_pad,
                                                                        unsigned *__restrict__ keys, int block_map,
                                                                        unsigned *__restrict__ thr,
                                                                        const float *__restrict__ slack,
                                                                        unsigned long long *__restrict__ stats,
                                                                        uint2 *__restrict__ list, long bucket_cap,
                                                                        unsigned *__restrict__ bcnt)
{
    constexpr int NW = 4, TPS = 2, NQB = 4;  // waves, tiles per step, query blocks per wave
    constexpr int UNITS = 2 * KSB;
    constexpr size_t TILE_BYTES = bank_tile_bytes_u(UNITS, false);  // = UNITS KiB
    constexpr size_t QBLK_BYTES = query_block_bytes_u(UNITS, false);
    constexpr size_t STEP_BYTES = TILE_BYTES * TPS;
    constexpr int QTB = QT_BF16;
    static_assert(NW * NQB * QB == QTB, "4 waves x 4 blocks x 32 queries");
    extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 x STEP_BYTES

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int l31 = lane & 31;
    const int h = lane >> 5;

    int qt, s, t0, t1;
    const int T = meta[META_T];
    if (FILTER && (block_map & 0xff) == 8) {
        if (!tapered_split_of_block(blockIdx.x, nQT, S, T, qt, s, t0, t1)) return;
    } else if (!split_of_block(blockIdx.x, nQT, S, T, block_map, qt, s, t0, t1))
        return;

    constexpr int PIECES = UNITS * TPS;  // 1 KiB pieces per step
    const unsigned smem_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)smem);
    auto stage_dma = [&](int t, int slot) __attribute__((always_inline)) {
        const int np = ((t1 - t) < TPS ? (t1 - t) : TPS) * UNITS;  // the split's last step may be short
        const unsigned l = smem_base + (unsigned)slot * (unsigned)STEP_BYTES;
        if (FILTER) {  // (at the register limit: a uniform base + this lane's 32-bit offset, no 64-bit address pair)
            const char *g = bpack + (size_t)t * TILE_BYTES;
#pragma unroll
            for (int i = 0; i < (PIECES + NW - 1) / NW; ++i) {
                const int pc = wave + i * NW;  // wave-uniform
                if (pc < np) lds_dma16_s(g + (size_t)pc * 1024, (unsigned)lane * 16u, l + (unsigned)pc * 1024u);
            }
            return;
        }
        const char *g = bpack + (size_t)t * TILE_BYTES + (size_t)lane * 16;
#pragma unroll
        for (int i = 0; i < (PIECES + NW - 1) / NW; ++i) {
            const int pc = wave + i * NW;  // wave-uniform
            if (pc < np) lds_dma16(g + (size_t)pc * 1024, l + (unsigned)pc * 1024u);
        }
    };
    stage_dma(t0, 0);
    if (t0 + TPS < t1) stage_dma(t0 + TPS, 1);

    u32x4 q[NQB][KSB];
    {
        const char *qb = qpack + (size_t)(qt * (QTB / QB) + wave * NQB) * QBLK_BYTES;
#pragma unroll
        for (int j = 0; j < NQB; ++j)
#pragma unroll
            for (int k = 0; k < KSB; ++k)
                q[j][k] = *(const u32x4 *)(qb + (size_t)j * QBLK_BYTES + ((size_t)(k * 2 + h) * QB + l31) * 16);
    }
    const unsigned qbase = (unsigned)(qt * QTB + wave * (NQB * QB) + l31);  // (N_pad < 2^31: check_common)
#pragma unroll
    for (int j = 0; j < NQB; ++j)
#pragma unroll
        for (int k = 0; k < KSB; ++k) asm volatile("" : "+v"(q[j][k]));  // compiler waits for q here

    int o = 0;
    while (meta[META_SEG + o + 1] <= t0) ++o;
    int seg_end = meta[META_SEG + o + 1];
    float ma[NQB], mb[NQB];  // two running minima per query block (even / odd accumulator registers)
    // FILTER: this lane's four queries' thresholds for the current object.  tq starts at the pair's current global
    // threshold -- the pre-pass's bound + slack, already tightened by the workgroups that finished before this one -- and
    // tightens to (smallest bf16 distance this lane meets) + slack: any row's bf16 distance bounds the minimum the same way
    // the pre-pass's does, and the slack 2.1 E(U) only shrinks with U.  Leaving an object, the lane publishes its threshold
    // (atomicMin on the key): the later rounds of workgroups filter against nearly the final minimum, which is what keeps
    // the candidate lists short.
    float tq[NQB], sq[NQB];
#pragma unroll
    for (int j = 0; j < NQB; ++j) ma[j] = mb[j] = MANET_WRONG_LABEL_PADDING_DISTANCE;
    // FILTER: the lowest key this lane KNOWS to be published for its four (query, object) pairs -- what it read or wrote
    // last -- lives in LDS (touched at exchanges only).  A lane publishes only below it: every lane every time was 13 M
    // atomics per launch, most of them no-ops at the L2 -- the filter pass's main overhead over the plain kernel.
    unsigned *pks = (unsigned *)(smem + 2 * STEP_BYTES + (size_t)REFINE_LDS_LIST * 8) + wave * 256 + lane;
    auto load_thr = [&](int obj) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NQB; ++j) {
            const unsigned kpub = FILTER ? (thr + (size_t)obj * N_pad)[qbase + 32u * j] : 0u;
            tq[j] = FILTER ? float_of(kpub) : 0.0f;
            sq[j] = FILTER ? (slack + (size_t)obj * N_pad)[qbase + 32u * j] : 0.0f;
            if (FILTER) pks[64 * j] = kpub;
        }
    };
    if (FILTER) load_thr(o);
    auto flush = [&](int obj) {
        if (FILTER) {
#pragma unroll
            for (int j = 0; j < NQB; ++j) {
                const float a = fminf(tq[j], __shfl_xor(tq[j], 32));
                const unsigned ka = key_of(a);
                if (h == 0 && a == a && ka < pks[64 * j]) {
                    atomicMin(&(thr + (size_t)obj * N_pad)[qbase + 32u * j], ka);
                    pks[64 * j] = ka;
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < NQB; ++j) {
            const float v = min3p(ma[j], mb[j], mb[j]);
            const float a = min3p(v, v, __shfl_xor(v, 32));
            if (h == 0) atomicMin(&(keys + (size_t)obj * N_pad)[qbase + 32u * j], key_of(a));
        }
    };
    // FILTER: minimum of a pass's 16 distances of one query block, and the slow path that appends the qualifying rows
    // (accumulator register r of lane (l31, h) is bank row (r & 3) + 8 (r >> 2) + 4 h of the pass)
    auto min16 = [&](const f32x16 &c) __attribute__((always_inline)) {
        float p = min3p(c[0], c[1], c[2]);
#pragma unroll
        for (int r = 3; r < 15; r += 2) p = min3p(p, c[r], c[r + 1]);
        return min3p(p, c[15], c[15]);
    };
    // A qualifying row goes to the WAVE's own LDS list first -- its fill count lives in a scalar register, a hit costs a
    // ballot, a population count and a ds_write, no atomic (a returning global atomic per row stalled the wave for a memory
    // round trip: 2x the kernel's time; a returning LDS atomic: +45 %) -- and reaches the global list in bulk when the wave
    // is done, or earlier when a sub-list fills up (flush_sub).
    // The wave's list is four sub-lists, one per query block: the re-rank kernel's waves then read 32 neighbouring queries
    // (for a fixed channel one 128-byte line of the C-major embedding) instead of the wave's 128.
    constexpr int WL = REFINE_LDS_LIST / NW / NQB;  // entries per wave and query block
    uint2 *fl = (uint2 *)(smem + 2 * STEP_BYTES) + wave * (WL * NQB);
    int wl_n[NQB] = {0, 0, 0, 0};  // (wave-uniform)
    int wl_total = 0;              // (statistics)
    // sub-list j of this wave -> its bucket of the global list (block 16 qt + 4 wave + j): one returning atomic reserves the
    // places.  Called when the sub-list cannot take a block's hits (so nothing is dropped here: on spatially smooth
    // embeddings whole regions qualify while the thresholds are still loose) and at the wave's end.
    auto flush_sub = [&](int j) {
        const int cnt = wl_n[j];
        if (cnt == 0) return;  // (wave-uniform)
        // (the bucket's address arithmetic stays HERE, in scalar registers: hipcc otherwise hoists four per-lane 64-bit list
        // addresses + four LDS addresses out of the step loop, 15 VGPRs it can only spill at this kernel's register budget --
        // r3: scratch_load + s_waitcnt vmcnt(0) in the flush path, which drained the LDS-DMA prefetch on every flush)
        int b32 = qt * (QTB / QB) + wave * NQB + j, sub_off = j * WL;
        asm volatile("" : "+s"(b32), "+s"(sub_off));
        const long b = (long)b32;
        unsigned base = 0u;
        if (lane == 0) base = atomicAdd(&bcnt[b], (unsigned)cnt) & 0x7fffffffu;  // (bit 31 = the bucket's "incomplete" mark)
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        uint2 *dst = list + b * bucket_cap + base;  // (wave-uniform)
        const long room = bucket_cap - (long)base;
        for (int i = lane; i < cnt; i += 64) {
            const uint2 e = fl[sub_off + i];  // (this wave's own ds_writes: ordered behind them in the LDS queue)
            if ((long)i < room)
                dst[i] = make_uint2((unsigned)((size_t)(e.x >> 16) * N_pad + (size_t)qt * QTB + (e.x & 0xffffu)), e.y);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the sub-list was read before it is refilled
        wl_n[j] = 0;
        wl_total += cnt;
    };
    auto emit_regs = [&](const f32x16 &c, float t, int j, int row0) __attribute__((always_inline)) {
        const unsigned lq = (unsigned)(wave * (NQB * QB) + l31 + 32 * j);  // query inside the workgroup's 512
        // (four registers at a time first: a block usually has its one or two hits in one group -- 8 tests instead of 16)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            // (the group's minimum is computed here, behind the branch: carrying the four group minima out of the pass's
            // own min16 -- 10 operations instead of 8 in front of the branch -- measured the same)
            const float gm = fminf(min3p(c[4 * g4], c[4 * g4 + 1], c[4 * g4 + 2]), c[4 * g4 + 3]);
            if (!__ballot(gm <= t)) continue;  // wave-uniform
#pragma unroll
            for (int r = 4 * g4; r < 4 * g4 + 4; ++r) {
                const bool hit = c[r] <= t;
                const unsigned long long m = __ballot(hit);
                if (m) {  // wave-uniform: most registers hold no qualifying row for any lane
                    const int slot = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int idx = wl_n[j] + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                    if (hit && idx < WL) fl[j * WL + idx] = make_uint2(((unsigned)o << 16) | lq, (unsigned)slot);
                    wl_n[j] += __popcll(m);
                }
            }
        }
    };
    // The hits of one 32 x 32 block go to sub-list j optimistically (the fast path is the loop above and one scalar compare).
    // If they did not fit behind what the sub-list held, nothing is lost: the sub-list is rolled back to its old fill,
    // flushed to its bucket, and the block is listed again into the empty sub-list.  A block with more hits than a whole
    // sub-list (> 128 of its 1 024 distances inside the threshold: embeddings the bf16 pass cannot tell apart) is listed as
    // ONE dense entry (r4; REFINE_DENSE_CAP per bucket, beyond that the bucket is marked incomplete and the rescue pass --
    // the exact fp32 kernel -- takes that query tile; through r4's first captures every such block went to the rescue pass:
    // 99 % of the tiles of a spatially smooth clip).
    auto emit = [&](const f32x16 &c, float t, int j, int row0, unsigned long long hm) __attribute__((always_inline)) {
        const int before = wl_n[j];
        // hm = the lanes (query, half of the pass's rows) whose 16 distances hold a qualifying one: more than
        // REFINE_DENSE_LANES of the 64 and the block goes dense without looking at single registers (video-like data:
        // neighbouring queries find their rows in the same pass -- the listing of such blocks was the filter pass's tail)
        const bool many = REFINE_DENSE_LANES < 64 && __popcll(hm) > REFINE_DENSE_LANES;
        if (!many) emit_regs(c, t, j, row0);
        if (many || wl_n[j] > WL || wl_n[j] - before > REFINE_DENSE_MIN) {  // (wave-uniform, rare)
            const int total = many ? __popcll(hm) : wl_n[j] - before;
            wl_n[j] = before;
            if (before >= WL || !(many || total > REFINE_DENSE_MIN)) flush_sub(j);  // (room for the dense entry / for the block's rows)
            if (many || total > REFINE_DENSE_MIN) {
                // a DENSE block (embeddings the bf16 pass cannot tell apart over this neighbourhood): one entry for its 1 024
                // distances, into the sub-list that was just emptied; the bucket's dense count lives behind the fill counts
                int b32 = qt * (QTB / QB) + wave * NQB + j, nb32 = (int)(N_pad >> 5);
                asm volatile("" : "+s"(b32), "+s"(nb32));
                if (lane == 0) {
                    if (atomicAdd(&bcnt[(long)nb32 + b32], 1u) >= (unsigned)REFINE_DENSE_CAP)
                        atomicOr(&bcnt[b32], 0x80000000u);  // (bit 31: incomplete -- the rescue pass takes this query tile)
                    fl[j * WL + wl_n[j]] = make_uint2(((unsigned)o << 16) | (unsigned)(wave * (NQB * QB) + 32 * j), REFINE_DENSE_BIT | (unsigned)row0);
                }
                wl_n[j] += 1;
                wl_total += total;  // (statistics: qualifying rows SEEN)
            } else
                emit_regs(c, t, j, row0);
        }
    };

    // this lane's fragment offset inside a tile image: unit (2k + h), row rb * 32 + l31
    const unsigned frag_off = (unsigned)((h * BT + l31) * 16);
    u32x4 F[KSB];
#define MANET_LOADF(k_, pass_base_) F[k_] = *(const u32x4 *)((pass_base_) + frag_off + (size_t)(k_) * (2 * BT * 16));
    // one pass = 32 bank rows x 128 queries: MFMAs of k-step k from F[k], then F[k] <- k-step k of the pass
    // at `next_base` (a tile's second row block is 32 * 16 bytes behind its first inside every unit)
#define MANET_PASS(next_base_, row0_)                                                              \
    {                                                                                              \
        f32x16 c0 = {0}, c1 = {0}, c2 = {0}, c3 = {0};                                             \
        _Pragma("unroll") for (int k = 0; k < KSB; ++k)                                            \
        {                                                                                          \
            MANET_MFMA_E(F[k], q[0][k], c0);                                                         \
            MANET_MFMA_E(F[k], q[1][k], c1);                                                         \
            MANET_MFMA_E(F[k], q[2][k], c2);                                                         \
            MANET_MFMA_E(F[k], q[3][k], c3);                                                         \
            MANET_LOADF(k, next_base_);                                                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); /* 4 MFMA */                        \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); /* the refill right behind them */  \
        }                                                                                          \
        _Pragma("unroll") for (int r = 0; r < 16; r += 4)                                          \
        {                                                                                          \
            ma[0] = min3p(ma[0], c0[r], c0[r + 2]);                                                \
            mb[0] = min3p(mb[0], c0[r + 1], c0[r + 3]);                                            \
            ma[1] = min3p(ma[1], c1[r], c1[r + 2]);                                                \
            mb[1] = min3p(mb[1], c1[r + 1], c1[r + 3]);                                            \
            ma[2] = min3p(ma[2], c2[r], c2[r + 2]);                                                \
            mb[2] = min3p(mb[2], c2[r + 1], c2[r + 3]);                                            \
            ma[3] = min3p(ma[3], c3[r], c3[r + 2]);                                                \
            mb[3] = min3p(mb[3], c3[r + 1], c3[r + 3]);                                            \
        }                                                                                          \
    }

    // FILTER form of a pass: the threshold test of two query blocks runs UNDER the MFMAs of the other two -- the pass is two
    // half-passes (blocks 0,1 then blocks 2,3, KSB k-steps each), and the test of a half's accumulators sits in the basic
    // block of the NEXT half's MFMAs, in front of its (rarely taken) branch to the slow path.  (First form: the test of all
    // four blocks behind the pass's last MFMA, then the branch -- hipcc does not move MFMAs across a branch, so the ~50 VALU
    // instructions of the test ran exposed in every pass: the filter cost +13 % over the plain kernel.)  Accumulators: two
    // accumulate while two are tested, 64 registers as before.  pc2 / pc3 = the pending second half (blocks 2,3 of the
    // previous pass, rows pend_row0..), tested under the next pass's first half; an object change or the end of the split
    // tests it on the spot.
#define MANET_TEST2(ca_, cb_, ja_, jb_, row0_)                                                     \
    {                                                                                              \
        const float pa = min16(ca_), pb = min16(cb_);                                              \
        tq[ja_] = fminf(tq[ja_], pa + sq[ja_]);                                                    \
        tq[jb_] = fminf(tq[jb_], pb + sq[jb_]);                                                    \
        const bool ha = pa <= tq[ja_], hb = pb <= tq[jb_];                                         \
        if (__ballot(ha | hb)) { /* wave-uniform */                                                \
            const unsigned long long ma_ = __ballot(ha), mb_ = __ballot(hb);                       \
            if (ma_) emit(ca_, tq[ja_], ja_, (row0_), ma_);                                        \
            if (mb_) emit(cb_, tq[jb_], jb_, (row0_), mb_);                                        \
        }                                                                                          \
    }
#define MANET_PASS_F(next_base_, row0_)                                                            \
    {                                                                                              \
        f32x16 c0 = {0}, c1 = {0};                                                                 \
        _Pragma("unroll") for (int k = 0; k < KSB; ++k)                                            \
        {                                                                                          \
            MANET_MFMA_E(F[k], q[0][k], c0);                                                         \
            MANET_MFMA_E(F[k], q[1][k], c1);                                                         \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); /* 2 MFMA */                        \
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0); /* a slice of the pending test */   \
        }                                                                                          \
        MANET_TEST2(pc2, pc3, 2, 3, pend_row0);                                                    \
        pc2 = (f32x16){0};                                                                         \
        pc3 = (f32x16){0};                                                                         \
        _Pragma("unroll") for (int k = 0; k < KSB; ++k)                                            \
        {                                                                                          \
            MANET_MFMA_E(F[k], q[2][k], pc2);                                                        \
            MANET_MFMA_E(F[k], q[3][k], pc3);                                                        \
            MANET_LOADF(k, next_base_);                                                            \
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                     \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); /* the refill right behind them */  \
            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                                     \
        }                                                                                          \
        MANET_TEST2(c0, c1, 0, 1, (row0_));                                                        \
        pend_row0 = (row0_);                                                                       \
    }
    unsigned xk[NQB] = {0u, 0u, 0u, 0u};  // FILTER: threshold keys asked for in the previous exchange step, of object xo
    int xo = -1;
    f32x16 pc2, pc3;  // FILTER: the pending half (nothing pending: distances no threshold admits)
    int pend_row0 = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) pc2[r] = pc3[r] = MANET_WRONG_LABEL_PADDING_DISTANCE;
    auto test_pending = [&]() __attribute__((always_inline)) {
        if (FILTER) {
            MANET_TEST2(pc2, pc3, 2, 3, pend_row0);
#pragma unroll
            for (int r = 0; r < 16; ++r) pc2[r] = pc3[r] = MANET_WRONG_LABEL_PADDING_DISTANCE;
        }
    };
    auto next_object = [&](int t) __attribute__((always_inline)) {
        if (t >= seg_end) {  // wave-uniform: tile t starts another object's rows
            test_pending();  // (FILTER: the previous pass's second half still belongs to the old object)
            flush(o);
#pragma unroll
            for (int j = 0; j < NQB; ++j) ma[j] = mb[j] = MANET_WRONG_LABEL_PADDING_DISTANCE;
            do { ++o; seg_end = meta[META_SEG + o + 1]; } while (t >= seg_end);
            if (FILTER) load_thr(o);
        }
    };

    // prologue: steps 0 and 1 in flight; publish step 0, fetch the first pass's fragments
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < KSB; ++k) MANET_LOADF(k, smem);

    int buf = 0;
    for (int t = t0; t < t1; t += TPS, buf ^= 1) {
        const char *cur = smem + (size_t)buf * STEP_BYTES;
        const char *nxt = smem + (size_t)(buf ^ 1) * STEP_BYTES;
        const bool has_b = (t + 1 < t1);
        // ---- tile A: rows 0-31 (refill: A rows 32-63), rows 32-63 (refill: B rows 0-31)
        next_object(t);
        if (FILTER) {
            MANET_PASS_F(cur + 32 * 16, t * BT);
            MANET_PASS_F(cur + TILE_BYTES, t * BT + 32);
        } else {
            MANET_PASS(cur + 32 * 16, t * BT);
            MANET_PASS(cur + TILE_BYTES, t * BT + 32);
        }
        // ---- tile B rows 0-31 (refill: B rows 32-63).  After this pass every fragment of `cur` is in
        // registers.
        if (has_b) {
            next_object(t + 1);
            if (FILTER) {
                MANET_PASS_F(cur + TILE_BYTES + 32 * 16, (t + 1) * BT);
            } else {
                MANET_PASS(cur + TILE_BYTES + 32 * 16, (t + 1) * BT);
            }
        }
        // ---- this wave's pieces of the next step have landed (issued one step ago) and its reads of `cur`
        // have returned; the barrier publishes the next buffer and frees `cur` for step + 2
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (FILTER) {
            // threshold exchange with the workgroups running beside this one on the same queries and object: every fourth
            // step the wave publishes its thresholds (non-returning atomics) and ASKS for the published ones; the answer is
            // taken one step later, right here behind the step's vmcnt(0) -- the loads never stall the wave (first form:
            // load and use in one place, a memory round trip exposed per exchange).
            if (xo == o) {
#pragma unroll
                for (int j = 0; j < NQB; ++j) {
                    tq[j] = fminf(tq[j], float_of(xk[j]));
                    if (h == 0 && xk[j] < pks[64 * j]) pks[64 * j] = xk[j];
                }
            }
            xo = -1;
            if ((((t - t0) / TPS) & REFINE_XCHG_MASK) == REFINE_XCHG_MASK) {
                flush(o);
                xo = o;
#pragma unroll
                for (int j = 0; j < NQB; ++j) xk[j] = (thr + (size_t)o * N_pad)[qbase + 32u * j];
            }
        }
        if (t + 2 * TPS < t1) stage_dma(t + 2 * TPS, buf);
        // ---- tile B rows 32-63 (refill: first pass of the next step; a stale read if there is none)
        if (has_b) {
            if (FILTER) {
                MANET_PASS_F(nxt, (t + 1) * BT + 32);
            } else {
                MANET_PASS(nxt, (t + 1) * BT + 32);
            }
        }
    }
    // (the fp16 filter: the lane's query column of the closing test is taken from the lane id again, not carried through the
    // step loop -- there every register is taken, and global_match_bf16_wide_kernel<7, true> spills exactly this value around it)
    if constexpr (FILTER && std::is_same<E, ElemF16>::value) l31 = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 31;
    test_pending();
#undef MANET_PASS
#undef MANET_PASS_F
#undef MANET_TEST2
#undef MANET_LOADF
    flush(o);
    if (FILTER) {
        // the wave's remaining candidates -> the global list, which is one BUCKET per 32-query block (flush_sub).  The
        // re-rank kernel runs one workgroup per bucket with the block's 32 query vectors in LDS.  A bucket that outgrows its
        // capacity keeps counting (bcnt > bucket_cap marks it) and the rescue pass takes that query tile.
#pragma unroll
        for (int j = 0; j < NQB; ++j) flush_sub(j);
        if (lane == 0 && wl_total) atomicAdd(&stats[0], (unsigned long long)wl_total);  // (statistics only)
    }
}
template <int KSB, bool FILTER = false>
__global__ __launch_bounds__(256, 2) void global_match_bf16_wide_kernel(const char *__restrict__ qpack,
                                                                        const char *__restrict__ bpack,
                                                                        const int *__restrict__ meta, int n_ids,
                                                                        int nQT, int S, long N_pad,
                                                                        unsigned *__restrict__ keys, int block_map,
                                                                        unsigned *__restrict__ thr,
                                                                        const float *__restrict__ slack,
                                                                        unsigned long long *__restrict__ stats,
                                                                        uint2 *__restrict__ list, long bucket_cap,
                                                                        unsigned *__restrict__ bcnt)
{
    plain_wide_body<KSB, FILTER, ElemBF16>(qpack, bpack, meta, n_ids, nQT, S, N_pad, keys, block_map, thr, slack, stats, list,
                                           bucket_cap, bcnt);
}
// MANET_COMPUTE_F16, C <= 106, and the pre-pass of MANET_COMPUTE_F16_REFINE: the plain form (the filter form: refine_filter_half_kernel)
template <int KSB>
__global__ __launch_bounds__(256, 2) void f16_match_wide_kernel(const char *__restrict__ qpack, const char *__restrict__ bpack,
                                                                const int *__restrict__ meta, int n_ids, int nQT, int S, long N_pad,
                                                                unsigned *__restrict__ keys, int block_map)
{
    plain_wide_body<KSB, false, ElemF16>(qpack, bpack, meta, n_ids, nQT, S, N_pad, keys, block_map, nullptr, nullptr, nullptr, nullptr,
                                         0L, nullptr);
}
// MANET_COMPUTE_F16_REFINE: the FILTER form on fp16 images, with global_match_bf16_wide_kernel<KSB, true>'s arguments.  The body
// has one fp16-only line (the closing test's lane column, a register matter); what differs from bf16 in VALUES is met as it stands:
//   * a tile's padding rows give +inf, not 1e20: a pass of padding alone has the minimum +inf, which tightens nothing
//     (fminf(tq, inf + slack) = tq) and is below no threshold (thresholds of in-domain pairs are finite);
//   * a row outside fp16's domain (bank or query) gives NaN distances: min3p carries a NaN into the pass's minimum, fminf drops it
//     from the tightening, `NaN <= tq` lists nothing -- the NaN may HIDE the other 15 rows of its lane's pass, so every pair such
//     a row takes part in must reach the exact route.  refine_threshold_f16_kernel (csrc/global_refine.hip) marks the query
//     blocks of out-of-domain queries incomplete; out-of-domain BANK rows (META_F16_OOD) concern every query, all tiles are
//     rescued, and nothing this kernel could list would be read: it returns at once.
template <int KSB>
__global__ __launch_bounds__(256, 2) void refine_filter_half_kernel(const char *__restrict__ qpack, const char *__restrict__ bpack,
                                                                    const int *__restrict__ meta, int n_ids, int nQT, int S,
                                                                    long N_pad, unsigned *__restrict__ keys, int block_map,
                                                                    unsigned *__restrict__ thr, const float *__restrict__ slack,
                                                                    unsigned long long *__restrict__ stats,
                                                                    uint2 *__restrict__ list, long bucket_cap,
                                                                    unsigned *__restrict__ bcnt)
{
    if (meta[META_F16_OOD]) return;  // (uniform)
    plain_wide_body<KSB, true, ElemF16>(qpack, bpack, meta, n_ids, nQT, S, N_pad, keys, block_map, thr, slack, stats, list,
                                        bucket_cap, bcnt);
}

#undef MANET_MFMA
#undef MANET_MFMA_E
#undef MANET_HF
#undef MANET_BF


// decode + (sigmoid-0.5)*2 (IntVOS.py:611-612) + min-merge with the stored map (IntVOS.py:620-622)
// MANET_EPI_KEYS_ARMED: the keys are put back to "no candidate" as they are read (every key, padding rows included), so
// the next armed call on the same match workspace needs no fill launch
__global__ void global_finish_kernel(unsigned *__restrict__ keys, long N, long N_pad, int n_ids,
                                     int flags, float *__restrict__ out, float *__restrict__ mem)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((flags & MANET_EPI_KEYS_ARMED) && i >= N * n_ids && i < N_pad * n_ids) {
        const long j = i - N * n_ids;  // the padding rows' keys: n = N + j / n_ids
        keys[(size_t)(j % n_ids) * N_pad + N + j / n_ids] = 0xffffffffu;
    }
    if (i >= N * n_ids) return;
    long n = i / n_ids;
    int o = (int)(i - n * n_ids);
    unsigned k = keys[(size_t)o * N_pad + n];
    if (flags & MANET_EPI_KEYS_ARMED) keys[(size_t)o * N_pad + n] = 0xffffffffu;
    // an object with no bank row keeps the initial key: padding distance (IntVOS.py:81-83)
    float g = (k == 0xffffffffu) ? MANET_WRONG_LABEL_PADDING_DISTANCE : float_of(k);
    if (flags & MANET_EPI_NORMALIZE) g = manet_normalize_dist(g);
    if (mem) {
        float mv = mem[i];
        g = (g <= mv) ? g : mv;
        mem[i] = g;
    }
    out[i] = g;
}

// top-k epilogue (IntVOS.py:87-94): merge the splits' lists, keep the k smallest; entries >= 1e20
// are the reference's masked rows (here: tile padding rows / missing rows): replaced by
// pad = max(valid distances, and 0 if any entry is invalid) -- `dists * valid_mask` zeroes them
// before the max -- then the mean.  Then the same normalise / merge as the k=1 path.
__global__ void global_finish_topk_kernel(const float *__restrict__ topk, int S, int k_nn, long N, long N_pad,
                                          int n_ids, int flags, float *__restrict__ out,
                                          float *__restrict__ mem)
{
    constexpr int K = MANET_MAX_KNN;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * n_ids) return;
    long n = i / n_ids;
    int o = (int)(i - n * n_ids);
    float best[K];
#pragma unroll
    for (int j = 0; j < K; ++j) best[j] = INFINITY;
    for (int sp = 0; sp < S; ++sp) {
        const float *p = topk + (((size_t)sp * n_ids + o) * N_pad + n) * K;
#pragma unroll
        for (int j = 0; j < K; ++j) topk_insert<K>(best, p[j]);
    }
    float pad = -INFINITY, sum = 0.0f;
    bool any_invalid = false;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k_nn) {
            if (best[j] < MANET_WRONG_LABEL_PADDING_DISTANCE) pad = fmaxf(pad, best[j]);
            else any_invalid = true;
        }
    if (any_invalid) pad = fmaxf(pad, 0.0f);
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k_nn) sum += (best[j] < MANET_WRONG_LABEL_PADDING_DISTANCE) ? best[j] : pad;
    float g = sum / (float)k_nn;
    if (flags & MANET_EPI_NORMALIZE) g = manet_normalize_dist(g);
    if (mem) {
        float mv = mem[i];
        g = (g <= mv) ? g : mv;
        mem[i] = g;
    }
    out[i] = g;
}

__global__ void normalize_merge_kernel(float *__restrict__ x, float *__restrict__ mem, long n,
                                       int normalize)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float g = x[i];
    if (normalize) g = manet_normalize_dist(g);
    if (mem) {
        float mv = mem[i];
        g = (g <= mv) ? g : mv;
        mem[i] = g;
    }
    x[i] = g;
}

// arg-min form: decode (distance key, bank slot) -> raw distance + source row of the caller's bank (-1: no row)
__global__ void global_finish_arg_kernel(const unsigned long long *__restrict__ keys64, const int *__restrict__ src_of,
                                         const int *__restrict__ meta, long N, long N_pad, int n_ids,
                                         float *__restrict__ out, int *__restrict__ arg)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * n_ids) return;
    long n = i / n_ids;
    int o = (int)(i - n * n_ids);
    const unsigned long long k = keys64[(size_t)o * N_pad + n];
    const unsigned hi = (unsigned)(k >> 32), slot = (unsigned)k;
    out[i] = (k == ~0ull) ? MANET_WRONG_LABEL_PADDING_DISTANCE : float_of(hi);
    arg[i] = (slot != 0xffffffffu && (long)slot < (long)meta[META_T] * BT) ? src_of[slot] : -1;
}

// Backward of the k = 1 global match w.r.t. both embeddings (reference: autograd through IntVOS.py:32-39 and the
// torch.min of :84): with m* = arg[n][o] and g = grad_out[n][o],
//   d/dq_n += 2 g (q_n - k_m*),   d/dk_m* += 2 g (k_m* - q_n)       (d = |q|^2 + |k|^2 - 2 q.k)
// thread = (query n, channel c), lanes along n; grad_bank is accumulated with atomicAdd (zeroed by the caller side
// of this entry point).  Element strides for every tensor.
__global__ void global_match_backward_kernel(const float *__restrict__ q, long q_sn, long q_sc,
                                             const float *__restrict__ k, long k_sm, long k_sc,
                                             const int *__restrict__ arg, const float *__restrict__ gout, long N,
                                             int C, int n_ids, float *__restrict__ gq, long gq_sn, long gq_sc,
                                             float *__restrict__ gk, long gk_sm, long gk_sc)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * C) return;
    const long n = i % N;
    const int c = (int)(i / N);
    const float qv = q[n * q_sn + (long)c * q_sc];
    float acc = 0.0f;
    for (int o = 0; o < n_ids; ++o) {
        const int m = arg[n * n_ids + o];
        const float g = gout[n * n_ids + o];
        if (m < 0 || g == 0.0f) continue;
        const float t = 2.0f * g * (qv - k[(long)m * k_sm + (long)c * k_sc]);
        acc += t;
        if (gk) atomicAdd(gk + (long)m * gk_sm + (long)c * gk_sc, -t);  // (NULL: the bank needs no gradient)
    }
    if (gq) gq[n * gq_sn + (long)c * gq_sc] = acc;
}

__global__ void zero_strided_kernel(float *__restrict__ p, long n0, long n1, long s0, long s1)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n0 * n1) return;
    p[(i % n0) * s0 + (i / n0) * s1] = 0.0f;
}

// ---------------------------------------------------------------------------------------------
}  // namespace

// The one launcher of the main kernels: the kernel follows from the plan's form, arithmetic and k-step count, the cut (grid,
// splits, block_map word, LDS bytes) is the plan's.  Bracketed for manet_profile_begin / _end (channel 0; the pre-pass: 3; the
// rescue: by its caller).  The LDS attribute is set per call (cheap, host side): it is per device and the library keeps no state.
//   plain bf16 -> global_match_bf16_wide_kernel (k-steps 2 / 7), global_match_bf16_pipe_kernel for C > 106 (k-step 9: its
//   144 operand VGPRs do not fit the wide form; MANET_COMPUTE_BF16_REFINE supports C <= 106); split-bf16 -> the x3 kernel;
//   MANET_COMPUTE_F16 -> the fp16 wrappers of the same two bodies, f16_match_wide_kernel<2 / 7> and f16_match_pipe_kernel<9>;
//   MANET_COMPUTE_F16_REFINE -> f16_match_wide_kernel (pre-pass) and refine_filter_half_kernel (filter), k-steps 2 / 7
void launch_match(const MatchPlan &P, const MatchArgs &A, hipStream_t st)
{
    const bool rescue = P.form == MATCH_FORM_REFINE_RESCUE || P.form == MATCH_FORM_REFINE_RESCUE_EXACT;
    const int chan = rescue ? -1 : (P.form == MATCH_FORM_REFINE_PRE ? 3 : 0);
    auto go = [&](auto kernel, int threads, auto... rest) {  // rest: the kernel's arguments behind N_pad
        (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds);
        if (chan >= 0) manet_profile_record(st, true, chan);
        hipLaunchKernelGGL(kernel, dim3(P.grid), dim3(threads), P.lds, st, A.qpack, A.bpack, A.meta, A.n_ids, P.nQT, P.S, A.N_pad,
                           rest...);
        if (chan >= 0) manet_profile_record(st, false, chan);
    };
    if (rescue || P.compute == MANET_COMPUTE_F32) {
        with_ks(P.steps, [&](auto k) {
            constexpr int KS = decltype(k)::value;
            if (rescue) go(global_match_f32_pipe_kernel<KS, true>, 256, A.keys, P.block_map, A.bcnt, A.bucket_cap);
            else if (P.form == MATCH_FORM_ARG) go(global_match_f32_kernel<KS, 1, true, false>, 256, A.keys, A.topk, P.block_map);
            else if (P.form == MATCH_FORM_NTH_ARG) go(global_match_f32_kernel<KS, 1, true, true>, 256, A.keys, A.topk, P.block_map);
            else if (P.k_nn > 1) go(global_match_f32_kernel<KS, MANET_MAX_KNN, false, false>, 256, A.keys, A.topk, P.block_map);
            else go(global_match_f32_pipe_kernel<KS, false>, 256, A.keys, P.block_map, nullptr, 0L);
        });
    } else {
        with_ksb(P.steps, [&](auto k) {
            constexpr int K = decltype(k)::value;
            if (P.compute == MANET_COMPUTE_BF16X3) go(global_match_bf16x3_kernel<K>, 512, A.keys, P.block_map);
            else if (P.compute == MANET_COMPUTE_F16) {  // (k-step 9 -- C > 106 -- takes the narrow form, as plain bf16)
                if constexpr (K == 9) go(f16_match_pipe_kernel<K>, 512, A.keys, P.block_map);
                else go(f16_match_wide_kernel<K>, 256, A.keys, P.block_map);
            }
            else if (P.compute == MANET_COMPUTE_F16_REFINE) {  // (C <= 106: check_common; the pre-pass is the plain fp16 kernel)
                if constexpr (K == 9) return;
                else if (P.form == MATCH_FORM_REFINE_FILTER)
                    go(refine_filter_half_kernel<K>, 256, A.keys, P.block_map, A.thr, A.slack, A.stats, A.list, A.bucket_cap, A.bcnt);
                else go(f16_match_wide_kernel<K>, 256, A.keys, P.block_map);
            }
            else if constexpr (K == 9) go(global_match_bf16_pipe_kernel<K>, 512, A.keys, P.block_map);
            else if (P.form == MATCH_FORM_REFINE_FILTER)
                go(global_match_bf16_wide_kernel<K, true>, 256, A.keys, P.block_map, A.thr, A.slack, A.stats, A.list, A.bucket_cap, A.bcnt);
            else  // (the FILTER form's six arguments are unused here)
                go(global_match_bf16_wide_kernel<K, false>, 256, A.keys, P.block_map, nullptr, nullptr, nullptr, nullptr, 0L, nullptr);
        });
    }
}

void launch_global_finish(unsigned *keys, long N, long N_pad, int n_ids, int flags, float *out, float *mem, long total,
                          hipStream_t st)
{
    hipLaunchKernelGGL(global_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, keys, N, N_pad, n_ids, flags,
                       out, mem);
}

extern "C" {

int manet_match_workspace_bytes(int64_t N, int64_t M0, int C, int n_ids, int k_nn, int compute,
                                size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = check_common(N, M0, C, n_ids, k_nn, compute);
    if (rc) return rc;
    *bytes = match_layout(N, C, n_ids, compute, k_nn).total;
    return MANET_OK;
}

int manet_global_match_workspace_bytes(int64_t N, int64_t M0, int C, int n_ids, int k_nn, int compute,
                                       size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = check_common(N, M0, C, n_ids, k_nn, compute);
    if (rc) return rc;
    *bytes = bank_layout(M0, C, n_ids, compute).total + match_layout(N, C, n_ids, compute, k_nn).total;
    return MANET_OK;
}

int manet_global_match_prepared(const float *query, int64_t q_stride_n, int64_t q_stride_c,
                                const void *bank_ws, int64_t N, int64_t M0, int C, int n_ids, int k_nn,
                                int compute, float *out, float *mem_inout, int epilogue_flags,
                                void *match_ws, size_t match_ws_bytes, manet_stream_t stream)
{
    return manet_global_match_prepared_ex(query, MANET_EMB_F32, q_stride_n, q_stride_c, bank_ws, N, M0, C, n_ids, k_nn,
                                          compute, out, mem_inout, epilogue_flags, match_ws, match_ws_bytes, stream);
}

int manet_global_match_prepared_ex(const void *query, int emb_dtype, int64_t q_stride_n, int64_t q_stride_c,
                                   const void *bank_ws, int64_t N, int64_t M0, int C, int n_ids, int k_nn,
                                   int compute, float *out, float *mem_inout, int epilogue_flags,
                                   void *match_ws, size_t match_ws_bytes, manet_stream_t stream)
{
    int rc = check_common(N, M0, C, n_ids, k_nn, compute);
    if (rc) return rc;
    if (!query || !bank_ws || !out || !match_ws) return manet_set_error(MANET_E_INVALID, "null pointer");
    BankLayout BL = bank_layout(M0, C, n_ids, compute);
    MatchLayout ML = match_layout(N, C, n_ids, compute, k_nn);
    if (match_ws_bytes < ML.total)
        return manet_set_error(MANET_E_WORKSPACE, "match workspace %zu < %zu bytes", match_ws_bytes, ML.total);
    hipStream_t st = (hipStream_t)stream;
    const char *bws = (const char *)bank_ws;
    char *mws = (char *)match_ws;
    const int *meta = (const int *)(bws + BL.off_meta);
    unsigned *keys = (unsigned *)(mws + ML.off_keys);
    // MANET_EMB_PACKED: `query` already is the operand image manet_query_pack / manet_frame_prepare wrote (same N, C,
    // compute)
    const char *qpack = (const char *)query;
    const bool armed = (epilogue_flags & MANET_EPI_KEYS_ARMED) && k_nn == 1;
    if (!armed) epilogue_flags &= ~MANET_EPI_KEYS_ARMED;
    if (emb_dtype != MANET_EMB_PACKED) {
        rc = launch_query_pack(query, emb_dtype, (long)q_stride_n, (long)q_stride_c, (long)N, ML.N_pad, C, ML.G,
                               mws + ML.off_q, keys, n_ids, st);  // also resets the keys
        if (rc) return rc;
        qpack = mws + ML.off_q;
    } else if (!armed) {
        fill32(keys, 0xffffffffu, (size_t)n_ids * ML.N_pad, st);
    }
    if (is_refine(compute)) {
        if (emb_dtype == MANET_EMB_PACKED)
            return manet_set_error(MANET_E_INVALID, "MANET_COMPUTE_%s_REFINE re-ranks in fp32 from the query as stored: pass "
                                                    "it to manet_global_match_refine next to its packed image",
                                   compute == MANET_COMPUTE_F16_REFINE ? "F16" : "BF16");
        return run_refine(compute, qpack, query, emb_dtype, (long)q_stride_n, (long)q_stride_c, bws, BL, mws, ML, (long)N, M0, C, n_ids, out,
                          mem_inout, epilogue_flags, st);
    }
    const char *bpack = bws + BL.off_pack;
    float *topk = (float *)(mws + ML.off_topk);
    if (k_nn > 1) {
        // splits that own no tile never write their lists: start from "no candidate"
        size_t words = (size_t)TOPK_SPLITS * n_ids * ML.N_pad * MANET_MAX_KNN;
        fill32(topk, 0x7f7f7f7fu, words, st);  // 3.39e38 >= 1e20: invalid
    }
    const MatchPlan P = match_plan(N, M0, C, n_ids, k_nn, compute, MATCH_FORM_MAIN, match_tune());
    launch_match(P, {qpack, bpack, meta, n_ids, ML.N_pad, keys, topk}, st);
    long total = (long)(armed ? ML.N_pad : N) * n_ids;
    if (k_nn == 1)
        launch_global_finish(keys, (long)N, ML.N_pad, n_ids, epilogue_flags, out, mem_inout, total, st);
    else
        hipLaunchKernelGGL(global_finish_topk_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           (const float *)topk, P.S, k_nn, (long)N, ML.N_pad, n_ids, epilogue_flags, out, mem_inout);
    return manet_check_launch("manet_global_match_prepared");
}

int manet_global_match(const float *query, int64_t q_stride_n, int64_t q_stride_c, const float *bank,
                       int64_t b_stride_m, int64_t b_stride_c, const int32_t *labels, int64_t N, int64_t M0,
                       int C, int n_ids, int k_nn, int compute, float *out, float *mem_inout,
                       int epilogue_flags, void *workspace, size_t workspace_bytes, manet_stream_t stream)
{
    return manet_global_match_ex(query, MANET_EMB_F32, q_stride_n, q_stride_c, bank, MANET_EMB_F32, b_stride_m, b_stride_c,
                                 labels, N, M0, C, n_ids, k_nn, compute, out, mem_inout, epilogue_flags, workspace,
                                 workspace_bytes, stream);
}

int manet_global_match_ex(const void *query, int q_dtype, int64_t q_stride_n, int64_t q_stride_c, const void *bank,
                          int b_dtype, int64_t b_stride_m, int64_t b_stride_c, const int32_t *labels, int64_t N,
                          int64_t M0, int C, int n_ids, int k_nn, int compute, float *out, float *mem_inout,
                          int epilogue_flags, void *workspace, size_t workspace_bytes, manet_stream_t stream)
{
    int rc = check_common(N, M0, C, n_ids, k_nn, compute);
    if (rc) return rc;
    if (!workspace) return manet_set_error(MANET_E_INVALID, "workspace == NULL");
    size_t bbytes = bank_layout(M0, C, n_ids, compute).total;
    size_t mbytes = match_layout(N, C, n_ids, compute, k_nn).total;
    if (workspace_bytes < bbytes + mbytes)
        return manet_set_error(MANET_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, bbytes + mbytes);
    char *ws = (char *)workspace;
    rc = manet_bank_prepare_ex(bank, b_dtype, b_stride_m, b_stride_c, labels, M0, C, n_ids, compute, ws, bbytes, stream);
    if (rc) return rc;
    return manet_global_match_prepared_ex(query, q_dtype, q_stride_n, q_stride_c, ws, N, M0, C, n_ids, k_nn, compute, out,
                                          mem_inout, epilogue_flags, ws + bbytes, mbytes, stream);
}

int manet_global_match_arg_workspace_bytes(int64_t N, int64_t M0, int C, int n_ids, size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = check_common(N, M0, C, n_ids, 1, MANET_COMPUTE_F32);
    if (rc) return rc;
    *bytes = bank_layout(M0, C, n_ids, MANET_COMPUTE_F32).total + match_layout(N, C, n_ids, MANET_COMPUTE_F32, 1, true).total;
    return MANET_OK;
}

int manet_global_match_arg_f32(const float *query, int64_t q_stride_n, int64_t q_stride_c, const float *bank,
                               int64_t b_stride_m, int64_t b_stride_c, const int32_t *labels, int64_t N, int64_t M0,
                               int C, int n_ids, float *out, int32_t *arg_out, void *workspace, size_t workspace_bytes,
                               manet_stream_t stream)
{
    const int compute = MANET_COMPUTE_F32;
    int rc = check_common(N, M0, C, n_ids, 1, compute);
    if (rc) return rc;
    if (!query || !out || !arg_out || !workspace) return manet_set_error(MANET_E_INVALID, "null pointer");
    BankLayout BL = bank_layout(M0, C, n_ids, compute);
    MatchLayout ML = match_layout(N, C, n_ids, compute, 1, true);
    if (workspace_bytes < BL.total + ML.total)
        return manet_set_error(MANET_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, BL.total + ML.total);
    char *bws = (char *)workspace, *mws = bws + BL.total;
    rc = manet_bank_prepare(bank, b_stride_m, b_stride_c, labels, M0, C, n_ids, compute, bws, BL.total, stream);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int *meta = (const int *)(bws + BL.off_meta);
    unsigned long long *keys64 = (unsigned long long *)(mws + ML.off_topk);
    fill32(keys64, 0xffffffffu, (size_t)2 * n_ids * ML.N_pad, st);
    rc = launch_query_pack(query, MANET_EMB_F32, (long)q_stride_n, (long)q_stride_c, (long)N, ML.N_pad, C, ML.G,
                           mws + ML.off_q, nullptr, 0, st);
    if (rc) return rc;
    unsigned *keys = (unsigned *)(mws + ML.off_keys);
    launch_match(match_plan(N, M0, C, n_ids, 1, compute, MATCH_FORM_ARG, match_tune()),
                 {mws + ML.off_q, bws + BL.off_pack, meta, n_ids, ML.N_pad, keys, (float *)keys64}, st);
    long total = (long)N * n_ids;
    hipLaunchKernelGGL(global_finish_arg_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       (const unsigned long long *)keys64, (const int *)(bws + BL.off_src), meta, (long)N, ML.N_pad, n_ids,
                       out, arg_out);
    return manet_check_launch("manet_global_match_arg_f32");
}

/* k_nn nearest rows per (query, object), with their row numbers: the forward of the TRAINING path of k_nearest_neighbors > 1
 * (IntVOS.py:87-94; manet_hip.h).  k_nn passes of the arg-min kernel, pass j bounded from below by pass j - 1's (distance key,
 * slot) pair: exact, ascending, ties ordered by bank slot.  out / arg_out: [k_nn][N][n_ids]; beyond an object's row count the
 * distance is the padding value 1e20 and the row -1. */
int manet_global_match_topk_arg_workspace_bytes(int64_t N, int64_t M0, int C, int n_ids, size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = check_common(N, M0, C, n_ids, 1, MANET_COMPUTE_F32);
    if (rc) return rc;
    MatchLayout ML = match_layout(N, C, n_ids, MANET_COMPUTE_F32, 1, true);
    *bytes = bank_layout(M0, C, n_ids, MANET_COMPUTE_F32).total + ML.total +
             manet_align_up((size_t)n_ids * ML.N_pad * sizeof(unsigned long long), 1024);
    return MANET_OK;
}

int manet_global_match_topk_arg_f32(const float *query, int64_t q_stride_n, int64_t q_stride_c, const float *bank,
                                    int64_t b_stride_m, int64_t b_stride_c, const int32_t *labels, int64_t N, int64_t M0,
                                    int C, int n_ids, int k_nn, float *out, int32_t *arg_out, void *workspace,
                                    size_t workspace_bytes, manet_stream_t stream)
{
    const int compute = MANET_COMPUTE_F32;
    int rc = check_common(N, M0, C, n_ids, k_nn, compute);
    if (rc) return rc;
    if (!query || !out || !arg_out || !workspace) return manet_set_error(MANET_E_INVALID, "null pointer");
    BankLayout BL = bank_layout(M0, C, n_ids, compute);
    MatchLayout ML = match_layout(N, C, n_ids, compute, 1, true);
    const size_t kbytes = manet_align_up((size_t)n_ids * ML.N_pad * sizeof(unsigned long long), 1024);
    if (workspace_bytes < BL.total + ML.total + kbytes)
        return manet_set_error(MANET_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, BL.total + ML.total + kbytes);
    char *bws = (char *)workspace, *mws = bws + BL.total;
    rc = manet_bank_prepare(bank, b_stride_m, b_stride_c, labels, M0, C, n_ids, compute, bws, BL.total, stream);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int *meta = (const int *)(bws + BL.off_meta);
    unsigned long long *kbuf[2] = {(unsigned long long *)(mws + ML.off_topk), (unsigned long long *)(mws + ML.total)};
    rc = launch_query_pack(query, MANET_EMB_F32, (long)q_stride_n, (long)q_stride_c, (long)N, ML.N_pad, C, ML.G,
                           mws + ML.off_q, nullptr, 0, st);
    if (rc) return rc;
    const MatchPlan P = match_plan(N, M0, C, n_ids, 1, compute, MATCH_FORM_NTH_ARG, match_tune());
    const long total = (long)N * n_ids;
    for (int j = 0; j < k_nn; ++j) {
        unsigned long long *cur = kbuf[j & 1], *prev = kbuf[(j & 1) ^ 1];
        fill32(cur, 0xffffffffu, (size_t)2 * n_ids * ML.N_pad, st);
        if (j == 0) fill32(prev, 0u, (size_t)2 * n_ids * ML.N_pad, st);  // bound 0: every real pair qualifies
        // (the bounded form reads the previous pass's pairs through `keys`)
        launch_match(P, {mws + ML.off_q, bws + BL.off_pack, meta, n_ids, ML.N_pad, (unsigned *)prev, (float *)cur}, st);
        hipLaunchKernelGGL(global_finish_arg_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                           (const unsigned long long *)cur, (const int *)(bws + BL.off_src), meta, (long)N, ML.N_pad, n_ids,
                           out + (size_t)j * total, arg_out + (size_t)j * total);
    }
    return manet_check_launch("manet_global_match_topk_arg_f32");
}

int manet_global_match_backward_f32(const float *query, int64_t q_stride_n, int64_t q_stride_c, const float *bank,
                                    int64_t b_stride_m, int64_t b_stride_c, const int32_t *arg, const float *grad_out,
                                    int64_t N, int64_t M0, int C, int n_ids, float *grad_query, int64_t gq_stride_n,
                                    int64_t gq_stride_c, float *grad_bank, int64_t gb_stride_m, int64_t gb_stride_c,
                                    manet_stream_t stream)
{
    int rc = check_common(N, M0, C, n_ids, 1, MANET_COMPUTE_F32);
    if (rc) return rc;
    if (!query || !arg || !grad_out || (!grad_query && !grad_bank) || (M0 > 0 && !bank))
        return manet_set_error(MANET_E_INVALID, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (M0 > 0 && grad_bank) {
        long tb = (long)M0 * C;
        hipLaunchKernelGGL(zero_strided_kernel, dim3((unsigned)((tb + 255) / 256)), dim3(256), 0, st, grad_bank, (long)M0,
                           (long)C, (long)gb_stride_m, (long)gb_stride_c);
    }
    long tq = (long)N * C;
    hipLaunchKernelGGL(global_match_backward_kernel, dim3((unsigned)((tq + 255) / 256)), dim3(256), 0, st, query,
                       (long)q_stride_n, (long)q_stride_c, bank, (long)b_stride_m, (long)b_stride_c, arg, grad_out, (long)N, C,
                       n_ids, grad_query, (long)gq_stride_n, (long)gq_stride_c, grad_bank, (long)gb_stride_m,
                       (long)gb_stride_c);
    return manet_check_launch("manet_global_match_backward_f32");
}

int manet_normalize_merge_f32(float *x, float *mem_inout, int64_t n, int normalize, manet_stream_t stream)
{
    if (n < 0 || (n > 0 && !x)) return manet_set_error(MANET_E_INVALID, "bad arguments");
    if (n == 0) return MANET_OK;
    hipLaunchKernelGGL(normalize_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       x, mem_inout, (long)n, normalize);
    return manet_check_launch("manet_normalize_merge_f32");
}

}  // extern "C"
