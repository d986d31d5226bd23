// Global nearest-neighbour matching, stage 1: the operands (the image: Geom, csrc/global_match_common.h).
//   * bank rows are SORTED BY OBJECT ID in a pre-pass (counting sort; rows whose label is not an object id are dropped,
//     which is what the reference's pixel selection / 1e20 mask amounts to).  Every 64-row bank tile then belongs to one
//     object: no per-element label compare in the match, and work shrinks with the number of labelled pixels.
//   * the pre-pass writes the bank in the exact LDS image the MFMA loop wants ([16-byte unit][row][4 floats | 8 bf16],
//     conflict-free ds_read_b128) so a tile is staged by linear, fully coalesced 16-byte loads.
//   * the query side: pack_rows_kernel<32, 32> for a query as stored, frame_prepare_kernel for a frame of the propagation loop.
#include "global_match_common.h"
#include "local_geom.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Bank pre-pass = a stable counting sort of the rows by object id, without global atomics
// (deterministic packing order):
//   label_hist_kernel      per block of 256 rows: rows per object            -> hist[block][o]
//   label_scan_kernel      one wave per object: exclusive prefix over blocks -> base[block][o], cnt[o]
//   label_segments_kernel  tile range of every object (rows padded to whole 64-row tiles)
//   label_scatter_kernel   slot of row i = seg_start[o]*64 + base[block][o] + rank inside the block
//   pack_rows_kernel       gather + transpose the rows into the MFMA operand image
// A row counts for object o iff label == o (IntVOS.py:137); other labels (-1 = unlabelled) are
// dropped, which is what _selected_pixel (:100-109) / the 1e20 mask (:81-83) amount to for a minimum.
constexpr int RPB = 256;  // rows per pre-pass block

__global__ __launch_bounds__(RPB) void label_hist_kernel(const int *__restrict__ labels, long M0, int n_ids,
                                                         int *__restrict__ hist)
{
    __shared__ int h[MANET_MAX_IDS];
    if (threadIdx.x < MANET_MAX_IDS) h[threadIdx.x] = 0;
    __syncthreads();
    long i = (long)blockIdx.x * RPB + threadIdx.x;
    if (i < M0) {
        int lab = labels[i];
        if (lab >= 0 && lab < n_ids) atomicAdd(&h[lab], 1);  // LDS atomic
    }
    __syncthreads();
    if (threadIdx.x < n_ids) hist[(long)blockIdx.x * n_ids + threadIdx.x] = h[threadIdx.x];
}

// grid = n_ids blocks of one wave: exclusive prefix of hist[:, o] over the blocks, in place
__global__ __launch_bounds__(64) void label_scan_kernel(int *__restrict__ hist, int nblocks, int n_ids,
                                                        int *__restrict__ meta)
{
    const int o = blockIdx.x, lane = threadIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < nblocks; b0 += 64) {
        int b = b0 + lane;
        int v = (b < nblocks) ? hist[(long)b * n_ids + o] : 0;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (b < nblocks) hist[(long)b * n_ids + o] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) meta[META_CNT + o] = carry;
}

__global__ void label_segments_kernel(int n_ids, int *meta)
{
    if (threadIdx.x == 0) {
        int t = 0;
        for (int o = 0; o < n_ids; ++o) {
            meta[META_SEG + o] = t;
            t += (meta[META_CNT + o] + BT - 1) / BT;
        }
        meta[META_SEG + n_ids] = t;
        meta[META_T] = t;
    }
}

// slot -> source row map (slots not hit stay -1 = padding row)
__global__ __launch_bounds__(RPB) void label_scatter_kernel(const int *__restrict__ labels, long M0, int n_ids,
                                                            const int *__restrict__ base,
                                                            const int *__restrict__ meta,
                                                            int *__restrict__ src_of)
{
    __shared__ int wcnt[RPB / 64][MANET_MAX_IDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = threadIdx.x; j < (RPB / 64) * MANET_MAX_IDS; j += RPB) (&wcnt[0][0])[j] = 0;
    __syncthreads();
    const long i = (long)blockIdx.x * RPB + threadIdx.x;
    const int lab = (i < M0) ? labels[i] : -1;
    const bool valid = (lab >= 0 && lab < n_ids);
    bool active = valid;
    int rank = 0;
    while (true) {  // ranks inside the wave from ballots, one pass per object present in the wave
        unsigned long long pending = __ballot(active);
        if (!pending) break;
        int leader = __ffsll((long long)pending) - 1;
        int L = __shfl(lab, leader);
        bool mine = active && (lab == L);
        unsigned long long mm = __ballot(mine);
        if (mine) {
            rank = __popcll(mm & ((1ull << lane) - 1ull));
            active = false;
        }
        if (lane == leader) wcnt[wave][L] = __popcll(mm);
    }
    __syncthreads();
    if (valid) {
        int before = 0;
        for (int w = 0; w < wave; ++w) before += wcnt[w][lab];
        int slot = meta[META_SEG + lab] * BT + base[(long)blockIdx.x * n_ids + lab] + before + rank;
        src_of[slot] = (int)i;
    }
}

// One 16-byte unit of a row's operand image (see Geom): `row` = the row's kpad staged values.
__device__ __forceinline__ f32x4 image_unit_f32(const float *row, int u)
{
    const float *p = row + 8 * (u >> 1) + (u & 1);
    return f32x4{p[0], p[2], p[4], p[6]};
}
template <bool IS_QUERY>
__device__ __forceinline__ uint4 image_unit_bf16(const float *row, int u, int hi_units, int C, float norm)
{
    const float scale = IS_QUERY ? -2.0f : 1.0f;  // the query operand is -2q (exact in bf16)
    const bool lo = u >= hi_units;
    const int uu = lo ? u - hi_units : u;
    const int k0 = 16 * (uu >> 1) + 8 * (uu & 1);
    unsigned e8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = row[k0 + e];
        unsigned b = f2bf(x);
        if (lo) b = f2bf(x - bf2f(b));
        e8[e] = f2bf(scale * bf2f(b));
    }
    if (k0 + 8 > C && k0 < C + BF16_SPECIAL) {  // this unit holds norm slots (see Geom)
        unsigned piece[3];
        split3_bf16(norm, piece);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = k0 + e - C;  // 0..2: bank norm / query ones, 3..5: bank ones / query norm
            if (j >= 0 && j < BF16_SPECIAL) {
                const bool norm_slot = IS_QUERY ? (j >= 3) : (j < 3);
                // (a select chain, not piece[j % 3]: a run-time index keeps the three words in a private-memory stack object --
                // 36 bytes of scratch in frame_prepare_kernel<unsigned short, 32> through r5, tests/test_kernel_resources.py)
                const int j3 = j % 3;
                const unsigned pj = j3 == 0 ? piece[0] : (j3 == 1 ? piece[1] : piece[2]);
                e8[e] = lo ? 0u : (norm_slot ? pj : 0x3f80u);
            }
        }
    }
    return make_uint4(e8[0] | (e8[1] << 16), e8[2] | (e8[3] << 16), e8[4] | (e8[5] << 16), e8[6] | (e8[7] << 16));
}

// MANET_COMPUTE_F16: the same unit with fp16 elements (rounded to nearest even from the staged fp32 value) and the scaled norm
// pieces against 1, 2^-11, 2^-14 (see Geom)
template <bool IS_QUERY>
__device__ __forceinline__ uint4 image_unit_f16(const float *row, int u, int C, float norm)
{
    const float scale = IS_QUERY ? -2.0f : 1.0f;  // the query operand is -2q (exact in fp16 up to its overflow: the norm slot's NaN)
    const int k0 = 16 * (u >> 1) + 8 * (u & 1);
    unsigned e8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) e8[e] = f2h(scale * h2f(f2h(row[k0 + e])));
    if (k0 + 8 > C && k0 < C + BF16_SPECIAL) {  // this unit holds norm slots
        unsigned piece[3];
        split3_f16(norm, piece);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = k0 + e - C;  // 0..2: bank norm / query constants, 3..5: bank constants / query norm
            if (j >= 0 && j < BF16_SPECIAL) {
                const bool norm_slot = IS_QUERY ? (j >= 3) : (j < 3);
                const int j3 = j % 3;  // (select chains: see image_unit_bf16)
                const unsigned pj = j3 == 0 ? piece[0] : (j3 == 1 ? piece[1] : piece[2]);
                const unsigned cj = j3 == 0 ? 0x3c00u : (j3 == 1 ? 0x1000u : 0x0400u);  // 1, 2^-11, 2^-14
                e8[e] = norm_slot ? pj : cj;
            }
        }
    }
    return make_uint4(e8[0] | (e8[1] << 16), e8[2] | (e8[3] << 16), e8[4] | (e8[5] << 16), e8[6] | (e8[7] << 16));
}
// |row|^2 of a MANET_COMPUTE_F16 row as its norm slot takes it: outside fp16's domain (or NaN) -> NaN
__device__ __forceinline__ float norm_f16_domain(float n) { return n <= 65504.0f ? n : __builtin_nanf(""); }

// bank (ROWS = 64) and query (ROWS = 32) pack: rows -> MFMA operand image (see Geom).
// Rows are staged through LDS so that both the global reads (along k for row-major sources, along
// rows for C-major sources) and the 16-byte image writes are coalesced.  |row|^2 is the k-ascending
// fmaf chain of the oracle (IntVOS.py:32,35) -- over the bf16-rounded values in MANET_COMPUTE_BF16
// (the path then IS the reference formula on rounded embeddings), over the fp32 values otherwise.
// f32 images carry the norms in a trailing block; bf16 images carry them in the spare k slots (Geom).
// ROWS = rows staged per workgroup (a whole number of image blocks); IMG = rows per image block (64: bank tile,
// 32: query block).  keys != nullptr (query):
// the rows' match keys are reset to "no candidate" here, which saves the fill launch of the per-frame sequence.
// F16 (MANET_COMPUTE_F16) is a compile-time form of this body with kernels of its own (pack_rows_f16_kernel).
template <int ROWS, int IMG, typename SRC, bool F16>
__device__ __forceinline__ void pack_rows_body(const SRC *__restrict__ src, long s_row,
                                                        long s_c, const int *__restrict__ src_of,
                                                        const int *__restrict__ meta, long n_rows,
                                                        int C, int compute, int units, int kpad,
                                                        char *__restrict__ dst, long tile_bytes,
                                                        float pad_norm, unsigned *__restrict__ keys, long N_pad,
                                                        int n_ids)
{
    constexpr bool IS_QUERY = (IMG == QB);
    const long tile = blockIdx.x;
    if (meta && tile >= meta[META_T]) return;
    if (keys)
        for (int i = threadIdx.x; i < ROWS * n_ids; i += 256) keys[(size_t)(i / ROWS) * N_pad + tile * ROWS + (i % ROWS)] = 0xffffffffu;
    extern __shared__ __attribute__((aligned(16))) char pack_smem[];
    const int KP = kpad + 1;  // odd row stride: column reads are conflict-free
    float *rows = (float *)pack_smem;                  // [ROWS][KP]
    int *s_src = (int *)(rows + (long)ROWS * KP);      // [ROWS]
    float *s_norm = (float *)(s_src + ROWS);           // [ROWS]
    const int tid = threadIdx.x;
    if (tid < ROWS) {
        long slot = tile * ROWS + tid;
        s_src[tid] = src_of ? src_of[slot] : (slot < n_rows ? (int)slot : -1);
    }
    __syncthreads();
    if (s_c == 1) {  // row-major source: lanes along k
        for (int idx = tid; idx < ROWS * C; idx += 256) {
            int r = idx / C, k = idx - r * C;
            int sr = s_src[r];
            rows[r * KP + k] = (sr >= 0) ? emb_load(src, (long)sr * s_row + k) : 0.0f;
        }
    } else {  // C-major (or generic) source: lanes along rows
        for (int idx = tid; idx < ROWS * C; idx += 256) {
            int k = idx / ROWS, r = idx - k * ROWS;
            int sr = s_src[r];
            rows[r * KP + k] = (sr >= 0) ? emb_load(src, (long)sr * s_row + (long)k * s_c) : 0.0f;
        }
    }
    for (int idx = tid; idx < ROWS * (kpad - C); idx += 256) {
        int r = idx / (kpad - C), k = C + idx - r * (kpad - C);
        rows[r * KP + k] = 0.0f;
    }
    __syncthreads();
    if (tid < ROWS) {
        float n = F16 && pad_norm > 65504.0f ? INFINITY : pad_norm;  // (fp16 has no 1e20: a bank tile's padding rows carry +inf)
        if (s_src[tid] >= 0) {
            n = 0.0f;
            const float *row = rows + tid * KP;
            if constexpr (F16) {
                for (int k = 0; k < C; ++k) {
                    float x = h2f(f2h(row[k]));
                    n = fmaf(x, x, n);
                }
                n = norm_f16_domain(n);
            } else if (compute == MANET_COMPUTE_BF16) {
                for (int k = 0; k < C; ++k) {
                    float x = bf2f(f2bf(row[k]));
                    n = fmaf(x, x, n);
                }
            } else {
                for (int k = 0; k < C; ++k) n = fmaf(row[k], row[k], n);
            }
        }
        s_norm[tid] = n;
    }
    __syncthreads();
    // image block of staged row r: block (tile * ROWS/IMG + r / IMG), row r % IMG inside it
    char *out0 = dst + tile * (ROWS / IMG) * tile_bytes;
    if constexpr (F16) {
        for (int item = tid; item < units * ROWS; item += 256) {
            int r = item % ROWS, u = item / ROWS;
            *(uint4 *)(out0 + (r / IMG) * tile_bytes + ((long)u * IMG + r % IMG) * 16) =
                image_unit_f16<IS_QUERY>(rows + r * KP, u, C, s_norm[r]);
        }
    } else if (compute == MANET_COMPUTE_F32) {
        for (int item = tid; item < units * ROWS; item += 256) {
            int r = item % ROWS, u = item / ROWS;
            *(f32x4 *)(out0 + (r / IMG) * tile_bytes + ((long)u * IMG + r % IMG) * 16) = image_unit_f32(rows + r * KP, u);
        }
        if (tid < ROWS) *(float *)(out0 + (tid / IMG) * tile_bytes + (long)units * IMG * 16 + (tid % IMG) * 4) = s_norm[tid];
    } else {
        const int hi_units = (compute == MANET_COMPUTE_BF16X3) ? units / 2 : units;
        for (int item = tid; item < units * ROWS; item += 256) {
            int r = item % ROWS, u = item / ROWS;
            *(uint4 *)(out0 + (r / IMG) * tile_bytes + ((long)u * IMG + r % IMG) * 16) =
                image_unit_bf16<IS_QUERY>(rows + r * KP, u, hi_units, C, s_norm[r]);
        }
    }
}
#define MANET_PACK_ROWS_PARAMS                                                                                          \
    const SRC *__restrict__ src, long s_row, long s_c, const int *__restrict__ src_of, const int *__restrict__ meta,   \
        long n_rows, int C, int compute, int units, int kpad, char *__restrict__ dst, long tile_bytes, float pad_norm, \
        unsigned *__restrict__ keys, long N_pad, int n_ids
#define MANET_PACK_ROWS_ARGS src, s_row, s_c, src_of, meta, n_rows, C, compute, units, kpad, dst, tile_bytes, pad_norm, keys, N_pad, n_ids
template <int ROWS, int IMG, typename SRC>
__global__ __launch_bounds__(256) void pack_rows_kernel(MANET_PACK_ROWS_PARAMS)
{
    pack_rows_body<ROWS, IMG, SRC, false>(MANET_PACK_ROWS_ARGS);
}
template <int ROWS, int IMG, typename SRC>
__global__ __launch_bounds__(256) void pack_rows_f16_kernel(MANET_PACK_ROWS_PARAMS)
{
    pack_rows_body<ROWS, IMG, SRC, true>(MANET_PACK_ROWS_ARGS);
}
#undef MANET_PACK_ROWS_PARAMS
#undef MANET_PACK_ROWS_ARGS

// ---------------------------------------------------------------------------------------------
// Per-frame prepare (the producer side of the path): ONE read of a frame's C-major embedding
// writes BOTH per-frame operands of the propagation step --
//   * the query operand image of the global match (what pack_rows_kernel<32,32> writes), and
//   * the 2x2-average-pooled plane of the local match, padded with the reference's 1e20 (IntVOS.py:287), plus the
//     fused local kernel's tile table (what lf_pool_pad_kernel writes; r2 read both full-resolution frames again for
//     it, every frame: the stage moved 3x its algorithmic bytes) --
// so a propagated frame reads its embedding from HBM once, and the previous frame's not at all (its plane was made when
// it was the current frame).  Workgroup = one full-resolution row pair x XC columns, all channels, staged in LDS as
// [pixel][k] (odd stride: the row-wise and the k-wise accesses are both conflict-free); grid.z = frame of the batch.
// Blocks behind the data blocks fill the plane's top / bottom border rows, zero the image's padding rows, write the
// tile table and serve one optional caller fill (the local match's `out` pre-set, IntVOS.py:429-430's 1.0).
struct FramePrep {
    const void *emb;
    long s_f, s_y, s_x, s_c;
    int h, w, C, compute, units, kpad;
    char *ws;
    long ws_stride, qblk_bytes, off_plane, off_tab;
    int d, hp, wp, HPAD, WS;
    long PS;
    int TY, TX, nty, ntx;
    long N, N_pad;
    unsigned *fill_ptr;
    long fill_words;
    unsigned fill_value;
    int n_data, nxc;
    // manet_embed_finish: the embedding layer's epilogue in front of the staging -- y = relu(x * scale[c] + shift[c]), rounded to
    // the embedding's storage type, written to emb_out [frame][C][h][w] -- `emb` then is the 1x1 convolution's raw fp32 output
    const float *scale, *shift;
    void *emb_out;
    int emb_out_bf16, relu;
    int vec2;   // s_x == 1, even w / strides, aligned base: two pixels per load
    int rcopy;  // fp32 source + MANET_COMPUTE_BF16 / _F16: LDS also holds a copy rounded to the operand's element type
    int abl;    // always 0 (kept: the hot kernel's argument block stays as measured)
};
// VEC2 (r6): the two staging forms are separate instantiations -- as a run-time branch (r3-r5) both lived in every kernel and the
// 2-byte instantiation ran out of scalar registers (22 SGPR spills and a 36-byte private segment; tests/test_kernel_resources.py)
constexpr int XC = 32;  // full-resolution columns per workgroup
template <typename SRC, bool VEC2>
__global__ __launch_bounds__(256) void frame_prepare_kernel(const FramePrep A)
{
    const bool F16 = A.compute == MANET_COMPUTE_F16;  // (block-uniform) the fp16 image: fp16 elements, scaled norm pieces
    constexpr int PIX = 2 * XC;
    extern __shared__ __attribute__((aligned(16))) char pack_smem[];
    const int tid = threadIdx.x;
    const SRC *src = (const SRC *)A.emb + (long)blockIdx.z * A.s_f;
    char *ws = A.ws + (long)blockIdx.z * A.ws_stride;
    float *plane = (float *)(ws + A.off_plane);
    const int C = A.C, kpad = A.kpad, units = A.units;
    if ((int)blockIdx.x >= A.n_data) {  // ---- auxiliary blocks
        const long gid = (long)(blockIdx.x - A.n_data) * 256 + tid, gstride = (long)(gridDim.x - A.n_data) * 256;
        if (A.d >= 0) {
            const int rows_b = A.HPAD - A.hp, WS4 = A.WS / 4;
            const long items = (long)C * rows_b * WS4;
            const f32x4 pad = {MANET_WRONG_LABEL_PADDING_DISTANCE, MANET_WRONG_LABEL_PADDING_DISTANCE,
                               MANET_WRONG_LABEL_PADDING_DISTANCE, MANET_WRONG_LABEL_PADDING_DISTANCE};
            for (long i = gid; i < items; i += gstride) {
                const int c = (int)(i / ((long)rows_b * WS4));
                const int rem = (int)(i - (long)c * rows_b * WS4);
                const int rb = rem / WS4, q = rem - rb * WS4;
                const int r = rb < A.d ? rb : A.hp + rb;  // rows [0, d) and [d + hp, HPAD)
                *(f32x4 *)(plane + (long)c * A.PS + (long)r * A.WS + 4 * q) = pad;
            }
            {  // ... and the left / right border columns of the data rows [d, d + hp): columns [0, d) and [d + wp, WS)
                const int nb = A.WS - A.wp;  // border floats per row
                const long items2 = (long)C * A.hp * nb;
                for (long i = gid; i < items2; i += gstride) {
                    const int c = (int)(i / ((long)A.hp * nb));
                    const int rem = (int)(i - (long)c * A.hp * nb);
                    const int r = rem / nb, j = rem - r * nb;
                    plane[(long)c * A.PS + (long)(A.d + r) * A.WS + (j < A.d ? j : A.wp + j)] = MANET_WRONG_LABEL_PADDING_DISTANCE;
                }
            }
            int *tab = (int *)(ws + A.off_tab);
            for (long i = gid; i <= A.nty + 1 + A.ntx; i += gstride)
                tab[i] = i <= A.nty ? bilin_first((int)i * A.TY, A.hp, A.h) : bilin_first((int)(i - A.nty - 1) * A.TX, A.wp, A.w);
        }
        {  // rows N .. N_pad of the image: zero operands (their results are never read)
            const long tail = A.N_pad - A.N;
            for (long i = gid; i < tail * units; i += gstride) {
                const long n = A.N + i % tail;
                const int u = (int)(i / tail);
                *(uint4 *)(ws + (n >> 5) * A.qblk_bytes + ((long)u * QB + (n & 31)) * 16) = make_uint4(0, 0, 0, 0);
            }
            if (A.compute == MANET_COMPUTE_F32)
                for (long i = gid; i < tail; i += gstride) {
                    const long n = A.N + i;
                    *(float *)(ws + (n >> 5) * A.qblk_bytes + (long)units * QB * 16 + (n & 31) * 4) = 0.0f;
                }
        }
        if (blockIdx.z == 0)
            for (long i = gid; i < A.fill_words; i += gstride) A.fill_ptr[i] = A.fill_value;
        return;
    }
    // ---- data blocks
    // LDS: rows [PIX][KP] = the embedding as stored (what the pooled plane, the f32 and the split-bf16 image are made from);
    // rq = the values the bf16 image and its |q|^2 are made from: bf16-rounded.  2-byte sources ARE rounded already (rq = rows);
    // fp32 sources with plain-bf16 arithmetic get a second, rounded copy (A.rcopy) so that neither the norm chain nor the image
    // assembly rounds per use (r3: 5 us of norm chain and 7 us of image assembly in a 20 us launch).
    // The fp16 image (F16) likewise, rounded to fp16: there only the rounded copy counts as exact.
    const int KP = kpad + 1;
    float *rows = (float *)pack_smem;           // [PIX][KP]
    float *rq = A.rcopy ? rows + (long)PIX * KP : rows;
    const int rp = blockIdx.x / A.nxc, cx = blockIdx.x - rp * A.nxc;
    const int x0 = cx * XC, y0 = 2 * rp;
    // rq holds bf16-exact values (a 2-byte source, the rounded copy, or the embedding epilogue's 2-byte output)
    // (MANET_COMPUTE_F16: the rounded copy only -- a bf16 value need not be an fp16 value)
    const bool plain2 = F16 || A.compute == MANET_COMPUTE_BF16;  // one 2-byte image made from rounded values
    const bool bf16_exact = F16 ? (bool)A.rcopy
                                : (A.compute == MANET_COMPUTE_BF16) && (A.rcopy || sizeof(SRC) == 2 || (A.scale && A.emb_out_bf16));
    auto round2 = [F16](float x) { return F16 ? h2f(f2h(x)) : bf2f(f2bf(x)); };
    // The launch is LATENCY-bound, not bandwidth-bound (1.6 workgroups per CU, 27 MB per frame; ablations in DESIGN 3.3): every
    // load of the workgroup is issued before the first one is waited for -- one memory round trip per workgroup.
    if constexpr (VEC2) {  // two horizontally adjacent pixels per lane (8-byte / 4-byte loads): half the load instructions
        constexpr int NP2 = PIX / 2, NKQ = 256 / NP2;
        const int pp = tid % NP2, kq = tid / NP2;
        const int p = 2 * pp, y = y0 + p / XC, x = x0 + p % XC;  // (XC is even: both pixels in one row; w is even)
        const bool in = (y < A.h && x < A.w);
        const SRC *sp = src + (long)(y < A.h ? y : A.h - 1) * A.s_y + (long)(x < A.w ? x : A.w - 2);
        const long sc_ = A.s_c;
        float *r0 = rows + p * KP, *q0 = rq + p * KP;
        auto stage2 = [&](auto kb_tag) __attribute__((always_inline)) {
            constexpr int KB = decltype(kb_tag)::value;
            for (int k0 = kq; k0 < C; k0 += NKQ * KB) {
                float va[KB], vb[KB];
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const int k = k0 + j * NKQ;
                    const SRC *a = sp + (long)(k < C ? k : C - 1) * sc_;
                    if (sizeof(SRC) == 4) {
                        const float2 t = *(const float2 *)a;
                        va[j] = t.x; vb[j] = t.y;
                    } else {
                        const unsigned t = *(const unsigned *)a;
                        va[j] = bf2f(t & 0xffffu); vb[j] = bf2f(t >> 16);
                    }
                }
                if (sizeof(SRC) == 4 && A.scale) {  // the embedding layer's epilogue (block-uniform)
#pragma unroll
                    for (int j = 0; j < KB; ++j) {
                        const int k = k0 + j * NKQ, kc = k < C ? k : C - 1;
                        const float sc = A.scale[kc], sh = A.shift[kc];
                        float a = fmaf(va[j], sc, sh), b = fmaf(vb[j], sc, sh);
                        if (A.relu) { a = fmaxf(a, 0.0f); b = fmaxf(b, 0.0f); }
                        const long eo = (((long)blockIdx.z * C + kc) * A.h + (y < A.h ? y : A.h - 1)) * A.w + (x < A.w ? x : A.w - 2);
                        if (A.emb_out_bf16) {
                            const unsigned ba = f2bf(a), bb = f2bf(b);
                            a = bf2f(ba); b = bf2f(bb);  // the operands are made from the embedding AS STORED
                            if (in && k < C) *(unsigned *)((unsigned short *)A.emb_out + eo) = ba | (bb << 16);
                        } else if (in && k < C) {
                            *(float2 *)((float *)A.emb_out + eo) = float2{a, b};
                        }
                        va[j] = a; vb[j] = b;
                    }
                }
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const int k = k0 + j * NKQ;
                    if (k < C) {
                        const float a = in ? va[j] : 0.0f, b = in ? vb[j] : 0.0f;
                        r0[k] = a; r0[KP + k] = b;
                        if (A.rcopy) { q0[k] = round2(a); q0[KP + k] = round2(b); }
                    }
                }
            }
        };
        if (C <= 13 * NKQ) stage2(std::integral_constant<int, 13>{});
        else stage2(std::integral_constant<int, 16>{});
    } else {  // generic strides: one pixel per lane, lanes along x
        constexpr int NKQ = 256 / PIX;
        const int p = tid % PIX, kq = tid / PIX;
        const int y = y0 + p / XC, x = x0 + p % XC;
        const bool in = (y < A.h && x < A.w);
        const SRC *sp = src + (long)(y < A.h ? y : A.h - 1) * A.s_y + (long)(x < A.w ? x : A.w - 1) * A.s_x;
        const long sc_ = A.s_c;
        float *rp_ = rows + p * KP, *qp_ = rq + p * KP;
        auto stage = [&](auto kb_tag) __attribute__((always_inline)) {
            constexpr int KB = decltype(kb_tag)::value;
            for (int k0 = kq; k0 < C; k0 += NKQ * KB) {
                float v[KB];
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const int k = k0 + j * NKQ;
                    v[j] = emb_load(sp, (long)(k < C ? k : C - 1) * sc_);
                }
                if (sizeof(SRC) == 4 && A.scale) {  // the embedding layer's epilogue (block-uniform)
#pragma unroll
                    for (int j = 0; j < KB; ++j) {
                        const int k = k0 + j * NKQ, kc = k < C ? k : C - 1;
                        float a = fmaf(v[j], A.scale[kc], A.shift[kc]);
                        if (A.relu) a = fmaxf(a, 0.0f);
                        const long eo = (((long)blockIdx.z * C + kc) * A.h + (y < A.h ? y : A.h - 1)) * A.w + (x < A.w ? x : A.w - 1);
                        if (A.emb_out_bf16) {
                            const unsigned ba = f2bf(a);
                            a = bf2f(ba);
                            if (in && k < C) ((unsigned short *)A.emb_out)[eo] = (unsigned short)ba;
                        } else if (in && k < C) {
                            ((float *)A.emb_out)[eo] = a;
                        }
                        v[j] = a;
                    }
                }
#pragma unroll
                for (int j = 0; j < KB; ++j) {
                    const int k = k0 + j * NKQ;
                    if (k < C) {
                        const float a = in ? v[j] : 0.0f;
                        rp_[k] = a;
                        if (A.rcopy) qp_[k] = round2(a);
                    }
                }
            }
        };
        // (the whole channel range in one batch: C <= 100 -> 25 x NKQ, C <= 128 -> 32 x NKQ channels in flight per thread)
        if (C <= 25 * NKQ) stage(std::integral_constant<int, 25>{});
        else stage(std::integral_constant<int, 32>{});
    }
    for (int idx = tid; idx < PIX * (kpad - C); idx += 256) {
        const int p = idx / (kpad - C), k = C + idx - p * (kpad - C);
        rows[p * KP + k] = 0.0f;
        if (A.rcopy) rq[p * KP + k] = 0.0f;
    }
    __syncthreads();
    // ---- roles (no further barrier): wave 0 walks the |q|^2 chain -- 100 dependent fmaf, 1.5 us -- and then writes what needs
    // it (the f32 image's norm block / the bf16 image's units with norm slots) and the plane's border columns; waves 1..3 write
    // the pooled plane and the image units that do not depend on the norm while that chain runs.
    const bool f32img = (A.compute == MANET_COMPUTE_F32);
    const int hi_units = (A.compute == MANET_COMPUTE_BF16X3) ? units / 2 : units;
    // bf16 images: unit u carries norm slots iff its k range reaches past C (both halves of the split image are handled alike)
    auto unit_is_special = [&](int u) { const int uu = u >= hi_units ? u - hi_units : u; return 16 * (uu >> 1) + 8 * (uu & 1) + 8 > C; };
    auto image_addr = [&](long n, int u) { return ws + (n >> 5) * A.qblk_bytes + ((long)u * QB + (n & 31)) * 16; };
    // the bf16 image unit from bf16-EXACT staged values: -2 x is exact, its upper 16 bits are the bf16 (no rounding, no NaN fix-up:
    // identical bits to f2bf(-2 * bf2f(f2bf(x))))
    auto unit_bf16_exact = [&](const float *row, int u) {
        const int k0 = 16 * (u >> 1) + 8 * (u & 1);
        unsigned e8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) e8[e] = F16 ? f2h(-2.0f * row[k0 + e]) : __float_as_uint(-2.0f * row[k0 + e]) >> 16;
        return make_uint4(e8[0] | (e8[1] << 16), e8[2] | (e8[3] << 16), e8[4] | (e8[5] << 16), e8[6] | (e8[7] << 16));
    };
    // (f32 image: the last units / 6 units of every pixel are wave 0's as well -- its share of the store work behind the chain)
    const int u_split = f32img ? units - units / 6 : units;
    if (tid < PIX) {  // ---- wave 0 (PIX = 64 lanes)
        const int p = tid;
        const int y = y0 + p / XC, x = x0 + p % XC;
        const bool in = (y < A.h && x < A.w);
        const long n = (long)y * A.w + x;
        float nrm = 0.0f;
        {  // |q|^2: the k-ascending fmaf chain of the oracle, as pack_rows_kernel (reads batched ahead)
            const float *row = (plain2 ? rq : rows) + p * KP;
            const bool rnd = plain2 && !bf16_exact;
            int k = 0;
            for (; k + 10 <= C; k += 10) {
                float v[10];
#pragma unroll
                for (int j = 0; j < 10; ++j) v[j] = row[k + j];
#pragma unroll
                for (int j = 0; j < 10; ++j) {
                    const float xv = rnd ? round2(v[j]) : v[j];
                    nrm = fmaf(xv, xv, nrm);
                }
            }
            for (; k < C; ++k) {
                const float xv = rnd ? round2(row[k]) : row[k];
                nrm = fmaf(xv, xv, nrm);
            }
            if (F16) nrm = norm_f16_domain(nrm);
        }
        if (in) {
            if (f32img) {
                *(float *)(ws + (n >> 5) * A.qblk_bytes + (long)units * QB * 16 + (n & 31) * 4) = nrm;
                for (int u = u_split; u < units; ++u) *(f32x4 *)image_addr(n, u) = image_unit_f32(rows + p * KP, u);
            } else {
                for (int u = 0; u < units; ++u)
                    if (unit_is_special(u)) {
                        if (F16) *(uint4 *)image_addr(n, u) = image_unit_f16<true>(rows + p * KP, u, C, nrm);
                        else *(uint4 *)image_addr(n, u) = image_unit_bf16<true>(rows + p * KP, u, hi_units, C, nrm);
                    }
            }
        }
    }
    if (tid >= PIX) {  // ---- the other waves
        const int t = tid - PIX, NT = 256 - PIX;
        // pooled plane row d + rp (IntVOS.py:282-284: window summed row-major, times 1/4)
        if (A.d >= 0 && rp < A.hp) {
            float *prow = plane + (long)(A.d + rp) * A.WS + A.d + x0 / 2;
            for (int idx = t; idx < (XC / 2) * C; idx += NT) {
                const int c = idx / (XC / 2), px = idx - c * (XC / 2);
                if (x0 / 2 + px < A.wp) {
                    const float *q = rows + (2 * px) * KP + c;
                    prow[(long)c * A.PS + px] = (((q[0] + q[KP]) + q[XC * KP]) + q[(XC + 1) * KP]) * 0.25f;
                }
            }
        }
        // operand image: pixel (y, x) is query row n = y w + x -> block n / 32, row n % 32
        for (int item = t; item < u_split * PIX; item += NT) {
            const int p = item % PIX, u = item / PIX;
            const int y = y0 + p / XC, x = x0 + p % XC;
            if (y >= A.h || x >= A.w) continue;
            const long n = (long)y * A.w + x;
            if (f32img) *(f32x4 *)image_addr(n, u) = image_unit_f32(rows + p * KP, u);
            else if (unit_is_special(u)) continue;  // (wave 0, behind the norm chain)
            else if (bf16_exact) *(uint4 *)image_addr(n, u) = unit_bf16_exact(rq + p * KP, u);
            else if (F16) *(uint4 *)image_addr(n, u) = image_unit_f16<true>(rows + p * KP, u, C, 0.0f);
            else *(uint4 *)image_addr(n, u) = image_unit_bf16<true>(rows + p * KP, u, hi_units, C, 0.0f);
        }
    }
}

// Workspace initialisation as a plain kernel.  (hipMemsetAsync nodes were observed to replay with the
// wrong fill value from the second replay of a captured HIP graph on ROCm 7.2; a kernel node has no
// such problem, and callers may capture a frame's launch sequence.)
__global__ void fill32_kernel(unsigned *__restrict__ p, unsigned value, long n)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = value;
}

// the sorted bank once more as fp32 rows + |k|^2 (k-ascending fmaf chain over the fp32 values, as the f32 images carry
// it) + the bank's max |k|^2; grid = tiles, 256 threads
template <typename SRC>
__global__ __launch_bounds__(256) void bank_rows_f32_kernel(const SRC *__restrict__ src, long s_row, long s_c,
                                                            const int *__restrict__ src_of, int *__restrict__ meta, int C,
                                                            float *__restrict__ rows, float *__restrict__ norms)
{
    const long tile = blockIdx.x;
    if (tile >= meta[META_T]) return;
    for (int idx = threadIdx.x; idx < BT * C; idx += 256) {
        const int r = s_c == 1 ? idx / C : idx % BT, k = s_c == 1 ? idx % C : idx / BT;  // lanes along the source's fast axis
        const int sr = src_of[tile * BT + r];
        rows[(tile * BT + r) * C + k] = sr >= 0 ? emb_load(src, (long)sr * s_row + (long)k * s_c) : 0.0f;
    }
    if (threadIdx.x < BT) {
        const long slot = tile * BT + threadIdx.x;
        float n = MANET_WRONG_LABEL_PADDING_DISTANCE;
        const int sr = src_of[slot];
        if (sr >= 0) {
            n = 0.0f;
            for (int k = 0; k < C; ++k) {
                const float x = emb_load(src, (long)sr * s_row + (long)k * s_c);
                n = fmaf(x, x, n);
            }
            if (n == n) {
                atomicMax((unsigned *)&meta[META_KMAX], __float_as_uint(n));  // n >= 0: the bit pattern orders like the value
            } else {  // a NaN row: its object's minimum is NaN for every query (what MANET_COMPUTE_F32's min3p gives); keep it out
                int o = 0;  // of max |k|^2, which would void every OTHER object's threshold
                while (meta[META_SEG + o + 1] <= tile) ++o;
                meta[META_NAN + o] = 1;
            }
        }
        norms[slot] = n;
    }
}

// MANET_COMPUTE_F16_REFINE: what the filter's threshold must know about the bank, read from the packed fp16 image ITSELF (so that
// "outside the domain" here is exactly "NaN in the norm slot" there); a wave per tile, a lane per row:
//   META_F16_KMAX  max |k~|^2 over the rows inside fp16's domain (the scaled norm pieces of slots C .. C+2, see the f16 image)
//   META_F16_SUBN  max over those rows of the number of elements that are nonzero fp16 subnormals
//   META_F16_OOD   set if a row is outside the domain (NaN in its first norm slot) and its object holds no NaN row (META_NAN,
//                  written by bank_rows_f32_kernel before this launch: a NaN object's minimum is NaN whatever else it holds)
// Padding rows (+inf in the first norm slot) count for nothing.
__global__ __launch_bounds__(64) void f16_domain_kernel(const char *__restrict__ bpack, long tile_bytes, int units, int C,
                                                        int *__restrict__ meta)
{
    const long tile = blockIdx.x;
    if (tile >= meta[META_T]) return;
    const int r = threadIdx.x;
    const char *img = bpack + tile * tile_bytes;
    auto elem = [&](int k) {
        const int u = 2 * (k >> 4) + ((k >> 3) & 1);
        return (unsigned)*(const unsigned short *)(img + ((long)u * BT + r) * 16 + (k & 7) * 2);
    };
    const unsigned p0 = elem(C), a0 = p0 & 0x7fffu;
    const bool ood = a0 > 0x7c00u, real = a0 < 0x7c00u;
    float n2 = 0.0f;
    int sub = 0;
    if (real) {
        n2 = h2f(p0) + h2f(elem(C + 1)) * (1.0f / 2048.0f) + h2f(elem(C + 2)) * (1.0f / 16384.0f);
        for (int u = 0; u < units; ++u) {
            const uint4 v = *(const uint4 *)(img + ((long)u * BT + r) * 16);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
            const int k0 = 16 * (u >> 1) + 8 * (u & 1);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned b = (w[e >> 1] >> (16 * (e & 1))) & 0x7fffu;
                sub += (k0 + e < C && b != 0u && b < 0x0400u) ? 1 : 0;
            }
        }
    }
    unsigned nb = __float_as_uint(n2);  // n2 >= 0: the bit pattern orders like the value
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned onb = (unsigned)__shfl_xor((int)nb, d);
        const int osub = __shfl_xor(sub, d);
        nb = onb > nb ? onb : nb;
        sub = osub > sub ? osub : sub;
    }
    const bool any_ood = __ballot(ood) != 0ull;
    if (r == 0) {
        atomicMax((unsigned *)&meta[META_F16_KMAX], nb);
        atomicMax(&meta[META_F16_SUBN], sub);
        if (any_ood) {
            int o = 0;
            while (meta[META_SEG + o + 1] <= tile) ++o;
            if (!meta[META_NAN + o]) meta[META_F16_OOD] = 1;
        }
    }
}

// sub-sampled bank of the pre-pass: every REFINE_SUB-th tile of every object (at least one per non-empty object)
__global__ void sub_segments_kernel(int n_ids, const int *__restrict__ meta, int *__restrict__ sub_meta, int REFINE_SUB)
{
    if (threadIdx.x == 0) {
        int t = 0;
        for (int o = 0; o < n_ids; ++o) {
            sub_meta[META_SEG + o] = t;
            t += (meta[META_SEG + o + 1] - meta[META_SEG + o] + REFINE_SUB - 1) / REFINE_SUB;
        }
        sub_meta[META_SEG + n_ids] = t;
        sub_meta[META_T] = t;
    }
}
__global__ __launch_bounds__(256) void sub_copy_kernel(int n_ids, const int *__restrict__ meta,
                                                       const int *__restrict__ sub_meta, const char *__restrict__ bpack,
                                                       char *__restrict__ spack, long tile_bytes, int REFINE_SUB)
{
    const int j = blockIdx.x;
    if (j >= sub_meta[META_T]) return;
    int o = 0;
    while (sub_meta[META_SEG + o + 1] <= j) ++o;
    const long src_tile = meta[META_SEG + o] + (long)(j - sub_meta[META_SEG + o]) * REFINE_SUB;
    const uint4 *a = (const uint4 *)(bpack + src_tile * tile_bytes);
    uint4 *b = (uint4 *)(spack + (long)j * tile_bytes);
    for (long i = threadIdx.x; i < tile_bytes / 16; i += 256) b[i] = a[i];
}

}  // namespace

void fill32(void *p, unsigned value, size_t words, hipStream_t st)
{
    if (!words) return;
    unsigned blocks = (unsigned)((words + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(fill32_kernel, dim3(blocks), dim3(256), 0, st, (unsigned *)p, value, (long)words);
}

// bank pack (64-row tiles) and query pack (32-row blocks; keys != nullptr: also resets the rows' match keys)
// for either embedding storage type
int launch_bank_pack(const void *src, int emb_dtype, long s_row, long s_c, const int *src_of, const int *meta, long n_rows,
                     int C, const Geom &G, char *dst, long ntiles, hipStream_t st)
{
    if (ntiles <= 0) return MANET_OK;
    const size_t lds = (size_t)BT * (G.kpad + 1) * sizeof(float) + 2 * BT * sizeof(int);
    if (emb_dtype != MANET_EMB_F32 && emb_dtype != MANET_EMB_BF16)
        return manet_set_error(MANET_E_INVALID, "embedding dtype %d (MANET_EMB_F32 / MANET_EMB_BF16)", emb_dtype);
    if (G.compute == MANET_COMPUTE_F16) {
        if (emb_dtype == MANET_EMB_F32)
            hipLaunchKernelGGL((pack_rows_f16_kernel<BT, BT, float>), dim3((unsigned)ntiles), dim3(256), lds, st, (const float *)src,
                               s_row, s_c, src_of, meta, n_rows, C, G.compute, G.units, G.kpad, dst, (long)G.tile_bytes,
                               MANET_WRONG_LABEL_PADDING_DISTANCE, (unsigned *)nullptr, 0L, 0);
        else
            hipLaunchKernelGGL((pack_rows_f16_kernel<BT, BT, unsigned short>), dim3((unsigned)ntiles), dim3(256), lds, st,
                               (const unsigned short *)src, s_row, s_c, src_of, meta, n_rows, C, G.compute, G.units, G.kpad,
                               dst, (long)G.tile_bytes, MANET_WRONG_LABEL_PADDING_DISTANCE, (unsigned *)nullptr, 0L, 0);
        return MANET_OK;
    }
    if (emb_dtype == MANET_EMB_F32)
        hipLaunchKernelGGL((pack_rows_kernel<BT, BT, float>), dim3((unsigned)ntiles), dim3(256), lds, st, (const float *)src,
                           s_row, s_c, src_of, meta, n_rows, C, G.compute, G.units, G.kpad, dst, (long)G.tile_bytes,
                           MANET_WRONG_LABEL_PADDING_DISTANCE, (unsigned *)nullptr, 0L, 0);
    else if (emb_dtype == MANET_EMB_BF16)
        hipLaunchKernelGGL((pack_rows_kernel<BT, BT, unsigned short>), dim3((unsigned)ntiles), dim3(256), lds, st,
                           (const unsigned short *)src, s_row, s_c, src_of, meta, n_rows, C, G.compute, G.units, G.kpad,
                           dst, (long)G.tile_bytes, MANET_WRONG_LABEL_PADDING_DISTANCE, (unsigned *)nullptr, 0L, 0);
    else
        return manet_set_error(MANET_E_INVALID, "embedding dtype %d (MANET_EMB_F32 / MANET_EMB_BF16)", emb_dtype);
    return MANET_OK;
}

int launch_query_pack(const void *src, int emb_dtype, long s_row, long s_c, long N, long N_pad, int C, const Geom &G,
                      char *dst, unsigned *keys, int n_ids, hipStream_t st)
{
    constexpr int SR = QB;  // staged rows per workgroup (two blocks per workgroup measured slower: 22 vs 16 us at 480p)
    const size_t lds = (size_t)SR * (G.kpad + 1) * sizeof(float) + 2 * SR * sizeof(int);
    const unsigned blocks = (unsigned)(N_pad / SR);
    if (emb_dtype != MANET_EMB_F32 && emb_dtype != MANET_EMB_BF16)
        return manet_set_error(MANET_E_INVALID, "embedding dtype %d (MANET_EMB_F32 / MANET_EMB_BF16)", emb_dtype);
    if (G.compute == MANET_COMPUTE_F16) {
        if (emb_dtype == MANET_EMB_F32)
            hipLaunchKernelGGL((pack_rows_f16_kernel<SR, QB, float>), dim3(blocks), dim3(256), lds, st, (const float *)src, s_row,
                               s_c, (const int *)nullptr, (const int *)nullptr, N, C, G.compute, G.units, G.kpad, dst,
                               (long)G.qblk_bytes, 0.0f, keys, N_pad, n_ids);
        else
            hipLaunchKernelGGL((pack_rows_f16_kernel<SR, QB, unsigned short>), dim3(blocks), dim3(256), lds, st,
                               (const unsigned short *)src, s_row, s_c, (const int *)nullptr, (const int *)nullptr, N, C,
                               G.compute, G.units, G.kpad, dst, (long)G.qblk_bytes, 0.0f, keys, N_pad, n_ids);
        return MANET_OK;
    }
    if (emb_dtype == MANET_EMB_F32)
        hipLaunchKernelGGL((pack_rows_kernel<SR, QB, float>), dim3(blocks), dim3(256), lds, st, (const float *)src, s_row, s_c,
                           (const int *)nullptr, (const int *)nullptr, N, C, G.compute, G.units, G.kpad, dst,
                           (long)G.qblk_bytes, 0.0f, keys, N_pad, n_ids);
    else if (emb_dtype == MANET_EMB_BF16)
        hipLaunchKernelGGL((pack_rows_kernel<SR, QB, unsigned short>), dim3(blocks), dim3(256), lds, st,
                           (const unsigned short *)src, s_row, s_c, (const int *)nullptr, (const int *)nullptr, N, C,
                           G.compute, G.units, G.kpad, dst, (long)G.qblk_bytes, 0.0f, keys, N_pad, n_ids);
    else
        return manet_set_error(MANET_E_INVALID, "embedding dtype %d (MANET_EMB_F32 / MANET_EMB_BF16)", emb_dtype);
    return MANET_OK;
}

ManetFrameLayout manet_frame_layout(int h, int w, int C, int compute, int max_distance)
{
    ManetFrameLayout F;
    const MatchLayout ML = match_layout((int64_t)h * w, C, 1, compute);
    F.N_pad = ML.N_pad;
    F.off_image = 0;
    F.image_bytes = (size_t)(ML.N_pad / QB) * ML.qblk_bytes;
    F.off_plane = manet_align_up(F.image_bytes, 1024);
    F.hp = h / 2;
    F.wp = w / 2;
    F.HPAD = F.WS = F.TY = F.TX = F.nty = F.ntx = 0;
    F.PS = 0;
    F.plane_bytes = F.tab_bytes = 0;
    if (max_distance >= 0) {
        const PoolPad G = lf_pool_pad(h, w, max_distance);
        F.HPAD = G.HPAD;
        F.WS = G.WS;
        F.PS = G.plane;
        F.TY = lf_sy(max_distance) - 1;
        F.TX = LF_SX - 1;
        F.nty = (F.hp + F.TY - 1) / F.TY;
        F.ntx = (F.wp + F.TX - 1) / F.TX;
        F.plane_bytes = (size_t)G.plane * C * sizeof(float);
        F.tab_bytes = (size_t)(F.nty + F.ntx + 2) * sizeof(int);
    }
    F.off_tab = manet_align_up(F.off_plane + F.plane_bytes, 256);
    F.total = manet_align_up(F.off_tab + F.tab_bytes, 1024);
    return F;
}

extern "C" {

int manet_frame_workspace_bytes(int h, int w, int C, int compute, int max_distance, size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    if (h <= 0 || w <= 0) return manet_set_error(MANET_E_INVALID, "h=%d w=%d", h, w);
    int rc = check_common((int64_t)h * w, 0, C, 1, 1, compute);
    if (rc) return rc;
    if (max_distance > MANET_MAX_LOCAL_DISTANCE || (max_distance >= 0 && (h < 2 || w < 2)))
        return manet_set_error(MANET_E_INVALID, "max_distance=%d (supported -1 = no pooled plane, 0..%d; h, w >= 2)",
                               max_distance, MANET_MAX_LOCAL_DISTANCE);
    *bytes = manet_frame_layout(h, w, C, compute, max_distance).total;
    return MANET_OK;
}

static int frame_prepare_impl(const void *emb, int emb_dtype, int64_t s_f, int64_t s_y, int64_t s_x, int64_t s_c, int n_frames,
                              int h, int w, int C, int compute, int max_distance, void *frames_ws, size_t frame_ws_stride,
                              void *fill_ptr, int64_t fill_words, uint32_t fill_value, const float *scale, const float *shift,
                              int relu, void *emb_out, int emb_out_dtype, manet_stream_t stream)
{
    size_t need = 0;
    int rc = manet_frame_workspace_bytes(h, w, C, compute, max_distance, &need);
    if (rc) return rc;
    if (!emb || !frames_ws || n_frames <= 0 || n_frames > 65535)
        return manet_set_error(MANET_E_INVALID, "null pointer or n_frames=%d", n_frames);
    if (frame_ws_stride < need || (frame_ws_stride & 1023))
        return manet_set_error(MANET_E_WORKSPACE, "frame workspace stride %zu < %zu bytes (or not a multiple of 1024)",
                               frame_ws_stride, need);
    if (fill_words < 0 || (fill_words > 0 && !fill_ptr)) return manet_set_error(MANET_E_INVALID, "bad fill request");
    const ManetFrameLayout F = manet_frame_layout(h, w, C, compute, max_distance);
    const Geom G = geom_of(C, compute);
    FramePrep A;
    A.emb = emb;
    A.s_f = (long)s_f; A.s_y = (long)s_y; A.s_x = (long)s_x; A.s_c = (long)s_c;
    A.h = h; A.w = w; A.C = C; A.compute = G.compute; A.units = G.units; A.kpad = G.kpad;  // (G.compute: _BF16_REFINE packs as _BF16, _F16_REFINE as _F16)
    A.ws = (char *)frames_ws; A.ws_stride = (long)frame_ws_stride; A.qblk_bytes = (long)G.qblk_bytes;
    A.off_plane = (long)F.off_plane; A.off_tab = (long)F.off_tab;
    A.d = max_distance; A.hp = F.hp; A.wp = F.wp; A.HPAD = F.HPAD; A.WS = F.WS; A.PS = F.PS;
    A.TY = F.TY; A.TX = F.TX; A.nty = F.nty; A.ntx = F.ntx;
    A.N = (long)h * w; A.N_pad = F.N_pad;
    A.fill_ptr = (unsigned *)fill_ptr; A.fill_words = (long)fill_words; A.fill_value = fill_value;
    A.nxc = (w + XC - 1) / XC;
    A.abl = 0;
    A.n_data = ((h + 1) / 2) * A.nxc;
    long aux_items = (long)(F.N_pad - A.N) * G.units + fill_words + 64;
    if (max_distance >= 0) aux_items += (long)C * (F.HPAD - F.hp) * (F.WS / 4) + (long)C * F.hp * (F.WS - F.wp) / 4;
    long aux = (aux_items + 1023) / 1024;
    if (aux < 1) aux = 1;
    if (aux > 256) aux = 256;
    const size_t esz = emb_dtype == MANET_EMB_F32 ? 4 : 2;
    A.vec2 = (s_x == 1 && (w & 1) == 0 && (s_y & 1) == 0 && (s_c & 1) == 0 && (n_frames == 1 || (s_f & 1) == 0) &&
              ((size_t)emb % (2 * esz)) == 0) ? 1 : 0;
    A.scale = scale; A.shift = shift; A.relu = relu; A.emb_out = emb_out; A.emb_out_bf16 = (scale && emb_out_dtype == MANET_EMB_BF16) ? 1 : 0;
    // (the epilogue form stores 2-pixel pairs: emb_out rows must pair up as the source's do)
    if (scale && (w & 1)) A.vec2 = 0;
    const bool f16 = G.compute == MANET_COMPUTE_F16;
    A.rcopy = (emb_dtype == MANET_EMB_F32 && (G.compute == MANET_COMPUTE_BF16 || f16) && !A.emb_out_bf16) ? 1 : 0;
    const size_t lds = (size_t)(A.rcopy ? 2 : 1) * 2 * XC * (G.kpad + 1) * sizeof(float) + 2 * XC * sizeof(float);
    const dim3 grid((unsigned)(A.n_data + aux), 1, (unsigned)n_frames);
    hipStream_t st = (hipStream_t)stream;
    if (emb_dtype != MANET_EMB_F32 && emb_dtype != MANET_EMB_BF16)
        return manet_set_error(MANET_E_INVALID, "embedding dtype %d (MANET_EMB_F32 / MANET_EMB_BF16)", emb_dtype);
    const void *fn = emb_dtype == MANET_EMB_F32
                         ? (A.vec2 ? (const void *)frame_prepare_kernel<float, true> : (const void *)frame_prepare_kernel<float, false>)
                         : (A.vec2 ? (const void *)frame_prepare_kernel<unsigned short, true>
                                   : (const void *)frame_prepare_kernel<unsigned short, false>);
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    void *args[] = {(void *)&A};
    manet_profile_record(st, true, 2);
    (void)hipLaunchKernel(fn, grid, dim3(256), args, lds, st);
    manet_profile_record(st, false, 2);
    return manet_check_launch("manet_frame_prepare");
}

int manet_frame_prepare(const void *emb, int emb_dtype, int64_t s_f, int64_t s_y, int64_t s_x, int64_t s_c, int n_frames,
                        int h, int w, int C, int compute, int max_distance, void *frames_ws, size_t frame_ws_stride,
                        void *fill_ptr, int64_t fill_words, uint32_t fill_value, manet_stream_t stream)
{
    return frame_prepare_impl(emb, emb_dtype, s_f, s_y, s_x, s_c, n_frames, h, w, C, compute, max_distance, frames_ws,
                              frame_ws_stride, fill_ptr, fill_words, fill_value, nullptr, nullptr, 0, nullptr, MANET_EMB_F32, stream);
}

int manet_embed_finish(const float *conv_out, int64_t s_f, int64_t s_y, int64_t s_x, int64_t s_c, const float *scale,
                       const float *shift, int relu, void *emb_out, int emb_out_dtype, int n_frames, int h, int w, int C,
                       int compute, int max_distance, void *frames_ws, size_t frame_ws_stride, manet_stream_t stream)
{
    if (!scale || !shift || !emb_out) return manet_set_error(MANET_E_INVALID, "null pointer");
    if (emb_out_dtype != MANET_EMB_F32 && emb_out_dtype != MANET_EMB_BF16)
        return manet_set_error(MANET_E_INVALID, "embedding dtype %d (MANET_EMB_F32 / MANET_EMB_BF16)", emb_out_dtype);
    if (((size_t)emb_out & 7) != 0) return manet_set_error(MANET_E_INVALID, "emb_out must be 8-byte aligned");
    return frame_prepare_impl(conv_out, MANET_EMB_F32, s_f, s_y, s_x, s_c, n_frames, h, w, C, compute, max_distance, frames_ws,
                              frame_ws_stride, nullptr, 0, 0u, scale, shift, relu, emb_out, emb_out_dtype, stream);
}

int manet_bank_workspace_bytes(int64_t M0, int C, int n_ids, int compute, size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = check_common(1, M0, C, n_ids, 1, compute);
    if (rc) return rc;
    *bytes = bank_layout(M0, C, n_ids, compute).total;
    return MANET_OK;
}

int manet_bank_prepare(const float *bank, int64_t b_stride_m, int64_t b_stride_c, const int32_t *labels,
                       int64_t M0, int C, int n_ids, int compute, void *bank_ws, size_t bank_ws_bytes,
                       manet_stream_t stream)
{
    return manet_bank_prepare_ex(bank, MANET_EMB_F32, b_stride_m, b_stride_c, labels, M0, C, n_ids, compute, bank_ws,
                                 bank_ws_bytes, stream);
}

int manet_bank_prepare_ex(const void *bank, int emb_dtype, int64_t b_stride_m, int64_t b_stride_c, const int32_t *labels,
                          int64_t M0, int C, int n_ids, int compute, void *bank_ws, size_t bank_ws_bytes,
                          manet_stream_t stream)
{
    int rc = check_common(1, M0, C, n_ids, 1, compute);
    if (rc) return rc;
    if ((M0 > 0 && (!bank || !labels)) || !bank_ws) return manet_set_error(MANET_E_INVALID, "null pointer");
    BankLayout L = bank_layout(M0, C, n_ids, compute);
    if (bank_ws_bytes < L.total)
        return manet_set_error(MANET_E_WORKSPACE, "bank workspace %zu < %zu bytes", bank_ws_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)bank_ws;
    int *meta = (int *)(ws + L.off_meta);
    int *hist = (int *)(ws + L.off_hist);
    int *src_of = (int *)(ws + L.off_src);
    fill32(meta, 0u, META_INTS, st);
    fill32(src_of, 0xffffffffu, (size_t)L.T_max * BT, st);
    if (M0 > 0) {
        hipLaunchKernelGGL(label_hist_kernel, dim3((unsigned)L.nblocks), dim3(RPB), 0, st, labels, (long)M0, n_ids, hist);
        hipLaunchKernelGGL(label_scan_kernel, dim3((unsigned)n_ids), dim3(64), 0, st, hist, (int)L.nblocks, n_ids, meta);
    }
    hipLaunchKernelGGL(label_segments_kernel, dim3(1), dim3(64), 0, st, n_ids, meta);
    if (M0 > 0)
        hipLaunchKernelGGL(label_scatter_kernel, dim3((unsigned)L.nblocks), dim3(RPB), 0, st, labels, (long)M0, n_ids,
                           (const int *)hist, (const int *)meta, src_of);
    rc = launch_bank_pack(bank, emb_dtype, (long)b_stride_m, (long)b_stride_c, (const int *)src_of, (const int *)meta, (long)M0,
                          C, L.G, ws + L.off_pack, L.T_max, st);
    if (rc) return rc;
    if (is_refine(compute)) {
        // the fp32 operand image of the same sorted bank: what the rescue pass (the exact fp32 kernel on the query blocks
        // whose candidate buckets are incomplete) multiplies against
        rc = launch_bank_pack(bank, emb_dtype, (long)b_stride_m, (long)b_stride_c, (const int *)src_of, (const int *)meta,
                              (long)M0, C, L.G32, ws + L.off_pack32, L.T_max, st);
        if (rc) return rc;
        // the fp32 copy of the sorted rows the exact re-rank reads, and the sub-sampled bank of the pre-pass
        float *rows = (float *)(ws + L.off_rows), *norms = (float *)(ws + L.off_norms);
        int *sub_meta = (int *)(ws + L.off_sub_meta);
        if (L.T_max > 0) {
            if (emb_dtype == MANET_EMB_F32)
                hipLaunchKernelGGL(bank_rows_f32_kernel<float>, dim3((unsigned)L.T_max), dim3(256), 0, st, (const float *)bank,
                                   (long)b_stride_m, (long)b_stride_c, (const int *)src_of, meta, C, rows, norms);
            else
                hipLaunchKernelGGL(bank_rows_f32_kernel<unsigned short>, dim3((unsigned)L.T_max), dim3(256), 0, st,
                                   (const unsigned short *)bank, (long)b_stride_m, (long)b_stride_c, (const int *)src_of, meta, C,
                                   rows, norms);
            if (compute == MANET_COMPUTE_F16_REFINE)
                hipLaunchKernelGGL(f16_domain_kernel, dim3((unsigned)L.T_max), dim3(64), 0, st, (const char *)(ws + L.off_pack),
                                   (long)L.tile_bytes, L.G.units, C, meta);
        }
        fill32(sub_meta, 0u, META_INTS, st);
        const int sub = refine_sub(L.T_max);
        hipLaunchKernelGGL(sub_segments_kernel, dim3(1), dim3(64), 0, st, n_ids, (const int *)meta, sub_meta, sub);
        hipLaunchKernelGGL(sub_copy_kernel, dim3((unsigned)L.T_sub_max), dim3(256), 0, st, n_ids, (const int *)meta,
                           (const int *)sub_meta, (const char *)(ws + L.off_pack), ws + L.off_sub_pack, (long)L.tile_bytes, sub);
    }
    return manet_check_launch("manet_bank_prepare");
}

int manet_query_pack_bytes(int64_t N, int C, int compute, size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = check_common(N, 0, C, 1, 1, compute);
    if (rc) return rc;
    MatchLayout ML = match_layout(N, C, 1, compute);
    *bytes = (size_t)(ML.N_pad / QB) * ML.qblk_bytes;
    return MANET_OK;
}

int manet_query_pack(const void *query, int emb_dtype, int64_t q_stride_n, int64_t q_stride_c, int64_t N, int C,
                     int compute, void *packed, size_t packed_bytes, manet_stream_t stream)
{
    int rc = check_common(N, 0, C, 1, 1, compute);
    if (rc) return rc;
    if (!query || !packed) return manet_set_error(MANET_E_INVALID, "null pointer");
    MatchLayout ML = match_layout(N, C, 1, compute);
    const size_t need = (size_t)(ML.N_pad / QB) * ML.qblk_bytes;
    if (packed_bytes < need) return manet_set_error(MANET_E_WORKSPACE, "packed query buffer %zu < %zu bytes", packed_bytes, need);
    rc = launch_query_pack(query, emb_dtype, (long)q_stride_n, (long)q_stride_c, (long)N, ML.N_pad, C, ML.G, (char *)packed,
                           nullptr, 0, (hipStream_t)stream);
    if (rc) return rc;
    return manet_check_launch("manet_query_pack");
}

}  // extern "C"
