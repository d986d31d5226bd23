// Depthwise 7x7 convolution + BatchNorm(eval) + ReLU, fused -- SURVEY.md 8f rank 1 (the step right after
// the matching path): the building block of the reference's DynamicSegHead (IntVOS.py:488-506,
// _split_separable_conv2d: conv1 (groups = channels, 7x7, padding 3) -> bn1 -> relu1).
//
// Why it is here: on MI355X the framework's conv library has no tuned depthwise-7x7 fp32 kernel and falls
// back to a naive one (0.83 ms per call at [3,256,120,214]; 55 % of the GPU time of a propagated frame,
// profiles/r01_e2e_kernel_stats.csv) although the op is a pure HBM stream: 2 x 4 B per element.
//
//   out[b][c][y][x] = relu( (sum_{ky,kx} in[b][c][y+ky-3][x+kx-3] * w[c][ky][kx] + bias[c]) * scale[c] + shift[c] )
// with zero padding, scale = gamma / sqrt(var + eps), shift = beta - mean * scale (BatchNorm in eval mode).
//
// r2 kernel.  The op is 49 FMAs per output on a pure stream (2 x 4 B per element): at [3,256,120,214] that is
// 158 MB (20 us at 8 TB/s) and 15 M scalar wave-FMAs (~28 us at the measured v_fma_f32 rate) -- the r1 kernel (one
// output row x 4 columns per thread, scalar FMAs, 16 x 64 tiles) took 58 us.  Here:
//  * a thread owns 2 rows x 8 columns; its running sums are VERTICAL pairs (out[y][x], out[y+1][x]), so every tap is one
//    v_pk_fma_f32 with the tap weight broadcast: half the VALU instructions (a wave issues one VALU instruction per
//    ~2.5 ns whatever its width: tools/ubench/valu_rate.hip);
//  * the packed operand must be an aligned register pair holding (in[r][x], in[r+1][x]): the input tile is kept in LDS
//    twice, rows interleaved in pairs starting at even rows (E) and at odd rows (O); a kernel row ky reads pair
//    (2t + ky, 2t + ky + 1) from E or O by parity, 14 columns = 7 ds_read_b128 for 56 packed FMAs;
//  * workgroup = 60 x 64 outputs (halo amplification 1.2x instead of 1.5x), 256 threads, 39 KB LDS -> 4 per CU;
//  * `relu_in`: max(x, 0) applied while staging, so the caller can drop the separate ReLU pass after the preceding
//    1x1 convolution (IntVOS.py:503-505: relu2 of the previous block) -- one HBM round trip less per block.
// Tap order (ky outer, kx inner, fmaf chain per output) is the r1 kernel's and the oracle's: bit-identical.
#include "manet_common.h"

#include <type_traits>

namespace {

constexpr int DW_K = 7, DW_R = 3;
// Tile shapes.  DwStd: 60 rows (480p's 120 and 720p's 180 grid rows tile exactly; 33 row pairs of LDS) x 64 columns, 16 column groups of
// 4 x 15 row groups of 4 = 240 of 256 threads.  LDS columns: image columns x0-4 .. x0+TX+3 (even start: aligned float2 loads) = 72,
// padded to 74: the row-pair stride 148 floats = 20 (mod 64 banks) puts the four (row pair, column group) quads of a ds_read_b128 lane
// group on disjoint banks (stride 144: 4-way conflicts on every window read).
// DwNarrow (r6): 120 rows x 24 columns for the strip a plane's last tile column leaves when it holds at most 24 columns -- 480p's 214
// columns are 3.34 tiles of 64: the fourth column's two 60 x 64 tiles did a full tile's work each for 22 of 64 columns; ONE 120 x 24 tile
// (6 column groups x 30 row groups = 180 threads) covers the strip: 7 workgroups per plane instead of 8.
struct DwStd {
    static constexpr int TY = 60, TX = 64, CG = TX / 4, LW = 74, NP = (TY + 2 * DW_R) / 2, IMG = NP * LW * 2, NQ = (TX + 8) / 2;
};
struct DwNarrow {
    static constexpr int TY = 120, TX = 24, CG = TX / 4, LW = 34, NP = (TY + 2 * DW_R) / 2, IMG = NP * LW * 2, NQ = (TX + 8) / 2;
};
static_assert(DwNarrow::IMG <= DwStd::IMG, "the narrow tile shares the standard tile's LDS array");
constexpr int DW_TY = DwStd::TY, DW_TX = DwStd::TX, DW_IMG = DwStd::IMG;

// FAST: w even (every aligned column pair is inside or outside the image as a whole, rows are 8-byte aligned)
// r3b: a workgroup owns one (tile, channel) and walks the BATCH items (the objects of a frame): the next item's global loads
// are issued before the current item's arithmetic and land under it, the weights are read once.  (One workgroup per
// (tile, plane), as before: every workgroup of a launch read, then computed, then wrote, in step with its neighbours -- the
// memory system saw alternating read and write bursts: 53 us for 158 MB at [3,256,120,214].)
// (the 4-byte-load form of odd widths needs ~148 registers: three workgroups per CU -- at four it spilled 20 of them, r4)
// RELU_IN / RELU (r5): compile-time -- as run-time flags each staged element paid a select on top of its max (76 v_cndmask +
// 76 v_max per item against 392 packed FMAs), each output one more.  (Worth ~1 % on a warm GPU: the kernel hides it.)
// TI / TO (head_act="f16", dwconv7x7_bn_relu_f16_kernel): the element types of the input and output planes, float or _Float16.
// Halves are widened while staging (a FAST load is then 4 bytes = two halves) and the output is rounded once, to nearest even,
// after the fp32 epilogue: out = rn16(min(relu(.), 65504)) with a NaN kept; the LDS image and the arithmetic are fp32 either way.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr float F16_MAX = 65504.0f;
template <typename T> struct DwPair { typedef f32x2 type; };
template <> struct DwPair<_Float16> { typedef f16x2 type; };
// relu and the saturation of an fp16 store, both keeping a NaN (fmaxf / fminf return the other operand)
__device__ __forceinline__ float f16_relu(float v) { return v <= 0.0f ? 0.0f : v; }
__device__ __forceinline__ float f16_sat(float v) { return v > F16_MAX ? F16_MAX : v; }

template <typename SH, bool FAST, bool RELU_IN, bool RELU, typename TI = float, typename TO = float>
__device__ __forceinline__ void dw_tile(float *__restrict__ tile, const TI *__restrict__ in, int C, int h, int w,
                                        const float *__restrict__ weight, const float *__restrict__ bias,
                                        const float *__restrict__ scale, const float *__restrict__ shift, TO *__restrict__ out,
                                        int c, int b_first, int b_end, int x0, int y0)
{
    typedef typename DwPair<TI>::type ld_t;
    constexpr unsigned IB = sizeof(TI), OB = sizeof(TO);
    constexpr bool relu_in = RELU_IN, relu = RELU;
    constexpr int DW_LW = SH::LW, DW_NP = SH::NP, DW_IMG = SH::IMG, DW_TY = SH::TY;
    const long plane = (long)h * w;
    const int tid = threadIdx.x;
    // staging item = (row pair p, column pair q): rows 2p, 2p+1, 2p+2 of the tile, two columns -- one b128 store into E
    // (rows 2p, 2p+1) and one into O (rows 2p+1, 2p+2).  Branch-free: clamped addresses, values selected afterwards.
    constexpr int NQ = SH::NQ, NITEM = DW_NP * NQ, KI = (NITEM + 255) / 256;  // column pairs = image columns x0-4 .. x0+TX+3
    // pass 1: every load of the thread is issued (clamped addresses, no predicate anywhere near them); pass 2 selects,
    // rectifies and stores.  Written as one loop, hipcc sinks each load into the branch of its select and waits
    // vmcnt(0) there: 15 serial L2 round trips per thread (r2 trace: this, not the 392 FMAs, was the kernel's time).
    ld_t ld[KI][3];
    unsigned off[KI][3];  // BYTE offsets inside a plane (the same for every batch item)
#pragma unroll
    for (int k = 0; k < KI; ++k) {
        const int i = tid + 256 * k;
        const int p = i / NQ, q = i - p * NQ;
        const int xx = x0 - 4 + 2 * q;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int yc = min(max(y0 - DW_R + 2 * p + e, 0), h - 1);
            off[k][e] = IB * (unsigned)(yc * w + min(max(xx, 0), FAST ? w - 2 : w - 1));
        }
    }
    auto issue_loads = [&](int b) __attribute__((always_inline)) {
        // (unsigned BYTE offsets on a uniform base: the loads take the scalar-base + 32-bit-offset form.  r2-r4 kept element
        // offsets: times 4 they need 33 bits, so hipcc widened each to a 64-bit VGPR pair and added the base with a
        // v_lshl_add_u64 per load and item -- 15 pairs of registers and 15 64-bit adds per item)
        const char *src = (const char *)(in + ((long)b * C + c) * plane);
#pragma unroll
        for (int k = 0; k < KI; ++k) {
            const int i = tid + 256 * k;
            const int xx = x0 - 4 + 2 * (i - (i / NQ) * NQ);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                if (FAST) {
                    ld[k][e] = *(const ld_t *)(src + off[k][e]);
                } else {
                    ld[k][e][0] = *(const TI *)(src + off[k][e]);
                    ld[k][e][1] = *(const TI *)(src + (unsigned)(off[k][e] - IB * (unsigned)min(max(xx, 0), w - 1) + IB * (unsigned)min(max(xx + 1, 0), w - 1)));
                }
            }
        }
    };
    const float *wk = weight + (long)c * DW_K * DW_K;
    const float bc = bias ? bias[c] : 0.0f, sc = scale ? scale[c] : 1.0f, sh = shift ? shift[c] : 0.0f;
    // r5: a thread owns FOUR rows x FOUR columns (r2-r4: two rows x eight): its two output row pairs A = (4t, 4t+1) and
    // B = (4t+2, 4t+3) share seven of the nine input row-pair lines they need, so each line is read once and used for both (27
    // ds_read_b128 per item instead of 56), and a store instruction's 16 lanes of a row write 256 contiguous bytes (the eight-column
    // form stored 16-byte pieces 32 bytes apart, twice)
    const int t = tid / SH::CG, tg = tid - t * SH::CG;  // output rows 4t .. 4t+3, columns 4 tg .. 4 tg + 3
    issue_loads(b_first);
    for (int b = b_first; b < b_end; ++b) {
#pragma unroll
        for (int k = 0; k < KI; ++k) asm volatile("" : "+v"(ld[k][0]), "+v"(ld[k][1]), "+v"(ld[k][2]));
#pragma unroll
        for (int k = 0; k < KI; ++k) {
            const int i = tid + 256 * k;
            const int p = i / NQ, q = i - p * NQ;
            const int xx = x0 - 4 + 2 * q;
            const bool iok = i < NITEM;
            f32x2 rv[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int yy = y0 - DW_R + 2 * p + e;
                const bool yok = yy >= 0 && yy < h && iok;
                rv[e][0] = (yok && xx >= 0 && xx < w) ? (float)ld[k][e][0] : 0.0f;
                rv[e][1] = (yok && xx + 1 >= 0 && xx + 1 < w) ? (float)ld[k][e][1] : 0.0f;
                if (relu_in) rv[e] = __builtin_elementwise_max(rv[e], f32x2{0.0f, 0.0f});
            }
            if (iok) {
                float *d = tile + (p * DW_LW + 2 * q) * 2;
                *(f32x4 *)d = f32x4{rv[0][0], rv[1][0], rv[0][1], rv[1][1]};
                *(f32x4 *)(d + DW_IMG) = f32x4{rv[1][0], rv[2][0], rv[1][1], rv[2][1]};
            }
        }
        // LDS-only barriers: __syncthreads() is also a release fence for GLOBAL memory -- it would wait out the previous
        // item's output stores (s_waitcnt vmcnt(0)) in front of every barrier
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (b + 1 < b_end) issue_loads(b + 1);  // in flight under this item's arithmetic
        if (t < DW_TY / 4) {
            f32x2 accA[4], accB[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) accA[j] = accB[j] = f32x2{0.0f, 0.0f};
#pragma unroll
            for (int m = 0; m < DW_K + 2; ++m) {
                // line m = input rows (4t + m, 4t + m + 1): pair 2t + m/2 of E (m even) or pair 2t + (m-1)/2 of O (m odd); it is
                // kernel row m of output pair A and kernel row m - 2 of pair B.  Output column 4 tg + j, tap kx reads LDS column
                // 4 tg + j + kx + 1 (LDS column 0 is image column x0 - 4): columns 4 tg .. 4 tg + 11 = three aligned b128
                const float *row = tile + ((m & 1) ? DW_IMG : 0) + ((2 * t + (m >> 1)) * DW_LW + 4 * tg) * 2;
                // (ties the reads of this line behind the previous line's arithmetic: the fully unrolled loop otherwise holds all
                // the reads in flight and the register count halves the occupancy)
                asm volatile("" : "+v"(accA[0]), "+v"(accA[1]), "+v"(accA[2]), "+v"(accA[3]), "+v"(accB[0]), "+v"(accB[1]), "+v"(accB[2]), "+v"(accB[3])::"memory");
                f32x2 win[12];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const f32x4 u = *(const f32x4 *)(row + 4 * i);
                    win[2 * i] = f32x2{u[0], u[1]};
                    win[2 * i + 1] = f32x2{u[2], u[3]};
                }
                if (m < DW_K) {
#pragma unroll
                    for (int kx = 0; kx < DW_K; ++kx) {
                        const float wv = wk[m * DW_K + kx];
                        const f32x2 w2 = {wv, wv};
#pragma unroll
                        for (int j = 0; j < 4; ++j) accA[j] = __builtin_elementwise_fma(win[kx + j + 1], w2, accA[j]);
                    }
                }
                if (m >= 2) {
#pragma unroll
                    for (int kx = 0; kx < DW_K; ++kx) {
                        const float wv = wk[(m - 2) * DW_K + kx];
                        const f32x2 w2 = {wv, wv};
#pragma unroll
                        for (int j = 0; j < 4; ++j) accB[j] = __builtin_elementwise_fma(win[kx + j + 1], w2, accB[j]);
                    }
                }
            }
            const int x = x0 + 4 * tg;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int y = y0 + 4 * t + e;
                if (y >= h) continue;
                TO *dst = (TO *)((char *)(out + ((long)b * C + c) * plane) + OB * (unsigned)(y * w + x));
                float r[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float o = fmaf((e < 2 ? accA[j][e] : accB[j][e - 2]) + bc, sc, sh);
                    if constexpr (OB == 2) r[j] = f16_sat(relu ? f16_relu(o) : o);
                    else r[j] = relu ? fmaxf(o, 0.0f) : o;
                }
                if constexpr (OB == 2) {
                    // the thread's four columns leave as one 8-byte store (rows of halves are 4-byte aligned: w is even); the
                    // plane's last column group holds four columns or two
                    const f16x4 r16 = __builtin_convertvector((f32x4){r[0], r[1], r[2], r[3]}, f16x4);
                    if (x + 3 < w) *(f16x4 *)dst = r16;
                    else if (x + 1 < w) *(f16x2 *)dst = f16x2{r16[0], r16[1]};
                    continue;
                }
                if (FAST && x + 3 < w) {  // w even, plane 8-byte aligned: float2 stores are always aligned
#pragma unroll
                    for (int j = 0; j < 4; j += 2) *(f32x2 *)(dst + j) = f32x2{r[j], r[j + 1]};
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x + j < w) dst[j] = r[j];
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the next item's staging overwrites the tile)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
}

template <bool FAST, bool RELU_IN, bool RELU>
__global__ __launch_bounds__(256, FAST ? 4 : 3) void dwconv7x7_bn_relu_kernel(const float *__restrict__ in, int B, int C, int h, int w,
                                                                   const float *__restrict__ weight,
                                                                   const float *__restrict__ bias,
                                                                   const float *__restrict__ scale,
                                                                   const float *__restrict__ shift,
                                                                   float *__restrict__ out, int per_item, int ntx, int nty,
                                                                   int nstd, int ntile_)
{
    // XCD-aware block map (r5): block L runs on XCD L % 8; all tiles of a plane go to ONE XCD (plane z = 8 g + L % 8), so the halo
    // rows / columns two neighbouring tiles share are hits in that XCD's L2 and the cache lines a tile boundary cuts (rows are
    // 856 bytes at 480p: no tile edge is line-aligned) are completed in one L2 before they are written back.  r2-r4: a 3-D grid,
    // tile index fastest -- the eight tiles of a plane sat on eight XCDs.
    // Tiles of a plane (r6): `nstd` standard 60 x 64 tiles over the first ntx (- 1) tile columns, then -- when the last column holds at
    // most 24 image columns -- 120 x 24 tiles for that strip (nstd < ntile_), else nstd == ntile_ == ntx * nty.
    const int xcd_ = blockIdx.x & 7, j_ = blockIdx.x >> 3;
    const int tile_ = j_ % ntile_, bz = (j_ / ntile_) * 8 + xcd_;
    if (bz >= (per_item ? B * C : C)) return;
    // E: element (r, col) at ((r >> 1) * LW + col) * 2 + (r & 1), r = row - (y0 - 3); O: the same for r - 1
    __shared__ __attribute__((aligned(16))) float tile[2 * DW_IMG];
    // per_item (r4): few channels (layer 1's 3 per-object ones: 24 workgroups walking 3 items each = 3 serial round trips on a
    // tenth of the chip) -- a workgroup per (tile, channel, batch item) instead of the batch walk
    const int c = per_item ? bz % C : bz;
    const int b_first = per_item ? bz / C : 0, b_end = per_item ? b_first + 1 : B;
    if (tile_ < nstd) {
        const int ncol = nstd / nty;  // standard tile columns
        const int bx = tile_ % ncol, by = tile_ / ncol;
        dw_tile<DwStd, FAST, RELU_IN, RELU>(tile, in, C, h, w, weight, bias, scale, shift, out, c, b_first, b_end, bx * DwStd::TX,
                                            by * DwStd::TY);
    } else {
        dw_tile<DwNarrow, FAST, RELU_IN, RELU>(tile, in, C, h, w, weight, bias, scale, shift, out, c, b_first, b_end,
                                               (nstd / nty) * DwStd::TX, (tile_ - nstd) * DwNarrow::TY);
    }
}

// head_act="f16": the same stage with its output -- and, behind layer 1, its input -- stored as fp16: the FAST (even w) form,
// relu on, the same block map, batch walk and tiles; dw_tile's fp32 LDS image and fmaf chain, so the result is the fp32 kernel's,
// saturated at 65504 and rounded once.
template <bool IN16>
__global__ __launch_bounds__(256, 4) void dwconv7x7_bn_relu_f16_kernel(const void *__restrict__ in, int B, int C, int h, int w,
                                                                     const float *__restrict__ weight, const float *__restrict__ bias,
                                                                     const float *__restrict__ scale, const float *__restrict__ shift,
                                                                     _Float16 *__restrict__ out, int per_item, int ntx, int nty, int nstd,
                                                                     int ntile_)
{
    typedef typename std::conditional<IN16, _Float16, float>::type TI;
    const int xcd_ = blockIdx.x & 7, j_ = blockIdx.x >> 3;
    const int tile_ = j_ % ntile_, bz = (j_ / ntile_) * 8 + xcd_;
    if (bz >= (per_item ? B * C : C)) return;
    __shared__ __attribute__((aligned(16))) float tile[2 * DW_IMG];
    const int c = per_item ? bz % C : bz;
    const int b_first = per_item ? bz / C : 0, b_end = per_item ? b_first + 1 : B;
    if (tile_ < nstd) {
        const int ncol = nstd / nty;
        const int bx = tile_ % ncol, by = tile_ / ncol;
        dw_tile<DwStd, true, false, true, TI, _Float16>(tile, (const TI *)in, C, h, w, weight, bias, scale, shift, out, c, b_first, b_end,
                                                        bx * DwStd::TX, by * DwStd::TY);
    } else {
        dw_tile<DwNarrow, true, false, true, TI, _Float16>(tile, (const TI *)in, C, h, w, weight, bias, scale, shift, out, c, b_first,
                                                           b_end, (nstd / nty) * DwStd::TX, (tile_ - nstd) * DwNarrow::TY);
    }
}

// DynamicSegHead's output layer (IntVOS.py:519,525: conv = Conv2d(embed_dim, 1, 1) applied to layer4's ReLU output):
//   out[b][p] = bias + sum_c w[c] * max(in[b][c][p], 0)
// a pure stream over the [B][C][HW] activation (79 MB at [3,256,120,214]: 10 us at 8 TB/s).  The framework runs it as
// clamp (22 us) + two layout transposes (31 us) + an implicit-GEMM with N = 1 (19 us).  Here: a workgroup owns 256 pixels
// (64 lanes x float4), its 4 waves split the channels; 8 independent float4 loads in flight per lane; the waves' partial
// sums meet in LDS.  Per output the sum is ((w0 + w1) + (w2 + w3)) of four ascending fmaf chains.
constexpr int RC_WAVES = 4;
__global__ __launch_bounds__(64 * RC_WAVES) void relu_conv1x1_c1_kernel(const float *__restrict__ in, int C, long HW,
                                                                       const float *__restrict__ weight,
                                                                       const float *__restrict__ bias, int relu_in,
                                                                       float *__restrict__ out)
{
    __shared__ f32x4 part[RC_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const long p0 = ((long)blockIdx.x * 64 + lane) * 4;
    const bool vec = (HW % 4 == 0) && p0 + 3 < HW;  // rows of whole float4 (16-byte aligned planes)
    const float *src = in + (long)b * C * HW;
    const int cper = (C + RC_WAVES - 1) / RC_WAVES, c0 = wave * cper, c1 = (c0 + cper < C) ? c0 + cper : C;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (vec) {
        int c = c0;
        for (; c + 8 <= c1; c += 8) {
            f32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *(const f32x4 *)(src + (long)(c + u) * HW + p0);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float wv = weight[c + u];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(relu_in ? fmaxf(v[u][j], 0.0f) : v[u][j], wv, acc[j]);
            }
        }
        for (; c < c1; ++c) {
            const f32x4 v = *(const f32x4 *)(src + (long)c * HW + p0);
            const float wv = weight[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(relu_in ? fmaxf(v[j], 0.0f) : v[j], wv, acc[j]);
        }
    } else {
        for (int c = c0; c < c1; ++c) {
            const float wv = weight[c];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (p0 + j < HW) {
                    const float v = src[(long)c * HW + p0 + j];
                    acc[j] = fmaf(relu_in ? fmaxf(v, 0.0f) : v, wv, acc[j]);
                }
            }
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) {
        const f32x4 s01 = part[0][lane] + part[1][lane], s23 = part[2][lane] + part[3][lane];
        const float bz = bias ? bias[0] : 0.0f;
        const f32x4 r = (s01 + s23) + f32x4{bz, bz, bz, bz};
        float *dst = out + (long)b * HW + p0;
        if (vec) *(f32x4 *)dst = r;
        else
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p0 + j < HW) dst[j] = r[j];
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// The 1x1 convolution of a _split_separable_conv2d (IntVOS.py:494,503-505: conv2 -> bn2 [-> relu2]) as an fp32-MFMA
// contraction (VERDICT r2 "next" #3: r2 left it to the framework's GEMM -- 108 us of kernel + layout transposes per block
// at [3,256,120,214], 45 % of an end-to-end frame):
//     out[b][co][p] = b2[co] + sum_ci w2t[ci][co] * in[b][ci][p]          (bn2 folded into w2t / b2; optional ReLU)
// v_mfma_f32_32x32x2_f32 is an exact fp32 fmaf chain in ascending ci.  A 1x1 convolution has no halo, so a tile is 64
// CONSECUTIVE pixels of one batch item's flat [h*w] plane: every operand row is a contiguous 256-byte run and arrives by
// LDS-DMA (no VGPR staging, no address arithmetic), every output store is 32 consecutive pixels = one full 128-byte line.
//   workgroup = 4 waves = all 256 output channels x 64 pixels; a wave owns 64 channels (2 x 2 blocks, 64 accumulator VGPRs)
//   chunk     = 16 input channels: in-slice [16][64] (4 KiB) + weight slice [16][256] (16 KiB), double buffered; per chunk a
//               wave issues 5 DMA pieces and 8 k-steps x 4 MFMAs, both operands one dword per lane from LDS (conflict-free)
//   41 KiB of LDS, 114 VGPRs: three workgroups per CU.
// Measured at [3,256,120,214] (tools/pw_bench.py): 109-111 us = 0.58 of the fp32 matrix peak (the framework's GEMM incl. its
// layout transposes: 131-134 us).  What was tried on top and did not move it: wave-private DMA pipelines without any barrier
// in the loop (120 us), a persistent form that defers a tile's stores into the next tile's MFMA loop (111 us), operand
// reads pinned one k-step ahead (hipcc already overlaps them with the previous k-step's MFMAs).  Ablations: the bare MFMA
// loop 84 us, + DMA 94, + epilogue 109: the workgroups of a launch start together and stay in phase, so the memory phases
// (79 MB in, 79 MB out, in 256-byte row pieces) mostly run with the matrix pipe idle.
// (the fused depthwise + 1x1 kernel built first in r3 -- depthwise waves feeding matrix waves through LDS, one 4 x 16-pixel
// tile per workgroup -- was correct but 2-3x SLOWER than the two-kernel path: the 7x7 halo makes its input 3.4x the tile in
// 88-byte row pieces, and with 95 KiB of LDS only one workgroup fits a CU, so every tile's prologue and epilogue -- 78 us of
// a launch, measured -- ran exposed)
constexpr int PW_P = 64, PW_KC = 16, PW_CO = 256, PW_NT = 256;
__global__ __launch_bounds__(PW_NT, 3) void conv1x1_mfma_kernel(const float *__restrict__ in, long in_bs, int Cin, long HW,
                                                                const float *__restrict__ w2t,
                                                                const float *__restrict__ b2, int relu_out,
                                                                float *__restrict__ out, const float *__restrict__ head_w,
                                                                const float *__restrict__ head_b,
                                                                float *__restrict__ head_out, const float *__restrict__ add)
{
    __shared__ __attribute__((aligned(1024))) float wbuf[2][PW_KC * PW_CO];
    __shared__ __attribute__((aligned(1024))) float xbuf[2][PW_KC * PW_P];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long p0 = (long)blockIdx.x * PW_P;
    const int b = blockIdx.y;
    const float *src = in + (long)b * in_bs;
    const int n = (Cin + PW_KC - 1) / PW_KC;  // any Cin >= 1 (r4): the last chunk may hold 1 .. 16 channels
    const unsigned wbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)&wbuf[0][0]);
    const unsigned xbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)&xbuf[0][0]);
    // in-slice piece of this wave: channels 4 wave .. 4 wave + 3 of the chunk, lane -> (channel lane / 16, pixels 4 (lane % 16) ..)
    long pix = p0 + 4 * (lane & 15);
    if (pix > HW - 4) pix = HW - 4;  // the plane's last tile: clamped columns are computed and never stored
    auto dma = [&](int c, int buf) __attribute__((always_inline)) {
        const int k0 = c * PW_KC, kn = (Cin - k0) < PW_KC ? (Cin - k0) : PW_KC;  // channels of this chunk
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wave * 4 + i;  // weight row = 1 KiB piece
            if (row < kn)
                lds_dma16(w2t + (long)(k0 + row) * PW_CO + lane * 4, wbase + (unsigned)buf * (unsigned)(PW_KC * PW_CO * 4) + (unsigned)row * 1024u);
        }
        if (wave * 4 < kn) {
            // (rows past Cin inside a piece -- layer 1's per-object half has 3 channels -- are not fetched: their lanes sit the
            // DMA out, the LDS rows keep zero_tail's zeros (one chunk) or an earlier chunk's values, against zero weight rows)
            const int ch = k0 + wave * 4 + (lane >> 4);
            if (ch < Cin)
                lds_dma16(src + (long)ch * HW + pix, xbase + (unsigned)buf * (unsigned)(PW_KC * PW_P * 4) + (unsigned)wave * 1024u);
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    const int co0 = wave * 64;
    __shared__ float bsh[PW_CO];
    bsh[tid] = b2[tid];  // the folded bias, read back in the epilogue (a global load per output would serialise it)
    const int tail = Cin - (n - 1) * PW_KC;  // channels of the last chunk: 1 .. 16
    // A partial last chunk multiplies all 16 rows like the others (no branch in the MFMA loop: a branch per k-step keeps
    // hipcc from overlapping a k-step's LDS reads with the previous k-step's MFMAs): its missing weight rows are ZERO in LDS,
    // so whatever finite in-slice rows an earlier chunk left there contribute nothing.  (n <= 2: the last chunk is the FIRST
    // use of its buffer -- its in-slice rows past the tail were never written and hold whatever the previous kernel left in
    // LDS, NaN bit patterns included; they are zeroed too.  r4 did that for n == 1 only: Cin in 17..32 multiplied
    // uninitialised LDS by zero -- found in r5 when another kernel's LDS image changed.)
    auto zero_tail = [&](int buf) __attribute__((always_inline)) {
        for (int i = tid; i < (PW_KC - tail) * PW_CO; i += PW_NT) wbuf[buf][tail * PW_CO + i] = 0.0f;
        if (n <= 2)
            for (int i = tid; i < (PW_KC - tail) * PW_P; i += PW_NT) xbuf[buf][tail * PW_P + i] = 0.0f;
    };
    dma(0, 0);
    if (n == 1 && tail < PW_KC) zero_tail(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int c = 0; c < n; ++c) {
        if (c + 1 < n) {
            dma(c + 1, (c + 1) & 1);  // (its buffer was last read in iteration c - 1: everyone is past that barrier)
            if (c + 2 == n && tail < PW_KC) zero_tail((c + 1) & 1);
        }
        const float *Wt = &wbuf[c & 1][(lane >> 5) * PW_CO + co0 + (lane & 31)];
        const float *X = &xbuf[c & 1][(lane >> 5) * PW_P + (lane & 31)];
#pragma unroll
        for (int kk = 0; kk < PW_KC / 2; ++kk) {
            const float a0 = Wt[2 * kk * PW_CO], a1 = Wt[2 * kk * PW_CO + 32];
            const float x0 = X[2 * kk * PW_P], x1 = X[2 * kk * PW_P + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, x0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, x1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, x0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, x1, acc[1][1], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // C/D layout: column = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel)
    if (head_w) {
        // DynamicSegHead's output layer fused in (IntVOS.py:519,525: conv = Conv2d(256, 1, 1) on layer4's ReLU output):
        //   head_out[b][p] = head_b + sum_co head_w[co] * max(acc[co][p] + b2[co], 0)
        // the [B,256,h,w] activation of layer4 is neither written nor read back.  Per pixel: each lane sums its 32
        // channels (ascending fmaf chain), the two lane halves meet by a shuffle, the four waves in LDS.
        float *red = &xbuf[0][0];  // (free: everyone is past the loop's last barrier)
        float sp[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            float a = 0.0f;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    a = fmaf(fmaxf(acc[cb][pb][r] + bsh[co], 0.0f), head_w[co], a);
                }
            sp[pb] = a + __shfl_xor(a, 32);
        }
        if (lane < 32) {
            red[wave * PW_P + lane] = sp[0];
            red[wave * PW_P + 32 + lane] = sp[1];
        }
        __syncthreads();
        if (tid < PW_P && p0 + tid < HW)
            head_out[(long)b * HW + p0 + tid] =
                ((red[tid] + red[PW_P + tid]) + (red[2 * PW_P + tid] + red[3 * PW_P + tid])) + (head_b ? head_b[0] : 0.0f);
        return;
    }
    float *dst = out + (long)b * PW_CO * HW;
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
        const long p = p0 + pb * 32 + (lane & 31);
        if (p >= HW) continue;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                float v = acc[cb][pb][r] + bsh[co];
                if (add) v += add[(long)co * HW + p];  // layer 1's shared-embedding half, the same for every batch item
                if (relu_out) v = fmaxf(v, 0.0f);
                dst[(long)co * HW + p] = v;
            }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// The same 1x1 stage in SPLIT-bf16 arithmetic (r3b): every fp32 factor is taken as hi + lo, two bf16 pieces (16
// significand bits), and a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- the
// dropped lo*lo term and the pieces' own rounding are <= 2^-16 relative per product (measured against the fp32-MFMA kernel:
// tests/test_seg_head.py; for comparison, the reference's cuDNN path runs these layers in TF32 -- 10 significand bits --
// wherever torch.backends.cudnn.allow_tf32 is left at its default).  The bf16 pipe retires a 32x32x16 block in 8 passes,
// so the three products cost 3/16 of the fp32 pipe's time for the same block: the stage stops being matrix-bound
// (fp32 kernel: 68 us of MFMA in a 111 us launch at 3 objects) and becomes what a 1x1 layer should be -- a stream: read
// the activation once, write it once.
//   workgroup = 128 pixels x 256 output channels, 4 waves = (pixel half) x (channel half), 128 accumulators per lane;
//   weights: packed ONCE per fold (conv1x1_x3_pack_kernel) as the MFMA A operand, hi and lo, 16 KiB per 16 input channels,
//     LDS-DMA'd chunk by chunk (shared by the 4 waves);
//   activation: LDS-DMA'd as fp32 rows [16 k][128 px]; each lane reads its 8 k of a pixel column and splits them in
//     registers (v_cvt_pk_bf16_f32: 5 VALU per pair) -- the depthwise kernel keeps writing plain fp32.
//   any Cin >= 1 (rows past Cin are clamped reads against zero weight rows); h*w a multiple of 4 (16-byte DMA rows).
//   `add` (layer1's shared-embedding half, [256][HW], the same for every batch entry) and the bias join in the epilogue.
constexpr int X3_P = 128, X3_KC = 16, X3_NT = 256, X3_WCHUNK = 2 * 8 * 1024, X3_NB = 2;
typedef __bf16 x3_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 x3_bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void x3_split(float x0, float x1, unsigned &hi, unsigned &lo)
{
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){x0, x1}, x3_bf16x2));
    const float h0 = __uint_as_float(hi << 16), h1 = __uint_as_float(hi & 0xffff0000u);
    float l0, l1;  // two scalar subtractions on purpose: hipcc packs them into v_pk_add_f32 + two v_mov otherwise
    asm("v_sub_f32 %0, %1, %2" : "=v"(l0) : "v"(x0), "v"(h0));
    asm("v_sub_f32 %0, %1, %2" : "=v"(l1) : "v"(x1), "v"(h1));
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){l0, l1}, x3_bf16x2));
}

// three pieces (r4, "split3"): x = hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid): 24 significand
// bits -- every fp32 value is represented exactly (up to bf16's exponent range at the low end)
__device__ __forceinline__ void x3_split3(float x0, float x1, unsigned &hi, unsigned &mid, unsigned &lo)
{
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){x0, x1}, x3_bf16x2));
    const float h0 = __uint_as_float(hi << 16), h1 = __uint_as_float(hi & 0xffff0000u);
    float r0, r1;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r0) : "v"(x0), "v"(h0));
    asm("v_sub_f32 %0, %1, %2" : "=v"(r1) : "v"(x1), "v"(h1));
    mid = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){r0, r1}, x3_bf16x2));
    const float m0 = __uint_as_float(mid << 16), m1 = __uint_as_float(mid & 0xffff0000u);
    float l0, l1;
    asm("v_sub_f32 %0, %1, %2" : "=v"(l0) : "v"(r0), "v"(m0));
    asm("v_sub_f32 %0, %1, %2" : "=v"(l1) : "v"(r1), "v"(m1));
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){l0, l1}, x3_bf16x2));
}

// w2t [Cin][256] fp32 -> A-operand image [chunk][hi | (mid |) lo][co block 8][lane 64] x 16 bytes; lane l of block b holds
// output channel 32 b + (l & 31), input channels 16 chunk + 8 (l >> 5) + 0..7 (zero past Cin).  NP = pieces (2 or 3)
template <int NP>
__global__ __launch_bounds__(256) void conv1x1_x3_pack_kernel(const float *__restrict__ w2t, int Cin, uint4 *__restrict__ wpk, int n_chunks)
{
    const int item = blockIdx.x * 256 + threadIdx.x;  // (chunk, block, lane)
    if (item >= n_chunks * 8 * 64) return;
    const int lane = item & 63, blk = (item >> 6) & 7, c = item >> 9;
    const int co = 32 * blk + (lane & 31), k0 = 16 * c + 8 * (lane >> 5);
    unsigned hi[4], mid[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ka = k0 + 2 * j, kb = ka + 1;
        const float a = ka < Cin ? w2t[(long)ka * PW_CO + co] : 0.0f, b = kb < Cin ? w2t[(long)kb * PW_CO + co] : 0.0f;
        if (NP == 3) x3_split3(a, b, hi[j], mid[j], lo[j]);
        else x3_split(a, b, hi[j], lo[j]);
    }
    uint4 *dst = wpk + (long)c * (NP * 8 * 1024 / 16) + blk * 64 + lane;
    dst[0] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    if (NP == 3) dst[8 * 64] = make_uint4(mid[0], mid[1], mid[2], mid[3]);
    dst[(NP - 1) * 8 * 64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// NP = 3 ("split3", r4): three pieces per factor, SIX products per pair -- hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi, the
// dropped ones (mid*lo, lo*mid, lo*lo) below 2^-24 of the product: fp32-class results (each product good to ~2^-23, the sum in
// fp32) at 6/16 of the fp32 pipe's time.  24 KiB of weights per chunk: 64 KiB of LDS, two workgroups per CU.
template <int NP = 2>
__global__ __launch_bounds__(X3_NT, NP == 3 ? 2 : 3) void conv1x1_x3_kernel(const float *__restrict__ in, long in_bs, int Cin, long HW,
                                                              const char *__restrict__ wpk, const float *__restrict__ b2,
                                                              const float *__restrict__ add, int relu_out,
                                                              float *__restrict__ out, const float *__restrict__ head_w,
                                                              const float *__restrict__ head_b, float *__restrict__ head_out)
{
    constexpr int WCHUNK = NP * 8 * 1024;
    __shared__ __attribute__((aligned(1024))) char wbuf[X3_NB][WCHUNK];
    __shared__ __attribute__((aligned(1024))) float xbuf[X3_NB][X3_KC * X3_P];
    // (the folded bias: its own 1 KiB for two pieces; with three the 64 KiB are full -- it moves into the weight ring once the
    // loop is done with it)
    float *bsh;
    if constexpr (NP == 3) {
        bsh = (float *)&wbuf[0][0];
    } else {
        __shared__ float bsh_own[PW_CO];
        bsh = bsh_own;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wave & 1, wc = wave >> 1;  // pixel half, output-channel half
    const long p0 = (long)blockIdx.x * X3_P;
    const int b = blockIdx.y;
    const float *src = in + (long)b * in_bs;
    const int n = (Cin + X3_KC - 1) / X3_KC;
    const unsigned wbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)&wbuf[0][0]);
    const unsigned xbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)&xbuf[0][0]);
    long pix = p0 + 4 * (lane & 31);
    if (pix > HW - 4) pix = HW - 4;  // the plane's last tile: clamped columns are computed and never stored
    // chunk c -> ring slot c % X3_NB; 6 pieces per wave (4 weight + 2 activation).  Chunks are fetched TWO steps ahead and
    // a step waits with vmcnt(6) -- the chunk issued in this step stays in flight: a step's matrix work (~0.6 us) is
    // shorter than a fetch, even of the L2-resident weights (first form, one step ahead with vmcnt(0): every step waited
    // out a whole fetch, 54 us).
    auto dma = [&](int c) __attribute__((always_inline)) {
        const unsigned slot = (unsigned)(c % X3_NB);
#pragma unroll
        for (int i = 0; i < 2 * NP; ++i) {
            const int piece = wave * (2 * NP) + i;
            lds_dma16(wpk + (long)c * WCHUNK + piece * 1024 + lane * 16, wbase + slot * (unsigned)WCHUNK + (unsigned)piece * 1024u);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int piece = wave * 2 + i;  // input rows 2 piece, 2 piece + 1 of the chunk
            int row = c * X3_KC + 2 * piece + (lane >> 5);
            row = row < Cin ? row : Cin - 1;  // past Cin: any finite row (its weights are zero)
            lds_dma16(src + (long)row * HW + pix, xbase + slot * (unsigned)(X3_KC * X3_P * 4) + (unsigned)piece * 1024u);
        }
    };
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    if (NP != 3) bsh[tid] = b2[tid];
    // chunks are fetched X3_NB - 1 steps ahead; a step waits for everything but the chunks issued behind its successor
    dma(0);
    if (X3_NB == 3 && n > 1) {
        dma(1);
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#define X3_MFMA(a_, b_, c_) c_ = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(x3_bf16x8, a_), __builtin_bit_cast(x3_bf16x8, b_), c_, 0, 0, 0)
    for (int c = 0; c < n; ++c) {
        const bool more = c + X3_NB - 1 < n;
        if (more) dma(c + X3_NB - 1);  // (its slot was last read in iteration c - 1: everyone is past that barrier)
        const float *X = &xbuf[c % X3_NB][8 * (lane >> 5) * X3_P + wq * 64 + (lane & 31)];
        uint4 bh[2], bl[2], bm[NP == 3 ? 2 : 1];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = X[j * X3_P + pb * 32];
            if (NP == 3) {
                x3_split3(v[0], v[1], bh[pb].x, bm[pb].x, bl[pb].x);
                x3_split3(v[2], v[3], bh[pb].y, bm[pb].y, bl[pb].y);
                x3_split3(v[4], v[5], bh[pb].z, bm[pb].z, bl[pb].z);
                x3_split3(v[6], v[7], bh[pb].w, bm[pb].w, bl[pb].w);
            } else {
                x3_split(v[0], v[1], bh[pb].x, bl[pb].x);
                x3_split(v[2], v[3], bh[pb].y, bl[pb].y);
                x3_split(v[4], v[5], bh[pb].z, bl[pb].z);
                x3_split(v[6], v[7], bh[pb].w, bl[pb].w);
            }
        }
        const uint4 *W = (const uint4 *)&wbuf[c % X3_NB][0] + (wc * 4) * 64 + lane;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            const uint4 ah = W[blk * 64], al = W[((NP - 1) * 8 + blk) * 64];
            if (NP == 3) {  // smallest terms first: (hi*lo, lo*hi, mid*mid), then (hi*mid, mid*hi), then hi*hi
                const uint4 am = W[(8 + blk) * 64];
#pragma unroll
                for (int pb = 0; pb < 2; ++pb) {
                    X3_MFMA(ah, bl[pb], acc[blk][pb]);
                    X3_MFMA(al, bh[pb], acc[blk][pb]);
                    X3_MFMA(am, bm[pb], acc[blk][pb]);
                    X3_MFMA(ah, bm[pb], acc[blk][pb]);
                    X3_MFMA(am, bh[pb], acc[blk][pb]);
                    X3_MFMA(ah, bh[pb], acc[blk][pb]);
                }
                continue;
            }
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                X3_MFMA(ah, bl[pb], acc[blk][pb]);
                X3_MFMA(al, bh[pb], acc[blk][pb]);
                X3_MFMA(ah, bh[pb], acc[blk][pb]);
            }
        }
        if (more && X3_NB == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#undef X3_MFMA
    if (NP == 3) {  // (everyone is past the loop's last barrier: the weight ring is free)
        bsh[tid] = b2[tid];
        __syncthreads();
    }
    // C/D layout: column = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel)
    const int co0 = wc * 128;
    if (head_w) {  // DynamicSegHead's output layer fused in (see conv1x1_mfma_kernel)
        float *red = &xbuf[0][0];
        float sp[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            float a = 0.0f;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    a = fmaf(fmaxf(acc[cb][pb][r] + bsh[co], 0.0f), head_w[co], a);
                }
            sp[pb] = a + __shfl_xor(a, 32);
        }
        if (lane < 32) {
            red[wc * X3_P + wq * 64 + lane] = sp[0];
            red[wc * X3_P + wq * 64 + 32 + lane] = sp[1];
        }
        __syncthreads();
        if (tid < X3_P && p0 + tid < HW)
            head_out[(long)b * HW + p0 + tid] = (red[tid] + red[X3_P + tid]) + (head_b ? head_b[0] : 0.0f);
        return;
    }
    float *dst = out + (long)b * PW_CO * HW;
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
        const long p = p0 + wq * 64 + pb * 32 + (lane & 31);
        if (p >= HW) continue;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                float v = acc[cb][pb][r] + bsh[co];
                if (add) v += add[(long)co * HW + p];
                if (relu_out) v = fmaxf(v, 0.0f);
                dst[(long)co * HW + p] = v;
            }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// The 1x1 stage of head_act="f16": fp16 activation in, fp16 activation (or the fused fp32 logits) out, the folded weight rounded
// once to fp16: exact fp16 x fp16 products on v_mfma_f32_32x32x16_f16, fp32 accumulators, an fp32 epilogue (+ b2, + the fp32
// `add` term, ReLU) and one rounding at the store: rn16(min(., 65504)), a NaN kept.  One MFMA per 32 x 32 x 16 block where the
// split kernel spends three and a register-side split, and half the bytes each way.
//   workgroup = 128 pixels x 256 output channels, 4 waves = (pixel half) x (channel half), 128 accumulators per lane;
//   weights: packed once per fold (conv1x1_f16_pack_kernel) as the MFMA operand image [chunk][co block 8][lane 64] x 16 bytes
//     (conv1x1_x3_pack_kernel's layout, one piece), 8 KiB per 16 input channels, LDS-DMA'd chunk by chunk;
//   activation: rows [16 k][128 px] of halves arrive by 16-byte LDS-DMA (h*w a multiple of 8) and are read TRANSPOSED
//     (ds_read_b64_tr_b16: two reads give a lane the 8 k of its pixel column).  The DMA's lanes choose WHICH 16 bytes they fetch,
//     so the LDS image is laid out for those reads at no cost: chunk ch of row r sits at 256 r + 16 (ch ^ (((r & 3) << 2) |
//     ((r >> 2) & 3))) -- plain 256-byte rows are 4-way conflicts for the transposed read.  Every lane holds a valid address at
//     every read (EXEC is all ones in the loop: no early return, no lane-dependent branch in front of it);
//   ring of 4 chunk slots, fetched three steps ahead; a step waits with a counted vmcnt (the younger chunks stay in flight) and
//     meets the others at a raw s_barrier behind lgkmcnt(0) -- __syncthreads() would drain the DMA queue;
//   operand order by form: HEAD (fused logits) -- weights as A, so a lane owns a pixel and its channels sit in its registers, as
//     in conv1x1_x3_kernel; else the ACTIVATION as A -- a lane owns a channel and 4 consecutive pixels per register quad, which
//     leave as one 8-byte store (no lane ever stores a single half), the fp32 term arrives as one 16-byte load.
//   any Cin >= 1 (rows past Cin are clamped reads against zero weight rows); the plane's last tile computes clamped columns
//   that are never stored.
constexpr int H16_P = 128, H16_KC = 16, H16_NT = 256, H16_NB = 4, H16_WCHUNK = 8 * 1024, H16_XCHUNK = H16_KC * H16_P * 2;
typedef short h16_s4 __attribute__((__vector_size__(8)));
typedef __attribute__((address_space(3))) h16_s4 *h16_lds_ptr;

// w2t [Cin][256] fp32 -> [chunk][co block 8][lane 64] x 16 bytes; lane l of block b holds output channel 32 b + (l & 31), input
// channels 16 chunk + 8 (l >> 5) + 0..7, each rounded to nearest-even fp16 (zero past Cin)
__global__ __launch_bounds__(256) void conv1x1_f16_pack_kernel(const float *__restrict__ w2t, int Cin, uint4 *__restrict__ wpk, int n_chunks)
{
    const int item = blockIdx.x * 256 + threadIdx.x;  // (chunk, block, lane)
    if (item >= n_chunks * 8 * 64) return;
    const int lane = item & 63, blk = (item >> 6) & 7, c = item >> 9;
    const int co = 32 * blk + (lane & 31), k0 = 16 * c + 8 * (lane >> 5);
    f16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)(k0 + j < Cin ? w2t[(long)(k0 + j) * PW_CO + co] : 0.0f);
    wpk[item] = __builtin_bit_cast(uint4, v);
}

// OUT32: the result leaves as fp32, unrounded (layer 1's shared-half term, which joins the per-object half in ITS epilogue)
template <bool HEAD, bool OUT32 = false>
__global__ __launch_bounds__(H16_NT, 3) void conv1x1_f16_kernel(const _Float16 *__restrict__ in, long in_bs, int Cin, long HW,
                                                               const char *__restrict__ wpk, const float *__restrict__ b2,
                                                               const float *__restrict__ add, int relu_out,
                                                               void *__restrict__ out, const float *__restrict__ head_w,
                                                               const float *__restrict__ head_b, float *__restrict__ head_out)
{
    __shared__ __attribute__((aligned(1024))) char wbuf[H16_NB][H16_WCHUNK];
    __shared__ __attribute__((aligned(1024))) char xbuf[H16_NB][H16_XCHUNK];
    __shared__ float bsh[PW_CO];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wq = wave & 1, wc = wave >> 1;  // pixel half, output-channel half
    const long p0 = (long)blockIdx.x * H16_P;
    const int b = blockIdx.y;
    const _Float16 *src = in + (long)b * in_bs;
    const int n = (Cin + H16_KC - 1) / H16_KC;
    const unsigned wbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)&wbuf[0][0]);
    const unsigned xbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)&xbuf[0][0]);
    // activation piece of this wave: LDS slots 64 wave .. 64 wave + 63 of the chunk's 256 (16 bytes each); slot s holds row
    // s >> 4, chunk (s & 15) ^ swz(row) -- the lane fetches exactly that
    const int xrow = 4 * wave + (lane >> 4);
    const int xch = (lane & 15) ^ (((xrow & 3) << 2) | ((xrow >> 2) & 3));
    long pix = p0 + 8 * xch;
    if (pix > HW - 8) pix = HW - 8;  // the plane's last tile: clamped columns are computed and never stored
    auto dma = [&](int c) __attribute__((always_inline)) {
        const unsigned slot = (unsigned)(c % H16_NB);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int piece = wave * 2 + i;
            lds_dma16(wpk + (long)c * H16_WCHUNK + piece * 1024 + lane * 16, wbase + slot * (unsigned)H16_WCHUNK + (unsigned)piece * 1024u);
        }
        int row = c * H16_KC + xrow;
        row = row < Cin ? row : Cin - 1;  // past Cin: any row of the input (its weights are zero)
        lds_dma16(src + (long)row * HW + pix, xbase + slot * (unsigned)H16_XCHUNK + (unsigned)wave * 1024u);
    };
    // transposed reads: read t (k = 8 h + 4 t + 0..3) of pixel block pb; 16-lane group g takes rows 8 (g >> 1) + 4 t + q, pixel
    // chunks 8 wq + 4 pb + 2 (g & 1) + (p >> 1), lane 4 q + p of the group the 8 bytes at + 8 (p & 1)
    unsigned xoff[2][2];
    {
        const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                const int r = 8 * (g >> 1) + 4 * t + q, ch = 8 * wq + 4 * pb + 2 * (g & 1) + (p >> 1);
                xoff[t][pb] = 256u * r + 16u * (unsigned)(ch ^ (((r & 3) << 2) | ((r >> 2) & 3))) + 8u * (p & 1);
            }
    }
    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    __shared__ float hsh[HEAD ? PW_CO : 1];  // the output layer's weights (128 global loads per lane in the epilogue spill)
    bsh[tid] = b2[tid];  // (before the first DMA: the wait hipcc puts behind this load must not see the queue)
    if (HEAD) hsh[tid] = head_w[tid];
    // a step needs its chunk landed and leaves the younger ones in flight: 3 pieces per wave and chunk
#define H16_WAIT(younger_)                                                                                             \
    do {                                                                                                               \
        if ((younger_) >= 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                                          \
        else if ((younger_) == 1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");                                     \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                          \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                             \
        __builtin_amdgcn_s_barrier();                                                                                  \
        asm volatile("" ::: "memory");                                                                                 \
    } while (0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    dma(0);
    if (n > 1) dma(1);
    if (n > 2) dma(2);
    H16_WAIT((n < 3 ? n : 3) - 1);
    for (int c = 0; c < n; ++c) {
        if (c + 3 < n) dma(c + 3);  // (its slot was last read in iteration c - 1: everyone is past that barrier)
        const unsigned slot = (unsigned)(c % H16_NB);
        const char *X = &xbuf[0][0] + slot * (unsigned)H16_XCHUNK;
        f16x8 xb[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            const f16x4 lo = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((h16_lds_ptr)(X + xoff[0][pb])));
            const f16x4 hi = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((h16_lds_ptr)(X + xoff[1][pb])));
            xb[pb] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
        const uint4 *W = (const uint4 *)(&wbuf[0][0] + slot * (unsigned)H16_WCHUNK) + (wc * 4) * 64 + lane;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            const f16x8 a = __builtin_bit_cast(f16x8, W[blk * 64]);
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                if (HEAD) acc[blk][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, xb[pb], acc[blk][pb], 0, 0, 0);
                else acc[blk][pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xb[pb], a, acc[blk][pb], 0, 0, 0);
            }
        }
        // chunk c + 1 must have landed; c + 2 and c + 3 may stay in flight
        const int last = (c + 3 < n ? c + 3 : n - 1);
        H16_WAIT(last - (c + 1));
    }
#undef H16_WAIT
    const int co0 = wc * 128;
    if (HEAD) {
        // C/D layout: column = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel); DynamicSegHead's
        // output layer on layer 4's ReLU, in fp32 as in conv1x1_x3_kernel: layer 4's activation is never rounded or written
        float *red = (float *)&xbuf[0][0];  // (free: everyone is past the loop's last barrier)
        float sp[2];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            float a = 0.0f;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                asm volatile("" : "+v"(a)::"memory");  // (a block's 32 LDS reads at a time: all 256 in flight spill)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = co0 + cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    a = fmaf(f16_relu(acc[cb][pb][r] + bsh[co]), hsh[co], a);
                }
            }
            sp[pb] = a + __shfl_xor(a, 32);
        }
        if (lane < 32) {
            red[wc * H16_P + wq * 64 + lane] = sp[0];
            red[wc * H16_P + wq * 64 + 32 + lane] = sp[1];
        }
        __syncthreads();
        if (tid < H16_P && p0 + tid < HW)
            head_out[(long)b * HW + p0 + tid] = (red[tid] + red[H16_P + tid]) + (head_b ? head_b[0] : 0.0f);
        return;
    }
    // C/D layout with the activation as A: column = lane & 31 (output channel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    // (pixel): registers 4 g .. 4 g + 3 are pixels 8 g + 4 (lane >> 5) + 0..3 of the lane's channel -- whole inside the plane or
    // whole outside it (h*w is a multiple of 8)
    const long obase = (long)b * PW_CO * HW;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        const int co = co0 + cb * 32 + (lane & 31);
        const float bz = bsh[co];
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const long p = p0 + wq * 64 + pb * 32 + 8 * g + 4 * (lane >> 5);
                if (p >= HW) continue;
                f32x4 v = {acc[cb][pb][4 * g] + bz, acc[cb][pb][4 * g + 1] + bz, acc[cb][pb][4 * g + 2] + bz, acc[cb][pb][4 * g + 3] + bz};
                if (add) v += *(const f32x4 *)(add + (long)co * HW + p);  // layer 1's shared-embedding half: fp32, unrounded
                if (OUT32) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = relu_out ? f16_relu(v[j]) : v[j];
                    *(f32x4 *)((float *)out + obase + (long)co * HW + p) = v;
                    continue;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = f16_sat(relu_out ? f16_relu(v[j]) : v[j]);
                *(f16x4 *)((_Float16 *)out + obase + (long)co * HW + p) = __builtin_convertvector(v, f16x4);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// DynamicSegHead layer 1, PER-OBJECT half, head_act="f16", ONE launch: the depthwise 7x7 + bn1 + relu1 of the Cp <= 4 per-object
// channels (fp32 planes in, rounded to fp16 as dwconv7x7_bn_relu_f16_kernel<false> stores them) -> their 1x1 (Cp -> 256, bn2 folded)
// + the shared half's fp32 term + relu2 -> the fp16 activation, as conv1x1_f16_kernel<false> stores it:
//   d_c  = rn16(min(relu(fmaf(taps_c + b1[c], scale1[c], shift1[c])), 65504)),  taps_c = the fmaf chain (ky outer, kx inner) from 0
//   acc  = v_mfma_f32_32x32x16_f16 on a zero accumulator: d_c in k slots 0 .. Cp-1, zeros in the others, the weights from the packed
//          HalfWeight image's one chunk (conv1x1_f16_kernel clamps its rows past Cin onto row Cin - 1 against zero weights: products
//          of +0 there and here, the same addends into the same instruction)
//   out[o][co][p] = rn16(min(relu?((acc + b2[co]) + term[co][p]), 65504))
// -- the two kernels' composition operation for operation: the same bits.  What it saves is the general kernel's shape: a K = 256
// pipeline (DMA ring, barriers, 128 x 256 tiles) run for 3 live rows, the term fetched once per OBJECT (26 MB each), and the [n, Cp]
// fp16 planes' round trip through a launch of their own.
// A workgroup owns 64 consecutive pixels of the flattened plane x all 256 output channels (wave = channel quarter: two 32-channel
// blocks x two 32-pixel blocks) and WALKS THE OBJECTS: its 64 KiB of the term are loaded once, 16 x 16 bytes per lane, all in flight
// before anything else, and stay in 64 registers; per object a lane issues 4 MFMAs and 16 8-byte stores.  Activation as the A
// operand, as in conv1x1_f16_kernel: a lane owns an output channel and 4 consecutive pixels per register quad (h*w is a multiple of
// 8: a quad is inside the plane or outside it as a whole; the last tile's term loads are clamped and its outside quads never stored).
// The depthwise stage runs once per tile and object, its taps read straight from the planes (they are 1.4 % of the stage's bytes and
// L2 hits after a tile's first touch; the loads go out behind the term's and land with it), split (object, channel) per wave, and
// reaches the MFMA lanes through a 4 KiB LDS table of L16_OG objects at a time.
constexpr int L16_P = 64, L16_NT = 256, L16_OG = 8;
__global__ __launch_bounds__(L16_NT, 3) void head_layer1_object_f16_kernel(const float *__restrict__ planes, int n, int Cp, int h, int w,
                                                                        const float *__restrict__ w1, const float *__restrict__ b1,
                                                                        const float *__restrict__ sc1, const float *__restrict__ sh1,
                                                                        const uint4 *__restrict__ wpk, const float *__restrict__ b2,
                                                                        const float *__restrict__ term, int relu_out,
                                                                        _Float16 *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) _Float16 dsh[L16_OG][L16_P][4];  // d_0 .. d_3 of a pixel: one 8-byte read
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int HW = h * w, p0 = blockIdx.x * L16_P;
    const int co0 = wave * 64;
    f32x4 tv[2][2][4];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int pb = 0; pb < 2; ++pb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                tv[cb][pb][g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (term) {  // (uniform)
                    int p = p0 + pb * 32 + 8 * g + 4 * lh;
                    p = p < HW - 4 ? p : HW - 4;
                    tv[cb][pb][g] = *(const f32x4 *)(term + (long)(co0 + cb * 32 + l31) * HW + p);
                }
            }
    f16x8 wf[2];
    float bz[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        wf[cb] = __builtin_bit_cast(f16x8, wpk[(wave * 2 + cb) * 64 + lane]);
        bz[cb] = b2[co0 + cb * 32 + l31];
    }
    // the lane's pixel in the depthwise stage (a clamped one past the plane: computed, never stored)
    const int pd = p0 + lane < HW ? p0 + lane : HW - 1;
    const int yd = pd / w, xd = pd - yd * w;
    for (int o0 = 0; o0 < n; o0 += L16_OG) {
        const int ng = n - o0 < L16_OG ? n - o0 : L16_OG;
        for (int oc = wave; oc < ng * Cp; oc += L16_NT / 64) {  // (object, channel): uniform per wave
            const int ol = oc / Cp, c = oc - ol * Cp;
            const char *src = (const char *)(planes + ((long)(o0 + ol) * Cp + c) * HW);
            const float *wk = w1 + c * DW_K * DW_K;
            // (the tap offsets and border predicates do not depend on (object, channel): hoisted out of this loop they are 49
            // registers and 49 lane masks, which spill; behind this they are recomputed per item, a few hundred VALU instructions)
            int y = yd, x = xd;
            asm volatile("" : "+v"(y), "+v"(x));
            // pass 1: all 49 loads, clamped addresses, no predicate near them; pass 2 selects and sums.  (As one loop hipcc sinks
            // each load into the branch of its select and waits vmcnt(0) there: 49 serial round trips per item -- dw_tile's r2 note.)
            float t[DW_K][DW_K];
#pragma unroll
            for (int ky = 0; ky < DW_K; ++ky) {
                const int row = min(max(y + ky - DW_R, 0), h - 1) * w;
#pragma unroll
                for (int kx = 0; kx < DW_K; ++kx)  // (unsigned BYTE offsets on a uniform base, as in dw_tile: h*w < 2^29)
                    t[ky][kx] = *(const float *)(src + 4u * (unsigned)(row + min(max(x + kx - DW_R, 0), w - 1)));
            }
#pragma unroll
            for (int ky = 0; ky < DW_K; ++ky)
                asm volatile("" : "+v"(t[ky][0]), "+v"(t[ky][1]), "+v"(t[ky][2]), "+v"(t[ky][3]), "+v"(t[ky][4]), "+v"(t[ky][5]), "+v"(t[ky][6]));
            float acc = 0.0f;
#pragma unroll
            for (int ky = 0; ky < DW_K; ++ky) {
                const int yy = y + ky - DW_R;
                const bool yok = yy >= 0 && yy < h;
#pragma unroll
                for (int kx = 0; kx < DW_K; ++kx) {
                    const int xx = x + kx - DW_R;
                    acc = fmaf((yok && xx >= 0 && xx < w) ? t[ky][kx] : 0.0f, wk[ky * DW_K + kx], acc);
                }
            }
            const float o = fmaf(acc + (b1 ? b1[c] : 0.0f), sc1 ? sc1[c] : 1.0f, sh1 ? sh1[c] : 0.0f);
            dsh[ol][lane][c] = (_Float16)f16_sat(f16_relu(o));
        }
        for (int i = tid; i < ng * L16_P; i += L16_NT)
            for (int c = Cp; c < 4; ++c) dsh[i >> 6][i & 63][c] = (_Float16)0.0f;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (LDS-only barriers: __syncthreads() would wait out the stores too)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        for (int ol = 0; ol < ng; ++ol) {
            f16x8 a[2];
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                const f16x4 d = *(const f16x4 *)dsh[ol][pb * 32 + l31];
                const f16x4 z = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
                a[pb] = __builtin_shufflevector(lh ? z : d, z, 0, 1, 2, 3, 4, 5, 6, 7);  // k = 8 lh + 0..7: live in the low half only
            }
            _Float16 *dst = out + (long)(o0 + ol) * PW_CO * HW;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                const int co = co0 + cb * 32 + l31;
#pragma unroll
                for (int pb = 0; pb < 2; ++pb) {
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[pb], wf[cb], acc, 0, 0, 0);
                    // C/D layout: column = lane & 31 (output channel), registers 4 g .. 4 g + 3 = pixels 8 g + 4 (lane >> 5) + 0..3
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int p = p0 + pb * 32 + 8 * g + 4 * lh;
                        if (p >= HW) continue;
                        f32x4 v = {acc[4 * g] + bz[cb], acc[4 * g + 1] + bz[cb], acc[4 * g + 2] + bz[cb], acc[4 * g + 3] + bz[cb]};
                        if (term) v += tv[cb][pb][g];
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = f16_sat(relu_out ? f16_relu(v[j]) : v[j]);
                        *(f16x4 *)(dst + (long)co * HW + p) = __builtin_convertvector(v, f16x4);
                    }
                }
            }
        }
        if (o0 + L16_OG < n) {  // (the next group's depthwise stage overwrites the table)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// The same fp32 contraction with the WEIGHTS RESIDENT IN REGISTERS (r4).  conv1x1_mfma_kernel streams a 16 KiB weight slice
// per 16 input channels into LDS for every 64-pixel tile (256 KiB of L2 -> LDS traffic per tile, two operand reads per MFMA
// pair) and measured 0.49 .. 0.58 of the fp32 matrix peak.  Here a wave owns 32 output channels and keeps their whole
// [Cin <= 256][32] weight block as the MFMA A operand -- Cin / 2 VGPRs, loaded once -- while the activation streams through
// a ring of LDS stage buffers by LDS-DMA: one ds_read_b32 per MFMA, no weight traffic after the prologue.  It is the
// global-match kernel's shape (one operand in registers, the other through LDS), which runs at 0.90 of the same peak.
//   workgroup = 4 waves = 128 output channels (one HALF of the 256) x a contiguous range of 64-pixel tiles (persistent);
//   two workgroups per CU (<= 256 VGPRs): a half-0 and a half-1 workgroup of the same pixel range sit 8 blocks apart, i.e.
//   on the same XCD (block b runs on XCD b % 8 -- observed, used for speed only), so the second reader of an activation row
//   hits that XCD's L2; while one workgroup drains its tile's stores (vmcnt counts stores too: the epilogue ends in the
//   only vmcnt(0) of the tile) the other keeps the matrix pipe busy.
//   FOUR accumulator chains per wave: tools/ubench/mfma_f32_chains.hip -- the fp32 pipe needs four independent chains per
//   wave (0.98 of the peak with one or two waves per SIMD); two chains reach 0.92 alone and 0.66 beside a second wave, which
//   is where this kernel's first form (32 channels x 2 pixel blocks = 2 chains) sat: 0.60.  64 channels per wave would need
//   256 weight registers, so the two extra chains come from K: even and odd k-steps accumulate separately and are added once
//   per tile -- still pure fp32 (every product and sum an fmaf / add in fp32), but the k-ascending chain of
//   conv1x1_mfma_kernel becomes two interleaved ones: results agree to summation-order rounding, not bit for bit.
//   stage = 32 input channels x 64 pixels (8 KiB, 2 DMA pieces per wave), ring of 4, fetched 3 steps ahead ACROSS tile
//   boundaries; a step's fragments F[s] are refilled with the next step's k-step s right behind the MFMAs that consumed them.
// r5: the stage size is a template parameter -- 64 input channels per stage where Cin allows (half the barriers and counted waits per
// tile: a wave then issues 64 MFMAs between two barriers), 32 otherwise.
constexpr int RW_P = 64, RW_NB = 4, RW_NT = 256, RW_KMAX = 256;
__device__ __forceinline__ void rw_wait_vmcnt(int n)  // wave-uniform n: 0, 2, 4 (pieces of the steps still in flight)
{
    if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (n >= 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
template <int RW_KC>
__global__ __launch_bounds__(RW_NT, 2) void conv1x1_rw_kernel(const float *__restrict__ in, long in_bs, int Cin, long HW,
                                                              const float *__restrict__ w2t, const float *__restrict__ b2,
                                                              int relu_out, float *__restrict__ out, int tpp, int total_tiles,
                                                              int G, int halves, int /* always 0 */)
{
    __shared__ __attribute__((aligned(1024))) float xbuf[RW_NB][RW_KC * RW_P];
    __shared__ float bsh[128];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kk = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int half = j & 1, grp = xcd + 8 * (j >> 1);
    if (grp >= G) return;
    // A group's range is cut in HALF-tile units (r5): 804 tiles on 256 groups are 3 or 4 tiles each -- the launch takes four tile
    // times for 3.14 of work; in halves the longest group has 3 1/2.  A range that starts / ends inside a tile computes only
    // the pixels of one parity there (pixel block 1 at its start, 0 at its end; the tile's other block belongs to the neighbour
    // group): the same staging, half the MFMAs, every output still the same two k-parity chains.
    // (halves: the launcher's choice -- a half tile costs ~0.65 of a tile, worth it only where the longest group gets shorter)
    const int u0 = halves ? (int)((long)grp * (2L * total_tiles) / G) : 2 * (int)((long)grp * total_tiles / G);
    const int u1 = halves ? (int)((long)(grp + 1) * (2L * total_tiles) / G) : 2 * (int)((long)(grp + 1) * total_tiles / G);
    const int t0 = u0 >> 1, t1 = (u1 + 1) >> 1;
    if (u0 >= u1) return;
    const int co0 = half * 128 + wave * 32;
    if (tid < 128) bsh[tid] = b2[half * 128 + tid];
    // A operand: lane (co = l31, kk) holds w[2 s + kk][co0 + co] for every k-step s (zero past Cin)
    const int nch = (Cin + RW_KC - 1) / RW_KC;  // (Cin % 32 == 0: checked by the launcher)
    // (Cin is a whole number of 32-channel stages: ONE uniform branch per stage around 16 plain loads -- r4 predicated every one of
    // the 128 loads on k < Cin: 128 exec-mask branches in the prologue of each of the 512 workgroups, ~5 us of a launch)
    float a[RW_KMAX / 2];
    {
        const float *wl = w2t + (long)kk * PW_CO + co0 + l31;
#pragma unroll
        for (int g = 0; g < RW_KMAX / RW_KC; ++g) {
            if (g < nch) {
#pragma unroll
                for (int s = 0; s < RW_KC / 2; ++s) a[g * (RW_KC / 2) + s] = wl[(long)(g * RW_KC + 2 * s) * PW_CO];
            } else {
#pragma unroll
                for (int s = 0; s < RW_KC / 2; ++s) a[g * (RW_KC / 2) + s] = 0.0f;
            }
        }
    }
    const unsigned xbase = __builtin_amdgcn_readfirstlane((unsigned)(size_t)&xbuf[0][0]);
    // step = (tile, chunk); step number n lives in ring slot n % RW_NB.  All of a step's address arithmetic is SCALAR (the
    // tile / chunk counters advance incrementally: no division, no per-lane 64-bit multiply): a lane contributes one 32-bit
    // byte offset, computed once.
    const int b0 = t0 / tpp;
    int pf_b = b0, pf_p = t0 - b0 * tpp, pf_c = 0, pf_left = (t1 - t0), issued = 0;
    const unsigned lane_off = (unsigned)(((long)(lane >> 4) * HW + 4 * (lane & 15)) * 4);
    // the plane's last tile may be partial: clamped columns are computed and never stored
    const long last_p0 = (long)(tpp - 1) * RW_P;
    long lpix = 4 * (lane & 15);
    if (last_p0 + lpix > HW - 4) lpix = HW - 4 - last_p0;
    const unsigned lane_off_last = (unsigned)(((long)(lane >> 4) * HW + lpix) * 4);
    auto issue = [&]() __attribute__((always_inline)) {
        if (pf_left <= 0) return;  // (uniform)
        // this wave's pieces: channel rows (RW_KC / 4) wave .. + RW_KC / 4 - 1 of the chunk, four rows (1 KiB) per piece
        const float *sbase = in + (long)pf_b * in_bs + (long)(pf_c * RW_KC + wave * (RW_KC / 4)) * HW + (long)pf_p * RW_P;
        const unsigned voff = (pf_p == tpp - 1) ? lane_off_last : lane_off;
        const unsigned dst = xbase + (unsigned)(issued % RW_NB) * (unsigned)(RW_KC * RW_P * 4) + (unsigned)wave * (unsigned)(RW_KC / 4 * 256);
#pragma unroll
        for (int pc = 0; pc < RW_KC / 16; ++pc) lds_dma16_s(sbase + (long)(4 * pc) * HW, voff, dst + 1024u * pc);
        ++issued;
        if (++pf_c == nch) {
            pf_c = 0;
            --pf_left;
            if (++pf_p == tpp) {
                pf_p = 0;
                ++pf_b;
            }
        }
    };
#pragma unroll
    for (int i = 0; i < RW_NB - 1; ++i) issue();
    // the compiler waits for the weights HERE (its counted vmcnt waits must not sink into the loop, where they would drain
    // the LDS-DMA it does not know about) -- and with them for the first steps' pieces
#pragma unroll
    for (int s = 0; s < RW_KMAX / 2; ++s) asm volatile("" : "+v"(a[s]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // F holds the NEXT eight k-steps' fragments: k-step s of a stage is refilled, right behind the MFMAs that consumed it, with
    // k-step s + 8 -- of the same stage, or the first eight of the next one (16 registers; a whole step's would not fit beside
    // 128 weights and 64 accumulators)
    constexpr int FH = 8;  // k-steps the fragment registers run ahead
    float F0[FH], F1[FH];
    // pixel block pb of the tile = the pixels of PARITY pb (MFMA column n <-> pixel 2 n + pb): a lane's two fragments of a
    // k-step are neighbours in LDS (one ds_read_b64, two k-steps per ds_read2_b64), and its two outputs of a channel are
    // neighbours in memory (one 8-byte store; 32 lanes = a full 256-byte run)
    {
        const float *X = &xbuf[0][kk * RW_P + 2 * l31];
#pragma unroll
        for (int s = 0; s < FH; ++s) {
            const f32x2 v = *(const f32x2 *)(X + 2 * s * RW_P);
            F0[s] = v[0];
            F1[s] = v[1];
        }
    }
    int st = 0;  // step number of (t, c); its stage was read into F during step st - 1, step st reads stage st + 1
    int cur_b = b0, cur_p = t0 - b0 * tpp;
    auto tile = [&](auto mode_) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_)::value;  // bit pb set: pixel block pb of the tile is this group's
        f32x16 acc[2][2];  // [pixel block][k-step parity]; a tile's first four MFMAs take C = 0 (no zeroing pass)
        const f32x16 zero16 = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < RW_KMAX / RW_KC; ++c) {
            if (c < nch) {  // (uniform)
                issue();  // step st + RW_NB - 1 -> the slot of step st - 1 (read during step st - 2: free)
                const float *Xc = &xbuf[st % RW_NB][kk * RW_P + 2 * l31], *Xn = &xbuf[(st + 1) % RW_NB][kk * RW_P + 2 * l31];
#pragma unroll
                for (int s = 0; s < RW_KC / 2; s += 2) {
                    const int ks = c * (RW_KC / 2) + s, f = s % FH;
                    const bool first = c == 0 && s == 0;  // (compile-time: both loops are unrolled)
                    if constexpr ((MODE & 1) != 0) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks], F0[f], first ? zero16 : acc[0][0], 0, 0, 0);
                    if constexpr ((MODE & 2) != 0) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks], F1[f], first ? zero16 : acc[1][0], 0, 0, 0);
                    if constexpr ((MODE & 1) != 0) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks + 1], F0[f + 1], first ? zero16 : acc[0][1], 0, 0, 0);
                    if constexpr ((MODE & 2) != 0) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks + 1], F1[f + 1], first ? zero16 : acc[1][1], 0, 0, 0);
                    // k-steps s + 8, s + 9 of this stage, or of the next stage's first eight (a stale read behind the last step)
                    const float *X = s + FH < RW_KC / 2 ? Xc + 2 * (s + FH) * RW_P : Xn + 2 * (s + FH - RW_KC / 2) * RW_P;
                    const f32x2 va = *(const f32x2 *)X, vb = *(const f32x2 *)(X + 2 * RW_P);
                    F0[f] = va[0];
                    F1[f] = va[1];
                    F0[f + 1] = vb[0];
                    F1[f + 1] = vb[1];
                    __builtin_amdgcn_sched_group_barrier(0x008, MODE == 3 ? 4 : 2, 0);  // the MFMAs
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // the refill (one ds_read2_b64) right behind them
                }
                rw_wait_vmcnt((RW_KC / 16) * (issued - 1 - (st + 2)));  // step st + 2 has landed: only the steps behind it may be out
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of stages st, st + 1 have returned
                __syncthreads();
                ++st;
            }
        }
        // C/D layout: column = lane & 31 (pixel), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (output channel); a store = a
        // scalar row base + this lane's 32-bit offset
        {
            const long p0 = (long)cur_p * RW_P;
            float *dst = out + ((long)cur_b * PW_CO + co0) * HW + p0;
            const unsigned voff = (unsigned)((long)(4 * kk) * HW + 2 * l31);
            if (p0 + 2 * l31 < HW) {  // (HW is a multiple of 4 and p0 of 64: a pixel pair is inside or outside as a whole)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2);
                    const float bb = bsh[wave * 32 + row + 4 * kk];
                    if constexpr (MODE == 3) {
                        f32x2 v = {(acc[0][0][r] + acc[0][1][r]) + bb, (acc[1][0][r] + acc[1][1][r]) + bb};
                        if (relu_out) v = __builtin_elementwise_max(v, f32x2{0.0f, 0.0f});
                        *(f32x2 *)((dst + (long)row * HW) + voff) = v;
                    } else {
                        constexpr int pb = MODE == 1 ? 0 : 1;
                        float v = (acc[pb][0][r] + acc[pb][1][r]) + bb;
                        if (relu_out) v = fmaxf(v, 0.0f);
                        (dst + (long)row * HW)[voff + pb] = v;
                    }
                }
            }
            if (++cur_p == tpp) {
                cur_p = 0;
                ++cur_b;
            }
            // No drain of the stores here (r5).  vmcnt counts loads and stores alike and the two kinds may complete out of order
            // with respect to EACH OTHER, but loads complete in issue order among themselves: a counted wait "at most n
            // outstanding" behind n younger DMA pieces still implies the older piece has landed (were it outstanding, so would
            // be its n younger ones: n + 1) -- outstanding stores only make the wait conservative.  r4 drained the 16 stores with
            // vmcnt(0) at the end of every tile: both waves of a SIMD reach that point together (all workgroups run in step), so
            // the matrix pipe idled for a store round trip per tile: 101.4 -> 96.6 us at [3,256,120,214].
        }
    };
    for (int t = t0; t < t1; ++t) {
        if (t == t0 && (u0 & 1))  // (uniform; a range is at least two units long: never both ends in one tile)
            tile(std::integral_constant<int, 2>{});
        else if (t == t1 - 1 && (u1 & 1))
            tile(std::integral_constant<int, 1>{});
        else
            tile(std::integral_constant<int, 3>{});
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// DynamicSegHead layer 1, PER-OBJECT half, fused (r5): the head-input assembly (IntVOS.py:663-669) -> the depthwise 7x7 + bn1 + relu1 of
// the three per-object channels (:491-493) -> their 1x1 (3 -> 256, bn2 folded, :494) + the shared-embedding half's term + relu2, ONE
// launch instead of three (head_inputs_kernel 3 us + dwconv [n,3,h,w] 11 us, launch-sized + conv1x1_mfma K = 3 22 us at 480p):
//   in_0 = global map of object o, in_1 = local map of o, in_2 = (label == o)                      (zero outside the image)
//   d_c  = relu(fmaf(taps_c + b1[c], scale1[c], shift1[c])),  taps_c = the depthwise kernel's fmaf chain (ky outer, kx inner)
//   out[o][co][p] = relu?((fmaf(w2[2][co], d_2, fmaf(w2[1][co], d_1, fmaf(w2[0][co], d_0, 0))) + b2[co]) + term[co][p])
// -- operation for operation what dwconv7x7_bn_relu_kernel and conv1x1_mfma_kernel (a k-ascending fmaf chain from zero, bias, `add`,
// ReLU) compute on head_inputs_kernel's channels: the same bits.  A stream: reads the term once per object (26 MB each, L2-shared
// between the objects' workgroups of a tile), writes the [n,256,h,w] activation once.
// A workgroup owns a 2 x 64 pixel tile for OB objects; its waves split the 256 output channels in L1_CW parts (25 680 pixels are only
// 401 waves' worth of lanes).  The depthwise stage runs ONCE per tile -- channel c by the threads of part c % L1_CW -- and reaches the
// other parts through LDS; then every thread streams its 64 channels, L1_UNROLL term loads in flight per lane (a lane's accesses are
// HW floats apart: the memory system sees a wave's 256-byte row segments only).  OB = 1 up to three objects, 2 from four.
// Timed by rocprofv3 on rotating buffers (nothing in the 256 MB memory-side cache; a python loop around the op is host-bound at
// ~30 us and hid this): 2 parts, each recomputing the depthwise stage, 16 loads in flight 40.9 us at 3 objects / 33.1 at 2; this form
// 37.3 / 26.4; a framework broadcast-add moving the same bytes 28.7 (docs/history/r05_experiments.md).
constexpr int L1_TH = 2, L1_TW = 64, L1_CW = 4, L1_NT = L1_TH * L1_TW * L1_CW, L1_LW = L1_TW + 6 + 1, L1_UNROLL = 8;
template <int L1_OB>
__global__ __launch_bounds__(L1_NT) void head_layer1_object_kernel(const float *__restrict__ gmap, const float *__restrict__ lmap,
                                                                   const int *__restrict__ labels, int h, int w, int n_ids,
                                                                   const float *__restrict__ w1, const float *__restrict__ b1,
                                                                   const float *__restrict__ sc1, const float *__restrict__ sh1,
                                                                   const float *__restrict__ w2, const float *__restrict__ b2,
                                                                   const float *__restrict__ term, int relu_out,
                                                                   float *__restrict__ out, int ntx, int ntiles, int chunk)
{
    __shared__ float tin[L1_OB][3][L1_TH + 6][L1_LW];
    __shared__ __attribute__((aligned(16))) float wtab[PW_CO][4];  // {w2[0][co], w2[1][co], w2[2][co], b2[co]}
    // XCD-aware block map: block L runs on XCD L % 8; each XCD owns a contiguous band of `chunk` tiles (row-major) for every object
    // group -- the cache lines a tile edge cuts (a tile row is 256 bytes at an arbitrary 8-byte alignment) are completed in ONE L2,
    // and the objects' workgroups of a tile find the term there.
    const int xcd_ = blockIdx.x & 7, j_ = blockIdx.x >> 3;
    const int t_ = xcd_ * chunk + j_ % chunk, bz = j_ / chunk;
    if (t_ >= ntiles) return;
    const int tid = threadIdx.x, o0 = bz * L1_OB;
    const int nob = (n_ids - o0) < L1_OB ? (n_ids - o0) : L1_OB;  // objects of this workgroup (uniform)
    const int x0 = (t_ % ntx) * L1_TW, y0 = (t_ / ntx) * L1_TH;
    for (int i = tid; i < (L1_TH + 6) * (L1_TW + 6); i += L1_NT) {
        const int r = i / (L1_TW + 6), c = i - r * (L1_TW + 6);
        const int yy = y0 - 3 + r, xx = x0 - 3 + c;
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const long p = in ? (long)yy * w + xx : 0;
        const int lab = in ? labels[p] : -1;
#pragma unroll
        for (int j = 0; j < L1_OB; ++j) {
            if (j < nob) {
                tin[j][0][r][c] = in ? gmap[p * n_ids + o0 + j] : 0.0f;
                tin[j][1][r][c] = in ? lmap[p * n_ids + o0 + j] : 0.0f;
                tin[j][2][r][c] = (in && lab == o0 + j) ? 1.0f : 0.0f;
            }
        }
    }
    for (int i = tid; i < PW_CO; i += L1_NT) {
        wtab[i][0] = w2[i];
        wtab[i][1] = w2[PW_CO + i];
        wtab[i][2] = w2[2 * PW_CO + i];
        wtab[i][3] = b2[i];
    }
    __syncthreads();
    const int cw = tid / (L1_TH * L1_TW), pt = tid - cw * (L1_TH * L1_TW);  // channel quarter (= wave), pixel of the tile
    const int ty = pt / L1_TW, tx = pt - ty * L1_TW;
    // the depthwise stage ONCE per tile: channel c by the threads of channel part c % L1_CW, shared through LDS
    __shared__ float dsh[L1_OB][3][L1_TH * L1_TW];
#pragma unroll
    for (int j = 0; j < L1_OB; ++j) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c % L1_CW != cw) continue;  // (uniform per wave)
            float acc = 0.0f;
            if (j < nob) {
#pragma unroll
                for (int ky = 0; ky < DW_K; ++ky)
#pragma unroll
                    for (int kx = 0; kx < DW_K; ++kx) acc = fmaf(tin[j][c][ty + ky][tx + kx], w1[c * DW_K * DW_K + ky * DW_K + kx], acc);
            }
            dsh[j][c][pt] = fmaxf(fmaf(acc + (b1 ? b1[c] : 0.0f), sc1 ? sc1[c] : 1.0f, sh1 ? sh1[c] : 0.0f), 0.0f);
        }
    }
    __syncthreads();
    float d[L1_OB][3];
#pragma unroll
    for (int j = 0; j < L1_OB; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) d[j][c] = dsh[j][c][pt];
    const int y = y0 + ty, x = x0 + tx;
    if (y >= h || x >= w) return;
    const long HW = (long)h * w, p = (long)y * w + x;
    const float *tp = term + p;
    float *dst = out + (long)o0 * PW_CO * HW + p;
    for (int c0 = cw * (PW_CO / L1_CW); c0 < (cw + 1) * (PW_CO / L1_CW); c0 += L1_UNROLL) {
        float tv[L1_UNROLL];
#pragma unroll
        for (int u = 0; u < L1_UNROLL; ++u) tv[u] = tp[(long)(c0 + u) * HW];
#pragma unroll
        for (int u = 0; u < L1_UNROLL; ++u) {
            const f32x4 t = *(const f32x4 *)wtab[c0 + u];
#pragma unroll
            for (int j = 0; j < L1_OB; ++j) {
                if (j < nob) {
                    float v = fmaf(t[2], d[j][2], fmaf(t[1], d[j][1], fmaf(t[0], d[j][0], 0.0f))) + t[3];
                    v += tv[u];
                    if (relu_out) v = fmaxf(v, 0.0f);
                    dst[((long)j * PW_CO + c0 + u) * HW] = v;
                }
            }
        }
    }
}

}  // namespace

/* DynamicSegHead layer 1, per-object half, fused (head_layer1_object_kernel): global_map / local_map [HW][n_ids] fp32, labels [HW]
 * int32, the depthwise weights / bias / folded bn1 of the THREE per-object channels, w2t_object [3][256] + b2 [256] (bn2 folded),
 * term [256][HW] = the shared-embedding half's contribution -> out [n_ids][256][HW]. */
extern "C" int manet_head_layer1_object_f32(const float *global_map, const float *local_map, const int32_t *labels, int h, int w,
                                            int n_ids, const float *dw_weight, const float *dw_bias, const float *bn_scale,
                                            const float *bn_shift, const float *w2t_object, const float *b2, const float *term,
                                            int relu_out, float *out, manet_stream_t stream)
{
    if (!global_map || !local_map || !labels || !dw_weight || !w2t_object || !b2 || !term || !out || h <= 0 || w <= 0 || n_ids <= 0 ||
        n_ids > 65535)
        return manet_set_error(MANET_E_INVALID, "bad arguments");
    const int ob = n_ids >= 4 ? 2 : 1;
    auto kern = ob == 2 ? head_layer1_object_kernel<2> : head_layer1_object_kernel<1>;
    const int ntx = (w + L1_TW - 1) / L1_TW, ntiles = ntx * ((h + L1_TH - 1) / L1_TH), chunk = (ntiles + 7) / 8;
    dim3 grid((unsigned)(8 * chunk * ((n_ids + ob - 1) / ob)));
    hipLaunchKernelGGL(kern, grid, dim3(L1_NT), 0, (hipStream_t)stream, global_map, local_map, (const int *)labels,
                       h, w, n_ids, dw_weight, dw_bias, bn_scale, bn_shift, w2t_object, b2, term, relu_out, out, ntx, ntiles, chunk);
    return manet_check_launch("manet_head_layer1_object_f32");
}

extern "C" int manet_relu_conv1x1_c1_f32(const float *in, int B, int C, long HW, const float *weight, const float *bias,
                                         int relu_in, float *out, manet_stream_t stream)
{
    if (!in || !weight || !out || B <= 0 || C <= 0 || HW <= 0 || B > 65535)
        return manet_set_error(MANET_E_INVALID, "bad arguments");
    dim3 grid((unsigned)((HW + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(relu_conv1x1_c1_kernel, grid, dim3(64 * RC_WAVES), 0, (hipStream_t)stream, in, C, HW, weight, bias,
                       relu_in, out);
    return manet_check_launch("manet_relu_conv1x1_c1_f32");
}

extern "C" int manet_dwconv7x7_bn_relu_f32(const float *in, int B, int C, int h, int w, const float *weight,
                                           const float *bias, const float *bn_scale, const float *bn_shift, int relu,
                                           float *out, manet_stream_t stream)
{
    return manet_dwconv7x7_bn_relu_ex(in, B, C, h, w, weight, bias, bn_scale, bn_shift, relu, 0, out, stream);
}

// relu_in != 0: the input is read through max(x, 0) (the preceding block's ReLU folded into this pass)
extern "C" int manet_dwconv7x7_bn_relu_ex(const float *in, int B, int C, int h, int w, const float *weight,
                                          const float *bias, const float *bn_scale, const float *bn_shift, int relu,
                                          int relu_in, float *out, manet_stream_t stream)
{
    if (!in || !weight || !out || B <= 0 || C <= 0 || h <= 0 || w <= 0 || (long)B * C > 65535)
        return manet_set_error(MANET_E_INVALID, "bad arguments (B*C must be <= 65535)");
    if (C > 65535) return manet_set_error(MANET_E_INVALID, "C must be <= 65535");
    const int ntx = (w + DW_TX - 1) / DW_TX, nty = (h + DW_TY - 1) / DW_TY;
    // the strip behind the last full tile column: 120 x 24 tiles instead of 60 x 64 ones when it holds at most 24 columns (480p: 22)
    const int rem = w - (ntx - 1) * DW_TX;
    const bool narrow = ntx >= 2 && rem <= DwNarrow::TX && manet_tune_get(MANET_TUNE_DW_NARROW, 1) != 0;
    const int nstd = narrow ? (ntx - 1) * nty : ntx * nty;
    const int ntile = narrow ? nstd + (h + DwNarrow::TY - 1) / DwNarrow::TY : nstd;
    // the batch walk pays when every CU has workgroups to overlap; below two workgroups per CU the items go into the grid
    const int per_item = (B > 1 && (long)ntile * C < 512) ? 1 : 0;
    const long planes = per_item ? (long)B * C : C;
    const long nblocks = 8L * ntile * ((planes + 7) / 8);  // (planes in groups of eight: one per XCD)
    if (nblocks > 0x7fffffffL) return manet_set_error(MANET_E_INVALID, "too many tiles for one launch");
    dim3 grid((unsigned)nblocks);
#define DW_LAUNCH2(F_, RI_, R_)                                                                                        \
    hipLaunchKernelGGL((dwconv7x7_bn_relu_kernel<F_, RI_, R_>), grid, dim3(256), 0, (hipStream_t)stream, in, B, C, h, w, weight, \
                       bias, bn_scale, bn_shift, out, per_item, ntx, nty, nstd, ntile)
#define DW_LAUNCH(F_)                                                                                                  \
    do {                                                                                                               \
        if (relu_in && relu) DW_LAUNCH2(F_, true, true);                                                               \
        else if (relu_in) DW_LAUNCH2(F_, true, false);                                                                 \
        else if (relu) DW_LAUNCH2(F_, false, true);                                                                    \
        else DW_LAUNCH2(F_, false, false);                                                                             \
    } while (0)
    if (w % 2 == 0 && w >= 2 && ((size_t)in & 7) == 0 && ((size_t)out & 7) == 0) DW_LAUNCH(true);
    else DW_LAUNCH(false);
#undef DW_LAUNCH2
#undef DW_LAUNCH
    return manet_check_launch("manet_dwconv7x7_bn_relu_f32");
}

static int conv1x1_f32_impl(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const float *w2t,
                            const float *b2, int Cout, int relu_out, float *out, const float *head_w, const float *head_b,
                            float *head_out, const float *add, manet_stream_t stream);

// 1x1 convolution with 256 output channels as an fp32-MFMA contraction (conv1x1_mfma_kernel)
extern "C" int manet_conv1x1_f32(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const float *w2t,
                                 const float *b2, int Cout, int relu_out, float *out, manet_stream_t stream)
{
    return manet_conv1x1_head_f32(in, in_batch_stride, B, Cin, HW, w2t, b2, Cout, relu_out, out, nullptr, nullptr, nullptr, stream);
}

// ... optionally with DynamicSegHead's output layer fused into the epilogue (head_w != NULL: `out` is not written)
extern "C" int manet_conv1x1_add_f32(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const float *w2t,
                                     const float *b2, const float *add, int Cout, int relu_out, float *out, manet_stream_t stream);

extern "C" int manet_conv1x1_head_f32(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const float *w2t,
                                      const float *b2, int Cout, int relu_out, float *out, const float *head_w,
                                      const float *head_b, float *head_out, manet_stream_t stream)
{
    return conv1x1_f32_impl(in, in_batch_stride, B, Cin, HW, w2t, b2, Cout, relu_out, out, head_w, head_b, head_out, nullptr, stream);
}

// ... or with an optional [256][HW] term shared by every batch entry added in the epilogue (layer 1's shared-embedding half)
extern "C" int manet_conv1x1_add_f32(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const float *w2t,
                                     const float *b2, const float *add, int Cout, int relu_out, float *out, manet_stream_t stream)
{
    return conv1x1_f32_impl(in, in_batch_stride, B, Cin, HW, w2t, b2, Cout, relu_out, out, nullptr, nullptr, nullptr, add, stream);
}

static int conv1x1_f32_impl(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const float *w2t,
                            const float *b2, int Cout, int relu_out, float *out, const float *head_w, const float *head_b,
                            float *head_out, const float *add, manet_stream_t stream)
{
    if (!in || !w2t || !b2 || (!out && !head_w) || (head_w && !head_out) || B <= 0 || B > 65535 || Cin <= 0 || HW <= 0)
        return manet_set_error(MANET_E_INVALID, "bad arguments");
    if (Cout != PW_CO) return manet_set_error(MANET_E_INVALID, "Cout=%d (this kernel is built for %d output channels)", Cout, PW_CO);
    if (HW % 4 != 0 || HW < 4)
        return manet_set_error(MANET_E_INVALID, "HW=%lld must be a multiple of 4 (16-byte LDS-DMA rows)", (long long)HW);
    if (((size_t)w2t & 15) != 0 || ((size_t)in & 15) != 0 || (in_batch_stride & 3) != 0)
        return manet_set_error(MANET_E_INVALID, "in / w2t must be 16-byte aligned, the batch stride a multiple of 4 elements");
    // weights resident in registers (conv1x1_rw_kernel) when the layer allows: whole 32-channel stages, no fused output layer
    if (head_w && add) return manet_set_error(MANET_E_INVALID, "add and the fused output layer are exclusive");
    if (!head_w && !add && Cin % 32 == 0 && Cin <= RW_KMAX && manet_tune_get(MANET_TUNE_CONV1X1, 0) != 1) {
        const int tpp = (int)((HW + RW_P - 1) / RW_P);
        const long total = (long)tpp * B;
        int G = 256;  // pixel-range groups: one per CU; each is served by two workgroups (the output-channel halves)
        if (total < G) G = (int)total;
        const unsigned blocks = (unsigned)(((G + 7) / 8) * 16);
        // ranges in half-tile units where that shortens the longest group by half a tile of at most ten (804 tiles on 256 groups:
        // 4 -> 3 1/2; 1 206: 5 either way, and two half tiles per group would only cost)
        const long per_whole = (total + G - 1) / G, per_half = (2 * total + G - 1) / G;
        int halves = (per_half < 2 * per_whole && per_whole <= 10) ? 1 : 0;
        const int tune = manet_tune_get(MANET_TUNE_CONV1X1, 0);
        if (tune == 3) halves = 0;  // (3 / 4: whole tiles / half-tile units everywhere, A/B timing and tests)
        if (tune == 4) halves = total >= G ? 1 : 0;
        if (Cin % 64 == 0 && tune != 2)  // (2: 32-channel stages everywhere, A/B timing)
            hipLaunchKernelGGL(conv1x1_rw_kernel<64>, dim3(blocks), dim3(RW_NT), 0, (hipStream_t)stream, in, (long)in_batch_stride, Cin,
                               (long)HW, w2t, b2, relu_out, out, tpp, (int)total, G, halves, 0);
        else
            hipLaunchKernelGGL(conv1x1_rw_kernel<32>, dim3(blocks), dim3(RW_NT), 0, (hipStream_t)stream, in, (long)in_batch_stride, Cin,
                               (long)HW, w2t, b2, relu_out, out, tpp, (int)total, G, halves, 0);
        return manet_check_launch("manet_conv1x1_f32 (resident weights)");
    }
    dim3 grid((unsigned)((HW + PW_P - 1) / PW_P), (unsigned)B);
    hipLaunchKernelGGL(conv1x1_mfma_kernel, grid, dim3(PW_NT), 0, (hipStream_t)stream, in, (long)in_batch_stride, Cin, (long)HW,
                       w2t, b2, relu_out, out, head_w, head_b, head_out, add);
    return manet_check_launch("manet_conv1x1_f32");
}

// bytes of the packed split-bf16 weight image of a [Cin][256] 1x1 layer (manet_conv1x1_x3_pack)
extern "C" int64_t manet_conv1x1_x3_weight_bytes(int Cin) { return Cin <= 0 ? 0 : (int64_t)((Cin + X3_KC - 1) / X3_KC) * X3_WCHUNK; }

static int x3_pack_impl(const float *w2t, int Cin, int Cout, void *wpk, int pieces, manet_stream_t stream)
{
    if (!w2t || !wpk || Cin <= 0) return manet_set_error(MANET_E_INVALID, "bad arguments");
    if (Cout != PW_CO) return manet_set_error(MANET_E_INVALID, "Cout=%d (this kernel is built for %d output channels)", Cout, PW_CO);
    if (((size_t)wpk & 15) != 0) return manet_set_error(MANET_E_INVALID, "wpk must be 16-byte aligned");
    const int n = (Cin + X3_KC - 1) / X3_KC;
    if (pieces == 3)
        hipLaunchKernelGGL(conv1x1_x3_pack_kernel<3>, dim3((unsigned)(n * 2)), dim3(256), 0, (hipStream_t)stream, w2t, Cin, (uint4 *)wpk, n);
    else
        hipLaunchKernelGGL(conv1x1_x3_pack_kernel<2>, dim3((unsigned)(n * 2)), dim3(256), 0, (hipStream_t)stream, w2t, Cin, (uint4 *)wpk, n);
    return manet_check_launch("manet_conv1x1_x3_pack");
}
extern "C" int manet_conv1x1_x3_pack(const float *w2t, int Cin, int Cout, void *wpk, manet_stream_t stream)
{
    return x3_pack_impl(w2t, Cin, Cout, wpk, 2, stream);
}
// the three-piece form ("split3": hi + mid + lo, six products per pair): 24 KiB per 16 input channels
extern "C" int64_t manet_conv1x1_x6_weight_bytes(int Cin) { return Cin <= 0 ? 0 : (int64_t)((Cin + X3_KC - 1) / X3_KC) * 3 * 8 * 1024; }
extern "C" int manet_conv1x1_x6_pack(const float *w2t, int Cin, int Cout, void *wpk, manet_stream_t stream)
{
    return x3_pack_impl(w2t, Cin, Cout, wpk, 3, stream);
}

// 1x1 convolution with 256 output channels in split-bf16 arithmetic (conv1x1_x3_kernel); add: optional [256][HW] term
// shared by every batch entry; head_w != NULL: DynamicSegHead's output layer fused (`out` is not written)
static int x3_impl(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const void *wpk, const float *b2,
                   const float *add, int Cout, int relu_out, float *out, const float *head_w, const float *head_b,
                   float *head_out, int pieces, manet_stream_t stream);
extern "C" int manet_conv1x1_x3_f32(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const void *wpk,
                                    const float *b2, const float *add, int Cout, int relu_out, float *out, const float *head_w,
                                    const float *head_b, float *head_out, manet_stream_t stream)
{
    return x3_impl(in, in_batch_stride, B, Cin, HW, wpk, b2, add, Cout, relu_out, out, head_w, head_b, head_out, 2, stream);
}
// ... with three pieces per factor (wpk from manet_conv1x1_x6_pack): fp32-class results at 6/16 of the fp32 matrix pipe's time
extern "C" int manet_conv1x1_x6_f32(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const void *wpk,
                                    const float *b2, const float *add, int Cout, int relu_out, float *out, const float *head_w,
                                    const float *head_b, float *head_out, manet_stream_t stream)
{
    return x3_impl(in, in_batch_stride, B, Cin, HW, wpk, b2, add, Cout, relu_out, out, head_w, head_b, head_out, 3, stream);
}
static int x3_impl(const float *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const void *wpk, const float *b2,
                   const float *add, int Cout, int relu_out, float *out, const float *head_w, const float *head_b,
                   float *head_out, int pieces, manet_stream_t stream)
{
    if (!in || !wpk || !b2 || (!out && !head_w) || (head_w && !head_out) || B <= 0 || B > 65535 || Cin <= 0 || HW <= 0)
        return manet_set_error(MANET_E_INVALID, "bad arguments");
    if (Cout != PW_CO) return manet_set_error(MANET_E_INVALID, "Cout=%d (this kernel is built for %d output channels)", Cout, PW_CO);
    if (HW % 4 != 0 || HW < 4) return manet_set_error(MANET_E_INVALID, "HW=%lld must be a multiple of 4 (16-byte LDS-DMA rows)", (long long)HW);
    if (((size_t)wpk & 15) != 0 || ((size_t)in & 15) != 0 || (in_batch_stride & 3) != 0)
        return manet_set_error(MANET_E_INVALID, "in / wpk must be 16-byte aligned, the batch stride a multiple of 4 elements");
    if (head_w && add) return manet_set_error(MANET_E_INVALID, "add and the fused output layer are exclusive");
    dim3 grid((unsigned)((HW + X3_P - 1) / X3_P), (unsigned)B);
    if (pieces == 3) {
        hipLaunchKernelGGL(conv1x1_x3_kernel<3>, grid, dim3(X3_NT), 0, (hipStream_t)stream, in, (long)in_batch_stride, Cin, (long)HW,
                           (const char *)wpk, b2, add, relu_out, out, head_w, head_b, head_out);
        return manet_check_launch("manet_conv1x1_x6_f32");
    }
    hipLaunchKernelGGL(conv1x1_x3_kernel<2>, grid, dim3(X3_NT), 0, (hipStream_t)stream, in, (long)in_batch_stride, Cin, (long)HW,
                       (const char *)wpk, b2, add, relu_out, out, head_w, head_b, head_out);
    return manet_check_launch("manet_conv1x1_x3_f32");
}

// ---- head_act="f16": fp16 activations between the stages of a DynamicSegHead -------------------------------------------------
// depthwise 7x7 + bias + folded bn1 + ReLU, fp16 out = rn16(min(., 65504)); in_f16 != 0: the input planes are fp16 too (layers
// 2-4), else fp32 (layer 1).  The even-w form only.
extern "C" int manet_dwconv7x7_bn_relu_f16(const void *in, int in_f16, int B, int C, int h, int w, const float *weight,
                                           const float *bias, const float *bn_scale, const float *bn_shift, void *out,
                                           manet_stream_t stream)
{
    if (!in) return manet_set_error(MANET_E_INVALID, "in is NULL");
    if (!weight) return manet_set_error(MANET_E_INVALID, "weight is NULL");
    if (!out) return manet_set_error(MANET_E_INVALID, "out is NULL");
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0 || (long)B * C > 65535)
        return manet_set_error(MANET_E_INVALID, "bad shape B=%d C=%d h=%d w=%d (B*C must be <= 65535)", B, C, h, w);
    if (w % 2 != 0) return manet_set_error(MANET_E_INVALID, "w=%d must be even (rows of halves are read and written in pairs)", w);
    if (((size_t)in & 7) != 0 || ((size_t)out & 7) != 0) return manet_set_error(MANET_E_INVALID, "in / out must be 8-byte aligned");
    const int ntx = (w + DW_TX - 1) / DW_TX, nty = (h + DW_TY - 1) / DW_TY;
    const int rem = w - (ntx - 1) * DW_TX;  // (the tile plan of manet_dwconv7x7_bn_relu_ex)
    const bool narrow = ntx >= 2 && rem <= DwNarrow::TX && manet_tune_get(MANET_TUNE_DW_NARROW, 1) != 0;
    const int nstd = narrow ? (ntx - 1) * nty : ntx * nty;
    const int ntile = narrow ? nstd + (h + DwNarrow::TY - 1) / DwNarrow::TY : nstd;
    const int per_item = (B > 1 && (long)ntile * C < 512) ? 1 : 0;
    const long planes = per_item ? (long)B * C : C;
    const long nblocks = 8L * ntile * ((planes + 7) / 8);
    if (nblocks > 0x7fffffffL) return manet_set_error(MANET_E_INVALID, "too many tiles for one launch");
    dim3 grid((unsigned)nblocks);
    if (in_f16)
        hipLaunchKernelGGL(dwconv7x7_bn_relu_f16_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, B, C, h, w, weight, bias,
                           bn_scale, bn_shift, (_Float16 *)out, per_item, ntx, nty, nstd, ntile);
    else
        hipLaunchKernelGGL(dwconv7x7_bn_relu_f16_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, B, C, h, w, weight, bias,
                           bn_scale, bn_shift, (_Float16 *)out, per_item, ntx, nty, nstd, ntile);
    return manet_check_launch("manet_dwconv7x7_bn_relu_f16");
}

// bytes of the packed fp16 weight image of a [Cin][256] 1x1 layer (manet_conv1x1_f16_pack)
extern "C" int64_t manet_conv1x1_f16_weight_bytes(int Cin) { return Cin <= 0 ? 0 : (int64_t)((Cin + H16_KC - 1) / H16_KC) * H16_WCHUNK; }

extern "C" int manet_conv1x1_f16_pack(const float *w2t, int Cin, int Cout, void *wpk, manet_stream_t stream)
{
    if (!w2t) return manet_set_error(MANET_E_INVALID, "w2t is NULL");
    if (!wpk) return manet_set_error(MANET_E_INVALID, "wpk is NULL");
    if (Cin <= 0) return manet_set_error(MANET_E_INVALID, "Cin=%d must be positive", Cin);
    if (Cout != PW_CO) return manet_set_error(MANET_E_INVALID, "Cout=%d (this kernel is built for %d output channels)", Cout, PW_CO);
    if (((size_t)wpk & 15) != 0) return manet_set_error(MANET_E_INVALID, "wpk must be 16-byte aligned");
    const int n = (Cin + H16_KC - 1) / H16_KC;
    hipLaunchKernelGGL(conv1x1_f16_pack_kernel, dim3((unsigned)(n * 2)), dim3(256), 0, (hipStream_t)stream, w2t, Cin, (uint4 *)wpk, n);
    return manet_check_launch("manet_conv1x1_f16_pack");
}

// 1x1 convolution with 256 output channels on the fp16 MFMA (conv1x1_f16_kernel): in [B][Cin][HW] fp16, out [B][256][HW] fp16, or
// head_w != NULL: the fused fp32 logits head_out [B][HW] (`out` is not written); out_f32 != 0: out is [B][256][HW] fp32, unrounded
extern "C" int manet_conv1x1_f16(const void *in, int64_t in_batch_stride, int B, int Cin, int64_t HW, const void *wpk,
                                 const float *b2, const float *add, int Cout, int relu_out, void *out, int out_f32,
                                 const float *head_w, const float *head_b, float *head_out, manet_stream_t stream)
{
    if (!in) return manet_set_error(MANET_E_INVALID, "in is NULL");
    if (!wpk) return manet_set_error(MANET_E_INVALID, "wpk is NULL");
    if (!b2) return manet_set_error(MANET_E_INVALID, "b2 is NULL");
    if (!out && !head_w) return manet_set_error(MANET_E_INVALID, "out is NULL (and no fused output layer: head_w is NULL)");
    if (head_w && !head_out) return manet_set_error(MANET_E_INVALID, "head_out is NULL");
    if (B <= 0 || B > 65535 || Cin <= 0 || HW <= 0) return manet_set_error(MANET_E_INVALID, "bad shape B=%d Cin=%d HW=%lld", B, Cin, (long long)HW);
    if (Cout != PW_CO) return manet_set_error(MANET_E_INVALID, "Cout=%d (this kernel is built for %d output channels)", Cout, PW_CO);
    if (HW % 8 != 0) return manet_set_error(MANET_E_INVALID, "HW=%lld must be a multiple of 8 (16-byte LDS-DMA rows of halves)", (long long)HW);
    if (((size_t)wpk & 15) != 0 || ((size_t)in & 15) != 0 || (in_batch_stride & 7) != 0 || ((size_t)out & 15) != 0 || ((size_t)add & 15) != 0)
        return manet_set_error(MANET_E_INVALID, "in / wpk / out / add must be 16-byte aligned, in_batch_stride a multiple of 8 elements");
    if (head_w && add) return manet_set_error(MANET_E_INVALID, "add and the fused output layer (head_w) are exclusive");
    dim3 grid((unsigned)((HW + H16_P - 1) / H16_P), (unsigned)B);
    if (head_w)
        hipLaunchKernelGGL(conv1x1_f16_kernel<true>, grid, dim3(H16_NT), 0, (hipStream_t)stream, (const _Float16 *)in, (long)in_batch_stride,
                           Cin, (long)HW, (const char *)wpk, b2, add, relu_out, out, head_w, head_b, head_out);
    else if (out_f32)
        hipLaunchKernelGGL((conv1x1_f16_kernel<false, true>), grid, dim3(H16_NT), 0, (hipStream_t)stream, (const _Float16 *)in,
                           (long)in_batch_stride, Cin, (long)HW, (const char *)wpk, b2, add, relu_out, out, head_w, head_b, head_out);
    else
        hipLaunchKernelGGL(conv1x1_f16_kernel<false>, grid, dim3(H16_NT), 0, (hipStream_t)stream, (const _Float16 *)in, (long)in_batch_stride,
                           Cin, (long)HW, (const char *)wpk, b2, add, relu_out, out, head_w, head_b, head_out);
    return manet_check_launch("manet_conv1x1_f16");
}

// DynamicSegHead layer 1, per-object half, head_act="f16", one launch (head_layer1_object_f16_kernel): the bits of
// manet_dwconv7x7_bn_relu_f16 (fp32 in) on planes [n][Cp][h][w] followed by manet_conv1x1_f16 with `add` = term
extern "C" int manet_head_layer1_object_f16(const float *planes, int n, int Cp, int h, int w, const float *dw_weight,
                                            const float *dw_bias, const float *bn_scale, const float *bn_shift, const void *wpk,
                                            const float *b2, const float *term, int relu_out, void *out, manet_stream_t stream)
{
    if (!planes) return manet_set_error(MANET_E_INVALID, "planes is NULL");
    if (!dw_weight) return manet_set_error(MANET_E_INVALID, "dw_weight is NULL");
    if (!wpk) return manet_set_error(MANET_E_INVALID, "wpk is NULL");
    if (!b2) return manet_set_error(MANET_E_INVALID, "b2 is NULL");
    if (!out) return manet_set_error(MANET_E_INVALID, "out is NULL");
    if (n < 1) return manet_set_error(MANET_E_INVALID, "n=%d must be at least 1", n);
    if (Cp < 1 || Cp > 4) return manet_set_error(MANET_E_INVALID, "Cp=%d must be 1..4 (the per-object channels share one k block)", Cp);
    if (h < 1 || w < 1) return manet_set_error(MANET_E_INVALID, "bad shape h=%d w=%d", h, w);
    if (w % 2 != 0) return manet_set_error(MANET_E_INVALID, "w=%d must be even", w);
    const int64_t HW = (int64_t)h * w;
    if (HW % 8 != 0 || HW < 8 || HW > 0x7fffffff / 4)
        return manet_set_error(MANET_E_INVALID, "h*w=%lld must be a multiple of 8, at least 8 (and at most 2^29 - 1)", (long long)HW);
    if (((size_t)wpk & 15) != 0) return manet_set_error(MANET_E_INVALID, "wpk must be 16-byte aligned");
    if (((size_t)term & 15) != 0) return manet_set_error(MANET_E_INVALID, "term must be 16-byte aligned");
    if (((size_t)out & 15) != 0) return manet_set_error(MANET_E_INVALID, "out must be 16-byte aligned");
    dim3 grid((unsigned)((HW + L16_P - 1) / L16_P));
    hipLaunchKernelGGL(head_layer1_object_f16_kernel, grid, dim3(L16_NT), 0, (hipStream_t)stream, planes, n, Cp, h, w, dw_weight,
                       dw_bias, bn_scale, bn_shift, (const uint4 *)wpk, b2, term, relu_out, (_Float16 *)out);
    return manet_check_launch("manet_head_layer1_object_f16");
}
