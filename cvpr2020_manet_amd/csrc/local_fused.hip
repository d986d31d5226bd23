// The fused local-window kernel, MI355X (gfx950): networks/IntVOS.py:266-315 and :345-434 in the live configuration (downsample on).
// csrc/local_match.hip holds the unfused kernels of the same formula, csrc/local_train.hip the training path, csrc/local_geom.h
// the geometry, the launch plan (lf_plan) and what the three files share.
//
// FUSED local match (the live configuration: downsample on): window distances -> normalise -> bilinear ->
// stride-2 label gather -> masked min in ONE kernel behind the pooling pass; the (2d+1)^2 volume never touches
// memory (r1: pooled volume written and re-read by a third launch, 47 us at d=4 / 125 us at d=12).
//
// Decomposition.  A full-resolution pixel (y, x) reads the pooled volume at rows {i0, i1}, columns {j0, j1}
// (bilinear, align_corners).  A workgroup owns the pixels whose (i0, j0) falls into a TY x 15 block of the
// pooled grid; they need the volume on a (TY+1) x 16 block S (a one-sided apron), for every window offset.
//   phase 1  distances on S: thread = (row of S, window row dy, group of COLS columns[, half of the window columns]);
//            running sums over C held as packed pairs of neighbouring window positions (v_pk_add_f32 / v_pk_fma_f32);
//            channels staged through LDS in double-buffered stages by asm LDS-DMA, one barrier per stage; a thread
//            slides its window over the offsets out of registers, the channel loop rotated by hand.  Per stored sum the
//            same ascending chain of fma(d, d, acc), d = x - y, as local_dist_kernel and the oracle.
//   phase 2  the normalised volume of S goes to LDS ([dy][cell][dx], dx contiguous), the previous frame's labels
//            around the tile too (one byte each, prefetched during phase 1), and every (pixel, window row) item walks
//            its row four columns at a time: b128 taps, the oracle's bilinear expression on two columns per packed op,
//            an LDS atomic min on the float bits into the (id, pixel) slot.  Bit-identical to r1's three-launch path
//            (local_dist_kernel -> local_min_kernel), which shares manet_normalize_dist_local.
// The pooling pass writes PADDED planes (lf_pool_pad_kernel): a border of the reference's padding value (1e20 for
// the previous frame, IntVOS.py:287) wide enough that no tile ever leaves the plane, rows a multiple of 16 bytes --
// staging is branch-free -- and the tile table (first pixel row / column of every tile).
// Wide windows (d >= 7) use COLS = 4: window reads are aligned ds_read_b128 and feed 4 x P fma pairs.
// For d >= 11 the window rows are dealt to NDG workgroups per tile (d=11: 2, d=12: 5); their partial minima meet
// by atomicMin on the float bits (all candidates lie in [0, 1]; `out` is pre-set to 1.0, the reference's
// "no match" value, IntVOS.py:429-430).
// DESIGN.md 3.4 has the measured phase timeline and the VALU-rate analysis.
#include "manet_common.h"
#include "local_geom.h"

namespace {

// IntVOS.py:282-284 F.avg_pool2d(x, (2,2), (2,2)) of both frames into padded planes: window summed row-major,
// times 1/4 (exact) -- the arithmetic of pool2x2_kernel; border = 0 for the current frame (never used), 1e20 for
// the previous frame (IntVOS.py:287: (x - 1e20)^2 = inf -> 1.0 after normalisation, no bounds logic downstream)
__device__ __forceinline__ float lf_ld(const float *p, long i) { return p[i]; }
__device__ __forceinline__ float lf_ld(const unsigned short *p, long i) { return __uint_as_float((unsigned)p[i] << 16); }  // bf16
// out_init != nullptr (window rows dealt to several workgroups per tile): `out` is pre-set to 1.0 here, the value the
// partial minima are atomicMin'ed into -- one launch fewer than a separate fill.
template <typename SRC>  // float, or bf16 as raw 16-bit words (the producer's storage)
__global__ void lf_pool_pad_kernel(const SRC *__restrict__ a, long a_sy, long a_sx, long a_sc,
                                   const SRC *__restrict__ b, long b_sy, long b_sx, long b_sc, int C, int hp, int wp,
                                   int d, int HPAD, int WS, float *__restrict__ ap, float *__restrict__ bp,
                                   float *__restrict__ out_init, long n_out, int *__restrict__ tab, int TY, int TX,
                                   int nty, int ntx, int h, int w)
{
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long plane = (long)HPAD * WS;
    if (out_init && i < n_out) out_init[i] = 1.0f;  // the launcher checked n_out <= plane * C
    // tile table of the fused kernel: tile row t owns the full-resolution rows [tab[t], tab[t+1]) (those whose upper
    // bilinear source row i0 lies in [t TY, (t+1) TY)), tile column t the columns [tab[nty+1+t], tab[nty+2+t]).
    // Computed here once instead of by every workgroup (four divisions and two scans on its critical path).
    if (i <= nty) tab[i] = bilin_first((int)i * TY, hp, h);
    else if (i <= nty + 1 + ntx) tab[i] = bilin_first((int)(i - nty - 1) * TX, wp, w);
    if (i >= plane * C) return;
    int c = (int)(i / plane);
    int rem = (int)(i - (long)c * plane);
    int r = rem / WS, col = rem - r * WS;
    int py = r - d, px = col - d;
    float va = 0.0f, vb = 1e20f;
    if (py >= 0 && py < hp && px >= 0 && px < wp) {
        const SRC *p = a + (2L * py) * a_sy + (2L * px) * a_sx + (long)c * a_sc;
        const SRC *q = b + (2L * py) * b_sy + (2L * px) * b_sx + (long)c * b_sc;
        va = (((lf_ld(p, 0) + lf_ld(p, a_sx)) + lf_ld(p, a_sy)) + lf_ld(p, a_sy + a_sx)) * 0.25f;
        vb = (((lf_ld(q, 0) + lf_ld(q, b_sx)) + lf_ld(q, b_sy)) + lf_ld(q, b_sy + b_sx)) * 0.25f;
    }
    ap[i] = va;
    bp[i] = vb;
}

// wave-uniform counted wait (LDS-DMA pieces and asm-issued loads are invisible to the compiler's own counters)
__device__ __forceinline__ void lf_wait_vmcnt(int n)
{
    switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
    case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
    case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
    case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
    case 17: asm volatile("s_waitcnt vmcnt(17)" ::: "memory"); break;
    case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
    case 19: asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); break;
    case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;  // (more pieces per wave than the table: wait for all)
    }
}
typedef _Float16 lf_h4 __attribute__((ext_vector_type(4)));
// four neighbouring window columns of one cell, widened to fp32 (exact)
__device__ __forceinline__ f32x4 lf_tap4(const float *p) { return *(const f32x4 *)p; }
__device__ __forceinline__ f32x4 lf_tap4(const _Float16 *p) { return __builtin_convertvector(*(const lf_h4 *)p, f32x4); }
template <int MODE>
using LfExtra = typename std::conditional<MODE == LF_VOL_OUT, LfBatch, typename std::conditional<MODE == LF_VOL_IN, LfTab, int>::type>::type;
// The body of local_fused_kernel<D, MODE> (VT = float: the volume image as fp32, every mode) and of local_fused_f16_kernel<D, MODE>
// (VT = _Float16: LF_VOL_OUT rounds each normalised distance once to IEEE half, to nearest even, subnormals kept; LF_VOL_IN widens
// the taps back to fp32 and runs the same expression).
template <int D, int MODE, typename VT>
__device__ __forceinline__ void lf_body(const float *__restrict__ curp_arg, const float *__restrict__ prevp_arg, int WS, long PS,
                                        const int *__restrict__ labels, int h, int w, int C, int n_ids, float *__restrict__ out,
                                        const int *__restrict__ tab, int /* always 0 */, int ntx, int nty, int rw, int rh,
                                        VT *__restrict__ vol_arg, const LfExtra<MODE> batch)
{
    static_assert(sizeof(VT) == 4 || MODE != LF_FUSED, "the fp16 image exists in memory only");
    constexpr bool F16 = sizeof(VT) == 2;
    const float *curp = curp_arg, *prevp = prevp_arg;
    VT *vol = vol_arg;
    if constexpr (MODE == LF_VOL_OUT) {
        curp = batch.cur[blockIdx.y];
        prevp = batch.prev[blockIdx.y];
        vol = (VT *)batch.vol[blockIdx.y];
    }
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int P = 2 * D + 1, NT = lf_nt(D), ND = lf_nd(D), NDG = lf_ndg(D), SY = lf_sy(D), TY = SY - 1;
    constexpr int TX = LF_SX - 1, CW = lf_cw(D), YR = lf_yr(D), CC = lf_cc(D), COLS = lf_cols(D), NG = LF_SX / COLS;
    constexpr int DXS = lf_dxs(D), PA = lf_pa(D), LF_PH = lf_ph(D);
    constexpr int yplane = YR * CW, xplane = SY * LF_SX;
    constexpr int NVY = yplane / 4, NVX = xplane / 4;          // float4 per channel
    constexpr int NITEM = CC * (NVY + NVX);                    // float4 per stage
    constexpr int NPIECE = (NITEM + 63) / 64;                  // 1 KiB LDS-DMA pieces per stage
    constexpr int NWV = NT / 64, KD = (NPIECE + NWV - 1) / NWV;  // pieces per wave
    constexpr int buf_floats = lf_stage_floats(D);             // = NPIECE * 256
    float *smem = (float *)smem_raw;
    const int tid = threadIdx.x;
    const int hp = h / 2, wp = w / 2;
    // XCD-aware block -> (tile column, tile row, window-row group): block L runs on XCD L % 8 (observed, used for speed
    // only), whose L2 serves the staging DMA.  Each XCD gets a compact rw x rh block of tiles (4 x 2 such regions cover the
    // grid) with all their window-row groups: its L2 then holds about a fifth of each pooled plane (region + halo) instead
    // of a full-height strip per tile column -- r3 PMC at 480p, d=12: the kernel's fabric fetch 33 -> 22 MB.
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int tix = (xcd & 3) * rw + idx % rw, tmp_ = idx / rw;
    const int tiy = (xcd >> 2) * rh + tmp_ % rh, tiz = tmp_ / rh;
    if (tix >= ntx || tiy >= nty) return;  // (the regions' padding)
    const int a = tiy * TY, b0 = tix * TX;  // pooled origin of S
    const int dy0 = tiz * ND;  // first window row of this workgroup
    // window rows this workgroup really owns (the last image of a tile may hold fewer)
    const int nd_here = min(P - dy0, ND);
    if (nd_here <= 0) return;
    VT *vimg = MODE == LF_FUSED ? nullptr : vol + (long)((tiz * nty + tiy) * ntx + tix) * lf_img_elems<VT>(D);

    // ---- phase 1: distances on S for window rows dy0 .. dy0+ND-1 ---------------------------------
    // Staging by LDS-DMA (lds_dma16: 64 lanes x 16 bytes land in 1 KiB of LDS, no VGPR hop, no ds_write): a stage is
    // NPIECE such pieces, dealt round-robin to the waves.  The stage image is [CC][YR][CW] previous-frame halo rows then
    // [CC][SY][16] current-frame rows; a lane's 16 bytes of piece p are float4 number 64 p + lane of that image.  Its
    // source address for stage 0 is computed once (below); every later stage is a uniform step of CC planes.
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned smem_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)smem_raw);
    const float *src[KD];
    int sch[KD];  // the item's channel inside the stage (the last stage may run past C: clamped there)
#pragma unroll
    for (int k = 0; k < KD; ++k) {
        int i = (k * NWV + wave) * 64 + lane;
        i = i < NITEM ? i : NITEM - 1;  // the tail of the last piece lands in the padding of the stage image
        if (i < CC * NVY) {
            const int c = i / NVY, v = i - c * NVY;
            const int r = v / (CW / 4), q = v - r * (CW / 4);
            // padded coordinates: image row a - D + dy0 + r sits at plane row a + dy0 + r
            src[k] = prevp + (long)c * PS + (a + dy0 + r) * WS + b0 + 4 * q;
            sch[k] = c;
        } else {
            const int j = i - CC * NVY;
            const int c = j / NVX, v = j - c * NVX;
            const int r = v / 4, q = v - r * 4;
            src[k] = curp + (long)c * PS + (D + a + r) * WS + D + b0 + 4 * q;
            sch[k] = c;
        }
    }
    auto stage_dma = [&](int c0, int buf) __attribute__((always_inline)) {
        const bool tail = c0 + CC > C;  // uniform
#pragma unroll
        for (int k = 0; k < KD; ++k) {
            if (k * NWV + wave < NPIECE) {  // wave-uniform
                const float *g_ = src[k] + (long)c0 * PS;
                if (tail) {
                    const int over = c0 + sch[k] - (C - 1);
                    if (over > 0) g_ -= (long)over * PS;  // channels past C re-read plane C-1; the arithmetic skips them
                }
                lds_dma16(g_, smem_base + (unsigned)buf * (unsigned)(buf_floats * 4) + (unsigned)(k * NWV + wave) * 1024u);
            }
        }
    };

    // lane -> (column group, slot): the window half is the thread index's TOP bit, so a wave's lanes read the same half
    // (with lf_cw's row stride that keeps every b128 lane group of the window reads conflict-free)
    const int g = tid % NG;
    constexpr bool XH_TOP = COLS == 4;  // (b64 reads of the COLS = 2 kernels: 32-lane groups, the interleaved order measured better)
    const int xh = XH_TOP ? tid / (NT / DXS) : (tid / NG) % DXS;  // which half of the window columns
    const int slot = XH_TOP ? (tid % (NT / DXS)) / NG : tid / (NG * DXS);
    const int dyi = slot % ND;
    const int ry = slot / ND;
    const bool active = ry < SY;
    const int dx_lo = xh * LF_PH;
    const int ndx = (xh == DXS - 1) ? P - dx_lo : LF_PH;  // window columns this thread really owns (<= PA)
    constexpr int WN = (COLS + PA - 1 + COLS - 1) / COLS * COLS;  // window floats read per channel (whole vectors)
    // Running sums, held as PAIRS of neighbouring window positions k = dx + j (k even first): one v_pk_add_f32 and one
    // v_pk_fma_f32 do two (x - y)^2 steps.  A wave issues a VALU instruction every ~5 cycles whatever its width
    // (tools/ubench/valu_rate.hip: v_fma_f32 5.3, v_pk_fma_f32 5.5 ticks per instruction per wave, flat from 1 to 4 waves
    // per SIMD), so at the 2 waves per SIMD this kernel runs at, packed math is twice the arithmetic per issue slot.
    // The packed operands must be even-aligned register pairs, which window pairs starting at even k are (they come out
    // of b64 / b128 LDS reads); column j's range k = j .. j+PA-1 is covered by the aligned pairs around it, so up to
    // one lane per end accumulates a neighbour that is never stored.  Every stored sum is the same ascending chain of
    // fma(d, d, acc), d = x - y, as local_dist_kernel's and the oracle's.
    constexpr int NP = (PA + 2) / 2;  // pairs per column
    f32x2 accp[COLS][NP];             // sum (j, dx) = accp[j][(dx + (j & 1)) >> 1][(dx + j) & 1]
#define LF_ACC(j_, dx_) accp[j_][((dx_) + ((j_) & 1)) >> 1][((dx_) + (j_)) & 1]
#pragma unroll
    for (int j = 0; j < COLS; ++j)
#pragma unroll
        for (int i = 0; i < NP; ++i) accp[j][i] = f32x2{0.0f, 0.0f};

    // One channel's operands: the thread's COLS current-frame values and its WN-wide slice of the previous frame's row
    struct Chan {
        f32x2 win[WN / 2];
        float xv[COLS];
    };
    auto compute = [&](int buf_, int nch) __attribute__((always_inline)) {
        if (active) {
        const float *ys = smem + (long)buf_ * buf_floats + (ry + dyi) * CW + COLS * g + dx_lo;
        const float *xs = smem + (long)buf_ * buf_floats + CC * yplane + ry * LF_SX + COLS * g;
        auto fetch = [&](Chan &W, int c) __attribute__((always_inline)) {
            const float *yrow = ys + c * yplane;
            const float *xrow = xs + c * xplane;
            if constexpr (COLS == 2) {
                const f32x2 t = *(const f32x2 *)xrow;
                W.xv[0] = t[0];
                W.xv[1] = t[1];
#pragma unroll
                for (int i = 0; i < WN / 2; ++i) W.win[i] = *(const f32x2 *)(yrow + 2 * i);
            } else {
                const f32x4 t = *(const f32x4 *)xrow;
#pragma unroll
                for (int j = 0; j < 4; ++j) W.xv[j] = t[j];
#pragma unroll
                for (int i = 0; i < WN / 4; ++i) {
                    const f32x4 u = *(const f32x4 *)(yrow + 4 * i);
                    W.win[2 * i] = f32x2{u[0], u[1]};
                    W.win[2 * i + 1] = f32x2{u[2], u[3]};
                }
            }
        };
        auto fma_chan = [&](const Chan &U) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < COLS; ++j) {
                const f32x2 xx = {U.xv[j], U.xv[j]};
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const int kp = (j >> 1) + i;  // window pair (2 kp, 2 kp + 1)
                    if (2 * kp <= j + PA - 1) {
                        const f32x2 dd = xx - U.win[kp];
                        accp[j][i] = __builtin_elementwise_fma(dd, dd, accp[j][i]);
                    }
                }
            }
        };
        // the channel loop rotated by hand: channel c+1's LDS reads are issued before channel c's arithmetic
        Chan W0, W1;  // loop-carried: the loop stays rolled, or the compiler hoists every channel's reads and spills
        fetch(W0, 0);
        int c = 0;
#pragma unroll 1
        for (; c + 2 < nch; c += 2) {  // branch-free body (a conditional fetch costs a register shuffle per trip)
            fetch(W1, c + 1);
            fma_chan(W0);
            fetch(W0, c + 2);
            fma_chan(W1);
        }
        if (c + 1 < nch) {
            fetch(W1, c + 1);
            fma_chan(W0);
            fma_chan(W1);
        } else {
            fma_chan(W0);
        }
    }
    };
    if constexpr (MODE != LF_VOL_IN) {
        stage_dma(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // LF_VOL_IN: order of the memory traffic.  (1) the label loads -- issued from asm so that the compiler's own counted waits (which
    // know nothing of the LDS-DMA pieces behind them) do not drain the volume stream when the labels are used; their addresses come
    // from the host's tile table, i.e. from the kernel argument: no dependent memory round trip; (2) the volume image of this (tile,
    // window-row group), all pieces; then counted waits: the labels (oldest) -> label bytes, change masks, tables, minima; the first
    // VR1 window rows -> their items; the rest -> the other items.  The launch is one wave of workgroups: without this every
    // workgroup waited 7 us for the whole 25.8 MB and then all of them computed (timeline in docs/history/r06_experiments.md).
    constexpr int VR1 = (2 * ND) / 5 > 0 ? (2 * ND) / 5 : 1;  // window rows whose items start first
    constexpr int IMG_PIECES = (int)(lf_vpad_bytes(D, ND, sizeof(VT)) / 1024);  // (whole 1 KiB pieces: the tail lands in the V region's padding)
    // the fetch of an image ends at most 1 KiB behind it: the slack manet_local_volume_bytes[_f16] adds behind the last image
    static_assert(MODE != LF_VOL_IN || (size_t)IMG_PIECES * 1024 <= (size_t)lf_img_elems<VT>(D) * sizeof(VT) + 1024,
                  "the stored-volume tail would fetch past the volume's 1 KiB of slack");
    constexpr int IMG_P1 = ND > VR1 ? (VR1 * SY * LF_SX * lf_vs(D) * (int)sizeof(VT) + 1023) / 1024 : IMG_PIECES;
    // this wave's pieces among the first x pieces of the image (dealt round-robin)
    auto my_pieces = [&](int x) __attribute__((always_inline)) { return x > wave ? (x - wave + NWV - 1) / NWV : 0; };
    // full-resolution pixels of this tile: rows with i0(y) in [a, a+TY), columns with j0(x) in [b0, b0+TX) -- the
    // pooling pass left the ranges in `tab`
    int ya = 0, yb = 0, xa = 0, xb = 0;
    bool host_tab = false;
    if constexpr (MODE == LF_VOL_IN) host_tab = batch.n > 0;
    if constexpr (MODE == LF_VOL_IN) {
        if (host_tab) {
            ya = batch.v[tiy], yb = batch.v[tiy + 1];
            xa = batch.v[nty + 1 + tix], xb = batch.v[nty + 2 + tix];
        }
    }
    if (!host_tab) {
        ya = tab[tiy], yb = tab[tiy + 1];
        xa = tab[nty + 1 + tix], xb = tab[nty + 2 + tix];
    }
    const int ny = yb - ya, nx = xb - xa;
    if (ny > 2 * TY + 4 || nx > 2 * TX + 4) __builtin_trap();  // cannot happen (ratio (hp-1)/(h-1) < 1/2): fail loudly, never overrun L
    // the previous frame's labels around the tile: rows ya + 2(dy0 - D) .., columns xa - 2D ..; outside the image = 0
    // (zero padding, IntVOS.py:400).  Loaded NOW (behind the first two stages' loads, under the first stage's arithmetic), used after phase 1: they come
    // from HBM (nobody has touched them this frame) and would otherwise cost a full miss latency between the phases
    constexpr int KL = (lf_lab_rows_of(D, ND) * lf_lab_cols(D) + NT - 1) / NT;
    const int lrows = ny + 2 * (ND - 1), lcols = nx + 4 * D;
    const int ly0 = ya + 2 * (dy0 - D), lx0 = xa - 2 * D;
    int labr[KL];
#pragma unroll
    for (int k = 0; k < KL; ++k) {
        const int e = tid + NT * k;
        const int r = e / lcols, c = e - r * lcols;
        const int yy = ly0 + r, xx = lx0 + c;
        const int yc = yy < 0 ? 0 : (yy < h ? yy : h - 1), xc = xx < 0 ? 0 : (xx < w ? xx : w - 1);
        int idx = yc * w + xc;
        asm volatile("" : "+v"(idx));  // the compiler must not turn the clamp back into a branch around the load:
        int v = 0;                     // unconditional loads issue back to back, a branchy one waits vmcnt(0) each time
        if constexpr (MODE == LF_FUSED) v = labels[idx];
        if constexpr (MODE == LF_VOL_IN) {
            const unsigned boff = 4u * (unsigned)idx;
            asm volatile("global_load_dword %0, %1, %2" : "=v"(v) : "v"(boff), "s"(labels) : "memory");
            labr[k] = v;  // (masked below, after the wait: the asm load's result must not be touched before it)
        } else {
            labr[k] = (yy == yc && xx == xc) ? v : 0;
        }
    }
    if constexpr (MODE == LF_VOL_IN) {
        for (int pc = wave; pc < IMG_PIECES; pc += NWV) lds_dma16((const float *)vimg + (pc * 64 + lane) * 4, smem_base + (unsigned)pc * 1024u);
        lf_wait_vmcnt(my_pieces(IMG_PIECES));  // the label loads are older than this wave's pieces: they have landed
    }
    if constexpr (MODE == LF_VOL_IN) {
#pragma unroll
        for (int k = 0; k < KL; ++k) {
            asm volatile("" : "+v"(labr[k]));  // (uses stay behind the wait)
            const int e = tid + NT * k;
            const int r = e / lcols, c = e - r * lcols;
            const int yy = ly0 + r, xx = lx0 + c;
            const bool inside = yy >= 0 && yy < h && xx >= 0 && xx < w;
            labr[k] = inside ? labr[k] : 0;
        }
    }

    // stage s is in LDS buffer s & 1.  The DMA of stage s + 1 into the other buffer (free: its last readers passed the
    // barrier) is issued first and runs under the arithmetic of stage s; the wave waits for its own pieces (vmcnt --
    // the DMA is hidden from the compiler's counters, this is the only wait on it) and the barrier publishes them.
    if constexpr (MODE != LF_VOL_IN) {
        for (int c0 = 0, st_i = 0; c0 < C; c0 += CC, ++st_i) {
            if (c0 + CC < C) stage_dma(c0 + CC, (st_i & 1) ^ 1);
            compute(st_i & 1, (C - c0) < CC ? (C - c0) : CC);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }

    constexpr int VS = lf_vs(D), NPS = lf_npix(D);
    VT *V = (VT *)smem;                                              // [ND][SY * 16][VS] (+ the tail of the last LDS-DMA piece)
    unsigned char *L = (unsigned char *)smem + lf_vpad_bytes(D, ND, sizeof(VT));  // [lab_rows][lab_cols]; a byte >= the pass's ids = "no id"
    if (MODE != LF_VOL_IN && active) {
        VT *vp0 = V + ((dyi * SY + ry) * LF_SX + COLS * g) * VS + dx_lo;
#pragma unroll
        for (int j = 0; j < COLS; ++j) {
#pragma unroll
            for (int d4 = 0; d4 < PA; d4 += 4) {
                if (LF_PH % 4 == 0 && d4 + 3 < PA && d4 + 3 < ndx) {
                    f32x4 t;
#pragma unroll
                    for (int i = 0; i < 4; ++i) t[i] = manet_normalize_dist_local(LF_ACC(j, d4 + i));
                    if constexpr (F16) *(lf_h4 *)(vp0 + j * VS + d4) = __builtin_convertvector(t, lf_h4);  // v_cvt_f16_f32: to nearest even
                    else *(f32x4 *)(vp0 + j * VS + d4) = t;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (d4 + i < PA && d4 + i < ndx) vp0[j * VS + d4 + i] = (VT)manet_normalize_dist_local(LF_ACC(j, d4 + i));
                }
            }
        }
    }
    if constexpr (MODE == LF_VOL_OUT) {
        // the image as phase 2 reads it, to memory in one linear pass (entries no thread wrote -- the cells' padding past the
        // window width, window rows past 2d+1 in the last group -- travel along and are never used)
        __syncthreads();
        constexpr int IMG4 = ND * SY * LF_SX * VS * (int)sizeof(VT) / 16;
        for (int i = tid; i < IMG4; i += NT) ((f32x4 *)vimg)[i] = ((const f32x4 *)V)[i];
        return;
    }
#pragma unroll
    for (int k = 0; k < KL; ++k) {
        const int e = tid + NT * k;
        // one pass over the ids (n_ids <= LF_NIP): store the M2 row directly -- the id, or n_ids for "no id" (the row behind the ids')
        const int lmax = n_ids <= LF_NIP ? n_ids : 255;
        if (e < lrows * lcols) L[e] = (labr[k] >= 0 && labr[k] < (n_ids <= LF_NIP ? n_ids : MANET_MAX_IDS)) ? (unsigned char)labr[k] : (unsigned char)lmax;
    }
    // per-(id, pixel) minima [LF_NIP + 1][NPS] (row LF_NIP collects the candidates whose label is not an id of this
    // pass), then the separable bilinear tables: tap offsets into V and the two weights, per pixel row / column
    unsigned *M2 = (unsigned *)(L + (((size_t)lf_lab_rows_of(D, ND) * lf_lab_cols(D) + 15) & ~(size_t)15));
    const int m2_rows = n_ids <= LF_NIP ? n_ids : LF_NIP;  // + the "no id" row (the launcher sized the LDS for it)
    struct Tap {
        int o0, o1;
        float l0, l1;
    };
    Tap *RT = (Tap *)(M2 + (m2_rows + 1) * NPS), *CT = RT + (2 * TY + 4);
    // r6: label-change masks.  CM[2 r + parity] bit k = (L[r][2 k + parity] != L[r][2 k + 2 + parity]): a (pixel, window row)
    // item's 2d+1 labels are the entries pxx, pxx + 2, .. of one row -- all the SAME iff bits pxx / 2 .. pxx / 2 + 2d - 1 of
    // its parity's mask are zero.  Masks are piecewise constant (objects are blobs): most items then take the minimum of
    // their window row in registers and touch ONE (id, pixel) slot instead of reading 2d+1 label bytes and issuing 2d+1 LDS
    // atomics (the per-pixel phase was LDS-bound on exactly those: 25 + 25 of 78 LDS instructions per item at d = 12).
    unsigned long long *CM = (unsigned long long *)(CT + (2 * TX + 4));
    if constexpr (P > 1) {
        __syncthreads();  // L is complete
        for (int rp = wave; rp < 2 * lrows; rp += NWV) {
            const int r_ = rp >> 1, c0 = 2 * lane + (rp & 1);
            const bool ok = c0 + 2 < lcols;
            const unsigned char *lr = L + r_ * lcols + (ok ? c0 : 0);
            const bool diff = ok && lr[0] != lr[2];
            const unsigned long long m_ = __builtin_amdgcn_ballot_w64(diff);
            if (lane == 0) CM[rp] = m_;
        }
    }
    if (tid < ny) {
        const Bilin cy = bilin_coeff(ya + tid, hp, h);
        RT[tid] = Tap{(cy.i0 - a) * LF_SX * VS, (cy.i1 - a) * LF_SX * VS, cy.l0, cy.l1};
    } else if (tid >= 64 && tid < 64 + nx) {
        const Bilin cx = bilin_coeff(xa + tid - 64, wp, w);
        CT[tid - 64] = Tap{(cx.i0 - b0) * VS, (cx.i1 - b0) * VS, cx.l0, cx.l1};
    }
    // work item = (pixel, window row): every lane busy whatever the tile's pixel count.  The item walks its window
    // row four columns at a time (four b128 taps), and every candidate goes to its (id, pixel) slot by an LDS
    // atomic min on the float bits -- all candidates lie in [0, 1], start value 1.0 = "no match" (IntVOS.py:429-432:
    // where(label == id, dist, 1) then min) -- instead of a compare/select/min per id in registers.
    const int npix = ny * nx;
    const float inv_npix = 1.0f / (float)npix, inv_nx = 1.0f / (float)nx;  // exact quotients below: see DESIGN 3.4
    for (int o0 = 0; o0 < n_ids; o0 += LF_NIP) {
        const int nk = (n_ids - o0) < LF_NIP ? (n_ids - o0) : LF_NIP;
        for (int e = tid; e < nk * NPS; e += NT) M2[e] = 0x3f800000u;  // the rows that are read back
        // (LF_VOL_IN: this wave's pieces of the first VR1 window rows have landed; the barrier publishes everyone's)
        if constexpr (MODE == LF_VOL_IN) lf_wait_vmcnt(my_pieces(IMG_PIECES) - my_pieces(IMG_P1));
        __syncthreads();
        // n_ids <= LF_NIP (one pass): the label byte, clamped to LF_NIP, IS the row of M2
        auto items = [&](auto single_pass, int item_lo, int item_hi) __attribute__((always_inline)) {
            constexpr bool SINGLE = decltype(single_pass)::value;
            for (int item = item_lo + tid; item < item_hi; item += NT) {
                const int by = (int)(((float)item + 0.5f) * inv_npix), pix = item - by * npix;
                const int py = (int)(((float)pix + 0.5f) * inv_nx), pxx = pix - py * nx;
                const Tap r = RT[py], c = CT[pxx];
                const VT *vb = V + by * (SY * LF_SX * VS);
                const VT *p00 = vb + r.o0 + c.o0, *p01 = vb + r.o0 + c.o1, *p10 = vb + r.o1 + c.o0, *p11 = vb + r.o1 + c.o1;
                const unsigned char *lrow = L + (py + 2 * by) * lcols + pxx;
                unsigned *mrow = M2 + pix;
                const f32x2 cl0 = {c.l0, c.l0}, cl1 = {c.l1, c.l1}, rl0 = {r.l0, r.l0}, rl1 = {r.l1, r.l1};
                if constexpr (P > 1) {
                    // every item of this wave sees ONE label along its window row (wave-uniform test: no divergence): the
                    // row's minimum in registers, one atomic.  Same candidates, same minimum: the same bits.
                    const unsigned long long cm = CM[2 * (py + 2 * by) + (pxx & 1)];
                    const bool mixed = ((cm >> (pxx >> 1)) & ((1ull << (P - 1)) - 1ull)) != 0ull;
                    if (__builtin_amdgcn_ballot_w64(mixed) == 0ull) {
                        float m_ = INFINITY;
#pragma unroll
                        for (int q = 0; q < (P + 3) / 4; ++q) {
                            const f32x4 t00 = lf_tap4(p00 + 4 * q), t01 = lf_tap4(p01 + 4 * q);
                            const f32x4 t10 = lf_tap4(p10 + 4 * q), t11 = lf_tap4(p11 + 4 * q);
#pragma unroll
                            for (int i = 0; i < 4; i += 2) {
                                if (4 * q + i >= P) continue;
                                const f32x2 a00 = {t00[i], t00[i + 1]}, a01 = {t01[i], t01[i + 1]};
                                const f32x2 a10 = {t10[i], t10[i + 1]}, a11 = {t11[i], t11[i + 1]};
                                const f32x2 v2 = rl0 * (cl0 * a00 + cl1 * a01) + rl1 * (cl0 * a10 + cl1 * a11);
                                m_ = (4 * q + i + 1 < P) ? fminf(fminf(m_, v2[0]), v2[1]) : fminf(m_, v2[0]);
                            }
                        }
                        unsigned idx = (unsigned)lrow[0];
                        if (!SINGLE) {
                            idx -= (unsigned)o0;
                            idx = idx < (unsigned)LF_NIP ? idx : (unsigned)LF_NIP;
                        }
                        atomicMin(mrow + idx * NPS, __float_as_uint(m_));
                        continue;
                    }
                }
#pragma unroll
                for (int q = 0; q < (P + 3) / 4; ++q) {
                    const f32x4 t00 = lf_tap4(p00 + 4 * q), t01 = lf_tap4(p01 + 4 * q);
                    const f32x4 t10 = lf_tap4(p10 + 4 * q), t11 = lf_tap4(p11 + 4 * q);
#pragma unroll
                    for (int i = 0; i < 4; i += 2) {
                        if (4 * q + i >= P) continue;
                        // two window columns per packed op; per element the expression of bilin_sample / the oracle:
                        // l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11)
                        const f32x2 a00 = {t00[i], t00[i + 1]}, a01 = {t01[i], t01[i + 1]};
                        const f32x2 a10 = {t10[i], t10[i + 1]}, a11 = {t11[i], t11[i + 1]};
                        const f32x2 v2 = rl0 * (cl0 * a00 + cl1 * a01) + rl1 * (cl0 * a10 + cl1 * a11);
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int bx = 4 * q + i + e;
                            if (bx < P) {
                                unsigned idx = (unsigned)lrow[2 * bx];
                                if (!SINGLE) {
                                    idx -= (unsigned)o0;
                                    idx = idx < (unsigned)LF_NIP ? idx : (unsigned)LF_NIP;
                                }
                                atomicMin(mrow + idx * NPS, __float_as_uint(v2[e]));
                            }
                        }
                    }
                }
            }
        };
        // (LF_VOL_IN: the first batch's rows, then -- once the second batch has landed -- the others)
        const int item_mid = (MODE == LF_VOL_IN && ND > VR1) ? npix * (nd_here < VR1 ? nd_here : VR1) : npix * nd_here;
        if (n_ids <= LF_NIP) items(std::true_type{}, 0, item_mid);
        else items(std::false_type{}, 0, item_mid);
        if constexpr (MODE == LF_VOL_IN && ND > VR1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (n_ids <= LF_NIP) items(std::true_type{}, item_mid, npix * nd_here);
            else items(std::false_type{}, item_mid, npix * nd_here);
        }
        __syncthreads();
        for (int e = tid; e < npix * nk; e += NT) {
            const int pix = e / nk, k = e - pix * nk;
            const int py = pix / nx, pxx = pix - py * nx;
            float *o = out + ((long)(ya + py) * w + (xa + pxx)) * n_ids + o0 + k;
            if (NDG == 1) *o = __uint_as_float(M2[k * NPS + pix]);
            else atomicMin((unsigned *)o, M2[k * NPS + pix]);  // several workgroups per tile: `out` was pre-set to 1.0
        }
        __syncthreads();
    }
}

template <int D, int MODE>
__global__ __launch_bounds__(lf_nt(D)) void local_fused_kernel(const float *__restrict__ curp_arg,
                                                               const float *__restrict__ prevp_arg, int WS, long PS,
                                                               const int *__restrict__ labels, int h, int w, int C,
                                                               int n_ids, float *__restrict__ out,
                                                               const int *__restrict__ tab, int abl_arg, int ntx, int nty,
                                                               int rw, int rh, float *__restrict__ vol_arg,
                                                               const LfExtra<MODE> batch)
{
    lf_body<D, MODE, float>(curp_arg, prevp_arg, WS, PS, labels, h, w, C, n_ids, out, tab, abl_arg, ntx, nty, rw, rh, vol_arg, batch);
}
// The two halves on an fp16 image (MODE = LF_VOL_OUT or LF_VOL_IN; the same arguments, the volume as _Float16)
template <int D, int MODE>
__global__ __launch_bounds__(lf_nt(D)) void local_fused_f16_kernel(const float *__restrict__ curp_arg,
                                                                   const float *__restrict__ prevp_arg, int WS, long PS,
                                                                   const int *__restrict__ labels, int h, int w, int C,
                                                                   int n_ids, float *__restrict__ out,
                                                                   const int *__restrict__ tab, int abl_arg, int ntx, int nty,
                                                                   int rw, int rh, _Float16 *__restrict__ vol_arg,
                                                                   const LfExtra<MODE> batch)
{
    static_assert(MODE == LF_VOL_OUT || MODE == LF_VOL_IN, "fp16 images are stored volumes");
    lf_body<D, MODE, _Float16>(curp_arg, prevp_arg, WS, PS, labels, h, w, C, n_ids, out, tab, abl_arg, ntx, nty, rw, rh, vol_arg, batch);
}

__global__ void fill_f32_kernel(float *__restrict__ p, float v, long n)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

// The one launcher of the fused kernel: the kernel of this (radius, mode, storage type) with the plan's figures.
template <int MODE, typename VT = float>
void launch_fused(const LfPlan &P, hipStream_t st, const float *ap, const float *bp, const int *labels, int h, int w, int C,
                  int n_ids, float *out, const int *tab, VT *vol = nullptr, const LfBatch *batch = nullptr)
{
    for_window(P.d, [&](auto dc) {
        constexpr int D = decltype(dc)::value;
        constexpr auto kern = [] {
            if constexpr (sizeof(VT) == 2) return local_fused_f16_kernel<D, MODE>;
            else return local_fused_kernel<D, MODE>;
        }();
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_attr);
        const LfExtra<MODE> extra = [&] {  // the pairs' pointers, the host's tile table, or nothing
            if constexpr (MODE == LF_VOL_OUT) return *batch;
            else if constexpr (MODE == LF_VOL_IN) return P.tab;
            else return 0;
        }();
        hipLaunchKernelGGL(kern, dim3(P.grid_x, P.grid_y), dim3(P.nt), P.lds, st, ap, bp, P.G.WS, P.G.plane, labels, h, w, C, n_ids,
                           out, tab, 0, P.ntx, P.nty, P.rw, P.rh, vol, extra);
    });
}
// ... on prepared frames (manet_frame_prepare): the planes' strides are the frame workspace's own
LfPlan frame_plan(const ManetFrameLayout &F, int h, int w, int d, int mode, int n_ids, size_t elem_bytes, int n_pairs)
{
    LfPlan P = lf_plan(h, w, d, mode, n_ids, elem_bytes, n_pairs);
    P.G = pool_pad_of(F);
    return P;
}

void fill(float *p, float v, long n, unsigned max_blocks, hipStream_t st)
{
    unsigned blocks = (unsigned)((n + 255) / 256);
    if (blocks > max_blocks) blocks = max_blocks;
    hipLaunchKernelGGL(fill_f32_kernel, dim3(blocks), dim3(256), 0, st, p, v, n);
}
// partial minima of several workgroups per tile (lf_ndg(d) > 1) meet by atomicMin: `out` starts from the "no match" value
void preset_out(float *out, long n, hipStream_t st) { fill(out, 1.0f, n, 1024, st); }

int local_volume_bytes(int h, int w, int max_distance, size_t elem_bytes, size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = check_local(h, w, 1, max_distance, 1);
    if (rc) return rc;
    *bytes = lf_volume_bytes(h, w, max_distance, elem_bytes);
    return MANET_OK;
}

template <typename VT>
int local_volume_frames_t(const char *what, const void *const *prev_frame_ws, const void *const *cur_frame_ws, void *const *volumes,
                          int n_pairs, int h, int w, int C, int compute, int max_distance, manet_stream_t stream)
{
    int rc = check_local(h, w, C, max_distance, 1);
    if (rc) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && (!prev_frame_ws || !cur_frame_ws || !volumes)))
        return manet_set_error(MANET_E_INVALID, "bad arguments");
    const ManetFrameLayout F = manet_frame_layout(h, w, C, compute, max_distance);
    hipStream_t st = (hipStream_t)stream;
    for (int i0 = 0; i0 < n_pairs; i0 += LF_BATCH) {
        const int n = (n_pairs - i0) < LF_BATCH ? (n_pairs - i0) : LF_BATCH;
        LfBatch B;
        for (int i = 0; i < LF_BATCH; ++i) {
            const int j = i0 + (i < n ? i : 0);
            if (!prev_frame_ws[j] || !cur_frame_ws[j] || !volumes[j] || ((size_t)volumes[j] & 15))
                return manet_set_error(MANET_E_INVALID, "pair %d: null frame / volume pointer, or a volume not 16-byte aligned", j);
            B.cur[i] = (const float *)((const char *)cur_frame_ws[j] + F.off_plane);
            B.prev[i] = (const float *)((const char *)prev_frame_ws[j] + F.off_plane);
            B.vol[i] = (float *)volumes[j];  // (the kernel of the storage type reads it as VT)
        }
        const int *tab = (const int *)((const char *)cur_frame_ws[i0] + F.off_tab);  // (the same table for every frame of a geometry)
        launch_fused<LF_VOL_OUT, VT>(frame_plan(F, h, w, max_distance, LF_VOL_OUT, 1, sizeof(VT), n), st, nullptr, nullptr, nullptr, h,
                                     w, C, 1, nullptr, tab, nullptr, &B);
    }
    return manet_check_launch(what);
}

template <typename VT>
int local_match_volume_t(const char *what, const VT *volume, const void *cur_frame_ws, const int32_t *prev_labels, int h, int w, int C,
                         int compute, int n_ids, int max_distance, float *out, int out_is_preset, manet_stream_t stream)
{
    int rc = check_local(h, w, C, max_distance, 1);
    if (rc) return rc;
    if ((rc = check_ids(n_ids))) return rc;
    if (!volume || !cur_frame_ws || !prev_labels || !out || ((size_t)volume & 15))
        return manet_set_error(MANET_E_INVALID, "null pointer (or a volume not 16-byte aligned)");
    const ManetFrameLayout F = manet_frame_layout(h, w, C, compute, max_distance);
    hipStream_t st = (hipStream_t)stream;
    const int *tab = (const int *)((const char *)cur_frame_ws + F.off_tab);
    manet_profile_record(st, true, 1);
    if (lf_ndg(max_distance) > 1 && !out_is_preset) preset_out(out, (long)h * w * n_ids, st);
    launch_fused<LF_VOL_IN, VT>(frame_plan(F, h, w, max_distance, LF_VOL_IN, n_ids, sizeof(VT), 1), st, nullptr, nullptr, prev_labels, h,
                                w, C, n_ids, out, tab, (VT *)volume);
    manet_profile_record(st, false, 1);
    return manet_check_launch(what);
}

}  // namespace

void manet_local_fill_zero(float *p, long n, hipStream_t st) { fill(p, 0.0f, n, 2048, st); }

void manet_local_launch_fused(int d, hipStream_t st, const void *cur, long c_sy, long c_sx, long c_sc, const void *prev, long p_sy,
                              long p_sx, long p_sc, int emb_dtype, const int *labels, int h, int w, int C, int n_ids, float *out,
                              float *pooled, int *tab)
{
    const LfPlan P = lf_plan(h, w, d, LF_FUSED, n_ids, sizeof(float), 1);
    const PoolPad &G = P.G;
    float *ap = pooled, *bp = pooled + G.plane * C;
    const long n = G.plane * C;
    // `out` is pre-set by the pooling pass when it has enough threads for it (always, for real shapes), else by a fill
    const long n_out = (long)h * w * n_ids;
    float *init = nullptr;
    if (lf_ndg(d) > 1) {
        if (n_out <= n) init = out;
        else preset_out(out, n_out, st);
    }
    if (emb_dtype == MANET_EMB_BF16)
        hipLaunchKernelGGL(lf_pool_pad_kernel<unsigned short>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           (const unsigned short *)cur, c_sy, c_sx, c_sc, (const unsigned short *)prev, p_sy, p_sx, p_sc, C,
                           G.hp, G.wp, d, G.HPAD, G.WS, ap, bp, init, n_out, tab, P.TY, P.TX, P.nty, P.ntx, h, w);
    else
        hipLaunchKernelGGL(lf_pool_pad_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                           (const float *)cur, c_sy, c_sx, c_sc, (const float *)prev, p_sy, p_sx, p_sc, C, G.hp, G.wp, d,
                           G.HPAD, G.WS, ap, bp, init, n_out, tab, P.TY, P.TX, P.nty, P.ntx, h, w);
    launch_fused<LF_FUSED>(P, st, ap, bp, labels, h, w, C, n_ids, out, tab);
}

extern "C" {

/* the fused kernel on two prepared frames (manet_frame_prepare): no pooling pass, no full-resolution read */
int manet_local_match_frames(const void *prev_frame_ws, const void *cur_frame_ws, const int32_t *prev_labels, int h, int w,
                             int C, int compute, int n_ids, int max_distance, float *out, int out_is_preset,
                             manet_stream_t stream)
{
    int rc = check_local(h, w, C, max_distance, 1);
    if (rc) return rc;
    if ((rc = check_ids(n_ids))) return rc;
    if (!prev_frame_ws || !cur_frame_ws || !prev_labels || !out) return manet_set_error(MANET_E_INVALID, "null pointer");
    const ManetFrameLayout F = manet_frame_layout(h, w, C, compute, max_distance);
    hipStream_t st = (hipStream_t)stream;
    const float *ap = (const float *)((const char *)cur_frame_ws + F.off_plane);
    const float *bp = (const float *)((const char *)prev_frame_ws + F.off_plane);
    const int *tab = (const int *)((const char *)cur_frame_ws + F.off_tab);
    manet_profile_record(st, true, 1);
    if (lf_ndg(max_distance) > 1 && !out_is_preset) preset_out(out, (long)h * w * n_ids, st);
    launch_fused<LF_FUSED>(frame_plan(F, h, w, max_distance, LF_FUSED, n_ids, sizeof(float), 1), st, ap, bp, prev_labels, h, w, C,
                           n_ids, out, tab);
    manet_profile_record(st, false, 1);
    return manet_check_launch("manet_local_match_frames");
}

/* r6: the label-independent half of the local match, kept per frame pair (see local_fused_kernel's MODE).
 * manet_local_volume_bytes: bytes of one frame pair's normalised window-distance volume, stored as the per-workgroup LDS images
 * of the per-pixel phase (1.5x the bare (2d+1)^2 x h/2 x w/2 floats at d=12: tile aprons, 16-byte cell padding). */
int manet_local_volume_bytes(int h, int w, int max_distance, size_t *bytes) { return local_volume_bytes(h, w, max_distance, 4, bytes); }
/* The same volume with every normalised distance rounded once to IEEE half (to nearest even, subnormals kept; 1.0 stays 1.0): at
 * most half the fp32 bytes plus one 1 KiB piece. */
int manet_local_volume_bytes_f16(int h, int w, int max_distance, size_t *bytes) { return local_volume_bytes(h, w, max_distance, 2, bytes); }

/* phase 1 (IntVOS.py:266-296) of n_pairs frame pairs, ceil(n_pairs / 32) launches: pair i = (prev_frame_ws[i], cur_frame_ws[i]),
 * two prepared frames (manet_frame_prepare) -> volumes[i] (manet_local_volume_bytes each, 16-byte aligned).  The three tables are
 * HOST arrays of device pointers. */
int manet_local_volume_frames(const void *const *prev_frame_ws, const void *const *cur_frame_ws, float *const *volumes, int n_pairs,
                              int h, int w, int C, int compute, int max_distance, manet_stream_t stream)
{
    return local_volume_frames_t<float>("manet_local_volume_frames", prev_frame_ws, cur_frame_ws, (void *const *)volumes, n_pairs, h, w,
                                        C, compute, max_distance, stream);
}
/* ... into fp16 volumes (manet_local_volume_bytes_f16 each, 16-byte aligned): the same arithmetic up to and including the
 * normalisation in fp32, then one conversion to half. */
int manet_local_volume_frames_f16(const void *const *prev_frame_ws, const void *const *cur_frame_ws, void *const *volumes, int n_pairs,
                                  int h, int w, int C, int compute, int max_distance, manet_stream_t stream)
{
    return local_volume_frames_t<_Float16>("manet_local_volume_frames_f16", prev_frame_ws, cur_frame_ws, volumes, n_pairs, h, w, C,
                                           compute, max_distance, stream);
}

/* phase 2 (IntVOS.py:398-432) on a stored volume: bilinear taps + stride-2 label gather + masked minimum -> out [h][w][n_ids]; the
 * same bits as manet_local_match_frames on the pair the volume was made from.  cur_frame_ws: the current frame's prepared
 * workspace (its tile table). */
int manet_local_match_volume(const float *volume, const void *cur_frame_ws, const int32_t *prev_labels, int h, int w, int C,
                             int compute, int n_ids, int max_distance, float *out, int out_is_preset, manet_stream_t stream)
{
    return local_match_volume_t<float>("manet_local_match_volume", volume, cur_frame_ws, prev_labels, h, w, C, compute, n_ids,
                                       max_distance, out, out_is_preset, stream);
}
/* ... on an fp16 volume: the taps widened to fp32 (exact), then the same expression, label handling and out_is_preset protocol.
 * Against the fp32 route |out_f16 - out_f32| <= min(2^-12, 2^-11 out_f32); an entry that is 1.0 stays 1.0. */
int manet_local_match_volume_f16(const void *volume, const void *cur_frame_ws, const int32_t *prev_labels, int h, int w, int C,
                                 int compute, int n_ids, int max_distance, float *out, int out_is_preset, manet_stream_t stream)
{
    return local_match_volume_t<_Float16>("manet_local_match_volume_f16", (const _Float16 *)volume, cur_frame_ws, prev_labels, h, w,
                                          C, compute, n_ids, max_distance, out, out_is_preset, stream);
}

}  // extern "C"
