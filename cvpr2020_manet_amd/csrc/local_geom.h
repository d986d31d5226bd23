// Geometry, launch plan and host-side declarations of the local-window stage: csrc/local_fused.hip (the fused kernel and its two
// halves), csrc/local_match.hip (the unfused kernels of the reference formula) and csrc/local_train.hip (arg-min and backward).
// The padded pooled planes are shared with the per-frame prepare kernel (csrc/global_prepare.hip: manet_frame_prepare writes those
// planes and the tile table).  No kernel lives here: a host-only program that includes this header compiles in seconds
// (tests/test_local_plan.py).
#pragma once
#include "manet_common.h"
#include <type_traits>
#include <utility>

namespace {

// F.interpolate(..., mode='bilinear', align_corners=True) coefficients (IntVOS.py:295):
// scale = (in-1)/(out-1), src = scale*dst, i0 = floor, i1 = i0 + (i0 < in-1), l1 = src - i0.
struct Bilin {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Bilin bilin_coeff(int dst, int in_size, int out_size)
{
    float scale = (out_size > 1) ? (float)(in_size - 1) / (float)(out_size - 1) : 0.0f;
    float src = scale * (float)dst;
    int a = (int)src;
    if (a > in_size - 1) a = in_size - 1;
    Bilin b;
    b.i0 = a;
    b.i1 = a + ((a < in_size - 1) ? 1 : 0);
    b.l1 = src - (float)a;
    b.l0 = 1.0f - b.l1;
    return b;
}
__device__ __forceinline__ float bilin_sample(const float *__restrict__ pl, int wp, const Bilin &by,
                                              const Bilin &bx)
{
    return by.l0 * (bx.l0 * pl[by.i0 * wp + bx.i0] + bx.l1 * pl[by.i0 * wp + bx.i1]) +
           by.l1 * (bx.l0 * pl[by.i1 * wp + bx.i0] + bx.l1 * pl[by.i1 * wp + bx.i1]);
}
// smallest dst in [0, out_size] whose i0 is >= target (i0 is monotone in dst): an estimate from the inverse map,
// settled with the forward expression itself -- a couple of evaluations instead of a scan over the tile
__host__ __device__ __forceinline__ int bilin_first(int target, int in_size, int out_size)
{
    if (target <= 0) return 0;
    if (target > in_size - 1) return out_size;
    const float scale = (out_size > 1) ? (float)(in_size - 1) / (float)(out_size - 1) : 0.0f;  // as bilin_coeff
    if (scale == 0.0f) return out_size;
    // i0(dst) of bilin_coeff is min((int)(scale * dst), in_size - 1); target <= in_size - 1 here, so the clamp never
    // decides the comparison
    int y = (int)((float)target * (1.0f / scale));
    y = y < 0 ? 0 : (y > out_size ? out_size : y);
    while (y > 0 && (int)(scale * (float)(y - 1)) >= target) --y;
    while (y < out_size && (int)(scale * (float)y) < target) ++y;
    return y;
}

__host__ __device__ constexpr int lf_cols(int d) { return d <= 6 ? 2 : 4; }                       // columns per thread
// d = 3, 4 and d >= 10: a thread owns one HALF of the window columns (d=4: dx 0..3 | 4..8, d=12: 0..11 | 12..24): half
// the running sums, twice the threads -- two waves per SIMD for the arithmetic (a workgroup per CU is all the grid
// offers, so threads are the only source of latency hiding) and twice the lanes for the per-pixel phase
__host__ __device__ constexpr int lf_dxs(int d) { return (d == 3 || d == 4 || d >= 10) ? 2 : 1; }
// window columns of the first half: a multiple of the column group, so the second half's vector reads stay aligned
__host__ __device__ constexpr int lf_ph(int d) { return lf_cols(d) == 4 ? 12 : ((d + 1) & ~1); }
__host__ __device__ constexpr int lf_pa(int d)  // running sums per column per thread
{
    return lf_dxs(d) == 1 ? 2 * d + 1 : ((2 * d + 1 - lf_ph(d)) > lf_ph(d) ? (2 * d + 1 - lf_ph(d)) : lf_ph(d));
}
__host__ __device__ constexpr int lf_nt(int d) { return d <= 2 ? 256 : (d <= 6 ? 512 : (d <= 9 ? 256 : 512)); }  // threads
__host__ __device__ constexpr int lf_slots(int d) { return lf_nt(d) / ((16 / lf_cols(d)) * lf_dxs(d)); }  // (row, dy) slots
__host__ __device__ constexpr int lf_nd(int d) { return d <= 10 ? 2 * d + 1 : (d == 11 ? 12 : 5); }  // dy per workgroup
__host__ __device__ constexpr int lf_ndg(int d) { return (2 * d + 1 + lf_nd(d) - 1) / lf_nd(d); }
__host__ __device__ constexpr int lf_sy(int d) { return lf_slots(d) / lf_nd(d) > 12 ? 12 : lf_slots(d) / lf_nd(d); }
constexpr int LF_SX = 16;  // columns of S
__host__ __device__ constexpr int lf_cw(int d)  // halo row stride (every thread reads whole vectors: room for the over-read)
{
    // COLS = 4 halves: 40 columns are needed; 48 = 16 (mod 64 banks) makes the four (row, dy) slots of a b128 lane
    // group land on disjoint banks (r2 PMC at stride 40: SQ_LDS_BANK_CONFLICT = 40 % of SQ_LDS_IDX_ACTIVE; a
    // window read cost 10 LDS cycles instead of 4)
    return lf_cols(d) == 4 && lf_dxs(d) == 2 ? 48 : ((LF_SX + 2 * d + 3) & ~3);
}
__host__ __device__ constexpr int lf_yr(int d) { return lf_sy(d) + lf_nd(d) - 1; }                // halo rows
__host__ __device__ constexpr int lf_yplane(int d) { return lf_yr(d) * lf_cw(d); }
__host__ __device__ constexpr int lf_xplane(int d) { return lf_sy(d) * LF_SX; }
// channels per LDS stage: two stages <= 128 KiB (the phase-2 volume needs as much at the wide windows anyway)
__host__ __device__ constexpr int lf_cc(int d)
{
    int cc = 131072 / (8 * (lf_yplane(d) + lf_xplane(d)));
    return cc < 2 ? 2 : (cc > 25 ? 25 : cc);
}
// floats of one stage image, padded to whole 1 KiB LDS-DMA pieces
__host__ __device__ constexpr int lf_stage_floats(int d)
{
    return (lf_cc(d) * (lf_yplane(d) + lf_xplane(d)) / 4 + 63) / 64 * 256;
}
__host__ __device__ constexpr int lf_lab_rows(int d) { return 2 * (lf_sy(d) - 1) + 4 + 2 * (lf_nd(d) - 1); }
__host__ __device__ constexpr int lf_lab_cols(int d) { return 2 * (LF_SX - 1) + 4 + 4 * d; }
// phase 2 volume: [dy][cell of S][dx], dx contiguous, cell stride an ODD number of float4 -- a pixel's four taps are
// ds_read_b128 of 4 window columns each, and the 16 cells of a row of S land on 64 distinct banks
__host__ __device__ constexpr int lf_vs(int d) { return 4 * (((2 * d + 1 + 3) / 4) | 1); }
// pixels of a tile, upper bound -- rounded up to a multiple of the 64 LDS banks: the (id, pixel) slot a lane's atomic min goes to
// is id * lf_npix + pixel, a wave's lanes hold 64 CONSECUTIVE pixels, so whatever ids they carry they hit 64 distinct banks
// (r1-r5: 884 = 52 mod 64 -- lanes with different ids collided)
__host__ __device__ constexpr int lf_npix(int d) { return ((2 * (lf_sy(d) - 1) + 4) * (2 * (LF_SX - 1) + 4) + 63) / 64 * 64; }
constexpr int LF_NIP = 8;  // object ids per pass of the per-pixel phase
// LDS of the per-pixel phase: the volume of `rows` window rows (padded to whole 1 KiB LDS-DMA pieces), the label bytes around the tile
// for those rows, the per-(id, pixel) minima of `m2_rows` ids + the "no id" row, the bilinear tables, the label-change masks
__host__ __device__ constexpr int lf_lab_rows_of(int d, int rows) { return 2 * (lf_sy(d) - 1) + 4 + 2 * (rows - 1); }
// (es: bytes of a volume element -- 4, or 2 for the fp16 image of the stored volumes: the same [dy][cell][dx] order and cell stride
// lf_vs(d) in elements, so a cell is 8 bytes times an odd number, a tap a ds_read_b64, and the region half as large)
__host__ __device__ constexpr size_t lf_vpad_bytes(int d, int rows, size_t es = 4) { return ((size_t)rows * lf_sy(d) * LF_SX * lf_vs(d) * es + 1023) / 1024 * 1024; }
__host__ __device__ constexpr size_t lf_lds_phase2_bytes(int d, int rows, int m2_rows, size_t es = 4)
{
    return lf_vpad_bytes(d, rows, es) + (((size_t)lf_lab_rows_of(d, rows) * lf_lab_cols(d) + 15) & ~(size_t)15) +
           (size_t)lf_npix(d) * (m2_rows + 1) * 4 + (size_t)(2 * (lf_sy(d) - 1) + 4 + 2 * (LF_SX - 1) + 4) * 16 +
           (size_t)lf_lab_rows_of(d, rows) * 16;
}
// The per-pixel phase ON A STORED VOLUME (the kernel's LF_VOL_IN mode, r6) runs one workgroup per (tile, window-row group), as the fused
// kernel does.  Dealing a group's rows to several workgroups was measured slower at 480p, d = 12 (docs/history/r06_experiments.md): 5 rows
// per workgroup 21.1 us, 2 rows 23.8, 1 row 26-30 -- every workgroup pays the label fetch, the tables, the minima's initialisation and
// the closing atomics again.  The fp16 image keeps the thread count of the fp32 one (half the pieces per workgroup; the counted waits
// are derived from the piece count).
__host__ __device__ constexpr size_t lf_lds_vol_bytes(int d, int n_ids, size_t es = 4)
{
    return lf_lds_phase2_bytes(d, lf_nd(d), n_ids <= LF_NIP ? n_ids : LF_NIP, es);
}
__host__ __device__ constexpr size_t lf_lds_bytes(int d)
{
    size_t stage = 2 * (size_t)lf_stage_floats(d) * 4;
    size_t vol = lf_lds_phase2_bytes(d, lf_nd(d), LF_NIP);
    return stage > vol ? stage : vol;
}
// padded pooled plane [HPAD][WS]: image pixel (py, px) at (d + py, d + px)
struct PoolPad {
    int hp, wp, HPAD, WS;
    long plane;  // HPAD * WS
};
static PoolPad lf_pool_pad(int h, int w, int d)
{
    PoolPad G;
    G.hp = h / 2;
    G.wp = w / 2;
    G.HPAD = G.hp + lf_sy(d) + lf_ndg(d) * lf_nd(d) - 1;  // last tile row + halo rows of the last dy group
    G.WS = (G.wp + lf_cw(d) + 3) & ~3;                     // last tile column + halo columns
    G.plane = (long)G.HPAD * G.WS;
    return G;
}

// ---- the fused kernel's modes and what travels with them ----
// MODE (r6): the window distances depend on the two EMBEDDINGS only (IntVOS.py:266-296), the masked minimum (:398-432) on the
// previous frame's labels -- and a clip's embeddings never change between the interaction rounds of a session (test.py:137-154
// extracts them once per sequence).  LF_VOL_OUT: phase 1 alone, for a BATCH of frame pairs in one launch (blockIdx.y = pair): each
// workgroup's normalised volume image -- the exact LDS image phase 2 reads, [ND][SY * 16][VS] floats -- goes to memory.  LF_VOL_IN:
// phase 2 alone on such an image (one LDS-DMA stream instead of the channel stages): what the sequential chain runs from a
// clip's second round on.  LF_FUSED: both in one launch, the volume never in memory (r1-r5).  Same arithmetic, same bits.
constexpr int LF_FUSED = 0, LF_VOL_OUT = 1, LF_VOL_IN = 2;
constexpr int LF_BATCH = 32;  // frame pairs per LF_VOL_OUT launch (their pointers travel as a kernel argument)
struct LfBatch {
    const float *cur[LF_BATCH], *prev[LF_BATCH];
    float *vol[LF_BATCH];
};
// LF_VOL_IN: the tile table (first pixel row / column of every tile) computed on the HOST with the device's expression (fp32 IEEE
// operations, no contraction: the same integers) and handed over as a kernel argument -- a workgroup's label loads then depend on no
// memory round trip (under the volume stream the table read alone took 2.5 us, timeline in docs/history/r06_experiments.md)
constexpr int LF_TAB_MAX = 96;
struct LfTab {
    int n;  // entries (nty + 1 + ntx + 1), or 0: read the frame's table from memory
    int v[LF_TAB_MAX];
};
// floats of one workgroup's volume image in memory: the LDS image padded to whole 1 KiB LDS-DMA pieces
__host__ __device__ constexpr int lf_img_floats(int d) { return (lf_nd(d) * lf_sy(d) * LF_SX * lf_vs(d) + 255) / 256 * 256; }
// The fp16 image (VT = _Float16, the opt-in storage type of the stored volumes): the SAME [dy][cell of S][dx] order and the same cell
// stride lf_vs(d) counted in ELEMENTS -- 8 bytes times an odd number, a pixel's taps are ds_read_b64 of 4 window columns and the 16
// cells of a row of S land on 16 distinct bank pairs.  In memory the images lie back to back WITHOUT the padding to whole pieces
// (every image is a multiple of 128 bytes; the last piece of a workgroup's fetch reads into the next image, or into the 1 KiB
// behind the last one, and lands in the padding of the LDS region): exactly half the bytes of the fp32 images' payload.
template <typename VT>
__host__ __device__ constexpr int lf_img_elems(int d)
{
    return sizeof(VT) == 4 ? lf_img_floats(d) : lf_nd(d) * lf_sy(d) * LF_SX * lf_vs(d);
}

// ---- tile geometry of local_dist_kernel<D> (csrc/local_match.hip) as a function of the window radius d ----
constexpr int LD_TX = 16;  // columns per workgroup
// tile geometry as a function of the window radius d (all compile-time in the kernel):
__host__ __device__ constexpr int ld_ry(int d)  // grid rows per workgroup: 32 (row, dy) slots
{
    return (32 / (2 * d + 1)) < 1 ? 1 : ((32 / (2 * d + 1)) > 8 ? 8 : (32 / (2 * d + 1)));
}
__host__ __device__ constexpr int ld_cw(int d) { return (LD_TX + 2 * d + 3) & ~3; }  // halo row stride, 16 B rows
__host__ __device__ constexpr int ld_yplane(int d) { return (ld_ry(d) + 2 * d) * ld_cw(d); }
__host__ __device__ constexpr int ld_nj(int d) { return (ld_yplane(d) + 255) / 256; }  // halo elements per thread
// channels per LDS stage: as many as two stages fit in 64 KiB and ~80 staging registers allow -- a
// stage costs one global round trip + one barrier, so few, fat stages (4 at d=4, 13 at d=12 for C=100)
__host__ __device__ constexpr int ld_cc(int d)
{
    int by_lds = 65536 / (8 * (ld_yplane(d) + ld_ry(d) * LD_TX));
    int by_regs = 80 / (ld_nj(d) + 1);
    int cc = by_lds < by_regs ? by_lds : by_regs;
    return cc > 25 ? 25 : (cc < 4 ? 4 : cc);
}
struct DistLaunch {
    int RY;
    dim3 grid;
    size_t lds;
};
static DistLaunch dist_launch(int H, int W, int d)
{
    DistLaunch L;
    int ry = ld_ry(d);  // 256 threads = 32 (row, dy) slots x 8 column pairs
    L.RY = ry;
    L.grid = dim3((unsigned)((W + LD_TX - 1) / LD_TX), (unsigned)((H + ry - 1) / ry));
    L.lds = 2 * (size_t)ld_cc(d) * ((size_t)ld_yplane(d) + (size_t)ry * LD_TX) * sizeof(float);  // 2 stages
    return L;
}

// ---- the launch plan of local_fused[_f16]_kernel<D, MODE>: every figure of a launch, of the pooling pass in front of it and of
// the stored volumes, computed once; the launcher, the entry points and tests/test_local_plan.py all read this ----
struct LfPlan {
    int d;
    PoolPad G;             // the padded pooled planes the kernel stages from
    int TY, TX, ntx, nty, rw, rh;  // pooled rows / columns of a tile (S without its apron); tiles; tiles per XCD region (4 x 2 regions)
    unsigned grid_x, grid_y;
    int nt;                // threads
    size_t lds, lds_attr;  // dynamic LDS of this launch, and the kernel's attribute (what the largest n_ids needs)
    long images;           // workgroups (= volume images) of one frame pair
    int img_elems;         // elements of one image in memory: the kernel's `vimg` stride
    LfTab tab;             // LF_VOL_IN: the tile table as a kernel argument; n = 0 in the other modes, or when it does not fit
};
static LfPlan lf_plan(int h, int w, int d, int mode, int n_ids, size_t elem_bytes, int n_pairs)
{
    LfPlan P;
    P.d = d; P.G = lf_pool_pad(h, w, d);
    P.TY = lf_sy(d) - 1; P.TX = LF_SX - 1;
    // i0 runs over 0..hp-1 (the last value only for the last row); tiles cover all of them
    P.ntx = (P.G.wp + P.TX - 1) / P.TX; P.nty = (P.G.hp + P.TY - 1) / P.TY;
    P.rw = (P.ntx + 3) / 4; P.rh = (P.nty + 1) / 2;
    P.grid_x = (unsigned)(8 * P.rw * P.rh * lf_ndg(d)); P.grid_y = (unsigned)(mode == LF_VOL_OUT ? n_pairs : 1);
    P.nt = lf_nt(d);
    P.lds = mode == LF_VOL_IN ? lf_lds_vol_bytes(d, n_ids, elem_bytes) : lf_lds_bytes(d);
    P.lds_attr = mode == LF_VOL_IN ? lf_lds_vol_bytes(d, LF_NIP, elem_bytes) : P.lds;
    P.images = (long)P.ntx * P.nty * lf_ndg(d);
    P.img_elems = elem_bytes == 4 ? lf_img_elems<float>(d) : lf_img_elems<_Float16>(d);
    P.tab.n = 0;
    if (mode == LF_VOL_IN && P.nty + 1 + P.ntx + 1 <= LF_TAB_MAX) {  // the device's expression on the host: the same integers (lf_pool_pad_kernel / frame prepare)
        P.tab.n = P.nty + 1 + P.ntx + 1;
        for (int i = 0; i <= P.nty; ++i) P.tab.v[i] = bilin_first(i * P.TY, P.G.hp, h);
        for (int i = 0; i <= P.ntx; ++i) P.tab.v[P.nty + 1 + i] = bilin_first(i * P.TX, P.G.wp, w);
    }
    return P;
}
// bytes of one frame pair's stored volume (+ 1 KiB: the per-pixel kernel fetches whole 1 KiB pieces, past the last image's end)
static size_t lf_volume_bytes(int h, int w, int d, size_t elem_bytes)
{
    const LfPlan P = lf_plan(h, w, d, LF_VOL_OUT, 1, elem_bytes, 1);
    return (size_t)P.images * P.img_elems * elem_bytes + 1024;
}
// the planes of a prepared frame (manet_frame_prepare) are lf_pool_pad's
static PoolPad pool_pad_of(const ManetFrameLayout &F) { return PoolPad{F.hp, F.wp, F.HPAD, F.WS, F.PS}; }

// f(std::integral_constant<int, D>{}) for the window radius d = D in 0..MANET_MAX_LOCAL_DISTANCE: the one place a runtime radius
// becomes a kernel's template argument (check_local() rejected every other value already)
template <class F, int... D>
void for_window_in(int d, F &&f, std::integer_sequence<int, D...>)
{
    (void)((d == D && (f(std::integral_constant<int, D>{}), true)) || ...);
}
template <class F>
void for_window(int d, F &&f) { for_window_in(d, f, std::make_integer_sequence<int, MANET_MAX_LOCAL_DISTANCE + 1>{}); }

// ---- workspaces and argument checks of the entry points ----
struct LocalLayout {
    int hp, wp, PP;
    size_t off_ap, off_bp, off_vol, total;
};
LocalLayout local_layout(int h, int w, int C, int d, int downsample)
{
    LocalLayout L;
    L.PP = (2 * d + 1) * (2 * d + 1);
    L.hp = downsample ? h / 2 : h;
    L.wp = downsample ? w / 2 : w;
    size_t plane = (size_t)L.hp * L.wp;
    // pooled frames: the padded planes of the fused path (the unpadded ones of the other paths fit inside)
    size_t pooled = downsample ? (size_t)lf_pool_pad(h, w, d).plane * C * sizeof(float) : 0;
    L.off_ap = 0;
    L.off_bp = manet_align_up(pooled, 256);
    L.off_vol = L.off_bp + manet_align_up(pooled, 256);
    // the volume region doubles as the fused path's tile table (first pixel row / column of every tile)
    size_t vol = plane * L.PP * sizeof(float), tab = (size_t)(L.hp + L.wp + 4) * sizeof(int);
    L.total = manet_align_up(L.off_vol + (vol > tab ? vol : tab), 256);
    return L;
}

int check_local(int h, int w, int C, int d, int downsample)
{
    if (h <= 0 || w <= 0 || C <= 0) return manet_set_error(MANET_E_INVALID, "h=%d w=%d C=%d", h, w, C);
    if (d < 0 || d > MANET_MAX_LOCAL_DISTANCE)
        return manet_set_error(MANET_E_INVALID, "max_distance=%d (supported 0..%d)", d, MANET_MAX_LOCAL_DISTANCE);
    if (downsample && (h < 2 || w < 2)) return manet_set_error(MANET_E_INVALID, "downsample needs h,w >= 2");
    return MANET_OK;
}
int check_ids(int n_ids)
{
    if (n_ids <= 0 || n_ids > MANET_MAX_IDS)
        return manet_set_error(MANET_E_INVALID, "n_ids=%d (supported 1..%d)", n_ids, MANET_MAX_IDS);
    return MANET_OK;
}
// manet_local_match_backward_f32: four pooled frames (both inputs, both gradients), then the volume's gradient
static size_t local_bwd_ws_bytes(int h, int w, int C, int d)
{
    size_t plane = (size_t)(h / 2) * (w / 2), PP = (size_t)(2 * d + 1) * (2 * d + 1);
    return manet_align_up(4 * plane * C * sizeof(float), 256) + manet_align_up(plane * PP * sizeof(float), 256);
}

}  // namespace

// Host functions one local file offers the others (every kernel is emitted by exactly one file).  csrc/local_match.hip:
// local_dist_kernel<d>; and pool2x2_kernel of both frames into ap / bp [C][hp][wp], then -- vol != nullptr -- their normalised volume
void manet_local_launch_dist(int d, hipStream_t st, const float *x, long x_sy, long x_sx, long x_sc, const float *y, long y_sy,
                             long y_sx, long y_sc, int H, int W, int C, int pooled_out, float *out);
void manet_local_pooled_volume(const float *cur, long c_sy, long c_sx, long c_sc, const float *prev, long p_sy, long p_sx, long p_sc,
                               int C, int hp, int wp, int d, float *ap, float *bp, float *vol, hipStream_t st);
// csrc/local_fused.hip: the pooling pass + the fused kernel (`pooled`: room for the two padded pooled frames, 2 * C *
// lf_pool_pad().plane floats; `tab`: the tile table); and fill_f32_kernel with zeros in at most 2048 blocks (the backwards)
void manet_local_launch_fused(int d, hipStream_t st, const void *cur, long c_sy, long c_sx, long c_sc, const void *prev, long p_sy,
                              long p_sx, long p_sc, int emb_dtype, const int *labels, int h, int w, int C, int n_ids, float *out,
                              float *pooled, int *tab);
void manet_local_fill_zero(float *p, long n, hipStream_t st);
