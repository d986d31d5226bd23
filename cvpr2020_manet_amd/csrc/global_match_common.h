// Global nearest-neighbour matching: what csrc/global_prepare.hip (makes the operands), csrc/global_match.hip (the match) and
// csrc/global_refine.hip (the bf16-filter + fp32-re-rank mode) share.  Host functions, constexpr and __device__ __forceinline__
// helpers only, no kernel: tile constants, the operand image (Geom), the workspace layouts (their totals are ABI), the launch
// plan (MatchPlan; tests/test_match_plan.py pins it on the CPU) and the prototypes of the host functions that cross files.
#pragma once
#include "manet_common.h"
#include <type_traits>

namespace {

constexpr int QT = 256;       // queries per workgroup (4 waves x 2 blocks of 32)
constexpr int QB = 32;        // queries per packed block (one MFMA N dimension)
constexpr int BT = 64;        // bank rows per tile (2 MFMA M blocks)
constexpr int META_INTS = 256;
constexpr int META_T = 0;          // [0]        number of bank tiles actually used
constexpr int META_SEG = 1;        // [1..65]    first tile of object o (entry n_ids = T)
constexpr int META_CNT = 130;      // [130..193] rows per object
constexpr int META_KMAX = 200;     // [200]      max |k|^2 over the bank's rows, float bits (MANET_COMPUTE_BF16_REFINE)
// MANET_COMPUTE_F16_REFINE, from the bank's fp16 image itself (f16_domain_kernel, csrc/global_prepare.hip):
constexpr int META_F16_KMAX = 201;  // [201]     max |k~|^2 over the rows INSIDE fp16's domain, float bits
constexpr int META_F16_SUBN = 202;  // [202]     max over those rows of the number of elements that are nonzero fp16 subnormals
constexpr int META_F16_OOD = 203;   // [203]     != 0: an object without a NaN row holds a row outside fp16's domain
// MANET_COMPUTE_BF16_REFINE: a pre-pass over every REFINE_SUB-th bank tile gives an upper bound of the minimum; the full
// bf16 pass then keeps, per (query, object), the bank rows that could beat it; up to REFINE_CAP of them are re-evaluated in
// the reference's fp32 arithmetic
// REFINE_SUB by bank size (refine_sub): the pre-pass costs 1 / REFINE_SUB of the filter pass's matrix work; a sparser sample
// leaves ~ln more candidates per pair for the cheap re-rank -- the larger the bank, the sparser the sample that pays.
constexpr int META_NAN = 66;       // [66..129]  object o's bank rows contain a NaN (MANET_COMPUTE_BF16_REFINE)
int refine_sub(long T_max) { return T_max <= 2500 ? 8 : 16; }  // 480p x 5 frames: 2 007 tiles; 720p x 10 frames: 9 006
constexpr int REFINE_XCHG_MASK = 3;  // threshold exchange every (mask + 1) steps
constexpr int REFINE_CAP = 128;  // capacity of a candidate bucket (one per 32-query block), in rows per (query, object) pair ON AVERAGE
constexpr int REFINE_LDS_LIST = 2048;  // candidate entries a filter workgroup collects in LDS before it appends them in bulk
// A 32-query x 32-row block with more qualifying distances than a sub-list holds is listed as ONE "dense" entry {block's
// first pair, 0x80000000 | first bank slot of the pass}: the re-rank evaluates all of its 1 024 distances exactly.  At most
// REFINE_DENSE_CAP of them per 32-query bucket (counted in bcnt's second half); one more marks the bucket incomplete and
// the rescue pass (the exact fp32 kernel on the 256-query tile) takes over.  A dense entry is one 32 x 32 x C tile on the fp32
// matrix pipe for ONE wave (1.4 us at C = 100, operands from global memory / LDS per entry): 1 024 of them in every bucket of a
// 480p frame are ~1.1 ms of the chip, a quarter of the fp32 kernel -- beyond that the fp32 kernel's operand reuse wins.
constexpr int REFINE_DENSE_CAP = 1024;
constexpr unsigned REFINE_DENSE_BIT = 0x80000000u;
// ... and a block is listed whole as soon as more than REFINE_DENSE_MIN of its 1 024 distances qualify: a listed row costs the
// re-rank a 400-byte gather of its bank row (C = 100) per (query, row) pair, a dense entry 12.8 KB of rows per 1 024 pairs and
// 1.4 us of one wave's matrix pipe (more when the wave has nothing else to hide the row loads behind).  Measured on one box,
// ms per step on video-like / smooth embeddings at cfg2 size for (REFINE_DENSE_MIN, REFINE_DENSE_LANES): (128, off) 0.798 /
// 0.963, (64, 24) 0.799 / 0.866, (64, 16) 0.803 / 0.856, (32, 16) 0.806 / 0.858, (32, 8) 0.813 / 0.854.
constexpr int REFINE_DENSE_MIN = 64;
constexpr int REFINE_DENSE_LANES = 16;  // (64: off; smooth embeddings at cfg2 size: filter 0.66 -> 0.56 ms)
constexpr int REFINE_RZ = 4;  // workgroups of the re-rank launch per bucket: each takes every 4th entry (the longest bucket is the launch's time)
constexpr int ONE_ROUND_OK = 1 << 29;   // block_map flag (fp32 pipe kernel): the device may swap the host's splits for ONE round of long ones
constexpr int RESCUE_LISTED = 1 << 30;  // block_map flag of the rescue launch: deal the workgroups to the LISTED tiles
// block_map word: bits 0-7 tuning, bits 8-20 small_S (<= 4096: 13 bits) -- or, in the rescue launch, bits 8-28 its split count --
// bit 29 ONE_ROUND_OK, bit 30 RESCUE_LISTED.  (the rescue field was masked with 22 bits and reached bit 29.)
constexpr int BLOCK_MAP_SMALL_S_MASK = 0x1fff, BLOCK_MAP_RESCUE_MASK = 0x1fffff;
static_assert(((BLOCK_MAP_RESCUE_MASK << 8) & (ONE_ROUND_OK | RESCUE_LISTED)) == 0 && ((BLOCK_MAP_SMALL_S_MASK << 8) & (ONE_ROUND_OK | RESCUE_LISTED)) == 0 &&
              4096 <= BLOCK_MAP_SMALL_S_MASK, "block_map fields overlap");

constexpr int FILTER_TAIL_CUTS = 4;  // pieces each XCD's last split of the filter launch is cut into (tapered_split_of_block; 1: bm == 3's map)

// Packed operand image of one row block: `units` 16-byte units per row, stored [unit][row][16 B].
//   f32    unit u = 2g+h holds k = 8g + 2j + h, j = 0..3 (4 floats)      -> v_mfma_f32_32x32x2_f32
//          followed by the rows' squared norms (fp32)
//   bf16   unit u = 2s+h holds k = 16s + 8h + e, e = 0..7 (8 bf16)        -> v_mfma_f32_32x32x16_bf16
//          no norm block: the norms ride in the spare k slots C..C+5 of the image itself (below)
//   bf16x3 the bf16 image of hi = bf16(x), then the image of lo = bf16(x - hi)
//
// bf16 images: d(n,m) = |q|^2 + |k|^2 - 2 q.k comes out of the MFMA chain itself, accumulator
// starting at 0, no per-element epilogue arithmetic:
//   query rows hold  -2*bf16(q)  (exact: a power of two)          bank rows hold  bf16(k)
//   query k = C+0..2 : 1, 1, 1                                      bank k = C+0..2 : |k|^2 as hi+mid+lo
//   query k = C+3..5 : |q|^2 as hi+mid+lo (three bf16 = 24 bits)    bank k = C+3..5 : 1, 1, 1
// (three bf16 pieces carry an fp32 value exactly; the products with 1 are exact, the sum is fp32.)
//
// f16 images (MANET_COMPUTE_F16, v_mfma_f32_32x32x16_f16): the bf16 image's layout with fp16 elements -- -2*f16(q) / f16(k) --
// and the same six norm slots.  fp16 has a narrow exponent range, so the norm's three pieces are SCALED by powers of two and
// meet the inverse power on the other side (products of a power of two: exact):
//   side that carries its norm: p0, p1 * 2^11, p2 * 2^14        other side: 1, 2^-11, 2^-14
// Every stored piece is zero or a NORMAL fp16 number (split3_f16), whether or not the matrix pipe honours subnormal operands:
// p0 + p1 + p2 == norm exactly for norms >= 2^-5, within 2^-28 below (asked for: exact from 2^-6, within 2^-25 below -- but the
// last bit of a norm in [2^-6, 2^-5), 2^-29, times the largest scale whose partner 2^-14 is still normal is subnormal: dropped).
// A row outside fp16's domain (|row|^2 of the rounded values > 65504, an infinity, a NaN) carries NaN in its first norm slot: all of its distances are NaN.  A bank tile's padding rows carry
// +inf there (fp16 has no 1e20): their distances are +inf and never win a minimum.
constexpr int BF16_SPECIAL = 6;  // spare k slots needed behind the C channels
__host__ __device__ constexpr size_t bank_tile_bytes_u(int units, bool norms)
{
    return ((size_t)units * BT * 16 + (norms ? BT * 4 : 0) + 1023) / 1024 * 1024;  // whole 1 KiB LDS-DMA pieces
}
__host__ __device__ constexpr size_t query_block_bytes_u(int units, bool norms)
{
    return (size_t)units * QB * 16 + (norms ? QB * 4 : 0);
}
__host__ __device__ constexpr size_t bank_tile_bytes(int NG) { return bank_tile_bytes_u(2 * NG, true); }
__host__ __device__ constexpr size_t query_block_bytes(int NG) { return query_block_bytes_u(2 * NG, true); }

// number of v_mfma_f32_32x32x2 k-steps (2 k each) the f32 kernel is instantiated for
int pick_ks(int C)
{
    if (C <= 32) return 16;
    if (C <= 100) return 50;   // the reference's embedding width: 50 MFMAs, not 52
    if (C <= 104) return 52;
    return 64;
}
// number of v_mfma_f32_32x32x16_bf16 k-steps (16 k each) the bf16 kernels are instantiated for:
// C channels + BF16_SPECIAL norm slots
int pick_ksb(int C)
{
    if (C + BF16_SPECIAL <= 32) return 2;
    if (C + BF16_SPECIAL <= 112) return 7;   // C = 100: 7 MFMAs per 32x32 block
    return 9;
}
constexpr int QT_BF16 = 512;  // queries per workgroup of the bf16 kernels (8 waves x 64)

}  // namespace

// (plain structs outside the anonymous namespace: they appear in the prototypes that cross files, at the end)
struct Geom {
    int compute;
    int steps;   // MFMA k-steps of the instantiation
    int units;   // 16-byte units per row of the packed image
    int kpad;    // k extent covered by the image
    int qt;      // queries per workgroup
    size_t tile_bytes, qblk_bytes;
};

struct BankLayout {
    Geom G;
    size_t tile_bytes;
    long T_max;  // upper bound on tiles: every object wastes < 1 tile
    long nblocks;  // pre-pass blocks of RPB rows
    size_t off_meta, off_hist, off_src, off_pack, total;
    // MANET_COMPUTE_BF16_REFINE / _F16_REFINE only: the sorted rows once more in fp32, row-major [T_max * 64][C] + their |k|^2 (what the
    // exact re-rank reads), and the sub-sampled bank of the pre-pass (its own meta block + every REFINE_SUB-th tile)
    long T_sub_max;
    size_t off_rows, off_norms, off_sub_meta, off_sub_pack;
    Geom G32;  // ... and its fp32 operand image (the rescue pass of incomplete candidate buckets: the exact fp32 kernel)
    size_t off_pack32;
};

struct MatchLayout {
    Geom G;
    long N_pad;
    int nQT;
    size_t qblk_bytes, off_q, off_keys, off_topk, total;
    // MANET_COMPUTE_BF16_REFINE: per (object, query) threshold and exact-distance key, the flat candidate list
    // {pair, bank slot} with its capacity, and two counters (candidates appended, list overflowed)
    size_t off_thr, off_slack, off_keys2, off_list, off_stats, off_bcnt, off_q32;
    long list_cap, bucket_cap;  // the candidate list = N_pad / 32 buckets (one per 32-query block) of bucket_cap entries
};

// How one launch of a main kernel is cut: grid = query tiles x S bank splits, the `block_map` word (split_of_block,
// csrc/global_match.hip), dynamic LDS.  match_plan() alone decides it, from the shape, the launch's form and the tune values;
// launch_match() (csrc/global_match.hip) picks the kernel from the same form.
enum MatchForm {
    MATCH_FORM_MAIN = 0,             // manet_global_match_prepared_ex: fp32 pipe / general fp32 (k_nn > 1) / bf16 wide, pipe, x3
    MATCH_FORM_ARG,                  // the arg-min form of the general fp32 kernel
    MATCH_FORM_NTH_ARG,              // ... and its bounded form (pass j of the k nearest rows): the same plan
    MATCH_FORM_REFINE_PRE,           // MANET_COMPUTE_BF16_REFINE / _F16_REFINE: the pre-pass over the sub-sampled bank (bf16 / fp16 wide),
    MATCH_FORM_REFINE_FILTER,        // ... the filter pass (the wide body's FILTER form; spread / tapered map),
    MATCH_FORM_REFINE_RESCUE,        // ... the rescue of the listed query tiles (fp32 pipe, RESCUE)
    MATCH_FORM_REFINE_RESCUE_EXACT,  // ... or of every tile (MANET_EPI_REFINE_EXACT)
};
struct MatchTune {  // MANET_TUNE_SPLITS, MANET_TUNE_BLOCK_MAP, MANET_TUNE_ONE_ROUND; unset = {0, -1, 0}
    int splits, block_map, one_round;
};
struct MatchPlan {
    int form, compute, k_nn;
    int steps;   // MFMA k-steps of the kernel's instantiation (pick_ks / pick_ksb)
    int nQT;     // query tiles (the rescue launch: 256-query tiles of the bf16 layout's padded rows)
    long T_max;  // upper bound of the bank tiles the splits are sized for (the pre-pass: of the sub-sampled bank)
    int S;       // bank splits
    int slots;   // resident workgroup slots the splits are sized for: 512 = two workgroups per CU, 256 = one
    int block_map;
    size_t lds;  // dynamic LDS bytes
    unsigned grid;
};
struct MatchArgs {  // the main kernels' arguments next to the plan's; from `thr` on: the FILTER and RESCUE forms'
    const char *qpack, *bpack;
    const int *meta;
    int n_ids;
    long N_pad;
    unsigned *keys;
    float *topk;
    unsigned *thr;
    const float *slack;
    unsigned long long *stats;
    uint2 *list;
    long bucket_cap;
    unsigned *bcnt;
};

namespace {

// the two filter + exact fp32 re-rank modes: one set of layouts, plans and limits (the images are the same size)
constexpr bool is_refine(int compute) { return compute == MANET_COMPUTE_BF16_REFINE || compute == MANET_COMPUTE_F16_REFINE; }

Geom geom_of(int C, int compute)
{
    Geom G;
    if (compute == MANET_COMPUTE_BF16_REFINE) compute = MANET_COMPUTE_BF16;  // same operand images as plain bf16
    if (compute == MANET_COMPUTE_F16_REFINE) compute = MANET_COMPUTE_F16;    // ... and as plain fp16
    G.compute = compute;  // (MANET_COMPUTE_F16 stays: the bf16 image's geometry, fp16 elements)
    if (compute == MANET_COMPUTE_F32) {
        G.steps = pick_ks(C);
        int NG = (G.steps + 3) / 4;
        G.units = 2 * NG;
        G.kpad = 8 * NG;
        G.qt = QT;
    } else {
        G.steps = pick_ksb(C);
        G.units = 2 * G.steps * (compute == MANET_COMPUTE_BF16X3 ? 2 : 1);
        G.kpad = 16 * G.steps;
        // 8 waves: the bf16 MFMA eats a bank tile 14x faster, so share it between more queries
        G.qt = QT_BF16;
    }
    const bool norms = (compute == MANET_COMPUTE_F32);
    G.tile_bytes = bank_tile_bytes_u(G.units, norms);
    G.qblk_bytes = query_block_bytes_u(G.units, norms);
    return G;
}

BankLayout bank_layout(int64_t M0, int C, int n_ids, int compute)
{
    BankLayout L;
    L.G = geom_of(C, compute);
    L.tile_bytes = L.G.tile_bytes;
    L.T_max = (long)((M0 + BT - 1) / BT) + n_ids;
    L.nblocks = (long)((M0 + 255) / 256);
    L.off_meta = 0;
    L.off_hist = manet_align_up(META_INTS * sizeof(int), 256);
    L.off_src = manet_align_up(L.off_hist + (size_t)(L.nblocks > 0 ? L.nblocks : 1) * n_ids * sizeof(int), 256);
    L.off_pack = manet_align_up(L.off_src + (size_t)L.T_max * BT * sizeof(int), 1024);
    L.total = manet_align_up(L.off_pack + (size_t)L.T_max * L.tile_bytes, 1024);
    L.T_sub_max = 0;
    L.off_rows = L.off_norms = L.off_sub_meta = L.off_sub_pack = L.off_pack32 = 0;
    L.G32 = L.G;
    if (is_refine(compute)) {
        L.T_sub_max = L.T_max / refine_sub(L.T_max) + n_ids + 1;
        L.off_rows = L.total;
        L.off_norms = manet_align_up(L.off_rows + (size_t)L.T_max * BT * C * sizeof(float), 256);
        L.off_sub_meta = manet_align_up(L.off_norms + (size_t)L.T_max * BT * sizeof(float), 256);
        L.off_sub_pack = manet_align_up(L.off_sub_meta + META_INTS * sizeof(int), 1024);
        L.G32 = geom_of(C, MANET_COMPUTE_F32);
        L.off_pack32 = manet_align_up(L.off_sub_pack + (size_t)L.T_sub_max * L.tile_bytes, 1024);
        L.total = manet_align_up(L.off_pack32 + (size_t)L.T_max * L.G32.tile_bytes, 1024);
    }
    return L;
}

constexpr int TOPK_SPLITS = 16;  // the top-k path trades a little tail balance for a bounded workspace

MatchLayout match_layout(int64_t N, int C, int n_ids, int compute, int k_nn = 1, bool arg = false)
{
    MatchLayout L;
    L.G = geom_of(C, compute);
    L.nQT = (int)((N + L.G.qt - 1) / L.G.qt);
    L.N_pad = (long)L.nQT * L.G.qt;
    L.qblk_bytes = L.G.qblk_bytes;
    L.off_q = 0;
    L.off_keys = manet_align_up((size_t)(L.N_pad / QB) * L.qblk_bytes, 256);
    L.off_topk = manet_align_up(L.off_keys + (size_t)n_ids * L.N_pad * sizeof(unsigned), 1024);
    L.total = L.off_topk;
    if (k_nn > 1)
        L.total = manet_align_up(L.off_topk + (size_t)TOPK_SPLITS * n_ids * L.N_pad * MANET_MAX_KNN * sizeof(float), 1024);
    if (arg)  // 64-bit (distance key, bank slot) pairs of the arg-min form live where the top-k lists would
        L.total = manet_align_up(L.off_topk + (size_t)n_ids * L.N_pad * sizeof(unsigned long long), 1024);
    L.off_thr = L.off_slack = L.off_keys2 = L.off_list = L.off_stats = L.off_bcnt = L.off_q32 = 0;
    L.list_cap = L.bucket_cap = 0;
    if (is_refine(compute)) {
        const size_t pairs = (size_t)n_ids * L.N_pad;
        L.list_cap = (long)pairs * REFINE_CAP;
        L.off_thr = L.off_topk;
        L.off_slack = manet_align_up(L.off_thr + pairs * sizeof(float), 256);
        L.off_keys2 = manet_align_up(L.off_slack + pairs * sizeof(float), 256);
        L.off_list = manet_align_up(L.off_keys2 + pairs * sizeof(unsigned), 256);
        L.bucket_cap = (long)n_ids * QB * REFINE_CAP;
        L.off_stats = manet_align_up(L.off_list + (size_t)L.list_cap * sizeof(uint2), 256);
        L.off_bcnt = L.off_stats + 256;
        // (bcnt: [N_pad / 32] entries appended | bit 31 incomplete, then [N_pad / 32] dense entries appended)
        // then {number of 256-query tiles to rescue, their ids} (written by the re-rank launch, read by the rescue launch)
        L.off_q32 = manet_align_up(L.off_bcnt + ((size_t)2 * (L.N_pad / QB) + 1 + (size_t)(L.N_pad / QT)) * sizeof(unsigned), 1024);  // fp32 query image (rescue)
        L.total = manet_align_up(L.off_q32 + (size_t)(L.N_pad / QB) * geom_of(C, MANET_COMPUTE_F32).qblk_bytes, 1024);
    }
    return L;
}

// Number of bank splits S (grid = query tiles x S).  Every split re-reads the query operand
// (S x 4C.N bytes of fabric traffic, the bank itself streams through each XCD's L2 once), so S
// should be as small as the tail allows: take the smallest multiple of 8 whose last round of
// workgroups over the `slots` resident workgroup slots is >= 97 % full, with >= 4 tiles per split.
int pick_splits(int nQT, long T_max, int slots)
{
    // Workgroups are dispatched as slots free up; what a split count costs is its last, partial round.  With two
    // workgroups per CU (slots = 512) a last round that fills at most half the slots leaves its workgroups alone on
    // their CUs, where they run about twice as fast: it costs half a round (r2 sweep at cfg2, S = 40 / 48 / 56 / 64 / 80:
    // 4.704 / 4.672 / 4.836 / 4.778 / 4.714 ms -- 48 leaves 0.47 of a round, 40 leaves 0.89).  Every workgroup also
    // pays a fixed prologue (query operand, first tile), a share that grows with S.
    long cap = T_max / 4 / 8 * 8;
    if (cap < 8) cap = 8;
    if (cap > 256) cap = 256;
    const bool two_per_cu = slots >= 512;
    int best = 8;
    double best_eff = 0.0;
    for (int S = 8; S <= cap; S += 8) {
        const double rounds = (double)nQT * S / slots;
        const double whole = (double)(long)rounds, frac = rounds - whole;
        const double last = frac <= 0.0 ? 0.0 : ((two_per_cu && frac <= 0.5) ? 0.5 : 1.0);
        const double eff = rounds / (whole + last) / (1.0 + 0.0003 * S);
        if (eff > best_eff) {
            best_eff = eff;
            best = S;
        }
    }
    return best;
}

int check_common(int64_t N, int64_t M0, int C, int n_ids, int k_nn, int compute)
{
    if (N <= 0 || M0 < 0) return manet_set_error(MANET_E_INVALID, "N=%lld M0=%lld", (long long)N, (long long)M0);
    if (M0 >= (1LL << 31) - 64 * (MANET_MAX_IDS + 1) || N >= (1LL << 31) - QT)
        return manet_set_error(MANET_E_INVALID, "N or M0 too large for 32-bit row indices");
    if (C <= 0 || C > MANET_MAX_C) return manet_set_error(MANET_E_INVALID, "C=%d (supported 1..%d)", C, MANET_MAX_C);
    if (n_ids <= 0 || n_ids > MANET_MAX_IDS)
        return manet_set_error(MANET_E_INVALID, "n_ids=%d (supported 1..%d)", n_ids, MANET_MAX_IDS);
    if (k_nn < 1 || k_nn > MANET_MAX_KNN)
        return manet_set_error(MANET_E_INVALID, "k_nn=%d (supported 1..%d)", k_nn, MANET_MAX_KNN);
    if (k_nn > 1 && compute != MANET_COMPUTE_F32)
        return manet_set_error(MANET_E_INVALID, "k_nn > 1 needs MANET_COMPUTE_F32");
    if (compute != MANET_COMPUTE_F32 && compute != MANET_COMPUTE_BF16 && compute != MANET_COMPUTE_BF16X3 &&
        compute != MANET_COMPUTE_BF16_REFINE && compute != MANET_COMPUTE_F16 && compute != MANET_COMPUTE_F16_REFINE)
        return manet_set_error(MANET_E_INVALID, "compute=%d (MANET_COMPUTE_F32 / _BF16 / _BF16X3 / _BF16_REFINE / _F16 / _F16_REFINE)",
                               compute);
    if (compute == MANET_COMPUTE_BF16_REFINE && C + BF16_SPECIAL > 112)
        return manet_set_error(MANET_E_INVALID, "MANET_COMPUTE_BF16_REFINE supports C <= 106 (the wide bf16 kernel)");
    if (compute == MANET_COMPUTE_F16_REFINE && C + BF16_SPECIAL > 112)
        return manet_set_error(MANET_E_INVALID, "MANET_COMPUTE_F16_REFINE supports C <= 106 (the wide fp16 kernel)");
    return MANET_OK;
}

// the kernels' `block_map` argument: mapping bits + small_S (see split_of_block).
// Mapping (r3b): XCD-aware with PB splits fastest, PB = how many of this bank's splits fit an XCD's L2 side by side
// (<= 3; 2.4 MB of the 4 MB: the query operands in flight want the rest).  The workgroups of an XCD that are resident
// together then cover 64 / PB query tiles x PB splits instead of 64 x 1, a query operand is fetched over the fabric once
// per PB workgroups, and the splits still stream through the L2 once.  Measured (FETCH_SIZE x 2, kernel time unchanged
// within 0.3 %): cfg2 fp32 692 -> 420 MB per launch (PB = 2; PB = 3: 538), cfg3 bf16 277 -> 142 MB (PB = 3; 4: 168),
// cfg5 bf16 1.26 GB at PB = 1, which its 1.6 MB splits keep (PB = 3: 1.64 GB).
// bank_bytes = packed bytes of the bank the launch streams; tune_block_map = MANET_TUNE_BLOCK_MAP's value (< 0: unset).
// S = 0 (the filter launch, which sets the map bits itself): no automatic map, whatever the bank's size.
int block_map_arg(int nQT, int slots, int S, double bank_bytes, int tune_block_map)
{
    int small_S = slots / (nQT > 0 ? nQT : 1);
    if (small_S < 1) small_S = 1;
    if (small_S > 4096) small_S = 4096;
    int bm = tune_block_map;
    if (bm < 0) {
        bm = 0;
        if (S >= 16 && (S & 7) == 0 && bank_bytes > 0.0) {
            int pb = (int)(2.4e6 / (bank_bytes / S));
            pb = pb > 3 ? 3 : pb;
            if (pb > S / 8) pb = S / 8;
            if (pb >= 2) bm = pb + 2;
        }
    }
    return (bm & 0xff) | (small_S << 8);
}

MatchTune match_tune()
{
    return {manet_tune_get(MANET_TUNE_SPLITS, 0), manet_tune_get(MANET_TUNE_BLOCK_MAP, -1), manet_tune_get(MANET_TUNE_ONE_ROUND, 0)};
}

// `compute` is MANET_COMPUTE_BF16_REFINE / _F16_REFINE for the refine forms and MANET_COMPUTE_F32 for the arg forms.
MatchPlan match_plan(int64_t N, int64_t M0, int C, int n_ids, int k_nn, int compute, int form, const MatchTune &tune)
{
    const BankLayout BL = bank_layout(M0, C, n_ids, compute);
    const MatchLayout ML = match_layout(N, C, n_ids, compute, k_nn, form == MATCH_FORM_ARG || form == MATCH_FORM_NTH_ARG);
    const bool main = form == MATCH_FORM_MAIN, filter = form == MATCH_FORM_REFINE_FILTER;
    const bool rescue = form == MATCH_FORM_REFINE_RESCUE || form == MATCH_FORM_REFINE_RESCUE_EXACT;
    MatchPlan P;
    P.form = form;
    P.compute = compute;
    P.k_nn = k_nn;
    P.steps = rescue ? BL.G32.steps : ML.G.steps;
    P.nQT = rescue ? (int)(ML.N_pad / QT) : ML.nQT;
    P.T_max = form == MATCH_FORM_REFINE_PRE ? BL.T_sub_max : BL.T_max;
    // resident workgroup slots: f32 and plain bf16 (wide kernel) = 2 x 256-thread workgroups per CU,
    // split-bf16 and the narrow plain-bf16 kernel (C > 106) = 1 x 512-thread workgroup per CU
    const bool plain2 = compute == MANET_COMPUTE_BF16 || compute == MANET_COMPUTE_F16;  // one MFMA per 16 k on 2-byte elements
    const bool one_per_cu = compute == MANET_COMPUTE_BF16X3 || (plain2 && ML.G.steps == 9);
    P.slots = main && one_per_cu ? 256 : 512;
    // two tile buffers (plain bf16: two tiles per step); the filter adds its candidate sub-lists and the published keys
    const size_t tile_bytes = rescue ? BL.G32.tile_bytes : BL.tile_bytes;
    P.lds = (size_t)((BL.G.compute == MANET_COMPUTE_BF16 || BL.G.compute == MANET_COMPUTE_F16) && !rescue ? 4 : 2) * tile_bytes;
    if (filter) P.lds += (size_t)REFINE_LDS_LIST * 8 + 4 * 256 * 4;
    P.S = pick_splits(P.nQT, P.T_max, P.slots);
    if (main && tune.splits > 0) P.S = (tune.splits + 7) / 8 * 8;  // tuning only
    if (main && k_nn > 1) P.S = TOPK_SPLITS;
    // (at most 16 splits: a healthy frame pays for the dispatch of nQT x S workgroups that return at once -- 7.7 us at 48
    // splits -- and a full rescue loses ~10 % to the coarser last round; forced exact: the fp32 kernel's own split count)
    if (form == MATCH_FORM_REFINE_RESCUE && P.S > 16) P.S = 16;
    P.grid = (unsigned)(P.nQT * P.S);
    P.block_map = block_map_arg(P.nQT, P.slots, filter ? 0 : P.S, (double)P.T_max * (double)tile_bytes, tune.block_map);
    if (main && compute == MANET_COMPUTE_F32 && k_nn == 1 && tune.one_round != 1) P.block_map |= ONE_ROUND_OK;  // (1: A/B timing)
    if (form == MATCH_FORM_REFINE_RESCUE) P.block_map = RESCUE_LISTED;  // dealt to the tiles the re-rank launch listed
    // the filter's spread map (see split_of_block).  (PB splits fastest on top of it, as the plain kernels have it: fabric
    // fetch of this pass 301 -> 176 MB at cfg3 shape, but concurrent splits of one object share thresholds later --
    // 4.3 -> 5.05 candidate rows per pair -- and the step got 1 % slower: not taken.)
    if (filter && (P.block_map & 0xff) == 0) {
        P.block_map |= 3;
        if (FILTER_TAIL_CUTS > 1 && (P.S & 7) == 0) {  // (tapered tail: see tapered_split_of_block)
            P.block_map = (P.block_map & ~0xff) | 8;
            P.grid = (unsigned)(P.nQT * (P.S + 8 * (FILTER_TAIL_CUTS - 1)));
        }
    }
    return P;
}

// One dispatch over the instantiated widths: f(std::integral_constant<int, K>{}) for the runtime k-step count (the last K for
// any other) -- fp32 (pick_ks): 16 / 50 / 52 / 64 v_mfma_f32_32x32x2_f32; bf16 (pick_ksb): 2 / 7 / 9 v_mfma_f32_32x32x16_bf16
template <int K0, int... Ks, typename F>
void with_steps(int steps, F &&f)
{
    if constexpr (sizeof...(Ks) == 0) f(std::integral_constant<int, K0>{});
    else if (steps == K0) f(std::integral_constant<int, K0>{});
    else with_steps<Ks...>(steps, f);
}
template <typename F> void with_ks(int ks, F &&f) { with_steps<16, 50, 52, 64>(ks, f); }
template <typename F> void with_ksb(int ksb, F &&f) { with_steps<2, 7, 9>(ksb, f); }

// fp32 -> bf16, round to nearest even (NaN stays quiet NaN); same bits as the oracle's bf16_round
__device__ __forceinline__ unsigned f2bf(float x)
{
    unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ float bf2f(unsigned b) { return __uint_as_float(b << 16); }

// an fp32 value as three bf16 pieces, p0 + p1 + p2 == x exactly (3 x 8 significand bits)
__device__ __forceinline__ void split3_bf16(float x, unsigned (&p)[3])
{
    p[0] = f2bf(x);
    float r = x - bf2f(p[0]);
    p[1] = f2bf(r);
    r = r - bf2f(p[1]);
    p[2] = f2bf(r);
}

// fp32 -> fp16, round to nearest even (v_cvt_f16_f32: beyond 65504 -> infinity, NaN stays NaN), and back (exact)
__device__ __forceinline__ unsigned f2h(float x) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)x); }
__device__ __forceinline__ float h2f(unsigned b) { return (float)__builtin_bit_cast(_Float16, (unsigned short)b); }
// ... with a subnormal result replaced by zero: what the norm slots store (see the f16 image)
__device__ __forceinline__ unsigned f2h_normal(float x)
{
    const unsigned b = f2h(x);
    return (b & 0x7c00u) ? b : 0u;
}

// a row's squared norm as three SCALED fp16 pieces, p[0] + p[1] * 2^-11 + p[2] * 2^-14 (see the f16 image): each piece zero or
// normal; the sum equals x for x >= 2^-5 and is within 2^-28 of it below.  x = +inf (a padding row) -> {+inf, 0, 0}; any other
// value outside [0, 65504], NaN included -> {NaN, 0, 0}.
__device__ __forceinline__ void split3_f16(float x, unsigned (&p)[3])
{
    if (!(x >= 0.0f && x <= 65504.0f)) {
        p[0] = (x == INFINITY) ? 0x7c00u : 0x7e00u;
        p[1] = p[2] = 0u;
        return;
    }
    p[0] = f2h_normal(x);
    float r = x - h2f(p[0]);                    // exact: |r| <= half an ulp of p[0] (or x itself, below 2^-14)
    p[1] = f2h_normal(r * 2048.0f);
    r = r - h2f(p[1]) * (1.0f / 2048.0f);       // exact
    p[2] = f2h_normal(r * 16384.0f);
}

// embedding element types the pack kernels read (the producer's storage):
// float, or bf16 as raw 16-bit words
__device__ __forceinline__ float emb_load(const float *p, long i) { return p[i]; }
__device__ __forceinline__ float emb_load(const unsigned short *p, long i) { return bf2f(p[i]); }

// order-preserving float -> uint key (so atomicMin on keys == min on floats, negatives included:
// d may be slightly negative from rounding and must not be clamped)
// NaN -> key 0: it wins every atomicMin and float_of(0) is a NaN again, so a NaN distance propagates
// to the output like torch.min does (IntVOS.py:84).
__device__ __forceinline__ unsigned key_of(float f)
{
    unsigned u = __float_as_uint(f);
    if (f != f) return 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(unsigned k)
{
    unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}

// NaN-propagating minimum (v_minimum3_f32 on gfx950): torch.min semantics, and -- unlike fminf on an MFMA
// result -- needs no canonicalising v_max in front of it.
__device__ __forceinline__ float min3p(float m, float a, float b)
{
    return __builtin_elementwise_minimum(__builtin_elementwise_minimum(m, a), b);
}

}  // namespace

// ---- host functions that cross files (each defined once).  csrc/global_prepare.hip:
void fill32(void *p, unsigned value, size_t words, hipStream_t st);
int launch_bank_pack(const void *src, int emb_dtype, long s_row, long s_c, const int *src_of, const int *meta, long n_rows,
                     int C, const Geom &G, char *dst, long ntiles, hipStream_t st);
int launch_query_pack(const void *src, int emb_dtype, long s_row, long s_c, long N, long N_pad, int C, const Geom &G,
                      char *dst, unsigned *keys, int n_ids, hipStream_t st);
// csrc/global_refine.hip (called by manet_global_match_prepared_ex):
int run_refine(int compute, const char *qimg, const void *qraw, int q_dtype, long q_sn, long q_sc, const char *bws,
               const BankLayout &BL, char *mws, const MatchLayout &ML, long N, int64_t M0, int C, int n_ids, float *out, float *mem,
               int flags, hipStream_t st);
// csrc/global_match.hip: the main kernel of the plan's form -- how run_refine reaches the three kernels it borrows, the pre-pass
// (bf16_wide<K, false> / f16_match_wide), the filter (bf16_wide<K, true> / refine_filter_half) and the rescue (f32_pipe<KS, true>)
// -- and the closing decode
void launch_match(const MatchPlan &P, const MatchArgs &A, hipStream_t st);
void launch_global_finish(unsigned *keys, long N, long N_pad, int n_ids, int flags, float *out, float *mem, long total,
                          hipStream_t st);
