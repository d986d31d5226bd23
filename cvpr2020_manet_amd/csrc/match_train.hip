// Ordered (atomic-free) backward of the matching path, MI355X (gfx950): the opt-in training route behind
// ops.global_match / ops.local_match(deterministic=True) and IntVOS(train_match="ordered").
//
// The default route (csrc/global_match.hip global_match_backward_kernel, csrc/local_train.hip local_bwd_scatter*_kernel) adds
// colliding contributions with float atomicAdd: the sum depends on arrival order and its last bits change from run to run.
// Here every sum has ONE owner that adds its terms in an order fixed by indices alone, so the gradients are the same bits on
// every run.  No float atomic anywhere in this file (tests/test_match_train_abi.py reads the device assembly).
//
//   global match (reference IntVOS.py:32-39, :84, :87-94; all k ranks in one call)
//     mt_rows_kernel          the query embedding as [N][C] rows (whatever the caller's strides): a bank row's owner reads the
//                             queries that selected it as 4 C-byte runs instead of C strided words
//     mt_global_query_kernel  d/dq_n = sum_{r,o} 2 gw (q_n - k_m): lane-local, ascending (r, o)
//     mt_global_bank_kernel   workgroup = ROWS bank rows.  It scans the whole entry list arg[r][n][o] (N n_ids r ints, L2-resident)
//                             twice: a counting pass (hits per 256-entry chunk), a prefix sum over the chunks, a filling pass
//                             that writes every hit at its exact rank -- the list is in ascending (r, n, o) order whichever
//                             wave found an entry.  Then thread c walks the list and adds -2 gw (q_n[c] - k_m[c]) into the LDS
//                             accumulator of (row m, channel c): one owner, ascending order -- a rank's terms into a sum of
//                             their own, the ranks' sums joined in ascending rank (the association of one backward per rank).
//   local match, downsample configuration (IntVOS.py:266-296, :398-432): sparse -- work scales with the winners, there is no
//   dense gradient volume and nothing is zero-filled in memory
//     mt_local_min_arg_kernel the training forward's masked minimum + winning offset, 25 x 2 candidates' worth of threads per pixel
//     mt_pool_cl_kernel       2x2 mean of both frames, channel-LAST [cell][C] (the arithmetic of pool2x2_kernel)
//     mt_local_cell_kernel    one wave per pooled cell t: the winners among the full-resolution pixels whose bilinear taps
//                             include t (at most 5 x 5 pixels x n_ids at this 2x ratio), in ascending (y, x, o), each adding
//                             a = g w_t (1 - Vn[l][t]^2) / 2 into the cell's per-offset sum in LDS; the touched offsets, ascending,
//                             become the cell's list (offset, A) + an offset bitmap; d/dx_p[c][t] = sum_l 2 A (x_p[c][t] - y_p[c][t+l])
//                             with channels across lanes
//     mt_local_prev_kernel    one wave per destination cell q: offsets l ascending, t = q - l; a bit test finds the cells that
//                             selected q, d/dy_p[c][q] -= 2 A (x_p[c][t] - y_p[c][q])
//     mt_unpool_kernel        backward of the 2x2 mean into the caller's strided gradient (x 0.25)
//   local match, MODEL_LOCAL_DOWNSAMPLE = False (IntVOS.py:299-313): the only collision is between the objects of one pixel
//     mt_full_dv_kernel       one owner per pixel adds its objects in ascending order into dV[l][pixel]
//     mt_full_dist_kernel     the dense gather of local_bwd_dist_kernel, each half only if its gradient is wanted
#include "manet_common.h"
#include "local_geom.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// global match

constexpr int MT_NT = 256;         // threads of the bank kernel
constexpr int MT_CHUNK = 256;      // entries per chunk: one wave, one 16-byte load of arg and of gw per lane
constexpr int MT_MAXCH = 512;      // chunks per epoch of the scan (128 Ki entries)
constexpr int MT_LCAP = 1024;      // list entries in LDS (>= MT_CHUNK: a chunk always fits)
constexpr int MT_UNROLL = 8;       // query rows in flight per thread in the sum phase

__global__ __launch_bounds__(256) void mt_rows_kernel(const float *__restrict__ q, long q_sn, long q_sc, long N, int C,
                                                      float *__restrict__ qt)
{
    __shared__ float tile[32][33];
    const long n0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {  // lanes along n: contiguous for the head's C-major embeddings
        const long n = n0 + tx;
        const int c = c0 + j;
        tile[j][tx] = (n < N && c < C) ? q[n * q_sn + (long)c * q_sc] : 0.0f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const long n = n0 + j;
        const int c = c0 + tx;
        if (n < N && c < C) qt[n * C + c] = tile[tx][j];
    }
}

// thread = (query n, channel c), lanes along n (global_match_backward_kernel's map); ranks outer, objects inner
__global__ void mt_global_query_kernel(const float *__restrict__ q, long q_sn, long q_sc, const float *__restrict__ k,
                                       long k_sm, long k_sc, const int *__restrict__ arg, const float *__restrict__ gw,
                                       long N, long M0, int C, int n_ids, int ranks, float *__restrict__ gq, long gq_sn,
                                       long gq_sc)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * C) return;
    const long n = i % N;
    const int c = (int)(i / N);
    const float qv = q[n * q_sn + (long)c * q_sc];
    float acc = 0.0f;
    for (int r = 0; r < ranks; ++r) {  // a rank's objects in ascending order, then the ranks' sums in ascending order
        const long e0 = ((long)r * N + n) * n_ids;
        float part = 0.0f;
        for (int o = 0; o < n_ids; ++o) {
            const int m = arg[e0 + o];
            const float g = gw[e0 + o];
            if (m < 0 || m >= M0 || g == 0.0f) continue;
            part += 2.0f * g * (qv - k[(long)m * k_sm + (long)c * k_sc]);
        }
        acc = r == 0 ? part : acc + part;
    }
    gq[n * gq_sn + (long)c * gq_sc] = acc;
}

// the four entries 4 v .. 4 v + 3 of a list (16-byte aligned base); past the end: m = -1, g = 0
__device__ __forceinline__ void mt_load4(const int *__restrict__ arg, const float *__restrict__ gw, long e, long E, int m[4],
                                         float g[4])
{
    if (e + 4 <= E) {
        const int4 a = *(const int4 *)(arg + e);
        const float4 b = *(const float4 *)(gw + e);
        m[0] = a.x, m[1] = a.y, m[2] = a.z, m[3] = a.w;
        g[0] = b.x, g[1] = b.y, g[2] = b.z, g[3] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = (e + j < E) ? arg[e + j] : -1;
            g[j] = (e + j < E) ? gw[e + j] : 0.0f;
        }
    }
}

template <int ROWS>
__global__ __launch_bounds__(MT_NT) void mt_global_bank_kernel(const float *__restrict__ qt, const float *__restrict__ k,
                                                               long k_sm, long k_sc, const int *__restrict__ arg,
                                                               const float *__restrict__ gw, long N, long M0, int C,
                                                               int n_ids, int ranks, float *__restrict__ gk, long gk_sm,
                                                               long gk_sc)
{
    __shared__ float kb[ROWS * MANET_MAX_C];                           // [row][C]: the bank rows,
    __shared__ float acc[ROWS * MANET_MAX_C], cur[ROWS * MANET_MAX_C];  // the sum of the finished ranks, the current rank's sum
    __shared__ int ln[MT_LCAP], lm[MT_LCAP];                           // the list: query row, (bank row - m0) | rank << 8,
    __shared__ float lg[MT_LCAP];                                      // weighted incoming gradient
    __shared__ int offc[MT_MAXCH + 1];                                 // hits per chunk -> exclusive prefix
    __shared__ int wsum[MT_NT / 64], group_end;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = MT_NT / 64;
    const long m0 = (long)blockIdx.x * ROWS;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int i = tid; i < ROWS * C; i += MT_NT) {  // lanes along the rows: contiguous for a C-major bank
        const int j = i % ROWS, c = i / ROWS;
        kb[j * C + c] = (m0 + j < M0) ? k[(m0 + j) * k_sm + (long)c * k_sc] : 0.0f;
        acc[j * C + c] = 0.0f;
        cur[j * C + c] = 0.0f;
    }
    int rank_now = 0;  // rank of the entries in `cur` (the list is in ascending rank: every thread sees the same changes)
    const long E = (long)ranks * N * n_ids;
    const long per_rank = N * n_ids;
    for (long eb = 0; eb < E; eb += (long)MT_MAXCH * MT_CHUNK) {
        const long left = E - eb;
        const int nch = left >= (long)MT_MAXCH * MT_CHUNK ? MT_MAXCH : (int)((left + MT_CHUNK - 1) / MT_CHUNK);
        __syncthreads();  // (the previous epoch's readers of offc are done; first epoch: kb / acc are staged)
        // counting pass: chunk j is entries eb + 256 j .., lane's four at + 4 lane
        for (int j = wave; j < nch; j += NW) {
            int m[4];
            float g[4];
            mt_load4(arg, gw, eb + (long)j * MT_CHUNK + 4 * lane, E, m, g);
            int c_ = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) c_ += __popcll(__ballot(m[u] >= m0 && m[u] < m0 + ROWS && m[u] < M0 && g[u] != 0.0f));
            if (lane == 0) offc[j] = c_;
        }
        __syncthreads();
        // exclusive prefix over the nch <= 512 counts: up to four per thread, a wave scan, the waves' sums through LDS
        {
            int v[4], s = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = (4 * tid + u < nch) ? offc[4 * tid + u] : 0;
                s += v[u];
            }
            int inc = s;
#pragma unroll
            for (int st = 1; st < 64; st <<= 1) {
                const int t = __shfl_up(inc, st);
                if (lane >= st) inc += t;
            }
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();
            int base = inc - s;
            for (int w_ = 0; w_ < wave; ++w_) base += wsum[w_];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (4 * tid + u < nch) offc[4 * tid + u] = base;
                base += v[u];
            }
            if (tid == MT_NT - 1) offc[nch] = base;  // (4 * 256 >= MT_MAXCH: the last thread's running sum is the total)
        }
        __syncthreads();
        // groups of chunks whose hits fit the list (all of them but for a bank row that a large share of the queries selected)
        int gs = 0;
        while (gs < nch) {
            int ge = nch;
            if (offc[nch] - offc[gs] > MT_LCAP) {
                if (tid == 0) {
                    int e_ = gs + 1;  // (one chunk always fits)
                    while (e_ < nch && offc[e_ + 1] - offc[gs] <= MT_LCAP) ++e_;
                    group_end = e_;
                }
                __syncthreads();
                ge = group_end;
            }
            const int first = offc[gs];
            // filling pass: every hit at its rank = ascending (r, n, o)
            for (int j = gs + wave; j < ge; j += NW) {
                int m[4];
                float g[4];
                const long e = eb + (long)j * MT_CHUNK + 4 * lane;
                mt_load4(arg, gw, e, E, m, g);
                bool hit[4];
                int p = offc[j] - first;  // + the hits of the lanes below: entries 4 lane .. 4 lane + 3 follow theirs
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    hit[u] = m[u] >= m0 && m[u] < m0 + ROWS && m[u] < M0 && g[u] != 0.0f;
                    p += __popcll(__ballot(hit[u]) & lt);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (hit[u]) {
                        ln[p] = (int)(((e + u) % per_rank) / n_ids);
                        lm[p] = (int)(m[u] - m0) | ((int)((e + u) / per_rank) << 8);
                        lg[p] = g[u];
                        ++p;
                    }
                }
            }
            __syncthreads();
            const int count = offc[ge] - first;
            if (tid < C) {
                // a rank's terms in ascending (n, o) into `cur`; at a change of rank `cur` joins `acc`: the association of one
                // backward per rank summed in ascending rank (what the atomic route's k > 1 backward computes, order aside)
                const float *qc = qt + tid;
                auto one_by_one = [&](int i0, int i1) {  // (a batch that crosses a change of rank, and the tail)
#pragma unroll 1
                    for (int i = i0; i < i1; ++i) {
                        const int r = lm[i] >> 8;
                        if (r != rank_now) {
#pragma unroll 1
                            for (int j = 0; j < ROWS; ++j) {
                                acc[j * C + tid] += cur[j * C + tid];
                                cur[j * C + tid] = 0.0f;
                            }
                            rank_now = r;
                        }
                        const int a = (lm[i] & 255) * C + tid;
                        cur[a] -= 2.0f * lg[i] * (qc[(long)ln[i] * C] - kb[a]);
                    }
                };
                int i = 0;
                for (; i + MT_UNROLL <= count; i += MT_UNROLL) {
                    if ((lm[i] >> 8) != rank_now || (lm[i + MT_UNROLL - 1] >> 8) != rank_now) {  // (ranks ascend along the list)
                        one_by_one(i, i + MT_UNROLL);
                        continue;
                    }
                    float qv[MT_UNROLL];
#pragma unroll
                    for (int u = 0; u < MT_UNROLL; ++u) qv[u] = qc[(long)ln[i + u] * C];
#pragma unroll
                    for (int u = 0; u < MT_UNROLL; ++u) {
                        const int a = (lm[i + u] & 255) * C + tid;
                        cur[a] -= 2.0f * lg[i + u] * (qv[u] - kb[a]);
                    }
                }
                one_by_one(i, count);
            }
            __syncthreads();  // the list is free again
            gs = ge;
        }
    }
    __syncthreads();
    for (int i = tid; i < ROWS * C; i += MT_NT) {
        const int j = i % ROWS, c = i / ROWS;
        if (m0 + j < M0) gk[(m0 + j) * gk_sm + (long)c * gk_sc] = acc[j * C + c] + cur[j * C + c];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// local match

constexpr int MT_MAXPP = (2 * MANET_MAX_LOCAL_DISTANCE + 1) * (2 * MANET_MAX_LOCAL_DISTANCE + 1);  // 625 window offsets
constexpr int MT_WORDS = (MT_MAXPP + 31) / 32;                                                      // 20 bitmap words
constexpr int MT_ROUNDS = (MT_MAXPP + 63) / 64;                                                     // 10 rounds of 64 offsets

int mt_check_local(int h, int w, int C, int d, int n_ids, int downsample)
{
    if (h <= 0 || w <= 0 || C <= 0) return manet_set_error(MANET_E_INVALID, "h=%d w=%d C=%d", h, w, C);
    if (C > MANET_MAX_C) return manet_set_error(MANET_E_INVALID, "C=%d (supported 1..%d)", C, MANET_MAX_C);
    if (d < 0 || d > MANET_MAX_LOCAL_DISTANCE)
        return manet_set_error(MANET_E_INVALID, "max_distance=%d (supported 0..%d)", d, MANET_MAX_LOCAL_DISTANCE);
    if (n_ids <= 0 || n_ids > MANET_MAX_IDS)
        return manet_set_error(MANET_E_INVALID, "n_ids=%d (supported 1..%d)", n_ids, MANET_MAX_IDS);
    if (downsample && (h < 2 || w < 2)) return manet_set_error(MANET_E_INVALID, "downsample needs h,w >= 2");
    return MANET_OK;
}

// most full-resolution positions whose bilinear taps (i0, i1) include one pooled position: 5 for every size from 12 to 480 at
// this 2x ratio (a few more below that), counted with the kernels' own expression
int mt_max_cover(int in_size, int out_size)
{
    int best = 1;
    for (int t = 0; t < in_size; ++t) {
        const int n = bilin_first(t + 1, in_size, out_size) - bilin_first(t - 1, in_size, out_size);
        best = n > best ? n : best;
    }
    return best;
}

struct MtLocalLayout {
    int hp, wp, cap;
    size_t off_xt, off_yt, off_gx, off_gy, off_cnt, off_ll, off_la, off_bits, off_pref, total;
};
MtLocalLayout mt_local_layout(int h, int w, int C, int n_ids, int d)
{
    MtLocalLayout L;
    L.hp = h / 2;
    L.wp = w / 2;
    const size_t plane = (size_t)L.hp * L.wp;
    const long PP = (long)(2 * d + 1) * (2 * d + 1);
    const long items = (long)mt_max_cover(L.hp, h) * mt_max_cover(L.wp, w) * n_ids;
    L.cap = (int)(items < PP ? items : PP);
    const size_t emb = manet_align_up(plane * C * sizeof(float), 256);
    L.off_xt = 0;
    L.off_yt = emb;
    L.off_gx = 2 * emb;
    L.off_gy = 3 * emb;
    L.off_cnt = 4 * emb;
    L.off_ll = L.off_cnt + manet_align_up(plane * sizeof(int), 256);
    L.off_la = L.off_ll + manet_align_up(plane * L.cap * sizeof(int), 256);
    L.off_bits = L.off_la + manet_align_up(plane * L.cap * sizeof(float), 256);
    L.off_pref = L.off_bits + manet_align_up(plane * MT_WORDS * sizeof(int), 256);
    L.total = L.off_pref + manet_align_up(plane * MT_WORDS * sizeof(int), 256);
    return L;
}

// IntVOS.py:282-284  F.avg_pool2d(x, (2,2), (2,2)) of both frames, channel-last: window summed row-major, times 1/4 (exact)
__global__ void mt_pool_cl_kernel(const float *__restrict__ a, long a_sy, long a_sx, long a_sc, const float *__restrict__ b,
                                  long b_sy, long b_sx, long b_sc, int C, int hp, int wp, float *__restrict__ at,
                                  float *__restrict__ bt)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)hp * wp * C) return;
    const int c = (int)(i % C);
    const long cell = i / C;
    const int py = (int)(cell / wp), px = (int)(cell - (long)py * wp);
    const float *p = a + (2L * py) * a_sy + (2L * px) * a_sx + (long)c * a_sc;
    const float *q = b + (2L * py) * b_sy + (2L * px) * b_sx + (long)c * b_sc;
    at[i] = (((p[0] + p[a_sx]) + p[a_sy]) + p[a_sy + a_sx]) * 0.25f;
    bt[i] = (((q[0] + q[b_sx]) + q[b_sy]) + q[b_sy + b_sx]) * 0.25f;
}

// One wave per pooled cell t.  xt / yt: pooled current / previous frame [cell][C]; vol: the forward's normalised pooled volume
// [P*P][hp][wp]; arg / gout [h][w][n_ids].  Writes the cell's list (ll, la: offsets ascending and their summed coefficient A, at
// most cap), its offset bitmap with the running bit counts (bits, pref: MT_WORDS words each) -- only if want_lists -- and
// gxp[c][cell] (NULL: the current frame needs no gradient).
__global__ __launch_bounds__(64) void mt_local_cell_kernel(const float *__restrict__ xt, const float *__restrict__ yt,
                                                           const float *__restrict__ vol, const int *__restrict__ arg,
                                                           const float *__restrict__ gout, int h, int w, int hp, int wp,
                                                           int C, int n_ids, int d, int cap, int want_lists,
                                                           int *__restrict__ lcnt, int *__restrict__ ll,
                                                           float *__restrict__ la, unsigned *__restrict__ bits,
                                                           int *__restrict__ pref, float *__restrict__ gxp)
{
    __shared__ float dv[MT_ROUNDS * 64];    // per-offset sum of a
    __shared__ unsigned touched[MT_WORDS];  // offsets some winner selected
    __shared__ int cl[MT_ROUNDS * 64], cq[MT_ROUNDS * 64];  // the list: offset; the previous-frame cell t + l (-1: outside)
    __shared__ float cA[MT_ROUNDS * 64];
    const int lane = threadIdx.x;
    const int cell = blockIdx.x;
    const int ty = cell / wp, tx = cell - ty * wp;
    const int P = 2 * d + 1, PP = P * P;
    const long plane = (long)hp * wp;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int i = lane; i < MT_ROUNDS * 64; i += 64) dv[i] = 0.0f;
    if (lane < MT_WORDS) touched[lane] = 0u;
    __syncthreads();
    // full-resolution rows / columns with i0 in {t - 1, t}: every position whose taps can include t
    const int ya = bilin_first(ty - 1, hp, h), yb = bilin_first(ty + 1, hp, h);
    const int xa = bilin_first(tx - 1, wp, w), xb = bilin_first(tx + 1, wp, w);
    const int nx = xb - xa, items = (yb - ya) * nx * n_ids;
    for (int base = 0; base < items; base += 64) {  // ascending (y, x, o)
        const int it = base + lane;
        bool act = it < items;
        int l = 0;
        float a00 = 0.0f, a01 = 0.0f, a10 = 0.0f, a11 = 0.0f;
        bool sy0 = false, sy1 = false, sx0 = false, sx1 = false;
        if (act) {
            const int o = it % n_ids, r = it / n_ids;
            const int y = ya + r / nx, x = xa + r % nx;
            const long e = ((long)y * w + x) * n_ids + o;
            l = arg[e];
            const float g = gout[e];
            const Bilin cy = bilin_coeff(y, hp, h), cx = bilin_coeff(x, wp, w);
            sy0 = cy.i0 == ty, sy1 = cy.i1 == ty, sx0 = cx.i0 == tx, sx1 = cx.i1 == tx;
            act = l >= 0 && l < PP && g != 0.0f && (sy0 || sy1) && (sx0 || sx1);
            if (act) {
                const float v = vol[(long)l * plane + cell];
                const float s = (1.0f - v * v) * 0.5f;  // d/dV of (sigmoid(V) - 0.5) * 2 at Vn = v (Vn = 1 where V = inf: 0)
                a00 = g * cy.l0 * cx.l0 * s;
                a01 = g * cy.l0 * cx.l1 * s;
                a10 = g * cy.l1 * cx.l0 * s;
                a11 = g * cy.l1 * cx.l1 * s;
            }
        }
        unsigned long long m = __ballot(act);
        while (m) {  // one lane at a time, ascending: the order of the sum is the order of the items
            const int i = __ffsll((long long)m) - 1;
            m &= m - 1;
            if (lane == i) {
                float s = dv[l];
                if (sy0 && sx0) s += a00;
                if (sy0 && sx1) s += a01;
                if (sy1 && sx0) s += a10;
                if (sy1 && sx1) s += a11;
                dv[l] = s;
                touched[l >> 5] |= 1u << (l & 31);
            }
        }
    }
    __syncthreads();
    int count = 0;
#pragma unroll 1
    for (int b = 0; b < PP; b += 64) {
        const int l = b + lane;
        const bool t = l < PP && ((touched[l >> 5] >> (l & 31)) & 1u);
        const unsigned long long m = __ballot(t);
        if (t) {
            const int p = count + __popcll(m & lt);
            const int qy = ty + l / P - d, qx = tx + l % P - d;
            cl[p] = l;
            cq[p] = (qy >= 0 && qy < hp && qx >= 0 && qx < wp) ? qy * wp + qx : -1;
            cA[p] = dv[l];
        }
        count += __popcll(m);
    }
    __syncthreads();
    if (want_lists) {
        const int n = count < cap ? count : cap;  // (count <= cap: the launcher sized cap from the same cover counts)
        if (lane == 0) lcnt[cell] = n;
        for (int i = lane; i < n; i += 64) {
            ll[(long)cell * cap + i] = cl[i];
            la[(long)cell * cap + i] = cA[i];
        }
        if (lane < MT_WORDS) {
            int before = 0;
            for (int j = 0; j < lane; ++j) before += __popc(touched[j]);
            bits[(long)cell * MT_WORDS + lane] = touched[lane];
            pref[(long)cell * MT_WORDS + lane] = before;
        }
    }
    if (!gxp) return;
    for (int c = lane; c < C; c += 64) {
        const float xv = xt[(long)cell * C + c];
        float acc = 0.0f;
        for (int i = 0; i < count; i += 4) {  // ascending offsets; four previous-frame values in flight
            float yv[4], A[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = (i + j < count) ? cq[i + j] : -1;
                ok[j] = q >= 0;
                yv[j] = yt[(long)(ok[j] ? q : cell) * C + c];
                A[j] = ok[j] ? cA[i + j] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ok[j]) acc += 2.0f * (xv - yv[j]) * A[j];
        }
        gxp[(long)c * plane + cell] = acc;
    }
}

// One wave per previous-frame cell q: for the offsets l in ascending order, the cell t = q - l that may have selected q; its
// bitmap says whether it did, the running bit count where in its list the coefficient is.  Lanes then hold channels (c, c + 64).
__global__ __launch_bounds__(64) void mt_local_prev_kernel(const float *__restrict__ xt, const float *__restrict__ yt,
                                                           const float *__restrict__ la, const unsigned *__restrict__ bits,
                                                           const int *__restrict__ pref, int hp, int wp, int C, int d,
                                                           int cap, float *__restrict__ gyp)
{
    const int lane = threadIdx.x;
    const int q = blockIdx.x;
    const int qy = q / wp, qx = q - qy * wp;
    const int P = 2 * d + 1, PP = P * P;
    const long plane = (long)hp * wp;
    int src[MT_ROUNDS];
    float coef[MT_ROUNDS];
#pragma unroll
    for (int r = 0; r < MT_ROUNDS; ++r) {  // every round's look-ups are independent: issued together
        const int l = r * 64 + lane;
        src[r] = -1;
        coef[r] = 0.0f;
        if (l < PP) {
            const int sy = qy - (l / P - d), sx = qx - (l % P - d);
            if (sy >= 0 && sy < hp && sx >= 0 && sx < wp) {
                const long t = (long)sy * wp + sx;
                const unsigned wd = bits[t * MT_WORDS + (l >> 5)];
                if ((wd >> (l & 31)) & 1u) {
                    const int idx = pref[t * MT_WORDS + (l >> 5)] + __popc(wd & ((1u << (l & 31)) - 1u));
                    if (idx < cap) {
                        src[r] = (int)t;
                        coef[r] = la[t * cap + idx];
                    }
                }
            }
        }
    }
    const int c0 = lane, c1 = lane + 64;
    const bool h0 = c0 < C, h1 = c1 < C;
    const float yv0 = h0 ? yt[(long)q * C + c0] : 0.0f, yv1 = h1 ? yt[(long)q * C + c1] : 0.0f;
    float acc0 = 0.0f, acc1 = 0.0f;
#pragma unroll
    for (int r = 0; r < MT_ROUNDS; ++r) {
        unsigned long long m = __ballot(src[r] >= 0);
        while (m) {  // hits in ascending lane = ascending offset, four cells in flight
            int t[4];
            float A[4], x0[4], x1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                t[j] = -1;
                A[j] = 0.0f;
                if (m) {
                    const int i = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    t[j] = __shfl(src[r], i);
                    A[j] = __shfl(coef[r], i);
                }
                const long row = (long)(t[j] >= 0 ? t[j] : q) * C;
                x0[j] = h0 ? xt[row + c0] : 0.0f;
                x1[j] = h1 ? xt[row + c1] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (t[j] >= 0) {
                    acc0 -= 2.0f * (x0[j] - yv0) * A[j];
                    acc1 -= 2.0f * (x1[j] - yv1) * A[j];
                }
            }
        }
    }
    if (h0) gyp[(long)c0 * plane + q] = acc0;
    if (h1) gyp[(long)c1 * plane + q] = acc1;
}

// backward of the 2x2 average pooling into ONE of the caller's (strided) gradient tensors; gp [C][hp][wp]
__global__ void mt_unpool_kernel(const float *__restrict__ gp, int C, int h, int w, int hp, int wp, float *__restrict__ gout,
                                 long sy, long sx, long sc)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long plane = (long)h * w;
    if (i >= plane * C) return;
    const int c = (int)(i / plane);
    const int rem = (int)(i - (long)c * plane);
    const int y = rem / w, x = rem - y * w;
    float a = 0.0f;
    if (y < 2 * hp && x < 2 * wp) a = 0.25f * gp[(long)c * hp * wp + (long)(y / 2) * wp + (x / 2)];
    gout[(long)y * sy + (long)x * sx + (long)c * sc] = a;
}

__global__ void mt_fill_kernel(float *__restrict__ p, float v, long n)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}

// MODEL_LOCAL_DOWNSAMPLE = False: dV[l][pixel] = sum of g over the objects of the pixel that selected l, objects ascending,
// by the pixel's one owner (dv zero-filled before)
__global__ void mt_full_dv_kernel(const int *__restrict__ arg, const float *__restrict__ gout, long npix, int n_ids, int PP,
                                  float *__restrict__ dv)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    for (int o = 0; o < n_ids; ++o) {
        const int l = arg[i * n_ids + o];
        const float g = gout[i * n_ids + o];
        if (l < 0 || l >= PP || g == 0.0f) continue;
        dv[(long)l * npix + i] += g;
    }
}

// local_bwd_dist_kernel's gather on contiguous [C][h][w] planes; gxp / gyp may be NULL (that half is skipped)
__global__ void mt_full_dist_kernel(const float *__restrict__ xp, const float *__restrict__ yp, const float *__restrict__ dv,
                                    int C, int hp, int wp, int d, float *__restrict__ gxp, float *__restrict__ gyp)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long plane = (long)hp * wp;
    if (i >= plane * C) return;
    const int c = (int)(i / plane);
    const int rem = (int)(i - (long)c * plane);
    const int py = rem / wp, px = rem - py * wp;
    const int P = 2 * d + 1;
    const float *xc = xp + (long)c * plane, *yc = yp + (long)c * plane;
    const float xv = xc[rem], yv = yc[rem];
    float gx = 0.0f, gy = 0.0f;
    for (int dy = 0; dy < P; ++dy) {
        for (int dx = 0; dx < P; ++dx) {
            const long l = (long)(dy * P + dx) * plane;
            const int qy = py + dy - d, qx = px + dx - d;  // neighbour this pixel looked at
            if (gxp && qy >= 0 && qy < hp && qx >= 0 && qx < wp) gx += 2.0f * (xv - yc[qy * wp + qx]) * dv[l + rem];
            const int sy = py - (dy - d), sx = px - (dx - d);  // pixel that looked at this one
            if (gyp && sy >= 0 && sy < hp && sx >= 0 && sx < wp) gy -= 2.0f * (xc[sy * wp + sx] - yv) * dv[l + sy * wp + sx];
        }
    }
    if (gxp) gxp[i] = gx;
    if (gyp) gyp[i] = gy;
}

// Training forward of the local match, downsample configuration: local_min_arg_kernel's result -- the masked minimum over the
// window and the offset that attains it, same candidates, same bilin_sample expression, strict <, first offset wins, -1 when the
// constant 1.0 wins: the same bits -- with the (2d+1)^2 candidates of a pixel dealt to 16 waves x 2 half-rows instead of one
// thread's serial loop (625 dependent round trips at d = 12).  Workgroup = 32 consecutive pixels: lane = (pixel, half of the
// window columns), wave k takes the window rows k, k + 16; every candidate is sampled unconditionally, so a wave's loads issue
// back to back; the partial (value, offset) pairs meet in LDS, smallest value first, smallest offset among equals.
constexpr int MT_FW_WAVES = 16, MT_FW_NI = 4;  // waves per workgroup; object ids per pass
__device__ __forceinline__ float mt_bilin_sample(const float *__restrict__ pl, int wp, const Bilin &by, const Bilin &bx)
{
    return by.l0 * (bx.l0 * pl[by.i0 * wp + bx.i0] + bx.l1 * pl[by.i0 * wp + bx.i1]) +
           by.l1 * (bx.l0 * pl[by.i1 * wp + bx.i0] + bx.l1 * pl[by.i1 * wp + bx.i1]);
}
__global__ __launch_bounds__(64 * MT_FW_WAVES) void mt_local_min_arg_kernel(const float *__restrict__ dvol,
                                                                            const int *__restrict__ labels, int h, int w,
                                                                            int hp, int wp, int d, int n_ids,
                                                                            float *__restrict__ out, int *__restrict__ arg)
{
    __shared__ float rv[MT_FW_WAVES][MT_FW_NI][64];
    __shared__ int rc[MT_FW_WAVES][MT_FW_NI][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pix = lane & 31, half = lane >> 5;
    const long i = (long)blockIdx.x * 32 + pix;
    const bool valid = i < (long)h * w;
    const int y = valid ? (int)(i / w) : 0, x = valid ? (int)(i - (long)y * w) : 0;
    const int P = 2 * d + 1;
    const Bilin cy = bilin_coeff(y, hp, h), cx = bilin_coeff(x, wp, w);
    const long plane = (long)hp * wp;
    const int bx0 = half ? (P + 1) / 2 : 0, bx1 = half ? P : (P + 1) / 2;
    for (int o0 = 0; o0 < n_ids; o0 += MT_FW_NI) {
        float m[MT_FW_NI];
        int code[MT_FW_NI];  // 2 l + (the candidate is the constant 1.0)
#pragma unroll
        for (int k = 0; k < MT_FW_NI; ++k) {
            m[k] = INFINITY;
            code[k] = 0x7fffffff;
        }
        if (valid) {
            for (int by = wave; by < P; by += MT_FW_WAVES) {
                const int yy = y + 2 * (by - d);
                const bool yin = (yy >= 0 && yy < h);
                for (int bx = bx0; bx < bx1; ++bx) {
                    const int xx = x + 2 * (bx - d);
                    const bool in = yin && xx >= 0 && xx < w;
                    const int lab_ = labels[in ? (long)yy * w + xx : 0];
                    const int lab = in ? lab_ : 0;
                    const int l = by * P + bx;
                    const float v = mt_bilin_sample(dvol + (long)l * plane, wp, cy, cx);
#pragma unroll
                    for (int k = 0; k < MT_FW_NI; ++k) {
                        const bool hit = (lab == o0 + k);
                        const float c = hit ? v : 1.0f;
                        if (c < m[k]) {
                            m[k] = c;
                            code[k] = 2 * l + (hit ? 0 : 1);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < MT_FW_NI; ++k) {
            rv[wave][k][lane] = m[k];
            rc[wave][k][lane] = code[k];
        }
        __syncthreads();
        if (threadIdx.x < 32 * MT_FW_NI) {
            const int p = threadIdx.x & 31, k = threadIdx.x >> 5;
            float best = INFINITY;
            int bc = 0x7fffffff;
            for (int ww = 0; ww < MT_FW_WAVES; ++ww) {
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const float v = rv[ww][k][p + 32 * hh];
                    const int c = rc[ww][k][p + 32 * hh];
                    if (v < best || (v == best && c < bc)) {
                        best = v;
                        bc = c;
                    }
                }
            }
            const long ii = (long)blockIdx.x * 32 + p;
            if (ii < (long)h * w && o0 + k < n_ids) {
                out[ii * n_ids + o0 + k] = best;
                arg[ii * n_ids + o0 + k] = (bc & 1) ? -1 : (bc >> 1);
            }
        }
        __syncthreads();
    }
}

int mt_check_global(int64_t N, int64_t M0, int C, int n_ids, int ranks)
{
    if (N <= 0 || M0 < 0) return manet_set_error(MANET_E_INVALID, "N=%lld M0=%lld", (long long)N, (long long)M0);
    if (M0 >= (1LL << 31) - 64 || N >= (1LL << 31) - 64)
        return manet_set_error(MANET_E_INVALID, "N or M0 too large for 32-bit row indices");
    if (C <= 0 || C > MANET_MAX_C) return manet_set_error(MANET_E_INVALID, "C=%d (supported 1..%d)", C, MANET_MAX_C);
    if (n_ids <= 0 || n_ids > MANET_MAX_IDS)
        return manet_set_error(MANET_E_INVALID, "n_ids=%d (supported 1..%d)", n_ids, MANET_MAX_IDS);
    if (ranks < 1 || ranks > 8) return manet_set_error(MANET_E_INVALID, "ranks=%d (supported 1..8)", ranks);
    return MANET_OK;
}

}  // namespace

// the tail of manet_local_match_train_forward_f32 (csrc/local_train.hip; csrc/local_match.hip owns the pooling and distance kernels in front of it)
void manet_mt_launch_local_min_arg(const float *vol, const int32_t *labels, int h, int w, int hp, int wp, int d, int n_ids,
                                   float *out, int32_t *arg, hipStream_t st)
{
    const long npix = (long)h * w;
    hipLaunchKernelGGL(mt_local_min_arg_kernel, dim3((unsigned)((npix + 31) / 32)), dim3(64 * MT_FW_WAVES), 0, st, vol, labels, h, w,
                       hp, wp, d, n_ids, out, arg);
}

extern "C" {

int manet_global_match_backward_ordered_workspace_bytes(int64_t N, int64_t M0, int C, int n_ids, int ranks, size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = mt_check_global(N, M0, C, n_ids, ranks);
    if (rc) return rc;
    *bytes = manet_align_up((size_t)N * C * sizeof(float), 256);
    return MANET_OK;
}

int manet_global_match_backward_ordered_f32(const float *query, int64_t q_stride_n, int64_t q_stride_c, const float *bank,
                                            int64_t b_stride_m, int64_t b_stride_c, const int32_t *arg, const float *grad_weighted,
                                            int64_t N, int64_t M0, int C, int n_ids, int ranks, float *grad_query,
                                            int64_t gq_stride_n, int64_t gq_stride_c, float *grad_bank, int64_t gb_stride_m,
                                            int64_t gb_stride_c, void *workspace, size_t workspace_bytes, manet_stream_t stream)
{
    int rc = mt_check_global(N, M0, C, n_ids, ranks);
    if (rc) return rc;
    if (!query || !arg || !grad_weighted || (!grad_query && !grad_bank) || (M0 > 0 && !bank))
        return manet_set_error(MANET_E_INVALID, "null pointer");
    if (((uintptr_t)arg | (uintptr_t)grad_weighted) & 15)
        return manet_set_error(MANET_E_INVALID, "arg and grad_weighted must be 16-byte aligned");
    const bool want_bank = grad_bank && M0 > 0;
    size_t need = 0;
    (void)manet_global_match_backward_ordered_workspace_bytes(N, M0, C, n_ids, ranks, &need);
    if (want_bank && (!workspace || workspace_bytes < need))
        return manet_set_error(MANET_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    if (grad_query) {
        const long tq = (long)N * C;
        hipLaunchKernelGGL(mt_global_query_kernel, dim3((unsigned)((tq + 255) / 256)), dim3(256), 0, st, query, (long)q_stride_n,
                           (long)q_stride_c, bank, (long)b_stride_m, (long)b_stride_c, arg, grad_weighted, (long)N, (long)M0, C,
                           n_ids, ranks, grad_query, (long)gq_stride_n, (long)gq_stride_c);
    }
    if (want_bank) {
        float *qt = (float *)workspace;
        hipLaunchKernelGGL(mt_rows_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)((C + 31) / 32)), dim3(256), 0, st, query,
                           (long)q_stride_n, (long)q_stride_c, (long)N, C, qt);
        // rows per workgroup: 16 fills the chip at the stage-1 crop (10 816 rows: 676 workgroups); 32 halves the number of
        // passes over the entry list for a large bank
        if (M0 <= 16384)
            hipLaunchKernelGGL(mt_global_bank_kernel<16>, dim3((unsigned)((M0 + 15) / 16)), dim3(MT_NT), 0, st, (const float *)qt,
                               bank, (long)b_stride_m, (long)b_stride_c, arg, grad_weighted, (long)N, (long)M0, C, n_ids, ranks,
                               grad_bank, (long)gb_stride_m, (long)gb_stride_c);
        else
            hipLaunchKernelGGL(mt_global_bank_kernel<32>, dim3((unsigned)((M0 + 31) / 32)), dim3(MT_NT), 0, st, (const float *)qt,
                               bank, (long)b_stride_m, (long)b_stride_c, arg, grad_weighted, (long)N, (long)M0, C, n_ids, ranks,
                               grad_bank, (long)gb_stride_m, (long)gb_stride_c);
    }
    return manet_check_launch("manet_global_match_backward_ordered_f32");
}

int manet_local_match_train_workspace_bytes(int h, int w, int C, int n_ids, int max_distance, size_t *bytes)
{
    if (!bytes) return manet_set_error(MANET_E_INVALID, "bytes == NULL");
    int rc = mt_check_local(h, w, C, max_distance, n_ids, 1);
    if (rc) return rc;
    *bytes = mt_local_layout(h, w, C, n_ids, max_distance).total;
    return MANET_OK;
}

int manet_local_match_train_backward_f32(const float *prev, int64_t p_sy, int64_t p_sx, int64_t p_sc, const float *cur,
                                         int64_t c_sy, int64_t c_sx, int64_t c_sc, const float *vol, const int32_t *arg,
                                         const float *grad_out, int h, int w, int C, int n_ids, int max_distance,
                                         float *grad_prev, int64_t gp_sy, int64_t gp_sx, int64_t gp_sc, float *grad_cur,
                                         int64_t gc_sy, int64_t gc_sx, int64_t gc_sc, void *workspace, size_t workspace_bytes,
                                         manet_stream_t stream)
{
    int rc = mt_check_local(h, w, C, max_distance, n_ids, 1);
    if (rc) return rc;
    if (!cur || !prev || !vol || !arg || !grad_out || (!grad_prev && !grad_cur) || !workspace)
        return manet_set_error(MANET_E_INVALID, "null pointer");
    const MtLocalLayout L = mt_local_layout(h, w, C, n_ids, max_distance);
    if (workspace_bytes < L.total) return manet_set_error(MANET_E_WORKSPACE, "workspace %zu < %zu bytes", workspace_bytes, L.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *xt = (float *)(ws + L.off_xt), *yt = (float *)(ws + L.off_yt), *gxp = (float *)(ws + L.off_gx), *gyp = (float *)(ws + L.off_gy);
    int *lcnt = (int *)(ws + L.off_cnt), *ll = (int *)(ws + L.off_ll), *pref = (int *)(ws + L.off_pref);
    float *la = (float *)(ws + L.off_la);
    unsigned *bits = (unsigned *)(ws + L.off_bits);
    const long cells = (long)L.hp * L.wp, n = cells * C, nf = (long)h * w * C;
    hipLaunchKernelGGL(mt_pool_cl_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cur, (long)c_sy, (long)c_sx,
                       (long)c_sc, prev, (long)p_sy, (long)p_sx, (long)p_sc, C, L.hp, L.wp, xt, yt);
    hipLaunchKernelGGL(mt_local_cell_kernel, dim3((unsigned)cells), dim3(64), 0, st, (const float *)xt, (const float *)yt, vol, arg,
                       grad_out, h, w, L.hp, L.wp, C, n_ids, max_distance, L.cap, grad_prev ? 1 : 0, lcnt, ll, la, bits, pref,
                       grad_cur ? gxp : (float *)nullptr);
    if (grad_cur)
        hipLaunchKernelGGL(mt_unpool_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, (const float *)gxp, C, h, w, L.hp,
                           L.wp, grad_cur, (long)gc_sy, (long)gc_sx, (long)gc_sc);
    if (grad_prev) {
        hipLaunchKernelGGL(mt_local_prev_kernel, dim3((unsigned)cells), dim3(64), 0, st, (const float *)xt, (const float *)yt,
                           (const float *)la, (const unsigned *)bits, (const int *)pref, L.hp, L.wp, C, max_distance, L.cap, gyp);
        hipLaunchKernelGGL(mt_unpool_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, (const float *)gyp, C, h, w, L.hp,
                           L.wp, grad_prev, (long)gp_sy, (long)gp_sx, (long)gp_sc);
    }
    return manet_check_launch("manet_local_match_train_backward_f32");
}

int manet_local_match_full_backward_ordered_f32(const float *prev_chw, const float *cur_chw, const int32_t *arg,
                                                const float *grad_out, int h, int w, int C, int n_ids, int max_distance,
                                                float *grad_prev_chw, float *grad_cur_chw, float *dv_ws, manet_stream_t stream)
{
    int rc = mt_check_local(h, w, C, max_distance, n_ids, 0);
    if (rc) return rc;
    if (!cur_chw || !prev_chw || !arg || !grad_out || (!grad_prev_chw && !grad_cur_chw) || !dv_ws)
        return manet_set_error(MANET_E_INVALID, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int P = 2 * max_distance + 1;
    const long plane = (long)h * w, nv = plane * P * P;
    {
        unsigned blocks = (unsigned)((nv + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(mt_fill_kernel, dim3(blocks), dim3(256), 0, st, dv_ws, 0.0f, nv);
    }
    hipLaunchKernelGGL(mt_full_dv_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, arg, grad_out, plane, n_ids, P * P,
                       dv_ws);
    const long n = plane * C;
    hipLaunchKernelGGL(mt_full_dist_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cur_chw, prev_chw,
                       (const float *)dv_ws, C, h, w, max_distance, grad_cur_chw, grad_prev_chw);
    return manet_check_launch("manet_local_match_full_backward_ordered_f32");
}

}  // extern "C"
