// kt_miobi.hip -- the kernels of kt_miobi_break and kt_pairs_score_topk
// (kt_miobi.cpp): the MIOBI edge score from the top-t
// eigenpairs on a pair list, the global argmin with the step applied on the
// device, and the column normalisation of the `paper` eigenvector update; and,
// at the end of the file, the two kernels of kt_miobi_make (§4.2f): the scores
// of a dense block of candidate pairs from LDS tiles, and its argmax and step;
// and the three of kt_miobi_break_node (§4.2g): the node score as a CSR row
// pass over V, its argmin and step, and V's column sums.
//
// V is n x 32 row-major in ORIGINAL numbering (t <= 32 live columns, the rest
// zero): one row is 256 bytes, so a half-wave with lane = column reads a row
// in one coalesced access.  No atomics; every sum has a fixed order, and the
// argmin is the minimum of a total order (score, key, list index), so neither
// depends on the grid or on how the pair list is stored.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "kt_launch.h"
#include "kt_wave.h"

namespace kt {

namespace {

typedef unsigned long long u64;

constexpr int kLd = kMiobiLd;
constexpr int kHalves = 8;                        // half-waves of a 256-thread workgroup
constexpr int kPer = kMiobiTilePairs / kHalves;   // pairs a half-wave has in flight per tile

// (s1, k1, i1) before (s2, k2, i2): the smaller score, exactly equal scores by
// the smaller key (max(i, j), min(i, j)) -- MATLAB's find(triu(A, 1)) order --
// then by the smaller list index (a list may name a pair twice).  i < 0: no
// candidate.  A NaN score loses to every number.
__device__ __forceinline__ bool before(double s1, u64 k1, int i1, double s2, u64 k2, int i2) {
    if (i1 < 0) return false;
    if (i2 < 0) return true;
    if (s1 != s2) return s1 < s2 || (s2 != s2 && s1 == s1);
    if (k1 != k2) return k1 < k2;
    return i1 < i2;
}

__device__ __forceinline__ u64 pair_key(int i, int j) {
    const unsigned hi = (unsigned)max(i, j), lo = (unsigned)min(i, j);
    return ((u64)hi << 32) | lo;
}

}  // namespace

// c[k] = exp(e[k]) for k < t, 0 for t <= k < 32
__global__ __launch_bounds__(64) void k_miobi_setc(int t, const double* __restrict__ e, double* __restrict__ c) {
    const int k = threadIdx.x;
    if (k < kLd) c[k] = k < t ? exp(e[k]) : 0.0;
}

hipError_t launch_miobi_setc(int t, const double* e, double* c, hipStream_t st) {
    if (t < 1 || t > kLd) return hipErrorInvalidValue;
    k_miobi_setc<<<1, 64, 0, st>>>(t, e, c);
    return hipGetLastError();
}

// score[p] = sum_{k < t} c[k] exp(sign V[pi[p], k] V[pj[p], k]) for the pairs
// whose alive byte is set (alive nullptr: all).  One half-wave per pair, lane =
// k; a workgroup takes tiles of 64 pairs, each half-wave kPer of them with all
// 2 kPer row reads issued before the first exp.  The t terms are added by the
// xor butterfly 16, 8, 4, 2, 1 (kt_wave.h), called by every lane of the wave
// whatever its pair: the order is fixed, the same inputs give the same bits.
// score (nullable) receives the live pairs' scores; part_*[blockIdx.x] the
// workgroup's first candidate in the order of before().  stop (nullable): a
// set word makes the launch a no-op.
__global__ __launch_bounds__(256) void k_miobi_score(int64_t npairs, int t, const double* __restrict__ V,
                                                     const double* __restrict__ c, const int* __restrict__ pi,
                                                     const int* __restrict__ pj,
                                                     const unsigned char* __restrict__ alive, double sign,
                                                     double* __restrict__ score, double* __restrict__ part_s,
                                                     u64* __restrict__ part_key, int* __restrict__ part_idx,
                                                     const int* __restrict__ stop) {
    if (stop && *stop) return;  // the same word for every thread
    __shared__ double red_s[kHalves];
    __shared__ u64 red_k[kHalves];
    __shared__ int red_i[kHalves];
    const int k = threadIdx.x & 31, h = threadIdx.x >> 5;
    const double ck = k < t ? c[k] : 0.0;
    double bs = 0.0;
    u64 bk = 0;
    int bi = -1;
    const int64_t ntiles = (npairs + kMiobiTilePairs - 1) / kMiobiTilePairs;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // wave-uniform trip count
        double a[kPer], b[kPer];
        int ii[kPer], jj[kPer];
        bool ok[kPer];
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int64_t p = tile * kMiobiTilePairs + u * kHalves + h;
            ok[u] = p < npairs && (!alive || alive[p]);
            ii[u] = jj[u] = 0;
            a[u] = b[u] = 0.0;
            if (ok[u]) {
                ii[u] = pi[p];
                jj[u] = pj[p];
                a[u] = V[(int64_t)ii[u] * kLd + k];
                b[u] = V[(int64_t)jj[u] * kLd + k];
            }
        }
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            double s = k < t ? ck * exp(sign * (a[u] * b[u])) : 0.0;
            s += shfl_xor_d(s, 16);
            s += shfl_xor_d(s, 8);
            s += shfl_xor_d(s, 4);
            s += shfl_xor_d(s, 2);
            s += shfl_xor_d(s, 1);
            if (ok[u]) {
                const int p = (int)(tile * kMiobiTilePairs + u * kHalves + h);
                if (score && k == 0) score[p] = s;
                const u64 key = pair_key(ii[u], jj[u]);
                if (before(s, key, p, bs, bk, bi)) {
                    bs = s;
                    bk = key;
                    bi = p;
                }
            }
        }
    }
    if (k == 0) {
        red_s[h] = bs;
        red_k[h] = bk;
        red_i[h] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < kHalves; ++q)
            if (before(red_s[q], red_k[q], red_i[q], bs, bk, bi)) {
                bs = red_s[q];
                bk = red_k[q];
                bi = red_i[q];
            }
        part_s[blockIdx.x] = bs;
        part_key[blockIdx.x] = bk;
        part_idx[blockIdx.x] = bi;
    }
}

int miobi_score_blocks(int64_t npairs, int max_blocks) {
    const int64_t ntiles = (npairs + kMiobiTilePairs - 1) / kMiobiTilePairs;
    const int cap = max_blocks > 0 ? std::min(max_blocks, kMiobiMaxBlocks) : kMiobiMaxBlocks;
    return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, cap));
}

hipError_t launch_miobi_score(int64_t npairs, int t, const double* V, const double* c, const int* pi, const int* pj,
                              const unsigned char* alive, double sign, double* score, int nblocks, double* part_s,
                              unsigned long long* part_key, int* part_idx, const int* stop, hipStream_t st) {
    if (npairs < 0 || npairs > INT32_MAX || t < 1 || t > kLd || nblocks < 1 || nblocks > kMiobiMaxBlocks)
        return hipErrorInvalidValue;
    k_miobi_score<<<nblocks, 256, 0, st>>>(npairs, t, V, c, pi, pj, alive, sign, score, part_s, part_key, part_idx,
                                           stop);
    return hipGetLastError();
}

// One workgroup: the minimum of the nparts workgroup candidates in the order
// of before(), then the step (MIOBIBreakEdge2.m:71-90, :140): with (i, j) the
// pair, a its weight (wt nullptr: 1) and s = state[0] the steps so far,
//   sel_i[s] = max(i, j), sel_j[s] = min(i, j), sel_score[s] = its score,
//   alive[pair] = 0, e[k] += -2 a V[i, k] V[j, k], c[k] = exp(e[k]),
//   track[(s + 1) 32 + k] = e[k]  (k < t),  state[0] = s + 1.
// paper != 0 also writes M (32 x 32 row-major) = I + S with S(r, c) =
// dH(r, c) / (e_c - e_r) for r != c < t, dH = -a (V[i, r] V[j, c] + V[j, r]
// V[i, c]), from e BEFORE the shift (:95-102, deltaV = V innerSum); 0 where the
// denominator is 0 or |e_c - e_r| <= gap_rel |e_0|; rows and columns >= t zero.
// No live candidate: state[1] = 1 (and M = I) and nothing else; a launch that
// finds state[1] set returns at once.
__global__ __launch_bounds__(256) void k_miobi_pick(int nparts, const double* __restrict__ part_s,
                                                    const u64* __restrict__ part_key,
                                                    const int* __restrict__ part_idx, int t, int paper,
                                                    double gap_rel, const double* __restrict__ V,
                                                    double* __restrict__ e, double* __restrict__ c,
                                                    const int* __restrict__ pi, const int* __restrict__ pj,
                                                    const double* __restrict__ wt, unsigned char* __restrict__ alive,
                                                    int* __restrict__ sel_i, int* __restrict__ sel_j,
                                                    double* __restrict__ sel_score, double* __restrict__ track,
                                                    double* __restrict__ M, int* __restrict__ state) {
    if (state[1]) return;
    __shared__ double ss[256];
    __shared__ u64 sk[256];
    __shared__ int si[256];
    __shared__ double su[kLd], sv[kLd], se[kLd];
    const int tid = threadIdx.x;
    const int step = state[0];
    double bs = 0.0;
    u64 bk = 0;
    int bi = -1;
    for (int q = tid; q < nparts; q += 256)
        if (before(part_s[q], part_key[q], part_idx[q], bs, bk, bi)) {
            bs = part_s[q];
            bk = part_key[q];
            bi = part_idx[q];
        }
    ss[tid] = bs;
    sk[tid] = bk;
    si[tid] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && before(ss[tid + w], sk[tid + w], si[tid + w], ss[tid], sk[tid], si[tid])) {
            ss[tid] = ss[tid + w];
            sk[tid] = sk[tid + w];
            si[tid] = si[tid + w];
        }
        __syncthreads();
    }
    const int idx = si[0];
    if (idx < 0) {
        if (tid == 0) state[1] = 1;
        if (paper)
            for (int q = tid; q < kLd * kLd; q += 256) M[q] = (q >> 5) == (q & 31) && (q & 31) < t ? 1.0 : 0.0;
        return;
    }
    const int i = pi[idx], j = pj[idx];
    const double a = wt ? wt[idx] : 1.0;
    if (tid < kLd) {
        const double u = tid < t ? V[(int64_t)i * kLd + tid] : 0.0;
        const double v = tid < t ? V[(int64_t)j * kLd + tid] : 0.0;
        const double eo = tid < t ? e[tid] : 0.0;
        su[tid] = u;
        sv[tid] = v;
        se[tid] = eo;
        if (tid < t) {
            const double en = eo + (-2.0 * a) * (u * v);
            e[tid] = en;
            c[tid] = exp(en);
            track[(int64_t)(step + 1) * kLd + tid] = en;
        }
    }
    if (tid == 0) {
        sel_i[step] = max(i, j);
        sel_j[step] = min(i, j);
        sel_score[step] = ss[0];
        alive[idx] = 0;
    }
    __syncthreads();  // every thread has read state[0]; su / sv / se are complete
    if (tid == 0) state[0] = step + 1;
    if (paper) {
        const double floor_gap = gap_rel * fabs(se[0]);
        for (int q = tid; q < kLd * kLd; q += 256) {
            const int r = q >> 5, cc = q & 31;
            double m = 0.0;
            if (r < t && cc < t) {
                if (r == cc) {
                    m = 1.0;
                } else {
                    const double d = se[cc] - se[r];
                    const double dh = -a * (su[r] * sv[cc] + sv[r] * su[cc]);
                    m = (d == 0.0 || fabs(d) <= floor_gap) ? 0.0 : dh / d;
                }
            }
            M[q] = m;
        }
    }
}

hipError_t launch_miobi_pick(int nparts, const double* part_s, const unsigned long long* part_key,
                             const int* part_idx, int t, int paper, double gap_rel, const double* V, double* e,
                             double* c, const int* pi, const int* pj, const double* wt, unsigned char* alive,
                             int* sel_i, int* sel_j, double* sel_score, double* track, double* M, int* state,
                             hipStream_t st) {
    if (nparts < 1 || nparts > kMiobiMaxBlocks || t < 1 || t > kLd || (paper && !M)) return hipErrorInvalidValue;
    k_miobi_pick<<<1, 256, 0, st>>>(nparts, part_s, part_key, part_idx, t, paper, gap_rel, V, e, c, pi, pj, wt, alive,
                                    sel_i, sel_j, sel_score, track, M, state);
    return hipGetLastError();
}

// The `paper` update's normalisation (MIOBIBreakEdge2.m:136-142): every column
// of V divided by its 2-norm, column 0 made non-negative.  k_miobi_colsq:
// workgroup b adds the squares of rows 8 b + (tid >> 5) + 8 gridDim.x q, q
// ascending, per thread, then the eight row groups in ascending order.
// k_miobi_scale adds the workgroups' partials in ascending order (every
// workgroup the same sum) and scales its rows; a zero column stays zero.
// Both return at once when state[1] is set.
__global__ __launch_bounds__(256) void k_miobi_colsq(int64_t n, const double* __restrict__ V,
                                                     double* __restrict__ part, const int* __restrict__ state) {
    if (state[1]) return;
    __shared__ double red[256];
    const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
    double acc = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 8 + g; r < n; r += (int64_t)gridDim.x * 8) {
        const double x = V[r * kLd + k];
        acc = fma(x, x, acc);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < kLd) {
        double s = 0.0;
        for (int q = 0; q < 8; ++q) s += red[q * 32 + threadIdx.x];
        part[(size_t)blockIdx.x * kLd + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void k_miobi_scale(int64_t n, int nparts, double* __restrict__ V,
                                                     const double* __restrict__ part,
                                                     const int* __restrict__ state) {
    if (state[1]) return;
    __shared__ double inv[kLd];
    if (threadIdx.x < kLd) {
        double s = 0.0;
        for (int q = 0; q < nparts; ++q) s += part[(size_t)q * kLd + threadIdx.x];
        inv[threadIdx.x] = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
    }
    __syncthreads();
    const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
    const double f = inv[k];
    for (int64_t r = (int64_t)blockIdx.x * 8 + g; r < n; r += (int64_t)gridDim.x * 8) {
        const double x = V[r * kLd + k] * f;
        V[r * kLd + k] = k == 0 ? fabs(x) : x;
    }
}

int miobi_norm_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, 256)); }

hipError_t launch_miobi_normalise(int64_t n, double* V, double* part, const int* state, hipStream_t st) {
    if (n <= 0) return hipErrorInvalidValue;
    const int nb = miobi_norm_blocks(n);
    k_miobi_colsq<<<nb, 256, 0, st>>>(n, V, part, state);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_miobi_scale<<<nb, 256, 0, st>>>(n, nb, V, part, state);
    return hipGetLastError();
}

// ---- make-edge (kt_miobi_make, MIOBIMakeEdge.m) -----------

namespace {

constexpr int kMT = kMiobiMakeTile;
// a panel is stored [k][rank] with the rank stride padded by one double: the
// transposing store (lane = k, stride kPanelLd doubles) then spreads over the
// banks, and the reads (consecutive ranks, or one address per wave row) stay
// conflict-free
constexpr int kPanelLd = kMT + 1;

// (s1, k1) before (s2, k2): the LARGER score, exactly equal scores by the
// smaller key (rank_a << 32) | rank_b -- the reference's first maximum in its
// a-then-b enumeration (MIOBIMakeEdge.m:72-80, :97).  ok = 0: no candidate.
// A NaN score loses to every number.
__device__ __forceinline__ bool make_before(double s1, u64 k1, int ok1, double s2, u64 k2, int ok2) {
    if (!ok1) return false;
    if (!ok2) return true;
    const bool n1 = s1 != s1, n2 = s2 != s2;
    if (n1 != n2) return n2;
    if (!n1 && s1 != s2) return s1 > s2;
    return k1 < k2;
}

}  // namespace

// The hot path: every non-adjacent pair of ranks a < b < m (m = state[3], the
// live candidate count) scored from the candidates' rows W,
//   score(a, b) = sum_{k < t} c[k] exp(2 W[a, k] W[b, k]),   k ascending.
// A workgroup takes 64 x 64 tiles (tile row <= tile column) of the rank square,
// grid-striding over the linear index L = tc (tc + 1) / 2 + tr.  The tile's two
// 64 x 32 panels are staged in LDS as [k][rank]; thread (tx, ty) owns the 4 x 4
// pairs (a0 + ty + 16 u, b0 + tx + 16 v): per k it reads 4 + 4 doubles (the b
// reads are 16 consecutive doubles per wave row, the a reads one address per
// wave row) and does 16 exp + 16 fma, one accumulator per pair.  No atomics and
// no cross-lane sums: a pair's bits depend on W, c and t only.  A pair is
// skipped on or below the diagonal, at or beyond m, or with its mask bit set
// (word tc of row a: one word per row per tile); a thread with no pair left
// skips the k loop, a tile at or beyond m is skipped by the whole workgroup.
// part_*[blockIdx.x]: the workgroup's first candidate under make_before().
__global__ __launch_bounds__(256) void k_miobi_make_score(int mcap, int t, const double* __restrict__ W,
                                                          const double* __restrict__ c,
                                                          const u64* __restrict__ mask,
                                                          const int* __restrict__ state, double* __restrict__ score,
                                                          double* __restrict__ part_s, u64* __restrict__ part_key,
                                                          int* __restrict__ part_ok) {
    if (state[1]) return;  // the same word for every thread
    __shared__ double sA[kLd * kPanelLd], sB[kLd * kPanelLd];
    __shared__ u64 sM[kMT];
    __shared__ double sc[kLd];
    __shared__ double red_s[256];
    __shared__ u64 red_k[256];
    __shared__ int red_o[256];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m = min(state[3], mcap);
    const int words = (mcap + kMT - 1) / kMT;  // tiles per side = mask words per row
    const int64_t ntiles = (int64_t)words * (words + 1) / 2;
    if (tid < kLd) sc[tid] = tid < t ? c[tid] : 0.0;
    double bs = 0.0;
    u64 bk = 0;
    int bo = 0;
    for (int64_t L = blockIdx.x; L < ntiles; L += gridDim.x) {  // workgroup-uniform trip count
        int tc = (int)((sqrt(8.0 * (double)L + 1.0) - 1.0) * 0.5);
        while ((int64_t)tc * (tc + 1) / 2 > L) --tc;
        while ((int64_t)(tc + 1) * (tc + 2) / 2 <= L) ++tc;
        const int tr = (int)(L - (int64_t)tc * (tc + 1) / 2);
        const int a0 = tr * kMT, b0 = tc * kMT;
        if (b0 >= m) continue;  // no pair with b < m: the whole workgroup skips
        __syncthreads();        // the previous tile's panels have been read
        for (int q = tid; q < kMT * kLd; q += 256) {
            const int row = q >> 5, kk = q & 31;
            sA[kk * kPanelLd + row] = a0 + row < mcap ? W[(int64_t)(a0 + row) * kLd + kk] : 0.0;
            sB[kk * kPanelLd + row] = b0 + row < mcap ? W[(int64_t)(b0 + row) * kLd + kk] : 0.0;
        }
        if (tid < kMT) sM[tid] = a0 + tid < mcap ? mask[(int64_t)(a0 + tid) * words + tc] : ~0ull;
        __syncthreads();
        unsigned live = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ra = a0 + ty + 16 * u;
            const u64 mw = sM[ty + 16 * u];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int rb = b0 + tx + 16 * v;
                if (ra < rb && rb < m && !((mw >> (tx + 16 * v)) & 1ull)) live |= 1u << (u * 4 + v);
            }
        }
        if (live) {
            double acc[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
            for (int kk = 0; kk < t; ++kk) {
                const double ck = sc[kk];
                double a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u] = sA[kk * kPanelLd + ty + 16 * u];
#pragma unroll
                for (int v = 0; v < 4; ++v) b[v] = sB[kk * kPanelLd + tx + 16 * v];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] = fma(ck, exp(2.0 * (a[u] * b[v])), acc[u][v]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (live & (1u << (u * 4 + v))) {
                        const int ra = a0 + ty + 16 * u, rb = b0 + tx + 16 * v;
                        const double s = acc[u][v];
                        const u64 key = ((u64)(unsigned)ra << 32) | (unsigned)rb;
                        if (score) score[(int64_t)ra * mcap + rb] = s;
                        if (make_before(s, key, 1, bs, bk, bo)) {
                            bs = s;
                            bk = key;
                            bo = 1;
                        }
                    }
        }
    }
    red_s[tid] = bs;
    red_k[tid] = bk;
    red_o[tid] = bo;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && make_before(red_s[tid + w], red_k[tid + w], red_o[tid + w], red_s[tid], red_k[tid], red_o[tid])) {
            red_s[tid] = red_s[tid + w];
            red_k[tid] = red_k[tid + w];
            red_o[tid] = red_o[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part_s[blockIdx.x] = red_s[0];
        part_key[blockIdx.x] = red_k[0];
        part_ok[blockIdx.x] = red_o[0];
    }
}

int miobi_make_blocks(int mcap, int max_blocks) {
    const int64_t side = (mcap + kMT - 1) / kMT, ntiles = side * (side + 1) / 2;
    const int cap = max_blocks > 0 ? std::min(max_blocks, kMiobiMaxBlocks) : kMiobiMaxBlocks;
    return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, cap));
}

hipError_t launch_miobi_make_score(int mcap, int t, const double* W, const double* c,
                                   const unsigned long long* mask, const int* state, double* score, int nblocks,
                                   double* part_s, unsigned long long* part_key, int* part_ok, hipStream_t st) {
    if (mcap < 2 || t < 1 || t > kLd || nblocks < 1 || nblocks > kMiobiMaxBlocks) return hipErrorInvalidValue;
    k_miobi_make_score<<<nblocks, 256, 0, st>>>(mcap, t, W, c, mask, state, score, part_s, part_key, part_ok);
    return hipGetLastError();
}

// One workgroup: the first of the nparts workgroup candidates under
// make_before(), then the step (MIOBIMakeEdge.m:97-118): with (a, b) the ranks,
// (i, j) = (node[a], node[b]) and s = state[0] the steps so far,
//   sel_i[s] = max(i, j), sel_j[s] = min(i, j), sel_score[s] = the score,
//   cand_m[s] = state[3], the m this step scored with,
//   mask bits (a, b) and (b, a) set,
//   e[k] += 2 W[a, k] W[b, k], c[k] = exp(e[k]), track[(s + 1) 32 + k] = e[k]  (k < t),
//   deg[a]++, deg[b]++, state[2] = maxdeg = max(maxdeg, deg[a], deg[b]),
//   state[3] = min(maxdeg + k, n) (<= mcap by the driver's construction, and
//   held to it), state[0] = s + 1.
// No candidate: state[1] = 1 and nothing else; a launch that finds state[1] set
// returns at once.
__global__ __launch_bounds__(256) void k_miobi_make_pick(int nparts, const double* __restrict__ part_s,
                                                         const u64* __restrict__ part_key,
                                                         const int* __restrict__ part_ok, int mcap, int t, int k,
                                                         int n, const double* __restrict__ W,
                                                         const int* __restrict__ node, double* __restrict__ e,
                                                         double* __restrict__ c, u64* __restrict__ mask,
                                                         int* __restrict__ deg, int* __restrict__ sel_i,
                                                         int* __restrict__ sel_j, double* __restrict__ sel_score,
                                                         double* __restrict__ track, int* __restrict__ cand_m,
                                                         int* __restrict__ state) {
    if (state[1]) return;
    __shared__ double ss[256];
    __shared__ u64 sk[256];
    __shared__ int so[256];
    const int tid = threadIdx.x;
    const int step = state[0], maxdeg = state[2], m_used = state[3];
    double bs = 0.0;
    u64 bk = 0;
    int bo = 0;
    for (int q = tid; q < nparts; q += 256)
        if (make_before(part_s[q], part_key[q], part_ok[q], bs, bk, bo)) {
            bs = part_s[q];
            bk = part_key[q];
            bo = 1;
        }
    ss[tid] = bs;
    sk[tid] = bk;
    so[tid] = bo;
    __syncthreads();  // every thread has read the state words
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && make_before(ss[tid + w], sk[tid + w], so[tid + w], ss[tid], sk[tid], so[tid])) {
            ss[tid] = ss[tid + w];
            sk[tid] = sk[tid + w];
            so[tid] = so[tid + w];
        }
        __syncthreads();
    }
    const int a = (int)(sk[0] >> 32), b = (int)(sk[0] & 0xffffffffull);
    if (!so[0] || a < 0 || a >= b || b >= mcap) {  // (a key outside the rank square cannot come from the score kernel)
        if (tid == 0) state[1] = 1;
        return;
    }
    if (tid < t) {
        const double en = e[tid] + 2.0 * (W[(int64_t)a * kLd + tid] * W[(int64_t)b * kLd + tid]);
        e[tid] = en;
        c[tid] = exp(en);
        track[(int64_t)(step + 1) * kLd + tid] = en;
    }
    if (tid == 0) {
        const int words = (mcap + kMT - 1) / kMT;
        const int i = node[a], j = node[b];
        sel_i[step] = max(i, j);
        sel_j[step] = min(i, j);
        sel_score[step] = ss[0];
        cand_m[step] = m_used;
        mask[(int64_t)a * words + (b >> 6)] |= 1ull << (b & 63);
        mask[(int64_t)b * words + (a >> 6)] |= 1ull << (a & 63);
        const int da = deg[a] + 1, db = deg[b] + 1;
        deg[a] = da;
        deg[b] = db;
        const int md = max(maxdeg, max(da, db));
        state[2] = md;
        state[3] = (int)min((int64_t)mcap, min((int64_t)md + k, (int64_t)n));
        state[0] = step + 1;
    }
}

hipError_t launch_miobi_make_pick(int nparts, const double* part_s, const unsigned long long* part_key,
                                  const int* part_ok, int mcap, int t, int k, int n, const double* W,
                                  const int* node, double* e, double* c, unsigned long long* mask, int* deg,
                                  int* sel_i, int* sel_j, double* sel_score, double* track, int* cand_m,
                                  int* state, hipStream_t st) {
    if (nparts < 1 || nparts > kMiobiMaxBlocks || mcap < 2 || t < 1 || t > kLd || k < 0 || n < mcap)
        return hipErrorInvalidValue;
    k_miobi_make_pick<<<1, 256, 0, st>>>(nparts, part_s, part_key, part_ok, mcap, t, k, n, W, node, e, c, mask, deg,
                                         sel_i, sel_j, sel_score, track, cand_m, state);
    return hipGetLastError();
}

// ---- break-node (kt_miobi_break_node, MIOBIBreakNode.m) ----

namespace {

constexpr int kNB = kMiobiNodeBatch;
constexpr int kNodeTrip = kHalves * kMiobiNodeChunk;  // entries of a split row a workgroup takes per trip

// (s1, i1) before (s2, i2): the smaller score, exactly equal scores by the
// smaller node index -- the first minimum of [~, minIndex] = min(score)
// (MIOBIBreakNode.m:204).  i < 0: no candidate.  A NaN score loses to every number.
__device__ __forceinline__ bool node_before(double s1, int i1, double s2, int i2) {
    if (i1 < 0) return false;
    if (i2 < 0) return true;
    if (s1 != s2) return s1 < s2 || (s2 != s2 && s1 == s1);
    return i1 < i2;
}

// w += V[col[j], k] over the entries j of [beg, end) (beg < end) whose node is
// alive, j ascending; cnt += their number.  kNB row reads are issued before the
// first add; the loads are unconditional (an index past the end is clamped to
// the last entry, a dead node's row is read and dropped), so none waits for a
// branch.
__device__ __forceinline__ void node_gather(const double* __restrict__ V, const int* __restrict__ col,
                                            const unsigned char* __restrict__ alive, int beg, int end, int k,
                                            double& w, int& cnt) {
    for (int j = beg; j < end; j += kNB) {
        double x[kNB];
        bool on[kNB];
#pragma unroll
        for (int u = 0; u < kNB; ++u) {
            const int cidx = col[min(j + u, end - 1)];
            on[u] = j + u < end && alive[cidx] != 0;
            x[u] = V[(int64_t)cidx * kLd + k];
        }
#pragma unroll
        for (int u = 0; u < kNB; ++u) {
            w += on[u] ? x[u] : 0.0;
            cnt += on[u] ? 1 : 0;
        }
    }
}

// half-wave h's share of the split row [beg, end): the chunks of
// kMiobiNodeChunk entries numbered h, h + 8, h + 16, ..., ascending
__device__ __forceinline__ void node_gather_split(const double* __restrict__ V, const int* __restrict__ col,
                                                  const unsigned char* __restrict__ alive, int beg, int end, int h,
                                                  int k, double& w, int& cnt) {
    for (int64_t c0 = (int64_t)beg + (int64_t)h * kMiobiNodeChunk; c0 < end; c0 += kNodeTrip)
        node_gather(V, col, alive, (int)c0, (int)min(c0 + kMiobiNodeChunk, (int64_t)end), k, w, cnt);
}

__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

}  // namespace

// The node score of MIOBIBreakNode.m:186-202 on the CSR (rowptr, col; unit
// weights, zero diagonal) of the window's matrix, with alive[] the nodes not
// yet removed in it: for a live row r
//   W[r, k] = sum_{j in row r, alive[col j]} V[col j, k]     (j ascending)
//   score[r] = sum_{k < t} c[k] exp(-2 V[r, k] W[r, k])
// with lane = k and the t terms added by the xor butterfly 16, 8, 4, 2, 1.  A
// dead row, and a row with no live neighbour, scores +Inf and is no candidate.
// Rows of at most kMiobiNodeLong entries: one half-wave per row, workgroup b
// takes rows 8 b + h + 8 gridDim.x q.  Longer rows (long_rows, n_long of them,
// every row longer than kMiobiNodeLong and no other): one workgroup per row,
// half-wave h the chunks h, h + 8, ... of kMiobiNodeChunk entries, the eight
// partial sums added in the order h = 0..7.  A row's bits depend on V, c, t,
// the row and alive only -- not on the grid.  score (nullable) receives every
// row's score; part_*[blockIdx.x] the workgroup's first candidate under
// node_before() and its live degree.  state (nullable): a set state[1] (stop)
// or state[3] (window end) makes the launch a no-op.
__global__ __launch_bounds__(256) void k_miobi_node_score(int n, int t, const double* __restrict__ V,
                                                          const double* __restrict__ c,
                                                          const int* __restrict__ rowptr,
                                                          const int* __restrict__ col,
                                                          const unsigned char* __restrict__ alive,
                                                          const int* __restrict__ long_rows, int n_long,
                                                          double* __restrict__ score, double* __restrict__ part_s,
                                                          int* __restrict__ part_node, int* __restrict__ part_deg,
                                                          const int* __restrict__ state) {
    if (state && (state[1] || state[3])) return;  // the same words for every thread
    __shared__ double sW[kHalves][kLd];
    __shared__ int sN[kHalves];
    __shared__ double red_s[kHalves];
    __shared__ int red_i[kHalves], red_d[kHalves];
    const int k = threadIdx.x & 31, h = threadIdx.x >> 5;
    const double ck = k < t ? c[k] : 0.0;
    const double inf = pos_inf();
    double bs = 0.0;
    int bi = -1, bd = 0;
    for (int64_t rb = (int64_t)blockIdx.x * kHalves; rb < n; rb += (int64_t)gridDim.x * kHalves) {  // wave-uniform
        const int64_t r = rb + h;
        double w = 0.0, v = 0.0;
        int cnt = 0;
        bool own = false;
        if (r < n) {
            const int beg = rowptr[r], end = rowptr[r + 1];
            own = end - beg <= kMiobiNodeLong;
            if (own && end > beg && alive[r]) {
                v = V[r * kLd + k];
                node_gather(V, col, alive, beg, end, k, w, cnt);
            }
        }
        double s = k < t ? ck * exp(-2.0 * (v * w)) : 0.0;
        s += shfl_xor_d(s, 16);
        s += shfl_xor_d(s, 8);
        s += shfl_xor_d(s, 4);
        s += shfl_xor_d(s, 2);
        s += shfl_xor_d(s, 1);
        if (own) {
            if (cnt == 0) s = inf;
            if (score && k == 0) score[r] = s;
            if (s != inf && node_before(s, (int)r, bs, bi)) {
                bs = s;
                bi = (int)r;
                bd = cnt;
            }
        }
    }
    for (int q = blockIdx.x; q < n_long; q += gridDim.x) {  // workgroup-uniform trip count
        const int r = long_rows[q];
        const int beg = rowptr[r], end = rowptr[r + 1];
        const bool live = alive[r] != 0;
        double w = 0.0;
        int cnt = 0;
        if (live) node_gather_split(V, col, alive, beg, end, h, k, w, cnt);
        sW[h][k] = w;
        if (k == 0) sN[h] = cnt;
        __syncthreads();
        w = 0.0;
        cnt = 0;
#pragma unroll
        for (int g = 0; g < kHalves; ++g) {
            w += sW[g][k];
            cnt += sN[g];
        }
        __syncthreads();  // the next trip writes sW / sN again
        const double v = live ? V[(int64_t)r * kLd + k] : 0.0;
        double s = k < t ? ck * exp(-2.0 * (v * w)) : 0.0;
        s += shfl_xor_d(s, 16);
        s += shfl_xor_d(s, 8);
        s += shfl_xor_d(s, 4);
        s += shfl_xor_d(s, 2);
        s += shfl_xor_d(s, 1);
        if (cnt == 0) s = inf;
        if (h == 0) {
            if (score && k == 0) score[r] = s;
            if (s != inf && node_before(s, r, bs, bi)) {
                bs = s;
                bi = r;
                bd = cnt;
            }
        }
    }
    if (k == 0) {
        red_s[h] = bs;
        red_i[h] = bi;
        red_d[h] = bd;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 1; q < kHalves; ++q)
            if (node_before(red_s[q], red_i[q], bs, bi)) {
                bs = red_s[q];
                bi = red_i[q];
                bd = red_d[q];
            }
        part_s[blockIdx.x] = bs;
        part_node[blockIdx.x] = bi;
        part_deg[blockIdx.x] = bd;
    }
}

int miobi_node_blocks(int64_t n, int max_blocks) {
    const int cap = max_blocks > 0 ? std::min(max_blocks, kMiobiMaxBlocks) : kMiobiMaxBlocks;
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + kHalves - 1) / kHalves, cap));
}

hipError_t launch_miobi_node_score(int64_t n, int t, const double* V, const double* c, const int* rowptr,
                                   const int* col, const unsigned char* alive, const int* long_rows, int n_long,
                                   double* score, int nblocks, double* part_s, int* part_node, int* part_deg,
                                   const int* state, hipStream_t st) {
    if (n < 1 || n > INT32_MAX || t < 1 || t > kLd || nblocks < 1 || nblocks > kMiobiMaxBlocks || n_long < 0 ||
        n_long > n || (n_long > 0 && !long_rows))
        return hipErrorInvalidValue;
    k_miobi_node_score<<<nblocks, 256, 0, st>>>((int)n, t, V, c, rowptr, col, alive, long_rows, n_long, score, part_s,
                                                part_node, part_deg, state);
    return hipGetLastError();
}

// One workgroup: the minimum of the nparts workgroup candidates under
// node_before(), then the step (MIOBIBreakNode.m:204-223, :283-295): with r the
// node, d its live degree and s = state[0] the steps so far,
//   sel_node[s] = r, sel_score[s] = its score, sel_deg[s] = d, alive[r] = 0,
//   e[k] += dE[k], c[k] = exp(e[k]), track[(s + 1) 32 + k] = e[k]  (k < t),
//   shift 0 (reference): dE[k] = -(2 V[r, k] colsum[k] - V[r, k]^2), the
//     diagonal of V' deltaA V with deltaA's WHOLE row and column r at -1 (:216-217),
//   shift 1 (first order): dE[k] = -2 V[r, k] W[r, k], W over the live
//     neighbours of r, gathered here in the score kernel's order,
//   state[2] = acc += 2 d (:208, :283); with refresh > 0 and acc >= refresh:
//   acc %= refresh and state[3] = 1, the window's end (:286-292); refresh <= 0
//   leaves state[2] alone;  state[0] = s + 1.
// No candidate (every score +Inf): state[1] = 1 and nothing else.  A launch
// that finds state[1] or state[3] set returns at once.
__global__ __launch_bounds__(256) void k_miobi_node_pick(int nparts, const double* __restrict__ part_s,
                                                         const int* __restrict__ part_node,
                                                         const int* __restrict__ part_deg, int t, int shift,
                                                         int refresh, const double* __restrict__ V,
                                                         const int* __restrict__ rowptr,
                                                         const int* __restrict__ col, unsigned char* alive,
                                                         double* __restrict__ e, double* __restrict__ c,
                                                         const double* __restrict__ colsum,
                                                         int* __restrict__ sel_node, double* __restrict__ sel_score,
                                                         int* __restrict__ sel_deg, double* __restrict__ track,
                                                         int* __restrict__ state) {
    if (state[1] || state[3]) return;
    __shared__ double ss[256];
    __shared__ int si[256], sd[256];
    __shared__ double sW[kHalves][kLd];
    const int tid = threadIdx.x, k = tid & 31, h = tid >> 5;
    const int step = state[0], acc = state[2];
    double bs = 0.0;
    int bi = -1, bd = 0;
    for (int q = tid; q < nparts; q += 256)
        if (node_before(part_s[q], part_node[q], bs, bi)) {
            bs = part_s[q];
            bi = part_node[q];
            bd = part_deg[q];
        }
    ss[tid] = bs;
    si[tid] = bi;
    sd[tid] = bd;
    __syncthreads();  // every thread has read the state words
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w && node_before(ss[tid + w], si[tid + w], ss[tid], si[tid])) {
            ss[tid] = ss[tid + w];
            si[tid] = si[tid + w];
            sd[tid] = sd[tid + w];
        }
        __syncthreads();
    }
    const int r = si[0], deg = sd[0];
    if (r < 0) {
        if (tid == 0) state[1] = 1;
        return;
    }
    double w = 0.0;
    if (shift) {  // the same value for every thread
        const int beg = rowptr[r], end = rowptr[r + 1];
        int cnt = 0;
        if (end - beg > kMiobiNodeLong) node_gather_split(V, col, alive, beg, end, h, k, w, cnt);
        else if (h == 0 && end > beg) node_gather(V, col, alive, beg, end, k, w, cnt);
        sW[h][k] = w;
        __syncthreads();  // the gathers have read alive[]
        w = 0.0;
#pragma unroll
        for (int g = 0; g < kHalves; ++g) w += sW[g][k];
    }
    if (tid < t) {
        const double v = V[(int64_t)r * kLd + tid];
        const double de = shift ? -2.0 * (v * w) : -(2.0 * v * colsum[tid] - v * v);
        const double en = e[tid] + de;
        e[tid] = en;
        c[tid] = exp(en);
        track[(int64_t)(step + 1) * kLd + tid] = en;
    }
    if (tid == 0) {
        sel_node[step] = r;
        sel_score[step] = ss[0];
        sel_deg[step] = deg;
        alive[r] = 0;
        if (refresh > 0) {
            long long a = (long long)acc + 2LL * deg;
            if (a >= refresh) {
                a %= refresh;
                state[3] = 1;
            }
            state[2] = (int)a;
        }
        state[0] = step + 1;
    }
}

hipError_t launch_miobi_node_pick(int nparts, const double* part_s, const int* part_node, const int* part_deg, int t,
                                  int shift, int refresh, const double* V, const int* rowptr, const int* col,
                                  unsigned char* alive, double* e, double* c, const double* colsum, int* sel_node,
                                  double* sel_score, int* sel_deg, double* track, int* state, hipStream_t st) {
    if (nparts < 1 || nparts > kMiobiMaxBlocks || t < 1 || t > kLd || (shift != 0 && shift != 1) ||
        (shift == 0 && !colsum))
        return hipErrorInvalidValue;
    k_miobi_node_pick<<<1, 256, 0, st>>>(nparts, part_s, part_node, part_deg, t, shift, refresh, V, rowptr, col, alive,
                                         e, c, colsum, sel_node, sel_score, sel_deg, track, state);
    return hipGetLastError();
}

// s[k] = sum_r V[r, k] over all n rows, in a fixed order (k_miobi_colsq's shape
// without the square): workgroup b adds rows 8 b + (tid >> 5) + 8 gridDim.x q,
// q ascending, per thread, then its eight row groups in ascending order;
// k_miobi_colsum_fin adds the workgroups' partials in ascending order.
__global__ __launch_bounds__(256) void k_miobi_colsum(int64_t n, const double* __restrict__ V,
                                                      double* __restrict__ part) {
    __shared__ double red[256];
    const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
    double acc = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 8 + g; r < n; r += (int64_t)gridDim.x * 8) acc += V[r * kLd + k];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < kLd) {
        double s = 0.0;
        for (int q = 0; q < 8; ++q) s += red[q * 32 + threadIdx.x];
        part[(size_t)blockIdx.x * kLd + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void k_miobi_colsum_fin(int nparts, const double* __restrict__ part,
                                                         double* __restrict__ s) {
    if (threadIdx.x < kLd) {
        double a = 0.0;
        for (int q = 0; q < nparts; ++q) a += part[(size_t)q * kLd + threadIdx.x];
        s[threadIdx.x] = a;
    }
}

hipError_t launch_miobi_colsum(int64_t n, const double* V, double* part, double* s, hipStream_t st) {
    if (n <= 0) return hipErrorInvalidValue;
    const int nb = miobi_norm_blocks(n);
    k_miobi_colsum<<<nb, 256, 0, st>>>(n, V, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_miobi_colsum_fin<<<1, 64, 0, st>>>(nb, part, s);
    return hipGetLastError();
}

}  // namespace kt
