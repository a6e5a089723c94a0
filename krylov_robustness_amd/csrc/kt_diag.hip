// kt_diag.hip -- streaming kernels of the deflated stochastic estimator of
// diag f(A) (kt_diag_fun.cpp) and of its off-diagonal twin on
// a pair list (kt_entries_fun, §4.2c: k_entries_accumulate, k_entries_e0).
//
// Every kernel walks an n x P row-major block (P probes of one sweep, rows in
// the hubs-first order of the probe sweep) with LPR = max(P / 2, 1) lanes per
// row and VEC = min(P, 2) doubles per lane, so a row of 16 probes is eight
// 16-byte accesses and a wave covers 1 KiB of every block it reads.  A lane
// keeps its probe pair for the whole grid-stride loop.  The deflation block Q
// is n x KP row-major (KP = 1, 4 or 16 >= kdef, the padding columns zero).
//
// Reductions are fixed-order: over a row's probes by an xor butterfly among
// the row's lanes, over rows by a butterfly among the lanes of a probe pair,
// the four waves through LDS, the workgroups' partials by k_diag_sum_parts (a
// wave per value, strided lanes then a butterfly).  No atomics: a row of
// dsum / dsum2 is added to by the one lane that owns the row in that launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "kt_launch.h"

namespace kt {

namespace {

constexpr int kDiagBlock = 256;

__device__ __forceinline__ uint64_t diag_sm64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

template <int P> struct DiagGeo {
    static constexpr int VEC = P >= 2 ? 2 : 1;
    static constexpr int LPR = P / VEC;              // lanes per row
    static constexpr int RPB = kDiagBlock / LPR;     // rows per workgroup and loop trip
};

using dbl2 = __attribute__((ext_vector_type(2))) double;

template <int VEC> __device__ __forceinline__ void ld_vec(const double* p, double* v) {
    if constexpr (VEC == 2) {
        const dbl2 t = *reinterpret_cast<const dbl2*>(p);
        v[0] = t[0];
        v[1] = t[1];
    } else {
        v[0] = *p;
    }
}
template <int VEC> __device__ __forceinline__ void ld_vec_nt(const double* p, double* v) {
    if constexpr (VEC == 2) {
        const dbl2 t = __builtin_nontemporal_load(reinterpret_cast<const dbl2*>(p));
        v[0] = t[0];
        v[1] = t[1];
    } else {
        v[0] = __builtin_nontemporal_load(p);
    }
}
template <int VEC> __device__ __forceinline__ void st_vec(double* p, const double* v) {
    if constexpr (VEC == 2) {
        dbl2 t = {v[0], v[1]};
        *reinterpret_cast<dbl2*>(p) = t;
    } else {
        *p = v[0];
    }
}

// the lane's probe keys (the stream of k_rademacher: probe base + p of row i
// is the sign bit of sm64(key_p + i), i the ORIGINAL row index)
template <int P> __device__ __forceinline__ void probe_keys(uint64_t seed, int64_t base, int sub, uint64_t* key) {
    using G = DiagGeo<P>;
#pragma unroll
    for (int v = 0; v < G::VEC; ++v) key[v] = diag_sm64(diag_sm64(seed) + (uint64_t)(base + sub * G::VEC + v));
}

__device__ __forceinline__ double probe_sign(uint64_t key, uint64_t i) {
    return (diag_sm64(key + i) >> 63) ? -1.0 : 1.0;
}

// Sum of acc[KP][VEC] over the workgroup's rows -> part[blockIdx][b * P + p].
// scratch: 4 * KP * P doubles of LDS.
template <int P, int KP>
__device__ __forceinline__ void block_sum_rows(double (&acc)[KP > 0 ? KP : 1][DiagGeo<P>::VEC], int sub,
                                               double* scratch, double* __restrict__ part) {
    using G = DiagGeo<P>;
    constexpr int KK = KP > 0 ? KP : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int b = 0; b < KK; ++b)
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) {
            double s = acc[b][v];
#pragma unroll
            for (int off = G::LPR; off < 64; off <<= 1) s += __shfl_xor(s, off);
            if (lane < G::LPR) scratch[(wave * KK + b) * P + sub * G::VEC + v] = s;
        }
    __syncthreads();
    for (int i = threadIdx.x; i < KK * P; i += kDiagBlock) {
        double s = scratch[i];
#pragma unroll
        for (int w = 1; w < kDiagBlock / 64; ++w) s += scratch[w * KK * P + i];
        part[(size_t)blockIdx.x * KK * P + i] = s;
    }
}

// Partials of Q' z for the sweep's probes (columns >= nc are zero columns).
template <int P, int KP>
__global__ __launch_bounds__(kDiagBlock) void k_diag_qtz(int n, uint64_t seed, int64_t base, int nc,
                                                         const int* __restrict__ perm,
                                                         const double* __restrict__ Q,
                                                         double* __restrict__ part) {
    using G = DiagGeo<P>;
    __shared__ double scratch[4 * KP * P];
    const int sub = threadIdx.x % G::LPR;
    uint64_t key[G::VEC];
    probe_keys<P>(seed, base, sub, key);
    double acc[KP][G::VEC];
#pragma unroll
    for (int b = 0; b < KP; ++b)
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) acc[b][v] = 0.0;
    for (int64_t rb = (int64_t)blockIdx.x * G::RPB; rb < n; rb += (int64_t)gridDim.x * G::RPB) {
        const int64_t r = rb + threadIdx.x / G::LPR;
        if (r < n) {
            const uint64_t i = perm ? (uint64_t)perm[r] : (uint64_t)r;
            double z[G::VEC];
#pragma unroll
            for (int v = 0; v < G::VEC; ++v) z[v] = (sub * G::VEC + v < nc) ? probe_sign(key[v], i) : 0.0;
            const double* q = Q + r * KP;
#pragma unroll
            for (int b = 0; b < KP; ++b) {
                const double qb = q[b];
#pragma unroll
                for (int v = 0; v < G::VEC; ++v) acc[b][v] = fma(qb, z[v], acc[b][v]);
            }
        }
    }
    block_sum_rows<P, KP>(acc, sub, scratch, part);
}

// out[i] = sum over the workgroups' partials, in a fixed order: a wave per
// output, lane l adds partials l, l + 64, ... in order, then an xor butterfly
__global__ __launch_bounds__(256) void k_diag_sum_parts(int nparts, int K, const double* __restrict__ part,
                                                        double* __restrict__ out) {
    const int i = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= K) return;  // wave-uniform
    double s = 0.0;
    for (int g = lane; g < nparts; g += 64) s += part[(size_t)g * K + i];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[i] = s;
}

// z' = z - Q c into the sweep's dense start block X, and the partials of the
// columns' squared norms (KP = 0: nothing is subtracted).
template <int P, int KP>
__global__ __launch_bounds__(kDiagBlock) void k_diag_start(int n, uint64_t seed, int64_t base, int nc,
                                                           const int* __restrict__ perm,
                                                           const double* __restrict__ Q,
                                                           const double* __restrict__ c,
                                                           double* __restrict__ X, double* __restrict__ part) {
    using G = DiagGeo<P>;
    __shared__ double scratch[4 * P];
    const int sub = threadIdx.x % G::LPR;
    uint64_t key[G::VEC];
    probe_keys<P>(seed, base, sub, key);
    double cc[KP > 0 ? KP : 1][G::VEC];
#pragma unroll
    for (int b = 0; b < KP; ++b)
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) cc[b][v] = c[b * P + sub * G::VEC + v];
    double acc[1][G::VEC];
#pragma unroll
    for (int v = 0; v < G::VEC; ++v) acc[0][v] = 0.0;
    for (int64_t rb = (int64_t)blockIdx.x * G::RPB; rb < n; rb += (int64_t)gridDim.x * G::RPB) {
        const int64_t r = rb + threadIdx.x / G::LPR;
        if (r < n) {
            const uint64_t i = perm ? (uint64_t)perm[r] : (uint64_t)r;
            double z[G::VEC];
#pragma unroll
            for (int v = 0; v < G::VEC; ++v) z[v] = (sub * G::VEC + v < nc) ? probe_sign(key[v], i) : 0.0;
            if constexpr (KP > 0) {
                const double* q = Q + r * KP;
                double s[G::VEC];
#pragma unroll
                for (int v = 0; v < G::VEC; ++v) s[v] = 0.0;
#pragma unroll
                for (int b = 0; b < KP; ++b) {
                    const double qb = q[b];
#pragma unroll
                    for (int v = 0; v < G::VEC; ++v) s[v] = fma(qb, cc[b][v], s[v]);
                }
#pragma unroll
                for (int v = 0; v < G::VEC; ++v) z[v] -= s[v];
            }
            st_vec<G::VEC>(X + r * P + sub * G::VEC, z);
#pragma unroll
            for (int v = 0; v < G::VEC; ++v) acc[0][v] = fma(z[v], z[v], acc[0][v]);
        }
    }
    block_sum_rows<P, 0>(acc, sub, scratch, part);
}

// the row's sum over its probes (every lane of the row gets it)
template <int P> __device__ __forceinline__ double row_sum(const double* t) {
    using G = DiagGeo<P>;
    double s = t[0];
    if constexpr (G::VEC == 2) s += t[1];
#pragma unroll
    for (int off = 1; off < G::LPR; off <<= 1) s += __shfl_xor(s, off);
    return s;
}

// One pass over the Lanczos basis (slot j at V + j * sstride, n x P):
//   y[r, p] = sum_{j < depth[p]} W[j, p] V_j[r, p]
// in slot order; slots at or past a column's cut are loaded only as the
// other half of a 16-byte pair and never enter a sum, slots at or past mdepth
// (the largest cut) are not read.  KP = 0: t = z .* y is reduced over the
// row's probes and added to dsum / dsum2 (y is never stored).  KP > 0: y goes
// to Y and the partials of Q' y to part.  YONLY (KP = 0, kt_entries_fun): y
// goes to Y and nothing else is formed.
// LDS (dynamic): W (m x P), then the 4 * KP * P reduction scratch.
template <int P, int KP, bool YONLY = false>
__global__ __launch_bounds__(kDiagBlock) void k_diag_combine(int n, int m, int mdepth, const double* __restrict__ V,
                                                             int64_t sstride, const double* __restrict__ W,
                                                             const int* __restrict__ depth, uint64_t seed,
                                                             int64_t base, const int* __restrict__ perm,
                                                             const double* __restrict__ Q, double* __restrict__ Y,
                                                             double* __restrict__ part, double* __restrict__ dsum,
                                                             double* __restrict__ dsum2) {
    using G = DiagGeo<P>;
    extern __shared__ double smem[];
    double* sW = smem;
    double* scratch = smem + (size_t)m * P;
    for (int i = threadIdx.x; i < mdepth * P; i += kDiagBlock) sW[i] = W[i];
    __syncthreads();
    const int sub = threadIdx.x % G::LPR;
    int dep[G::VEC];
#pragma unroll
    for (int v = 0; v < G::VEC; ++v) dep[v] = depth[sub * G::VEC + v];
    uint64_t key[G::VEC];
    probe_keys<P>(seed, base, sub, key);
    double acc[KP > 0 ? KP : 1][G::VEC];
#pragma unroll
    for (int b = 0; b < (KP > 0 ? KP : 1); ++b)
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) acc[b][v] = 0.0;
    for (int64_t rb = (int64_t)blockIdx.x * G::RPB; rb < n; rb += (int64_t)gridDim.x * G::RPB) {
        const int64_t r = rb + threadIdx.x / G::LPR;
        const bool live = r < n;
        double y[G::VEC];
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) y[v] = 0.0;
        if (live) {
            const double* u = V + r * P + sub * G::VEC;
            // a group's loads issue together, then the fma chain in slot order
            constexpr int kG = 8;
            for (int j0 = 0; j0 < mdepth; j0 += kG) {
                double x[kG][G::VEC];
#pragma unroll
                for (int g = 0; g < kG; ++g)
                    if (j0 + g < mdepth) ld_vec_nt<G::VEC>(u + (int64_t)(j0 + g) * sstride, x[g]);
#pragma unroll
                for (int g = 0; g < kG; ++g)
                    if (j0 + g < mdepth) {
#pragma unroll
                        for (int v = 0; v < G::VEC; ++v)
                            if (j0 + g < dep[v]) y[v] = fma(sW[(j0 + g) * P + sub * G::VEC + v], x[g][v], y[v]);
                    }
            }
        }
        if constexpr (YONLY) {
            if (live) st_vec<G::VEC>(Y + r * P + sub * G::VEC, y);
        } else if constexpr (KP == 0) {
            double t[G::VEC], t2[G::VEC];
            const uint64_t i = live ? (perm ? (uint64_t)perm[r] : (uint64_t)r) : 0;
#pragma unroll
            for (int v = 0; v < G::VEC; ++v) {
                t[v] = probe_sign(key[v], i) * y[v];
                t2[v] = t[v] * t[v];
            }
            const double s1 = row_sum<P>(t), s2 = row_sum<P>(t2);
            if (live && sub == 0) {
                dsum[i] += s1;
                dsum2[i] += s2;
            }
        } else if (live) {
            st_vec<G::VEC>(Y + r * P + sub * G::VEC, y);
            const double* q = Q + r * KP;
#pragma unroll
            for (int b = 0; b < KP; ++b) {
                const double qb = q[b];
#pragma unroll
                for (int v = 0; v < G::VEC; ++v) acc[b][v] = fma(qb, y[v], acc[b][v]);
            }
        }
    }
    if constexpr (KP > 0) block_sum_rows<P, KP>(acc, sub, scratch, part);
}

// t = z .* (y - Q c), reduced over the row's probes, into dsum / dsum2
template <int P, int KP>
__global__ __launch_bounds__(kDiagBlock) void k_diag_finish(int n, uint64_t seed, int64_t base,
                                                            const int* __restrict__ perm,
                                                            const double* __restrict__ Q,
                                                            const double* __restrict__ c,
                                                            const double* __restrict__ Y, double* __restrict__ dsum,
                                                            double* __restrict__ dsum2) {
    using G = DiagGeo<P>;
    const int sub = threadIdx.x % G::LPR;
    uint64_t key[G::VEC];
    probe_keys<P>(seed, base, sub, key);
    double cc[KP][G::VEC];
#pragma unroll
    for (int b = 0; b < KP; ++b)
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) cc[b][v] = c[b * P + sub * G::VEC + v];
    for (int64_t rb = (int64_t)blockIdx.x * G::RPB; rb < n; rb += (int64_t)gridDim.x * G::RPB) {
        const int64_t r = rb + threadIdx.x / G::LPR;
        const bool live = r < n;
        double y[G::VEC], s[G::VEC];
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) y[v] = s[v] = 0.0;
        if (live) {
            ld_vec<G::VEC>(Y + r * P + sub * G::VEC, y);
            const double* q = Q + r * KP;
#pragma unroll
            for (int b = 0; b < KP; ++b) {
                const double qb = q[b];
#pragma unroll
                for (int v = 0; v < G::VEC; ++v) s[v] = fma(qb, cc[b][v], s[v]);
            }
        }
        const uint64_t i = live ? (perm ? (uint64_t)perm[r] : (uint64_t)r) : 0;
        double t[G::VEC], t2[G::VEC];
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) {
            t[v] = probe_sign(key[v], i) * (y[v] - s[v]);
            t2[v] = t[v] * t[v];
        }
        const double s1 = row_sum<P>(t), s2 = row_sum<P>(t2);
        if (live && sub == 0) {
            dsum[i] += s1;
            dsum2[i] += s2;
        }
    }
}

// d0[r] = 2 sum_c Q[r, c] G[r, c] - sum_c (sum_b Q[r, b] H[b, c]) Q[r, c]
// (Q, G n x ld row-major in original row numbering; H k x k column-major)
__global__ __launch_bounds__(256) void k_diag_d0(int n, int k, const double* __restrict__ Q,
                                                 const double* __restrict__ G, int ld,
                                                 const double* __restrict__ H, double* __restrict__ d0) {
    __shared__ double sH[16 * 16];
    for (int i = threadIdx.x; i < k * k; i += blockDim.x) sH[i] = H[i];
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const double* q = Q + r * ld;
        const double* g = G + r * ld;
        double a = 0.0, b2 = 0.0;
        for (int c = 0; c < k; ++c) {
            a = fma(q[c], g[c], a);
            double h = 0.0;
            for (int b = 0; b < k; ++b) h = fma(q[b], sH[b + c * k], h);
            b2 = fma(h, q[c], b2);
        }
        d0[r] = 2.0 * a - b2;
    }
}

// kt_entries_fun: the sweep's terms of f(A) entries on a pair list.  The
// DiagGeo<P> geometry per PAIR: LPR lanes own pair e = tab[e] = (r_i, r_j, i,
// j) (rows of Y and Q in the sweep's order, original indices for the signs),
// each lane with its 16-byte probe pair of both rows.  With yt = y - Q c in
// the fma order of k_diag_finish, t = (z_i yt_j + z_j yt_i) / 2 and t^2 are
// reduced over the pair's probes by the butterfly of row_sum and added to
// esum[e] / esum2[e] by the group's lane 0 (every pair has its own slot: no
// atomics).  Dead lanes of a tail group carry zeros through the butterfly; a
// remainder sweep's dead columns are zero columns of Y and c.
template <int P, int KP>
__global__ __launch_bounds__(kDiagBlock) void k_entries_accumulate(int64_t npairs, const int4* __restrict__ tab,
                                                                   uint64_t seed, int64_t base,
                                                                   const double* __restrict__ Q,
                                                                   const double* __restrict__ c,
                                                                   const double* __restrict__ Y,
                                                                   double* __restrict__ esum,
                                                                   double* __restrict__ esum2) {
    using G = DiagGeo<P>;
    const int sub = threadIdx.x % G::LPR;
    uint64_t key[G::VEC];
    probe_keys<P>(seed, base, sub, key);
    double cc[KP > 0 ? KP : 1][G::VEC];
#pragma unroll
    for (int b = 0; b < KP; ++b)
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) cc[b][v] = c[b * P + sub * G::VEC + v];
    for (int64_t eb = (int64_t)blockIdx.x * G::RPB; eb < npairs; eb += (int64_t)gridDim.x * G::RPB) {
        const int64_t e = eb + threadIdx.x / G::LPR;
        const bool live = e < npairs;
        double yi[G::VEC], yj[G::VEC], si[G::VEC], sj[G::VEC];
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) yi[v] = yj[v] = si[v] = sj[v] = 0.0;
        int4 pe = {0, 0, 0, 0};
        if (live) {
            pe = tab[e];
            ld_vec<G::VEC>(Y + (int64_t)pe.x * P + sub * G::VEC, yi);
            ld_vec<G::VEC>(Y + (int64_t)pe.y * P + sub * G::VEC, yj);
            if constexpr (KP > 0) {
                const double* qi = Q + (int64_t)pe.x * KP;
                const double* qj = Q + (int64_t)pe.y * KP;
#pragma unroll
                for (int b = 0; b < KP; ++b) {
                    const double qib = qi[b], qjb = qj[b];
#pragma unroll
                    for (int v = 0; v < G::VEC; ++v) {
                        si[v] = fma(qib, cc[b][v], si[v]);
                        sj[v] = fma(qjb, cc[b][v], sj[v]);
                    }
                }
            }
        }
        double t[G::VEC], t2[G::VEC];
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) {
            const double zi = probe_sign(key[v], (uint64_t)pe.z), zj = probe_sign(key[v], (uint64_t)pe.w);
            t[v] = 0.5 * (zi * (yj[v] - sj[v]) + zj * (yi[v] - si[v]));
            t2[v] = t[v] * t[v];
        }
        const double s1 = row_sum<P>(t), s2 = row_sum<P>(t2);
        if (live && sub == 0) {
            esum[e] += s1;
            esum2[e] += s2;
        }
    }
}

// e0[e] = sum_c (Q[i, c] G[j, c] + G[i, c] Q[j, c])
//         - (sum_c (QH)[i, c] Q[j, c] + (QH)[j, c] Q[i, c]) / 2,  (i, j) = tab[e].zw
// (Q, G n x ld row-major in original row numbering; H k x k column-major).
// Each column's two products are rounded and added symmetrically, so (i, j)
// and (j, i) give the same bits.  The column loop is compiled without
// contraction: __dmul_rn / __dadd_rn are plain operators here, and an fma of
// one product onto the other rounds (i, j) and (j, i) differently.
__global__ __launch_bounds__(256) void k_entries_e0(int64_t npairs, const int4* __restrict__ tab, int k,
                                                    const double* __restrict__ Q, const double* __restrict__ G,
                                                    int ld, const double* __restrict__ H,
                                                    double* __restrict__ e0) {
    __shared__ double sH[16 * 16];
    for (int i = threadIdx.x; i < k * k; i += blockDim.x) sH[i] = H[i];
    __syncthreads();
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < npairs;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int4 pe = tab[e];
        const double* qi = Q + (int64_t)pe.z * ld;
        const double* qj = Q + (int64_t)pe.w * ld;
        const double* gi = G + (int64_t)pe.z * ld;
        const double* gj = G + (int64_t)pe.w * ld;
        double a = 0.0, b2 = 0.0;
        for (int c = 0; c < k; ++c) {
#pragma clang fp contract(off)
            a += qi[c] * gj[c] + gi[c] * qj[c];
            double hi = 0.0, hj = 0.0;
            for (int b = 0; b < k; ++b) {
                hi = fma(qi[b], sH[b + c * k], hi);
                hj = fma(qj[b], sH[b + c * k], hj);
            }
            b2 += hi * qj[c] + hj * qi[c];
        }
        e0[e] = a - 0.5 * b2;
    }
}

template <class F> hipError_t by_width(int P, F&& f) {
    switch (P) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        default: return hipErrorInvalidValue;
    }
}
template <class F> hipError_t by_defl(int KP, F&& f) {
    switch (KP) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 16: return f(std::integral_constant<int, 16>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

int diag_grid(int n, int P) {
    const int vec = P >= 2 ? 2 : 1, rpb = kDiagBlock / (P / vec);
    return (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n + rpb - 1) / rpb, 1024));
}

hipError_t launch_diag_qtz(int P, int KP, int grid, int n, uint64_t seed, int64_t base, int nc, const int* perm,
                           const double* Q, double* part, hipStream_t st) {
    return by_width(P, [&](auto p) {
        return by_defl(KP, [&](auto k) {
            k_diag_qtz<decltype(p)::value, decltype(k)::value>
                <<<grid, kDiagBlock, 0, st>>>(n, seed, base, nc, perm, Q, part);
            return hipGetLastError();
        });
    });
}

hipError_t launch_diag_sum_parts(int nparts, int K, const double* part, double* out, hipStream_t st) {
    k_diag_sum_parts<<<(K + 3) / 4, 256, 0, st>>>(nparts, K, part, out);
    return hipGetLastError();
}

hipError_t launch_diag_start(int P, int KP, int grid, int n, uint64_t seed, int64_t base, int nc, const int* perm,
                             const double* Q, const double* c, double* X, double* part, hipStream_t st) {
    return by_width(P, [&](auto p) {
        constexpr int PP = decltype(p)::value;
        if (KP == 0) {
            k_diag_start<PP, 0><<<grid, kDiagBlock, 0, st>>>(n, seed, base, nc, perm, Q, c, X, part);
            return hipGetLastError();
        }
        return by_defl(KP, [&](auto k) {
            k_diag_start<PP, decltype(k)::value><<<grid, kDiagBlock, 0, st>>>(n, seed, base, nc, perm, Q, c, X, part);
            return hipGetLastError();
        });
    });
}

hipError_t launch_diag_combine(int P, int KP, int grid, int n, int m, int mdepth, const double* V, int64_t sstride,
                               const double* W, const int* depth, uint64_t seed, int64_t base, const int* perm,
                               const double* Q, double* Y, double* part, double* dsum, double* dsum2,
                               hipStream_t st) {
    const size_t lds = sizeof(double) * ((size_t)m * P + (size_t)4 * KP * P);
    return by_width(P, [&](auto p) {
        constexpr int PP = decltype(p)::value;
        if (KP == 0) {
            k_diag_combine<PP, 0><<<grid, kDiagBlock, lds, st>>>(n, m, mdepth, V, sstride, W, depth, seed, base, perm,
                                                                 Q, Y, part, dsum, dsum2);
            return hipGetLastError();
        }
        return by_defl(KP, [&](auto k) {
            k_diag_combine<PP, decltype(k)::value><<<grid, kDiagBlock, lds, st>>>(
                n, m, mdepth, V, sstride, W, depth, seed, base, perm, Q, Y, part, dsum, dsum2);
            return hipGetLastError();
        });
    });
}

hipError_t launch_diag_combine_y(int P, int grid, int n, int m, int mdepth, const double* V, int64_t sstride,
                                 const double* W, const int* depth, double* Y, hipStream_t st) {
    const size_t lds = sizeof(double) * (size_t)m * P;
    return by_width(P, [&](auto p) {
        k_diag_combine<decltype(p)::value, 0, true><<<grid, kDiagBlock, lds, st>>>(
            n, m, mdepth, V, sstride, W, depth, 0, 0, nullptr, nullptr, Y, nullptr, nullptr, nullptr);
        return hipGetLastError();
    });
}

int entries_grid(int64_t npairs, int P) {
    const int vec = P >= 2 ? 2 : 1, ppb = kDiagBlock / (P / vec);
    return (int)std::max<int64_t>(1, std::min<int64_t>((npairs + ppb - 1) / ppb, 4096));
}

hipError_t launch_entries_accumulate(int P, int KP, int64_t npairs, const void* tab, uint64_t seed, int64_t base,
                                     const double* Q, const double* c, const double* Y, double* esum,
                                     double* esum2, hipStream_t st) {
    const int grid = entries_grid(npairs, P);
    const int4* t = static_cast<const int4*>(tab);
    return by_width(P, [&](auto p) {
        constexpr int PP = decltype(p)::value;
        if (KP == 0) {
            k_entries_accumulate<PP, 0><<<grid, kDiagBlock, 0, st>>>(npairs, t, seed, base, Q, c, Y, esum, esum2);
            return hipGetLastError();
        }
        return by_defl(KP, [&](auto k) {
            k_entries_accumulate<PP, decltype(k)::value>
                <<<grid, kDiagBlock, 0, st>>>(npairs, t, seed, base, Q, c, Y, esum, esum2);
            return hipGetLastError();
        });
    });
}

hipError_t launch_entries_e0(int64_t npairs, const void* tab, int k, const double* Q, const double* G, int ld,
                             const double* H, double* e0, hipStream_t st) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((npairs + 255) / 256, 2048));
    k_entries_e0<<<grid, 256, 0, st>>>(npairs, static_cast<const int4*>(tab), k, Q, G, ld, H, e0);
    return hipGetLastError();
}

hipError_t launch_diag_finish(int P, int KP, int grid, int n, uint64_t seed, int64_t base, const int* perm,
                              const double* Q, const double* c, const double* Y, double* dsum, double* dsum2,
                              hipStream_t st) {
    return by_width(P, [&](auto p) {
        return by_defl(KP, [&](auto k) {
            k_diag_finish<decltype(p)::value, decltype(k)::value>
                <<<grid, kDiagBlock, 0, st>>>(n, seed, base, perm, Q, c, Y, dsum, dsum2);
            return hipGetLastError();
        });
    });
}

hipError_t launch_diag_d0(int n, int k, const double* Q, const double* G, int ld, const double* H, double* d0,
                          hipStream_t st) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n + 255) / 256, 2048));
    k_diag_d0<<<grid, 256, 0, st>>>(n, k, Q, G, ld, H, d0);
    return hipGetLastError();
}

}  // namespace kt
