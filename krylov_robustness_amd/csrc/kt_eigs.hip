// kt_eigs.hip -- the streaming kernels of kt_eigs_topk (kt_eigs.cpp, DESIGN.md
// §4.2d): the start / replacement block from the counter RNG, the in-place
// Ritz rotation of the basis at a restart, and the explicit residual pass.
// All three are one pass over row-major blocks with 16-byte accesses that run
// along a row; none uses an atomic, every reduction has a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "kt_launch.h"

namespace kt {

namespace {

using dbl2 = __attribute__((ext_vector_type(2))) double;

__device__ __forceinline__ uint64_t eig_sm64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// column `col` of row `i` (ORIGINAL numbering): the stream of k_rademacher
__device__ __forceinline__ double eig_sign(uint64_t seed, uint64_t col, uint64_t i) {
    const uint64_t key = eig_sm64(eig_sm64(seed) + col);
    return (eig_sm64(key + i) >> 63) ? -1.0 : 1.0;
}

}  // namespace

// X[r, c] for the columns c < 16 whose bit is set in mask: the Rademacher
// column col0 + c keyed by (seed, perm[r], col0 + c); with ones_first, column
// 0 is 1 / sqrt(n) instead.  Eight lanes per row, a column pair (16 bytes)
// per lane; a pair with one bit set stores the one double.
__global__ __launch_bounds__(256) void k_eig_start(int64_t n, uint64_t seed, int64_t col0, unsigned mask,
                                                   int ones_first, double inv_sqrt_n,
                                                   const int* __restrict__ perm, double* __restrict__ X,
                                                   int ldx) {
    const int sub = threadIdx.x & 7;
    const unsigned m2 = (mask >> (2 * sub)) & 3u;
    if (!m2) return;
    for (int64_t r = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3); r < n; r += (int64_t)gridDim.x * 32) {
        const uint64_t i = perm ? (uint64_t)perm[r] : (uint64_t)r;
        double v0 = eig_sign(seed, (uint64_t)(col0 + 2 * sub), i);
        const double v1 = eig_sign(seed, (uint64_t)(col0 + 2 * sub + 1), i);
        if (ones_first && sub == 0) v0 = inv_sqrt_n;
        double* p = X + r * ldx + 2 * sub;
        if (m2 == 3u) {
            const dbl2 t = {v0, v1};
            *reinterpret_cast<dbl2*>(p) = t;
        } else if (m2 == 1u) {
            p[0] = v0;
        } else {
            p[1] = v1;
        }
    }
}

hipError_t launch_eig_start(int64_t n, uint64_t seed, int64_t col0, unsigned mask, bool ones_first, const int* perm,
                            double* X, int ldx, hipStream_t st) {
    if (n <= 0 || !(mask & 0xFFFFu)) return hipSuccess;
    if ((ldx & 1) || ldx < 16 || (reinterpret_cast<uintptr_t>(X) & 15)) return hipErrorInvalidValue;
    const int grid = (int)std::min<int64_t>((n + 31) / 32, 4096);
    k_eig_start<<<grid, 256, 0, st>>>(n, seed, col0, mask & 0xFFFFu, ones_first ? 1 : 0, 1.0 / sqrt((double)n),
                                      perm, X, ldx);
    return hipGetLastError();
}

// V(:, 0:p) <- V(:, 0:mb) Y in place; Y is mb x p ROW-major (Y[k * p + c]).
// A workgroup owns kRotRows rows.  It stages their mb columns in LDS with
// 16-byte loads that run along the row (a lane never walks its own row in
// memory), forms every output of those rows from LDS, and only then stores:
// every input column of a row is read before the row's first store, and no
// other workgroup touches the row.  Thread t: output columns (t & 15) + 16 i,
// i < p / 16, of the rows 4 (t >> 4) .. + 3.  A wave's 16-lane groups read Y
// as 128-byte runs (the other groups the same addresses: broadcasts) and four
// different rows of the stage, whose stride of mb + 2 doubles puts them on
// different banks.  Each output is one fma chain over k ascending.
constexpr int kRotRows = 64;
constexpr int kRotMaxMb = 128;
constexpr int kRotMaxP = 48;

__global__ __launch_bounds__(256) void k_eig_rotate(int64_t n, int mb, int p, double* V, int ld,
                                                    const double* __restrict__ Y) {
    extern __shared__ double lds[];
    const int ss = mb + 2;               // stage row stride (even: 16-byte rows)
    double* S = lds;                     // kRotRows x ss
    double* Ys = lds + kRotRows * ss;    // mb x p
    const int64_t rbase = (int64_t)blockIdx.x * kRotRows;
    const int half = mb >> 1;
    for (int t = threadIdx.x; t < kRotRows * half; t += 256) {
        const int rr = t / half, c2 = t - rr * half;
        const int64_t r = rbase + rr;
        dbl2 v = {0.0, 0.0};
        if (r < n) v = *reinterpret_cast<const dbl2*>(V + r * ld + 2 * c2);
        *reinterpret_cast<dbl2*>(S + rr * ss + 2 * c2) = v;
    }
    for (int t = threadIdx.x; t < mb * p; t += 256) Ys[t] = Y[t];
    __syncthreads();
    const int c = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int np = p >> 4;
    double acc[4][3];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[a][i] = 0.0;
    const double* s0 = S + (4 * rg) * ss;
    for (int k = 0; k < mb; ++k) {
        double y[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) y[i] = i < np ? Ys[k * p + c + 16 * i] : 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double x = s0[a * ss + k];
#pragma unroll
            for (int i = 0; i < 3; ++i) acc[a][i] = fma(x, y[i], acc[a][i]);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t r = rbase + 4 * rg + a;
        if (r >= n) continue;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < np) V[r * ld + c + 16 * i] = acc[a][i];
    }
}

hipError_t launch_eig_rotate(int64_t n, int mb, int p, double* V, int ld, const double* Y, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (mb < 2 || mb > kRotMaxMb || (mb & 1) || p < 16 || p > kRotMaxP || (p & 15) || p > mb || ld < mb ||
        (ld & 1) || (reinterpret_cast<uintptr_t>(V) & 15))
        return hipErrorInvalidValue;
    const size_t bytes = sizeof(double) * ((size_t)kRotRows * (mb + 2) + (size_t)mb * p);
    // the largest shape needs 113 KB of the CU's 160 (per device: set at every launch)
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(k_eig_rotate),
                                              hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)(sizeof(double) * (kRotRows * (kRotMaxMb + 2) + kRotMaxMb * kRotMaxP)));
    if (ea != hipSuccess) return ea;
    const unsigned grid = (unsigned)((n + kRotRows - 1) / kRotRows);
    k_eig_rotate<<<grid, 256, bytes, st>>>(n, mb, p, V, ld, Y);
    return hipGetLastError();
}

// Partials of the explicit residual pass over X and AX (n x kp row-major at
// ldx / ldax, kp = 16 or 32): for column i
//   part[chunk][0][i] = sum_r (AX[r, i] - theta[i] X[r, i])^2
//   part[chunk][1][i] = sum_r X[r, i]^2
//   part[chunk][2][i] = sum_r X[r, i]
// over the chunk's kResidRows rows.  kp / 2 lanes per row, a column pair (16
// bytes) per lane; a lane adds its rows in ascending order, the lanes of a
// column pair are added in ascending order through LDS.  launch_eig_resid sums
// the chunks in a fixed order (k_eig_resid_sum: a wave per value, lane l adds
// chunks l, l + 64, ... in order, then an xor butterfly).
constexpr int kResidRows = 512;

__global__ __launch_bounds__(256) void k_eig_resid(int64_t n, int kp, const double* __restrict__ X, int ldx,
                                                   const double* __restrict__ AX, int ldax,
                                                   const double* __restrict__ theta, double* __restrict__ part) {
    __shared__ double red[256][6];
    const int lpr = kp >> 1;               // lanes per row: 8 or 16
    const int sub = threadIdx.x % lpr, rl = threadIdx.x / lpr, nrl = 256 / lpr;
    const double t0 = theta[2 * sub], t1 = theta[2 * sub + 1];
    const int64_t rb = (int64_t)blockIdx.x * kResidRows;
    const int64_t re = rb + kResidRows < n ? rb + kResidRows : n;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t r = rb + rl; r < re; r += nrl) {
        const dbl2 x = __builtin_nontemporal_load(reinterpret_cast<const dbl2*>(X + r * ldx + 2 * sub));
        const dbl2 y = __builtin_nontemporal_load(reinterpret_cast<const dbl2*>(AX + r * ldax + 2 * sub));
        const double d0 = y[0] - t0 * x[0], d1 = y[1] - t1 * x[1];
        a[0] = fma(d0, d0, a[0]);
        a[1] = fma(d1, d1, a[1]);
        a[2] = fma(x[0], x[0], a[2]);
        a[3] = fma(x[1], x[1], a[3]);
        a[4] += x[0];
        a[5] += x[1];
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) red[threadIdx.x][q] = a[q];
    __syncthreads();
    if (threadIdx.x < 3 * kp) {
        const int which = threadIdx.x / kp, i = threadIdx.x - which * kp;
        const int q = 2 * which + (i & 1), s = i >> 1;
        double acc = 0.0;
        for (int l = 0; l < nrl; ++l) acc += red[l * lpr + s][q];
        part[((size_t)blockIdx.x * 3 + which) * kp + i] = acc;
    }
}

__global__ __launch_bounds__(256) void k_eig_resid_sum(int nchunks, int count, const double* __restrict__ part,
                                                       double* __restrict__ out) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= count) return;  // wave-uniform
    double acc = 0.0;
    for (int s = lane; s < nchunks; s += 64) acc += part[(size_t)s * count + t];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) out[t] = acc;
}

int eig_resid_chunks(int64_t n) { return (int)((n + kResidRows - 1) / kResidRows); }

hipError_t launch_eig_resid(int64_t n, int kp, const double* X, int ldx, const double* AX, int ldax,
                            const double* theta, double* part, double* out, hipStream_t st) {
    if (n <= 0) return hipErrorInvalidValue;
    if ((kp != 16 && kp != 32) || ldx < kp || ldax < kp || (ldx & 1) || (ldax & 1) ||
        (reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(AX) & 15))
        return hipErrorInvalidValue;
    const int chunks = eig_resid_chunks(n);
    k_eig_resid<<<chunks, 256, 0, st>>>(n, kp, X, ldx, AX, ldax, theta, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_eig_resid_sum<<<(3 * kp + 3) / 4, 256, 0, st>>>(chunks, 3 * kp, part, out);
    return hipGetLastError();
}

}  // namespace kt
