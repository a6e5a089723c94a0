// kt_eigs.cpp -- kt_eigs_topk: the k largest algebraic eigenpairs of symmetric
// A by thick-restart block Lanczos with full reorthogonalisation and
// Rayleigh-Ritz on the host.
//
// Geometry: block width b = 16; one row-major basis of 128 columns (capacity
// mb = 128, or 112 where n < 144) and one 16-wide work block, both in the row
// order of the block SpMM's device copy.  After a rotation the columns 64..95
// of the basis are free and hold A X for the residual pass.
//
//   start    column 0 = 1/sqrt(n), columns 1..15 Rademacher from the counter
//            RNG keyed by (seed, original row, column); CholQR
//   expand   W = A V_j; two block-CGS passes against every basis column
//            (gram_device + combine_device): their coefficients are T's block
//            column T(:, j) = V' A V_j, filled symmetrically on the host, so T
//            is the Rayleigh quotient of the expanded columns whatever the next
//            block is; CholQR of W gives V_{j+1}
//   rank     a column of W whose remainder after the earlier ones is below
//            1e-8 ||A V_j|| (or that CholQR could not factor) is replaced by a
//            fresh counter-RNG column, projected against the basis twice
//   restart  eig of sym(T) on the calling thread; V(:, 0:p) <- V Y in place
//            (k_eig_rotate), p = kp + 16 with kp = 16 or 32 >= k; T becomes
//            diag(theta) and the work block follows the kept vectors
//   check    at every restart A X is formed for the leading kp Ritz vectors
//            (one more block product, two for kp = 32) and k_eig_resid gives
//            ||A x - theta x||, ||x||^2 and sum(x) explicitly: the values
//            returned are those of the vectors returned
// No atomics; every host eigenproblem runs on the calling thread.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>

#include "kt_block.h"
#include "kt_krylov.h"
#include "kt_launch.h"

namespace kt {

namespace {

constexpr int kB = 16;        // block width
constexpr int kLd = 128;      // the basis' row stride
constexpr int kAxCol = 64;    // A X lives in basis columns [64, 96) after a rotation
constexpr int kDenseMaxN = 130;

double converged_scale(const double* lambda, int k) { return std::max(std::fabs(lambda[0]), std::fabs(lambda[k - 1])); }

int leading_converged(const double* resid, int k, double tol, double scale) {
    int c = 0;
    while (c < k && resid[c] <= tol * scale) ++c;
    return c;
}

// eigenvalue order: descending, ties by index (a fixed order)
std::vector<int> descending(const std::vector<double>& w) {
    std::vector<int> idx(w.size());
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return w[a] > w[b]; });
    return idx;
}

// n <= 130: the dense host path (the shortcut of the other drivers)
void topk_dense(kt_matrix_s* A, int k, double tol, double* lambda, double* V, double* resid, int* nconv) {
    const int n = (int)A->n;
    std::vector<double> D((size_t)n * n, 0.0), w(n), Q((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int64_t e = A->h_rowptr[i]; e < A->h_rowptr[i + 1]; ++e) D[i + (size_t)A->h_col[e] * n] += A->h_val[e];
    sym_eig_host(n, D.data(), w.data(), Q.data());
    const std::vector<int> idx = descending(w);
    std::vector<double> res(k), v(n);
    for (int c = 0; c < k; ++c) {
        const double* q = Q.data() + (size_t)idx[c] * n;
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += q[i];
        const double sg = sum < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < n; ++i) v[i] = sg * q[i];
        lambda[c] = w[idx[c]];
        double s2 = 0.0;
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int64_t e = A->h_rowptr[i]; e < A->h_rowptr[i + 1]; ++e) s += A->h_val[e] * v[A->h_col[e]];
            s -= lambda[c] * v[i];
            s2 += s * s;
        }
        res[c] = std::sqrt(s2);
        if (V) std::copy(v.begin(), v.end(), V + (size_t)c * n);
    }
    if (resid) std::copy(res.begin(), res.end(), resid);
    if (nconv) *nconv = leading_converged(res.data(), k, tol, converged_scale(lambda, k));
}

// The columns of the 16-wide block with Gram matrix G (column-major) that add
// nothing to the columns before them: a Cholesky sweep that skips such a
// column.  A column's remainder d^2 counts as nothing when it is below 1e-16
// scale2 (1e-8 of ||A V_j|| in norm) or below 1e-13 of the column's own square
// (CholQR2 cannot restore a block that ill-conditioned); a NaN flags too.
unsigned deficient_columns(const std::vector<double>& G, double scale2) {
    double R[kB][kB];
    unsigned mask = 0;
    for (int c = 0; c < kB; ++c) {
        double d = G[c + (size_t)c * kB];
        for (int i = 0; i < c; ++i) {
            if (mask & (1u << i)) continue;
            double s = G[i + (size_t)c * kB];
            for (int l = 0; l < i; ++l)
                if (!(mask & (1u << l))) s -= R[l][i] * R[l][c];
            R[i][c] = s / R[i][i];
            d -= R[i][c] * R[i][c];
        }
        if (!(d > std::max(1e-13 * G[c + (size_t)c * kB], 1e-16 * scale2))) mask |= 1u << c;
        else R[c][c] = std::sqrt(d);
    }
    return mask;
}

struct Solver {
    kt_matrix_s* A;
    kt_context_s* ctx;
    int64_t n;
    int k, kp, pkeep, mb;
    uint64_t seed;
    int64_t next_col = kB;  // the next unused counter-RNG column
    DevMat basis, work, aux;
    double *dY, *dTheta, *dOut, *dPart;
    std::vector<double> T;  // mb x mb column-major: V' A V of the expanded columns
    int nsp = 0, restarts = 0;

    double* Vc(int c) { return basis.col(c); }

    void fresh(unsigned mask) {
        prof_begin(ctx, PROF_EIGS, ctx->stream, kB);
        KT_HIP(launch_eig_start(n, seed, next_col, mask, false, nullptr, work.col(0), kB, ctx->stream));
        prof_end(ctx, PROF_EIGS, ctx->stream);
        next_col += kB;
    }

    // work <- (I - V V') work over the basis columns [0, nb), one block-CGS
    // pass; the coefficients V' work also into C (nb x 16 column-major, host:
    // valid after the next stream synchronisation), nullptr: not wanted
    void project(int nb, double* C) {
        const double* dC = gram_device(ctx, n, Vc(0), kLd, nb, work.col(0), kB, kB);
        if (C)
            KT_HIP(hipMemcpyAsync(C, dC, sizeof(double) * (size_t)nb * kB, hipMemcpyDeviceToHost, ctx->stream));
        combine_device(ctx, n, Vc(0), kLd, nb, dC, kB, -1.0, 1.0, work.col(0), kB);
    }

    // work <- an orthonormal block orthogonal to the basis columns [0, nb); the
    // columns that lost rank are replaced (see the header).  scale2: ||A V_j||^2.
    void orthonormalise_work(int nb, double scale2) {
        std::vector<double> G, R;
        gram(ctx, n, work.col(0), kB, kB, work.col(0), kB, kB, G);
        double rest = 0.0;  // what the projections left: ||A V_j||^2 = ||V' A V_j||^2 + ||W||^2 per column
        for (int c = 0; c < kB; ++c) rest = std::max(rest, G[c + (size_t)c * kB]);
        scale2 += rest;
        unsigned mask = deficient_columns(G, scale2);
        if (!mask && cholqr(ctx, n, work.col(0), kB, kB, R)) return;
        if (!mask) mask = 0xFFFFu;  // CholQR gave up on the whole block
        for (int attempt = 0; attempt < 2; ++attempt) {
            fresh(mask);
            project(nb, nullptr);
            project(nb, nullptr);
            if (cholqr(ctx, n, work.col(0), kB, kB, R)) return;
            mask = 0xFFFFu;
        }
        fail(KT_ERR_UNSUPPORTED, "kt_eigs_topk: the basis could not be extended");
    }

    // Rayleigh-Ritz on the ne expanded columns: V(:, 0:p) <- V Y, theta (p,
    // descending), then the explicit residual pass on the leading kp vectors.
    // sums: [||A x - theta x||^2 | ||x||^2 | sum x], kp each.
    int ritz(int ne, std::vector<double>& theta, std::vector<double>& sums) {
        const int p = std::min(pkeep, ne);
        std::vector<double> S((size_t)ne * ne), w(ne), Q((size_t)ne * ne);
        for (int j = 0; j < ne; ++j)
            for (int i = 0; i < ne; ++i) S[i + (size_t)j * ne] = 0.5 * (T[i + (size_t)j * mb] + T[j + (size_t)i * mb]);
        sym_eig_host(ne, S.data(), w.data(), Q.data());
        const std::vector<int> idx = descending(w);
        std::vector<double> Y((size_t)ne * p);  // row-major ne x p
        theta.assign(std::max(p, kp), 0.0);
        for (int c = 0; c < p; ++c) {
            theta[c] = w[idx[c]];
            for (int i = 0; i < ne; ++i) Y[(size_t)i * p + c] = Q[i + (size_t)idx[c] * ne];
        }
        KT_HIP(hipMemcpyAsync(dY, Y.data(), sizeof(double) * Y.size(), hipMemcpyHostToDevice, ctx->stream));
        KT_HIP(hipMemcpyAsync(dTheta, theta.data(), sizeof(double) * kp, hipMemcpyHostToDevice, ctx->stream));
        prof_begin(ctx, PROF_EIGS, ctx->stream, p);
        KT_HIP(launch_eig_rotate(n, ne, p, Vc(0), kLd, dY, ctx->stream));
        prof_end(ctx, PROF_EIGS, ctx->stream);
        spmm(A, Vc(0), kLd, Vc(kAxCol), kLd, kp);
        nsp += kp / kB;
        prof_begin(ctx, PROF_EIGS, ctx->stream, kp);
        KT_HIP(launch_eig_resid(n, kp, Vc(0), kLd, Vc(kAxCol), kLd, dTheta, dPart, dOut, ctx->stream));
        prof_end(ctx, PROF_EIGS, ctx->stream);
        sums.assign((size_t)3 * kp, 0.0);
        KT_HIP(hipMemcpyAsync(sums.data(), dOut, sizeof(double) * sums.size(), hipMemcpyDeviceToHost, ctx->stream));
        KT_HIP(hipStreamSynchronize(ctx->stream));
        return p;
    }

    void run(double tol, int cap, double* lambda, double* V, double* resid, int* nconv) {
        basis.alloc(ctx, n, kLd);
        work.alloc(ctx, n, kB);
        const int chunks = eig_resid_chunks(n);
        aux.alloc(ctx, 1, kLd * 48 + 32 + 96 + 96 * chunks);
        dY = aux.col(0);
        dTheta = dY + kLd * 48;
        dOut = dTheta + 32;
        dPart = dOut + 96;
        T.assign((size_t)mb * mb, 0.0);
        std::vector<double> R, C1((size_t)mb * kB), C2((size_t)mb * kB), theta, sums;

        prof_begin(ctx, PROF_EIGS, ctx->stream, kB);
        KT_HIP(launch_eig_start(n, seed, 0, 0xFFFFu, true, nullptr, Vc(0), kLd, ctx->stream));
        prof_end(ctx, PROF_EIGS, ctx->stream);
        if (!cholqr(ctx, n, Vc(0), kLd, kB, R)) fail(KT_ERR_UNSUPPORTED, "kt_eigs_topk: the start block has no rank");

        int ne = 0;  // expanded columns; the block at [ne, ne + 16) is next
        int found = 0;
        for (;;) {
            const int nb = ne + kB;
            spmm(A, Vc(ne), kLd, work.col(0), kB, kB);
            ++nsp;
            project(nb, C1.data());
            project(nb, C2.data());
            KT_HIP(hipStreamSynchronize(ctx->stream));
            double scale2 = 0.0;
            for (int c = 0; c < kB; ++c) {
                double s = 0.0;
                for (int i = 0; i < nb; ++i) {
                    const double t = C1[i + (size_t)c * nb] + C2[i + (size_t)c * nb];
                    T[i + (size_t)(ne + c) * mb] = t;
                    s += t * t;
                }
                scale2 = std::max(scale2, s);
            }
            for (int c = 0; c < kB; ++c)  // the symmetric fill (the block's own square is symmetrised at the eig)
                for (int i = 0; i < ne; ++i) T[(ne + c) + (size_t)i * mb] = T[i + (size_t)(ne + c) * mb];
            orthonormalise_work(nb, scale2);
            ne = nb;
            const bool spent = nsp + 1 + kp / kB > cap;  // no room for one more product and the check
            if (ne < mb && !(spent && ne >= kp)) {
                copy_cols(ctx, n, work.col(0), kB, Vc(ne), kLd, kB);
                continue;
            }
            const int p = ritz(ne, theta, sums);
            std::vector<double> res(k);
            for (int c = 0; c < k; ++c) res[c] = std::sqrt(std::max(0.0, sums[c]));
            found = leading_converged(res.data(), k, tol, converged_scale(theta.data(), k));
            if (found == k || nsp + 1 + kp / kB > cap) {
                for (int c = 0; c < k; ++c) lambda[c] = theta[c];
                if (resid) std::copy(res.begin(), res.end(), resid);
                break;
            }
            std::fill(T.begin(), T.end(), 0.0);
            for (int c = 0; c < p; ++c) T[c + (size_t)c * mb] = theta[c];
            copy_cols(ctx, n, work.col(0), kB, Vc(p), kLd, kB);
            ne = p;
            ++restarts;
        }
        if (nconv) *nconv = found;
        if (V) {
            download_block(A, Vc(0), kLd, k, V);
            for (int c = 0; c < k; ++c)
                if (sums[(size_t)2 * kp + c] < 0.0)
                    for (int64_t i = 0; i < n; ++i) V[i + (size_t)c * n] = -V[i + (size_t)c * n];
        }
    }
};

}  // namespace

void eigs_topk_impl(kt_matrix_s* A, int k, double tol, int max_spmm, uint64_t seed, double* lambda, double* V,
                    double* resid, int* nconv, int* spmm_out) {
    if (tol <= 0.0) tol = 1e-10;
    const int cap = max_spmm > 0 ? max_spmm : 2000;
    if (A->n <= kDenseMaxN) {
        topk_dense(A, k, tol, lambda, V, resid, nconv);
        if (spmm_out) *spmm_out = 0;
        return;
    }
    kt_context_s* ctx = A->ctx;
    KT_HIP(hipSetDevice(ctx->device));
    prof_recycle(ctx);
    Solver s;
    s.A = A;
    s.ctx = ctx;
    s.n = A->n;
    s.k = k;
    s.kp = k <= kB ? kB : 2 * kB;
    s.pkeep = s.kp + kB;
    s.mb = A->n >= 144 ? 128 : 112;  // mb + 16 <= n: the work block has room beside a full basis
    s.seed = seed;
    s.run(tol, cap, lambda, V, resid, nconv);
    ctx->eigs_restarts += s.restarts;
    if (spmm_out) *spmm_out = s.nsp;
}

}  // namespace kt

using namespace kt;

extern "C" int kt_eigs_topk(kt_matrix_t A, int k, double tol, int max_spmm, uint64_t seed, double* lambda, double* V,
                            double* resid, int* nconv, int* spmm) {
    try {
        if (!A || !lambda) fail(KT_ERR_ARG, "kt_eigs_topk: NULL argument");
        if (k < 1 || k > 32 || k > A->n) fail(KT_ERR_ARG, "kt_eigs_topk: k must be in [1, min(32, n)]");
        require_symmetric(A, "EIGS:: symmetric A required");
        if (A->ctx->ws.slq_submitted != A->ctx->ws.slq_collected)
            fail(KT_ERR_ARG, "kt_eigs_topk: kt_slq_submit calls are outstanding on this context");
        eigs_topk_impl(A, k, tol, max_spmm, seed, lambda, V, resid, nconv, spmm);
    } catch (const Status& s) {
        set_error(s.msg);
        return s.code;
    } catch (const std::bad_alloc&) {
        set_error("host allocation failed");
        return KT_ERR_ALLOC;
    }
    return KT_OK;
}
