// kt_nodes.cpp -- node removal scored exactly:
// kt_trace_fun_update_nodes, Xm ~= tr f(A_{-i}) - tr f(A) for a list of nodes
// (A_{-i}: row and column i zeroed, the node left as an isolated vertex), and
// kt_krylov_break_node, the greedy loop over it.
//
// Removing node i is a rank-2 update whose block Krylov space is the
// single-vector space K_{j+1}(A, e_i), so the candidates are columns of the
// sweep engine (kt_slq.cpp lanczos_nodes_adaptive; the stopping test is
// kt_adapt.hip k_node_check).  n <= 130 takes the dense host path, as
// trace_fun_update.m:37-51 does.
//
// kt_diag_fun_bracket (§4.2i) runs the same unit-vector sweeps with the Gauss /
// Gauss-Radau bracket of exp(A)_ii as their check (lanczos_nodes_bracket,
// k_bracket_check); kt_entries_fun_bracket (§4.2j) brackets exp(A)_ij from two
// such columns per pair, started at (e_i +- e_j) / sqrt 2 (lanczos_pairs_bracket,
// k_pair_start, k_pair_bracket_check).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "kt_krylov.h"
#include "kt_slq.h"

namespace kt {

namespace {

// dense path: eig(A) once, eig(A_{-i}) per candidate, on the host
void nodes_dense(kt_matrix_s* A, int64_t ncand, const int64_t* nodes, int fun, double* Xm, int* iter, int* lucky) {
    const int n = (int)A->n;
    std::vector<double> D((size_t)n * n, 0.0), w2(n), w1(n);
    for (int r = 0; r < n; ++r)
        for (int64_t k = A->h_rowptr[r]; k < A->h_rowptr[r + 1]; ++k) D[r + (size_t)A->h_col[k] * n] = A->h_val[k];
    sym_eig_host(n, D.data(), w2.data(), nullptr);
    std::sort(w2.begin(), w2.end());
    for (int64_t c = 0; c < ncand; ++c) {
        std::vector<double> Di = D;
        const int64_t i = nodes[c];
        for (int r = 0; r < n; ++r) Di[r + (size_t)i * n] = Di[i + (size_t)r * n] = 0.0;
        sym_eig_host(n, Di.data(), w1.data(), nullptr);
        std::sort(w1.begin(), w1.end());
        Xm[c] = trace_diff(w1, w2, fun);
        if (iter) iter[c] = 0;
        if (lucky) lucky[c] = 0;
    }
}

// what both entries check before the device is touched: first what needs no
// matrix, then (node_checks) the rest; returns `it` resolved
void scalar_checks(int64_t ncand, int it, int fun, const char* who) {
    const std::string w(who);
    if (ncand < 0) fail(KT_ERR_ARG, w + ": negative candidate count");
    if (fun < KT_FUN_EXP || fun > KT_FUN_SQRT) fail(KT_ERR_ARG, w + ": unknown fun");
    if (fun == KT_FUN_LOG) fail(KT_ERR_ARG, w + ": fun = log is not supported (f(0) of the isolated node is not finite)");
    if (it > kAdaptMaxCap) fail(KT_ERR_ARG, w + ": it must be at most 256");
}

int node_checks(kt_matrix_s* A, int64_t ncand, const int64_t* nodes, double& tol, int it, const char* who) {
    const std::string w(who);
    if (A->n > INT32_MAX) fail(KT_ERR_ARG, w + ": n must fit 32-bit indices");
    for (int64_t c = 0; c < ncand; ++c)
        if (nodes[c] < 0 || nodes[c] >= A->n) fail(KT_ERR_ARG, w + ": node index out of range");
    if (A->ctx->ws.slq_submitted != A->ctx->ws.slq_collected)
        fail(KT_ERR_ARG, w + ": kt_slq_submit calls are outstanding on this context");
    require_symmetric(A, "TRACE_FUN_UPDATE_NODES:: symmetric A required");
    if (!(tol > 0.0)) tol = 1e-12;
    if (it <= 0) it = (int)std::min<int64_t>(100, A->n);  // trace_fun_update.m:25-27
    return it;
}

void nodes_update(kt_matrix_s* A, int64_t ncand, const int64_t* nodes, double tol, int it, int fun, double* Xm,
                  int* iter, int* lucky) {
    if (ncand == 0) return;
    if (A->n <= 130) {
        nodes_dense(A, ncand, nodes, fun, Xm, iter, lucky);
        return;
    }
    KT_HIP(hipSetDevice(A->ctx->device));
    prof_recycle(A->ctx);
    lanczos_nodes_adaptive(A, ncand, nodes, tol, it, fun, Xm, iter, lucky);
}

}  // namespace

}  // namespace kt

using namespace kt;

#define KT_NODES_GUARD_END                             \
    catch (const Status& s) {                          \
        set_error(s.msg);                              \
        return s.code;                                 \
    }                                                  \
    catch (const std::bad_alloc&) {                    \
        set_error("host allocation failed");           \
        return KT_ERR_ALLOC;                           \
    }                                                  \
    return KT_OK;

extern "C" int kt_trace_fun_update_nodes(kt_matrix_t A, int64_t ncand, const int64_t* nodes, double tol, int it,
                                         int fun, double* Xm, int* iter, int* lucky) {
    try {
        scalar_checks(ncand, it, fun, "kt_trace_fun_update_nodes");
        if (!A || (ncand > 0 && (!nodes || !Xm))) fail(KT_ERR_ARG, "kt_trace_fun_update_nodes: NULL argument");
        it = node_checks(A, ncand, nodes, tol, it, "kt_trace_fun_update_nodes");
        nodes_update(A, ncand, nodes, tol, it, fun, Xm, iter, lucky);
    }
    KT_NODES_GUARD_END
}

extern "C" int kt_diag_fun_bracket(kt_matrix_t A, int64_t ncand, const int64_t* nodes, double lam_hi, double rtol,
                                   int it, double* lo, double* hi, int* iter, int* flag) {
    try {
        const std::string w("kt_diag_fun_bracket");
        if (ncand < 0) fail(KT_ERR_ARG, w + ": negative candidate count");
        if (it > kAdaptMaxCap) fail(KT_ERR_ARG, w + ": it must be at most 256");
        if (!std::isfinite(lam_hi) || lam_hi > 700.0)
            fail(KT_ERR_ARG, w + ": lam_hi must be finite and at most 700 (exp(lam_hi) scales the result)");
        if (!A || (ncand > 0 && (!nodes || !lo || !hi))) fail(KT_ERR_ARG, w + ": NULL argument");
        if (A->n > INT32_MAX) fail(KT_ERR_ARG, w + ": n must fit 32-bit indices");
        for (int64_t c = 0; c < ncand; ++c)
            if (nodes[c] < 0 || nodes[c] >= A->n) fail(KT_ERR_ARG, w + ": node index out of range");
        if (A->ctx->ws.slq_submitted != A->ctx->ws.slq_collected)
            fail(KT_ERR_ARG, w + ": kt_slq_submit calls are outstanding on this context");
        require_symmetric(A, "DIAG_FUN_BRACKET:: symmetric A required");
        if (!(rtol > 0.0)) rtol = 1e-10;
        if (it <= 0) it = (int)std::min<int64_t>(100, A->n);
        if (ncand == 0) return KT_OK;
        if (A->n <= 130) {
            // dense path: exp(A)_ii = sum_k V_ik^2 exp(w_k), on the host
            const int n = (int)A->n;
            std::vector<double> D((size_t)n * n, 0.0), wv(n), V((size_t)n * n);
            for (int r = 0; r < n; ++r)
                for (int64_t k = A->h_rowptr[r]; k < A->h_rowptr[r + 1]; ++k)
                    D[r + (size_t)A->h_col[k] * n] = A->h_val[k];
            sym_eig_host(n, D.data(), wv.data(), V.data());
            for (int64_t c = 0; c < ncand; ++c) {
                double s = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double v = V[(size_t)nodes[c] + (size_t)k * n];
                    s += v * v * std::exp(wv[k]);
                }
                lo[c] = hi[c] = s;
                if (iter) iter[c] = 0;
                if (flag) flag[c] = 0;
            }
            return KT_OK;
        }
        KT_HIP(hipSetDevice(A->ctx->device));
        prof_recycle(A->ctx);
        lanczos_nodes_bracket(A, ncand, nodes, lam_hi, rtol, it, lo, hi, iter, flag);
    }
    KT_NODES_GUARD_END
}

extern "C" int kt_entries_fun_bracket(kt_matrix_t A, int64_t npairs, const int64_t* ei, const int64_t* ej,
                                      double lam_hi, double rtol, double ftol, int it, double* lo, double* hi,
                                      int* iter, int* flag, int* col_iter) {
    try {
        const std::string w("kt_entries_fun_bracket");
        if (npairs < 0) fail(KT_ERR_ARG, w + ": negative pair count");
        if (it > kAdaptMaxCap) fail(KT_ERR_ARG, w + ": it must be at most 256");
        if (!std::isfinite(lam_hi) || lam_hi > 700.0)
            fail(KT_ERR_ARG, w + ": lam_hi must be finite and at most 700 (exp(lam_hi) scales the result)");
        if (npairs > 0 && (!ei || !ej || !lo || !hi)) fail(KT_ERR_ARG, w + ": NULL argument");
        for (int64_t p = 0; p < npairs; ++p)  // needs no matrix
            if (ei[p] == ej[p])
                fail(KT_ERR_ARG, w + ": a pair with i == j is a diagonal entry; kt_diag_fun_bracket bounds those");
        if (!A) fail(KT_ERR_ARG, w + ": NULL argument");
        if (A->n > INT32_MAX) fail(KT_ERR_ARG, w + ": n must fit 32-bit indices");
        for (int64_t p = 0; p < npairs; ++p)
            if (ei[p] < 0 || ei[p] >= A->n || ej[p] < 0 || ej[p] >= A->n)
                fail(KT_ERR_ARG, w + ": pair index out of range");
        if (A->ctx->ws.slq_submitted != A->ctx->ws.slq_collected)
            fail(KT_ERR_ARG, w + ": kt_slq_submit calls are outstanding on this context");
        require_symmetric(A, "ENTRIES_FUN_BRACKET:: symmetric A required");
        if (!(rtol > 0.0)) rtol = 1e-10;
        if (!(ftol > 0.0)) ftol = 1e-12;
        if (it <= 0) it = (int)std::min<int64_t>(100, A->n);
        if (npairs == 0) return KT_OK;
        // (i, j) and (j, i) are one pair: both run as (min, max)
        std::vector<int64_t> pi((size_t)npairs), pj((size_t)npairs);
        for (int64_t p = 0; p < npairs; ++p) {
            pi[p] = std::min(ei[p], ej[p]);
            pj[p] = std::max(ei[p], ej[p]);
        }
        if (A->n <= 130) {
            // dense path: exp(A)_ij = sum_k V_ik V_jk exp(w_k), on the host
            const int n = (int)A->n;
            std::vector<double> D((size_t)n * n, 0.0), wv(n), V((size_t)n * n);
            for (int r = 0; r < n; ++r)
                for (int64_t k = A->h_rowptr[r]; k < A->h_rowptr[r + 1]; ++k)
                    D[r + (size_t)A->h_col[k] * n] = A->h_val[k];
            sym_eig_host(n, D.data(), wv.data(), V.data());
            for (int64_t p = 0; p < npairs; ++p) {
                double s = 0.0;
                for (int k = 0; k < n; ++k)
                    s += V[(size_t)pi[p] + (size_t)k * n] * V[(size_t)pj[p] + (size_t)k * n] * std::exp(wv[k]);
                lo[p] = hi[p] = s;
                if (iter) iter[p] = 0;
                if (flag) flag[p] = 0;
                if (col_iter) col_iter[2 * p] = col_iter[2 * p + 1] = 0;
            }
            return KT_OK;
        }
        KT_HIP(hipSetDevice(A->ctx->device));
        prof_recycle(A->ctx);
        lanczos_pairs_bracket(A, npairs, pi.data(), pj.data(), lam_hi, rtol, ftol, it, lo, hi, iter, flag, col_iter);
    }
    KT_NODES_GUARD_END
}

extern "C" int kt_krylov_break_node(kt_matrix_t A, int k, int64_t ncand, const int64_t* nodes, double tol, int it,
                                    int fun, int64_t* sel, double* sel_xm, double* rob, int64_t* nsel) {
    try {
        scalar_checks(ncand, it, fun, "kt_krylov_break_node");
        if (!A || !nsel || (ncand > 0 && !nodes) || (k > 0 && ncand > 0 && !sel))
            fail(KT_ERR_ARG, "kt_krylov_break_node: NULL argument");
        if (k < 0) fail(KT_ERR_ARG, "kt_krylov_break_node: k must not be negative");
        it = node_checks(A, ncand, nodes, tol, it, "kt_krylov_break_node");
        *nsel = 0;
        if (rob) *rob = 0.0;
        std::vector<int64_t> cand(nodes, nodes + ncand), ei, ej;
        std::vector<double> xm;
        double total = 0.0;
        for (int s = 0; s < k && !cand.empty(); ++s) {
            xm.assign(cand.size(), 0.0);
            nodes_update(A, (int64_t)cand.size(), cand.data(), tol, it, fun, xm.data(), nullptr, nullptr);
            size_t best = 0;  // the smallest Xm, the first on ties
            for (size_t c = 1; c < cand.size(); ++c)
                if (xm[c] < xm[best]) best = c;
            const int64_t r = cand[best];
            // the node's row and column out of A: one host-ordered edit per step
            ei.clear();
            ej.clear();
            for (int64_t q = A->h_rowptr[r]; q < A->h_rowptr[r + 1]; ++q) {
                ei.push_back(r);
                ej.push_back(A->h_col[q]);
            }
            if (!ei.empty()) {
                KT_HIP(hipSetDevice(A->ctx->device));
                set_pairs(A, (int64_t)ei.size(), ei.data(), ej.data(), 0.0);
            }
            sel[s] = r;
            if (sel_xm) sel_xm[s] = xm[best];
            total += xm[best];
            if (rob) *rob = total;
            *nsel = s + 1;
            cand.erase(cand.begin() + (std::ptrdiff_t)best);
        }
    }
    KT_NODES_GUARD_END
}
