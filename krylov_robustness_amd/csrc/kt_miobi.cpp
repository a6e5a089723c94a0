// kt_miobi.cpp -- kt_miobi_break and kt_pairs_score_topk: MIOBI's top-t edge
// removal (MIOBIBreakEdge2.m / MIOBIBreakEdge2_weighted.m) with the step loop
// on the device (kernels in kt_miobi.hip).
//
// A window is the run of steps between two eigenpair recomputations.  Its
// steps are queued back to back -- per step k_miobi_score over the pair list
// and k_miobi_pick (argmin, selection record, alive byte, eigenvalue shift);
// in `paper` mode also V <- V (I + S) by k_eig_rotate and the column
// normalisation -- and the selection list, eigenvalue track and stop flag are
// read back once, at the window's end.  A recomputation applies the window's
// removals to A through set_pairs and runs eigs_topk_impl on the edited matrix.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kt_block.h"
#include "kt_krylov.h"
#include "kt_launch.h"

namespace kt {

namespace {

constexpr int kLd = kMiobiLd;

// slices of one pooled device block, 256-byte aligned
struct Carver {
    size_t bytes = 0;
    size_t take(size_t b) {
        const size_t off = bytes;
        bytes += (b + 255) / 256 * 256;
        return off;
    }
};

struct Block {
    DevMat m;
    void alloc(kt_context_s* ctx, size_t bytes) {
        m.alloc(ctx, 1, (int)((bytes + 7) / 8), false);
    }
    template <class T>
    T* at(size_t off) {
        return reinterpret_cast<T*>(static_cast<char*>(m.ptr) + off);
    }
};

// host V (n x t column-major) as the device's n x 32 row-major block, the
// columns >= t zero; abs0: column 0 by absolute value (MIOBIBreakEdge2.m:48)
void upload_v(kt_context_s* ctx, int64_t n, int t, const double* V, bool abs0, double* dV,
              std::vector<double>& stage) {
    stage.assign((size_t)n * kLd, 0.0);
    for (int c = 0; c < t; ++c)
        for (int64_t i = 0; i < n; ++i) {
            const double x = V[i + (size_t)c * n];
            stage[(size_t)i * kLd + c] = (abs0 && c == 0) ? std::fabs(x) : x;
        }
    KT_HIP(hipMemcpyAsync(dV, stage.data(), sizeof(double) * stage.size(), hipMemcpyHostToDevice, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));
}

void upload_e(kt_context_s* ctx, int t, const double* lam, double* dE, double* dC) {
    double e[kLd] = {0.0};
    std::copy(lam, lam + t, e);
    KT_HIP(hipMemcpyAsync(dE, e, sizeof e, hipMemcpyHostToDevice, ctx->stream));
    KT_HIP(hipStreamSynchronize(ctx->stream));  // e leaves scope
    KT_HIP(launch_miobi_setc(t, dE, dC, ctx->stream));
}

void miobi_break_impl(kt_matrix_s* A, int k, int t, int refresh, int mode, double gap_rel, double tol, int max_spmm,
                      uint64_t seed, int64_t* sel_i, int64_t* sel_j, double* sel_score, double* track,
                      double* V_final, int64_t* nsel, int* nconv_min, int* refreshes) {
    kt_context_s* ctx = A->ctx;
    const int64_t n = A->n;
    *nsel = 0;
    if (nconv_min) *nconv_min = t;
    if (refreshes) *refreshes = 0;
    if (track) std::fill(track, track + (size_t)(k + 1) * t, 0.0);
    if (V_final) std::fill(V_final, V_final + (size_t)n * t, 0.0);
    if (A->nnz == 0) return;  // nothing to remove; every eigenvalue is 0

    // [p, r] = find(triu(A, 1)) as a list (:57); the order is free, the key breaks ties
    std::vector<int> hpi, hpj;
    std::vector<double> hwt;
    const bool weighted = !A->unit_values;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = A->h_rowptr[i]; e < A->h_rowptr[i + 1]; ++e)
            if (A->h_col[e] > i) {
                hpi.push_back((int)i);
                hpj.push_back(A->h_col[e]);
                if (weighted) hwt.push_back(A->h_val[e]);
            }
    const int64_t npairs = (int64_t)hpi.size();

    KT_HIP(hipSetDevice(ctx->device));
    prof_recycle(ctx);
    std::vector<double> lam(t), Vh((size_t)n * t), stage;
    int nconv = 0, nc_min;
    eigs_topk_impl(A, t, tol, max_spmm, seed, lam.data(), Vh.data(), nullptr, &nconv, nullptr);
    nc_min = nconv;
    if (track) std::copy(lam.begin(), lam.end(), track);

    const int nblocks = miobi_score_blocks(npairs, 0);
    const int kk = std::max(k, 1);
    DevMat dV;
    dV.alloc(ctx, n, kLd, false);
    Carver cv;
    const size_t oE = cv.take(sizeof(double) * kLd), oC = cv.take(sizeof(double) * kLd),
                 oM = cv.take(sizeof(double) * kLd * kLd), oPs = cv.take(sizeof(double) * kMiobiMaxBlocks),
                 oPk = cv.take(sizeof(unsigned long long) * kMiobiMaxBlocks),
                 oPi = cv.take(sizeof(int) * kMiobiMaxBlocks),
                 oNp = cv.take(sizeof(double) * kLd * miobi_norm_blocks(n)), oSt = cv.take(sizeof(int) * 2),
                 oSi = cv.take(sizeof(int) * kk), oSj = cv.take(sizeof(int) * kk),
                 oSs = cv.take(sizeof(double) * kk), oTr = cv.take(sizeof(double) * kLd * (kk + 1)),
                 oLi = cv.take(sizeof(int) * std::max<int64_t>(npairs, 1)),
                 oLj = cv.take(sizeof(int) * std::max<int64_t>(npairs, 1)),
                 oLw = cv.take(sizeof(double) * std::max<int64_t>(npairs, 1)),
                 oAl = cv.take(std::max<int64_t>(npairs, 1));
    Block blk;
    blk.alloc(ctx, cv.bytes);
    double *dE = blk.at<double>(oE), *dC = blk.at<double>(oC), *dM = blk.at<double>(oM);
    double *dPs = blk.at<double>(oPs), *dNp = blk.at<double>(oNp), *dSs = blk.at<double>(oSs);
    double *dTr = blk.at<double>(oTr), *dLw = weighted ? blk.at<double>(oLw) : nullptr;
    unsigned long long* dPk = blk.at<unsigned long long>(oPk);
    int *dPi = blk.at<int>(oPi), *dSt = blk.at<int>(oSt), *dSi = blk.at<int>(oSi), *dSj = blk.at<int>(oSj);
    int *dLi = blk.at<int>(oLi), *dLj = blk.at<int>(oLj);
    unsigned char* dAl = blk.at<unsigned char>(oAl);
    hipStream_t st = ctx->stream;
    if (npairs) {
        KT_HIP(hipMemcpyAsync(dLi, hpi.data(), sizeof(int) * npairs, hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(dLj, hpj.data(), sizeof(int) * npairs, hipMemcpyHostToDevice, st));
        if (weighted) KT_HIP(hipMemcpyAsync(dLw, hwt.data(), sizeof(double) * npairs, hipMemcpyHostToDevice, st));
        KT_HIP(hipMemsetAsync(dAl, 1, (size_t)npairs, st));
    }
    KT_HIP(hipMemsetAsync(dSt, 0, sizeof(int) * 2, st));
    KT_HIP(hipMemsetAsync(dTr, 0, sizeof(double) * kLd * (kk + 1), st));
    KT_HIP(hipStreamSynchronize(st));
    upload_v(ctx, n, t, Vh.data(), true, dV.col(0), stage);
    upload_e(ctx, t, lam.data(), dE, dC);

    std::vector<int> hsi(kk), hsj(kk);
    std::vector<double> hss(kk), htr((size_t)kLd * (kk + 1));
    std::vector<int64_t> ei, ej;
    int done = 0, nref = 0;
    while (done < k) {
        int w = k - done;
        if (refresh > 0) w = std::min(w, refresh - done % refresh);
        for (int s = 0; s < w; ++s) {
            prof_begin(ctx, PROF_MIOBI, st, t);
            KT_HIP(launch_miobi_score(npairs, t, dV.col(0), dC, dLi, dLj, dAl, -2.0, nullptr, nblocks, dPs, dPk, dPi,
                                      dSt + 1, st));
            KT_HIP(launch_miobi_pick(nblocks, dPs, dPk, dPi, t, mode, gap_rel, dV.col(0), dE, dC, dLi, dLj, dLw, dAl,
                                     dSi, dSj, dSs, dTr, dM, dSt, st));
            if (mode) {  // after the stop M = I: the rotation leaves V as it is
                KT_HIP(launch_eig_rotate(n, kLd, kLd, dV.col(0), kLd, dM, st));
                KT_HIP(launch_miobi_normalise(n, dV.col(0), dNp, dSt, st));
            }
            prof_end(ctx, PROF_MIOBI, st);
        }
        int state[2] = {0, 0};
        KT_HIP(hipMemcpyAsync(state, dSt, sizeof state, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hsi.data() + done, dSi + done, sizeof(int) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hsj.data() + done, dSj + done, sizeof(int) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hss.data() + done, dSs + done, sizeof(double) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(htr.data() + (size_t)kLd * (done + 1), dTr + (size_t)kLd * (done + 1),
                              sizeof(double) * kLd * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        const int now = state[0];
        if (now < done || now > done + w) fail(KT_ERR_HIP, "kt_miobi_break: the device step count is out of range");
        ei.clear();
        ej.clear();
        for (int s = done; s < now; ++s) {
            sel_i[s] = hsi[s];
            sel_j[s] = hsj[s];
            sel_score[s] = hss[s];
            if (track) std::copy(htr.begin() + (size_t)kLd * (s + 1), htr.begin() + (size_t)kLd * (s + 1) + t,
                                 track + (size_t)(s + 1) * t);
            ei.push_back(hsi[s]);
            ej.push_back(hsj[s]);
        }
        if (!ei.empty()) set_pairs(A, (int64_t)ei.size(), ei.data(), ej.data(), 0.0);
        done = now;
        *nsel = done;
        if (state[1] || done >= k || A->nnz == 0) break;  // (an empty matrix has nothing left to score)
        // :255-261  the eigenpairs of the edited matrix
        eigs_topk_impl(A, t, tol, max_spmm, seed, lam.data(), Vh.data(), nullptr, &nconv, nullptr);
        nc_min = std::min(nc_min, nconv);
        ++nref;
        upload_v(ctx, n, t, Vh.data(), true, dV.col(0), stage);
        upload_e(ctx, t, lam.data(), dE, dC);
        if (track) std::copy(lam.begin(), lam.end(), track + (size_t)done * t);
    }
    if (V_final) {
        stage.resize((size_t)n * kLd);
        KT_HIP(hipMemcpyAsync(stage.data(), dV.col(0), sizeof(double) * stage.size(), hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        for (int c = 0; c < t; ++c)
            for (int64_t i = 0; i < n; ++i) V_final[i + (size_t)c * n] = stage[(size_t)i * kLd + c];
    }
    if (nconv_min) *nconv_min = nc_min;
    if (refreshes) *refreshes = nref;
}

void pairs_score_impl(kt_context_s* ctx, int64_t n, int t, const double* lambda, const double* V, int64_t npairs,
                      const int64_t* pi, const int64_t* pj, double sign, double* score) {
    if (npairs == 0) return;
    std::vector<int> hpi(npairs), hpj(npairs);
    for (int64_t p = 0; p < npairs; ++p) {
        hpi[p] = (int)pi[p];
        hpj[p] = (int)pj[p];
    }
    KT_HIP(hipSetDevice(ctx->device));
    prof_recycle(ctx);
    const int nblocks = miobi_score_blocks(npairs, 0);
    DevMat dV;
    dV.alloc(ctx, n, kLd, false);
    Carver cv;
    const size_t oE = cv.take(sizeof(double) * kLd), oC = cv.take(sizeof(double) * kLd),
                 oPs = cv.take(sizeof(double) * kMiobiMaxBlocks),
                 oPk = cv.take(sizeof(unsigned long long) * kMiobiMaxBlocks),
                 oPi = cv.take(sizeof(int) * kMiobiMaxBlocks), oSc = cv.take(sizeof(double) * npairs),
                 oLi = cv.take(sizeof(int) * npairs), oLj = cv.take(sizeof(int) * npairs);
    Block blk;
    blk.alloc(ctx, cv.bytes);
    hipStream_t st = ctx->stream;
    std::vector<double> stage;
    upload_v(ctx, n, t, V, false, dV.col(0), stage);
    upload_e(ctx, t, lambda, blk.at<double>(oE), blk.at<double>(oC));
    KT_HIP(hipMemcpyAsync(blk.at<int>(oLi), hpi.data(), sizeof(int) * npairs, hipMemcpyHostToDevice, st));
    KT_HIP(hipMemcpyAsync(blk.at<int>(oLj), hpj.data(), sizeof(int) * npairs, hipMemcpyHostToDevice, st));
    prof_begin(ctx, PROF_MIOBI, st, t);
    KT_HIP(launch_miobi_score(npairs, t, dV.col(0), blk.at<double>(oC), blk.at<int>(oLi), blk.at<int>(oLj), nullptr,
                              sign, blk.at<double>(oSc), nblocks, blk.at<double>(oPs),
                              blk.at<unsigned long long>(oPk), blk.at<int>(oPi), nullptr, st));
    prof_end(ctx, PROF_MIOBI, st);
    KT_HIP(hipMemcpyAsync(score, blk.at<double>(oSc), sizeof(double) * npairs, hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
}

}  // namespace

}  // namespace kt

using namespace kt;

#define KT_MIOBI_GUARD_END                             \
    catch (const Status& s) {                          \
        set_error(s.msg);                              \
        return s.code;                                 \
    }                                                  \
    catch (const std::bad_alloc&) {                    \
        set_error("host allocation failed");           \
        return KT_ERR_ALLOC;                           \
    }                                                  \
    return KT_OK;

extern "C" int kt_pairs_score_topk(kt_context_t ctx, int64_t n, int t, const double* lambda, const double* V,
                                   int64_t npairs, const int64_t* pi, const int64_t* pj, double sign,
                                   double* score) {
    try {
        if (!ctx || !lambda || !V || (npairs > 0 && (!pi || !pj || !score)))
            fail(KT_ERR_ARG, "kt_pairs_score_topk: NULL argument");
        if (n < 1 || n > INT32_MAX || npairs < 0 || npairs > INT32_MAX)
            fail(KT_ERR_ARG, "kt_pairs_score_topk: n and npairs must fit 32-bit indices");
        if (t < 1 || t > kMiobiLd) fail(KT_ERR_ARG, "kt_pairs_score_topk: t must be in [1, 32]");
        for (int64_t p = 0; p < npairs; ++p)
            if (pi[p] < 0 || pi[p] >= n || pj[p] < 0 || pj[p] >= n)
                fail(KT_ERR_ARG, "kt_pairs_score_topk: pair index out of range");
        pairs_score_impl(ctx, n, t, lambda, V, npairs, pi, pj, sign, score);
    }
    KT_MIOBI_GUARD_END
}

extern "C" int kt_miobi_break(kt_matrix_t A, int k, int t, int refresh, int mode, double gap_rel, double tol,
                              int max_spmm, uint64_t seed, int64_t* sel_i, int64_t* sel_j, double* sel_score,
                              double* lambda_track, double* V_final, int64_t* nsel, int* nconv_min,
                              int* refreshes) {
    try {
        if (!A || !nsel || (k > 0 && (!sel_i || !sel_j || !sel_score)))
            fail(KT_ERR_ARG, "kt_miobi_break: NULL argument");
        if (k < 0) fail(KT_ERR_ARG, "kt_miobi_break: k must not be negative");
        if (t < 2 || t > kMiobiLd || t > A->n) fail(KT_ERR_ARG, "kt_miobi_break: t must be in [2, min(32, n)]");
        if (mode != 0 && mode != 1) fail(KT_ERR_ARG, "kt_miobi_break: mode must be 0 (reference) or 1 (paper)");
        if (!(gap_rel >= 0.0)) fail(KT_ERR_ARG, "kt_miobi_break: gap_rel must not be negative");
        require_symmetric(A, "MIOBI:: adjacency matrix has to be symmetric");
        if (A->ctx->ws.slq_submitted != A->ctx->ws.slq_collected)
            fail(KT_ERR_ARG, "kt_miobi_break: kt_slq_submit calls are outstanding on this context");
        miobi_break_impl(A, k, t, refresh, mode, gap_rel, tol, max_spmm, seed, sel_i, sel_j, sel_score, lambda_track,
                         V_final, nsel, nconv_min, refreshes);
    }
    KT_MIOBI_GUARD_END
}
