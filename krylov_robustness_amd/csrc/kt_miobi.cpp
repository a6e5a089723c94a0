// kt_miobi.cpp -- kt_miobi_break and kt_pairs_score_topk: MIOBI's top-t edge
// removal (MIOBIBreakEdge2.m / MIOBIBreakEdge2_weighted.m) with the step loop
// on the device (kernels in kt_miobi.hip); and kt_miobi_make,
// its edge addition (MIOBIMakeEdge.m), and kt_miobi_break_node
// with kt_nodes_score_topk, its node removal (MIOBIBreakNode.m; §4.2g), at the
// end of the file.
//
// A window is the run of steps between two eigenpair recomputations.  Its
// steps are queued back to back -- per step k_miobi_score over the pair list
// and k_miobi_pick (argmin, selection record, alive byte, eigenvalue shift);
// in `paper` mode also V <- V (I + S) by k_eig_rotate and the column
// normalisation -- and the selection list, eigenvalue track and stop flag are
// read back once, at the window's end.  A recomputation applies the window's
// removals to A through set_pairs and runs eigs_topk_impl on the edited matrix.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "kt_block.h"
#include "kt_krylov.h"
#include "kt_launch.h"
#include "kt_miobi_host.h"

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

// kt_miobi_make past its argument checks (MIOBIMakeEdge.m with t a parameter).
// Per window (the steps between two eigenpair recomputations): the eigenpairs,
// the candidate ranking by |V(:, 1)| and, for the mcap ranks the window can
// reach, the rows of V, node ids, degrees and adjacency bitmask go up; the
// window's steps (k_miobi_make_score, k_miobi_make_pick) are queued back to
// back; selections, scores, track rows, the m of every step and the state come
// back once, and the additions go into A through set_pairs.  The vectors stay
// as computed between recomputations (what the reference's update amounts to,
// §4.2e), so the ranking is the window's.  added_i / added_j: every pair handed
// to set_pairs so far (the caller removes them again on an error).
void miobi_make_impl(kt_matrix_s* A, int k, int t, int refresh, double tol, int max_spmm, uint64_t seed,
                     int64_t* sel_i, int64_t* sel_j, double* sel_score, double* track, int* cand_m, int64_t* nsel,
                     int* nconv_min, int* refreshes, std::vector<int64_t>& added_i, std::vector<int64_t>& added_j) {
    kt_context_s* ctx = A->ctx;
    const int64_t n = A->n;
    *nsel = 0;
    if (nconv_min) *nconv_min = t;
    if (refreshes) *refreshes = 0;
    if (track) std::fill(track, track + (size_t)(k + 1) * t, 0.0);
    if (cand_m) std::fill(cand_m, cand_m + k, 0);

    KT_HIP(hipSetDevice(ctx->device));
    prof_recycle(ctx);
    // host time by part (kt_context_stat 10-12)
    ctx->make_eig_us = ctx->make_rank_us = ctx->make_edit_us = 0;
    auto mark = std::chrono::steady_clock::now();
    const auto lap = [&mark](int64_t& into) {
        const auto now = std::chrono::steady_clock::now();
        into += std::chrono::duration_cast<std::chrono::microseconds>(now - mark).count();
        mark = now;
    };
    std::vector<double> lam(t), Vh((size_t)n * t), v0((size_t)n);
    int nconv = 0, nc_min;
    eigs_topk_impl(A, t, tol, max_spmm, seed, lam.data(), Vh.data(), nullptr, &nconv, nullptr);
    lap(ctx->make_eig_us);
    nc_min = nconv;
    if (track) std::copy(lam.begin(), lam.end(), track);

    // the maximum degree grows by at most one per step, so no window's mcap
    // exceeds min(maxdeg + 2 k, n): one allocation serves them all
    int maxdeg = miobi_max_degree(n, A->h_rowptr.data());
    const int kk = std::max(k, 1);
    const int64_t mcap_max = std::max(2, miobi_cap_m(maxdeg, k, k, n)), words_max = (mcap_max + 63) / 64;
    Carver cv;
    const size_t oE = cv.take(sizeof(double) * kLd), oC = cv.take(sizeof(double) * kLd),
                 oPs = cv.take(sizeof(double) * kMiobiMaxBlocks),
                 oPk = cv.take(sizeof(unsigned long long) * kMiobiMaxBlocks),
                 oPo = cv.take(sizeof(int) * kMiobiMaxBlocks), oSt = cv.take(sizeof(int) * 4),
                 oSi = cv.take(sizeof(int) * kk), oSj = cv.take(sizeof(int) * kk),
                 oSs = cv.take(sizeof(double) * kk), oCm = cv.take(sizeof(int) * kk),
                 oTr = cv.take(sizeof(double) * kLd * (kk + 1)), oW = cv.take(sizeof(double) * kLd * mcap_max),
                 oNd = cv.take(sizeof(int) * mcap_max), oDg = cv.take(sizeof(int) * mcap_max),
                 oMk = cv.take(sizeof(unsigned long long) * mcap_max * words_max);
    if (cv.bytes / 8 > (size_t)INT32_MAX)
        fail(KT_ERR_ALLOC, "kt_miobi_make: the candidate block's adjacency mask does not fit the pool");
    Block blk;
    blk.alloc(ctx, cv.bytes);
    double *dE = blk.at<double>(oE), *dC = blk.at<double>(oC), *dPs = blk.at<double>(oPs);
    double *dSs = blk.at<double>(oSs), *dTr = blk.at<double>(oTr), *dW = blk.at<double>(oW);
    unsigned long long *dPk = blk.at<unsigned long long>(oPk), *dMk = blk.at<unsigned long long>(oMk);
    int *dPo = blk.at<int>(oPo), *dSt = blk.at<int>(oSt), *dSi = blk.at<int>(oSi), *dSj = blk.at<int>(oSj);
    int *dCm = blk.at<int>(oCm), *dNd = blk.at<int>(oNd), *dDg = blk.at<int>(oDg);
    hipStream_t st = ctx->stream;
    KT_HIP(hipMemsetAsync(dTr, 0, sizeof(double) * kLd * (kk + 1), st));

    std::vector<int> hsi(kk), hsj(kk), hcm(kk), node, rank_of((size_t)n, -1), hdeg;
    std::vector<double> hss(kk), htr((size_t)kLd * (kk + 1)), hW;
    std::vector<uint64_t> hmask;
    std::vector<int64_t> ei, ej;
    int done = 0, nref = 0;
    while (done < k) {
        int w = k - done;
        if (refresh > 0) w = std::min(w, refresh - done % refresh);
        mark = std::chrono::steady_clock::now();
        // :49, :60-64  column 0 by absolute value, the ranking, the ranks in reach
        const int mcap = miobi_cap_m(maxdeg, k, w, n), words = miobi_make_words(mcap);
        for (int64_t i = 0; i < n; ++i) v0[(size_t)i] = std::fabs(Vh[(size_t)i]);
        miobi_rank(n, v0.data(), mcap, node);
        miobi_set_ranks(node, rank_of, true);
        miobi_build_mask(A->h_rowptr.data(), A->h_col.data(), node, rank_of, hmask, hdeg);
        hW.assign((size_t)mcap * kLd, 0.0);
        for (int a = 0; a < mcap; ++a)
            for (int c = 0; c < t; ++c) {
                const double x = Vh[(size_t)node[a] + (size_t)c * n];
                hW[(size_t)a * kLd + c] = c == 0 ? std::fabs(x) : x;
            }
        int hm = miobi_live_m(maxdeg, k, n), hmax = maxdeg;
        int state[4] = {done, 0, maxdeg, hm};
        KT_HIP(hipMemcpyAsync(dW, hW.data(), sizeof(double) * hW.size(), hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(dNd, node.data(), sizeof(int) * mcap, hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(dDg, hdeg.data(), sizeof(int) * mcap, hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(dMk, hmask.data(), sizeof(uint64_t) * (size_t)mcap * words, hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(dSt, state, sizeof state, hipMemcpyHostToDevice, st));
        upload_e(ctx, t, lam.data(), dE, dC);  // (synchronises: the host buffers above are free again)
        lap(ctx->make_rank_us);

        const int nblocks = miobi_make_blocks(mcap, 0);
        for (int s = 0; s < w; ++s) {
            prof_begin(ctx, PROF_MIOBI_MAKE, st, t);
            KT_HIP(launch_miobi_make_score(mcap, t, dW, dC, dMk, dSt, nullptr, nblocks, dPs, dPk, dPo, st));
            KT_HIP(launch_miobi_make_pick(nblocks, dPs, dPk, dPo, mcap, t, k, (int)n, dW, dNd, dE, dC, dMk, dDg, dSi,
                                          dSj, dSs, dTr, dCm, dSt, st));
            prof_end(ctx, PROF_MIOBI_MAKE, st);
        }
        KT_HIP(hipMemcpyAsync(state, dSt, sizeof state, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hsi.data() + done, dSi + done, sizeof(int) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hsj.data() + done, dSj + done, sizeof(int) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hss.data() + done, dSs + done, sizeof(double) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hcm.data() + done, dCm + done, sizeof(int) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(htr.data() + (size_t)kLd * (done + 1), dTr + (size_t)kLd * (done + 1),
                              sizeof(double) * kLd * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        const int now = state[0];
        if (now < done || now > done + w) fail(KT_ERR_HIP, "kt_miobi_make: the device step count is out of range");
        ei.clear();
        ej.clear();
        for (int s = done; s < now; ++s) {
            // the device's m bookkeeping replayed on the host
            const bool inside = hsi[s] >= 0 && hsi[s] < n && hsj[s] >= 0 && hsj[s] < hsi[s];
            const int a = inside ? rank_of[(size_t)hsi[s]] : -1, b = inside ? rank_of[(size_t)hsj[s]] : -1;
            if (a < 0 || b < 0) fail(KT_ERR_HIP, "kt_miobi_make: the device selected a pair outside the candidates");
            if (hcm[s] != hm) fail(KT_ERR_HIP, "kt_miobi_make: the device's candidate count differs from the host's");
            hm = miobi_book_step(hdeg, hmax, a, b, k, n);
            sel_i[s] = hsi[s];
            sel_j[s] = hsj[s];
            sel_score[s] = hss[s];
            if (cand_m) cand_m[s] = hcm[s];
            if (track) std::copy(htr.begin() + (size_t)kLd * (s + 1), htr.begin() + (size_t)kLd * (s + 1) + t,
                                 track + (size_t)(s + 1) * t);
            ei.push_back(hsi[s]);
            ej.push_back(hsj[s]);
        }
        miobi_set_ranks(node, rank_of, false);
        if (!ei.empty()) {
            added_i.insert(added_i.end(), ei.begin(), ei.end());
            added_j.insert(added_j.end(), ej.begin(), ej.end());
            mark = std::chrono::steady_clock::now();
            set_pairs(A, (int64_t)ei.size(), ei.data(), ej.data(), 1.0);
            lap(ctx->make_edit_us);
        }
        maxdeg = miobi_max_degree(n, A->h_rowptr.data());
        if (state[2] != hmax || maxdeg != hmax)
            fail(KT_ERR_HIP, "kt_miobi_make: the device's maximum degree differs from the host rows'");
        done = now;
        *nsel = done;
        if (state[1] || done >= k) break;
        // :326-331  the eigenpairs of the edited matrix
        mark = std::chrono::steady_clock::now();
        eigs_topk_impl(A, t, tol, max_spmm, seed, lam.data(), Vh.data(), nullptr, &nconv, nullptr);
        lap(ctx->make_eig_us);
        nc_min = std::min(nc_min, nconv);
        ++nref;
        if (track) std::copy(lam.begin(), lam.end(), track + (size_t)done * t);
    }
    if (nconv_min) *nconv_min = nc_min;
    if (refreshes) *refreshes = nref;
}

// the window's long-row list (rows longer than kMiobiNodeLong) on the device
int upload_long_rows(kt_matrix_s* A, int* dLr, std::vector<int>& rows) {
    miobi_long_rows(A->n, A->h_rowptr.data(), kMiobiNodeLong, rows);
    if (!rows.empty()) {
        KT_HIP(hipMemcpyAsync(dLr, rows.data(), sizeof(int) * rows.size(), hipMemcpyHostToDevice, A->ctx->stream));
        KT_HIP(hipStreamSynchronize(A->ctx->stream));
    }
    return (int)rows.size();
}

// kt_miobi_break_node past its argument checks (MIOBIBreakNode.m:176-297 with t
// and the threshold parameters).  Per window (the steps between two eigenpair
// recomputations): the eigenpairs go up, the column sums of V are formed
// (shift 0), and min(remaining, ceil(refresh / 2)) steps (k_miobi_node_score,
// k_miobi_node_pick) are queued back to back -- the device ends the window
// itself once the removed-entry count reaches `refresh`, and the launches
// queued past that point return at once.  Selections, scores, degrees, track
// rows and the state come back once; the host replays the count, clears the
// removed nodes' rows and columns in one pass over its CSR and drops the device
// copies.  edited: the host CSR was changed (the caller restores it on an error).
void miobi_break_node_impl(kt_matrix_s* A, int k, int t, int refresh, int shift, double tol, int max_spmm,
                           uint64_t seed, int64_t* sel, double* sel_score, int64_t* sel_deg, double* track,
                           int64_t* nsel, int* nconv_min, int* refreshes, bool& edited) {
    kt_context_s* ctx = A->ctx;
    const int64_t n = A->n;
    *nsel = 0;
    if (nconv_min) *nconv_min = t;
    if (refreshes) *refreshes = 0;
    if (track) std::fill(track, track + (size_t)(k + 1) * t, 0.0);
    if (A->nnz == 0) return;  // every node is isolated: nothing scores below +Inf

    KT_HIP(hipSetDevice(ctx->device));
    prof_recycle(ctx);
    ctx->make_eig_us = ctx->make_rank_us = ctx->make_edit_us = 0;
    auto mark = std::chrono::steady_clock::now();
    const auto lap = [&mark](int64_t& into) {
        const auto now = std::chrono::steady_clock::now();
        into += std::chrono::duration_cast<std::chrono::microseconds>(now - mark).count();
        mark = now;
    };
    std::vector<double> lam(t), Vh((size_t)n * t), stage;
    int nconv = 0, nc_min;
    eigs_topk_impl(A, t, tol, max_spmm, seed, lam.data(), Vh.data(), nullptr, &nconv, nullptr);
    lap(ctx->make_eig_us);
    nc_min = nconv;
    if (track) std::copy(lam.begin(), lam.end(), track);

    std::vector<int> long_rows;
    miobi_long_rows(n, A->h_rowptr.data(), kMiobiNodeLong, long_rows);  // rows only shrink: the most there will be
    const int nblocks = miobi_node_blocks(n, 0);
    const int kk = std::max(k, 1);
    DevMat dV;
    dV.alloc(ctx, n, kLd, false);
    Carver cv;
    const size_t oE = cv.take(sizeof(double) * kLd), oC = cv.take(sizeof(double) * kLd),
                 oS = cv.take(sizeof(double) * kLd), oNp = cv.take(sizeof(double) * kLd * miobi_norm_blocks(n)),
                 oPs = cv.take(sizeof(double) * kMiobiMaxBlocks), oPn = cv.take(sizeof(int) * kMiobiMaxBlocks),
                 oPd = cv.take(sizeof(int) * kMiobiMaxBlocks), oSt = cv.take(sizeof(int) * 4),
                 oSn = cv.take(sizeof(int) * kk), oSs = cv.take(sizeof(double) * kk),
                 oSd = cv.take(sizeof(int) * kk), oTr = cv.take(sizeof(double) * kLd * (kk + 1)),
                 oLr = cv.take(sizeof(int) * std::max<size_t>(long_rows.size(), 1)), oAl = cv.take((size_t)n);
    Block blk;
    blk.alloc(ctx, cv.bytes);
    double *dE = blk.at<double>(oE), *dC = blk.at<double>(oC), *dS = blk.at<double>(oS), *dNp = blk.at<double>(oNp);
    double *dPs = blk.at<double>(oPs), *dSs = blk.at<double>(oSs), *dTr = blk.at<double>(oTr);
    int *dPn = blk.at<int>(oPn), *dPd = blk.at<int>(oPd), *dSt = blk.at<int>(oSt), *dSn = blk.at<int>(oSn);
    int *dSd = blk.at<int>(oSd), *dLr = blk.at<int>(oLr);
    unsigned char* dAl = blk.at<unsigned char>(oAl);
    hipStream_t st = ctx->stream;
    KT_HIP(hipMemsetAsync(dAl, 1, (size_t)n, st));
    KT_HIP(hipMemsetAsync(dTr, 0, sizeof(double) * kLd * (kk + 1), st));
    KT_HIP(hipStreamSynchronize(st));

    std::vector<int> hsn(kk), hsd(kk);
    std::vector<double> hss(kk), htr((size_t)kLd * (kk + 1));
    std::vector<unsigned char> dead((size_t)n, 0);
    int done = 0, nref = 0, hacc = 0;
    while (done < k) {
        const int w = miobi_node_window(k - done, refresh);
        mark = std::chrono::steady_clock::now();
        const DevCSR& M = natural_csr(A);  // the edited matrix's copy
        const int n_long = upload_long_rows(A, dLr, long_rows);
        int state[4] = {done, 0, hacc, 0};
        KT_HIP(hipMemcpyAsync(dSt, state, sizeof state, hipMemcpyHostToDevice, st));
        upload_v(ctx, n, t, Vh.data(), true, dV.col(0), stage);  // :177  column 0 by absolute value
        upload_e(ctx, t, lam.data(), dE, dC);
        if (shift == 0) KT_HIP(launch_miobi_colsum(n, dV.col(0), dNp, dS, st));
        lap(ctx->make_rank_us);
        for (int s = 0; s < w; ++s) {
            prof_begin(ctx, PROF_MIOBI_NODE, st, t);
            KT_HIP(launch_miobi_node_score(n, t, dV.col(0), dC, M.rowptr, M.col, dAl, dLr, n_long, nullptr, nblocks,
                                           dPs, dPn, dPd, dSt, st));
            KT_HIP(launch_miobi_node_pick(nblocks, dPs, dPn, dPd, t, shift, refresh, dV.col(0), M.rowptr, M.col, dAl,
                                          dE, dC, dS, dSn, dSs, dSd, dTr, dSt, st));
            prof_end(ctx, PROF_MIOBI_NODE, st);
        }
        KT_HIP(hipMemcpyAsync(state, dSt, sizeof state, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hsn.data() + done, dSn + done, sizeof(int) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hsd.data() + done, dSd + done, sizeof(int) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(hss.data() + done, dSs + done, sizeof(double) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(htr.data() + (size_t)kLd * (done + 1), dTr + (size_t)kLd * (done + 1),
                              sizeof(double) * kLd * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        const int now = state[0];
        if (now < done || now > done + w)
            fail(KT_ERR_HIP, "kt_miobi_break_node: the device step count is out of range");
        bool ended = false;
        for (int s = done; s < now; ++s) {
            const int r = hsn[s], d = hsd[s];
            if (r < 0 || r >= n || dead[(size_t)r] || d < 1 || d > A->h_rowptr[r + 1] - A->h_rowptr[r] || ended)
                fail(KT_ERR_HIP, "kt_miobi_break_node: the device's selection record is inconsistent");
            ended = miobi_node_book(hacc, d, refresh);
            dead[(size_t)r] = 1;
            sel[s] = r;
            sel_score[s] = hss[s];
            sel_deg[s] = d;
            if (track) std::copy(htr.begin() + (size_t)kLd * (s + 1), htr.begin() + (size_t)kLd * (s + 1) + t,
                                 track + (size_t)(s + 1) * t);
        }
        if ((refresh > 0 && state[2] != hacc) || (state[3] != 0) != ended)
            fail(KT_ERR_HIP, "kt_miobi_break_node: the device's removed-entry count differs from the host's");
        if (now > done) {  // :211-212 for the window's nodes
            mark = std::chrono::steady_clock::now();
            edited = true;
            miobi_clear_nodes(n, dead, A->h_rowptr, A->h_col, A->h_val);
            A->nnz = (int64_t)A->h_col.size();
            refresh_device(A);
            lap(ctx->make_edit_us);
        }
        done = now;
        *nsel = done;
        if (state[1] || done >= k || A->nnz == 0) break;  // (an empty matrix has nothing left to score)
        if (!ended) fail(KT_ERR_HIP, "kt_miobi_break_node: a full window did not reach its end");
        // :286-295  the eigenpairs of the edited matrix
        mark = std::chrono::steady_clock::now();
        eigs_topk_impl(A, t, tol, max_spmm, seed, lam.data(), Vh.data(), nullptr, &nconv, nullptr);
        lap(ctx->make_eig_us);
        nc_min = std::min(nc_min, nconv);
        ++nref;
        if (track) std::copy(lam.begin(), lam.end(), track + (size_t)done * t);
    }
    if (nconv_min) *nconv_min = nc_min;
    if (refreshes) *refreshes = nref;
}

void nodes_score_impl(kt_matrix_s* A, int t, const double* lambda, const double* V, double* score) {
    kt_context_s* ctx = A->ctx;
    const int64_t n = A->n;
    KT_HIP(hipSetDevice(ctx->device));
    prof_recycle(ctx);
    const DevCSR& M = natural_csr(A);
    std::vector<int> long_rows;
    miobi_long_rows(n, A->h_rowptr.data(), kMiobiNodeLong, long_rows);
    const int nblocks = miobi_node_blocks(n, 0);
    DevMat dV;
    dV.alloc(ctx, n, kLd, false);
    Carver cv;
    const size_t oE = cv.take(sizeof(double) * kLd), oC = cv.take(sizeof(double) * kLd),
                 oPs = cv.take(sizeof(double) * kMiobiMaxBlocks), oPn = cv.take(sizeof(int) * kMiobiMaxBlocks),
                 oPd = cv.take(sizeof(int) * kMiobiMaxBlocks), oSc = cv.take(sizeof(double) * n),
                 oLr = cv.take(sizeof(int) * std::max<size_t>(long_rows.size(), 1)), oAl = cv.take((size_t)n);
    Block blk;
    blk.alloc(ctx, cv.bytes);
    hipStream_t st = ctx->stream;
    std::vector<double> stage;
    KT_HIP(hipMemsetAsync(blk.at<unsigned char>(oAl), 1, (size_t)n, st));
    const int n_long = upload_long_rows(A, blk.at<int>(oLr), long_rows);
    upload_v(ctx, n, t, V, false, dV.col(0), stage);
    upload_e(ctx, t, lambda, blk.at<double>(oE), blk.at<double>(oC));
    prof_begin(ctx, PROF_MIOBI_NODE, st, t);
    KT_HIP(launch_miobi_node_score(n, t, dV.col(0), blk.at<double>(oC), M.rowptr, M.col, blk.at<unsigned char>(oAl),
                                   blk.at<int>(oLr), n_long, blk.at<double>(oSc), nblocks, blk.at<double>(oPs),
                                   blk.at<int>(oPn), blk.at<int>(oPd), nullptr, st));
    prof_end(ctx, PROF_MIOBI_NODE, st);
    KT_HIP(hipMemcpyAsync(score, blk.at<double>(oSc), sizeof(double) * n, hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
}

// what both node entries require of A (MIOBIBreakNode.m:31-39 binarises its
// input; its datasets have no self-loop)
void node_matrix_checks(kt_matrix_s* A, const char* who) {
    const std::string w(who);
    if (A->n > INT32_MAX) fail(KT_ERR_ARG, (w + ": n must fit 32-bit indices").c_str());
    if (A->nnz > 0 && !A->unit_values)
        fail(KT_ERR_ARG, (w + ": the matrix must be a unit-weight adjacency matrix (MIOBIBreakNode.m binarises "
                              "its input)").c_str());
    if (miobi_has_diagonal(A->n, A->h_rowptr.data(), A->h_col.data()))
        fail(KT_ERR_ARG, (w + ": the matrix must have a zero diagonal").c_str());
    if (A->ctx->ws.slq_submitted != A->ctx->ws.slq_collected)
        fail(KT_ERR_ARG, (w + ": kt_slq_submit calls are outstanding on this context").c_str());
    require_symmetric(A, "MIOBI:: adjacency matrix has to be symmetric");
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

extern "C" int kt_miobi_make(kt_matrix_t A, int k, int t, int refresh, double tol, int max_spmm, uint64_t seed,
                             int64_t* sel_i, int64_t* sel_j, double* sel_score, double* lambda_track, int* cand_m,
                             int64_t* nsel, int* nconv_min, int* refreshes) {
    std::vector<int64_t> added_i, added_j;
    try {
        try {
            if (!A || !nsel || (k > 0 && (!sel_i || !sel_j || !sel_score)))
                fail(KT_ERR_ARG, "kt_miobi_make: NULL argument");
            if (k < 0) fail(KT_ERR_ARG, "kt_miobi_make: k must not be negative");
            if (t < 2 || t > kMiobiLd || t > A->n) fail(KT_ERR_ARG, "kt_miobi_make: t must be in [2, min(32, n)]");
            if (A->nnz == 0 || !A->unit_values)
                fail(KT_ERR_ARG, "kt_miobi_make: the matrix must be a unit-weight adjacency matrix with at least one "
                                 "edge (MIOBIMakeEdge.m binarises its input)");
            if (A->ctx->ws.slq_submitted != A->ctx->ws.slq_collected)
                fail(KT_ERR_ARG, "kt_miobi_make: kt_slq_submit calls are outstanding on this context");
            require_symmetric(A, "MIOBI:: adjacency matrix has to be symmetric");
            miobi_make_impl(A, k, t, refresh, tol, max_spmm, seed, sel_i, sel_j, sel_score, lambda_track, cand_m, nsel,
                            nconv_min, refreshes, added_i, added_j);
        } catch (...) {
            // on any error the matrix stays as it was: the pairs added so far were non-adjacent
            if (!added_i.empty()) {
                try {
                    set_pairs(A, (int64_t)added_i.size(), added_i.data(), added_j.data(), 0.0);
                } catch (...) {
                }
                *nsel = 0;
            }
            throw;
        }
    }
    KT_MIOBI_GUARD_END
}

extern "C" int kt_nodes_score_topk(kt_matrix_t A, int t, const double* lambda, const double* V, double* score) {
    try {
        if (!A || !lambda || !V || !score) fail(KT_ERR_ARG, "kt_nodes_score_topk: NULL argument");
        if (t < 1 || t > kMiobiLd) fail(KT_ERR_ARG, "kt_nodes_score_topk: t must be in [1, 32]");
        node_matrix_checks(A, "kt_nodes_score_topk");
        nodes_score_impl(A, t, lambda, V, score);
    }
    KT_MIOBI_GUARD_END
}

extern "C" int kt_miobi_break_node(kt_matrix_t A, int k, int t, int refresh, int shift, double tol, int max_spmm,
                                   uint64_t seed, int64_t* sel, double* sel_score, int64_t* sel_deg,
                                   double* lambda_track, int64_t* nsel, int* nconv_min, int* refreshes) {
    std::vector<int64_t> rowptr0;
    std::vector<int32_t> col0;
    bool edited = false;
    try {
        try {
            if (!A || !nsel || (k > 0 && (!sel || !sel_score || !sel_deg)))
                fail(KT_ERR_ARG, "kt_miobi_break_node: NULL argument");
            if (k < 0) fail(KT_ERR_ARG, "kt_miobi_break_node: k must not be negative");
            if (t < 2 || t > kMiobiLd || t > A->n)
                fail(KT_ERR_ARG, "kt_miobi_break_node: t must be in [2, min(32, n)]");
            if (shift != 0 && shift != 1)
                fail(KT_ERR_ARG, "kt_miobi_break_node: shift must be 0 (reference) or 1 (first_order)");
            node_matrix_checks(A, "kt_miobi_break_node");
            rowptr0 = A->h_rowptr;  // unit weights: the pattern is the matrix
            col0 = A->h_col;
            miobi_break_node_impl(A, k, t, refresh, shift, tol, max_spmm, seed, sel, sel_score, sel_deg, lambda_track,
                                  nsel, nconv_min, refreshes, edited);
        } catch (...) {
            // on any error the matrix stays as it was
            if (edited) {
                A->h_rowptr = rowptr0;
                A->h_col = col0;
                A->h_val.assign(col0.size(), 1.0);
                A->nnz = (int64_t)col0.size();
                refresh_device(A);
                *nsel = 0;
            }
            throw;
        }
    }
    KT_MIOBI_GUARD_END
}
