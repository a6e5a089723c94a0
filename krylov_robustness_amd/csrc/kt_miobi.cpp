// kt_miobi.cpp -- kt_miobi_break and kt_pairs_score_topk: MIOBI's top-t edge
// removal (MIOBIBreakEdge2.m / MIOBIBreakEdge2_weighted.m) with the step loop
// on the device (kernels in kt_miobi.hip); kt_miobi_make, its
// edge addition (MIOBIMakeEdge.m); and kt_miobi_break_node
// with kt_nodes_score_topk, its node removal (MIOBIBreakNode.m; §4.2g).
//
// A window is the run of steps between two eigenpair recomputations.  The
// three drivers share one window loop (Run::windows): what the variant needs
// goes up, the window's steps are queued back to back, the selection record
// (Selection) is read back once at the window's end, the variant replays it
// and edits A, and eigs_topk_impl runs on the edited matrix.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "kt_block.h"
#include "kt_krylov.h"
#include "kt_launch.h"
#include "kt_miobi_host.h"

namespace kt {

namespace {

constexpr int kLd = kMiobiLd;

// One pooled device block cut into 256-byte aligned slices: take() them all,
// then alloc(); a Slice converts to its address from then on.  The order of
// the takes is the layout.
struct Block {
    template <class T>
    struct Slice {
        const Block* b = nullptr;
        size_t off = 0;
        operator T*() const { return reinterpret_cast<T*>(static_cast<char*>(b->m.ptr) + off); }
    };
    size_t bytes = 0;
    DevMat m;
    template <class T>
    Slice<T> take(size_t count) {
        const size_t off = bytes;
        bytes += (sizeof(T) * count + 255) / 256 * 256;
        return {this, off};
    }
    void alloc(kt_context_s* ctx) { m.alloc(ctx, 1, (int)((bytes + 7) / 8), false); }
};
using Doubles = Block::Slice<double>;
using Ints = Block::Slice<int>;
using Keys = Block::Slice<unsigned long long>;
using Bytes = Block::Slice<unsigned char>;

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

// The selection record of a run, slices of the variant's block mirrored on the
// host: four state words (0 the step count, 1 the stop flag, 2 and 3 the
// variant's), ncols <= 3 integer columns and the score column of max(k, 1)
// rows, and k + 1 track rows of 32 eigenvalues.
struct Selection {
    const std::string who;  // the entry's name, for the error message
    const int kk, t, ncols;
    Ints dSt, dCol[3];
    Doubles dSs, dTr;
    int state[4] = {0, 0, 0, 0};
    std::vector<int> col[3];
    std::vector<double> score, tr;

    Selection(const char* who_, int k, int t_, int ncols_, Block& blk)
        : who(who_), kk(std::max(k, 1)), t(t_), ncols(ncols_), score(kk), tr((size_t)kLd * (kk + 1)) {
        dSt = blk.take<int>(4);
        for (int c = 0; c < ncols; ++c) {
            dCol[c] = blk.take<int>(kk);
            col[c].resize(kk);
        }
        dSs = blk.take<double>(kk);
        dTr = blk.take<double>((size_t)kLd * (kk + 1));
    }

    // (once the block is allocated) the track rows start as zeros
    void clear(hipStream_t st) { KT_HIP(hipMemsetAsync(dTr, 0, sizeof(double) * kLd * (kk + 1), st)); }

    // The rows [done, done + w) of a window that has been queued on st, and the
    // state words.  Returns the device's step count; the track rows of the steps
    // it took go to `track` (row s + 1 for step s).
    int fetch(hipStream_t st, int done, int w, double* track) {
        const size_t row = (size_t)kLd * (done + 1);
        KT_HIP(hipMemcpyAsync(state, dSt, sizeof state, hipMemcpyDeviceToHost, st));
        for (int c = 0; c < ncols; ++c)
            KT_HIP(hipMemcpyAsync(&col[c][done], dCol[c] + done, sizeof(int) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(&score[done], dSs + done, sizeof(double) * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipMemcpyAsync(&tr[row], dTr + row, sizeof(double) * kLd * w, hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        const int now = state[0];
        if (!miobi_step_in_window(now, done, w)) fail(KT_ERR_HIP, who + ": the device step count is out of range");
        for (int s = done; track && s < now; ++s)
            std::copy_n(&tr[(size_t)kLd * (s + 1)], t, track + (size_t)(s + 1) * t);
        return now;
    }
};

// One MIOBI run: the arguments the three drivers share, the eigenpairs of the
// current matrix, the step count, and the stopwatch behind kt_context_stat
// 10-12 (host time by part: the eigensolver, the staging, the edits of A).
struct Run {
    kt_matrix_s* A;
    kt_context_s* ctx;
    int64_t n;
    int k, t, refresh, max_spmm;
    double tol;
    uint64_t seed;
    double* track;  // the caller's outputs
    int64_t* nsel;
    int *nconv_min, *refreshes;
    std::vector<double> lam, Vh;
    int done = 0, nref = 0, nc_min = INT_MAX;
    std::chrono::steady_clock::time_point mark;

    // the outputs of a run that takes no step
    void zero() {
        *nsel = 0;
        if (nconv_min) *nconv_min = t;
        if (refreshes) *refreshes = 0;
        if (track) std::fill(track, track + (size_t)(k + 1) * t, 0.0);
    }
    void start() { mark = std::chrono::steady_clock::now(); }
    void lap(int64_t& into) {
        const auto now = std::chrono::steady_clock::now();
        into += std::chrono::duration_cast<std::chrono::microseconds>(now - mark).count();
        mark = now;
    }

    // the eigenpairs of the matrix as it is now, timed from the last start();
    // their values are track row `done`
    void eig() {
        int nconv = 0;
        eigs_topk_impl(A, t, tol, max_spmm, seed, lam.data(), Vh.data(), nullptr, &nconv, nullptr);
        lap(ctx->make_eig_us);
        nc_min = std::min(nc_min, nconv);
        if (track) std::copy(lam.begin(), lam.end(), track + (size_t)done * t);
    }

    void begin() {
        KT_HIP(hipSetDevice(ctx->device));
        prof_recycle(ctx);
        ctx->make_eig_us = ctx->make_rank_us = ctx->make_edit_us = 0;
        start();  // (stat 10 has always included the eigenvector buffer's allocation)
        lam.resize(t);
        Vh.resize((size_t)n * t);
        eig();
    }

    // The window loop.  window(): the steps to queue for the window that starts
    // at `done`.  stage(w): what the window's steps read goes up.  step(): one
    // step's launches (one interval of profile id prof).  commit(now): the
    // fetched rows [done, now) validated and replayed, the caller's arrays
    // written, A edited; returns whether the run ends here.
    template <class Window, class Stage, class Step, class Commit>
    void windows(Selection& sel, int prof, Window window, Stage stage, Step step, Commit commit) {
        hipStream_t st = ctx->stream;
        while (done < k) {
            const int w = window();
            start();
            stage(w);
            lap(ctx->make_rank_us);
            for (int s = 0; s < w; ++s) {
                prof_begin(ctx, prof, st, t);
                step();
                prof_end(ctx, prof, st);
            }
            const int now = sel.fetch(st, done, w, track);
            const bool ends = commit(now);
            done = now;
            *nsel = done;
            if (ends || done >= k) break;
            start();
            eig();  // MIOBIBreakEdge2.m:255-261, MIOBIMakeEdge.m:326-331, MIOBIBreakNode.m:286-295
            ++nref;
        }
        if (nconv_min) *nconv_min = nc_min;
        if (refreshes) *refreshes = nref;
    }

    // a window's pairs set to `value` in A (the edge drivers' edit)
    void set_edges(const std::vector<int64_t>& ei, const std::vector<int64_t>& ej, double value) {
        if (ei.empty()) return;
        start();
        set_pairs(A, (int64_t)ei.size(), ei.data(), ej.data(), value);
        lap(ctx->make_edit_us);
    }
};

// kt_miobi_break past its argument checks.  Stage: V and the eigenvalues.
// Step: k_miobi_score over the pair list and k_miobi_pick (argmin, selection
// record, alive byte, eigenvalue shift); in `paper` mode also V <- V (I + S) by
// k_eig_rotate and the column normalisation.  Commit: set_pairs.
void miobi_break_impl(Run& r, int mode, double gap_rel, int64_t* sel_i, int64_t* sel_j, double* sel_score,
                      double* V_final) {
    kt_matrix_s* A = r.A;
    kt_context_s* ctx = r.ctx;
    const int64_t n = r.n;
    const int t = r.t;
    r.zero();
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
    const int64_t npairs = (int64_t)hpi.size(), cap = std::max<int64_t>(npairs, 1);
    r.begin();

    const int nblocks = miobi_score_blocks(npairs, 0);
    DevMat dV;
    dV.alloc(ctx, n, kLd, false);
    Block blk;
    const Doubles dE = blk.take<double>(kLd), dC = blk.take<double>(kLd), dM = blk.take<double>(kLd * kLd),
                  dPs = blk.take<double>(kMiobiMaxBlocks);
    const Keys dPk = blk.take<unsigned long long>(kMiobiMaxBlocks);
    const Ints dPi = blk.take<int>(kMiobiMaxBlocks);
    const Doubles dNp = blk.take<double>((size_t)kLd * miobi_norm_blocks(n));
    Selection sel("kt_miobi_break", r.k, t, 2, blk);  // columns: i, j
    const Ints dLi = blk.take<int>(cap), dLj = blk.take<int>(cap);
    const Doubles sLw = blk.take<double>(cap);
    const Bytes dAl = blk.take<unsigned char>(cap);
    blk.alloc(ctx);
    double* dLw = weighted ? (double*)sLw : nullptr;
    hipStream_t st = ctx->stream;
    if (npairs) {
        KT_HIP(hipMemcpyAsync(dLi, hpi.data(), sizeof(int) * npairs, hipMemcpyHostToDevice, st));
        KT_HIP(hipMemcpyAsync(dLj, hpj.data(), sizeof(int) * npairs, hipMemcpyHostToDevice, st));
        if (weighted) KT_HIP(hipMemcpyAsync(dLw, hwt.data(), sizeof(double) * npairs, hipMemcpyHostToDevice, st));
        KT_HIP(hipMemsetAsync(dAl, 1, (size_t)npairs, st));
    }
    sel.clear(st);
    KT_HIP(hipMemsetAsync(sel.dSt, 0, sizeof(int) * 4, st));  // the steps count on from the device's own word
    KT_HIP(hipStreamSynchronize(st));

    std::vector<double> stage;
    std::vector<int64_t> ei, ej;
    const auto upload = [&](int) {
        upload_v(ctx, n, t, r.Vh.data(), true, dV.col(0), stage);
        upload_e(ctx, t, r.lam.data(), dE, dC);
    };
    if (r.k == 0) upload(0);  // no window will: V_final is read from dV
    r.windows(
        sel, PROF_MIOBI, [&] { return miobi_edge_window(r.k - r.done, r.done, r.refresh); }, upload,
        [&] {
            KT_HIP(launch_miobi_score(npairs, t, dV.col(0), dC, dLi, dLj, dAl, -2.0, nullptr, nblocks, dPs, dPk, dPi,
                                      sel.dSt + 1, st));
            KT_HIP(launch_miobi_pick(nblocks, dPs, dPk, dPi, t, mode, gap_rel, dV.col(0), dE, dC, dLi, dLj, dLw, dAl,
                                     sel.dCol[0], sel.dCol[1], sel.dSs, sel.dTr, dM, sel.dSt, st));
            if (mode) {  // after the stop M = I: the rotation leaves V as it is
                KT_HIP(launch_eig_rotate(n, kLd, kLd, dV.col(0), kLd, dM, st));
                KT_HIP(launch_miobi_normalise(n, dV.col(0), dNp, sel.dSt, st));
            }
        },
        [&](int now) {
            ei.assign(sel.col[0].begin() + r.done, sel.col[0].begin() + now);
            ej.assign(sel.col[1].begin() + r.done, sel.col[1].begin() + now);
            std::copy(ei.begin(), ei.end(), sel_i + r.done);
            std::copy(ej.begin(), ej.end(), sel_j + r.done);
            std::copy(sel.score.begin() + r.done, sel.score.begin() + now, sel_score + r.done);
            r.set_edges(ei, ej, 0.0);
            return sel.state[1] || A->nnz == 0;  // (an empty matrix has nothing left to score)
        });
    if (V_final) {
        stage.resize((size_t)n * kLd);
        KT_HIP(hipMemcpyAsync(stage.data(), dV.col(0), sizeof(double) * stage.size(), hipMemcpyDeviceToHost, st));
        KT_HIP(hipStreamSynchronize(st));
        for (int c = 0; c < t; ++c)
            for (int64_t i = 0; i < n; ++i) V_final[i + (size_t)c * n] = stage[(size_t)i * kLd + c];
    }
}

// The score-only entries (kt_pairs_score_topk, kt_nodes_score_topk).  blk: the
// entry's own slices taken; the scratch both need (e, c = exp(e), the score
// partials, `count` scores) is taken after them.  upload() sends what the
// entry adds, V and e go up, launch(dV, dC, dSc, dPs) is the entry's one
// launch, inside an interval of profile id prof, and the scores come back.
template <class Upload, class Launch>
void score_once(kt_context_s* ctx, Block& blk, int64_t n, int t, const double* lambda, const double* V, int prof,
                int64_t count, double* score, Upload upload, Launch launch) {
    KT_HIP(hipSetDevice(ctx->device));
    prof_recycle(ctx);
    DevMat dV;
    dV.alloc(ctx, n, kLd, false);
    const Doubles dE = blk.take<double>(kLd), dC = blk.take<double>(kLd), dPs = blk.take<double>(kMiobiMaxBlocks),
                  dSc = blk.take<double>(count);
    blk.alloc(ctx);
    hipStream_t st = ctx->stream;
    std::vector<double> stage;
    upload();
    upload_v(ctx, n, t, V, false, dV.col(0), stage);
    upload_e(ctx, t, lambda, dE, dC);
    prof_begin(ctx, prof, st, t);
    KT_HIP(launch(dV.col(0), dC, dSc, dPs));
    prof_end(ctx, prof, st);
    KT_HIP(hipMemcpyAsync(score, dSc, sizeof(double) * count, hipMemcpyDeviceToHost, st));
    KT_HIP(hipStreamSynchronize(st));
}

void pairs_score_impl(kt_context_s* ctx, int64_t n, int t, const double* lambda, const double* V, int64_t npairs,
                      const int64_t* pi, const int64_t* pj, double sign, double* score) {
    if (npairs == 0) return;
    const std::vector<int> hpi(pi, pi + npairs), hpj(pj, pj + npairs);
    const int nblocks = miobi_score_blocks(npairs, 0);
    hipStream_t st = ctx->stream;
    Block blk;
    const Keys dPk = blk.take<unsigned long long>(kMiobiMaxBlocks);
    const Ints dPi = blk.take<int>(kMiobiMaxBlocks), dLi = blk.take<int>(npairs), dLj = blk.take<int>(npairs);
    score_once(
        ctx, blk, n, t, lambda, V, PROF_MIOBI, npairs, score,
        [&] {
            KT_HIP(hipMemcpyAsync(dLi, hpi.data(), sizeof(int) * npairs, hipMemcpyHostToDevice, st));
            KT_HIP(hipMemcpyAsync(dLj, hpj.data(), sizeof(int) * npairs, hipMemcpyHostToDevice, st));
        },
        [&](double* dV, double* dC, double* dSc, double* dPs) {
            return launch_miobi_score(npairs, t, dV, dC, dLi, dLj, nullptr, sign, dSc, nblocks, dPs, dPk, dPi, nullptr,
                                      st);
        });
}

// kt_miobi_make past its argument checks (MIOBIMakeEdge.m with t a parameter).
// Stage: the candidate ranking by |V(:, 1)| and, for the mcap ranks the window
// can reach, the rows of V, node ids, degrees and adjacency bitmask.  Step:
// k_miobi_make_score, k_miobi_make_pick.  Commit: the additions go into A
// through set_pairs.  The vectors stay as computed between recomputations
// (§4.2e), so the ranking is the window's.  added_i / added_j: every pair
// handed to set_pairs so far (the caller removes them again on an error).
void miobi_make_impl(Run& r, int64_t* sel_i, int64_t* sel_j, double* sel_score, int* cand_m,
                     std::vector<int64_t>& added_i, std::vector<int64_t>& added_j) {
    kt_matrix_s* A = r.A;
    kt_context_s* ctx = r.ctx;
    const int64_t n = r.n;
    const int k = r.k, t = r.t;
    r.zero();
    if (cand_m) std::fill(cand_m, cand_m + k, 0);
    r.begin();

    // the maximum degree grows by at most one per step, so no window's mcap
    // exceeds min(maxdeg + 2 k, n): one allocation serves them all
    int maxdeg = miobi_max_degree(n, A->h_rowptr.data());
    const size_t mcap_max = std::max(2, miobi_cap_m(maxdeg, k, k, n)), words_max = (mcap_max + 63) / 64;
    Block blk;
    const Doubles dE = blk.take<double>(kLd), dC = blk.take<double>(kLd), dPs = blk.take<double>(kMiobiMaxBlocks);
    const Keys dPk = blk.take<unsigned long long>(kMiobiMaxBlocks);
    const Ints dPo = blk.take<int>(kMiobiMaxBlocks);
    Selection sel("kt_miobi_make", k, t, 3, blk);  // columns: i, j, the candidate count m
    const Doubles dW = blk.take<double>(kLd * mcap_max);
    const Ints dNd = blk.take<int>(mcap_max), dDg = blk.take<int>(mcap_max);
    const Keys dMk = blk.take<unsigned long long>(mcap_max * words_max);
    if (blk.bytes / 8 > (size_t)INT32_MAX)
        fail(KT_ERR_ALLOC, "kt_miobi_make: the candidate block's adjacency mask does not fit the pool");
    blk.alloc(ctx);
    hipStream_t st = ctx->stream;
    sel.clear(st);

    std::vector<int> node, rank_of((size_t)n, -1), hdeg;
    std::vector<double> v0((size_t)n), hW;
    std::vector<uint64_t> hmask;
    std::vector<int64_t> ei, ej;
    int mcap = 0, nblocks = 0, hm = 0, hmax = 0;  // of the current window
    r.windows(
        sel, PROF_MIOBI_MAKE, [&] { return miobi_edge_window(k - r.done, r.done, r.refresh); },
        [&](int w) {
            // :49, :60-64  column 0 by absolute value, the ranking, the ranks in reach
            mcap = miobi_cap_m(maxdeg, k, w, n);
            nblocks = miobi_make_blocks(mcap, 0);
            const int words = miobi_make_words(mcap);
            for (int64_t i = 0; i < n; ++i) v0[(size_t)i] = std::fabs(r.Vh[(size_t)i]);
            miobi_rank(n, v0.data(), mcap, node);
            miobi_set_ranks(node, rank_of, true);
            miobi_build_mask(A->h_rowptr.data(), A->h_col.data(), node, rank_of, hmask, hdeg);
            hW.assign((size_t)mcap * kLd, 0.0);
            for (int a = 0; a < mcap; ++a)
                for (int c = 0; c < t; ++c) {
                    const double x = r.Vh[(size_t)node[a] + (size_t)c * n];
                    hW[(size_t)a * kLd + c] = c == 0 ? std::fabs(x) : x;
                }
            hm = miobi_live_m(maxdeg, k, n);
            hmax = maxdeg;
            const int state[4] = {r.done, 0, maxdeg, hm};
            KT_HIP(hipMemcpyAsync(dW, hW.data(), sizeof(double) * hW.size(), hipMemcpyHostToDevice, st));
            KT_HIP(hipMemcpyAsync(dNd, node.data(), sizeof(int) * mcap, hipMemcpyHostToDevice, st));
            KT_HIP(hipMemcpyAsync(dDg, hdeg.data(), sizeof(int) * mcap, hipMemcpyHostToDevice, st));
            KT_HIP(hipMemcpyAsync(dMk, hmask.data(), sizeof(uint64_t) * (size_t)mcap * words, hipMemcpyHostToDevice,
                                  st));
            KT_HIP(hipMemcpyAsync(sel.dSt, state, sizeof state, hipMemcpyHostToDevice, st));
            upload_e(ctx, t, r.lam.data(), dE, dC);  // (synchronises: the host buffers above are free again)
        },
        [&] {
            KT_HIP(launch_miobi_make_score(mcap, t, dW, dC, dMk, sel.dSt, nullptr, nblocks, dPs, dPk, dPo, st));
            KT_HIP(launch_miobi_make_pick(nblocks, dPs, dPk, dPo, mcap, t, k, (int)n, dW, dNd, dE, dC, dMk, dDg,
                                          sel.dCol[0], sel.dCol[1], sel.dSs, sel.dTr, sel.dCol[2], sel.dSt, st));
        },
        [&](int now) {
            const std::vector<int>&hsi = sel.col[0], &hsj = sel.col[1], &hcm = sel.col[2];
            ei.clear();
            ej.clear();
            for (int s = r.done; s < now; ++s) {
                // the device's m bookkeeping replayed on the host
                const bool inside = hsi[s] >= 0 && hsi[s] < n && hsj[s] >= 0 && hsj[s] < hsi[s];
                const int a = inside ? rank_of[(size_t)hsi[s]] : -1, b = inside ? rank_of[(size_t)hsj[s]] : -1;
                if (a < 0 || b < 0)
                    fail(KT_ERR_HIP, "kt_miobi_make: the device selected a pair outside the candidates");
                if (hcm[s] != hm)
                    fail(KT_ERR_HIP, "kt_miobi_make: the device's candidate count differs from the host's");
                hm = miobi_book_step(hdeg, hmax, a, b, k, n);
                sel_i[s] = hsi[s];
                sel_j[s] = hsj[s];
                sel_score[s] = sel.score[s];
                if (cand_m) cand_m[s] = hcm[s];
                ei.push_back(hsi[s]);
                ej.push_back(hsj[s]);
            }
            miobi_set_ranks(node, rank_of, false);
            added_i.insert(added_i.end(), ei.begin(), ei.end());
            added_j.insert(added_j.end(), ej.begin(), ej.end());
            r.set_edges(ei, ej, 1.0);
            maxdeg = miobi_max_degree(n, A->h_rowptr.data());
            if (sel.state[2] != hmax || maxdeg != hmax)
                fail(KT_ERR_HIP, "kt_miobi_make: the device's maximum degree differs from the host rows'");
            return sel.state[1] != 0;
        });
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
// and the threshold parameters).  Stage: the eigenpairs, the column sums of V
// (shift 0).  Step: k_miobi_node_score, k_miobi_node_pick -- the device ends
// the window itself once the removed-entry count reaches `refresh`, and the
// launches queued past that point return at once.  Commit: the count replayed,
// the removed nodes' rows and columns cleared in one pass over the host CSR,
// the device copies dropped.  edited: the host CSR was changed (the caller
// restores it on an error).
void miobi_break_node_impl(Run& r, int shift, int64_t* sel_n, double* sel_score, int64_t* sel_deg, bool& edited) {
    kt_matrix_s* A = r.A;
    kt_context_s* ctx = r.ctx;
    const int64_t n = r.n;
    const int t = r.t, refresh = r.refresh;
    r.zero();
    if (A->nnz == 0) return;  // every node is isolated: nothing scores below +Inf
    r.begin();

    std::vector<int> long_rows;
    miobi_long_rows(n, A->h_rowptr.data(), kMiobiNodeLong, long_rows);  // rows only shrink: the most there will be
    const int nblocks = miobi_node_blocks(n, 0);
    DevMat dV;
    dV.alloc(ctx, n, kLd, false);
    Block blk;
    const Doubles dE = blk.take<double>(kLd), dC = blk.take<double>(kLd), dS = blk.take<double>(kLd),
                  dNp = blk.take<double>((size_t)kLd * miobi_norm_blocks(n)), dPs = blk.take<double>(kMiobiMaxBlocks);
    const Ints dPn = blk.take<int>(kMiobiMaxBlocks), dPd = blk.take<int>(kMiobiMaxBlocks);
    Selection sel("kt_miobi_break_node", r.k, t, 2, blk);  // columns: the node, its degree
    const Ints dLr = blk.take<int>(std::max<size_t>(long_rows.size(), 1));
    const Bytes dAl = blk.take<unsigned char>((size_t)n);
    blk.alloc(ctx);
    hipStream_t st = ctx->stream;
    KT_HIP(hipMemsetAsync(dAl, 1, (size_t)n, st));
    sel.clear(st);
    KT_HIP(hipStreamSynchronize(st));

    std::vector<double> stage;
    std::vector<unsigned char> dead((size_t)n, 0);
    const DevCSR* M = nullptr;  // of the current window
    int n_long = 0, hacc = 0;
    r.windows(
        sel, PROF_MIOBI_NODE, [&] { return miobi_node_window(r.k - r.done, refresh); },
        [&](int) {
            M = &natural_csr(A);  // the edited matrix's copy
            n_long = upload_long_rows(A, dLr, long_rows);
            const int state[4] = {r.done, 0, hacc, 0};
            KT_HIP(hipMemcpyAsync(sel.dSt, state, sizeof state, hipMemcpyHostToDevice, st));
            upload_v(ctx, n, t, r.Vh.data(), true, dV.col(0), stage);  // :177  column 0 by absolute value
            upload_e(ctx, t, r.lam.data(), dE, dC);
            if (shift == 0) KT_HIP(launch_miobi_colsum(n, dV.col(0), dNp, dS, st));
        },
        [&] {
            KT_HIP(launch_miobi_node_score(n, t, dV.col(0), dC, M->rowptr, M->col, dAl, dLr, n_long, nullptr, nblocks,
                                           dPs, dPn, dPd, sel.dSt, st));
            KT_HIP(launch_miobi_node_pick(nblocks, dPs, dPn, dPd, t, shift, refresh, dV.col(0), M->rowptr, M->col, dAl,
                                          dE, dC, dS, sel.dCol[0], sel.dSs, sel.dCol[1], sel.dTr, sel.dSt, st));
        },
        [&](int now) {
            bool ended = false;
            for (int s = r.done; s < now; ++s) {
                const int row = sel.col[0][s], d = sel.col[1][s];
                if (row < 0 || row >= n || dead[(size_t)row] || d < 1 ||
                    d > A->h_rowptr[row + 1] - A->h_rowptr[row] || ended)
                    fail(KT_ERR_HIP, "kt_miobi_break_node: the device's selection record is inconsistent");
                ended = miobi_node_book(hacc, d, refresh);
                dead[(size_t)row] = 1;
                sel_n[s] = row;
                sel_score[s] = sel.score[s];
                sel_deg[s] = d;
            }
            if ((refresh > 0 && sel.state[2] != hacc) || (sel.state[3] != 0) != ended)
                fail(KT_ERR_HIP, "kt_miobi_break_node: the device's removed-entry count differs from the host's");
            if (now > r.done) {  // :211-212 for the window's nodes
                r.start();
                edited = true;
                miobi_clear_nodes(n, dead, A->h_rowptr, A->h_col, A->h_val);
                A->nnz = (int64_t)A->h_col.size();
                refresh_device(A);
                r.lap(ctx->make_edit_us);
            }
            if (sel.state[1] || now >= r.k || A->nnz == 0) return true;  // (an empty matrix has nothing left to score)
            if (!ended) fail(KT_ERR_HIP, "kt_miobi_break_node: a full window did not reach its end");
            return false;
        });
}

void nodes_score_impl(kt_matrix_s* A, int t, const double* lambda, const double* V, double* score) {
    const int64_t n = A->n;
    std::vector<int> long_rows;
    miobi_long_rows(n, A->h_rowptr.data(), kMiobiNodeLong, long_rows);
    const int nblocks = miobi_node_blocks(n, 0);
    hipStream_t st = A->ctx->stream;
    Block blk;
    const Ints dPn = blk.take<int>(kMiobiMaxBlocks), dPd = blk.take<int>(kMiobiMaxBlocks),
               dLr = blk.take<int>(std::max<size_t>(long_rows.size(), 1));
    const Bytes dAl = blk.take<unsigned char>((size_t)n);
    const DevCSR* M = nullptr;
    int n_long = 0;
    score_once(
        A->ctx, blk, n, t, lambda, V, PROF_MIOBI_NODE, n, score,
        [&] {
            M = &natural_csr(A);
            KT_HIP(hipMemsetAsync(dAl, 1, (size_t)n, st));
            n_long = upload_long_rows(A, dLr, long_rows);
        },
        [&](double* dV, double* dC, double* dSc, double* dPs) {
            return launch_miobi_node_score(n, t, dV, dC, M->rowptr, M->col, dAl, dLr, n_long, dSc, nblocks, dPs, dPn,
                                           dPd, nullptr, st);
        });
}

// What the five entries check first, in this order: the pointers (null_arg:
// whether a required one is NULL), k, t -- in [2, min(32, n)] for a loop entry,
// in [1, 32] for a score-only one -- and, with a matrix, that no kt_slq_submit
// call is outstanding on its context and that it is symmetric.
void entry_checks(const char* who, bool null_arg, int k, int t, bool loop, kt_matrix_s* A) {
    const std::string w(who);
    if (null_arg) fail(KT_ERR_ARG, w + ": NULL argument");
    if (k < 0) fail(KT_ERR_ARG, w + ": k must not be negative");
    if (loop ? (t < 2 || t > kMiobiLd || t > A->n) : (t < 1 || t > kMiobiLd))
        fail(KT_ERR_ARG, w + (loop ? ": t must be in [2, min(32, n)]" : ": t must be in [1, 32]"));
    if (!A) return;
    if (A->ctx->ws.slq_submitted != A->ctx->ws.slq_collected)
        fail(KT_ERR_ARG, w + ": kt_slq_submit calls are outstanding on this context");
    require_symmetric(A, "MIOBI:: adjacency matrix has to be symmetric");
}

// what both node entries require of A beyond that (MIOBIBreakNode.m:31-39
// binarises its input; its datasets have no self-loop)
void node_matrix_checks(kt_matrix_s* A, const char* who) {
    const std::string w(who);
    if (A->n > INT32_MAX) fail(KT_ERR_ARG, w + ": n must fit 32-bit indices");
    if (A->nnz > 0 && !A->unit_values)
        fail(KT_ERR_ARG, w + ": the matrix must be a unit-weight adjacency matrix (MIOBIBreakNode.m binarises "
                             "its input)");
    if (miobi_has_diagonal(A->n, A->h_rowptr.data(), A->h_col.data()))
        fail(KT_ERR_ARG, w + ": the matrix must have a zero diagonal");
}

// body(); on any error undo() puts the matrix back as it was -- it returns
// whether there was anything to put back, and then no selection is reported
template <class Body, class Undo>
void restoring(int64_t* nsel, Body body, Undo undo) {
    try {
        body();
    } catch (...) {
        if (undo()) *nsel = 0;
        throw;
    }
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
        entry_checks("kt_pairs_score_topk", !ctx || !lambda || !V || (npairs > 0 && (!pi || !pj || !score)), 0, t,
                     false, nullptr);
        if (n < 1 || n > INT32_MAX || npairs < 0 || npairs > INT32_MAX)
            fail(KT_ERR_ARG, "kt_pairs_score_topk: n and npairs must fit 32-bit indices");
        for (int64_t p = 0; p < npairs; ++p)
            if (pi[p] < 0 || pi[p] >= n || pj[p] < 0 || pj[p] >= n)
                fail(KT_ERR_ARG, "kt_pairs_score_topk: pair index out of range");
        pairs_score_impl(ctx, n, t, lambda, V, npairs, pi, pj, sign, score);
    }
    KT_MIOBI_GUARD_END
}

// (no rollback: an error after the first window leaves that window's removals in A)
extern "C" int kt_miobi_break(kt_matrix_t A, int k, int t, int refresh, int mode, double gap_rel, double tol,
                              int max_spmm, uint64_t seed, int64_t* sel_i, int64_t* sel_j, double* sel_score,
                              double* lambda_track, double* V_final, int64_t* nsel, int* nconv_min,
                              int* refreshes) {
    try {
        entry_checks("kt_miobi_break", !A || !nsel || (k > 0 && (!sel_i || !sel_j || !sel_score)), k, t, true, A);
        if (mode != 0 && mode != 1) fail(KT_ERR_ARG, "kt_miobi_break: mode must be 0 (reference) or 1 (paper)");
        if (!(gap_rel >= 0.0)) fail(KT_ERR_ARG, "kt_miobi_break: gap_rel must not be negative");
        Run run{A, A->ctx, A->n, k, t, refresh, max_spmm, tol, seed, lambda_track, nsel, nconv_min, refreshes};
        miobi_break_impl(run, mode, gap_rel, sel_i, sel_j, sel_score, V_final);
    }
    KT_MIOBI_GUARD_END
}

extern "C" int kt_miobi_make(kt_matrix_t A, int k, int t, int refresh, double tol, int max_spmm, uint64_t seed,
                             int64_t* sel_i, int64_t* sel_j, double* sel_score, double* lambda_track, int* cand_m,
                             int64_t* nsel, int* nconv_min, int* refreshes) {
    std::vector<int64_t> added_i, added_j;
    try {
        restoring(
            nsel,
            [&] {
                entry_checks("kt_miobi_make", !A || !nsel || (k > 0 && (!sel_i || !sel_j || !sel_score)), k, t, true,
                             A);
                if (A->nnz == 0 || !A->unit_values)
                    fail(KT_ERR_ARG, "kt_miobi_make: the matrix must be a unit-weight adjacency matrix with at least "
                                     "one edge (MIOBIMakeEdge.m binarises its input)");
                Run run{A, A->ctx, A->n, k, t, refresh, max_spmm, tol, seed, lambda_track, nsel, nconv_min, refreshes};
                miobi_make_impl(run, sel_i, sel_j, sel_score, cand_m, added_i, added_j);
            },
            [&] {  // the pairs added so far were non-adjacent
                if (added_i.empty()) return false;
                try {
                    set_pairs(A, (int64_t)added_i.size(), added_i.data(), added_j.data(), 0.0);
                } catch (...) {
                }
                return true;
            });
    }
    KT_MIOBI_GUARD_END
}

extern "C" int kt_nodes_score_topk(kt_matrix_t A, int t, const double* lambda, const double* V, double* score) {
    try {
        entry_checks("kt_nodes_score_topk", !A || !lambda || !V || !score, 0, t, false, A);
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
        restoring(
            nsel,
            [&] {
                entry_checks("kt_miobi_break_node", !A || !nsel || (k > 0 && (!sel || !sel_score || !sel_deg)), k, t,
                             true, A);
                if (shift != 0 && shift != 1)
                    fail(KT_ERR_ARG, "kt_miobi_break_node: shift must be 0 (reference) or 1 (first_order)");
                node_matrix_checks(A, "kt_miobi_break_node");
                rowptr0 = A->h_rowptr;  // unit weights: the pattern is the matrix
                col0 = A->h_col;
                Run run{A, A->ctx, A->n, k, t, refresh, max_spmm, tol, seed, lambda_track, nsel, nconv_min, refreshes};
                miobi_break_node_impl(run, shift, sel, sel_score, sel_deg, edited);
            },
            [&] {
                if (!edited) return false;
                A->h_rowptr = rowptr0;
                A->h_col = col0;
                A->h_val.assign(col0.size(), 1.0);
                A->nnz = (int64_t)col0.size();
                refresh_device(A);
                return true;
            });
    }
    KT_MIOBI_GUARD_END
}
