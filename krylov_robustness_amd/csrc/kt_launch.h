// kt_launch.h -- internal launcher declarations (kt_kernels.hip <-> runtime).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kt {

int spmm_grid(int n, int P, int max_blocks);
int long_blocks_for(int n_long, int max_blocks);

hipError_t launch_rademacher(int P, int n, uint64_t seed, int64_t probe_base, const int* perm,
                             double* X, hipStream_t st);
// probes probe_base .. probe_base + ncols - 1 as ncols (<= 64) columns of a
// row-major block with row stride ldx (natural row order)
hipError_t launch_rademacher_cols(int n, int ncols, uint64_t seed, int64_t probe_base, double* X, int ldx,
                                  hipStream_t st);
hipError_t launch_spmm_dot(int P, int flags, int grid, const int* rp, const int* ci,
                           const double* va, int n, const double* ucur, const double* sc,
                           double* y, double* partial, const int* long_rows, int n_long,
                           int long_thresh, int long_blocks, hipStream_t st);
// device CSR + its long-row list and hub-row chunk table (kt_internal.h DevCSR)
struct CsrView {
    const int* rp;
    const int* ci;
    const double* va;
    int n;
    const int* long_rows;
    int n_long, long_thresh, split_thresh;
    const int* ck_beg;
    const int* ck_end;
    int n_chunks;
    const int* sp_rows;
    const int* sp_first;
    int n_split;
    // natural CSR only: rows of degree <= kMedThresh as {row, beg, end, 0},
    // degree-descending (the row-blocked expmv term; nullptr elsewhere)
    const int* short_tasks = nullptr;
    int n_short = 0;
    // natural CSR only: the medium rows (med_rows) as {row, beg, end, 0}
    const int* med_tasks = nullptr;
    // the first n_heavy long rows have degree > kExpmvCoopThresh
    int n_heavy = 0;
};
constexpr int kExpmvCoopThresh = 256;  // expmv terms: a long row this heavy takes a whole workgroup
constexpr int kChunkNnz = 32;      // nonzeros per hub-row chunk
constexpr int kSplitThresh = 64;   // rows longer than this are chunked (block SpMM)
constexpr int kMedThresh = 16;     // expmv terms: rows longer than this get a wave (or a workgroup)
// One workgroup per greedy candidate runs its whole trace_fun_update (kt_pairs.hip
// k_pair_fused); vec: C x 3 x n x 2 doubles; big: C x big_stride doubles of
// eigen scratch, needed only when 2 it > 56 (else may be null); state: C x 8.
size_t pair_fused_lds_bytes(int it);
// KT_PAIRS_DENSE_EIG=1 (read per call): the dense projected eigensolvers
// instead of block Sturm counts, in every candidate kernel
bool pairs_dense_eig();
hipError_t launch_pair_fused(int C, int n, int64_t nnz, const CsrView& A, bool unit, const int* ii,
                             const int* jj, const double* B, int it, int fun, double tol, double* vec,
                             double* big, int64_t big_stride, double* state, hipStream_t st);
// device-resident greedy steps (kt_greedy.cpp): k_pair_reg with the CSR's
// {nnz, n_long} read from dyn (the LDS sized for nnz_max), and one step's
// selection + ranking update + edge deletion into the other CSR buffer
// k_pair_reg: the first kRegLongCap long rows (degree > long_thresh, in the
// CSR's long-row list order) are summed by whole waves, the rest by their
// owning threads -- so the list order is part of the kernel's arithmetic
constexpr int kRegLongCap = 256;
bool pair_reg_applies(int n, int64_t nnz, int it, int n_long, bool unit);
// the k_pair_reg<rows, csr> instance and `spec` value that shape takes (what
// pair_reg_applies decides on; rows = 0 when it does not apply)
bool pair_reg_form(int n, int64_t nnz, int it, int n_long, bool unit, int* rows, int* csr, int* spec);
hipError_t launch_pair_reg_dyn(int C, int n, int64_t nnz_max, const CsrView& A, bool unit, const int* ii,
                               const int* jj, const double* B, int it, int fun, double tol, double* state,
                               const int* dyn, hipStream_t st);
hipError_t launch_greedy_edit(int C, const double* state, int* Ti, int* Tj, int nT, int n, int long_thresh,
                              const int* rp, const int* ci, const double* va, const int* lr, const int* dyn,
                              int* rp2, int* ci2, double* va2, int* lr2, int* dyn2, int step, int* sel,
                              double* selv, hipStream_t st);
hipError_t launch_spmm_block(int P, int flags, int grid, const CsrView& M, const double* X, int ldx,
                             double* Y, int ldy, int long_blocks, int chunk_blocks, double* ck_part,
                             hipStream_t st, int slices = 1, const int* skip = nullptr);
// hist (nullable): P doubles receiving the step's scale s_j (sc)
hipError_t launch_coef_cgs2(int P, const double* partial, int nblk, int first, const double* k2s,
                            const double* sc, const double* sp, double* coef, double* t_alpha,
                            double* t_up, double* hist, hipStream_t st);
// rec (optional): u_next's first bcols columns also to rec[row * bcols + c]
hipError_t launch_update(int P, int grid, int n, const double* y, double* uprev,
                         const double* ucur, const double* sc, const double* sp,
                         const double* coef, int first, double* partial, hipStream_t st,
                         bool nt = false, double* rec = nullptr, int bcols = 0);
hipError_t launch_norm(int P, const double* partial, int nblk, double* k2s, double* scale_next,
                       double* t_low, hipStream_t st);
// y-form probe Lanczos (one pass per step; slot-major partials [3P][grid]
// for launch_ycoef, the per-probe coefficient step).
// Vn != nullptr: also v_{j+1} = g y_j - a v_j - b v_{j-1} into basis slot Vn
// from slots Vc (v_j) and Vo (v_{j-1}, nullptr at j = 0), columns < bcols
// (every slot n x P, row-major).  flags bit 7 (a compact sweep's second
// step; unit weights, no basis): Yold is the start pass's n x P int16 table,
// y_0 = s0 * (double)Yold.
// gate (nullable; ngate <= kGateWordsMax words): the gated form of an
// error-controlled sweep (kt_slq.cpp slq_trace_auto) -- when every word reads
// zero each workgroup returns at once and nothing is written; bits as the
// ungated launch otherwise (forms-only passes; y_{j+1} stored nontemporal)
hipError_t launch_spmm_lanczos(int P, int flags, int grid, const int* rp, const int* ci,
                               const double* va, int n, const double* X, const double* Yold,
                               double* Out, const double* coef, double* partial,
                               const int* long_rows, int n_long, int long_thresh, int long_blocks,
                               hipStream_t st, const double* Vc = nullptr, const double* Vo = nullptr,
                               double* Vn = nullptr, int bcols = 0, double s0 = 0.0,
                               const int* gate = nullptr, int ngate = 0);
// First ordinary step of a compact sweep (unit weights): launch_spmm_lanczos
// with X = y_0 = s0 * (double)T read from the int16 table T and no Yold
hipError_t launch_spmm_lanczos_first(int P, int flags, int grid, const int* rp, const int* ci, int n,
                                     const int16_t* T, double s0, double* Out, const double* coef,
                                     double* partial, const int* long_rows, int n_long, int long_thresh,
                                     int long_blocks, hipStream_t st, const int* gate = nullptr,
                                     int ngate = 0);
// The last pass of a y-form sweep: only slab 0, X'A X per probe, from each
// row's strictly-lower prefix and diagonal (lower = DevCSR::lower; slabs 1, 2
// are written as zeros).  Vn as above.
hipError_t launch_spmm_quadform(int P, int flags, int grid, const int* rp, const int* ci,
                                const double* va, const int* lower, int n, const double* X,
                                const double* coef, double* partial, const int* long_rows, int n_long,
                                int long_thresh, int long_blocks, hipStream_t st,
                                const double* Vc = nullptr, const double* Vo = nullptr,
                                double* Vn = nullptr, int bcols = 0);
hipError_t launch_rademacher_signs(int P, int n, uint64_t seed, int64_t probe_base,
                                  const int* perm, uint32_t* S, hipStream_t st);
// flags bit 7 (unit weights): Out is the n x P int16 table of the row sums
// (y_0 = s0 * sum is not stored); the partials are the same
hipError_t launch_spmm_lanczos_start(int P, int flags, int grid, const int* rp, const int* ci,
                                     const double* va, int n, const uint32_t* S, double s0,
                                     double* Out, double* partial, const int* long_rows, int n_long,
                                     int long_thresh, int long_blocks, hipStream_t st);
hipError_t launch_ycoef(int P, const double* partial, int nblk, int start, int last, double s0,
                        double* ys, double* t_alpha, double* t_up, double* t_low, double* guard,
                        hipStream_t st, const int* gate = nullptr, int ngate = 0);
// the adaptive Lanczos depth (kt_adapt.hip): the stopping test at depth j on a
// sweep's device record [alpha | up | low][mcap][P] (state: kAdaptState
// doubles per column, zeroed before the sweep's first check; the checks of a
// sweep run at consecutive depths), and k_weighted_sum over a basis kept in
// chunks of spc slots (slot j: n x nc row-major)
constexpr int kAdaptState = 8;
constexpr int kSlotTabChunks = 8;
struct SlotTab {
    const double* chunk[kSlotTabChunks];
};
hipError_t launch_quad_check(const double* trec, int mcap, int P, int j, int live, int nfe, const double* n2,
                             int fun, double rtol, double* state, int* active, hipStream_t st);
// The same test for any sweep width, P <= 128 and depths <= 256, one launch
// per check: workgroup b owns columns [16 b, 16 b + 16) and stores the count
// of its own running columns to running[b], b < ceil(live / 16) (the words a
// gated step launch reads).  guard (nullable, with gsnap): the y-form sweep's
// guard values; a column whose guard is not >= gmin stops at once, and every
// column that stops leaves the guard it stopped with in gsnap[c].
constexpr int kWideCheckCols = 16;
constexpr int kGateWordsMax = 128 / kWideCheckCols;
hipError_t launch_quad_check_wide(const double* trec, int mcap, int P, int j, int live, int nfe, const double* n2,
                                  int fun, double rtol, double* state, int* running, hipStream_t st,
                                  const double* guard = nullptr, double gmin = 0.0, double* gsnap = nullptr);
hipError_t launch_weighted_sum_tab(int n, int m, int nc, const SlotTab& tab, int spc, const double* W, double* Y,
                                   int ldy, hipStream_t st);
// The node-removal columns (kt_slq.cpp lanczos_nodes_adaptive; DESIGN.md
// §4.2h).  launch_node_check: launch_quad_check's shape and state block for
// the lag-2 rule of trace_fun_update.m:104-124 on X_j = f(0) + sum f(eig(T_j[2:,
// 2:])) - sum f(eig(T_j)), tol absolute; state per column: [0] X_j [1] [2] the
// stored pair [3] depth [4] stopped [5] theta_max_j [6] lucky [7] last depth
// (fun = exp: the X scaled by exp(-theta_max_j)).  launch_unit_start: column
// c < nc of the zeroed n x P block X gets 1 at row pos[c] (device array, rows
// in the sweep's order; out of range: the column stays zero), sc / k2s (P
// each) the start scale and squared norm.
hipError_t launch_node_check(const double* trec, int mcap, int P, int j, int live, int fun, double tol, double* state,
                             int* active, hipStream_t st);
hipError_t launch_unit_start(int n, int P, int nc, const int* pos, double* X, double* sc, double* k2s,
                             hipStream_t st);
// The bracket columns (kt_slq.cpp lanczos_nodes_bracket):
// launch_node_check's shape and state block for the Gauss / Gauss-Radau bracket
// of exp(A)_ii with a Radau node at mu; state per column: [0] L_j [1] U_j (both
// scaled by exp(-mu)) [3] depth [4] stopped [6] flag (0 the gap U_j - L_j <=
// rtol L_j, 1 beta_j < 1e-8, 2 mu proved below lambda_max, 3 depth mcap
// reached) [7] last depth.  24 (j + 1) G bytes of LDS: G = P while that fits
// 64 KB less the static words, else groups of 8.
hipError_t launch_bracket_check(const double* trec, int mcap, int P, int j, int live, double mu, double rtol,
                                double* state, int* active, hipStream_t st);
// The pair columns (kt_slq.cpp lanczos_pairs_bracket): columns
// 2p, 2p + 1 of a sweep are pair p's runs started at (e_i +- e_j) / sqrt 2.
// launch_pair_start: launch_unit_start for them, pos[2p], pos[2p + 1] the
// pair's rows (np pairs, 2 np <= P, P even), sc = 1 / sqrt 2 and k2s = 2 for
// live columns.  launch_pair_bracket_check: launch_bracket_check's shape (P and
// live even, groups of P or 8 lanes hold whole pairs) for the bracket lo = (L+
// - U-) / 2, hi = (U+ - L-) / 2 of exp(A)_ij; state per column: [0] L [1] U
// [3] depth [4] stopped [5] the pair is decided [6] flag (1 a frozen column of
// an undecided pair; then the pair's: 0 the gap <= rtol min(|lo|, |hi|) with lo
// hi > 0, 1 both columns frozen, 2 mu proved below lambda_max, 3 depth mcap
// reached, 4 the gap <= ftol (U+ + U-) / 2) [7] last depth.
hipError_t launch_pair_start(int n, int P, int np, const int* pos, double* X, double* sc, double* k2s,
                             hipStream_t st);
hipError_t launch_pair_bracket_check(const double* trec, int mcap, int P, int j, int live, double mu, double rtol,
                                     double ftol, double* state, int* active, hipStream_t st);
hipError_t launch_fill(double* x, int count, double v, hipStream_t st);
hipError_t launch_delay(double microseconds, hipStream_t st);
// sweep start scales from device column norms (kt_slq.cpp; mode 0 explicit: sc,
// k2s; mode 1 y-form: the 9P coefficient block) and a Gram block's diagonal
hipError_t launch_sweep_scales(const double* n2, int nc, int P, int mode, double* a, double* b, hipStream_t st);
hipError_t launch_gram_diag(const double* G, int ld, int nc, double* n2, hipStream_t st);
// out[i] = D[off[i]], i < count
// tall-skinny Gram / combine (kt_gemm_ts.hip)
int gram_ts_chunks(int64_t n);
hipError_t launch_gram_ts(int64_t n, const double* X, int ldx, int px, const double* Y, int ldy, int py,
                          double* part, double* G, hipStream_t st);
hipError_t launch_combine_ts(int64_t n, const double* X, int ldx, int px, const double* C, int q, double alpha,
                             double beta, double* Y, int ldy, hipStream_t st);
hipError_t launch_fro_colmax_scale(int n, double* M, double* out, double* colsq, hipStream_t st);
// device CholeskyQR factor: G + shift_coef tr(G) I = R' R, Rinv = R^-1 (bs <= 64); ok[0] = 0 on a failed pivot
hipError_t launch_chol_rinv(int bs, const double* G, double shift_coef, double* R, double* Rinv, int* ok,
                            hipStream_t st);
hipError_t launch_scatter_elems(int64_t count, const int64_t* off, const double* val, double* D,
                                hipStream_t st);
hipError_t launch_gather_elems(int64_t count, const double* D, const int64_t* off, double* out,
                               hipStream_t st);
// out (nr x cols, column-major) = rows[r] of the row-major block D (leading dimension ldd)
hipError_t launch_gather_rows(int nr, int cols, const double* D, int ldd, const int64_t* rows, double* out,
                              hipStream_t st);
// Y[r, c] = sum_j U[r * ldu + j * sstride + c] W[j * P + c]
hipError_t launch_weighted_sum(int n, int m, int P, int nc, const double* U, int ldu, int64_t sstride,
                               const double* W, double* Y, int ldy, hipStream_t st);
// dst[r] = src[perm[r]] (gather != 0) or dst[perm[r]] = src[r], rows of `cols` doubles
hipError_t launch_perm_rows(int n, int cols, const int* perm, int gather, const double* src, int lds,
                            double* dst, int ldd, hipStream_t st);
hipError_t launch_axpby(int n, int nc, double a, const double* X, int ldx, double b, double* Y,
                        int ldy, hipStream_t st);
// diag f(A) estimator (kt_diag.hip; driver kt_diag_fun.cpp).  Blocks are n x P
// row-major in the probe sweep's row order, P a power of two <= 16; Q is the
// deflation block, n x KP row-major, KP in {0, 1, 4, 16} (0: none).  The
// reducing kernels write `grid` workgroup partials of K values each
// (K = KP P, or P for the norms); launch_diag_sum_parts adds them in order.
int diag_grid(int n, int P);
hipError_t launch_diag_qtz(int P, int KP, int grid, int n, uint64_t seed, int64_t base, int nc, const int* perm,
                           const double* Q, double* part, hipStream_t st);
hipError_t launch_diag_sum_parts(int nparts, int K, const double* part, double* out, hipStream_t st);
// X = z - Q c (c: KP x P), columns >= nc zero; part: the columns' squared-norm partials
hipError_t launch_diag_start(int P, int KP, int grid, int n, uint64_t seed, int64_t base, int nc, const int* perm,
                             const double* Q, const double* c, double* X, double* part, hipStream_t st);
// y = sum_{j < depth[p]} W[j, p] V_j (slot j at V + j sstride; mdepth = max depth).
// KP = 0: dsum[perm[r]] += sum_p z y, dsum2 likewise with squares.  KP > 0: y
// into Y and the partials of Q' y into part.
hipError_t launch_diag_combine(int P, int KP, int grid, int n, int m, int mdepth, const double* V, int64_t sstride,
                               const double* W, const int* depth, uint64_t seed, int64_t base, const int* perm,
                               const double* Q, double* Y, double* part, double* dsum, double* dsum2,
                               hipStream_t st);
// t = z .* (Y - Q c) reduced over the row's probes into dsum / dsum2
hipError_t launch_diag_finish(int P, int KP, int grid, int n, uint64_t seed, int64_t base, const int* perm,
                              const double* Q, const double* c, const double* Y, double* dsum, double* dsum2,
                              hipStream_t st);
// d0 = 2 rowsum(Q .* G) - rowsum((Q H) .* Q); Q, G n x ld row-major, H k x k column-major
hipError_t launch_diag_d0(int n, int k, const double* Q, const double* G, int ld, const double* H, double* d0,
                          hipStream_t st);
// f(A) entries on a pair list (kt_entries_fun).  tab: npairs x (r_i, r_j, i, j)
// int32, rows in the sweep's order and original indices.  launch_diag_combine_y
// is launch_diag_combine's KP = 0 pass storing y into Y (no sums);
// launch_entries_accumulate adds the sweep's sum_p t and sum_p t^2 to esum /
// esum2 (Y, Q in the sweep's row order, c = Q'y: KP x P); launch_entries_e0
// forms the exact deflated part (Q, G in original numbering, H k x k column-major).
hipError_t launch_diag_combine_y(int P, int grid, int n, int m, int mdepth, const double* V, int64_t sstride,
                                 const double* W, const int* depth, double* Y, hipStream_t st);
hipError_t launch_entries_accumulate(int P, int KP, int64_t npairs, const void* tab, uint64_t seed, int64_t base,
                                     const double* Q, const double* c, const double* Y, double* esum,
                                     double* esum2, hipStream_t st);
hipError_t launch_entries_e0(int64_t npairs, const void* tab, int k, const double* Q, const double* G, int ld,
                             const double* H, double* e0, hipStream_t st);
// kt_eigs_topk's streaming kernels (kt_eigs.hip; driver kt_eigs.cpp).
// launch_eig_start: the columns c < 16 of X (n x ldx row-major) whose bit is set
// in mask become the counter-RNG Rademacher column col0 + c keyed by (seed,
// ORIGINAL row perm[r], col0 + c) (perm nullptr: identity); ones_first: column
// 0 is 1 / sqrt(n) instead.
hipError_t launch_eig_start(int64_t n, uint64_t seed, int64_t col0, unsigned mask, bool ones_first, const int* perm,
                            double* X, int ldx, hipStream_t st);
// V(:, 0:p) <- V(:, 0:mb) Y in place (Y: mb x p ROW-major, device); mb even
// <= 128, p in {16, 32, 48}, p <= mb <= ld
hipError_t launch_eig_rotate(int64_t n, int mb, int p, double* V, int ld, const double* Y, hipStream_t st);
// out[0:kp] = ||AX_i - theta_i X_i||^2, out[kp:2kp] = ||X_i||^2, out[2kp:3kp] =
// sum_r X_i(r); kp = 16 or 32; part: 3 kp eig_resid_chunks(n) doubles
int eig_resid_chunks(int64_t n);
hipError_t launch_eig_resid(int64_t n, int kp, const double* X, int ldx, const double* AX, int ldax,
                            const double* theta, double* part, double* out, hipStream_t st);
// MIOBI top-t edge scores and the device step (kt_miobi.hip; driver
// kt_miobi.cpp).  V: n x kMiobiLd row-major in ORIGINAL numbering, columns >= t
// zero; c[k] = exp(e[k]); pairs (pi, pj) 0-based with an optional alive byte.
// launch_miobi_score: nblocks = miobi_score_blocks(npairs, max_blocks)
// workgroups, each leaving its first candidate (smallest score, ties by the
// key (max, min), then by list index; index -1: none) in part_*[b]; score
// (nullable) receives every live pair's score.  launch_miobi_pick reduces the
// candidates and applies the step (see the kernel); state = {steps, stop}.
// launch_miobi_normalise: V's columns to unit 2-norm, column 0 non-negative
// (part: kMiobiLd miobi_norm_blocks(n) doubles).  A set state[1] / *stop makes
// each of the three a no-op.
constexpr int kMiobiLd = 32;
constexpr int kMiobiTilePairs = 64;   // pairs a workgroup scores per trip
constexpr int kMiobiMaxBlocks = 2048;
int miobi_score_blocks(int64_t npairs, int max_blocks);
hipError_t launch_miobi_setc(int t, const double* e, double* c, hipStream_t st);
hipError_t launch_miobi_score(int64_t npairs, int t, const double* V, const double* c, const int* pi, const int* pj,
                              const unsigned char* alive, double sign, double* score, int nblocks, double* part_s,
                              unsigned long long* part_key, int* part_idx, const int* stop, hipStream_t st);
hipError_t launch_miobi_pick(int nparts, const double* part_s, const unsigned long long* part_key,
                             const int* part_idx, int t, int paper, double gap_rel, const double* V, double* e,
                             double* c, const int* pi, const int* pj, const double* wt, unsigned char* alive,
                             int* sel_i, int* sel_j, double* sel_score, double* track, double* M, int* state,
                             hipStream_t st);
int miobi_norm_blocks(int64_t n);
hipError_t launch_miobi_normalise(int64_t n, double* V, double* part, const int* state, hipStream_t st);
// MIOBI make-edge (kt_miobi_make).  W: the candidates' rows of
// V, mcap x kMiobiLd row-major in RANK order, columns >= t zero; mask: mcap rows
// of miobi_make_words(mcap) 64-bit words, bit (a, b) = "ranks a and b are
// adjacent" (both halves); state = {steps, stop, maxdeg, live m}.
// launch_miobi_make_score scores every pair of ranks a < b < state[3] whose
// mask bit is clear, score = sum_{k < t} c[k] exp(2 W[a, k] W[b, k]), over 64 x
// 64 tiles of the rank square; nblocks = miobi_make_blocks(mcap, max_blocks)
// workgroups each leave their first candidate (largest score, exactly equal
// scores by the smaller key (a << 32) | b; part_ok 0: none) in part_*[b].
// score (nullable) is mcap x mcap row-major and receives the scored pairs.
// launch_miobi_make_pick reduces the candidates and applies the step (see the
// kernel).  A set state[1] makes both a no-op.
constexpr int kMiobiMakeTile = 64;   // ranks along each side of a workgroup's tile
inline int miobi_make_words(int mcap) { return (mcap + 63) / 64; }
int miobi_make_blocks(int mcap, int max_blocks);
hipError_t launch_miobi_make_score(int mcap, int t, const double* W, const double* c,
                                   const unsigned long long* mask, const int* state, double* score, int nblocks,
                                   double* part_s, unsigned long long* part_key, int* part_ok, hipStream_t st);
hipError_t launch_miobi_make_pick(int nparts, const double* part_s, const unsigned long long* part_key,
                                  const int* part_ok, int mcap, int t, int k, int n, const double* W,
                                  const int* node, double* e, double* c, unsigned long long* mask, int* deg,
                                  int* sel_i, int* sel_j, double* sel_score, double* track, int* cand_m,
                                  int* state, hipStream_t st);
// MIOBI break-node (kt_miobi_break_node).  V as above; (rowptr,
// col): the natural-order CSR of a unit-weight matrix with a zero diagonal;
// alive: one byte per node; long_rows: the n_long rows longer than
// kMiobiNodeLong, in any order; state = {steps, stop, acc, window end}.
// launch_miobi_node_score: score[r] = sum_{k < t} c[k] exp(-2 V[r, k] W[r, k]),
// W[r, .] the sum of the live neighbours' rows; +Inf for a dead row or one with
// no live neighbour; nblocks = miobi_node_blocks(n, max_blocks) workgroups each
// leave their first candidate (smallest score, exactly equal scores by the
// smaller node; node -1: none) and its live degree in part_*[b]; score
// (nullable, n doubles) receives every row's score.  launch_miobi_node_pick
// reduces the candidates and applies the step (see the kernel); shift 0 reads
// colsum (launch_miobi_colsum: s[k] = sum_r V[r, k], part: kMiobiLd
// miobi_norm_blocks(n) doubles), shift 1 gathers the node's row again.  A set
// state[1] or state[3] makes the score and pick launches a no-op.
constexpr int kMiobiNodeBatch = 8;    // row reads a half-wave issues before the first add
constexpr int kMiobiNodeLong = 128;   // a longer row is split over a workgroup
constexpr int kMiobiNodeChunk = 64;   // entries of a split row per half-wave and trip (8 x 64 per workgroup trip)
int miobi_node_blocks(int64_t n, int max_blocks);
hipError_t launch_miobi_node_score(int64_t n, int t, const double* V, const double* c, const int* rowptr,
                                   const int* col, const unsigned char* alive, const int* long_rows, int n_long,
                                   double* score, int nblocks, double* part_s, int* part_node, int* part_deg,
                                   const int* state, hipStream_t st);
hipError_t launch_miobi_node_pick(int nparts, const double* part_s, const int* part_node, const int* part_deg, int t,
                                  int shift, int refresh, const double* V, const int* rowptr, const int* col,
                                  unsigned char* alive, double* e, double* c, const double* colsum, int* sel_node,
                                  double* sel_score, int* sel_deg, double* track, int* state, hipStream_t st);
hipError_t launch_miobi_colsum(int64_t n, const double* V, double* part, double* s, hipStream_t st);
int inf_norm_blocks();
// normest1 (t = 1) reductions, normest1_blocks(n) partials each: sum |Y| in
// partial[0, nb), S_prev . S in partial[nb, 2 nb), S = mysign(Y); per-block
// max |Z| and its smallest index
int normest1_blocks(int n);
hipError_t launch_normest1_y(int n, const double* Y, const double* Sprev, double* S, double* partial,
                             hipStream_t st);
hipError_t launch_absmax_idx(int n, const double* Z, double* pval, int* pidx, hipStream_t st);
// batched greedy candidates (kt_pairs.hip)
hipError_t launch_pair_select(int C, const int* ii, const int* jj, double* X, int ld,
                              hipStream_t st);
// CGS2 of W against [prev cur] (cur == nullptr: none) + Householder thin QR,
// per candidate; hr[c*11 + 0..10] = (h [8], R11, R12, R22)
hipError_t launch_pairs_orth(int C, int n, int num_cu, const double* prev, const double* cur,
                             double* W, int ld, double* coef, double* part, double* hr,
                             hipStream_t st,
                             const int* skip = nullptr);
size_t pairs_part_doubles(int n, int C, int num_cu);
// per-candidate projected eigenproblems + stop logic; state C x 8 doubles
hipError_t launch_pair_eig(int C, int j, int it, int fun, double tol, const double* hist,
                           const double* Cm, double* scratch, int64_t sstride, double* state,
                           int* active, hipStream_t st);
// tall-skinny Householder QR (kt_tsqr.hip)
int ts_nrb(int n, int num_cu);
hipError_t launch_ts_reflectors(int n, int bs, int BP, double* W, int ld, double* V, double* pivot,
                                double* sums, double* part, double* taus, int num_cu,
                                hipStream_t st);
// one launch per column (k_ts_step1): ts_step1_grid > 0 when it applies;
// part: 2 * BP * grid doubles, piv: 2 * BP doubles
int ts_step1_grid(int n, int* rows_per_wg);
hipError_t launch_ts_reflectors1(int n, int bs, int BP, double* W, int ld, double* V, double* part, double* piv,
                                 double* taus, hipStream_t st);
hipError_t launch_ts_formq(int n, int bs, int BP, const double* V, const double* M, double* W,
                           int ld, hipStream_t st);
hipError_t launch_sum_slabs(int count, int S, const double* part, double* G, hipStream_t st);
hipError_t launch_poly4(int n, double beta, const double* in, double c0, double c1, const double* X1,
                        double c2, const double* X2, double c3, const double* X3, double* out,
                        hipStream_t st,
                        int batch = 1);
// column-batched single-vector Arnoldi (kt_colbatch.hip); V blocks at stride vstride
int col_nrb(int n, int num_cu, int rpb_lo = 64);
hipError_t launch_col_dots(int n, int P, int nb, int64_t vstride, const double* V, const double* W,
                           int r_lo, int num_cu, double* part, double* out, hipStream_t st, int rpb_lo = 64);
hipError_t launch_col_update(int n, int P, int nb, int64_t vstride, const double* V,
                             const double* h, double* W, hipStream_t st);
hipError_t launch_col_householder(int n, int P, const double* s, double* W, double* Q, double* r,
                                  hipStream_t st);
hipError_t launch_col_select(int C, int P, const int* idx, double* X, hipStream_t st);
size_t pairs_coef_doubles(int C);
hipError_t launch_inf_norm(int n, int nc, const double* X, int ldx, double* partial,
                           hipStream_t st);
// expmv Taylor stage with the stop test on the device (state: expmv_state_bytes();
// layout {int active; int mv; double c1;}); partial: 2 * inf_norm_blocks() doubles
size_t expmv_state_bytes();
// term maxima of the fused expmv path: 64 slots per term, one 128-B line
// each (workgroup b folds into slot b % 64), so same-address atomics stay few
// (config 1: 340 workgroups, 31k at n = 1M)
constexpr int kTermSlots = 64, kTermSlotStride = 16;
struct ExpmvState {
    int active;
    int mv;
    double c1;
    double c1s[2];  // fused path: c1 of the check of term j in c1s[j & 1]
    // fused path: term j's row-sum maxima of |b| and |f| in set j % 3, as
    // the bit patterns of the (non-negative) doubles, so an unsigned atomic
    // max is the exact fmax; term j zeroes set (j + 1) % 3 for the next
    // term, k_expmv_begin set 1 for a stage's first term
    unsigned long long term_max[3][kTermSlots][kTermSlotStride];
};
hipError_t launch_expmv_begin(const double* partial, int nb, void* state, hipStream_t st);
hipError_t launch_expmv_term(int n, int nc, double mu, double coef, const double* Ab, double* b,
                             double* F, int ld, double* partial, const void* state, hipStream_t st);
hipError_t launch_expmv_check(int n, const double* partial, double tol, void* state, hipStream_t st);
// one fused launch per Taylor term k (P = pow2 >= nc, P <= 32, ld >= P): the
// check of term k-1, SpMM of the natural-order CSR (M), update, the maxima
// of term k's row sums folded into the state (term_max slot k % 3)
// waves: per block (0: the per-term kernel's)
int expmv_step_blocks(int n, int P, int n_long, int n_med, int waves = 0);
// the grid of forms 2 and 3 (k_expmv_rows) for tasks = n_long + n_med +
// ceil(n_short / 8): a workgroup per 4 tasks, at most the resident workgroups
int expmv_rows_blocks(int tasks);
// the default form of launch_expmv_step for this shape (true: SPLIT, grids
// above 1,024 workgroups); with split the host launches
// launch_expmv_slot_check after every term but a stage's last.
// launch_expmv_step form: 0 fused, 1 split (a workgroup per row class unit),
// 2 row-blocked (k_expmv_rows: resident workgroups) with the stop test in
// k_expmv_slot_check, 3 row-blocked with the stop test of term k - 1 at the
// start of term k (no slot-check launch; the default on large grids)
bool expmv_split_check(int n, int P, int n_long, int n_med);
hipError_t launch_expmv_slot_check(void* state, int k, double tol, hipStream_t st, int* hflag, int stage);
hipError_t launch_expmv_step(int P, bool unit, const CsrView& M, const int* med_rows, int n_med, int nc,
                             int ld, double mu, double coef,
                             double tol, int k, const double* bin, double* bout, double* F,
                             void* state, hipStream_t st, int form, int* hflag = nullptr, int stage = 0);

}  // namespace kt
