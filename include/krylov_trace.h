/* krylov_trace.h -- C ABI of libkrylov_hip.so, the MI355X trace(f(A)) evaluator.
 *
 * This is the drop-in boundary of SURVEY.md §8b.  The reference is MATLAB;
 * its callers (Tests/ scripts, greedy_krylov.m, fmincon closures) resolve the
 * functions below by name, so a MEX file of the same name placed in
 * functions/ shadows the .m (krylov_robustness_amd/mex/).
 * The MEX shim forwards mxArray data to these plain-pointer entry points; the
 * ctypes binding in krylov_robustness_amd/_lib.py binds the same symbols for
 * tests.
 *
 * Conventions
 *   - All functions return an int status (KT_OK == 0).  On failure a
 *     thread-local message is available from kt_last_error(); messages
 *     reproduce the reference's error strings where one exists.
 *   - Matrices: MATLAB sparse CSC (mwIndex = int64 jc[n+1], ir[nnz], 0-based;
 *     double pr[nnz]).  A is symmetric on every hot path, so CSC == CSR.
 *   - Dense arrays are column-major fp64 (MATLAB layout); Omega is 1-based.
 *   - Inputs are borrowed (read-only); outputs are caller-allocated.
 *   - A context is externally synchronised: no concurrent calls on one
 *     context (MATLAB calls a MEX on its single interpreter thread).
 *   - fun codes mirror fun_update.m:43-59's handle identities.
 */
#ifndef KRYLOV_TRACE_H
#define KRYLOV_TRACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KT_ABI_VERSION 3

enum kt_status {
    KT_OK = 0,
    KT_ERR_ARG = 1,           /* bad argument (sizes, null pointers)            */
    KT_ERR_HIP = 2,           /* HIP runtime failure                            */
    KT_ERR_NOT_HERMITIAN = 3, /* fun_and_grad_krylov_exp.m:21-23                */
    KT_ERR_NOT_SQUARE = 4,    /* lanczos_krylov.m:36-38                         */
    KT_ERR_ALLOC = 5,         /* device allocation failed                       */
    KT_ERR_UNSUPPORTED = 6,   /* size / option outside what the build supports  */
    KT_ERR_CALLBACK = 7       /* a caller-supplied callback returned non-zero   */
};

enum kt_fun { /* fun_update.m:43-59 */
    KT_FUN_EXP = 0,
    KT_FUN_SINH = 1,
    KT_FUN_COSH = 2,
    KT_FUN_SIN = 3,
    KT_FUN_COS = 4,
    KT_FUN_LOG = 5,
    KT_FUN_SQRT = 6
};

typedef struct kt_context_s* kt_context_t;
typedef struct kt_matrix_s* kt_matrix_t;

/* ---- runtime ------------------------------------------------------------ */
int kt_abi_version(void);
const char* kt_last_error(void);
int kt_device_count(int* count);
int kt_context_create(int device, kt_context_t* ctx);
int kt_context_destroy(kt_context_t ctx);

/* Device-resident A (SURVEY.md §7 hard part (e): fmincon and greedy call the
 * shim repeatedly with the same A, so the CSR stays in HBM across calls).
 * Replaces the sparse `A` argument of trace_exp.m:1, mc_trace.m:32-34,
 * trace_fun_update.m:1, fun_update.m:1, fun_and_grad_krylov_exp.m:1,
 * fun_and_grad_krylov_fun.m:1.  `check_symmetric` != 0 rejects a
 * non-symmetric A with KT_ERR_NOT_HERMITIAN. */
int kt_matrix_create_csc(kt_context_t ctx, int64_t n, const int64_t* colptr,
                         const int64_t* rowind, const double* vals, int check_symmetric,
                         kt_matrix_t* A);
int kt_matrix_destroy(kt_matrix_t A);
int kt_matrix_info(kt_matrix_t A, int64_t* n, int64_t* nnz);

/* ---- hot path: stochastic Lanczos quadrature ------------------------------
 * For probes p in [probe_offset, probe_offset + nprobes) (Rademacher,
 * splitmix64 stream keyed by the GLOBAL probe index, so any sharding over
 * GPUs gives the same probes), run m steps of the single-vector
 * lanczos_krylov recurrence (lanczos_krylov.m:73-115, bs = 1) and form
 * q_p = ||z||^2 e1' f(T_m) e1.  Returns sum_p q_p and sum_p q_p^2 (for the
 * all-reduce of partial traces and the variance), and optionally q[nprobes].
 * `block` = probes per SpMM sweep (power of two 1..128; 0 = auto).
 * This is the Afun of mc_trace.m:45-49 evaluated as quadratic forms and the
 * plain-Hutchinson estimator of BASELINE.json configs 2-4. */
int kt_slq_trace(kt_matrix_t A, int fun, int m, uint64_t seed, int64_t probe_offset,
                 int64_t nprobes, int block, double* sum_q, double* sum_q2, double* q);

/* kt_slq_trace in two halves, for a pipeline of evaluations: submit queues
 * the probe sweeps on the device and returns at once with a ticket; collect
 * waits for THAT call's sweeps only (not for work submitted after it), runs
 * the guard redo and the host quadrature and returns what kt_slq_trace
 * returns.  So evaluation k + 1's sweeps run on the device while the host
 * finishes evaluation k.  At most two submissions outstanding per context,
 * collected once each in submission order (KT_ERR_ARG otherwise);
 * kt_slq_trace == submit + collect and refuses to run while submissions are
 * outstanding. */
int kt_slq_submit(kt_matrix_t A, int fun, int m, uint64_t seed, int64_t probe_offset, int64_t nprobes,
                  int block, int* ticket);
int kt_slq_collect(kt_matrix_t A, int ticket, double* sum_q, double* sum_q2, double* q);

/* kt_slq_trace with an error-controlled depth: the same probes (seed,
 * probe_offset, nprobes, block as above), each run until the stopping test
 * of kt_lanczos_fmv_auto holds on its own tridiagonal (two consecutive
 * agreements of the quadrature to rtol from depth 8 on, fun = KT_FUN_EXP
 * scaled by exp(-theta_max); a beta < 1e-8 cuts the probe) or m_max rows are
 * reached (m_max <= 0: 128; above 256: KT_ERR_ARG).  rtol <= 0: the default,
 * 1e-12.  q_p is formed from probe p's record truncated at depth[p]; it
 * depends only on (A, seed, p, block, m_max, rtol) and on whether its sweep
 * was redone by the explicit sweep, as kt_slq_trace's does -- not on the
 * other probes of its sweep or call, the lane, or timing.  A probe that
 * reaches m_max unconverged is not an error: *capped counts them
 * (kt_context_stat 6; stat 5 takes the largest depth).  depth (nprobes), q
 * and capped are optional.  Blocking; refused while kt_slq_submit tickets
 * are outstanding.  kt_slq_submit / kt_slq_collect stay fixed-depth. */
int kt_slq_trace_auto(kt_matrix_t A, int fun, int m_max, double rtol, uint64_t seed, int64_t probe_offset,
                      int64_t nprobes, int block, double* sum_q, double* sum_q2, double* q, int* depth,
                      int64_t* capped);

/* The probes-per-sweep width kt_slq_trace picks when block == 0. */
int kt_slq_plan(kt_matrix_t A, int64_t nprobes, int* block);

/* Deflated stochastic estimator of diag f(A) (compute_centrality.m:9-10 is
 * fun = KT_FUN_EXP: the subgraph centrality).  Q (n x kdef column-major,
 * original row numbering, borrowed; NULL exactly when kdef == 0, 0 <= kdef <=
 * 16) has orthonormal columns: max |Q'Q - I| > 1e-8 is KT_ERR_ARG.  With
 * Pi = I - Q Q', F = f(A), G = F Q by m-step Lanczos and H = Q'G,
 *   diag F = d0 + diag(Pi F Pi),  d0 = 2 rowsum(Q .* G) - rowsum((Q H) .* Q),
 * for any orthonormal Q, and E[z .* (Pi F Pi z)] = diag(Pi F Pi) over
 * Rademacher z.  For every probe p of [probe_offset, probe_offset + nprobes)
 * (the stream of kt_slq_trace: splitmix64 keyed by the global probe index):
 * z' = Pi z, the m-step Lanczos tridiagonal T of A from z'/||z'||,
 * y = ||z'|| V f(T) e1, t_p = z .* (y - Q (Q'y)) and q_p = ||z'||^2 e1'f(T)e1.
 *   dsum (n, required) = sum_p t_p        dsum2 (n) = sum_p t_p .* t_p
 *   sum_q = sum_p q_p                     sum_q2 = sum_p q_p^2
 *   d0 (n; zeros when kdef == 0)
 * dsum2, d0, sum_q, sum_q2 are optional.  The estimate is d0 + dsum / N, row
 * i's standard error sqrt((dsum2_i / N - (dsum_i / N)^2) / (N - 1)); in exact
 * arithmetic sum_i dsum_i = sum_q.  All outputs but d0 are plain sums over the
 * probe range: shards of a range add.  block = probes per sweep, a power of
 * two from 1 to 16 (0: 16); nprobes >= 1; 1 <= m <= 256; fun unscaled, as in
 * kt_slq_trace.  Probe p's terms depend only on (A, fun, m, seed, p, block,
 * Q), dsum and dsum2 only on those and the range -- not on the lane count,
 * timing or other calls; the sums are accumulated in sweep order without
 * atomics, so two identical calls return identical bits.  Each sweep in
 * flight keeps its Lanczos basis (m n block doubles): KT_ERR_ALLOC if not
 * even one fits.  Blocking; refused while kt_slq_submit tickets are
 * outstanding. */
int kt_diag_fun(kt_matrix_t A, int fun, int m, uint64_t seed, int64_t probe_offset, int64_t nprobes, int block,
                int64_t kdef, const double* Q, double* dsum, double* dsum2, double* d0, double* sum_q,
                double* sum_q2);

/* The same estimator for entries of f(A) on a pair list.  fun, m, seed,
 * probe_offset, nprobes, block, kdef, Q, sum_q and sum_q2 are kt_diag_fun's,
 * with its checks, probe stream, padded deflation widths and sweep lanes.
 * Pairs e = (ei[e], ej[e]) are 0-based in original row numbering; i == j,
 * repeated pairs and both orientations are allowed, and every pair owns its
 * output slot.  npairs < 1, an index outside [0, n) or a NULL ei, ej or esum
 * is KT_ERR_ARG.  With yt_p = y - Q (Q'y) of probe p (kt_diag_fun's vector),
 *   t_p[e] = (z_i yt_p[j] + z_j yt_p[i]) / 2,     E[t_p[e]] = (Pi F Pi)_ij
 *   esum (npairs, required) = sum_p t_p    esum2 (npairs) = sum_p t_p .* t_p
 *   e0[e] = sum_c (Q_ic G_jc + G_ic Q_jc)
 *           - (sum_c (QH)_ic Q_jc + (QH)_jc Q_ic) / 2     (zeros when kdef == 0)
 * since F = Pi F Pi + Q G' + G Q' - Q H Q' for any orthonormal Q.  esum2 and
 * e0 are optional.  The estimate is e0 + esum / N with kt_diag_fun's standard
 * error; for i == j the terms are kt_diag_fun's own.  All outputs but e0 are
 * plain sums over the probe range: shards add.  A probe's terms depend only
 * on (A, fun, m, seed, p, block, Q) and the pair, esum and esum2 only on those
 * and the range -- not on the lane count, timing or other calls; the sums are
 * accumulated in sweep order without atomics, so two identical calls, and a
 * call on one lane, return identical bits.  KT_ERR_ALLOC if not even one
 * sweep's basis fits.  Blocking; refused while kt_slq_submit tickets are
 * outstanding. */
int kt_entries_fun(kt_matrix_t A, int fun, int m, uint64_t seed, int64_t probe_offset, int64_t nprobes, int block,
                   int64_t kdef, const double* Q, int64_t npairs, const int64_t* ei, const int64_t* ej,
                   double* esum, double* esum2, double* e0, double* sum_q, double* sum_q2);

/* ---- block-Krylov entry points (bs = number of columns of U, <= 128) ------
 * U: n x rk column-major in ORIGINAL row numbering; B: rk x rk column-major.
 * it <= 0 selects the reference default min(100, n). */

/* MATLAB normest(A, tol): power estimate of ||A||_2 (called with tol 1e-2 at
 * fun_and_grad_krylov_exp.m:26 / fun_and_grad_krylov_fun.m:27). */
int kt_normest(kt_matrix_t A, double tol, double* nrm);

/* [Xm, iter, lucky] = trace_fun_update(A, U, B, tol, it, debug, fun)
 * (trace_fun_update.m:1): tr f(A + U B U') - tr f(A) by block Lanczos seeded
 * with U (lanczos_krylov.m), lag-2 stopping, dense path when n <= 130. */
int kt_trace_fun_update(kt_matrix_t A, int64_t rk, const double* U, const double* B, double tol,
                        int it, int fun, double* Xm, int* iter, int* lucky);

/* Elementwise scalar function for a function handle outside enum kt_fun:
 * y[i] = f(x[i]), i < count; called on the host, on the calling thread.
 * Returns 0 on success; any other value aborts the call, which then returns
 * KT_ERR_CALLBACK (the partial result is discarded, never summed). */
typedef int (*kt_scalar_fn)(const double* x, double* y, int64_t count, void* user);

/* trace_fun_update with an arbitrary elementwise handle (trace_fun_update.m:
 * 85-89 `Xm = sum(fun(d1) - fun(d2))`; the same call as kt_trace_fun_update
 * otherwise): f is applied to the two sorted eigenvalue vectors of each
 * projected pair (tGm, Gm), or of A + UBU' and A on the dense path. */
int kt_trace_fun_update_fn(kt_matrix_t A, int64_t rk, const double* U, const double* B, double tol,
                           int it, kt_scalar_fn f, void* user, double* Xm, int* iter, int* lucky);

/* [Xm, iter, lucky, Um] = fun_update(A, U, B, fun, tol, it, debug) with four
 * outputs (fun_update.m:1, Arnoldi branch :77-91): f(A+UBU') - f(A) ~= Um Xm Um'.
 * Xm is ncols x ncols (column-major, buffer of max_cols^2 doubles); Um (may be
 * NULL) is n x ncols.  When the basis reaches n/2 columns the reference's
 * dense fallback applies (:85-90): Um = eye(n), ncols = n. */
int kt_fun_update(kt_matrix_t A, int64_t rk, const double* U, const double* B, int fun, double tol,
                  int it, int64_t max_cols, double* Xm, int64_t* ncols, int* iter, int* lucky,
                  double* Um);

/* [Xm, iter, lucky] = fun_update(A, U, B, fun, tol, it, debug) with at most
 * three outputs (fun_update.m:69-76: the block-Lanczos branch over
 * lanczos_krylov's 2-block window; Xm = f(tGm) - f(Gm) on the projected
 * block tridiagonal, 2-norm lag-2 stop, no dense fallback).  Xm: ncols x
 * ncols column-major (buffer of max_cols^2).  The reference then evaluates
 * Um(:, 1:size(Xm, 1)) on the n x 2rk window (fun_update.m:137), which errors
 * once ncols > 2 rk; that error is the caller's (the MEX shim raises it). */
int kt_fun_update_lanczos(kt_matrix_t A, int64_t rk, const double* U, const double* B, int fun,
                          double tol, int it, int64_t max_cols, double* Xm, int64_t* ncols, int* iter,
                          int* lucky);

/* [f, gr] = fun_and_grad_krylov_exp(X, A, Omega, eA, tol, it, debug)
 * (fun_and_grad_krylov_exp.m:1).  Omega: nomega x 2 column-major, 1-based
 * (MATLAB doubles); X, eA, gr: nomega.  KT_ERR_NOT_HERMITIAN if A is not
 * symmetric ("FUN_AND_GRAD_KRYLOV:: matrix A is not Hermitian"). */
int kt_fun_and_grad_krylov_exp(kt_matrix_t A, int64_t nomega, const double* X, const double* Omega,
                               const double* eA, double tol, int it, double* f, double* gr);

/* [f, gr] = fun_and_grad_krylov_fun(X, A, Omega, fun, dfun, dfA, tol, it, debug, fun_M)
 * (fun_and_grad_krylov_fun.m:1); fun / dfun are kt_fun codes. */
int kt_fun_and_grad_krylov_fun(kt_matrix_t A, int64_t nomega, const double* X, const double* Omega,
                               int fun, int dfun, const double* dfA, double tol, int it, double* f,
                               double* gr);

/* ---- mc_trace / trace_exp / expmv --------------------------------------- */
enum kt_afun { /* the Afun argument of mc_trace.m:1 */
    KT_AFUN_MATRIX = 0,  /* Afun is the matrix itself (mc_trace.m:32-34)              */
    KT_AFUN_LANCZOS = 1, /* f(A) x by m-step Lanczos (north star)   */
    KT_AFUN_EXPMV = 2,   /* @(x) expmv(1, A, x, [], 'double') (trace_exp.m:5)          */
    /* KT_AFUN_LANCZOS with the depth chosen per column by a stopping test
     * (kt_lanczos_fmv_auto below).  The `m` argument of kt_mc_trace,
     * kt_mc_trace_sharded and kt_trace_exp is then the depth cap m_max: m <= 0
     * means 128, at most 256.  A column that reaches the cap unconverged is
     * not an error: the call returns KT_OK and kt_context_stat 6 counts it. */
    KT_AFUN_LANCZOS_AUTO = 3
};

/* [tr, res, it] = mc_trace(Afun, n, tol, maxit, isAreal, debug) (mc_trace.m:1):
 * block Hutchinson, m = 10 columns per round, K = ceil(maxit/30) rounds with
 * nested deflation (mc_trace.m:41-58).  Probes of round it are Rademacher
 * columns (it-1)*20 + [0,10) (S) and + [10,20) (G) of the counter RNG. */
int kt_mc_trace(kt_matrix_t A, int afun, int fun, int m, double tol, int maxit, int isAreal,
                uint64_t seed, double* tr, double* res, int* it);

/* All-reduce (sum) of `count` doubles in place across the ranks of a job;
 * supplied by the caller (torch.distributed / RCCL, MPI, ...).  0 = ok. */
typedef int (*kt_reduce_fn)(double* buf, int64_t count, void* user);

/* mc_trace on `world` GPUs (Hutch++ structure): every rank
 * recomputes S, Q and tr(Q' Afun Q) from the shared seed; the 10 G-probe
 * columns of each round are dealt round-robin (column c to rank c % world),
 * their quadratic forms all-reduced with `allreduce` (one call per round,
 * count = 10) and summed in column order, so every rank returns the same
 * tr / res / it.  KT_AFUN_EXPMV is computed replicated (its Taylor degree is
 * chosen per block, expmv.m:41) and never calls `allreduce`.  Replaces
 * mc_trace.m:1-63 on a multi-GPU node; world = 1 equals kt_mc_trace (with a
 * non-NULL `allreduce` the round sums still pass through it, bit-identically;
 * `allreduce` may be NULL only at world = 1). */
int kt_mc_trace_sharded(kt_matrix_t A, int afun, int fun, int m, double tol, int maxit,
                        int isAreal, uint64_t seed, int rank, int world, kt_reduce_fn allreduce,
                        void* user, double* tr, double* res, int* it);

/* tr = trace_exp(A) (trace_exp.m:1-7) = mc_trace(Afun, n, 1e-4, 1000, 1) with
 * Afun = KT_AFUN_EXPMV (the reference composition) or KT_AFUN_LANCZOS (m steps). */
int kt_trace_exp(kt_matrix_t A, int afun, int m, uint64_t seed, double* tr);

/* [F, s, m, mv] = expmv(t, A, B, [], 'double') (expmv.m:1-94; degree selection
 * select_taylor_degree.m, normAm.m for A >= 0).  B, F: n x ncols column-major. */
int kt_expmv(kt_matrix_t A, double t, int64_t ncols, const double* B, double* F, int* s, int* mdeg,
             int* mv);

/* Y = f(A) X by per-column m-step Lanczos: y = ||x|| V f(T) e1 (the Lanczos-f
 * Afun handle).  X, Y: n x ncols column-major, ncols <= 128. */
int kt_lanczos_fmv(kt_matrix_t A, int fun, int m, int64_t ncols, const double* X, double* Y);

/* kt_lanczos_fmv with an error-controlled depth: column c runs Lanczos steps
 * until its own stopping test holds, at most m_max (m_max <= 0: 128; at most
 * 256), and its result is formed from its record truncated at depth[c], so
 * it does not depend on the columns it shares a call with.  The test, at
 * depth j >= 8 on T_j (theta_i, first / last eigenvector rows s_1i, s_ji):
 *   q_j = sum_i s_1i^2 f(theta_i):  |q_j - q_{j-1}| <= rtol |q_j|  and
 *                                   |q_{j-1} - q_{j-2}| <= rtol |q_{j-1}|,
 *   and, when Y is asked for,  beta_j |sum_i s_ji s_1i f(theta_i)|
 *                                   <= rtol (sum_i s_1i^2 f(theta_i)^2)^(1/2);
 * a lucky breakdown (beta < 1e-8) or a zero column stops at once.
 * rtol <= 0: the default, 1e-12.  Y (n x ncols) and quad[c] = x_c' f(A) x_c:
 * each optional, at least one required; depth (ncols) and capped (the number
 * of columns that reached m_max unconverged) optional.  ncols <= 128. */
int kt_lanczos_fmv_auto(kt_matrix_t A, int fun, int m_max, double rtol, int64_t ncols, const double* X,
                        double* Y, double* quad, int* depth, int* capped);

/* [Q, R] = qr(W, 0) on the device (MATLAB's economy Householder QR: LAPACK
 * reflector signs, tau = 0 completions of exactly dependent columns), the
 * factorisation lanczos_krylov.m:90, arnoldi_krylov.m:99 and mc_trace.m use.
 * W, Q: n x bs column-major, R: bs x bs column-major, 1 <= bs <= 128. */
int kt_householder_qr(kt_context_t ctx, int64_t n, int64_t bs, const double* W, double* Q,
                      double* R);

/* Host symmetric eigensolver used for the small projected matrices (the
 * m x m / 2j x 2j eig of trace_fun_update.m:83-84, lanczos quadrature):
 * Householder tridiagonalisation + implicit QL.  A: n x n column-major
 * (symmetric), w: n eigenvalues (unsorted), V: n x n eigenvectors or NULL.
 * Pure host code (no device needed). */
int kt_host_sym_eig(int n, const double* A, double* w, double* V);

/* Host Gauss quadrature of one probe's m x m symmetric tridiagonal T
 * (alpha: m diagonal entries, off: m - 1 off-diagonal ones), the per-probe
 * step after every sweep (trace_fun_update.m:78-84 restated for a single
 * vector: e1' f(T) e1 = sum_k tau_k^2 f(theta_k)): one implicit-shift QL pass
 * rotating the first row of the eigenvector matrix.  q: e1' f(T) e1; fe1
 * (m, nullable): f(T) e1, from the same pass by replaying its rotations (the
 * weights of the Lanczos-f Afun, f(A) x = ||x|| V f(T) e1).  fun: KT_FUN_*.
 * Pure host code (no device needed). */
int kt_host_tridiag_quad(int m, const double* alpha, const double* off, int fun, double* q, double* fe1);

/* The stopping test of the adaptive Lanczos depth (kt_lanczos_fmv_auto) at
 * depth j, 1 <= j <= 256, on one column's tridiagonal: alpha (j), off (j - 1
 * averaged off-diagonals; with want_fe1 != 0 one more, off[j-1] = beta_j, the
 * next one).  An off-diagonal below 1e-8 cuts T there (the lucky breakdown)
 * and sets *converged; below depth 8 nothing else does.  *q = e1' f(T) e1 on
 * the rows used (fun = KT_FUN_EXP: scaled by exp(-theta_max), so it stays
 * finite).  rtol <= 0: the default.  Pure host code (no device needed). */
int kt_host_quad_converged(int j, const double* alpha, const double* off, int fun, int want_fe1,
                           double rtol, int* converged, double* q);

/* ---- greedy edge selection (krylov_miobi.m / greedy_krylov.m) ---------- */

/* Batched trace_fun_update over candidate edges, the inner loop of
 * krylov_miobi.m:76-99.  Candidate c (0-based node indices ei[c], ej[c]):
 *   ei != ej : U = [e_ei, e_ej], B (2 x 2 column-major, Hermitian)
 *   ei == ej : U = e_ei,         B = b_self
 * Xm[c] = tr f(A + U B U') - tr f(A) estimated exactly as trace_fun_update.m
 * does (tol, it, lag-2 stop, lucky breakdown, dense shortcut n <= 130);
 * iter, lucky (nullable) as trace_fun_update's outputs.  Replaces ncand
 * calls of trace_fun_update.m:1 from krylov_miobi.m:99. */
int kt_trace_fun_update_pairs(kt_matrix_t A, int64_t ncand, const int64_t* ei, const int64_t* ej,
                              const double* B, double b_self, double tol, int it, int fun,
                              double* Xm, int* iter, int* lucky);

/* krylov_miobi.m:1 with E given as 0-based pairs (E(j,1) >= E(j,2) in the
 * reference's 1-based form).  make = 0 ('break') or 1 ('make'); rescale as
 * krylov_miobi.m:78-84 (B = -+[0 1;1 0]/rescale).  A is edited IN PLACE
 * (A(i,j) = A(j,i) = 0 or 1, krylov_miobi.m:129-135), the returned A_new.
 * sel_i/sel_j (capacity min(k, nE), nullable) receive the chosen edges in
 * order, rob the summed variation, nsel their count.  Errors: the
 * reference's KRYLOV_MIOBI:: messages. */
int kt_krylov_miobi(kt_matrix_t A, int k, int64_t nE, const int64_t* ei, const int64_t* ej,
                    double tol, int it, int make, double rescale, int64_t* sel_i, int64_t* sel_j,
                    double* rob, int64_t* nsel);

/* The step loop of greedy_krylov.m:64-93 once its search space is ranked
 * (find_top_edges / find_top_missing_edges, greedy_krylov.m:82): ntop >= k
 * ranked pairs ti/tj (0-based).  Step s runs krylov_miobi(A, 1, E, tol, it,
 * ...) on E = the first Q remaining pairs (one selection, A edited in place,
 * :89) and drops the selected pair from the ranking (first match, :84-86).
 * sel_i/sel_j (capacity k, nullable) receive the chosen edges, rob the summed
 * variation (:90), nsel their count.  Replaces the per-step host round trips
 * of calling kt_krylov_miobi k times; same results. */
int kt_greedy_krylov_steps(kt_matrix_t A, int k, int64_t Q, int64_t ntop, const int64_t* ti,
                           const int64_t* tj, double tol, int it, int make, double rescale, int64_t* sel_i,
                           int64_t* sel_j, double* rob, int64_t* nsel);

/* A(i,j) = A(j,i) = value for each pair (value 0 removes the entry, as MATLAB
 * sparse assignment does); device copies are refreshed. */
int kt_matrix_set_pairs(kt_matrix_t A, int64_t count, const int64_t* ei, const int64_t* ej,
                        double value);
/* Copy A back out as CSC (colptr n+1, rowind/vals nnz; sizes from
 * kt_matrix_info).  rowind / vals may be NULL. */
int kt_matrix_export_csc(kt_matrix_t A, int64_t* colptr, int64_t* rowind, double* vals);

/* ---- entries of f(A) (function_multiple_entries.m) -------------------- */

/* X[h] ~= f(A)(oi[h], oj[h]) for h < k (0-based indices) by one Arnoldi run
 * per distinct row index (function_multiple_entries.m:1 with poles = inf);
 * tol / it as the reference (lag-3 stop on f(Gm) e1, it <= 0: min(100, n));
 * iter (nullable) = Krylov steps taken.  Replaces
 * function_multiple_entries.m:1 (Tests/test_weighted_*.m:52-77). */
int kt_function_multiple_entries(kt_matrix_t A, int64_t k, const int64_t* oi, const int64_t* oj,
                                 int fun, double tol, int it, double* X, int* iter);

/* ---- Frechet derivatives and Hessians (multiple_frechet_eval.m,
 *      hessianfcn_exp.m, hessianfcn_fun.m) ----------------------------- */

/* out[h + t * k] = Df(A)(e_oi[h] e_oj[h]')(ti[t], tj[t]) for h < k, t < ntarget
 * (0-based), i.e. the reference's Um{row(i)}(ti, :) * Xm{h} * Vm{col(j)}(tj, :)'
 * from multiple_frechet_eval.m:1 (poles = inf, same tol / it / lag-3 stop).
 * A must be symmetric (the Hessians' A + XX + XX' are).  iter nullable. */
int kt_frechet_entries(kt_matrix_t A, int64_t k, const int64_t* oi, const int64_t* oj, int fun,
                       double tol, int it, int64_t ntarget, const int64_t* ti, const int64_t* tj,
                       double* out, int* iter);

/* Hes = hessianfcn_exp(X, A, Omega, tol, it) (fun = KT_FUN_EXP) or
 * hessianfcn_fun(X, A, Omega, f, tol, it): Omega nomega x 2 column-major,
 * 1-based (MATLAB doubles), X nomega, Hes nomega x nomega column-major.
 * Replaces hessianfcn_exp.m:1 / hessianfcn_fun.m:1 (fmincon HessianFcn). */
int kt_hessianfcn(kt_matrix_t A, int64_t nomega, const double* X, const double* Omega, int fun,
                  double tol, int it, double* Hes);

/* Leading eigenpair of symmetric A (compute_centrality.m:15-17: [u, lambda]
 * = eigs(A, 1); centrality = abs(u)): full-reorthogonalisation Arnoldi on
 * the device from the ones vector, restarted from the Ritz vector, residual
 * |h(j+1,j) y(j)| <= tol |lambda| (tol <= 0: machine epsilon); maxit = Krylov
 * steps per restart (<= 0: 300).  v (n, nullable): unit 2-norm, sum(v) >= 0.
 * steps (nullable): total Arnoldi steps.  Largest algebraic eigenvalue (the
 * Perron root of an adjacency matrix). */
int kt_eigs_leading(kt_matrix_t A, double tol, int maxit, double* lambda, double* v, int* steps);

/* The k largest algebraic eigenpairs of symmetric A, 1 <= k <= 32, k <= n.
 * lambda (k, descending); V (n x k column-major, original row numbering,
 * nullable): orthonormal, each column's sign fixed so its sum is >= 0; inside
 * an eigenspace of a multiple eigenvalue the basis is arbitrary.
 * resid (k, nullable): ||A v_i - lambda_i v_i||_2 computed explicitly on the
 * device from the returned vectors, not a Krylov estimate.
 * Converged: resid_i <= tol * max(|lambda_1|, |lambda_k|); tol <= 0: 1e-10.
 * max_spmm <= 0: 2000 block products (16 columns each; the residual check of
 * a restart counts its one or two).  Reaching the cap is not an error:
 * KT_OK, *nconv (nullable) = how many LEADING pairs converged, resid says
 * the rest; at least ceil(k / 16) expansions and one check are always made.
 * spmm (nullable): block products used.  seed keys the start block: column 0
 * is 1/sqrt(n), columns 1..15 Rademacher from the counter RNG keyed by (seed,
 * original row index, column).  The same (A, k, tol, max_spmm, seed) gives the
 * same bits.  Thick-restart block Lanczos (block width 16, basis of 128
 * columns, full reorthogonalisation, Rayleigh-Ritz on the host); n <= 130
 * takes the dense host path (spmm = 0).  k outside 1..min(32, n) or a NULL A
 * or lambda: KT_ERR_ARG before the device is touched; KT_ERR_NOT_HERMITIAN for
 * non-symmetric A; KT_ERR_ARG while kt_slq_submit calls are outstanding;
 * KT_ERR_ALLOC if the basis (136 n doubles) does not fit. */
int kt_eigs_topk(kt_matrix_t A, int k, double tol, int max_spmm, uint64_t seed,
                 double* lambda, double* V, double* resid, int* nconv, int* spmm);

/* The MIOBI edge score from t eigenpairs on a pair list (MIOBIBreakEdge2.m:60-68):
 * score[p] = sum_{k < t} exp(lambda[k]) exp(sign V[pi[p], k] V[pj[p], k]),
 * sign = -2 for removing the pair's edge, +2 for adding it.  lambda (t), V
 * (n x t column-major), pi / pj (npairs, 0-based) and score (npairs) are host
 * arrays; 1 <= t <= 32.  The t terms are added in a fixed order: the same
 * arguments give the same bits.  NULL arguments, t or an index out of range:
 * KT_ERR_ARG before the device is touched. */
int kt_pairs_score_topk(kt_context_t ctx, int64_t n, int t, const double* lambda, const double* V,
                        int64_t npairs, const int64_t* pi, const int64_t* pj, double sign, double* score);

/* MIOBI's top-t edge removal (MIOBIBreakEdge2.m, MIOBIBreakEdge2_weighted.m)
 * with the step loop on the device: k times, score every remaining edge of
 * the upper triangle with the leading t eigenpairs (kt_eigs_topk with tol,
 * max_spmm, seed; column 0 of V taken by absolute value), remove the edge with
 * the smallest score (exactly equal scores: the smaller (max(i, j), min(i, j)),
 * the order of find(triu(A, 1))), and shift the eigenvalues to first order,
 * lambda_k += -2 a_ij V[i, k] V[j, k].  mode 0 (`reference`): V stays as
 * computed, which is what the reference's update amounts to;
 * mode 1 (`paper`): V <- V (I + S), S(r, c) = dH(r, c) / (lambda_c - lambda_r)
 * for r != c (0 where the denominator is 0 or |lambda_c - lambda_r| <= gap_rel
 * |lambda_1|), columns normalised, column 0 by absolute value.  refresh > 0:
 * after every refresh-th step but the last the removals so far are applied to
 * A and the eigenpairs are recomputed; refresh <= 0: never.  The steps between
 * two recomputations are queued without a host synchronisation.  A is edited
 * in place (the selected edges removed).
 * Outputs: sel_i >= sel_j (0-based) and sel_score, k each; lambda_track
 * (nullable), (k + 1) x t ROW-major: row s = the eigenvalues that score step
 * s + 1 (row 0 the computed ones, a recomputation replaces its step's row);
 * V_final (nullable), n x t column-major: V after the last step; *nsel < k
 * when no edge was left; *nconv_min (nullable) the smallest nconv a
 * kt_eigs_topk run returned (an unconverged pair is reported, not an error);
 * *refreshes (nullable) the recomputations.  The same arguments give the same
 * bits.  KT_ERR_ARG before the device is touched for NULL arguments, k < 0, t
 * outside 2..min(32, n), a mode other than 0 / 1 or a negative gap_rel;
 * KT_ERR_NOT_HERMITIAN for non-symmetric A. */
int kt_miobi_break(kt_matrix_t A, int k, int t, int refresh, int mode, double gap_rel, double tol,
                   int max_spmm, uint64_t seed, int64_t* sel_i, int64_t* sel_j, double* sel_score,
                   double* lambda_track, double* V_final, int64_t* nsel, int* nconv_min, int* refreshes);

/* MIOBI's top-t edge addition (MIOBIMakeEdge.m, with t a parameter) with the
 * step loop on the device: k times, take m = min(max degree + k, n) of the
 * CURRENT matrix (k the whole budget), the first m nodes of a stable
 * descending sort of |V(:, 1)| as candidates, score every non-adjacent pair of
 * them, score = sum_{kappa < t} exp(lambda_kappa) exp(2 V[p, kappa] V[r, kappa]),
 * add the pair with the largest score (exactly equal scores: the first in the
 * reference's enumeration, rank of p ascending, then rank of r), and shift the
 * eigenvalues to first order, lambda_kappa += 2 V[p, kappa] V[r, kappa].  The
 * vectors stay as computed between two recomputations, which is what the
 * reference's update amounts to; there is no `paper`
 * mode.  refresh > 0: after every refresh-th step but the last the eigenpairs
 * are recomputed on the edited matrix (kt_eigs_topk with tol, max_spmm, seed);
 * refresh <= 0: never.  The steps between two recomputations are queued
 * without a host synchronisation.  A must hold unit weights (the reference
 * binarises its input) and at least one entry; it is edited in place (the
 * selected pairs set to 1).
 * Outputs: sel_i >= sel_j (0-based) and sel_score, k each; lambda_track
 * (nullable), (k + 1) x t ROW-major: row s = the eigenvalues that score step
 * s + 1 (a recomputation replaces its step's row); cand_m (nullable, k ints):
 * the m of every step; *nsel < k once no non-adjacent candidate pair is left;
 * *nconv_min (nullable) the smallest nconv a kt_eigs_topk run returned;
 * *refreshes (nullable) the recomputations.  The same arguments give the same
 * bits.  KT_ERR_ARG before the device is touched for NULL arguments, k < 0, t
 * outside 2..min(32, n), a matrix that is empty or not unit-weight, or
 * outstanding kt_slq_submit calls; KT_ERR_NOT_HERMITIAN for non-symmetric A;
 * KT_ERR_ALLOC if the candidate block (m x m / 8 bytes of adjacency bits) does
 * not fit.  On any error A is left as it was. */
int kt_miobi_make(kt_matrix_t A, int k, int t, int refresh, double tol, int max_spmm, uint64_t seed,
                  int64_t* sel_i, int64_t* sel_j, double* sel_score, double* lambda_track,
                  int* cand_m, int64_t* nsel, int* nconv_min, int* refreshes);

/* The MIOBI node score from t eigenpairs on the rows of A (MIOBIBreakNode.m:
 * 186-202): score[r] = sum_{k < t} exp(lambda[k]) exp(-2 V[r, k] W[r, k]) with
 * W[r, .] the sum of the rows of V over the neighbours of r; +Inf for a node
 * without a neighbour.  lambda (t), V (n x t column-major, used as given) and
 * score (n) are host arrays; 1 <= t <= 32.  A row's neighbours and the t terms
 * are added in a fixed order: the same arguments give the same bits.  Errors
 * as kt_miobi_break_node's, without k and shift. */
int kt_nodes_score_topk(kt_matrix_t A, int t, const double* lambda, const double* V, double* score);

/* MIOBI's top-t node removal (MIOBIBreakNode.m's second loop, with t and the
 * recomputation threshold parameters) with the step loop on the device: k
 * times, score every node that still has a neighbour with the leading t
 * eigenpairs (kt_eigs_topk with tol, max_spmm, seed; column 0 of V taken by
 * absolute value), remove the node with the smallest score (exactly equal
 * scores: the smaller index) -- its row and column are cleared -- and shift
 * the eigenvalues.  shift 0 (`reference`): lambda_k -= 2 V[r, k] s_k -
 * V[r, k]^2 with s_k the sum of column k over ALL n rows, which is what the
 * reference's deltaA (the whole row and column at -1, :216-217) gives; shift 1
 * (`first_order`): lambda_k -= 2 V[r, k] W[r, k] over the entries actually
 * removed.  The vectors stay as computed between two recomputations, which is
 * what the reference's update amounts to.  Every step
 * adds 2 deg(r) to a count of removed entries; refresh > 0: once the count
 * reaches refresh it is taken mod refresh and, unless the step was the last,
 * the eigenpairs are recomputed on the edited matrix (the reference uses 50);
 * refresh <= 0: never.  The steps between two recomputations are queued
 * without a host synchronisation; the device ends the window.  A must hold
 * unit weights and a zero diagonal; it is edited in place.
 * Outputs: sel (0-based), sel_score and sel_deg (the node's degree when it
 * was removed), k each; lambda_track (nullable), (k + 1) x t ROW-major: row s
 * = the eigenvalues that score step s + 1 (a recomputation replaces its step's
 * row); *nsel < k once no node has a neighbour; *nconv_min (nullable) the
 * smallest nconv a kt_eigs_topk run returned; *refreshes (nullable) the
 * recomputations.  The same arguments give the same bits.  KT_ERR_ARG before
 * the device is touched for NULL arguments, k < 0, t outside 2..min(32, n), a
 * shift other than 0 / 1, a matrix that is not unit-weight or has a diagonal
 * entry, or outstanding kt_slq_submit calls; KT_ERR_NOT_HERMITIAN for
 * non-symmetric A.  On any error A is left as it was. */
int kt_miobi_break_node(kt_matrix_t A, int k, int t, int refresh, int shift, double tol, int max_spmm,
                        uint64_t seed, int64_t* sel, double* sel_score, int64_t* sel_deg,
                        double* lambda_track, int64_t* nsel, int* nconv_min, int* refreshes);

/* Node removal scored exactly.  For every candidate node
 * nodes[c] (0-based; duplicates are legal) Xm[c] ~= tr f(A_{-i}) - tr f(A),
 * where A_{-i} is A with row and column i zeroed (the node stays as an isolated
 * vertex, as kt_miobi_break_node leaves it).  Removing node i is a rank-2
 * update whose block Krylov space is the single-vector space of e_i, so with
 * T_j the Lanczos tridiagonal started at e_i
 *   X_j = f(0) + sum f(eig(T_j[2:j, 2:j])) - sum f(eig(T_j)),
 * and the stopping rule is trace_fun_update.m:104-124: stop at the first j > 2
 * with |X_j - X_{j-2}| < tol (absolute, the tol of kt_trace_fun_update_pairs),
 * or with lucky = 1 at a step whose beta_j < 1e-8.  The candidates are columns
 * of explicit CGS2 sweeps 16 wide on up to four lanes, the rule applied on the
 * device after every step; Xm comes from the host on the record cut at the
 * column's depth, so a candidate's Xm, iter and lucky depend on (A, node, tol,
 * it, fun) only -- not on what shares its sweep or its call -- bit for bit.
 * tol <= 0: 1e-12.  it <= 0: min(100, n).  iter, lucky (nullable, ncand each):
 * as kt_trace_fun_update's; a column that reaches `it` unstopped returns its
 * last X with iter = it.  n <= 130 takes the dense host path (eig of A and of
 * A_{-i}), iter = 0.
 * KT_ERR_ARG before the device is touched for fun = KT_FUN_LOG (f(0) is not
 * finite), it > 256, NULL arguments, a node index outside 0..n-1 or
 * outstanding kt_slq_submit calls; KT_ERR_NOT_HERMITIAN for non-symmetric A. */
int kt_trace_fun_update_nodes(kt_matrix_t A, int64_t ncand, const int64_t* nodes, double tol, int it,
                              int fun, double* Xm, int* iter, int* lucky);

/* The greedy loop over kt_trace_fun_update_nodes: up to k times, score every
 * remaining candidate on the current A, take the smallest Xm (the first in
 * the list on ties), zero that node's row and column in place (the edit
 * kt_matrix_set_pairs makes), drop it from the list and add its Xm to *rob.
 * Stops after k steps or when the list is empty.  Outputs: sel (0-based) and
 * sel_xm (nullable), min(k, ncand) each; *rob (nullable) the summed Xm, an
 * estimate of tr f(A_new) - tr f(A); *nsel the steps made.  Arguments and
 * errors as kt_trace_fun_update_nodes', and k < 0. */
int kt_krylov_break_node(kt_matrix_t A, int k, int64_t ncand, const int64_t* nodes, double tol, int it,
                         int fun, int64_t* sel, double* sel_xm, double* rob, int64_t* nsel);

/* The value kt_trace_fun_update_nodes forms at depth j: X_j above from the
 * tridiagonal (alpha[0..j-1], off[0..j-2]) of a Lanczos run started at e_i, by
 * the host QL.  1 <= j <= 256; fun any kt_fun but KT_FUN_LOG.  Host only. */
int kt_host_node_update(int j, const double* alpha, const double* off, int fun, double* xm);

/* Proved bounds on subgraph centrality.  For every candidate
 * node nodes[c] (0-based; duplicates are legal) lo[c] <= exp(A)_ii <= hi[c] by
 * Golub-Meurant quadrature on the Lanczos run started at e_i: with T_j its
 * tridiagonal, the Gauss rule sum z_k^2 exp(theta_k) over the eigenpairs of
 * T_j is a lower bound, and the Gauss-Radau rule -- the same sum over T_j
 * bordered by beta_j with last diagonal entry lam_hi + beta_j^2 / d_j, d the
 * pivots of T_j - lam_hi I -- an upper bound when lam_hi >= lambda_max(A); both
 * tighten monotonically with j.  The bounds hold for f = exp only (every
 * derivative positive), so the entry takes no kt_fun.  The candidates are
 * columns of kt_trace_fun_update_nodes' sweeps (explicit CGS2, 16 wide, up to
 * four lanes) with the bracket evaluated on the device after every step; a
 * column stops at the first depth j with
 *   flag 1: beta_j < 1e-8 -- the Gauss rule is exact, hi = lo;
 *   flag 2: a Ritz value of T_j above lam_hi or a pivot d_k >= 0 -- lam_hi is
 *           proved to be below lambda_max(A); lo still holds, hi is NaN;
 *   flag 0: hi - lo <= rtol lo;
 *   flag 3: j = it, the last bracket, still a valid one (also a column the
 *           device stopped on a gap that the returned values miss by rounding).
 * lo, hi and flag come from the host on the record cut at the column's depth
 * (kt_host_gauss_radau), so a candidate's lo, hi, iter and flag depend on (A,
 * node, lam_hi, rtol, it) only -- not on what shares its sweep or its call --
 * bit for bit.  Both sums are formed scaled by exp(-lam_hi) and multiplied by
 * exp(lam_hi) once.  rtol <= 0: 1e-10.  it <= 0: min(100, n).  iter, flag
 * (nullable, ncand each).  n <= 130 takes the dense host path (lo = hi = the
 * diagonal of exp(A) from one eigendecomposition), iter = 0, flag = 0.
 * KT_ERR_ARG before the device is touched for NULL arguments, a node index
 * outside 0..n-1, it > 256, a lam_hi that is not finite or above 700, or
 * outstanding kt_slq_submit calls; KT_ERR_NOT_HERMITIAN for non-symmetric A. */
int kt_diag_fun_bracket(kt_matrix_t A, int64_t ncand, const int64_t* nodes, double lam_hi, double rtol, int it,
                        double* lo, double* hi, int* iter, int* flag);

/* The bracket kt_diag_fun_bracket forms at depth j from the tridiagonal
 * (alpha[0..j-1], off[0..j-2]) of a Lanczos run started at e_i, its next
 * off-diagonal beta_j and the Radau node mu, by the host QL: *lo and *hi (times
 * exp(mu)), *flag 0 a bracket, 1 beta_j < 1e-8 (hi = lo), 2 mu proved below
 * lambda_max (hi = NaN).  1 <= j <= 256, mu finite and <= 700.  Host only. */
int kt_host_gauss_radau(int j, const double* alpha, const double* off, double beta_j, double mu, double* lo,
                        double* hi, int* flag);

/* Proved bounds on communicability.  For every pair (ei[p],
 * ej[p]) (0-based, i != j; repeats are legal) lo[p] <= exp(A)_ij <= hi[p].  With
 * z+- = e_i +- e_j and g+- = (z+- / sqrt 2)' exp(A) (z+- / sqrt 2), exp(A)_ij =
 * (g+ - g-) / 2; each g is a quadratic form of exp, bracketed as
 * kt_diag_fun_bracket brackets exp(A)_ii by the Gauss rule L and the
 * Gauss-Radau rule U of the Lanczos run started at z+- / sqrt 2, so
 *   lo = (L+ - U-) / 2,  hi = (U+ - L-) / 2.
 * A pair is canonicalised to (min, max) first: (i, j) and (j, i) return the
 * same bits.  It takes two adjacent columns of kt_diag_fun_bracket's sweeps (8
 * pairs a sweep); at every depth j, in this order:
 *   a column whose own beta_j < 1e-8 becomes exact (U := L) and is frozen at
 *           depth j while the other one goes on;
 *   flag 2: a running column proves lam_hi below lambda_max(A) (a pivot d_k >=
 *           0 or a Ritz value above lam_hi): lo = hi = NaN;
 *   flag 1: both columns are frozen: lo = hi;
 *   flag 0: lo hi > 0 and 0 <= hi - lo <= rtol min(|lo|, |hi|);
 *   flag 4: hi - lo <= ftol (U+ + U-) / 2 -- the bracket has closed to the
 *           rounding level of the two quadratic forms, whose size is that of
 *           (exp(A)_ii + exp(A)_jj) / 2, and the entry lies below what the
 *           method resolves; such a bracket can come out inverted (hi < lo) by
 *           a few ulps of that scale;
 *   flag 3: j = it, the last bracket, still a valid one.
 * The device decides depths only; lo, hi and flag come from the host rule on
 * each column's record cut at that column's depth (col_iter, 2 per pair: the +
 * and the - column; iter is the larger), the flag judged on the values
 * returned: a device flag 0 that they miss by rounding falls to 4 or 3.  So a
 * pair's results depend on (A, i, j, lam_hi, rtol, ftol, it) only -- not on what
 * shares its sweep or its call -- bit for bit.  The sums are formed scaled by
 * exp(-lam_hi) and multiplied by exp(lam_hi) once.  rtol <= 0: 1e-10.  ftol <=
 * 0: 1e-12.  it <= 0: min(100, n).  iter, flag (npairs each) and col_iter (2
 * npairs) are nullable.  n <= 130 takes the dense host path (lo = hi = the
 * entry from one eigendecomposition), iter = 0, flag = 0.  f = exp only.
 * KT_ERR_ARG before the device is touched for NULL arguments, an index outside
 * 0..n-1, a pair with i == j (kt_diag_fun_bracket bounds those), it > 256, a
 * lam_hi that is not finite or above 700, or outstanding kt_slq_submit calls;
 * KT_ERR_NOT_HERMITIAN for non-symmetric A. */
int kt_entries_fun_bracket(kt_matrix_t A, int64_t npairs, const int64_t* ei, const int64_t* ej, double lam_hi,
                           double rtol, double ftol, int it, double* lo, double* hi, int* iter, int* flag,
                           int* col_iter);

/* Per-kernel timing (HIP events recorded on the library's stream around each
 * launch of the named kernel while enabled).  kernel: 0 = the probe-Lanczos
 * gather pass (k_spmm_lanczos in the y-form sweep, k_spmm_dot = K1 in the
 * explicit sweep), 1 = K2 (k_update, explicit sweep only), 2 = the y-form
 * start pass (k_spmm_lanczos_start), 5 = the first step of a compact y-form
 * sweep alone (k_spmm_lanczos_first; the launch is also counted among the
 * sweep's passes in 0), 3 = the y-form pass of a sweep seeded
 * by a given block (k_spmm_lanczos in mc_trace's quadrature-only columns),
 * 4 = the expmv Taylor-term kernel (k_expmv_rows / k_expmv_step, one launch
 * per term; a term queued past its stage's stop is a short no-op launch),
 * 6 = the stopping test of kt_slq_trace_auto's sweeps (k_quad_check_wide),
 * 7 = kt_diag_fun's combine and accumulate kernels (k_diag_combine,
 * k_diag_finish), 8 = its start-block kernels (k_diag_qtz, k_diag_start; its
 * sweeps' passes report in 3, or 0 and 1 for a sweep redone explicitly),
 * 9 = kt_entries_fun's pair kernels (k_entries_accumulate, k_entries_e0; its
 * sweeps, start blocks and combine report in 3, 8 and 7 as kt_diag_fun's do),
 * 10 = kt_eigs_topk's own kernels (k_eig_start, k_eig_rotate, k_eig_resid with
 * its chunk sum; the solver's block SpMM, Gram and combine launches are the
 * block-Krylov paths' own and are not event-timed),
 * 11 = kt_miobi_break's steps, one interval per step (k_miobi_score,
 * k_miobi_pick and, in mode 1, the rotation and normalisation), and
 * kt_pairs_score_topk's scoring launch,
 * 12 = kt_miobi_make's steps, one interval per step (k_miobi_make_score,
 * k_miobi_make_pick),
 * 13 = kt_miobi_break_node's steps, one interval per step (k_miobi_node_score,
 * k_miobi_node_pick; a step queued past its window's end is a pair of no-op
 * launches), and kt_nodes_score_topk's scoring launch,
 * 14 = kt_trace_fun_update_nodes' own launches: the stopping tests
 * (k_node_check, one interval per sweep and depth) and the unit-vector starts
 * (k_unit_start); its sweeps' passes report in 0 and 1.  kt_diag_fun_bracket's
 * (k_bracket_check, k_unit_start) and kt_entries_fun_bracket's
 * (k_pair_bracket_check, k_pair_start) report here too.
 * Returns launch count and summed milliseconds. */
int kt_profile_enable(kt_context_t ctx, int enable);
int kt_profile_read(kt_context_t ctx, int kernel, int64_t* launches, double* total_ms);
int kt_profile_reset(kt_context_t ctx);
/* The same totals restricted to launches of sweep width `width` (the probe
 * block P of the sweep that launched them). */
int kt_profile_read_width(kt_context_t ctx, int kernel, int width, int64_t* launches, double* total_ms);
/* Wall time during which at least one launch of `kernel` was in flight (the
 * union of the launches' event intervals, on whichever sweep-lane stream
 * each ran): with several lanes overlapping, summed per-launch durations
 * count shared time twice; this does not. */
int kt_profile_busy(kt_context_t ctx, int kernel, double* busy_ms);

/* Test hook: queue a kernel that keeps sweep lane `lane` (0 = the context's
 * stream, 1..3 = the extra sweep-lane streams kt_slq_submit uses) busy for
 * `microseconds` (<= 1e6) and return at once.  Lets a test make one lane's
 * sweeps finish after another's (the profiler's out-of-order completion). */
int kt_debug_delay(kt_context_t ctx, int lane, double microseconds);

/* Hot-path statistics.  stat 0: kt_slq_trace sweeps whose y-form probe
 * Lanczos tripped the cancellation guard (a lucky breakdown, or a beta^2
 * below 1e-4 ||A v||^2) and were recomputed by the explicit CGS2 sweep,
 * counted since context creation.  stat 1: fun_update runs (kt_fun_update,
 * kt_fun_and_grad_krylov_*) that took the dense fallback of fun_update.m:85-90,
 * since context creation.  stat 2: the projected size (basis columns) of the
 * last fun_update run on this context (n when it went dense).  stat 3: expmv
 * calls (kt_expmv and mc_trace's expmv Afun), stat 4: the Taylor terms they
 * executed (one A b product on the block each, expmv.m:75), since context
 * creation.  stat 5: the largest Lanczos depth the adaptive Afun
 * (KT_AFUN_LANCZOS_AUTO, kt_lanczos_fmv_auto) used for a column, stat 6: its
 * columns that reached the depth cap unconverged, both since context
 * creation.  stat 7: kt_slq_trace y-form sweeps that carried y_0 as int16 row
 * sums (kt_host_int0_applies; KT_SLQ_INT0=0, read per call, turns the form
 * off), since context creation.  stat 8: y-form step passes queued by
 * kt_slq_trace_auto calls (those queued past a sweep's last stop, which
 * return at once, included), since context creation.  stat 9: thick restarts
 * of kt_eigs_topk calls, since context creation.  stats 10, 11, 12: host
 * microseconds of the last kt_miobi_break, kt_miobi_make or
 * kt_miobi_break_node call on this context that got as far as its first
 * eigensolver run -- its eigensolver runs; its candidate ranking, mask
 * construction and uploads (kt_miobi_break: staging V and the eigenvalues;
 * kt_miobi_break_node: those and the window's row lists); its edits of A.
 * stats 13, 14, 15: of the last
 * kt_trace_fun_update_nodes call on this context (kt_krylov_break_node: of its
 * last greedy step), kt_diag_fun_bracket or kt_entries_fun_bracket call -- its sweeps, the sweep steps
 * it queued (one SpMM pass over A each) and the depth of its deepest column. */
int kt_context_stat(kt_context_t ctx, int stat, int64_t* value);

/* Threads of the process-wide host pool (the per-column / per-candidate
 * host work between device steps: Gauss quadratures, the greedy host
 * eigenproblems), the calling thread included: min(16, the CPUs this
 * process may use -- its affinity mask capped by the cgroup CPU quota --
 * divided by LOCAL_WORLD_SIZE, the ranks torchrun started on this node),
 * at least 1; KT_HOST_THREADS overrides.  Fixed at the pool's first use. */
int kt_host_threads(void);

/* Whether kt_slq_trace's y-form sweeps of depth m keep y_0 = A z / ||z|| as
 * int16 row sums on a matrix whose longest row has max_row entries: the
 * matrix is unit-weight (each sum is then an integer of magnitude <= the
 * row's length), max_row <= 32767 and m >= 3.  The results do not depend on
 * it, bit for bit.  Host only. */
int kt_host_int0_applies(int unit_weight, int64_t max_row, int m, int* applies);

#ifdef __cplusplus
}
#endif
#endif /* KRYLOV_TRACE_H */
