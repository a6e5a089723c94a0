// kt_slq.h -- probe-Lanczos sweep engine shared by the SLQ hot path and the
// Lanczos-f Afun of mc_trace.
#pragma once
#include <memory>

#include "kt_block.h"

namespace kt {

int slq_auto_block(int64_t n, int64_t nprobes);

// One sweep of P independent single-vector Lanczos runs (see kt_slq.cpp).
// lane 0 runs on ctx->stream with ws.sweep[0]; lane l > 0 on
// ctx->aux_stream[l-1] with ws.sweep[l] (independent sweeps overlap).
// basis (optional, >= n m bcols doubles): slot j = u_j's first bcols columns
// as an n x bcols row-major block at basis->col(0) + j n bcols.
void lanczos_sweep(kt_matrix_s* A, const DevCSR& M, int P, int m, uint64_t seed, int64_t probe_base,
                   const double* x, int ldx, int ncols, const double* dnorms2, double* rec_host,
                   DevMat* basis, std::vector<double>* scale_hist, int lane = 0, int bcols = 0);

// What the sweep classes share on lane `lane`: the lane check, its stream
// (lane 0: ctx->stream; lane l > 0: ctx->aux_stream[l-1], created on first
// use by lane_stream), the launch grids of an n x P block and the lane's
// buffers.
hipStream_t lane_stream(kt_context_s* ctx, int lane);
struct SweepLane {
    SweepLane(kt_matrix_s* A, const DevCSR& M, int P, int lane);
    hipStream_t st;
    int grid, lblocks, grid1;  // K2 / short rows, long-row blocks, K1 total
    size_t blk_bytes;          // one n x P fp64 block
    SweepBufs& w;
};

// A sweep enqueued step by step: start(), step(j) for j < nsteps(), finish().
// run_sweeps queues a list launch by launch -- every start() in list order,
// then for j = 0, 1, .. step(j) of each sweep with j < nsteps(), then every
// finish() -- so sweeps on different lanes start at once (the runtime
// throttles a long enqueue burst to ~58 us per call once the host runs ~1 ms
// ahead, so a lane queued after a whole sweep would start ms late).  Two
// sweeps on one lane may not share a list (they share the lane's buffers).
struct Sweep {
    virtual ~Sweep() = default;
    virtual void start() = 0;
    virtual void step(int j) = 0;
    virtual void finish() = 0;
    virtual int nsteps() const = 0;
};
using SweepList = std::vector<std::unique_ptr<Sweep>>;
void run_sweeps(const SweepList& sweeps);

// lanczos_sweep as a Sweep of m steps.
class ExplicitSweep : public Sweep {
   public:
    ExplicitSweep(kt_matrix_s* A, const DevCSR& M, int P, int m, uint64_t seed, int64_t probe_base, const double* x,
                  int ldx, int ncols, const double* dnorms2, double* rec_host, DevMat* basis,
                  std::vector<double>* scale_hist, int lane, int bcols);
    void start() override;
    void step(int j) override;
    void finish() override;
    int nsteps() const override { return m; }
    // The resumable form (lanczos_columns_adaptive): a sweep constructed with
    // capacity m (record rows, scale history, basis slots) runs step(j) only
    // as far as needed; finish(rows) copies the rows written.  The basis of
    // its first bcols columns may live in growth chunks of `spc` slots each
    // (slot j in (*chunks)[j / spc], allocated when step j - 1 is queued)
    // instead of one m-slot block: pass basis = nullptr and call this before
    // start().
    void use_basis_chunks(std::vector<DevMat>* chunks, int spc);
    // The unit-vector start (lanczos_nodes_adaptive): a sweep constructed with
    // x = nullptr and ncols columns starts column c at e_{pos[c]}, pos a device
    // array of rows in M's order, instead of the RNG's probes (kt_adapt.hip
    // k_unit_start).  Call before start().
    void use_unit_start(const int* pos_dev);
    // The pair start (lanczos_pairs_bracket): ncols = 2 np columns, columns 2p
    // and 2p + 1 start at (e_i + e_j) / sqrt 2 and (e_i - e_j) / sqrt 2 with i =
    // pos[2p], j = pos[2p + 1] (kt_adapt.hip k_pair_start).  Call before start().
    void use_pair_start(const int* pos_dev);
    void finish(int rows);
    const double* device_record() const { return trec; }
    hipStream_t stream() const { return L.st; }

   private:
    double* slot(int j);
    std::vector<DevMat>* chunks = nullptr;
    int spc = 0;
    const int* unit_pos = nullptr;
    bool pair_start = false;
    kt_matrix_s* A;
    const DevCSR& M;
    int P, m;
    uint64_t seed;
    int64_t probe_base;
    const double* x;
    int ldx, ncols;
    const double* dnorms2;
    double* rec_host;
    DevMat* basis;
    std::vector<double>* scale_hist;
    int bcols, n;
    SweepLane L;
    double *part1 = nullptr, *part2 = nullptr, *k2s = nullptr, *coef = nullptr, *trec = nullptr, *Yb = nullptr;
    double *ucur = nullptr, *uprev = nullptr, *sc = nullptr, *sp = nullptr, *sn = nullptr, *bbase = nullptr;
    DevBuf* hist_dev = nullptr;
};

// Whether a sign-table-seeded y-form sweep of depth m may carry y_0 as int16
// row sums: unit weights, so a row's start-pass sum is an
// integer of magnitude <= its length, every row at most 32,767 long, and at
// least one ordinary pass after the start (m >= 3; at m = 2 the only pass is
// the half-gather last pass, which has no int16 variant).
inline bool int0_applies(bool unit_values, int64_t max_row, int m) {
    return unit_values && max_row <= 32767 && m >= 3;
}

// The y-form sweep as a Sweep of m - 1 steps, seeded one of two ways.
// Sign-seeded (the Hutchinson hot path): the probes are a packed sign table
// from the counter RNG.
// int0: the compact form -- the start pass stores y_0 as an n x P int16 table
// behind the sign table, the first step (k_spmm_lanczos_first) gathers it and
// the second reads it as Yold; from the third step on nothing differs, and
// every record is bit-identical to the fp64 form's.
// The resumable form (slq_trace_auto): constructed with gate != nullptr and m
// the record's row capacity, every step(j) is the ordinary pass in its gated
// form (never the half-gather last pass), so record row j + 1 is complete
// after it and T_{j+2} can be tested; finish(rows) copies the rows written
// and the guard.  int0 then needs int0_applies at the depth the sweep may
// reach.  A fixed-depth sweep (gate == nullptr) queues what it always did.
// Block-seeded (lanczos_sweep_y_block): the ncols columns of the device block
// x.  With `basis` (m slots of n x P, slot j at basis + j n P; bcols > 0) the
// sweep also forms the normalised Lanczos vectors v_0 .. v_{m-1} of its
// first bcols columns there (KF_VB passes; v_0 is the start table itself).
class YSweep : public Sweep {
   public:
    YSweep(kt_matrix_s* A, const DevCSR& M, int P, int m, uint64_t seed, int64_t probe_base, double* rec_host,
           int lane, bool int0 = false, const int* gate = nullptr, int ngate = 0);
    YSweep(kt_matrix_s* A, const DevCSR& M, int P, int m, const double* x, int ldx, int ncols, const double* dnorms2,
           double* rec_host, int lane, double* basis = nullptr, int bcols = 0);
    void start() override;
    void step(int j) override;
    void finish() override;
    int nsteps() const override { return m - 1; }
    void finish(int rows);
    const double* device_record() const { return trec; }
    const double* device_guard() const { return guard; }
    hipStream_t stream() const { return L.st; }

   private:
    void setup();
    double* rec_at(int row, int j) { return trec + (size_t)(row * m + j) * P; }
    double* slot(int j) { return basis ? basis + (size_t)j * n * P : nullptr; }
    kt_matrix_s* A;
    const DevCSR& M;
    int P, m, n;
    double* rec_host;
    SweepLane L;
    // the sign seed
    uint64_t seed = 0;
    int64_t probe_base = 0;
    bool int0 = false;
    const int* gate = nullptr;  // the resumable form: the sweep's running words
    int ngate = 0;
    // the block seed (x != nullptr)
    const double* x = nullptr;
    int ldx = 0, ncols = 0;
    const double* dnorms2 = nullptr;
    double* basis = nullptr;
    int bcols = 0;
    int flags = 0;
    double *part = nullptr, *ys = nullptr, *trec = nullptr, *guard = nullptr;
    uint32_t* Z = nullptr;   // the sign table
    int16_t* T0 = nullptr;   // int0: y_0's row sums
    double* V0 = nullptr;    // the block seed's gathered table v_0 (basis slot 0)
    double *Xc = nullptr, *Yo = nullptr, *Ot = nullptr;
    double s0 = 1.0;         // the start's scale: 1 / ||z|| (the block seed is normalised: 1)
};

// A y-form probe is accepted when every used beta_k^2 kept at least this
// fraction of ||y_{k-1}||^2 (its Gram-identity cancellation then costs at most
// ~1e4 ulp); otherwise its sweep is recomputed by the explicit CGS2 sweep.
// Measured minimum on the golden graphs and Chung-Lu up to m = 100: 6.4e-3.
constexpr double kYformGuard = 1e-4;

// Whether a live column of a y-form record R ([alpha | up | low][m][P], then
// guard[P]) tripped the guard; n2 (nullable): the columns' squared norms,
// zero columns never trip.
bool guard_tripped(const double* R, int m, int P, int live, const double* n2);

// Column c of a sweep record with row capacity mcap, cut at depth d (a
// fixed-depth record: d == mcap) -> symmetric tridiagonal (alpha, off);
// returns the number of steps before a lucky breakdown (lanczos_krylov.m:91-93).
int record_tridiag(const double* R, int mcap, int d, int P, int c, double* al, double* off);

// One f(A) x column's basis weights W[j ldw] = ||x|| fe1_j (j < steps) for a
// y-form basis (normalised v_j; hist == nullptr), ||x|| hist[j P] fe1_j for an
// explicit-layout one (v_j = s_j u_j, hist the column's scale history).
void basis_weights(int steps, double nx, const double* fe1, const double* hist, int P, double* W, int ldw);

// KT_SLQ_LANES (else dflt; the caller clamps to [1, 4]) and KT_SLQ_INT0 (0:
// the y-form sweeps keep y_0 in fp64, the A/B of the compact form).
int slq_lanes_env(int dflt);
bool slq_int0_env();

// For the ncols columns of the device block X (n x ldx, natural row order):
// quad[c] = x_c' f(A) x_c by m-step Lanczos quadrature (may be NULL) and, if
// Y != NULL, Y[:, c] = ||x_c|| V_c f(T_c) e1 ~= f(A) x_c.
void lanczos_columns(kt_matrix_s* A, const double* X, int ldx, int ncols, int m, int fun,
                     double* quad, double* Y, int ldy);

// lanczos_columns for a block whose first ny columns need f(A) x (into Y)
// and every column its quadratic form: columns [0, ne) by the explicit CGS2
// sweep (sweeps of px columns, or pow2 >= ne capped at 16 when px = 0), the
// basis kept for the ny f(A)x columns; columns [ne, ncols) -- quadratic
// forms only -- by y-form sweeps (one pass per step, no K2, no basis) on the
// extra sweep lanes, all queued together.  A column's form depends only on
// the widths of the sweeps, which depend only on (ncols, ny, ne, px) -- not
// on the values (zero columns included).  The y-form suits random probes;
// columns that start close to an invariant subspace (mc_trace's Q) trip its
// cancellation guard and belong in [0, ne).
// ychunk: columns per y-form sweep (each sweep at the power of two >= its
// columns, <= 16): 16 packs them; a smaller chunk splits them evenly (mc_trace's
// final round: [Q | pad] and [G | pad] instead of 16 + 4).
// yb (<= ny): the first yb columns run as y-form sweeps that also form their
// Lanczos basis (KF_VB) instead of the explicit sweep: columns [0, yb) y-form
// with basis, [yb, ne) explicit, [ne, ncols) y-form forms only.  A y-form
// basis sweep whose guard trips is redone whole by the explicit sweep.
void lanczos_columns_split(kt_matrix_s* A, const double* X, int ldx, int ncols, int ny, int ne, int m, int fun,
                           double* quad, double* Y, int ldy, int px = 0, int ychunk = 16, int yb = 0);

// lanczos_columns_split's column contract (the first ny columns need f(A) x
// into Y, every column its quadratic form) with the depth chosen per column:
// every column by explicit CGS2 sweeps, always 16 wide, each step followed by
// the device stopping test (kt_adapt.hip k_quad_check); a sweep is queued
// until its columns have all stopped or reached m_max (<= 0: 128; <= 256).
// A column's values come from its record truncated at its own depth, by the
// host quadrature lanczos_columns_split uses, so they do not depend on the
// columns it shares a sweep or a call with.  rtol <= 0: kAdaptRtol.
// depth (ncols, nullable): steps used per column (0 for a zero column).
// Returns the number of columns that reached m_max unconverged; the
// context's stats (kt_context_stat 5, 6) follow.
int lanczos_columns_adaptive(kt_matrix_s* A, const double* X, int ldx, int ncols, int ny, int m_max, double rtol,
                             int fun, double* quad, double* Y, int ldy, int* depth = nullptr);

// Node removal: for every candidate node i_c (0-based,
// duplicates legal) Xm[c] ~= tr f(A_{-i}) - tr f(A), A_{-i} = A with row and
// column i zeroed, from the single-vector Lanczos run started at e_i: with T_j
// its tridiagonal, X_j = f(0) + sum f(eig(T_j[2:, 2:])) - sum f(eig(T_j)).
// Candidates are columns of explicit CGS2 sweeps, always 16 wide, on up to
// four lanes; after every step the device applies trace_fun_update.m's lag-2
// rule (kt_adapt.hip k_node_check; tol absolute, lucky at beta_j < 1e-8) and a
// sweep is queued until its columns have all stopped or reached `it` (1..256).
// Xm is formed on the host from the record cut at the column's depth, so it
// depends on (A, i, tol, it, fun) only.  iter / lucky (nullable): the depth and
// whether its beta broke down; a column that reaches `it` unstopped returns
// its last X with iter = it.  The context's stats 13-15 follow.
void lanczos_nodes_adaptive(kt_matrix_s* A, int64_t ncand, const int64_t* nodes, double tol, int it, int fun,
                            double* Xm, int* iter, int* lucky);

// Gauss / Gauss-Radau bracket of exp(A)_ii: for every
// candidate node i_c (0-based, duplicates legal) lo[c] <= exp(A)_ii <= hi[c]
// from the same unit-vector sweeps (16 wide, up to four lanes, `it` in 1..256)
// with kt_adapt.hip k_bracket_check after every step: the Gauss rule of T_j and
// the Gauss-Radau rule with a node at mu >= lambda_max(A), both scaled by
// exp(-mu).  A column stops at the first depth whose gap hi - lo <= rtol lo
// (flag 0), at a beta_j < 1e-8 (1: hi = lo), where mu is proved below
// lambda_max (2: hi = NaN) or at `it` (3).  lo / hi / flag are formed on the
// host from the record cut at the column's depth, so they depend on (A, i, mu,
// rtol, it) only.  iter / flag nullable.  The context's stats 13-15 follow.
void lanczos_nodes_bracket(kt_matrix_s* A, int64_t ncand, const int64_t* nodes, double mu, double rtol, int it,
                           double* lo, double* hi, int* iter, int* flag);

// Gauss / Gauss-Radau bracket of exp(A)_ij, i != j: pair p
// (0-based, i < j, repeats legal) takes two columns of those sweeps, started at
// (e_i +- e_j) / sqrt 2, so a sweep holds 8 pairs; with L, U their Gauss and
// Gauss-Radau sums, lo = (L+ - U-) / 2 <= exp(A)_ij <= hi = (U+ - L-) / 2.
// kt_adapt.hip k_pair_bracket_check decides the depths; lo / hi / flag come
// from pair_bracket_combine on gauss_radau_sums of each column's record cut at
// its own depth (col_iter, nullable, 2 per pair), so they depend on (A, i, j,
// mu, rtol, ftol, it) only.  iter: the deeper column's depth.  iter / flag
// nullable.  The context's stats 13-15 follow.
void lanczos_pairs_bracket(kt_matrix_s* A, int64_t npairs, const int64_t* ei, const int64_t* ej, double mu,
                           double rtol, double ftol, int it, double* lo, double* hi, int* iter, int* flag,
                           int* col_iter);

// y-form sweep seeded by a device block (see kt_slq.cpp)
void lanczos_sweep_y_block(kt_matrix_s* A, const DevCSR& M, int P, int m, const double* x, int ldx, int ncols,
                           const double* dnorms2, double* rec_host, int lane);

}  // namespace kt
