/*
 * nemo.h -- C-ABI of the MI355X order-score engine for Nested Effects Model
 * order MCMC (drop-in for the per-step scorer of MrGreyPanda/NEM-MCMC-optimization).
 *
 * The reference has no FFI layer: its boundary is the Python method surface of
 * NEMOrderMCMC.  Each entry point below replaces one of those
 * methods; the Python host (nemo.nem_order_mcmc) keeps the reference's names
 * and signatures and delegates here through ctypes.
 *
 * Conventions
 *   - plain pointers and sizes; host buffers are caller-owned and only borrowed
 *     for the call; device buffers are owned by the context;
 *   - every call returns NEMO_OK (0) or a negative code, and nemo_last_error()
 *     (thread-local) explains it; the Python host raises RuntimeError with it;
 *   - host-pointer calls are synchronous (the context stream is synchronised
 *     before return); *_dev calls take device pointers and only enqueue work on
 *     the given stream (hipStream_t passed as void*; NULL = HIP's null stream);
 *   - one context per (device, model); calls on one context must not overlap.
 *     Different contexts may be driven from different threads: graph capture
 *     and the calls that allocate or use the legacy stream (create, destroy,
 *     stage, reserve, the probes) serialise on one process-wide lock.
 *
 * Layouts (row-major, C order):
 *   T    [S][S][E]  score table, T[i][j][e]: child i, candidate parent j
 *   U    [S+1][E]   node LR table, row S = "effect attached to nothing"
 *   pos  [batch][S] int32 position of every S-gene in the order (inverse of pi)
 *   w01  [batch][S][S] parent weights already mapped to [0,1]
 *        (the reference maps with expit inside compute_cell_ratios,
 *         nem_order_mcmc.py:84-86; methods.py:52-57 passes them unmapped)
 *   Only entries (i, j) with pos[j] < pos[i] (and, with cap > 0,
 *   pos[i] - pos[j] <= cap) are read: these are the permissible parents.
 */
#ifndef NEMO_H
#define NEMO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nemo_ctx nemo_ctx;

/* table storage / elementwise arithmetic type */
enum { NEMO_F64 = 0, NEMO_F32 = 1 };

/* return codes */
enum {
  NEMO_OK = 0,
  NEMO_ERR_ARG = -1,     /* bad argument (shape, pointer, range)          */
  NEMO_ERR_HIP = -2,     /* HIP runtime error (no device, OOM, launch)    */
  NEMO_ERR_STATE = -3,   /* tables not staged / capacity not reserved     */
  NEMO_ERR_OPT = -5,     /* a local optimisation did not converge         */
  NEMO_ERR_LINALG = -6   /* ancestor_x: I - W~ singular or not finite      */
};

/* per-problem termination codes of the local optimiser (scipy task names) */
enum {
  NEMO_LBFGSB_CONV_PGTOL = 0,  /* CONVERGENCE: NORM_OF_PROJECTED_GRADIENT_<=_PGTOL */
  NEMO_LBFGSB_CONV_REL = 1,    /* CONVERGENCE: REL_REDUCTION_OF_F_<=_FACTR*EPSMCH  */
  NEMO_LBFGSB_ABNORMAL = 2,    /* ABNORMAL_TERMINATION_IN_LNSRCH                  */
  NEMO_LBFGSB_MAXITER = 3      /* STOP: TOTAL NO. of ITERATIONS REACHED LIMIT     */
};

const char* nemo_last_error(void);
int nemo_version(void);
/* identity of this build: a hash of the sources and compile flags it was
 * built from (bench.py matches profiler records against it) */
const char* nemo_build_id(void);
/* number of visible HIP devices (0 on a host without GPU; never an error) */
int nemo_device_count(int* count);

/* option "exact_generic": the largest |T| (off-diagonal rows) and |U| of a
 * generic or row-shared table the exact kernels cover.  U only has to stay
 * inside the SVML exp's fast path.  T is bounded so that a flushed order
 * weight (see "exact") cannot change a local optimum: c = a / b with a =
 * (lv - 1) ow, b = (1 - s) + s lv - s a, lv = e^T, so for a tail weight ow <=
 * e^-707.70 |c| <= max(lv, 1) / min(lv, 1) * e^-707.70 = e^(|T| - 707.70),
 * and 1 + c ex (ex in [0, 1]) is 1 with ow or with 0 once |c| < 2^-54 =
 * e^-37.43: |T| <= 670.27, rounded down (nemo.limits holds the same values) */
#define NEMO_EXACT_GENERIC_MAX_ABS_T 670.0
#define NEMO_EXACT_GENERIC_MAX_ABS_U 700.0

/* nemo_edge_sweep: the most effects one evaluation's block holds in its
 * registers, 16 per thread of 1024 (nemo.limits.MAX_E_EDGE_SWEEP holds the
 * same value); a model with more is refused with NEMO_ERR_ARG */
#define NEMO_EDGE_SWEEP_MAX_E 16384

/* ---- context lifetime (replaces NEMOrderMCMC.__init__'s table setup,
 *      nem_order_mcmc.py:40-46) ------------------------------------------
 * num_s in [2, 256] (a model of one S-gene has no parent pair: num_s = 1 is
 * NEMO_ERR_ARG), num_e >= 1 */
int nemo_ctx_create(int device, int num_s, int num_e, int dtype, nemo_ctx** out);
void nemo_ctx_destroy(nemo_ctx* ctx);
/* grow per-batch scratch so *_dev calls with up to max_batch evaluations
 * (and max_chains chains for nemo_optimal_weights_dev) never allocate: with a
 * model staged (before or after this call) that covers the exact step's
 * buffers as well, so such a _dev call only enqueues and may be captured into
 * the caller's graph.  Without the reservation the first _dev call with more
 * chains allocates and synchronises the context's stream (not capturable). */
int nemo_reserve(nemo_ctx* ctx, int max_batch, int max_chains);

/* ---- A1/A2: stage the model once (nem.py:25-64 outputs) ---------------- */
int nemo_stage_tables(nemo_ctx* ctx, const double* U, const double* T);
/* the same model built on the device from the observed knockdown matrix
 * (nem.py:25-64, the tables NEM.__init__ derives, nem_order_mcmc.py:44):
 *   D [S][E] bytes in {0,1} (NEM.observed_knockdown_mat), A = log(alpha/(1-beta)),
 *   B = log(beta/(1-alpha)) (NEM.A, NEM.B, nem.py:17-18).
 * T[i][j] = where(D[j]==0, B, -A) off the diagonal, T[i][i] = U[i] with
 * U[i] = where(D[i]==1, 0, B) + A per other 1 in the column, U[S] = A per 1.
 * Stages bit-for-bit what nemo_stage_tables stages for those U and T, with
 * no S*S*E host table (655 MB at C5 in fp64). */
int nemo_stage_knockdown(nemo_ctx* ctx, const uint8_t* D, double A, double B);
/* the model of per-effect log-likelihood ratios R [S][E]
 * (TableModel.from_log_ratios): T[i][j] = R[j] for every child i and parent j,
 * U [S+1][E] as given.  R alone crosses to the device, where the table is
 * made by a broadcast; from there on it is nemo_stage_tables' own path, so
 * everything obtainable afterwards equals, to the bit, what
 * nemo_stage_tables(U, T) with that T gives under the same options -- with no
 * S*S*E host table (65 MB at 64 x 2000, 655 MB at 128 x 5000).  A two-valued R
 * stages the factored kernels; a real-valued one with "exact_generic" is a
 * row-shared table ("exact_shared"). */
int nemo_stage_log_ratios(nemo_ctx* ctx, const double* U, const double* R);

/* ---- A4+A5: batched order-score evaluation --------------------------------
 * Replaces NEMOrderMCMC.compute_cell_ratios + calculate_ll
 * (nem_order_mcmc.py:79-93) and utils.compute_ll (utils.py:84-94).
 *   ll_out    [batch]           sum_e logsumexp_i cell[i][e]
 *   cs_out    [batch][E]        per-effect log-sum-exp (nullable)
 *   cells_out [batch][S+1][E]   cell ratios (nullable)
 *   ow_out    [batch][S+1][E]   order weights exp(cell - cs) (nullable)
 * cap = 0: every predecessor is a permissible parent (the reference);
 * cap > 0: only the `cap` nearest predecessors (build-defined C5 extension). */
int nemo_score(nemo_ctx* ctx, int batch, const int32_t* pos, const double* w01, int cap,
               double* ll_out, double* cs_out, double* cells_out, double* ow_out);
int nemo_score_dev(nemo_ctx* ctx, int batch, const int32_t* d_pos, const double* d_w01, int cap,
                   double* d_ll, double* d_cs, double* d_cells, double* d_ow, void* stream);

/* ---- gradient of the order score in the mapped weights --------------------
 * What NEMOrderMCMC.opt_weights / global_opt_fun (nem_order_mcmc.py:105-150)
 * and the unused Jacobian of methods.py:84-104 were after; no reference
 * counterpart runs, so the arithmetic is the fp64 fast arithmetic whatever
 * "exact" / "exact_dev" / "fact_kernel" say.
 *   ll_out   [batch]        as nemo_score
 *   grad_out [batch][S][S]  d ll / d w01[i][j] = sum_e ow[i][e] (v - 1) /
 *                           (1 - w + w v), v = exp(T[i][j][e]), at the
 *                           permissible pairs; exactly 0.0 elsewhere (every
 *                           entry is written; w01 is read only at those pairs)
 * cap as for nemo_score.  NEMO_F64 contexts only (NEMO_F32: NEMO_ERR_ARG); a
 * wide generic table is served (no products of exp(T) are taken).  A factored
 * model with S <= 64 runs one fused MFMA kernel (the order weights never
 * leave the registers), everything else two passes: the forward with order
 * weights into the context's scratch, then a reduction (option "grad_path").
 * Every sum has a fixed order that depends on the staged model alone: an
 * evaluation's bits depend neither on the batch nor on its slot in it.
 * _dev: enqueue only; after nemo_reserve(max_batch, .) with batch <=
 * max_batch it neither allocates nor synchronises (else NEMO_ERR_STATE). */
int nemo_score_grad(nemo_ctx* ctx, int batch, const int32_t* pos, const double* w01, int cap,
                    double* ll_out, double* grad_out);
int nemo_score_grad_dev(nemo_ctx* ctx, int batch, const int32_t* d_pos, const double* d_w01, int cap,
                        double* d_ll, double* d_grad, void* stream);

/* ---- exact score change of every single-weight move -----------------------
 * What a greedy search over the DAG of a fixed order (the nem R package's
 * nem.greedy), an edge-Gibbs conditional or a finite-difference check of the
 * gradient asks: what does the score become if this ONE weight changes?  With
 * f_ij(e) = 1 - w_ij + w_ij v, v = exp(T[i][j][e]), and ow = exp(cell - cs),
 * replacing w_ij by w'_ij moves only row i of the cells, so in closed form,
 * with no differencing of two scores,
 *   ll(w with w_ij := w'_ij) - ll(w) = sum_e log1p(ow[i][e] kappa_ij(e)),
 *   kappa_ij(e) = (w'_ij - w_ij) (v - 1) / f_ij(e)
 * -- exact to fp64 rounding however small the move's effect; nemo_score_grad
 * is this sum's first-order term.  No reference counterpart runs, so "exact" /
 * "exact_dev" / "fact_kernel" do not route this call.
 *   w_alt    [batch][S][S]  the value each permissible pair would take; read
 *                           only at the permissible pairs, exactly where w01 is
 *   ll_out   [batch]        as nemo_score_grad
 *   dll_out  [batch][S][S]  the sum above at the permissible pairs (each entry
 *                           is the change of that one move alone); exactly
 *                           +0.0 elsewhere (every entry is written), and
 *                           exactly 0.0 where w_alt == w01
 * cap as for nemo_score.  NEMO_F64 contexts only (NEMO_F32: NEMO_ERR_ARG); a
 * wide generic table is served (no products of exp(T) are taken).  A factored
 * model with S <= 64 runs one fused kernel between the factored prep and a
 * finish (nemo_score_grad's MFMA forward, then one log1p per pair and effect
 * from the order weights in the LDS), everything else two passes: the forward
 * with order weights into the context's scratch, then a reduction (option
 * "moves_path").  Every sum has a fixed order that depends on the staged
 * model alone: an evaluation's bits depend neither on the batch, nor on its
 * slot in it, nor on the run.  The host entry wants w_alt finite within [0, 1]
 * at the permissible pairs (else NEMO_ERR_ARG; it does not look elsewhere).
 * _dev: enqueue only; after nemo_reserve(max_batch, .) with batch <=
 * max_batch it neither allocates nor synchronises (else NEMO_ERR_STATE). */
int nemo_score_moves(nemo_ctx* ctx, int batch, const int32_t* pos, const double* w01, const double* w_alt,
                     int cap, double* ll_out, double* dll_out);
int nemo_score_moves_dev(nemo_ctx* ctx, int batch, const int32_t* d_pos, const double* d_w01,
                         const double* d_w_alt, int cap, double* d_ll, double* d_dll, void* stream);

/* ---- exact score change of every single-node relocation of an order --------
 * What order MCMC with node relocation (Kuipers & Moffa) or a greedy search
 * over orders asks: what does the score become if node a moves to position q
 * and everything else keeps its relative order?  The state is (order, W) with a
 * FULL weight matrix: W[i][j] is the weight pair (i, j) carries whenever j
 * precedes i.  Moving a from position p to q > p, the nodes m at positions
 * p+1 .. q lose parent a and a gains them all; to q < p, the nodes m at q ..
 * p-1 gain parent a and a loses them all.  With f_ij(e) = 1 - w_ij + w_ij
 * exp(T[i][j][e]), z = cell - cs and ow = exp(z), in closed form
 *   ll(a moved to q) - ll = sum_e log(1 + X_aq(e)),
 *   q > p: X = -ow[a] + sum_m ow[m] (1 / f_ma - 1) + exp(z_a + sum_m log f_am)
 *   q < p: X = -ow[a] + sum_m ow[m] (f_ma - 1)     + exp(z_a - sum_m log f_am)
 * and both sums grow by one term per step away from p: the S - 1 targets of a
 * node are one walk.  The factors of a are carried as a sum of logs (never a
 * running product) and no exp overflows, so no model is refused for the range
 * of its table.  No reference counterpart runs, so "exact" / "exact_dev" /
 * "fact_kernel" do not route this call.
 *   w01      [batch][S][S]  read at EVERY off-diagonal entry: the current
 *                           weight at the permissible pairs, elsewhere the
 *                           weight the pair takes when a relocation makes it
 *                           permissible; the diagonal is never read
 *   ll_out   [batch]        as nemo_score_grad: nemo_score(pos, w01) of the state
 *   dll_out  [batch][S][S]  dll[a][q] = the score after moving NODE a to
 *                           POSITION q, minus ll; every entry is written and
 *                           dll[a][pos[a]] is exactly +0.0
 * cap must cut nothing: 0 or >= S - 1 (else NEMO_ERR_ARG).  NEMO_F64 contexts
 * only (NEMO_F32: NEMO_ERR_ARG); factored models at every S, generic and
 * row-shared tables, wide ones included.  Two passes for every model: the
 * forward with cells and cs into the context's scratch, then one block per
 * (evaluation, node); no scratch beyond nemo_score's.  Every sum has a fixed
 * order that depends on the staged model alone: an evaluation's bits depend
 * neither on the batch, nor on its slot in it, nor on the run.  The host entry
 * wants the off-diagonal entries of w01 finite within [0, 1] (else
 * NEMO_ERR_ARG).  _dev: enqueue only; after nemo_reserve(max_batch, .) with
 * batch <= max_batch it neither allocates nor synchronises (else
 * NEMO_ERR_STATE). */
int nemo_score_relocations(nemo_ctx* ctx, int batch, const int32_t* pos, const double* w01, int cap,
                           double* ll_out, double* dll_out);
int nemo_score_relocations_dev(nemo_ctx* ctx, int batch, const int32_t* d_pos, const double* d_w01, int cap,
                               double* d_ll, double* d_dll, void* stream);

/* ---- one sweep over the single-weight moves, each taken or not in turn -----
 * nemo_score_moves scores every move at ONE state; once a move is taken every
 * other score is stale.  This call walks the permissible pairs in sequence and
 * keeps the state exact across the moves it takes: a Gibbs sweep over the
 * edges of a fixed order, or one round of coordinate ascent, in one launch.
 * With x_e = ow[i][e] kappa_ij(e) and t_e = log1p(x_e), taking move (i, j) is
 *   cs[e] += t_e,  ow[i][e] *= (1 + kappa_ij(e)) / (1 + x_e),
 *   ow[k][e] /= 1 + x_e  (k != i),
 * so one number per effect, c[e] = the change of cs[e] so far, carries the
 * sweep: child i's row is ow0[i][e] exp(-c[e]) when its turn comes (ow0: the
 * forward's order weights) and the swept weights score ll0 + sum_e c[e].
 *   visit order  children by order position q = 1 .. S-1 ascending, within a
 *                child its permissible parents by order position ascending;
 *                each pair once
 *   gain         sum_e log1p(ow_cur[i][e] kappa_ij(e)) at the current state,
 *                kappa as in nemo_score_moves from w01[i][j] and w_alt[i][j];
 *                exactly +0.0 where w_alt == w01
 *   decision     taken iff gain > thr[i][j], strictly: +inf never, -inf always
 *   thr      [batch][S][S]  read only at the permissible pairs
 *   w_out    [batch][S][S]  w_alt[i][j] where the move was taken, else
 *                           w01[i][j]; alt_out the other one (bits copied, no
 *                           arithmetic): a call on (w_out, alt_out) proposes
 *                           every taken move's reverse.  Off the permissible
 *                           pairs both carry the inputs' bits through.
 *                           w_out == w01 and alt_out == w_alt (in place) are
 *                           allowed, no other overlap
 *   ll0_out  [batch]        the score of w01 (nullable)
 *   ll_out   [batch]        the score of w_out, as ll0 + sum_e c[e]
 *   gain_out [batch][S][S]  each pair's gain at its visit, taken or not; +0.0
 *                           off the permissible pairs (nullable)
 *   nacc_out [batch]        moves taken (nullable)
 * cap as for nemo_score.  NEMO_F64 contexts only (NEMO_F32: NEMO_ERR_ARG);
 * factored models at every S, generic and row-shared tables, wide ones
 * included (no products of exp(T) are taken); E <= NEMO_EDGE_SWEEP_MAX_E
 * (else NEMO_ERR_ARG).  No option routes the call: the two-pass forward
 * (order weights into the context's scratch), then one block per evaluation.
 * Every sum has a fixed order that depends on the staged model alone: an
 * evaluation's bits depend neither on the batch, nor on its slot in it, nor on
 * the run.  The host entry wants w_alt finite within [0, 1] and thr not NaN at
 * the permissible pairs (else NEMO_ERR_ARG; it does not look elsewhere); on
 * the _dev entry a NaN threshold never takes its move.
 * _dev: enqueue only; after nemo_reserve(max_batch, .) with batch <=
 * max_batch it neither allocates nor synchronises (else NEMO_ERR_STATE). */
int nemo_edge_sweep(nemo_ctx* ctx, int batch, const int32_t* pos, const double* w01, const double* w_alt,
                    const double* thr, int cap, double* w_out, double* alt_out, double* ll0_out, double* ll_out,
                    double* gain_out, int32_t* nacc_out);
int nemo_edge_sweep_dev(nemo_ctx* ctx, int batch, const int32_t* d_pos, const double* d_w01,
                        const double* d_w_alt, const double* d_thr, int cap, double* d_w_out, double* d_alt_out,
                        double* d_ll0, double* d_ll, double* d_gain, int32_t* d_nacc, void* stream);

/* ---- relocations walked in sequence: a Gibbs or greedy sweep over orders -----
 * nemo_score_relocations scores every relocation at ONE order; once one is
 * taken every other score is stale.  This call walks a list of node visits per
 * evaluation inside one launch and keeps the state exact.  The state is (order,
 * W) with a full weight matrix as for nemo_score_relocations: w01 is read at
 * every off-diagonal entry and never changes; the diagonal is never read.
 * Visit k of evaluation b, a = visit[b][k] at its current position p:
 *   row       r[q] = ll(a moved to q) - ll at the CURRENT order, by
 *             nemo_score_relocations' closed form (the exponent a sum of logs,
 *             no exp overflows); r[p] is exactly +0.0
 *   Gibbs     (beta finite, > 0) g = beta r, pq[q] = exp(g[q] - max g), cdf the
 *             running sum of pq over q ascending, added sequentially;
 *             q* = min(#{q : cdf[q] < u cdf[S-1]}, S - 1): u = 0 lands on
 *             position 0 and u >= 1 on S - 1
 *   greedy    (beta = +inf) q* the position of the largest r[q], ties to the
 *             lowest q, taken only if r[q*] > min_gain, strictly, else q* = p;
 *             u is not read and may be null
 *   update    for q* != p the order changes; for every effect each passed
 *             node's cell takes -+log f_ma, a's cell +-sum_m log f_am, and cs[e]
 *             is formed afresh as the log-sum-exp of the updated column (rows 0
 *             .. S ascending, the maximum subtracted)
 * A row that holds a NaN leaves q* = p on the device entry.
 *   visit      [batch][nvisit]     node labels in [0, S), any number of times each
 *   u          [batch][nvisit]     one uniform per visit (Gibbs)
 *   pos_out    [batch][S]          the final order; pos_out == pos (in place)
 *                                  is allowed, no other overlap
 *   ll0_out    [batch]             the score of the initial state (nullable)
 *   ll_out     [batch]             the score of the final state, sum_e cs[e]
 *   q_out      [batch][nvisit]     the position each visited node took (nullable)
 *   dll_out    [batch][nvisit][S]  the row r of each visit (nullable)
 *   ll_vis_out [batch][nvisit]     the score held after each visit; a visit that
 *                                  moved nothing carries the previous bits (nullable)
 *   nmoved_out [batch]             moves taken (nullable)
 * cap must cut nothing: 0 or >= S - 1; nvisit >= 0; beta > 0; min_gain >= 0
 * (else NEMO_ERR_ARG).  nvisit = 0 scores the state and copies pos through.
 * NEMO_F64 contexts only (NEMO_F32: NEMO_ERR_ARG); factored models at every S
 * <= 256, generic and row-shared tables, wide ones included.  No option routes
 * the call ("exact" / "exact_dev" / "fact_kernel" included): the two-pass
 * forward with cells and cs into the context's scratch, then one block per
 * evaluation; E is not bounded.  Every sum has a fixed order that depends on S
 * and E alone: an evaluation's bits, and hence its decisions, depend neither on
 * the batch, nor on its slot in it, nor on the run.  The host entry wants pos a
 * permutation, the off-diagonal entries of w01 finite within [0, 1], visit
 * within [0, S) and, in Gibbs mode, u finite and >= 0 (else NEMO_ERR_ARG with
 * the offending index; no refused call writes any output).
 * _dev: enqueue only; after nemo_reserve(max_batch, .) with batch <=
 * max_batch it neither allocates nor synchronises (else NEMO_ERR_STATE). */
int nemo_order_sweep(nemo_ctx* ctx, int batch, const int32_t* pos, const double* w01, int nvisit,
                     const int32_t* visit, const double* u, double beta, double min_gain, int cap,
                     int32_t* pos_out, double* ll0_out, double* ll_out, int32_t* q_out, double* dll_out,
                     double* ll_vis_out, int32_t* nmoved_out);
int nemo_order_sweep_dev(nemo_ctx* ctx, int batch, const int32_t* d_pos, const double* d_w01, int nvisit,
                         const int32_t* d_visit, const double* d_u, double beta, double min_gain, int cap,
                         int32_t* d_pos_out, double* d_ll0, double* d_ll, int32_t* d_q, double* d_dll,
                         double* d_ll_vis, int32_t* d_nmoved, void* stream);

/* ---- the error rates as parameters: score and gradient in per-gene A_k, B_k --
 * The closing comment of nem.py ("shared probability between clusters for the
 * error rates, use that as a latent variable") names what the reference never
 * built; no reference counterpart runs, so "exact" / "exact_dev" /
 * "fact_kernel" do not route this call.  Every evaluation carries its own
 * rates, per S-gene: A_k = log(alpha_k / (1 - beta_k)), B_k = log(beta_k /
 * (1 - alpha_k)), and nothing is restaged.  With D the staged knockdown
 * matrix the tables of nem.py:25-64 generalise to
 *   T[i][j][e] = D[j][e] ? -A_j : B_j                      (j != i),
 *   U[i][e]    = (D[i][e] ? 0 : B_i) + sum_{k != i} D[k][e] A_k,
 *   U[S][e]    = sum_k D[k][e] A_k
 * (scalar rates: the staged tables up to the rounding of their addition
 * chains), and the call evaluates the offset form, n_k = sum_e D[k][e]:
 *   x[i][e] = (D[i][e] ? -A_i : B_i) + sum_{j in pa(i)} log(1 - w + w e^{T[i][j][e]})
 *   ll      = sum_k A_k n_k + sum_e log(1 + sum_i exp(x[i][e])).
 *   rates      [batch][2][S]   row 0: A_k, row 1: B_k of each evaluation
 *   ll_out     [batch]         as nemo_score at those rates
 *   drates_out [batch][2][S]   row 0: d ll / d A_k, row 1: d ll / d B_k; with
 *                              ow = exp(cell - cs), w = w01[i][k] over the
 *                              children i that have k as a permissible parent,
 *       d ll / d A_k = sum_e D[k][e] (1 - ow[k][e] - sum_i h_ik ow[i][e]),
 *       d ll / d B_k = sum_e (1 - D[k][e]) (ow[k][e] + sum_i k_ik ow[i][e]),
 *       h_ik = w e^{-A_k} / (1 - w + w e^{-A_k}),  k_ik = w e^{B_k} / (1 - w + w e^{B_k})
 *   grad_out   [batch][S][S]   d ll / d w01 as nemo_score_grad at these rates
 *                              (nullable; exactly 0.0 off the permissible pairs,
 *                              where w01 is not read)
 * ll is a ratio against a baseline that depends on the rates; a fit maximises
 *   L = ll + sum_k [ n_k log(1 - beta_k) + (E - n_k) log(1 - alpha_k) ]
 * (nemo.rates.absolute_ll).  One fused MFMA launch between a prep and a finish;
 * every sum has a fixed order that depends on E and the evaluation alone: an
 * evaluation's bits depend neither on the batch nor on its slot nor on the run.
 * Serves NEMO_F64 contexts (NEMO_F32: NEMO_ERR_ARG) with S <= 64 (more:
 * NEMO_ERR_ARG -- past 64 the forward runs in two passes and reads the staged
 * U) staged by nemo_stage_knockdown (else NEMO_ERR_STATE: generic and
 * log-ratio tables have no rates), with any cap.  The host entry wants every
 * rate finite with |A_k|, |B_k| <= 700, so that e^{-A} stays finite (else
 * NEMO_ERR_ARG).  _dev: enqueue only; after nemo_reserve(max_batch, .) with
 * batch <= max_batch it neither allocates nor synchronises (else
 * NEMO_ERR_STATE); it cannot validate the rates: non-finite rates give
 * non-finite outputs and nothing worse. */
int nemo_score_rates(nemo_ctx* ctx, int batch, const int32_t* pos, const double* w01, const double* rates,
                     int cap, double* ll_out, double* drates_out, double* grad_out);
int nemo_score_rates_dev(nemo_ctx* ctx, int batch, const int32_t* d_pos, const double* d_w01,
                         const double* d_rates, int cap, double* d_ll, double* d_drates, double* d_grad,
                         void* stream);

/* reuse-batched variant: `group` evaluations share every table row read
 * (group in {1,4,8,16}); same results as nemo_score_dev */
int nemo_score_group_dev(nemo_ctx* ctx, int batch, int group, const int32_t* d_pos, const double* d_w01,
                         int cap, double* d_ll, void* stream);

/* ---- utils.compute_ll / calculate_ll on a given cell matrix ------------- */
int nemo_lse(nemo_ctx* ctx, int rows, const double* cells, double* ll_out, double* cs_out, double* ow_out);

/* ---- A8 core: batch of penalised 1-D local problems -----------------------
 * Replaces scipy.optimize.minimize(local_ll_sum_penalized, x0,
 * bounds=[(-inf, inf)], args=(c, x_anc), method='L-BFGS-B', tol=0.01)
 * (nem_order_mcmc.py:18-23, 167): f(x) = -sum_e log(c_e*expit(x) + 1)
 *   + |expit(x) - x_anc| + expit(x)*(1 - expit(x)), forward-difference
 * gradient with absolute step 1e-8, L-BFGS-B 3.0 logic for n = 1.
 *   c [n][E], anc [n], x0 [n] -> xstar, fstar [n]; nit, nfev, status [n] */
int nemo_local_opt(nemo_ctx* ctx, int n, const double* c, const double* anc, const double* x0,
                   double* xstar, double* fstar, int32_t* nit, int32_t* nfev, int32_t* status);

/* ---- A6 fused per-step scorer (get_optimal_weights(init=True, max_iter=1),
 *      nem_order_mcmc.py:172-208) for a batch of chains --------------------
 * per chain: eval#1 on w01 (order weights kept on device), the local optimum
 * of every permissible (i, k) pair (c built from T[i][k], order weights row k,
 * w01[i][k]; x0 = w01[i][k]; anc[i][k]), then eval#2 on the binarised weights
 * (sigma(x*) > 0.5 ? sig1 : sig0, sig0 = expit(0), sig1 = expit(1)).
 *   anc    [nchains][S][S]  clip(inv(I - expit_parent_weights(W)) - I, 0, 1)
 *   w_new  [nchains][S][S]  expit(x*) at permissible entries (others untouched)
 *   info   [nchains][S][S]  nullable; status | nit << 4 | nfev << 16 per pair,
 *                           -1 at entries that are not a permissible pair
 *   ll1, ll_dag [nchains]
 * Returns NEMO_ERR_OPT (results still written) if any pair ended abnormally.
 * _dev: the same on device pointers, queued on `stream` (null: the context's),
 * without the NEMO_ERR_OPT check (read it from d_info). */
int nemo_optimal_weights(nemo_ctx* ctx, int nchains, const int32_t* pos, const double* w01,
                         const double* anc, double sig0, double sig1, int cap, double* w_new,
                         double* ll1, double* ll_dag, int32_t* info);
int nemo_optimal_weights_dev(nemo_ctx* ctx, int nchains, const int32_t* d_pos, const double* d_w01,
                             const double* d_anc, double sig0, double sig1, int cap, double* d_w_new,
                             double* d_ll1, double* d_ll_dag, int32_t* d_info, void* stream);
/* nemo_optimal_weights as a queued call: _begin checks the context and
 * pointers and returns at once; a library thread runs the queued calls in
 * order (transfers, launches, the NEMO_ERR_OPT check), two in flight at a
 * time: it stages and queues the next call's device work before it waits for
 * the previous one, so the device runs them back to back; _end waits for the
 * oldest call not yet ended and returns its result code (nemo_last_error()
 * then holds its message).  The caller keeps every buffer alive and untouched
 * until the matching _end, and makes no other call on ctx in between except
 * further _begin / _end.  Replaces, like nemo_optimal_weights,
 * get_optimal_weights(init=True) (nem_order_mcmc.py:172-208) for a caller
 * that runs chain groups in a pipeline (nemo/chains.py). */
int nemo_optimal_weights_begin(nemo_ctx* ctx, int nchains, const int32_t* pos, const double* w01,
                               const double* anc, double sig0, double sig1, int cap, double* w_new,
                               double* ll1, double* ll_dag, int32_t* info);
int nemo_optimal_weights_end(nemo_ctx* ctx);
/* nemo_optimal_weights from the weights themselves, as the reference's step
 * starts (nem_order_mcmc.py:172-208 with :98-103 and :185): the device makes
 * each chain's W~ = expit(W) on the permissible entries (cap as below; the
 * other entries W's own) and ancestor_x = clip(inv(I - W~) - I, 0, 1) in
 * scipy.linalg.inv's bits (LAPACK getrf + getri of scipy's OpenBLAS 0.3.28,
 * restated in csrc/nemo_ancestor.hip), then runs the step on them.  S <= 64.
 *   w        [nchains][S][S]  the weights W (after the proposal's reset)
 *   w01_out, anc_out [nchains][S][S]  nullable: W~ and ancestor_x (both null:
 *                             neither leaves the device)
 *   anc_flag [nchains]        nullable: 0, or 1 singular / 2 not finite /
 *                             4 non-finite factors (recompute on the host)
 * Returns NEMO_ERR_LINALG when a flag is set (the step's results are then
 * not meaningful: scipy.linalg.inv raises LinAlgError / ValueError for 1 / 2),
 * else as nemo_optimal_weights.  _begin: the queued form (ended by
 * nemo_optimal_weights_end, in submission order with the other _begin). */
int nemo_optimal_weights_w(nemo_ctx* ctx, int nchains, const int32_t* pos, const double* w, double sig0,
                           double sig1, int cap, double* w01_out, double* anc_out, double* w_new,
                           double* ll1, double* ll_dag, int32_t* info, int32_t* anc_flag);
int nemo_optimal_weights_w_begin(nemo_ctx* ctx, int nchains, const int32_t* pos, const double* w,
                                 double sig0, double sig1, int cap, double* w01_out, double* anc_out,
                                 double* w_new, double* ll1, double* ll_dag, int32_t* info,
                                 int32_t* anc_flag);
/* the same W~ / ancestor_x / flags on device buffers, queued on `stream`
 * (null: HIP's null stream); feeds nemo_optimal_weights_dev.  S <= 64. */
int nemo_ancestor_dev(nemo_ctx* ctx, int nchains, const int32_t* d_pos, const double* d_w, int cap,
                      double* d_w01, double* d_anc, int32_t* d_flag, void* stream);
/* order weights of chain `chain` from the last eval#1 of nemo_optimal_weights:
 * (S+1)*E doubles (NEMOrderMCMC.order_weights after get_optimal_weights) */
int nemo_fetch_order_weights(nemo_ctx* ctx, int chain, double* ow_out);
/* diagnostic (option "exact_trace" 1): the last exact fused step's local
 * optima, [*n][4]: start / end times (wall_clock64, 100 MHz ticks) and the
 * shader cycles spent in the objective / the optimiser's control, in launch
 * order (chain-major, each chain's pair list); out may be NULL to query *n.
 * No reference counterpart: profiling of the scheduling only. */
int nemo_fetch_exact_trace(nemo_ctx* ctx, int* n, long long* out);

/* ---- fixed-order optimizers of methods.py ---------
 * Every call handles nprob independent problems (one order each) with host
 * buffers; w / w_out are [nprob][S][S] (w_out = w with every permissible pair
 * replaced by its optimum), ll_out [nprob] is the sweep's evaluation, info
 * (nullable) as for nemo_optimal_weights.  NEMO_ERR_OPT (results written)
 * when a local optimisation fails, where the reference raises
 * (methods.py:115, :394).
 *
 * Method.opt_gamma (methods.py:397-405): evaluation on the raw weights in
 * [0, 1], then per pair minimize(local_ll_sum_gamma (:8-9), x0 = w[i][k],
 * bounds [(0, 1)], jac=True, tol=0.01) with c from exp(T[i][k]) and order
 * weights row k (:385-395).  cap as for nemo_score (0 = the reference). */
int nemo_gamma_sweep(nemo_ctx* ctx, int nprob, const int32_t* pos, const double* w, int cap,
                     double* w_out, double* ll_out, int32_t* info);
/* InverseMethod (methods.py:21-172): w holds log-weights (-5000 off the
 * parents).  out = unorder_arr(order, B / (1 + B)) with B =
 * solve_triangular(I - order_arr(order, exp(w)), I, lower=True)
 * (:118-121, :160-164). */
int nemo_inverse_ancestral(nemo_ctx* ctx, int nprob, const int32_t* pos, const double* w, double* out);
/* InverseMethod.opt_b (:117-129): evaluation on B/(1+B), then every pair
 * in the reference's loop order minimises local_ll_sum_b_inv (:73-82),
 * bounds [(-5000, 500)], eps 1e-3, tol 0.1, each pair seeing the optima of
 * the pairs before it (levels of independent pairs on the device). */
int nemo_inverse_sweep(nemo_ctx* ctx, int nprob, const int32_t* pos, const double* w, double* w_out,
                       double* ll_out, int32_t* info);

/* ---- NEM.compute_real_score's sweep (nem.py:112-125) ------------------------
 * One pass of the reference's fit of the true graph, for nprob problems (one
 * order each): the evaluation on the weights w (ll_out, order weights kept on
 * the device), then for every permissible pair (i, j)
 *   minimize(-sum log(c x + 1), x0 = 0.5, bounds [(0, 1)], L-BFGS-B, tol 0.1)
 * with c = a / b, a = (exp(T[i][j]) - 1) * order_weights -- the whole
 * (S+1, E) matrix, T's row broadcast over its rows (nem.py:117) -- and
 * b = 1 - w[i][j] a + w[i][j] (exp(T[i][j]) - 1); no jac (forward differences,
 * step 1e-8, flipped at the bound), x0 always 0.5.  w, w_out, ll_out, info as
 * for nemo_gamma_sweep (no cap).  A solve that ends abnormally is no error
 * (the reference keeps res.x without reading res.success): the call returns
 * NEMO_OK and the status is in info.  One block per pair streams the order
 * weights, so E is bounded only by what the context stages; every sum has a
 * fixed order: a pair's bits depend neither on nprob nor on its slot.
 * NEMO_F64 contexts, factored or generic (NEMO_F32: NEMO_ERR_ARG); a wide
 * table (|T| > 170, option "exact_generic") is refused like the other sweeps. */
int nemo_real_sweep(nemo_ctx* ctx, int nprob, const int32_t* pos, const double* w, double* w_out,
                    double* ll_out, int32_t* info);

/* ---- options -------------------------------------------------------------
 *   "xcd_remap"  1 (default) XCD-aware block order; speed only
 *   "score_path" 0 (default) auto: the factored MFMA kernel when the staged
 *                table has the NEM structure (every off-diagonal row T[.][j]
 *                shared by all children and two-valued), else the streaming
 *                kernel; 1 = always stream; 2 = always factored
 *   "fact_kernel" 0 (default) auto: ll-only calls with S <= 64 take the
 *                int8 fixed-point factored kernel, the rest the chunked fp64
 *                one; 1 = chunked; 2 / 3 = fp64 pipelined with 4 / 8 waves
 *                per block; 4 / 5 = int8 with 4 / 5 digit pairs; 6 = int8
 *                with 8 waves per block; 7 / 8 = int8 with the offset
 *                log-sum-exp (4 / 8 waves), which auto prefers when the
 *                staged model passes its range checks (option "i8o");
 *                9 = the banded lookup-table kernel for capped calls
 *                (1 <= cap <= 6), which auto prefers for ll-only capped
 *                calls when the model passes its checks (option "win");
 *                10 / 11 = the offset kernel in log2 fixed point (8 / 4
 *                waves), which auto prefers over 7 / 8 when staged
 *                (option "i8l"; 10 walks two 16-effect tiles per
 *                iteration); 12 = the same with 16 waves per block,
 *                13 = its register-stationary variant, 14 = 8 waves with
 *                one tile per iteration compiled for 6 waves per SIMD,
 *                16 = 8 waves with one tile per iteration (11, 12, 14 and
 *                16 give one another's bits, within 1e-11 of 10's);
 *                15 = the round-1 form of 9 (row bits re-read from LDS);
 *                17 = 10's walk in persistent blocks that prep the next
 *                evaluation's digits during the walk (10's bits);
 *                18 = the log2 kernel for 64 < S <= 128 (two K = 64 halves,
 *                two tiles per iteration), which auto takes for uncapped
 *                ll-only calls there within the error budget; 19 = the same
 *                with one tile per iteration; 20 = 10 as two launches, a
 *                prep-only one writing each evaluation's digits to HBM and a
 *                walk-only one reading them (10's bits; an experiment,
 *                measured slower)
 *   "grad_path"  0 (default) auto: nemo_score_grad runs the fused kernel for a
 *                factored model with S <= 64, else the two-pass path; 1 = the
 *                two-pass path always (tests, A/B measurement)
 *   "grad_path_used" (get only) the path the last nemo_score_grad(_dev) ran:
 *                1 two-pass, 2 fused; 0 before any call
 *   "moves_path" 0 (default) auto: nemo_score_moves runs the fused kernel for a
 *                factored model with S <= 64, else the two-pass path; 1 = the
 *                two-pass path always (tests, A/B measurement)
 *   "moves_path_used" (get only) the path the last nemo_score_moves(_dev) ran:
 *                1 two-pass, 2 fused; 0 before any call
 *   "reloc_path" 0 (default) auto, 1 = the two-pass path always.  Auto takes
 *                the two-pass path for every model: a fused kernel measured no
 *                faster, so both values run the same code
 *   "reloc_path_used" (get only) the path the last nemo_score_relocations(_dev)
 *                ran: 1 two-pass; 0 before any call
 *   "factored"   (get only) 1 if the staged table is factorable
 *   "win"        (get only) 1 if the capped lookup-table kernel is staged
 *                (U - U[S] two-valued per row, partial sums in range)
 *   "i8o"        (get only) 0: no offset int8 kernel for this model; 1: it
 *                reads U - U[S] per cell; 2: U - U[S] is two-valued per row
 *                and rides in the contraction (no U reads)
 *   "i8o_nodiag" 1 = keep the U reads even when 2 is available (testing)
 *   "i8l"        (get only) 1 if the log2 fixed-point offset kernel is staged
 *                (i8o = 2 and |Delta|, |U - U[S]| / ln 2 within its digit range)
 *   "i8w"        (get only) 1 if the same is staged for 64 < S <= 128 (18 / 19)
 *   "graphs"     1 (default): nemo_optimal_weights replays its device work
 *                as a hipGraph per (nchains, cap); 0 = direct launches
 *   "step_host_sum" 1 (default): nemo_optimal_weights (and _begin / _end)
 *                copy eval #2's per-evaluation partials out with the other
 *                outputs and sum them on the host in the device's fixed
 *                order (same bits, one launch fewer); 0 = the device sums
 *                them (as nemo_optimal_weights_dev always does)
 *   "local_split" 2 = run each local optimum of a fused step on a 4-wave
 *                block (the objective's products split over the waves; same
 *                bits; measured slower for one chain, so 0 = auto never
 *                takes it), 1 = never, 3 = the same on a 2-wave block
 *   "exact"      1 (default): nemo_optimal_weights, nemo_local_opt and the
 *                ll-only host-pointer nemo_score (any batch; with
 *                "fact_kernel" 0 -- an explicitly chosen kernel runs as
 *                chosen -- and no effective cap) compute in the
 *                reference's own arithmetic -- numpy's SVML log / exp, glibc's
 *                exp / log1p, numpy's pairwise sum and scipy's compact-form
 *                L-BFGS-B with OpenBLAS's small kernels, restated bit for bit
 *                (csrc/refmath.h, csrc/lbfgsb_exact.h, csrc/nemo_exact.hip):
 *                the same order scores, order weights, local optima and
 *                weights as nem_order_mcmc.py, to the bit, when "exact_ok";
 *                0 = the fast kernels (scores within ~1e-9).
 *                One exception, in the order weights only: np.exp is restated
 *                on its fast path, |x| < 707.70 (0x1.61da04cbafe44p+9), so an
 *                order weight exp(cell - cs) of a cell more than 707.70 below
 *                its column's log-sum is exactly 0.0 where numpy's rare path
 *                gives 5e-324 .. 4.6e-308 (ll, cs and the cells are not
 *                affected).  The local optima keep the reference's bits all
 *                the same: such a weight enters c = a / b with |c| <=
 *                e^(|T| - 707.70), and 1 + c ex = 1 with it or with 0 -- for
 *                factored tables always (|T| <= 170), for generic ones by the
 *                bound on |T| below (tests/test_exact_edges_cpu.py)
 *   "exact_dev"  0 (default): nemo_score_dev runs the fast kernels; 1 = the
 *                same conditions as "exact" on nemo_score, on device buffers
 *                (cells built in d_ow -- then order weights in place -- or in
 *                d_cells, not both)
 *   "exact_ok"   (get only) 1 if the staging supports "exact": factored
 *                tables, any parent cap, E <= 524288 (numpy's np.sum adds
 *                buffers of 8192 terms in order, each summed pairwise, and
 *                the local optima run one wave plan per buffer -- of at most
 *                64 leaf blocks: 441 buffer sizes in 7689 .. 8191, 8191 among
 *                them, split into 65 and have no plan, "exact_ok" 0 for such
 *                an E or last buffer; nemo.limits); or, with
 *                "exact_generic", a generic table within that option's bounds
 *   "exact_generic" 0 (default); 1 = nemo_stage_tables also stages a table
 *                that is not factorable (real-valued rows, e.g. per-effect
 *                log-likelihood ratios) for the exact kernels: np.exp(T) in
 *                numpy's bits in its own fp64 buffer and the wave plan of E.
 *                Covered ("exact_ok" 1) when max|T| (off-diagonal rows) <=
 *                670 (NEMO_EXACT_GENERIC_MAX_ABS_T: a flushed order weight
 *                cannot change a local optimum), max|U| <= 700 and
 *                  - a table with its own rows per child: E <= 8192 (one numpy
 *                    buffer); X is [S][S][E] and the local optima read stored
 *                    c rows ("exact_form" 1 or 2 -- a form that needs the
 *                    recomputed rows runs as 2; chains x pairs x plan doubles
 *                    of device memory);
 *                  - a row-shared table (T[i][j] bit-identical for every child
 *                    i != j; what nemo_stage_log_ratios stages): E <= 524288 as
 *                    for factored tables; X is [S][E], and the local optima
 *                    follow "exact_cform" like the factored model -- per
 *                    (chain, parent) recompute rows, chains x S x plan doubles,
 *                    with lv - 1 a real number per element in place of the two
 *                    values a bit selects ("exact_form" 1, 2, 4 and 7; 3 and 5
 *                    run as 2).
 *                Then everything "exact" / "exact_dev" route runs the generic
 *                exact kernels (any parent cap).
 *                Outside the bounds "exact_ok" stays 0 and the fast kernels
 *                run.  With the option set an fp64 generic table may hold |T|
 *                up to 705 instead of 170 (the exact kernels take no
 *                products).  Past 170 the score calls still run on the fast
 *                path (the streaming kernel renormalises every factor); the
 *                other fast kernels that read exp(T) -- the fused step with
 *                "exact" 0 or outside the bounds, nemo_score_group_dev (group
 *                > 1), nemo_gamma_sweep, nemo_inverse_sweep -- return
 *                NEMO_ERR_ARG on such a table.  A factorable
 *                table takes the factored kernels whatever the option says.
 *                Set between nemo_ctx_create and staging: on a staged context
 *                NEMO_ERR_STATE
 *   "exact_form" the exact local-optimum kernel's form (same bits): 0 auto
 *                (default: the latency form while chains x pairs <=
 *                "exact_lat_waves", 20000 by default ~ 10 C3 chains, the slot
 *                form beyond; the pair form while chains x pairs <=
 *                "exact_pair_waves", 0 by default), 1 latency (one wave per
 *                optimum, two per SIMD, the optimum's c values held in
 *                registers), 2 throughput (four per SIMD, c recomputed each
 *                evaluation), 3 pair (two waves per optimum, the objective's
 *                slots split between them; E > 1024), 4 cached throughput
 *                (three per SIMD, the cache partly in scratch), 5 dual (two
 *                optima per wave, one per half; measured slower, DESIGN.md
 *                3.5e), 7 slot (four per SIMD, c made once per optimum into
 *                the resident wave's own row set in device memory, read at
 *                each evaluation; needs "exact_cform" 1 and "exact_persist",
 *                else the throughput form); E > 8192 always runs the
 *                throughput form.  A row-shared real-valued table
 *                ("exact_shared") with recompute rows has forms 1, 2, 4 and 7;
 *                the pair and dual forms run as 2 there, and auto changes to
 *                the slot form at a quarter of "exact_lat_waves" (measured
 *                ahead from 4 chains at 64 x 2000)
 *   "exact_shared" (get only) 1 if the staged generic table is row-shared
 *   "exact_rc"   (get only) 1 if the exact local optima recompute c from the
 *                per-parent a rows, 0 if they read stored c rows
 *   "exact_form_used" (get only) the form the last exact local-optimum launch
 *                ran after every fall-back (1 latency, 2 throughput, 3 pair, 4
 *                cached throughput, 5 dual, 6 the throughput form over several
 *                plan parts, 7 slot); 0 before any launch
 *   "timing_kernel" 0 (default): nemo_timing_enable / _read time the score
 *                kernels; 1: the exact local optima's kernel (bench.py);
 *                2: nemo_real_sweep's pair solves (tools/real_score_time.py);
 *                3: nemo_score_moves' kernels (tools/moves_bench.py);
 *                4: nemo_score_relocations' kernels (tools/reloc_bench.py);
 *                5: nemo_order_sweep's kernel (tools/order_sweep_bench.py)
 *   "anc_overlap" 1 (default): nemo_optimal_weights_w makes ancestor_x on a
 *                second stream beside eval #1 (same bits); 0 = in line */
int nemo_set_option(nemo_ctx* ctx, const char* name, int value);
int nemo_get_option(nemo_ctx* ctx, const char* name, int* value);

/* ---- the fixed-point kernels' error budget ---------------------------------
 * The int8 kernels round every entry of their contraction once (Delta of each
 * permissible parent, the diagonal U entry, the row constant G); the roundings
 * repeat over the effects, so their worst-case ll error grows with E:
 *   |d ll| <= eps * sum_e (min(colbits_e, k) + 1) + E * series
 * (colbits_e = staged rows whose D1 bit is set at effect e, k = S or cap + 1;
 * eps = 2^-39 ln 2 for the log2 kernels 10-14, 16, 17, 2^(c - 49) for 4-8;
 * DESIGN.md 3.5a).  Auto (fact_kernel 0) takes an int8 kernel only while that
 * bound stays within "err_budget", else the next more precise one, down to
 * the fp64 MFMA kernels.
 *   f64 options: "err_budget" (get / set; default 1e-7, the north star's
 *                1e-6 ll tolerance with a 10x margin);
 *                "i8l_bound", "i8o_bound" (get only): the bound of the log2 /
 *                natural-units kernels for an uncapped call on the staged model */
int nemo_set_option_f64(nemo_ctx* ctx, const char* name, double value);

/* Test hook: refmath.h's restatements evaluated on the current device, for
 * the tests that compare them with numpy / scipy bit for bit.  fn: 0 np.log
 * (SVML), 1 np.exp (SVML), 2 scipy.special.expit, 3 np.logaddexp(x, y),
 * 4 glibc exp, 5 glibc log1p, 6 sqrt, 7 x / y (the optimiser's IEEE operations),
 * 8 glibc log1p on [0, 1] as logaddexp evaluates it.
 * Host arrays of n doubles (y only for fn 3 and 7). */
int nemo_refmath_probe(int fn, int n, const double* x, const double* y, double* out);
int nemo_get_option_f64(nemo_ctx* ctx, const char* name, double* value);
/* which fact_kernel a factored score call with this cap takes (ll_only: no
 * cs / cells / order-weight outputs), with the worst-case |ll error| bound of
 * its fixed-point arithmetic (0 for the fp64 kernels); *fact_kernel = -1 when
 * the call takes the streaming kernel or the requested kernel cannot serve it */
int nemo_score_kernel(nemo_ctx* ctx, int cap, int ll_only, int* fact_kernel, double* bound);

/* ---- timing of the dominant (score) kernel, for bench.py ---------------- */
int nemo_timing_enable(nemo_ctx* ctx, int enable);
/* total milliseconds and number of score-kernel launches since enable/reset */
int nemo_timing_read(nemo_ctx* ctx, double* total_ms, int* launches);

#ifdef __cplusplus
}
#endif

#endif /* NEMO_H */
