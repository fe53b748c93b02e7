/*
 * mpo.h -- C ABI of libmpo.so, the MI355X (gfx950) engine for mpi_opt's
 * trial-evaluation hot path.
 *
 * Conventions:
 *   - every function returns int status (MPO_OK = 0); the message of the last
 *     failure on the calling thread is mpo_last_error();
 *   - no exceptions cross the ABI;
 *   - the CALLER owns every device buffer (e.g. torch tensors' data_ptr());
 *     the library never allocates device memory: scratch comes from a caller
 *     workspace whose size is returned by the matching *_ws_bytes query;
 *   - every launching call takes an explicit hipStream_t (passed as void*) and
 *     only enqueues work: no host synchronisation, no allocation, so callers
 *     may capture any sequence of calls into a hipGraph;
 *   - not re-entrant per stream; thread-safe across streams/devices.  The
 *     population engines (mpo_pop_*, mpo_dn_*) fork part of a step onto side
 *     streams pooled per (device, caller stream): engines stepped from distinct
 *     caller streams never wait for each other's work.
 *
 * Row-major layouts throughout: matrix A(i,j) lives at A[i*ld + j].
 *
 * Each entry point cites the reference interface it replaces
 * (/root/reference/<file>:<line>).
 */
#ifndef MPO_H_
#define MPO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPO_OK 0
#define MPO_EINVAL 1      /* bad argument (shape, null pointer, workspace too small) */
#define MPO_EHIP 2        /* HIP runtime error (launch failure, ...) */
#define MPO_ENOTSUP 3     /* shape outside what the kernels support */

/* Acquisition selection flags for mpo_gp_acq_score (skopt acquisition.py). */
#define MPO_ACQ_EI 1u     /* value = -EI  (skopt minimises -EI)  */
#define MPO_ACQ_PI 2u     /* value = -PI                         */
#define MPO_ACQ_LCB 4u    /* value = mu - kappa * sd             */

#define MPO_TOPK_MAX 8

const char* mpo_last_error(void);
/* Library version string, e.g. "mpo 0.1 gfx950". */
const char* mpo_version(void);

/* ------------------------------------------------------------------------
 * GP surrogate ("ask" hot path).
 * Replaces skopt.Optimizer.tell/ask's GaussianProcessRegressor fit tail and
 * _gaussian_acquisition, reached from Coordinator.fit (coordinator.py:63-79)
 * and Coordinator.ask (coordinator.py:46-50).
 * ---------------------------------------------------------------------- */

/* A prepared GP posterior (device pointers into the prepare workspace). */
typedef struct MpoGpModel {
    int32_t n;             /* observations                          */
    int32_t d;             /* dimensions                            */
    int32_t dp;            /* padded dimensions (4, 8, 16 or 32)    */
    int32_t np16;          /* n rounded up to 16                    */
    double amp;            /* ConstantKernel value                  */
    double y_mean;         /* normalize_y mean                      */
    double y_std;          /* normalize_y std                       */
    const double* xs;      /* [n][dp]  observations / length_scale  */
    const double* ls;      /* [dp]     length scales (pad = 1)      */
    const double* alpha;   /* [n]      K^-1 y_norm                  */
    const double* wfrag;   /* packed L^-1 MFMA B-fragments          */
    const double* L;       /* [n][n]   lower Cholesky factor        */
    const double* W;       /* [n][n]   L^-1 (lower)                 */
    int32_t* info;         /* device int: 0 ok, j+1 = chol failed at column j */
    const int32_t* wmeta;  /* per-wave B-stream plan of wfrag (scoring kernel) */
    const double* xb;      /* [np16+32][dp] (-2 xs, 1, |xs|^2, 0..) + a guard flag, or NULL:
                              the MFMA form of the candidate-observation distance,
                              set by mpo_gp_prepare when d + 2 <= dp; the flag is
                              the self-check's verdict (see mpo_gp_prepare) */
} MpoGpModel;

/* K(i,j) = amp * Matern52(|X_i/ls - X_j/ls|) + (i==j ? diag_add : 0).
 * X: [n][d] device, ls: [d] device, K: [n][ldk] device. */
int mpo_gp_kernel_matrix(const double* X, int n, int d, const double* ls, double amp,
                         double diag_add, double* K, int ldk, void* stream);

/* In-place lower Cholesky A = L L^T (upper triangle left untouched).
 * info (device int) = 0 on success, j+1 if the pivot of column j is <= 0. */
int mpo_chol_f64(double* A, int n, int lda, int32_t* info, void* stream);

/* Triangular solve with the lower factor L: trans=0 solves L X = B,
 * trans=1 solves L^T X = B; B [n][ldb] (nrhs columns) is overwritten with X. */
int mpo_trsm_f64(const double* L, int n, int lda, double* B, int nrhs, int ldb,
                 int trans, void* stream);

/* Workspace bytes for mpo_gp_prepare; 0 for n > 2048, d > 32 or bad arguments. */
size_t mpo_gp_prepare_ws_bytes(int n, int d);

/* Build a GP posterior from observations and fitted hyper-parameters:
 *   xs = X/ls;  K = amp*Matern52 + (noise + 1e-10 jitter) I;  L = chol(K);
 *   W = L^-1;  alpha = L^-T L^-1 y_norm;  pack W for the scoring kernel.
 * When d + 2 <= dp, model->xb is set and the scoring kernel may form
 * |c - x|^2 = |c|^2 + |x|^2 - 2 c.x on fp64 MFMA (absolute rounding error of a few
 * eps (|c|^2 + |x|^2) instead of the direct form's eps |c - x|^2).  The guard is
 * empirical, not a closed-form bound: (1) a device flag requires every |x/ls|^2 <= 2;
 * (2) a prepare-time self-check scores the model's own observations both ways --
 * r^2 = 0 on each one's own row and the smallest sd, the expansion's worst case --
 * and clears the flag unless (mu_n, q) agree within 1e-10 (q relative to
 * sd^2 = amp - q, mu_n relative to amp sum |alpha|); (3) per 16-candidate tile, the
 * expanded form is used only when every |c/ls|^2 <= 2.  Any other tile or model
 * takes the direct differences.  tests/test_gp_gpu.py checks the expanded path
 * against the exact posterior at 1e-9 on the fixtures and on a small-noise,
 * near-duplicate-observation problem.  MPO_GP_DIST=0 disables it.
 * Two scoring paths serve a prepared model (mpo_gp_score_path): "resident" while the
 * K* tile of 16 candidates x np16 observations fits the 160 KiB LDS (np16 <= 1248 at
 * dp = 4, 1232 at dp = 8 / 12, 1216 at dp = 32), "streamed" past it, up to n = 2048;
 * n > 2048 returns MPO_ENOTSUP.  A streamed model always takes the direct distance
 * (xb = NULL, no self-check).  MPO_GP_SCORE=streamed forces the streamed path at any n
 * (resident or unset: the automatic choice); MPO_GP_PANEL=<rows> (a multiple of 16,
 * >= 16, else MPO_EINVAL) sets its panel height.  Both are read here and at score time.
 * X [n][d], y_norm [n], ls [d]: device.  `model` (host struct) receives
 * device pointers into `ws`, which must stay alive while the model is used.
 * Replaces GaussianProcessRegressor.fit's tail (sklearn _gpr.py:345-365) and
 * skopt's post-fit K_inv_ (skopt learning/gaussian_process/gpr.py). */
int mpo_gp_prepare(const double* X, const double* y_norm, int n, int d, const double* ls,
                   double amp, double noise, double y_mean, double y_std,
                   MpoGpModel* model, void* ws, size_t ws_bytes, void* stream);

/* Extend a prepared posterior by one observation at the SAME hyper-parameters: the
 * model of n + 1 points from the model of n in O(n^2), no factorisation.  With
 * k* = amp*Matern52(|xs_i - xs_new|), l = W k* and delta^2 = amp + noise + 1e-10 - |l|^2:
 *   L' = [L 0; l^T delta]    W' = [W 0; -(1/delta) l^T W  1/delta]    alpha' = W'^T W' y_norm
 * then the same packing, scoring-path choice and xb self-check as mpo_gp_prepare, into
 * the same workspace layout (`ws` sized by mpo_gp_prepare_ws_bytes(n + 1, d)), so an
 * appended model scores, exports and appends again like a prepared one.  Every sum
 * runs in a fixed order (the rule of mpo_gp_prepare's blocked factorisation).
 *   base    a prepared model of n observations (mpo_gp_prepare or an earlier append);
 *           its workspace is only read and must stay alive until this call's work on
 *           `stream` is done.  amp, d and dp are taken from it.
 *   X       [n+1][d] device: the base's n observations, then the new point
 *   y_norm  [n+1] device: the targets re-normalised over all n + 1 values (y_mean, y_std)
 *   ls, noise  the length scales [d] (device) and noise the base was built with
 * *info of the new model: the base's when that is non-zero, else n + 1 when delta^2 is
 * not positive and finite (the value mpo_chol_f64 reports for that column).
 * n + 1 > 2048 returns MPO_ENOTSUP; a null pointer, a malformed base, a workspace that
 * is too small or is the base's own returns MPO_EINVAL.  Only enqueues work: no
 * allocation, no host synchronisation, capturable in a graph.
 * NOT the reference's semantics: skopt's constant-liar ask (Coordinator.ask,
 * coordinator.py:46-50 -> Optimizer.ask(n_points)) refits the hyper-parameters for
 * every lie; this entry point serves the opt-in fixed-theta batch
 * (Optimizer(lie_refit="never")). */
int mpo_gp_append(const MpoGpModel* base, const double* X, const double* y_norm,
                  const double* ls, double noise, double y_mean, double y_std,
                  MpoGpModel* model, void* ws, size_t ws_bytes, void* stream);

/* Workspace bytes for mpo_gp_lml_grad (n <= 2048, d <= 32, batch thetas); 0 if unsupported. */
size_t mpo_gp_lml_ws_bytes(int n, int d, int batch);

/* Log-marginal likelihood and its gradient for `batch` hyper-parameter vectors at
 * once (one workgroup each): sklearn GaussianProcessRegressor(normalize_y=True,
 * alpha=1e-10).log_marginal_likelihood(theta, eval_gradient=True) for skopt's
 * kernel C * Matern(ls, nu=2.5) + WhiteKernel (sklearn _gpr.py:537-655), the
 * objective of the L-BFGS-B refit that skopt.Optimizer.tell runs from
 * Coordinator.fit (coordinator.py:63-79).
 *   X [n][d], y_norm [n] (normalised targets)      device
 *   theta [batch][d+2] = log[amp, ls_0..ls_{d-1}, noise]  (sklearn kernel.theta)
 *   lml [batch], grad [batch][d+2], info [batch]    device outputs
 * info[b] = j+1 when the Cholesky fails at column j: lml = -inf, grad = 0 (as
 * sklearn's LinAlgError branch); 0 otherwise. */
int mpo_gp_lml_grad(const double* X, const double* y_norm, int n, int d,
                    const double* theta, int batch, double* lml, double* grad,
                    int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* Bytes of the device buffer mpo_gp_lml_grad_host stages through (d dims, batch thetas). */
size_t mpo_gp_lml_io_bytes(int d, int batch);

/* mpo_gp_lml_grad for one L-BFGS-B round of the refit with host-side input and
 * output: theta_host [batch][d+2] is copied into dev_io, the objective runs, and
 * out_host receives lml [batch] | grad [batch][d+2] | info (int32 [batch]) --
 * one call and one stream synchronisation per round instead of separate copies
 * (the refit runs ~100-200 rounds per fit, sklearn _gpr.py:296-337).  Pinned host
 * buffers avoid a staging copy.  Synchronises `stream`. */
int mpo_gp_lml_grad_host(const double* X, const double* y_norm, int n, int d,
                         const double* theta_host, int batch, double* out_host,
                         void* dev_io, size_t io_bytes, void* ws, size_t ws_bytes, void* stream);

/* Workspace bytes for mpo_gp_acq_score over m candidates; 0 for a model with
 * n > 2048, k > MPO_TOPK_MAX or bad arguments.  A streamed model adds its
 * workgroups' partial rows (at most 48 MiB; 26 MiB at n = 2048 with the default panel). */
size_t mpo_gp_score_ws_bytes(const MpoGpModel* model, int64_t m, int k);

/* Which scoring kernel mpo_gp_acq_score / mpo_gp_ei_score run for this model under
 * the current MPO_GP_SCORE / MPO_GP_PANEL: 0 resident, 1 streamed, negative
 * (-MPO_ENOTSUP: n > 2048; -MPO_EINVAL: malformed model or panel value) when the
 * model cannot be scored.  Host arithmetic only: reads n, dp and np16. */
int mpo_gp_score_path(const MpoGpModel* model);

/* Score m candidates (transformed space, [m][d] device) under the posterior:
 *   mu, sd           : posterior mean / std (skopt predict(return_std=True));
 *   vals[a*m + i]    : minimised acquisition value for each flag a in
 *                      {EI, PI, LCB} order (rows for unset flags untouched);
 *   topk_idx/val[a*k + r] : the k smallest values of acquisition a, ties to the
 *                      lowest index (np.argsort(values)[:k] / np.argmin).
 * Any of mu, sd, vals may be NULL (not written).  topk arrays are device.
 * Resident path: K* of a 16-candidate tile stays in the LDS for the whole triangular
 * product.  Streamed path (models past the LDS limit, n <= 2048): K* is built one
 * panel of observations at a time; the later panels' partial rows of L^-1 K*^T wait
 * in the workspace.  Same posterior, same top-k and tie rules, same NULL-output
 * rules; no allocation, no host synchronisation, capturable in a graph.
 * Replaces skopt _gaussian_acquisition + gaussian_ei/pi/lcb over the
 * n_points candidate sample, and the argsort/argmin that picks L-BFGS starts. */
int mpo_gp_acq_score(const MpoGpModel* model, const double* cand, int64_t m,
                     double y_opt, double xi, double kappa, unsigned flags,
                     double* mu, double* sd, double* vals, int k,
                     int64_t* topk_idx, double* topk_val,
                     void* ws, size_t ws_bytes, void* stream);

/* EI-only convenience (SURVEY §8b signature family): writes mu, sd, ei (= +EI)
 * and argmax (device int64, lowest index among maximal EI). */
int mpo_gp_ei_score(const MpoGpModel* model, const double* cand, int64_t m,
                    double y_opt, double xi, double* mu, double* sd, double* ei,
                    int64_t* argmax, void* ws, size_t ws_bytes, void* stream);

/* Acquisition value and gradient at `batch` points x [batch][d] (transformed
 * space, device): f[b] = the minimised value of acquisition acq[b] (device int32,
 * one of MPO_ACQ_EI / MPO_ACQ_PI / MPO_ACQ_LCB), g[b][d] its gradient.  The
 * objective of skopt's L-BFGS-B polish of the best candidates (skopt
 * gaussian_acquisition_1D with predict(return_mean_grad, return_std_grad)),
 * reached from Coordinator.ask (coordinator.py:46-50); one point per live
 * polish, all of an ask step's polishes in lockstep. */
int mpo_gp_acq_grad(const MpoGpModel* model, const double* x, int batch, const int32_t* acq,
                    double y_opt, double xi, double kappa, double* f, double* g, void* stream);

/* Which form of the polish kernel mpo_gp_acq_grad launches for this model: 16 waves per
 * point while 19 n doubles plus the kernel's static LDS fit the 160 KiB LDS (n <= 914),
 * 4 waves per point (7 n doubles) past it; negative (-MPO_EINVAL: null or unprepared
 * model, -MPO_ENOTSUP: n too large for either) when mpo_gp_acq_grad would refuse the
 * model.  The launch makes its choice through the same helper.  Reads only model->n once
 * the model is accepted; needs a device, because the static LDS size is asked of the code
 * object (without one every model is answered -MPO_ENOTSUP). */
int mpo_gp_acq_grad_path(const MpoGpModel* model);

/* One polish round from the host: mpo_gp_acq_grad with x, acq, f, g in pinned
 * (hipHostMalloc / registered) host memory, read and written by the kernel in
 * place (no staging copies), then a synchronisation of `stream`.  MPO_EINVAL if
 * a buffer is not pinned host memory. */
int mpo_gp_acq_grad_host(const MpoGpModel* model, const double* x_host, int batch, const int32_t* acq_host,
                         double y_opt, double xi, double kappa, double* f_host, double* g_host, void* stream);

/* ------------------------------------------------------------------------
 * Cost-aware acquisitions EIps / PIps (skopt acquisition.py: acq_func "EIps" / "PIps",
 * reached from Coordinator.ask, coordinator.py:46-50, once tell receives (value, time)
 * pairs).  Two prepared models over the SAME observations: fmodel on the objective, tmodel
 * on log t.  With a(x) = -EI or -PI under fmodel (mpo_gp_acq_score's value, the sd <= 0 -> 0
 * rule included) and (mu, s) = tmodel's posterior mean / std in the units of log t:
 *   inv_t(x) = exp(-mu + s^2 / 2)      E[1/t] of a log-normal t, evaluated as
 *                                      exp(fma(0.5 s, s, -mu)) with the device library's exp
 *   v(x)     = a(x) inv_t(x)           the value that is minimised
 *   grad v   = grad a inv_t + v (-grad mu + s grad s)
 * MPO_EINVAL: a null or malformed model, fmodel->n != tmodel->n or another d.  All refusals
 * are made on the host before any launch; the device forms only enqueue work: no
 * allocation, no host synchronisation, no atomics.
 * ---------------------------------------------------------------------- */

/* Workspace bytes of mpo_gp_acq_ps_score: the larger of the two models' scoring workspaces
 * (the passes run one after the other), 4 rows of m doubles and the finish pass's top-k
 * lists.  0 for what that call refuses. */
size_t mpo_gp_acq_ps_ws_bytes(const MpoGpModel* fmodel, const MpoGpModel* tmodel, int64_t m, int k);

/* Score m candidates ([m][d] device): fmodel's scoring path (resident or streamed, as
 * mpo_gp_score_path says) into workspace value rows, tmodel's into workspace mu / sd rows,
 * then one elementwise finish pass:
 *   vals[a*m + i]          v of acquisition a in {EI, PI} order (mpo_gp_acq_score's rows;
 *                          rows of unset flags untouched)            ([2][m] or NULL)
 *   inv_t[i]                                                           ([m] or NULL)
 *   topk_idx/val[a*k + r]  the k smallest v of acquisition a by (value, index): lowest index
 *                          on ties, -0.0 == 0.0; index -1 where m < k (NULL with k = 0)
 * flags is a non-empty subset of MPO_ACQ_EI | MPO_ACQ_PI.  A candidate's outputs do not
 * depend on m, on the grid or on the rows around it.  MPO_EINVAL also for m < 1, a flag
 * outside EI | PI, k outside [0, MPO_TOPK_MAX], k > 0 without top-k outputs, k = 0 with
 * neither vals nor inv_t, a workspace smaller than mpo_gp_acq_ps_ws_bytes. */
int mpo_gp_acq_ps_score(const MpoGpModel* fmodel, const MpoGpModel* tmodel, const double* cand, int64_t m,
                        double y_opt, double xi, unsigned flags, double* vals, double* inv_t, int k,
                        int64_t* topk_idx, double* topk_val, void* ws, size_t ws_bytes, void* stream);

/* The polish objective: f[b] = v and g[b][d] = grad v of acquisition acq[b] (device int32,
 * MPO_ACQ_EI or MPO_ACQ_PI; any other code cannot be seen from the host and gives NaN) at
 * the points x [batch][d] (device); parts (or NULL) [batch][4] = (a, inv_t, mu_t, s_t).  One
 * launch, one workgroup per point: both posteriors and their gradients one model after the
 * other in the same LDS, each by the sequence of mpo_gp_acq_grad's kernel in that kernel's
 * summation order; 16 waves per point while 19 n doubles plus the static LDS fit the
 * 160 KiB, 4 past it (mpo_gp_acq_ps_grad_path), every n <= 2048.  Every sum runs in a fixed
 * order: a point's f and g are the same bits whatever the batch or its order.
 * batch in [1, 65535]. */
int mpo_gp_acq_ps_grad(const MpoGpModel* fmodel, const MpoGpModel* tmodel, const double* x, int batch,
                       const int32_t* acq, double y_opt, double xi, double* f, double* g, double* parts,
                       void* stream);

/* Waves per point (16 or 4) of the kernel mpo_gp_acq_ps_grad launches for this pair, or
 * negative (-MPO_EINVAL, -MPO_ENOTSUP) when it would be refused.  Needs a device, as
 * mpo_gp_acq_grad_path does. */
int mpo_gp_acq_ps_grad_path(const MpoGpModel* fmodel, const MpoGpModel* tmodel);

/* One polish round from the host: mpo_gp_acq_ps_grad with x, acq, f, g (and parts, when
 * given) in pinned host memory, read and written in place, then one synchronisation of
 * `stream`.  MPO_EINVAL also if a buffer is not pinned or a code is neither EI nor PI
 * (checked on the host here). */
int mpo_gp_acq_ps_grad_host(const MpoGpModel* fmodel, const MpoGpModel* tmodel, const double* x_host, int batch,
                            const int32_t* acq_host, double y_opt, double xi, double* f_host, double* g_host,
                            double* parts_host, void* stream);

/* ------------------------------------------------------------------------
 * A committee of exact GPs as one surrogate: the robust Bayesian committee machine (rBCM;
 * Deisenroth & Ng, "Distributed Gaussian Processes", ICML 2015).  NOT the reference's
 * semantics (skopt fits one GP to all told points); it serves the opt-in
 * Optimizer(surrogate="committee") past one GP's 2048 observations.  `models` is a HOST array
 * of E prepared MpoGpModel ("experts") over disjoint parts of the observations that share d,
 * dp, amp, the length scales and ONE target normalisation (y_mean, y_std).  In normalised
 * units expert e gives the mean m_e and the variance v_e = amp - q_e at a point; with
 *   r_e = v_e / amp clamped to [2^-52, 1]   (a clamped r_e has zero derivative; r_e = 1
 *                                            contributes nothing)
 *   b_e = -ln(r_e) / 2
 *   S   = sum_e b_e (1 / r_e - 1)           P = 1 + S >= 1: never less certain than the prior
 *   M   = sum_e b_e m_e / r_e
 * the committee's posterior is mu = y_mean + y_std M / P, sd = y_std sqrt(amp / P); EI, PI
 * and LCB and their gradients are mpo_gp_acq_score's / mpo_gp_acq_grad's on (mu, sd).  Both
 * sums start from 0 and add expert 0 .. E-1 in that order: a point's outputs are the same
 * bits whatever m, the batch or the launch.  E = 1 is the rBCM of one expert (b_0 != 1), not
 * that expert's own posterior.
 * Refused on the host before any launch, with a message in mpo_last_error(): MPO_EINVAL for
 * E outside [1, MPO_COMMITTEE_MAX], a null or malformed expert, experts that differ in d,
 * dp, amp, y_mean or y_std; MPO_ENOTSUP for an expert with n > 2048.  The length scales are
 * device data: mpo_gp_committee_check compares them (and synchronises); the other entry
 * points only enqueue and take them on trust.  A caller who skips the check and passes experts
 * with different length scales gets NO error: every expert is then scored and differentiated
 * under its own length scales, which is a different model from the one documented here.
 * ---------------------------------------------------------------------- */
#define MPO_COMMITTEE_MAX 32

/* The refusals above, then the experts' length scales read back and compared (MPO_EINVAL
 * when two differ).  Synchronises `stream`; call it once after the experts are prepared. */
int mpo_gp_committee_check(const MpoGpModel* models, int E, void* stream);

/* Workspace bytes of mpo_gp_committee_score: the largest expert's scoring workspace (the
 * passes run one after the other), 4 rows of m doubles (the running S and M, one expert's
 * mu and sd) and the finish pass's top-k lists -- independent of E.  0 for what that call
 * refuses. */
size_t mpo_gp_committee_ws_bytes(const MpoGpModel* models, int E, int64_t m, int k);

/* Score m candidates ([m][d] device) under the committee: each expert's own scoring path
 * (resident or streamed, as mpo_gp_score_path says) writes its (mu, sd) rows, one elementwise
 * pass folds them into S and M, and the last expert's pass also finishes:
 *   mu, sd                 the committee's posterior mean / std          ([m] or NULL)
 *   vals[a*m + i]          the minimised value of acquisition a in {EI, PI, LCB} order (rows
 *                          of unset flags untouched)                      ([3][m] or NULL)
 *   topk_idx/val[a*k + r]  the k smallest values of acquisition a by (value, index): lowest
 *                          index on ties; index -1 where m < k (NULL with k = 0)
 * MPO_EINVAL also for m < 1, bad flags, k outside [0, MPO_TOPK_MAX], k > 0 without top-k
 * outputs, k = 0 with none of mu, sd, vals, a workspace smaller than
 * mpo_gp_committee_ws_bytes.  Only enqueues work: no allocation, no host synchronisation,
 * no atomics, capturable in a graph.  The experts' length scales are NOT compared here
 * (mpo_gp_committee_check does that once): see above for what unequal ones give. */
int mpo_gp_committee_score(const MpoGpModel* models, int E, const double* cand, int64_t m,
                           double y_opt, double xi, double kappa, unsigned flags,
                           double* mu, double* sd, double* vals, int k,
                           int64_t* topk_idx, double* topk_val,
                           void* ws, size_t ws_bytes, void* stream);

/* The polish objective under the committee: f[b] and g[b][d] of acquisition acq[b] (device
 * int32, MPO_ACQ_EI / MPO_ACQ_PI / MPO_ACQ_LCB) at the points x [batch][d] (device).  One
 * launch, one workgroup per point: every expert's posterior and gradient one after the other
 * in the same LDS, each by the sequence of mpo_gp_acq_grad's kernel, the wave form (16 or 4,
 * mpo_gp_committee_grad_path) chosen for the largest expert.  Every sum runs in a fixed order:
 * a point's f and g are the same bits whatever the batch or its order.  batch in [1, 65535].
 * The experts' length scales are NOT compared here (mpo_gp_committee_check): each expert's
 * posterior is taken under its own, as mpo_gp_committee_score takes it. */
int mpo_gp_committee_grad(const MpoGpModel* models, int E, const double* x, int batch,
                          const int32_t* acq, double y_opt, double xi, double kappa,
                          double* f, double* g, void* stream);

/* Waves per point (16 or 4) of the kernel mpo_gp_committee_grad launches, or negative
 * (-MPO_EINVAL, -MPO_ENOTSUP) when it would be refused.  Needs a device, as
 * mpo_gp_acq_grad_path does. */
int mpo_gp_committee_grad_path(const MpoGpModel* models, int E);

/* One polish round from the host: mpo_gp_committee_grad with x, acq, f, g in pinned host
 * memory, read and written in place, then one synchronisation of `stream`. */
int mpo_gp_committee_grad_host(const MpoGpModel* models, int E, const double* x_host, int batch,
                               const int32_t* acq_host, double y_opt, double xi, double kappa,
                               double* f_host, double* g_host, void* stream);

/* ------------------------------------------------------------------------
 * The JOINT posterior of a prepared model over m query points (transformed space,
 * [m][d] device): what sklearn's GaussianProcessRegressor.predict(X, return_cov=True)
 * and sample_y(X, n_samples) give (_gpr.py:370-470, 472-507), for skopt's fitted GP
 * (result.models[-1]).  Reads the model's plain W = L^-1, xs and alpha only: any
 * prepared, appended or copied (from its exported workspace) model of n <= 2048
 * observations is served, whatever its scoring path.  fp64 MFMA throughout; every sum
 * runs in a fixed order, so two calls give the same bits.
 * ---------------------------------------------------------------------- */
#define MPO_JOINT_MAX 4096
/* The most draws of one mpo_gp_sample call: 16 x 65535, the y extent of the sampling
 * kernel's grid (16 draws per workgroup). */
#define MPO_JOINT_SMAX 1048560

/* Workspace bytes of mpo_gp_posterior_cov (s = 0) or mpo_gp_sample (s >= 1 draws) over m
 * query points: V = K* W^T [m32][np16], and for s >= 1 the [m32][m32] matrix that is
 * factored (m32 = m rounded up to 32; 194 MiB at n = 2048, m = 4096).  0 if unsupported:
 * null or malformed model, n > 2048, m < 1, m > MPO_JOINT_MAX, s < 0, s > MPO_JOINT_SMAX. */
size_t mpo_gp_joint_ws_bytes(const MpoGpModel* model, int m, int s);

/* mu [m] (or NULL: not written) and cov [m][ldc]:
 *   mu = y_mean + y_std K* alpha,   cov = y_std^2 (amp Matern52(|c_i - c_j|) - V V^T),
 * V = K* W^T, K* = amp Matern52(|c - xs|) by direct differences.  No noise term (skopt
 * zeroes the WhiteKernel after the fit): diag(cov) is the sd^2 of mpo_gp_acq_score.
 * cov is exactly symmetric (each lower 16 x 16 tile is written with its mirror).
 * MPO_ENOTSUP: m > MPO_JOINT_MAX or n > 2048.  MPO_EINVAL: a null pointer (mu excepted),
 * m < 1, ldc < m, a malformed model, a workspace smaller than
 * mpo_gp_joint_ws_bytes(model, m, 0).  All checks run on the host before any launch.
 * Only enqueues work: no allocation, no host synchronisation, capturable in a graph. */
int mpo_gp_posterior_cov(const MpoGpModel* model, const double* cand, int m,
                         double* mu /*[m] or NULL*/, double* cov /*[m][ldc]*/, int ldc,
                         void* ws, size_t ws_bytes, void* stream);

/* s correlated draws of the posterior at the m query points, and the argmin of each:
 *   Lc Lc^T = Sigma_n + jitter amp I   (Sigma_n = cov / y_std^2; blocked Cholesky, the
 *                                       kernels and step order of mpo_gp_prepare)
 *   samples[r][i] = mu[i] + y_std sum_{j <= i} Lc[i][j] z[j][r]
 *   argmin[r]     = the lowest index among the smallest samples[r][.]  (np.argmin)
 * z [m][s] (device) holds the caller's standard normal variates; samples [s][m] and
 * argmin [s] may each be NULL (not written).  *info (device int32): 0, or the first
 * failed column + 1 as mpo_chol_f64 reports it -- the outputs are then meaningless and
 * the caller retries with a larger jitter.
 * MPO_ENOTSUP: m > MPO_JOINT_MAX, n > 2048 or s > MPO_JOINT_SMAX.  MPO_EINVAL: a null model,
 * cand, z, info or workspace, m < 1, s < 1, a negative or non-finite jitter, a malformed
 * model, a workspace smaller than mpo_gp_joint_ws_bytes(model, m, s).  All checks run on the
 * host before any launch.  Only enqueues work: no allocation, no host synchronisation.
 * sklearn's sample_y draws through multivariate_normal's SVD: the same distribution,
 * other bits.
 * NOT the reference's semantics: skopt's ask(n_points) (Coordinator.ask,
 * coordinator.py:46-50) is a constant-liar batch; this entry point serves the opt-in
 * Thompson batch (Optimizer(batch_strategy="thompson") / ask(n, strategy="thompson")),
 * and GPModel.sample_y. */
int mpo_gp_sample(const MpoGpModel* model, const double* cand, int m,
                  const double* z /*[m][s]*/, int s, double jitter /* >= 0, relative to amp */,
                  double* samples /*[s][m] or NULL*/, int64_t* argmin /*[s] or NULL*/,
                  int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * PARTIAL DEPENDENCE of a prepared model's posterior mean: the post-analysis of a finished
 * search.  Replaces the loops of skopt plots.partial_dependence_1D / _2D (plot_objective),
 * which a user of the reference reaches after Coordinator.run (coordinator.py:102-103) and
 * which evaluate predict() at every sample with one or two dimensions overwritten by a grid
 * value.  Reads n, d, dp, amp, y_mean, y_std, xs, ls and alpha only: any prepared, appended
 * or copied model of n <= 2048 observations is served, whatever its scoring path.
 *
 * samples [S][d] (device) are rows of the transformed space.  A task names one or two column
 * spans [col, col + width) of it (a one-hot Categorical is a span of width > 1; width 0: the
 * axis is absent -- a 1-D task has no b) and, per span, `count` grid values of `width` doubles
 * each at grid + grid_off ([count][width], device).  For every cell (ga, gb)
 *   out[out_off + ga * max(b.count, 1) + gb] =
 *       y_mean + y_std (1 / S) sum_s sum_i alpha_i amp Matern52(r_si(ga, gb))
 *   r_si^2 = sum_{k outside the spans} (samples[s][k] / ls_k - xs[i][k])^2
 *          + sum_{k in a} (grid_a[ga][k] / ls_k - xs[i][k])^2 + sum_{k in b} (grid_b[gb][k] / ls_k - xs[i][k])^2
 * -- the mean over the samples of the posterior mean at the sample with the spans' columns
 * overwritten.  The three parts are sums of squares of direct differences (nothing is
 * subtracted); the first is formed once per tile of samples and observations, the other two
 * once per axis, and a cell costs S n Matern evaluations.  No atomics; every sum runs in a
 * fixed order given (S, n), and a task's output bits depend on the model, the samples and
 * that task alone -- not on T, its position, the other tasks or earlier calls.
 * ---------------------------------------------------------------------- */
#define MPO_PD_GMAX 64      /* grid values per axis            */
#define MPO_PD_SMAX 4096    /* sample rows                     */
#define MPO_PD_TMAX 1024    /* tasks per call (d = 32: 32 + 496) */
typedef struct MpoPdAxis {
    int32_t col, width, count, reserved;   /* width 0: absent */
    int64_t grid_off;                      /* doubles into grid */
} MpoPdAxis;
typedef struct MpoPdTask {
    MpoPdAxis a, b;
    int64_t out_off;                       /* doubles into out: [a.count][max(b.count, 1)] */
} MpoPdTask;

/* Workspace bytes of mpo_gp_partial_dependence: the scaled samples [S][d] and, per task, one
 * partial sum per cell and split (min(ceil(S / 64), 8) x min(ceil(n / 256), 4) splits:
 * 4 x 1600 doubles for a 40 x 40 pair at S = 250, n = 200).  0 for anything the call would
 * refuse. */
size_t mpo_gp_pd_ws_bytes(const MpoGpModel* model, int S, const MpoPdTask* tasks_host, int T);

/* The T tasks of tasks_host (HOST memory, read during the call: it travels to the kernels by
 * value, 48 tasks per launch) over one sample set.  MPO_ENOTSUP: n > 2048.  MPO_EINVAL: a null
 * or unprepared model, a null buffer, S outside [1, MPO_PD_SMAX], T outside [1, MPO_PD_TMAX],
 * an absent first axis, a span outside [0, d), spans a and b that overlap, a count outside
 * [1, MPO_PD_GMAX], a negative width or offset, output ranges of two tasks that overlap, a
 * workspace smaller than mpo_gp_pd_ws_bytes.  All checks run on the host before any launch
 * (the extents of grid and out are the caller's promise).  Only enqueues work: no allocation,
 * no host synchronisation, no asynchronous read of host memory; capturable in a graph. */
int mpo_gp_partial_dependence(const MpoGpModel* model, const double* samples /*[S][d]*/, int S,
                              const MpoPdTask* tasks_host, int T, const double* grid, double* out,
                              void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * PATHWISE posterior samples of a prepared model (Matheron's rule; Wilson et al. 2020,
 * "Efficiently sampling functions from Gaussian process posteriors"): a draw is a
 * function that can be evaluated at any point -- a prior draw from F random Fourier
 * features plus a data-dependent correction through the factor the model holds.  No
 * m x m matrix, no factorisation, no jitter and no cap on m.  With c = x / ls,
 * phi_j(x) = cos(omega_j . c + phase_j), scale = sqrt(2 amp / F) and the caller's
 *   omega [F][d]  frequencies in the length-scaled space, the spectral law of the
 *                 unit-length-scale Matern-5/2 kernel: z sqrt(5 / u), z ~ N(0, I_d),
 *                 u ~ chi^2_5
 *   phase [F]     uniform on [0, 2 pi)
 *   w [F][s], eps [n][s]   standard normal
 * the s paths are
 *   resid[:, r] = scale Phi(X) w[:, r] + sqrt(noise + 1e-10) eps[:, r]
 *   v[:, r]     = alpha - W^T (W resid[:, r])
 *   coef        = [scale w ; v]                                          [(F + n)][s]
 *   f_r(x)      = y_mean + y_std (sum_j phi_j(x) coef[j][r]
 *                                 + sum_i amp Matern52(|c - xs_i|) coef[F + i][r])
 * The conditioning on the data is exact; the prior is a random-feature APPROXIMATION of
 * the Matern-5/2 prior.  With an exact prior f_r has the mean and the noise-free
 * covariance of mpo_gp_posterior_cov.  Reads the model's plain W, xs, alpha and ls only:
 * any prepared, appended or copied model of n <= 2048 observations is served, whatever
 * its scoring path.  Every sum runs in a fixed order: two calls give the same bits, and
 * the value of a point under a draw does not depend on m, on the rows around it or on
 * the draw range of the call.
 * NOT the reference's semantics and not exact Thompson sampling: skopt's ask(n_points)
 * (Coordinator.ask, coordinator.py:46-50) is a constant-liar batch, and sklearn's
 * sample_y (_gpr.py:472-507) draws from the exact joint posterior; these entry points
 * serve the opt-in acq_optimizer_kwargs["ts_sampler"] = "paths" Thompson batch and
 * GPModel.sample_paths.
 * ---------------------------------------------------------------------- */
#define MPO_PATHS_FMAX 4096      /* random features per set of paths   */
#define MPO_PATHS_SMAX 1024      /* draws per set of paths             */

/* A prepared set of paths (host struct): device pointers into the prepare workspace. */
typedef struct MpoGpPaths {
    int32_t F;             /* features                                           */
    int32_t s;             /* draws                                              */
    int32_t n;             /* observations of the model the paths were built for */
    int32_t dp;            /* its padded dimensions                              */
    int32_t Fp;            /* F rounded up to 16                                 */
    int32_t Kp;            /* Fp + np16 rounded up to 64: rows of coef           */
    int32_t sp;            /* s rounded up to 16, plus 16: row stride of coef    */
    int32_t reserved;
    const double* omega;   /* [Fp][dp] zero-padded                               */
    const double* phase;   /* [Fp]                                               */
    const double* coef;    /* [Kp][sp] rows [0, F): scale w; [Fp, Fp + n): v; 0 elsewhere */
} MpoGpPaths;

/* Workspace bytes of mpo_gp_paths_prepare: the paths plus Phi(X) [n][F] and two [n][s]
 * intermediates (145 MiB at n = 2048, F = 4096, s = 1024; 10 MiB at 256, 2048, 256).  0 if
 * unsupported: a null or malformed model, n > 2048, F < 1, F > MPO_PATHS_FMAX, s < 1,
 * s > MPO_PATHS_SMAX. */
size_t mpo_gp_paths_ws_bytes(const MpoGpModel* model, int F, int s);

/* Build coef by the formulas above into `ws`; `paths` receives pointers into it, so `ws`
 * stays alive while the paths are used.  `noise` is the WhiteKernel value the model was
 * prepared with.  omega, phase, w, eps: device.
 * MPO_ENOTSUP: n > 2048, F > MPO_PATHS_FMAX or s > MPO_PATHS_SMAX.  MPO_EINVAL: a null
 * pointer, F < 1, s < 1, a negative or non-finite noise, a malformed model, a workspace
 * smaller than mpo_gp_paths_ws_bytes(model, F, s).  All checks run on the host before any
 * launch.  Only enqueues work: no allocation, no host synchronisation, capturable in a
 * graph. */
int mpo_gp_paths_prepare(const MpoGpModel* model, double noise,
                         const double* omega /*[F][d]*/, const double* phase /*[F]*/,
                         const double* w /*[F][s]*/, const double* eps /*[n][s]*/, int F, int s,
                         MpoGpPaths* paths, void* ws, size_t ws_bytes, void* stream);

/* Workspace bytes of mpo_gp_paths_eval (the workgroups' (min, index) partials); 0 if
 * unsupported: a null or malformed model or paths, m < 1, n_draws outside [1, s]. */
size_t mpo_gp_paths_eval_ws_bytes(const MpoGpModel* model, const MpoGpPaths* paths, int64_t m, int n_draws);

/* Draws first_draw .. first_draw + n_draws - 1 at the m candidates (transformed space,
 * [m][d] device), one fused kernel: per tile of 64 candidates the operand
 * [cos(omega_j . c + phase_j) | amp Matern52(|c - xs_i|)] is computed once, panel by panel,
 * and multiplied into coef on fp64 MFMA for every draw of the call.
 *   samples[k][i]  draw first_draw + k at candidate i              ([n_draws][m] or NULL)
 *   argmin[k]      the lowest index among the smallest samples[k][.]  (np.argmin; or NULL)
 *   minval[k]      that sample, bit for bit                                     (or NULL)
 * MPO_ENOTSUP: n > 2048, F > MPO_PATHS_FMAX or s > MPO_PATHS_SMAX.  MPO_EINVAL: a null
 * model, paths, cand or workspace, m < 1, a draw range outside [0, s), a malformed model
 * or paths struct (or paths of another model shape), a workspace smaller than
 * mpo_gp_paths_eval_ws_bytes(model, paths, m, n_draws).  All checks run on the host before
 * any launch.  Only enqueues work: no allocation, no host synchronisation, no atomics,
 * capturable in a graph.  MPO_PATHS_GRID=<workgroups> lowers the cap on the grid's x extent
 * (512 workgroups per 256 draws; a test knob: the values do not depend on it). */
int mpo_gp_paths_eval(const MpoGpModel* model, const MpoGpPaths* paths,
                      const double* cand /*[m][d]*/, int64_t m, int first_draw, int n_draws,
                      double* samples /*[n_draws][m] or NULL*/, int64_t* argmin /*[n_draws] or NULL*/,
                      double* minval /*[n_draws] or NULL*/, void* ws, size_t ws_bytes, void* stream);

/* Value and gradient of draw[b] at the point x[b] (transformed space), b < batch: the
 * objective of a continuous minimisation of a sample path.  With a_j = omega_j . c + phase_j,
 * D_i = c - xs_i, k_i = sqrt(5) |D_i|:
 *   f   = y_mean + y_std (sum_j cos(a_j) coef[j][r] + sum_i amp (1 + k_i + k_i^2/3) e^-k_i coef[Fp+i][r])
 *   g_k = y_std / ls_k (- sum_j sin(a_j) coef[j][r] omega_jk
 *                       - sum_i amp (5/3)(1 + k_i) e^-k_i coef[Fp+i][r] D_ik)
 * ((dMatern/dr) / r: no division by r, an observation at x adds exactly 0).  One workgroup
 * per run; every sum in a fixed order that depends on (F, n) alone: a run's f and g are the
 * same bits whatever the batch, its order or the other runs in it.  Reads the model's plain
 * xs and ls and the paths' omega, phase and coef only.
 * MPO_EINVAL: a null pointer, batch outside [1, MPO_PATHS_GRAD_BMAX], a malformed model or
 * paths struct, paths of another model shape; all checked on the host before any launch.  A
 * draw[b] outside [0, s) cannot be seen from the host: that run's f and g are NaN, and
 * nothing out of range is read.  Only enqueues work: no allocation, no host
 * synchronisation, no atomics, capturable in a graph.
 * NOT the reference's semantics (see above). */
#define MPO_PATHS_GRAD_BMAX 8192
int mpo_gp_paths_grad(const MpoGpModel* model, const MpoGpPaths* paths,
                      const double* x /*[batch][d]*/, const int32_t* draw /*[batch]*/, int batch,
                      double* f /*[batch]*/, double* g /*[batch][d]*/, void* stream);

/* mpo_gp_paths_grad with x, draw, f, g in pinned (hipHostMalloc / registered) host memory,
 * read and written by the kernel in place, then a synchronisation of `stream`.  MPO_EINVAL
 * also if a buffer is not pinned host memory or a draw lies outside [0, s) (checked on the
 * host here). */
int mpo_gp_paths_grad_host(const MpoGpModel* model, const MpoGpPaths* paths, const double* x_host,
                           const int32_t* draw_host, int batch, double* f_host, double* g_host, void* stream);

/* ------------------------------------------------------------------------
 * Acquisition candidates drawn on the device (opt-in: Optimizer(candidates="device")).
 * skopt draws the n_points candidates of every ask on the host, column by column from
 * one RandomState (Space.rvs + transform, reached from Coordinator.ask,
 * coordinator.py:46-50); that stays the default.  NOT the reference's stream: here
 * candidate i is a pure function of (seed, i), so any slice of the set can be made on
 * any device without being sent.
 * ---------------------------------------------------------------------- */
#define MPO_DIM_REAL 0
#define MPO_DIM_INTEGER 1
#define MPO_DIM_CATEGORICAL 2

/* One dimension of the ORIGINAL search space. */
typedef struct MpoDimDesc {
    int32_t kind;          /* MPO_DIM_*                                                   */
    int32_t pad;
    int64_t count;         /* Integer: high - low (>= 0, < 2^52); Categorical: number of
                              categories (>= 1); Real: ignored                            */
} MpoDimDesc;

/* Rows first .. first + m - 1 of the candidate set of `seed`, in the transformed space:
 * out [m][d] fp64 row-major (device), the layout mpo_gp_acq_score takes.  Transformed
 * widths: Real and Integer 1 column; Categorical 1 column with <= 2 categories, else one
 * column per category.  d must equal the sum of the widths and be <= 32; n_dims 1..32.
 * The law (fixed: tests compare bits with a numpy restatement, tests/philox_ref.py):
 *   Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl 0x9E3779B9 / 0xBB67AE85),
 *   key (seed low 32, seed high 32); for candidate i and the pair b of original
 *   dimensions (2b, 2b+1) the counter is (i low 32, i high 32, b, 0) and, of the output
 *   words r0..r3, dimension 2b takes u = u53(r0, r1) and 2b+1 takes u = u53(r2, r3),
 *   u53(a, b) = ((a >> 5) 2^26 + (b >> 6)) 2^-53 in [0, 1).
 *   Real (either prior)  the column is u (the transformed space is the warped unit interval)
 *   Integer, span s      0.0 when s == 0, else rint(u s) / s in fp64, ties to even: the
 *                        grid k/s of Integer.transform, the end values with half the
 *                        mass of the inner ones, as skopt's round of a uniform draw gives
 *   Categorical, c       j = min((int)(u c), c - 1); one column: (double)j; else the
 *                        one-hot row of j
 * Against the host path the distribution differs on a set of measure zero only (the
 * host draws Reals with an inclusive upper bound and round-trips them through
 * inverse_transform / transform, a few ulp); the bits and the RandomState stream differ.
 * dims is a HOST array; it reaches the kernel by value, so there is no workspace and no
 * upload.  Every argument is validated before any GPU call.  m == 0 returns MPO_OK and
 * launches nothing; first < 0, m < 0 and first + m > 2^62 return MPO_EINVAL, as do a
 * null or misaligned (8 B) out with m > 0, an unknown kind and a count outside its
 * range.  Only enqueues on `stream`: no allocation, no synchronisation, capturable. */
int mpo_space_sample(const MpoDimDesc* dims, int n_dims, int d, uint64_t seed, int64_t first, int64_t m,
                     double* out, void* stream);

/* Candidates that ARE the legal points of the discrete dimensions (opt-in:
 * Optimizer(candidates="lattice")).  skopt scores random draws of a relaxed box, polishes
 * them in that box and rounds the result; here every combination of the Integer and
 * Categorical values is a candidate and only the Reals are drawn.  NOT the reference's
 * semantics, and not its stream.
 * The law (fixed: tests compare bits with a numpy restatement, tests/test_lattice_gpu.py):
 *   Discrete dimensions are the Integers and the Categoricals.  The radix of an Integer of
 *   span s = count is s + 1, that of a Categorical its count c.  L is the product of the
 *   radices, 1 for a space without a discrete dimension; L > 2^62 is MPO_EINVAL from both
 *   calls.
 *   Row r (first <= r < first + m) belongs to lattice point l = r mod L.  l is a mixed-radix
 *   number over the discrete dimensions in table order with the LAST one fastest
 *   (itertools.product over their values): digit_j = (l / place_j) mod radix_j, place_j the
 *   product of the radices of the discrete dimensions after j.
 *   Integer, digit k      0.0 when s == 0, else (double)k / (double)s: the grid of
 *                         Integer.transform
 *   Categorical, digit j  one column: (double)j; else the one-hot row of j (the widths of
 *                         mpo_space_sample)
 *   Real                  exactly the column mpo_space_sample(seed) writes at row r: the
 *                         Philox counter (r low 32, r high 32, b, 0) of its pair b, its half
 *                         of the output words and u53.  Rows of one lattice point (r, r + L,
 *                         ...) so carry different Reals.
 * Rows and l are 64-bit; with L < 2^32 the digits are taken in 32-bit arithmetic, the same
 * integers.
 * mpo_space_lattice_size is host only: *L from a checked table (no d: it writes no rows).
 * mpo_space_lattice takes mpo_space_sample's arguments with its conventions and refusals:
 * dims is a HOST array that reaches the kernel by value; every argument is validated before
 * any GPU call; m == 0 returns MPO_OK and launches nothing; only enqueues on `stream`: no
 * workspace, no allocation, no synchronisation, capturable. */
int mpo_space_lattice_size(const MpoDimDesc* dims, int n_dims, int64_t* L);
int mpo_space_lattice(const MpoDimDesc* dims, int n_dims, int d, uint64_t seed, int64_t first, int64_t m,
                      double* out, void* stream);

/* ------------------------------------------------------------------------
 * L-BFGS-B drivers (host C++, no Python in the loop).  skopt's refit runs
 * scipy.optimize.minimize(method="L-BFGS-B") from sklearn's
 * _constrained_optimization (_gpr.py:296-337) and its polish runs
 * fmin_l_bfgs_b(maxiter=20); both are reached from Coordinator.fit / ask
 * (coordinator.py:63-79, 46-50).  These run L-BFGS-B 3.0 with scipy's driver
 * rules over `nruns` independent starts whose objective evaluations are batched:
 * every round evaluates the point each live run needs in one call.  Outputs:
 * x_out [nruns][nvar], f_out [nruns] (scipy's OptimizeResult.fun), stats
 * [nruns][4] = (nit, nfev, status, 0) with status 1 = projected gradient <= gtol,
 * 2 = relative reduction <= ftol, 3 = maxiter, 4 = maxfun, 5 = abnormal line
 * search; *rounds = objective rounds.  bounds [nvar][2] = (lower, upper).
 * ---------------------------------------------------------------------- */
typedef struct MpoLbfgsbOptions {
    double ftol;        /* scipy ftol (factr * eps): minimize's default 2.22e-9, fmin_l_bfgs_b's 1e7 * eps */
    double gtol;        /* scipy gtol / pgtol (1e-5) */
    int32_t maxiter;    /* 15000 (minimize), 20 (skopt's polish) */
    int32_t maxfun;     /* 15000 */
    int32_t maxcor;     /* 10 */
    int32_t maxls;      /* 20 */
} MpoLbfgsbOptions;

/* Objective of mpo_lbfgsb_batched: f [batch], g [batch][nvar] at the points X
 * [batch][nvar] of runs ids [batch]; nonzero return aborts the minimisation. */
typedef int (*mpo_fg_batch_fn)(int batch, const double* X, const int32_t* ids, double* f, double* g, void* user);

/* The driver over a caller objective (host; the CPU tests compare it with scipy). */
int mpo_lbfgsb_batched(int nvar, int nruns, const double* x0, const double* bounds, const MpoLbfgsbOptions* opts,
                       mpo_fg_batch_fn fg, void* user, double* x_out, double* f_out, int32_t* stats,
                       int32_t* rounds);

/* mpo_lbfgsb_batched with a column mask shared by all runs: frozen [nvar], and where
 * frozen[j] != 0 run r holds coordinate j at its start -- its bounds there are
 * lo = hi = x0[r][j], clipped into bounds[j] first as every start is; L-BFGS-B treats such a
 * variable as fixed (scipy's does under the same bounds), so x_out[r][j] is that value bit
 * for bit.  A null mask is mpo_lbfgsb_batched. */
int mpo_lbfgsb_batched_frozen(int nvar, int nruns, const double* x0, const double* bounds, const uint8_t* frozen,
                              const MpoLbfgsbOptions* opts, mpo_fg_batch_fn fg, void* user, double* x_out,
                              double* f_out, int32_t* stats, int32_t* rounds);

/* A rendezvous for the concurrent refits on one device (the cl_min chains):
 * fits that share it evaluate their pending rounds together, one grouped launch
 * set per round of all registered fits, each theta's result unchanged.  Thread
 * safe; stats = grouped launch sets and the rounds they carried. */
int mpo_gp_lml_batcher_create(int device, void** handle);
int mpo_gp_lml_batcher_destroy(void* handle);
int mpo_gp_lml_batcher_stats(const void* handle, int64_t* launches, int64_t* rounds);

/* skopt's whole refit on the device objective: L-BFGS-B from starts [nruns][d+2]
 * (log theta) on -mpo_gp_lml_grad, one mpo_gp_lml_grad_host round per iteration
 * of all live runs (theta_host [nruns][d+2] and out_host as that call's pinned
 * buffers).  With a `batcher` (or NULL) of the stream's device, each round goes
 * through it and may launch together with other fits' rounds.  Replaces sklearn's
 * restart loop (_gpr.py:296-337) around scipy.optimize.minimize.  Synchronises
 * every round. */
int mpo_gp_fit_lml_host(const double* X, const double* y_norm, int n, int d, const double* starts, int nruns,
                        const double* bounds, const MpoLbfgsbOptions* opts, double* theta_host, double* out_host,
                        void* dev_io, size_t io_bytes, void* ws, size_t ws_bytes, double* x_out, double* f_out,
                        int32_t* stats, int32_t* rounds, void* batcher, void* stream);

/* skopt's polish of the best candidates: L-BFGS-B from starts [nruns][d] on the
 * minimised acquisition acq[r] of run r (mpo_gp_acq_grad_host rounds through the
 * pinned x_host [nruns][d], acq_host [nruns], f_host [nruns], g_host [nruns][d]).
 * Replaces skopt's fmin_l_bfgs_b(gaussian_acquisition_1D, x0, bounds, maxiter=20)
 * loop over the n_restarts_optimizer best candidates. */
int mpo_gp_polish_host(const MpoGpModel* model, const double* starts, const int32_t* acq, int nruns,
                       const double* bounds, const MpoLbfgsbOptions* opts, double y_opt, double xi, double kappa,
                       double* x_host, int32_t* acq_host, double* f_host, double* g_host, double* x_out,
                       double* f_out, int32_t* stats, int32_t* rounds, void* stream);

/* mpo_gp_polish_host that moves the continuous columns only (NOT the reference's semantics;
 * the polish of Optimizer(candidates="lattice")): frozen [d] as in mpo_lbfgsb_batched_frozen,
 * so the Integer and Categorical columns of every start stay where the lattice put them.  A
 * null mask is mpo_gp_polish_host.  The cost-aware, committee and pathwise polishes have no
 * such variant. */
int mpo_gp_polish_frozen_host(const MpoGpModel* model, const double* starts, const int32_t* acq, int nruns,
                              const double* bounds, const uint8_t* frozen, const MpoLbfgsbOptions* opts,
                              double y_opt, double xi, double kappa, double* x_host, int32_t* acq_host,
                              double* f_host, double* g_host, double* x_out, double* f_out, int32_t* stats,
                              int32_t* rounds, void* stream);

/* mpo_gp_polish_host on the cost-aware objective: L-BFGS-B from starts [nruns][d] on
 * acquisition acq[r] (MPO_ACQ_EI / MPO_ACQ_PI) per unit cost, one mpo_gp_acq_ps_grad_host
 * round per iteration of all live runs through the same pinned buffers.  skopt's polish
 * with acq_func "EIps" / "PIps". */
int mpo_gp_polish_ps_host(const MpoGpModel* fmodel, const MpoGpModel* tmodel, const double* starts,
                          const int32_t* acq, int nruns, const double* bounds, const MpoLbfgsbOptions* opts,
                          double y_opt, double xi, double* x_host, int32_t* acq_host, double* f_host, double* g_host,
                          double* x_out, double* f_out, int32_t* stats, int32_t* rounds, void* stream);

/* mpo_gp_polish_host on a committee's objective (NOT the reference's semantics): L-BFGS-B
 * from starts [nruns][d] on acquisition acq[r] under the E experts' rBCM posterior, one
 * mpo_gp_committee_grad_host round per iteration of all live runs through the same pinned
 * buffers. */
int mpo_gp_polish_committee_host(const MpoGpModel* models, int E, const double* starts, const int32_t* acq,
                                 int nruns, const double* bounds, const MpoLbfgsbOptions* opts, double y_opt,
                                 double xi, double kappa, double* x_host, int32_t* acq_host, double* f_host,
                                 double* g_host, double* x_out, double* f_out, int32_t* stats, int32_t* rounds,
                                 void* stream);

/* Each draw of a set of sample paths minimised from its own start (NOT the reference's
 * semantics): L-BFGS-B from starts [nruns][d] on draw[r] of `paths` (mpo_gp_paths_grad_host
 * rounds through the pinned x_host [nruns][d], draw_host [nruns], f_host [nruns], g_host
 * [nruns][d]).  MPO_EINVAL also for a draw outside [0, s). */
int mpo_gp_paths_polish_host(const MpoGpModel* model, const MpoGpPaths* paths, const double* starts,
                             const int32_t* draw, int nruns, const double* bounds, const MpoLbfgsbOptions* opts,
                             double* x_host, int32_t* draw_host, double* f_host, double* g_host, double* x_out,
                             double* f_out, int32_t* stats, int32_t* rounds, void* stream);

/* ------------------------------------------------------------------------
 * Population training of ragged MNIST-CNN trials.
 * Replaces ProcessBlock.train_model -> mpi_learn MPIKFoldManager.train()
 * (process_block.py:71-96) for test_mnist (mpiLAPI.py:138-176): every member
 * is one (trial, fold) pair; all members step together on one GPU.
 * ---------------------------------------------------------------------- */

/* One population member: the test_mnist hyper-parameters (option3:127-131)
 * plus the optimizer/dropout settings that the device table carries per trial.
 * Accepted (each extreme is compared with the fp64 oracle, tests/pop_cases.py):
 * nb_filters 1..64, kernel_size 1..10, pool_size 1..16 with pool_size <= 30 - 2 k
 * (one pool window at least), dense 1..4096, 0 <= dropout < 1, lr > 0.  The
 * comments below give option3's search space, which lies inside. */
typedef struct MpoCnnSpec {
    int32_t nb_filters;   /* F      Integer(10, 50)  */
    int32_t kernel_size;  /* k      Integer(2, 10)   */
    int32_t pool_size;    /* p      Integer(2, 10)   */
    int32_t dense;        /* dense  Integer(50, 200) */
    float lr;             /* learning rate (reference: Adam, 1e-3)           */
    float dropout;        /* dropout rate (reference: 0.25, mpiLAPI.py:151)   */
    uint32_t seed;        /* dropout stream seed                             */
    int32_t options;      /* MPO_LOSS_* | MPO_OPT_* (0: the reference's binary_crossentropy + Adam) */
} MpoCnnSpec;

/* MpoCnnSpec.options: option3's --loss (hyperparameter_search_option3.py:61) and
 * master --optimizer (:60), both handed to mpi_learn's Algo (:270-275). */
#define MPO_LOSS_BCE 0x0      /* Keras binary_crossentropy on the softmax (mean over the 10 outputs) */
#define MPO_LOSS_CCE 0x1      /* Keras categorical_crossentropy (renormalised, clipped 1e-7)        */
#define MPO_LOSS_MASK 0xff
#define MPO_OPT_ADAM 0x000    /* Keras Adam (beta 0.9 / 0.999, eps 1e-8)                            */
#define MPO_OPT_SGD 0x100     /* Keras SGD, no momentum: p -= lr g                                  */
#define MPO_OPT_MASK 0xff00

typedef struct MpoPopSizes {
    int64_t n_params;     /* floats in the parameter arena (also grads, adam m, adam v) */
    int64_t act_floats;   /* floats in the activation arena                              */
    int64_t table_bytes;  /* device bytes for the member table + work lists              */
    int32_t n_members;
    int32_t batch;
} MpoPopSizes;

/* Plan a population (host only: layouts, ragged work lists).  *handle owns host
 * memory only; release with mpo_pop_destroy.  n_members >= 1, batch 1..256 (else
 * MPO_EINVAL); a member outside MpoCnnSpec's accepted ranges returns MPO_ENOTSUP with
 * the member and the reason in mpo_last_error(): kernel_size > 10 (the conv1 weight
 * gradient holds k*k + 1 <= 112 rows per wave) and pool_size > 16 (the max-pool argmax
 * is one byte) computed wrong gradients before they were refused. */
int mpo_pop_create(const MpoCnnSpec* specs, int n_members, int batch, void** handle);
int mpo_pop_destroy(void* handle);
int mpo_pop_sizes(const void* handle, MpoPopSizes* out);
/* offsets[9] (floats into the parameter arena) of member's
 * w1 (k,k,1,F), b1, w2 (k,k,F,F), b2, w3 (s*s*F, dense), b3, w4 (dense,10), b4, end.
 * Keras weight shapes and order (Conv2D kernel (kh,kw,cin,cout), Dense (in,out)). */
int mpo_pop_param_layout(const void* handle, int member, int64_t* offsets);
/* offsets[15] (floats into the activation arena) of member's a1, a2, pd,
 * argmax (bytes at that float offset), h, hd, z3, dz3, dh, dp, dz2, dz1, w2t,
 * conv1 / conv2 weight-gradient partial slabs (diagnostics and tests). */
int mpo_pop_act_layout(const void* handle, int member, int64_t* offsets);
/* Bind caller-owned device arenas (zero-initialised by the caller) and upload
 * the work tables (async on `stream`). */
int mpo_pop_bind(void* handle, float* params, float* grads, float* adam_m, float* adam_v, float* act,
                 void* tables, void* stream);
/* One training step of every member on batch rows [row0, row0+batch) of its
 * sample order: sample = order[member*order_stride + row0 + b] indexes x
 * [n][784] f32 and labels [n] i32 (the k-fold split is this index gather).
 * step = global step counter (dropout stream; Adam t = step + 1).
 * loss_out[member] = mean Keras binary_crossentropy of the batch. */
int mpo_pop_train_step(void* handle, const float* x, const int32_t* labels, const int32_t* order,
                       int64_t order_stride, int64_t row0, int32_t step, float* loss_out, void* stream);
/* Validation forward (no dropout) of one batch: loss_sum[member] += sum of
 * per-sample losses, correct[member] += argmax hits. */
int mpo_pop_eval_step(void* handle, const float* x, const int32_t* labels, const int32_t* order,
                      int64_t order_stride, int64_t row0, float* loss_sum, int32_t* correct, void* stream);

/* Retire / re-activate members (a population whose members stop early, option3's
 * --early-stopping / --target-metric handed to MPIKFoldManager, process_block.py:83-90,
 * stops paying for them).  active: HOST array of n_members bytes, non-zero = the member
 * takes part in the following mpo_pop_train_step / mpo_pop_eval_step calls.  Every
 * member is active after mpo_pop_create; any mask may follow any other (a member may
 * come back), the current mask again is a no-op.
 * A retired member costs no kernel work: the work lists are rebuilt from the active
 * members' items (bucketed as a plan of those members alone) into the same `tables`
 * region, whose size and every layout (mpo_pop_sizes, mpo_pop_param_layout,
 * mpo_pop_act_layout) do not change.  Its parameters, gradients, Adam m / v and
 * activations are not written, nor its loss_out / loss_sum / correct entries.  An
 * active member's bits are those of the same steps with nobody retired.  With every
 * member retired a step returns MPO_OK and launches nothing.
 * Before mpo_pop_bind the call only replans (stream unused); after it the tables are
 * uploaded on `stream`, which must be the stream the steps run on, and the call waits
 * for that stream.  NOT capturable; a hipGraph captured before the call replays the
 * old work lists and grid sizes and must be re-captured. */
int mpo_pop_set_active(void* handle, const uint8_t* active, void* stream);
/* Work of one mpo_pop_train_step under the current mask (host arithmetic only):
 * workgroups over all its launches, and the launches.  Equal to those of a plan
 * created from the active members' specs alone; 0 and 0 with every member retired. */
int mpo_pop_step_work(const void* handle, int64_t* items, int64_t* launches);

/* Diagnostics: per-phase device milliseconds accumulated over the steps run
 * since the last reset, as "phase ms\n" lines into buf (cap bytes).  Only
 * populated when the plan was created with MPO_POP_PROFILE=1 in the
 * environment (then every step ends in an event sync); returns MPO_ENOTSUP
 * otherwise.  reset != 0 clears the accumulators after the read. */
int mpo_pop_profile(void* handle, char* buf, size_t cap, int reset);

/* ------------------------------------------------------------------------
 * DenseNet population (BASELINE config 5).
 * Replaces the per-block Keras training of DenseNet (densenet.py:135-196, built
 * by base_model.py:61-72 / mpiLAPI.py:197-201, trained by process_block.py:71-96).
 * All members share one architecture (the reference grid searches lr only,
 * base_model.py:84-92); each member has its own lr, weights and sample order.
 * ---------------------------------------------------------------------- */
typedef struct MpoDnArch {
    int32_t H, W, C;          /* img_dim (channels last)                 */
    int32_t classes;          /* nb_classes                              */
    int32_t depth;            /* 3 N + 4                                 */
    int32_t nb_dense_block;
    int32_t growth;           /* growth_rate                             */
    int32_t nb_filter;
} MpoDnArch;

typedef struct MpoDnSizes {
    int64_t n_params;     /* floats per member in the parameter arena (also grads, adam m, v) */
    int64_t n_state;      /* floats per member of BN moving statistics                         */
    int64_t act_floats;   /* floats in the activation arena (all members); ends with the per-member
                             lr table and the active member table of mpo_dn_set_active (int32
                             [n_members], each rounded up to 64 floats)                        */
    int32_t n_members;
    int32_t batch;
    int32_t n_layers;
    int32_t reserved;
} MpoDnSizes;

int mpo_dn_create(const MpoDnArch* arch, int n_members, int batch, void** handle);
int mpo_dn_destroy(void* handle);
int mpo_dn_sizes(const void* handle, MpoDnSizes* out);
/* Layer i: geom[8] = kind (0 initial conv, 1 dense-block conv, 2 transition, 3 head),
 * stage, H, W, cin, cout, kernel size, concat channel offset; offs[6] = float
 * offsets within a member's parameter block of the conv kernel (head: dense kernel),
 * gamma, beta, and within its state block of moving mean, moving variance, and
 * (head only) the dense bias; -1 where absent.  Keras shapes: conv (ks,ks,cin,cout),
 * gamma/beta/moving stats [H] (BatchNormalization axis=1 of NHWC). */
int mpo_dn_layer(const void* handle, int i, int32_t* geom, int64_t* offs);
/* Bind caller-owned, zero-initialised device arenas: params/grads/adam_m/adam_v
 * [n_members][n_params], state [n_members][n_state], act [act_floats]; lr is a
 * HOST array of n_members learning rates (copied, stream-synchronised). */
int mpo_dn_bind(void* handle, float* params, float* grads, float* adam_m, float* adam_v, float* state, float* act,
                const float* lr, void* stream);
/* One Adam step of every member on rows [row0, row0+batch) of its order table:
 * sample = order[member*order_stride + row0 + b] into x [n][H][W][C] f32, labels
 * [n] i32.  BN uses batch statistics and updates the moving averages.
 * loss_out[member] = mean categorical CE + l2 penalty (before the update);
 * Adam t = step + 1. */
int mpo_dn_train_step(void* handle, const float* x, const int32_t* labels, const int32_t* order,
                      int64_t order_stride, int64_t row0, int32_t step, float* loss_out, void* stream);
/* Inference-mode forward (BN moving averages) of one batch: loss_sum[member] +=
 * sum of per-sample CE, correct[member] += argmax hits. */
int mpo_dn_eval_step(void* handle, const float* x, const int32_t* labels, const int32_t* order,
                     int64_t order_stride, int64_t row0, float* loss_sum, int32_t* correct, void* stream);
/* out[member] = 1e-4 * sum of squared parameters (Keras adds it to val_loss).
 * Written for every member, retired or not. */
int mpo_dn_penalty(void* handle, float* out, void* stream);
/* mpo_pop_set_active for the DenseNet population, same semantics: active is a HOST
 * array of n_members bytes; the following mpo_dn_train_step / mpo_dn_eval_step calls
 * launch grids over the active members only, each workgroup reading its member from a
 * device table of active indices in the activation arena (act_floats grew by that table
 * only).  A retired member's parameters, gradients, Adam m / v, BN state and
 * activations are not written, nor its loss_out / loss_sum / correct entries.  The work
 * splits stay sized for the nominal population, so an active member's bits do not
 * change; with every member retired a step returns MPO_OK and launches nothing.
 * Before mpo_dn_bind it only replans; after it the table is uploaded on `stream` (the
 * stream the steps run on) and the call waits for that stream, as mpo_dn_bind does.
 * NOT capturable; a hipGraph captured before the call replays the old grid sizes and
 * must be re-captured. */
int mpo_dn_set_active(void* handle, const uint8_t* active, void* stream);
/* Workgroups and launches of one mpo_dn_train_step under the current mask (host
 * arithmetic only): those of a plan of as many members as are active. */
int mpo_dn_step_work(const void* handle, int64_t* workgroups, int64_t* launches);

/* ------------------------------------------------------------------------
 * Population training of the strided test_cnn, option3's `topclass` example
 * (mpiLAPI.py:178-195, hyperparameter_search_option3.py:108-123, base_model.py:21-55):
 *   Conv2D(32, k, strides 3, valid, relu) x 2 -> MaxPool 2x2 -> Dropout(dropout / 2)
 *   -> Flatten (NHWC) -> Dense(128, relu) -> Dropout(dropout) -> Dense(classes, softmax).
 * The input shape and the class count belong to the population; each member has its
 * own kernel_size, dropout, lr, seed and loss / optimizer bits.
 * ---------------------------------------------------------------------- */
typedef struct MpoTcSpec {
    int32_t kernel_size;  /* k 1..9 (option3: Integer(1, 6); CNNModel grid: 3..9)                 */
    float lr;             /* learning rate of the trainer (the builder's llr never reaches it)   */
    float dropout;        /* layer 0 drops dropout / 2, layer 1 dropout; a rate outside (0, 1)
                             is the identity, as Keras 2's Dropout.call                          */
    uint32_t seed;        /* dropout stream seed                                                 */
    int32_t options;      /* MPO_LOSS_* | MPO_OPT_*                                              */
} MpoTcSpec;

/* Plan a population on x [n][H][W][C] with `classes` outputs (host only).  n_members >= 1,
 * batch 1..256 (else MPO_EINVAL).  MPO_ENOTSUP, with the reason in mpo_last_error(), for
 * H or W outside 1..256, C outside 1..8, classes outside 2..16, a kernel_size outside
 * 1..9, a conv2 output ((in - k) / 3 + 1 per axis, twice) below 2 on either axis, lr <= 0,
 * a non-finite lr / dropout or an unknown option bit.  Nothing is clamped. */
int mpo_tc_create(const MpoTcSpec* specs, int n_members, int batch, int H, int W, int C, int classes, void** handle);
int mpo_tc_destroy(void* handle);
int mpo_tc_sizes(const void* handle, MpoPopSizes* out);
/* offsets[9] (floats into the parameter arena) of member's w1 (k,k,C,32), b1, w2 (k,k,32,32),
 * b2, w3 (Hp*Wp*32, 128), b3, w4 (128, classes), b4, end: Keras shapes and order, each
 * tensor contiguous. */
int mpo_tc_param_layout(const void* handle, int member, int64_t* offsets);
/* offsets[12] (floats into the activation arena) of member's a1 [B,H1,W1,32], a2 [B,H2,W2,32],
 * pd [B,K1], the pool argmax (int32 [B,K1]: 2 dy + dx), h, hd [B,128], z3, dz3 [B,classes],
 * dh, dp, dz2, dz1 (diagnostics and tests). */
int mpo_tc_act_layout(const void* handle, int member, int64_t* offsets);
/* As mpo_pop_bind (arenas zero-initialised by the caller); waits for the table upload. */
int mpo_tc_bind(void* handle, float* params, float* grads, float* adam_m, float* adam_v, float* act, void* tables,
                void* stream);
/* As mpo_pop_train_step / mpo_pop_eval_step, on x [n][H][W][C] f32: one update of every
 * member on rows [row0, row0 + batch) of its order row (dropout masks from the counter
 * hash at `step`, layer 0 after the pool, layer 1 after the dense layer; Adam t = step + 1);
 * loss_out[member] = mean loss of the batch.  The eval step runs without dropout and
 * accumulates loss_sum / correct. */
int mpo_tc_train_step(void* handle, const float* x, const int32_t* labels, const int32_t* order,
                      int64_t order_stride, int64_t row0, int32_t step, float* loss_out, void* stream);
int mpo_tc_eval_step(void* handle, const float* x, const int32_t* labels, const int32_t* order,
                     int64_t order_stride, int64_t row0, float* loss_sum, int32_t* correct, void* stream);

/* k-fold index gather: out[r][:] = X[idx[r]][:] (the fold split
 * that mpi_learn does with per-fold communicators becomes an index gather). */
int mpo_kfold_gather(const float* X, const int32_t* idx, int64_t rows, int row_elems, float* out,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPO_H_ */
