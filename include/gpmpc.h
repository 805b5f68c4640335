/* gpmpc.h -- C ABI of libgpmpc_hip.so: the MI355X (gfx950) GP-regression inner loop of GP-MPC.
 *
 * The reference (helgeanl/GP-MPC) is pure Python and has no FFI layer; its de-facto operator API
 * for this path is the `GP` object as `mpc_class.MPC` uses it.  Each entry
 * point below names the reference code it replaces (file:line into /root/reference/gp_mpc/).
 * `INTEGRATION.md` shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C symbols, no exceptions cross the boundary; every function returns an int status
 *     (GPMPC_OK = 0, < 0 error; text via gpmpc_last_error()).
 *   - all arrays are C-contiguous IEEE fp64 (numpy default), row-major; the caller owns every
 *     buffer.  By default array arguments are HOST pointers (copied in/out on the handle's
 *     stream); gpmpc_set_pointer_mode(h, GPMPC_PTR_DEVICE) makes the bulk arguments of the
 *     predict family device pointers (inputs already resident in HBM, no PCIe in the call).
 *   - hyper[a] = [ell_1 .. ell_d, sf, sn], sf and sn are STANDARD DEVIATIONS
 *     (gp_functions.py:129-130, optimize.py:338-340).  Z rows are z = [x, u] in the GP's own
 *     (standardised) input units; standardisation stays in the Python host class like
 *     gp_class.py:253-261.
 *   - one handle = one GP model = one HIP stream.  Calls on different handles are thread-safe (the
 *     factorisations of different handles on one device take turns, see gpmpc_get_counter), calls on
 *     one handle are serialised by the caller.
 */
#ifndef GPMPC_H
#define GPMPC_H

#ifdef __cplusplus
extern "C" {
#endif

#define GPMPC_ABI_VERSION 2   /* 2 (r04): + gpmpc_profile_set_mask, gpmpc_runtime_info, gpmpc_schedule_stats; gpmpc_profile_enable: nonzero = all phases again */

/* status codes */
#define GPMPC_OK 0
#define GPMPC_EINVAL (-1)  /* bad argument */
#define GPMPC_EHIP (-2)    /* HIP runtime error / no usable gfx950 device */
#define GPMPC_ENOTFIT (-3) /* model has no factors yet (call gpmpc_fit / gpmpc_set_factors) */
#define GPMPC_ENOTPD (-4)  /* K not positive definite even after the one-shot 1e-8 jitter */
#define GPMPC_ENOMEM (-5)

/* uncertainty-propagation methods: the strings of GP.set_method, gp_class.py:193-242 */
#define GPMPC_ME 0     /* 'ME'     gp_class.py:212-215: [mean(z), diag(var(z))]            */
#define GPMPC_TA 1     /* 'TA'     gp_class.py:216-219: diag(var) + J Sigma J^T            */
#define GPMPC_EM 2     /* 'EM'     gp_class.py:220-224: gp_exact_moment                    */
#define GPMPC_OLD_ME 3 /* 'old_ME' gp_class.py:225-229: gp()                               */
#define GPMPC_OLD_TA 4 /* 'old_TA' gp_class.py:230-235: gp_taylor_approx(diag=True)        */

/* prior mean functions: the strings of get_mean_function, gp_functions.py:25-69.  With a mean function set, a hyper
 * row is [ell_1..ell_d, sf, sn, mean parameters] (train_gp optimize.py:136-151): */
#define GPMPC_MEAN_ZERO 0       /* 'zero'        m(x) = 0                        no parameters          */
#define GPMPC_MEAN_CONST 1      /* 'const'       m(x) = c                        [c]                    */
#define GPMPC_MEAN_LINEAR 2     /* 'linear'      m(x) = a^T x + c                [a_1..a_d, c]          */
#define GPMPC_MEAN_POLYNOMIAL 3 /* 'polynomial'  m(x) = a^T x^2 + b^T x + c      [a_1..a_d, b_1..b_d, c] */

#define GPMPC_PTR_HOST 0
#define GPMPC_PTR_DEVICE 1

/* profiling phases for gpmpc_profile_read */
#define GPMPC_PH_GRAM 0       /* SE-ARD K build                              */
#define GPMPC_PH_FACTOR 1     /* Cholesky + triangular inverse recursion     */
#define GPMPC_PH_SOLVE 2      /* w = L^-1 y, alpha = L^-T w                  */
#define GPMPC_PH_INVK 3       /* K^-1 = L^-T L^-1                            */
#define GPMPC_PH_CROSSCOV 4   /* ks(X, Z) + mean                             */
#define GPMPC_PH_VARGEMM 5    /* V = L^-1 Ks, column sums of squares (MFMA)  */
#define GPMPC_PH_FINISH 6     /* var / Jacobian / TA covariance assembly     */
#define GPMPC_PH_EM 7         /* exact-moment N x N pair tiles               */
#define GPMPC_PH_NLL 8        /* NLL reductions + gradient pass              */
#define GPMPC_PH_CHAIN 9      /* the persistent chain kernel alone = the Cholesky without the inverse (inside FACTOR) */
#define GPMPC_PH_MC 10        /* Monte Carlo roll-out: particle init, hand-over and moment kernels (not its predictions) */
#define GPMPC_PH_COUNT 11

typedef struct gpmpc_gp gpmpc_gp; /* opaque model handle */

/* ---- library / device -------------------------------------------------------------------- */
int gpmpc_abi_version(void);
const char* gpmpc_last_error(void); /* thread-local text of the last failing call */
int gpmpc_device_count(int* count);
int gpmpc_device_name(int device, char* buf, int buflen);
/* fp64 MFMA self-test: verifies the v_mfma_f64_16x16x4_f64 fragment layout the kernels assume
 * (layout_out: 0 = row=(lane>>4)+4r documented for gfx950, 1 = row=4(lane>>4)+r) and measures the
 * issue-bound rate of the instruction (TFLOP/s over the whole chip; the fp64 roofline "peak"). */
int gpmpc_mfma_selftest(int device, int* layout_out, double* tflops_out);

/* ---- model life cycle -------------------------------------------------------------------- */
/* Copies X[N x d] and Y[N x Ny] to the device (the GP owns its data, gp_class.py:29-35). */
int gpmpc_create(int device, int N, int d, int Ny, const double* X, const double* Y, gpmpc_gp** out);
int gpmpc_destroy(gpmpc_gp* h);
/* (N, d, Ny); GP.get_size gp_class.py:266-274 derives (N, Ny, Nu = d - Ny) from these. */
int gpmpc_get_size(const gpmpc_gp* h, int* N, int* d, int* Ny);
/* Prior mean function of the model (get_mean_function gp_functions.py:25-69; train_gp optimize.py:100-294 is the
 * reference path that trains with one).  alpha and the NLL are then formed from y - m(X) (optimize.py:75,96,285), and
 * every hyper array of this API -- gpmpc_fit, gpmpc_get_factors, gpmpc_set_factors, gpmpc_nll (and its gradient) -- has
 * rows of gpmpc_hyper_width() = d + 2 + #parameters entries.  add_to_prediction != 0 adds m(z) to the predicted mean and
 * its derivatives, i.e. build_gp(..., meanFunc=kind) gp_functions.py:131,135; 0 reproduces GP.__init__, which calls
 * build_gp WITHOUT meanFunc (gp_class.py:68-71), so the reference's GP object predicts ks^T alpha only.  'EM' and
 * 'old_ME' ignore the mean function like the reference (gp_functions.py:383,232); 'old_TA' with one is refused (the
 * reference raises there, gp_functions.py:309-311).  Changing the kind discards the factors. */
int gpmpc_set_mean_func(gpmpc_gp* h, int kind, int add_to_prediction);
int gpmpc_hyper_width(const gpmpc_gp* h, int* width);
/* Gaussian hyper-priors of calc_NLL (optimize.py:77-93; unused by the reference itself, prior = None :157):
 * prior6 = [ell_mean, ell_std, sf_mean, sf_std, sn_mean, sn_std]; gpmpc_nll then returns NLL + log_prior exactly as
 * :97 does (log-densities of every ell_i, of sf^2 and of sn^2, ADDED to the negative log-likelihood), and its gradient
 * follows.  NULL switches the priors off. */
int gpmpc_set_hyper_prior(gpmpc_gp* h, const double* prior6);
int gpmpc_set_pointer_mode(gpmpc_gp* h, int mode);
int gpmpc_set_stream(gpmpc_gp* h, void* hip_stream); /* NULL restores the handle's own stream */
int gpmpc_synchronize(gpmpc_gp* h);
/* Diagnostics of the factorisation path.  The fit runs its sequential chain and its bulk in persistent kernels that hand
 * tiles over through flags and must be co-resident; on a GPU shared with other work a hand-off can time out (~30 ms),
 * in which case THAT factorisation is repeated on the single-queue path (same result) and the next call tries again;
 * after three consecutive time-outs the handle stays on the single-queue path for 64 fits.  Handles of one process
 * take turns for the factorisation itself.  Counters: "handoff_timeouts", "chained_factorisations",
 * "single_queue_factorisations", "predictions_behind_tail" (see gpmpc_fit), "fused_fit_predicts" (gpmpc_fit_predict_mean_var calls that took the fused route), "persistent_variance_products" (variance products
 * of gpmpc_predict_mean_var that ran as one persistent launch over a static tile schedule, vargemm_persist.hpp); process-wide: "workspace_blocks_fresh" / "workspace_blocks_reused" (the N x N blocks
 * of a workspace, >= 64 MB, come from size classes and return to a free list: gpmpc_append at large N re-uses what the
 * previous append gave back instead of paying for fresh multi-GB allocations). */
int gpmpc_get_counter(gpmpc_gp* h, const char* name, long* value);
/* HIP-event brackets per phase on the handle's stream.  enable: 0 off, nonzero on.  gpmpc_profile_set_mask restricts the
 * brackets to the phases whose bit (the GPMPC_PH_* index) is set (0 = all) -- each bracket is two timing events, ~5 us of the
 * stream's time: with all seven phases of a fit + predict step bracketed the step takes 65 us longer at N = 4096 (r03). */
int gpmpc_profile_enable(gpmpc_gp* h, int enable);
int gpmpc_profile_set_mask(gpmpc_gp* h, unsigned mask);
int gpmpc_profile_read(gpmpc_gp* h, int phase, double* total_ms, long* launches, int reset);

/* ---- fit: a1,a3-a6 ----------------------------------------------------------------------- */
/* K_a = k_a(X,X) + sn_a^2 I (optimize.py:303-319,343-344), L = chol(K) with the one-shot jitter
 * rule (optimize.py:345-350, :483-488; gp_class.py:524-529): info[a] = 0 ok, 1 = 1e-8*I was added
 * once, and the call returns GPMPC_ENOTPD (info[a] = -(first bad pivot index, 1-based)) if that
 * also fails.  alpha = K^-1 y (optimize.py:494), and if want_invK: K^-1 (optimize.py:489-490).
 * hyper is [Ny x gpmpc_hyper_width()] (= d+2 for the zero mean); info may be NULL.
 * The call returns when `info` is known -- with the persistent-kernel factorisation that is when L is complete; the
 * last rows of L^-1 and alpha may still be in flight, and everything this API does afterwards is ordered behind them.
 * The first gpmpc_predict_mean_var with more than 64 points behind a fit (device pointers, the handle's own stream)
 * uses that window: its cross-covariances are formed on a second queue while the last row panel of L^-1 is inverted,
 * its mean next to the variance product (counter "predictions_behind_tail"; same results as any later call). */
int gpmpc_fit(gpmpc_gp* h, const double* hyper, int want_invK, int* info);
/* gpmpc_fit followed by gpmpc_predict_mean_var in ONE call (r06; same arguments, same results bit for bit).  What a caller
 * that refits and then evaluates a batch does in two calls -- GP.optimize / update_data_all followed by validate or a
 * prediction sweep, gp_class.py:131-142,145-190,474-550 -- leaves the device idle between them (the host learns `info`,
 * returns, calls again: ~0.12 ms at N = 4096) and can start the prediction's cross-covariances only then, although they
 * depend on hyper and Z alone.  With device pointers, the handle's own stream, no K^-1, a zero prior mean and 64 < B <=
 * one scratch chunk the prediction's launches are enqueued before the host waits for `info` (the cross-covariances start
 * at the end of the factorisation's chain kernel, next to the tail of L^-1); in every other case this IS the two calls.
 * If the factorisation has to be repeated (jitter rule, hand-off time-out) the prediction is repeated behind it.
 * Measured at N = 4096, B = 10 000: within 10 us of the two calls -- the step behind the chain is bound by the inverse's
 * tail, not by the host (docs/history_r06.md).
 * Counter "fused_fit_predicts". */
int gpmpc_fit_predict_mean_var(gpmpc_gp* h, const double* hyper, int want_invK, int* info, int B, const double* Z,
                               double* mean, double* var);
/* Export in the reference's save_model layout (gp_class.py:693-704): hyper[Ny x gpmpc_hyper_width()],
 * chol[Ny x N x N] (lower, zeros above), alpha[Ny x N], invK[Ny x N x N]; any pointer may be NULL. */
int gpmpc_get_factors(gpmpc_gp* h, double* hyper, double* chol, double* alpha, double* invK);
/* Append n training points and update L, L^-1, alpha with the EXISTING hyper-parameters: the result of
 * GP.update_data_all (gp_class.py:474-550, which recomputes everything from scratch) as a rank-n extension of
 * the factors, O(N^2 n) instead of O(N^3).  info[Ny]: 0 ok, <0 = -(first non-positive pivot); on
 * GPMPC_ENOTPD the model is left unchanged.  Large n (more than a quarter of the new size) refits instead. */
int gpmpc_append(gpmpc_gp* h, int n, const double* Xnew, const double* Ynew, int* info);
/* Greedy max-variance selection among n candidates, then gpmpc_append of the chosen rows: what GP.update_data
 * (gp_class.py:384-471) set out to do -- from n fresh observations keep the N_new most informative ones -- with an arg-MAX
 * (the reference takes argmin, :421) and the squared norm (it takes the norm, :443).  Xcand[n x d], Ycand[n x Ny]: HOST
 * pointers in standardised units, whatever the pointer mode.  1 <= k <= n <= the single-chunk limit of gpmpc_covar.
 * Step t = 0, 1, ...: score_j = sum_a var_a(x_j | training data + the t points picked so far) for every candidate not yet
 * picked, var_a = the noise-free predictive variance sf_a^2 - |L^-1 ks|^2 (the diagonal of gpmpc_covar) with the stored
 * hyper-parameters; the pick is the candidate with the largest score, the lowest index among equal scores.  A picked point
 * enters the model with its noise (k(x, x) + sn^2 [+ the stored jitter], gp_class.py:440); the scores stay noise-free.  If the
 * best score is < min_gain the selection stops before that pick (min_gain <= 0: never; NaN: GPMPC_EINVAL).
 * selected[k], gain[k] (the pick's score when it was picked; may be NULL) and *k_out (may be NULL) describe the first k_out
 * picks.  Unless Ycand == NULL those rows are then appended in pick order: the model is bit for bit the one
 * gpmpc_append(h, k_out, Xcand[selected], Ycand[selected], info) gives, GPMPC_ENOTPD included (model unchanged; selected / gain /
 * k_out stay valid).  k_out == 0 leaves the model untouched and returns GPMPC_OK.  Ycand == NULL: selection only (experiment
 * design: where to measure before any y exists) -- data, factors and N are unchanged.
 * Work: the candidates' posterior covariance once (O(n^2 N), the GEMMs of gpmpc_covar), then k steps of a jointly pivoted
 * partial Cholesky of it (O(Ny n t) each, select_kernels.hpp) that never touch the N x N factors, then one append.
 * GPMPC_ENOTFIT without factors; GPMPC_EINVAL for bad sizes or NULLs (the handle stays usable). */
int gpmpc_append_select(gpmpc_gp* h, int n, const double* Xcand, const double* Ycand, int k, double min_gain,
                        int* selected, double* gain, int* k_out, int* info);
/* Remove n training points and update L, L^-1, alpha with the EXISTING hyper-parameters and the stored jitter: the model
 * that gpmpc_fit gives on the remaining points (kept in their original order), to rounding, in O(N^2 n) instead of O(N^3).
 * The reference can only replace all the data (GP.replace_data_all, gp_class.py:553-626: a full recomputation); together with
 * gpmpc_append this keeps an online model at a fixed size.  idx[n]: HOST array of distinct indices in [0, N), any order,
 * 1 <= n < N (at least one point stays).  GPMPC_EINVAL for duplicates, indices out of range, n <= 0, n >= N, NULL handle or
 * idx (the handle stays usable, the model untouched); GPMPC_ENOTFIT without factors.  X, Y, N and the padded size follow; alpha
 * is recomputed from the new L^-1 (stored mean parameters included), K^-1 is rebuilt lazily, as after gpmpc_append.  The new
 * buffers are built beside the old ones and installed at the end: a HIP or allocation failure leaves the model unchanged.  A
 * principal submatrix of a positive-definite matrix is positive definite: there is no `info` and no GPMPC_ENOTPD on the downdate.
 * Method (remove_kernels.hpp): one Householder reflector per kept column from the first removed index on maps [L[S,S] L[S,R]] to
 * [L' 0] and, from the left, [L^-1[S,S]; L^-1[R,S]] to L'^-1; 64 removed points per pass, two launches per 64-column panel;
 * trailing indices leave the leading blocks of L and L^-1 bit for bit.  Where that cannot pay (small N, many points) the call
 * refits on the remaining rows instead, with gpmpc_append's rollback; gpmpc_set_tuning("remove_mode", 0 automatic / 1 always
 * downdate / 2 always refit / -1 default) overrides the choice, counters "remove_downdates" / "remove_refits" tell which ran. */
int gpmpc_remove(gpmpc_gp* h, int n, const int* idx);

/* FITC sparse model (what GP.sparse, gp_class.py:681-689, names and leaves empty: "Use Fully Independent Training Conditional
 * (FITC) ... reduce the model size from N to M"): from the N training points of `h` and M inducing points Xu[M x d] (HOST
 * pointer, standardised units, 1 <= M <= N) a NEW handle *out of size (M, d, Ny) on h's device; `h` is untouched.
 * hyper[Ny x (d+2)]: the hyper-parameters to build with; `h` then needs no factors and the call allocates nothing of size
 * N x N (gpmpc_create does not either: the N x N blocks of a handle come with its first fit / import), so a source may hold
 * far more points than an exact fit can factor.  hyper == NULL: the ones stored on `h` (GPMPC_ENOTFIT without factors).
 * The source's prior mean must be 'zero' (GPMPC_EINVAL otherwise).  Per output a with (ell, sf, sn):
 *   Kuu = k(Xu,Xu) + 1e-6 sf^2 I (GPML's inducing jitter), Luu = chol(Kuu) -- info[a] follows the rule of gpmpc_fit (may be NULL);
 *   V = Luu^-1 k(Xu,X);  lambda_i = max(sf^2 - sum_m V_mi^2, 0) + sn^2;  Vs = V Lambda^-1/2;  B = I + Vs Vs^T;  r = Vs Lambda^-1/2 y;
 *   alpha_u = Luu^-T B^-1 r;  P = Luu^-T (I - B^-1) Luu^-1  (= Kuu^-1 - Sigma^-1, Quinonero-Candela & Rasmussen 2005 eq. 24).
 * The FITC predictor mean = k(z,Xu) alpha_u, var = sf^2 - k(z,Xu) P k(Xu,z) has the form of an exact GP on the inducing points
 * with K^-1 -> P, and so have the exact-moment formulas (as in PILCO).  The new handle therefore carries X = Xu, the given
 * hyper rows, alpha = alpha_u, K^-1 = P, L^-1 = W and L = W^-1 for the lower triangular W with W^T W = P (the Cholesky factor of
 * the index-reversed P, transposed and reversed back), Y = Yu = L L^T alpha_u, stored jitter 0 -- and EVERY entry point that
 * predicts (the predict family, sensitivities, gpmpc_covar, all five methods, the roll-outs) evaluates FITC on it unchanged;
 * gpmpc_get_factors exports it in the reference's save_model layout.  A Cholesky of B or of the reversed P that fails:
 * GPMPC_ENOTPD, info[a] = -(pivot), *out = NULL; every other error leaves *out = NULL and `h` usable as well.
 * The sparse handle is predict-only: gpmpc_fit, gpmpc_fit_predict_mean_var, gpmpc_append, gpmpc_append_select, gpmpc_remove,
 * gpmpc_nll, gpmpc_train_multistart, gpmpc_set_mean_func and gpmpc_set_factors return GPMPC_EINVAL on it (the handle stays
 * usable); it cannot be the source of another gpmpc_sparse_fitc.
 * Work: the training points are visited in chunks of the predict family's size (gpmpc_set_tuning "predict_chunk"); per chunk
 * the cross-covariances, one product with Luu^-1 and the symmetric rank update B += Vs Vs^T on the fp64 matrix cores
 * (fitc_kernels.hpp): O(N M^2); then an O(M^3) tail.  Nothing N-sized goes to the host.  The new handle inherits the
 * source's profiling switch and mask; its GPMPC_PH_GRAM / _FACTOR brackets then hold the fit of Kuu, GPMPC_PH_VARGEMM the
 * rank updates. */
int gpmpc_sparse_fitc(gpmpc_gp* h, const double* hyper, int M, const double* Xu, int* info, gpmpc_gp** out);

/* Import a saved model (GP.load_model -> ctor branch gp_class.py:58-66): chol and hyper are
 * required; alpha == NULL recomputes it from Y; invK == NULL computes it lazily when a method
 * needs it.  L^-1 (the predict operand) is rebuilt on the device. */
int gpmpc_set_factors(gpmpc_gp* h, const double* hyper, const double* chol, const double* alpha,
                      const double* invK);

/* ---- predict: a9-a13 --------------------------------------------------------------------- */
/* mean[B x Ny], var[B x Ny]: build_gp's mean/var functions, gp_functions.py:114-136
 * (mean = ks^T alpha, var = sf^2 - ||L^-1 ks||^2, no noise term). */
int gpmpc_predict_mean_var(gpmpc_gp* h, int B, const double* Z, double* mean, double* var);
/* mean[B x Ny] and J[B x Ny x d] = d mean / d z: mean_jac_z gp_functions.py:146-147 (CasADi AD
 * there, analytic here); the operand of GP.discrete_linearize / jacobian gp_class.py:647-672. */
int gpmpc_mean_jac(gpmpc_gp* h, int B, const double* Z, double* mean, double* J);
/* Derivative outputs for a casadi Callback around GP.__predict (the reference obtains them
 * from CasADi's AD of build_gp / build_TA_cov, gp_functions.py:114-173): besides mean[B x Ny], var[B x Ny]
 * and J[B x Ny x d] = d mean/dz also Hm[B x Ny x d x d] = d2 mean/dz2 and dvar[B x Ny x d] = d var/dz, from
 * which d cov/dz and d cov/dSigma of the 'ME' and 'TA' methods follow in closed form
 * (cov = diag(var) + J Sigma J^T).  Any output pointer may be NULL.  d var/dz needs K^-1 ks: formed as
 * L^-T (L^-1 ks) from the factor the variance already uses, so the call neither needs nor builds K^-1. */
int gpmpc_predict_sens(gpmpc_gp* h, int B, const double* Z, double* mean, double* var, double* J,
                       double* Hm, double* dvar);
/* 'EM' (gp_exact_moment gp_functions.py:344-418) with its first derivatives: besides mean[B x Ny] and cov[B x Ny x Ny]
 * the Jacobians dmean_dz[B x Ny x d], dmean_dS[B x Ny x d x d], dcov_dz[B x Ny x Ny x d], dcov_dS[B x Ny x Ny x d x d]
 * with respect to the input mean z and the d x d entries of the input covariance (entries independent, as in CasADi's
 * jacobian(..., covar_s) which the reference relies on inside IPOPT).  Sigma must be symmetric: like gpmpc_predict's
 * 'EM' value path, which visits each pair (i, j) of training points once, the formulas use Sigma = Sigma^T.  Any output
 * may be NULL; with cov == NULL the value kernels' pair sums are not formed (a Jacobian callback: 3.9 instead of 5.6 ms
 * per input at N = 8192, Ny = 6).  Every d the library takes (<= 16): d <= 8 on an 8-deep, d = 9..16 on a 16-deep cross term. */
int gpmpc_predict_em_sens(gpmpc_gp* h, int B, const double* Z, const double* Sigma, double* mean, double* cov,
                          double* dmean_dz, double* dmean_dS, double* dcov_dz, double* dcov_dS);
/* GP.__predict (gp_class.py:212-235) batched over B input distributions:
 * Z[B x d], Sigma[B x d x d] (ignored for ME/old_ME, may be NULL) -> mean[B x Ny],
 * cov[B x Ny x Ny] in standardised units (gp_class.py:262 leaves cov unscaled). */
int gpmpc_predict(gpmpc_gp* h, int method, int B, const double* Z, const double* Sigma,
                  double* mean, double* cov);
/* gpmpc_predict for 'ME' / 'TA' plus J[B x Ny x d] = d mean / d z from the same pass (what one evaluation of an NLP
 * callback needs: GP.__predict and its jac_x / jac_u, gp_class.py:212-219,239-242). */
int gpmpc_predict_jac(gpmpc_gp* h, int method, int B, const double* Z, const double* Sigma, double* mean,
                      double* cov, double* J);
/* a17: T-step uncertainty propagation entirely on the device (the numeric loop of GP.predict_compare,
 * gp_class.py:777-804: feed (mean_t, cov_t) back into GP.predict), one synchronisation at the end instead of
 * one per step.  All quantities in the GP's standardised units: z0[d] first input, U[T x Nu] controls,
 * Sigma0[d x d] initial input covariance (its [:Ny,:Ny] block is replaced by cov_t every step, the rest kept),
 * sa/sb[Ny]: x_{t+1} = sa * mean_t + sb maps an output mean to the next state input (re-standardisation of
 * GP.predict, gp_class.py:253-261; NULL = identity).  Outputs mean[T x Ny], cov[T x Ny x Ny] (host pointers). */
int gpmpc_rollout(gpmpc_gp* h, int method, int T, const double* z0, const double* U, const double* Sigma0,
                  const double* sa, const double* sb, double* mean, double* cov);
/* The same loop with the reference's state feedback (predict_compare(feedback=True), gp_class.py:772-803):
 * u_t = K (mean_{t-1} - x_ref) and the input covariance [[C, C K^T], [K C, K C K^T]], C = cov_{t-1}.  The caller
 * supplies the gain as data (the reference computes K with mpc_class.lqr from discrete_linearize at (x0, u_0)):
 * Kz[Nu x Ny], k0[Nu]: u_t in the GP's input units as an affine function of the STANDARDISED output mean
 * (u_t = Kz mean_{t-1} + k0: GP.predict's un-/re-standardisation folded in); Kc[Nu x Ny]: the gain applied to the
 * covariance blocks (the reference applies the raw K to the standardised cov, :798-799).  z0 = [x_0, u_0] carries
 * the first control.  U_out[T x Nu] (may be NULL) returns the controls that were applied. */
int gpmpc_rollout_feedback(gpmpc_gp* h, int method, int T, const double* z0, const double* Sigma0, const double* sa,
                           const double* sb, const double* Kz, const double* k0, const double* Kc, double* mean,
                           double* cov, double* U_out);
/* M roll-outs in lock-step (r06; SURVEY a17 "batch across trajectories / methods": gp_class.py:777-804 runs the methods one
 * after the other and synchronises with the predictor at every step).  Trajectory m has its own method methods[m], first
 * input z0[m] (z0[M x d]), controls U[m] (U[M x T x Nu]) and initial input covariance Sigma0[m] (Sigma0[M x d x d]); sa / sb
 * as in gpmpc_rollout.  Outputs mean[M x T x Ny], cov[M x T x Ny x Ny].  Per time step ONE pass over the factors serves
 * every trajectory: all 'ME' / 'TA' trajectories form one prediction batch (the lower triangles of L^-1 are streamed once
 * for up to 32 of them -- at N = 8192, Ny = 6 that stream IS the step: 1.6 GB), the trajectories of a moment method
 * one batched launch set.  M <= 64.  Open loop only (gpmpc_rollout_multi_feedback for the reference's feedback law).
 * Parity: trajectories do not influence each other; a trajectory's numbers are bitwise those of gpmpc_rollout when it
 * is the only 'ME' / 'TA' trajectory of the call (or a moment method), and otherwise agree with it to rounding (the
 * batched variance kernel sums the same N terms in another order than the one-column kernel: ~1e-15 sf^2 per step). */
int gpmpc_rollout_multi(gpmpc_gp* h, int M, const int* methods, int T, const double* z0, const double* U,
                        const double* Sigma0, const double* sa, const double* sb, double* mean, double* cov);
/* gpmpc_rollout_multi with per-trajectory state feedback: closed-loop roll-outs in lock-step.  Trajectory m with
 * closed[m] != 0 (closed == NULL: every trajectory) follows the reference's closed-loop propagation
 * (predict_compare(feedback=True), gp_class.py:787-804: u_t = K (mean_{t-1} - x_ref), input covariance
 * [[C, C K^T], [K C, K C K^T]]) exactly as gpmpc_rollout_feedback runs it, with its own gains Kz[m] (Kz[M x Nu x Ny]),
 * k0[m] (k0[M x Nu]) and Kc[m] (Kc[M x Nu x Ny]): Kz / k0 act on the standardised output mean and give u_t in the GP's
 * input units, Kc acts on the covariance blocks, the state block of Sigma is replaced by cov_{t-1} every step; its first
 * control comes with z0[m] = [x_0, u_0].  Trajectory m with closed[m] == 0 is an open-loop trajectory of
 * gpmpc_rollout_multi with the controls U[m] (U[M x T x Nu]); its rows of Kz / k0 / Kc are ignored, as are the rows of U
 * of a closed trajectory.  U may be NULL when no trajectory is open, the gains when none is closed.  U_out[M x T x Nu]
 * (may be NULL) returns the controls that were applied (the given ones for an open trajectory).  Host pointers, M <= 64,
 * all five method codes.  GPMPC_EINVAL: the rules of gpmpc_rollout_multi, and a closed trajectory with Nu = 0 or with a
 * NULL gain, an open one with U == NULL (Nu > 0).
 * Per time step the work is gpmpc_rollout_multi's: all 'ME' / 'TA' trajectories, closed and open, form one prediction
 * batch (ONE stream of L^-1 instead of one per trajectory), the moment-method trajectories one batched launch set; only
 * the hand-over between two steps differs.  The gains travel in the same upload as z0 / Sigma0 / U.
 * Parity: a call with one closed trajectory gives the bits of gpmpc_rollout_feedback, a call without a closed one the bits
 * of gpmpc_rollout_multi; a moment-method trajectory always has the bits of its single call, an 'ME' / 'TA' trajectory next
 * to another one agrees with its single call to rounding (gpmpc_rollout_multi's note); among calls with 2..32 'ME' / 'TA'
 * trajectories its bits do not depend on its position or on what else is in the call (a wider batch takes another
 * variance kernel: rounding again). */
int gpmpc_rollout_multi_feedback(gpmpc_gp* h, int M, const int* methods, int T, const double* z0, const double* Sigma0,
                                 const double* sa, const double* sb, const int* closed, const double* Kz,
                                 const double* k0, const double* Kc, const double* U, double* mean, double* cov,
                                 double* U_out);
/* Monte Carlo roll-out: S particles propagated through the GP for T steps on the device -- what the GP itself predicts for
 * the propagated distribution, next to the moment-matching methods above, which collapse it to a Gaussian at every step
 * (no reference counterpart; predict_compare, gp_class.py:746-861, compares them with one simulated trajectory only).
 * Host pointers, standardised units; z0[d], Sigma0[d x d], U[T x Nu], sa / sb[Ny], Kz[Nu x Ny], k0[Nu] exactly as in
 * gpmpc_rollout / gpmpc_rollout_feedback.  Particle s starts at z_s = z0 + L0 eps0_s, L0 a lower-triangular factor of
 * Sigma0 formed on the host (a semidefinite Sigma0 is fine: a pivot below d eps max(diag) gives a zero column; an
 * indefinite one is GPMPC_EINVAL).  Step t: (m_s, v_s) = gpmpc_predict_mean_var at z_s for all S particles (in chunks of the
 * predict family's size, gpmpc_set_tuning "predict_chunk"), then
 *   y_s = m_s + sqrt(max(v_s, 0) + noise sn^2) eps_{t,s}      (noise != 0 adds the observation noise of hyper's sn)
 * and the next input z_s = [sa y_s + sb, u]: open loop u = U[t + 1] (U[0] is not read: the first control comes with z0, as
 * in gpmpc_rollout), closed loop (Kz != NULL; U is ignored) u = Kz y_s + k0 PER PARTICLE -- gpmpc_rollout_feedback's
 * convention applied to every trajectory of its own.  Outputs: mean[T x Ny] and cov[T x Ny x Ny], the sample mean and the
 * unbiased sample covariance of the S vectors y_s of each step (S = 1: cov = 0), and, unless NULL, particles[T x S x Ny].
 * The moments are reduced in two passes (mean, then centred products) over fixed blocks of 256 particles combined in a
 * fixed order, without atomics: a function of the data only.
 * Random numbers: eps0_s[d] and eps_{t,s}[Ny] are standard normals from a counter-based generator, Philox-4x32-10 with
 * key = the two halves of `seed` and counter = (row s, column pair, stream, 0), stream 0 for eps0 and 1 + t for step t;
 * the four words give two 53-bit uniforms in (0, 1], Box-Muller the normals of columns 2j (cosine) and 2j + 1 (sine):
 * gpmpc_randn returns exactly these arrays.  A value depends on (seed, stream, row, column) only -- not on S, the launch
 * geometry or the chunking -- so a call is reproducible bit for bit.  eps0[S x d] and eps[T x S x Ny] (each may be NULL)
 * REPLACE the generator: common random numbers for comparing controllers, and an exact replay; `seed` is then unused.
 * Each step draws the outputs INDEPENDENTLY given the particle's input (and independently per output): that is the
 * assumption the moment methods approximate; it is not a consistent draw of one function over the horizon.
 * DIFF: after step 0 the controls are exact.  gpmpc_rollout keeps the control block of Sigma0 in every step's input
 * covariance; here Sigma0 -- its control block included -- enters the initial particles only.
 * Everything runs on the handle's stream, one upload and one download per call, no graph capture.  A FITC handle and a
 * prior mean added to the prediction work unchanged.  GPMPC_EINVAL: the rules of gpmpc_rollout, S < 1, S > 2^20, a closed
 * loop with Nu = 0 or k0 == NULL; GPMPC_ENOTFIT without factors; the handle stays usable. */
int gpmpc_rollout_mc(gpmpc_gp* h, int S, int T, unsigned long long seed, int noise, const double* z0,
                     const double* Sigma0, const double* U, const double* sa, const double* sb, const double* Kz,
                     const double* k0, const double* eps0, const double* eps, double* mean, double* cov, double* particles);
/* out[rows x cols] (HOST pointer): the standard normals of gpmpc_rollout_mc's generator at (seed, stream, row, column). */
int gpmpc_randn(int device, unsigned long long seed, unsigned stream, int rows, int cols, double* out);

/* ---- pathwise posterior samples: consistent Monte Carlo roll-outs -------------------------------- */
/* S functions drawn ONCE from the posterior and then evaluated wherever a particle goes: a particle that returns to a state
 * sees the same dynamics there, which gpmpc_rollout_mc's independent per-step draws do not give.  Pathwise conditioning
 * (Matheron's rule) with a random-feature prior (Wilson, Borovitskiy, Terenin, Mostowsky, Deisenroth: "Efficiently sampling
 * functions from Gaussian process posteriors", ICML 2020), per output a with hyper row (ell, sf, sn), standardised units:
 *   frequencies  omega_j = eps_j / ell (elementwise), eps_j ~ N(0, I_d), j < F / 2, shared by all paths;
 *   features     phi_2j(z) = c cos(omega_j . z), phi_2j+1(z) = c sin(omega_j . z), c = sf sqrt(2 / F)   (E[phi(z) . phi(z')] = k(z, z'));
 *   per path s   w_s ~ N(0, I_F), xi_s ~ N(0, I_N),  v_s = alpha - K^-1 (Phi w_s + sn xi_s),  Phi = phi(X) [N x F],  K^-1 r = L^-T (L^-1 r);
 *   the path     f_s(z) = m(z) + phi(z) . w_s + sum_i v_s,i k(z, x_i)
 * with the prior mean m added exactly when the handle adds it to a prediction: w = 0, xi = 0 gives gpmpc_predict_mean_var's
 * mean.  Exact given the frequencies: the data term; approximate: the prior, by its F features ("Pathwise samples",
 * has the closed-form covariance of f_s - mean for a given omega and how it approaches the posterior covariance with F).
 * Random streams of gpmpc_randn's generator, a value depending on (seed, stream, row, column) only: */
#define GPMPC_PATHS_STREAM_OMEGA 0x40000000u   /* + a: eps_a, row j, d columns  */
#define GPMPC_PATHS_STREAM_W 0x50000000u       /* + a: w_a, row s, F columns    */
#define GPMPC_PATHS_STREAM_XI 0x60000000u      /* + a: xi_a, row s, N columns   */
/* (streams 0 and 1 + t keep their roll-out meaning).  Host pointers throughout, everything on the handle's stream.
 * gpmpc_paths_draw: draws S paths of F features (F even, the same for all outputs); eps_omega[Ny x F/2 x d], w[Ny x S x F],
 * xi[Ny x S x N] (each may be NULL) REPLACE the generator per array.  Cost: the features, then per output the products
 * Phi W^T, L^-1 R and L^-T T1 on the fp64 matrix cores, O(N (F + N) S).  The paths live on the handle in grow-only device
 * buffers: Ny Np S doubles of weights (S rounded up to even; Np = N rounded up to 64), Ny F S of feature weights; scratch of
 * the setup is released before the call returns.  They are released by gpmpc_paths_free (with the staging of the eval / roll-out
 * calls) / gpmpc_destroy, and every call that
 * changes or drops the factors or the data (gpmpc_fit, gpmpc_fit_predict_mean_var, gpmpc_append*, gpmpc_remove,
 * gpmpc_set_factors, gpmpc_set_mean_func, gpmpc_train_multistart) makes them STALE: the calls below then return
 * GPMPC_EINVAL until paths are drawn again.  GPMPC_EINVAL: S outside 1 .. 2^20, F odd, < 2 or > 65536, a FITC handle (a sample
 * of its predictor is another construction); GPMPC_ENOTFIT without factors; after these the handle stays usable and earlier
 * paths stay valid.  GPMPC_ENOMEM: a device allocation failed; earlier paths stay valid unless
 * one of their own buffers had to grow for this call. */
int gpmpc_paths_draw(gpmpc_gp* h, int S, int F, unsigned long long seed, const double* eps_omega, const double* w,
                     const double* xi);
/* What was drawn (any pointer may be NULL): S, F, omega[Ny x F/2 x d] (already divided by ell), w[Ny x S x F], v[Ny x S x N]. */
int gpmpc_paths_get(gpmpc_gp* h, int* S, int* F, double* omega, double* w, double* v);
/* f[S x Ny]: path s at its own input Z[s] (Z[S x d]).  One pass over the weights: the training points are cut into fixed
 * blocks of 128 and the frequencies into blocks of 16, partial sums per (block, path, output) are added in a fixed order:
 * the result is a function of the data only. */
int gpmpc_paths_eval(gpmpc_gp* h, const double* Z, double* f);
/* f[S x B x Ny]: all paths at the common points Z[B x d] (Thompson-sampling draws, plots): cross-covariances and two
 * matrix products, in chunks of the predict family's size. */
int gpmpc_paths_eval_grid(gpmpc_gp* h, int B, const double* Z, double* f);
int gpmpc_paths_free(gpmpc_gp* h);
/* gpmpc_rollout_mc with the step replaced: particle s follows path s (S is the drawn S), y_s = f_s(z_s) + noise sn eps_{t,s}
 * with eps from stream 1 + t or the caller's eps[T x S x Ny] (noise == 0 draws nothing after step 0), the initial particles
 * z_s = z0 + L0 eps0_s from stream 0 (the same `seed` gives gpmpc_rollout_mc's initial particles) or eps0[S x d]; every other
 * argument, the semidefinite Sigma0, the hand-over, the moment reduction and the outputs are gpmpc_rollout_mc's.  A step
 * reads the path weights once and forms no variance.  GPMPC_EINVAL also without valid paths. */
int gpmpc_rollout_paths(gpmpc_gp* h, int T, unsigned long long seed, int noise, const double* z0, const double* Sigma0,
                        const double* U, const double* sa, const double* sb, const double* Kz, const double* k0,
                        const double* eps0, const double* eps, double* mean, double* cov, double* particles);
/* a14 GP.covar gp_class.py:353-381: covar[Ny x n x n] = sf^2 - V^T V for n new inputs. */
int gpmpc_covar(gpmpc_gp* h, int n, const double* Xnew, double* covar);

/* ---- training objective: a7 (+ gradient) ------------------------------------------------- */
/* NLL of output `a` at hyper_row[gpmpc_hyper_width()] (calc_NLL_numpy optimize.py:322-356: 0.5 y^T alpha +
 * sum log|L_ii|, jitter rule included; with a mean function calc_NLL optimize.py:22-97 without its unused
 * hyper-priors); grad[gpmpc_hyper_width()] (may be NULL) is dNLL/dhyper, Rasmussen &
 * Williams eq. 5.9 -- the reference has no analytic gradient (optimize.py:371-375).
 * jitter_out (may be NULL) reports whether the jitter branch was taken. */
int gpmpc_nll(gpmpc_gp* h, int a, const double* hyper_row, double* nll, double* grad, int* jitter_out);

/* ---- training: a8 ------------------------------------------------------------------------------ */
/* Multistart hyper-parameter training of all Ny outputs, then the fit at the optimum: train_gp_numpy
 * optimize.py:359-503 (SLSQP + finite differences) / train_gp :100-294 (IPOPT on CasADi AD), here a projected L-BFGS on
 * gpmpc_nll and its analytic gradient, in two stages per restart: (1) length scales and sf -- if their bounds are
 * positive and finite -- in log space, the noise sn and the mean parameters linear (as in the reference's optimisers;
 * d NLL / d log sn vanishes at the reference's start sn = 1e-5, a log-space search never leaves it); (2) if stage 1 stops
 * with iterations to spare, a polish from its end point with sn in log space as well, kept when it ends lower.  An
 * accepted step always lowers the NLL; the L-BFGS memory is dropped when the set of bound-pinned variables changes.
 * optimizer_opts written for IPOPT / SLSQP have no counterpart here: only max_iter and tol exist.  Iteration and
 * evaluation totals of the last call (this rank's restarts, both stages): gpmpc_get_counter "train_iterations" /
 * "train_evaluations", and "train_gflop" = its algorithmic matrix work (N^3/3 per Cholesky, per L^-1 formed, per K^-1).
 * Which route the lock-step search of the last call took, reset by every call like the totals above:
 * "train_retained_gradients" = points whose gradient was formed from the factors a value-only batch had left behind
 * (0 when this rank's restarts do not fit one batch, and with a single restart); "train_jitter_repeats" = points that a
 * lock-step batch evaluated a second time with the 1e-8 jitter (the single-restart route reports its jitter through
 * gpmpc_nll's jitter_out and does not count here).  starts[Ny x nstart x W] (W =
 * gpmpc_hyper_width): one initial point per restart -- the reference starts every restart from the same point
 * (optimize.py:462-466, its Latin-hypercube line :218 is commented out); lb, ub[Ny x W]: the box (optimize.py:434-443 or
 * :204-229; +-HUGE_VAL for none).  For every output the restart with the smallest NLL wins (first minimum, np.argmin
 * :474), the model is fitted there (:476-494) and hyper_opt[Ny x W], obj[Ny x nstart] (+inf: restart failed),
 * theta_all[Ny x nstart x W] (may be NULL), info[Ny] (as gpmpc_fit) are returned.  max_iter <= 0 / tol <= 0 select the
 * defaults (200, 1e-8 on the projected gradient relative to |NLL|).
 * Restart shard (the only part of the path that shards, north_star): restart r is run by rank r mod world.  With an
 * RCCL communicator (gpmpc_rccl_comm_create, one rank per GPU) the ranks exchange their (NLL, theta) rows with ONE
 * ncclAllGather -- (1 + W) doubles per restart -- take the same arg-min and each fits its own copy; nothing else
 * crosses xGMI.  world > 1 with rccl_comm == NULL: no exchange and no fit; the caller merges the obj / theta_all rows
 * of the ranks (row r is valid on rank r mod world) and calls gpmpc_fit.
 * Failure of ONE rank (HIP error, out of memory) never strands the others: the rank still joins the exchange with +inf
 * rows and its error code in a status word of the same all-gather, and EVERY rank returns that code.  Without a
 * communicator the code is written to *status (may be NULL; 0 = fine) and the call returns GPMPC_OK so that the caller
 * reaches its own exchange. */
int gpmpc_train_multistart(gpmpc_gp* h, int nstart, const double* starts, const double* lb, const double* ub,
                           int max_iter, double tol, int rank, int world, void* rccl_comm, int want_invK,
                           double* hyper_opt, double* obj, double* theta_all, int* info, int* status);
/* RCCL bootstrap for the restart shard (librccl is bound at run time).  Rank 0 obtains the 128-byte id and hands it to
 * the other ranks by any side channel (a file, MPI, torch.distributed's store); every rank then creates its
 * communicator on its own GPU. */
int gpmpc_rccl_unique_id(char* id128);
int gpmpc_rccl_comm_create(int device, int world, int rank, const char* id128, void** comm_out);
int gpmpc_rccl_comm_destroy(void* comm);
/* Number of ranks the communicator spans (ncclCommCount): what bench.py reports as `rccl_ranks`. */
int gpmpc_rccl_comm_count(void* comm, int* count);
/* The HIP runtime and the RCCL build this process runs the library on, as text "hip_runtime=<version> hip_path=<file>
 * rccl=<version|unavailable> rccl_path=<file>".  The library runs on the libamdhip64 the process mapped first (PyTorch's
 * bundled copy if torch was imported before the library, /opt/rocm's otherwise) and binds, at run time, the librccl that
 * sits NEXT TO that runtime -- in a process that imported torch first that is the RCCL torch.distributed runs on. */
int gpmpc_runtime_info(char* buf, int buflen);

/* ---- low-level dense ops (host pointers), used by the parity tests ------------------------ */
/* k(X, Z)[n1 x n2] = sf2 exp(-1/2 sum_d (x_d - z_d)^2 / ell_d^2) for X[n1 x d], Z[n2 x d]: GP.covSEard
 * gp_class.py:314-350 (same expanded-form operation order, no FMA contraction). */
int gpmpc_kernel_matrix(int device, int n1, int n2, int d, const double* X, const double* Z,
                        const double* ell, double sf2, double* out);
/* In-place lower Cholesky of the n x n row-major SPD matrix A (np.linalg.cholesky,
 * optimize.py:346).  *info = 0 ok, k > 0: leading minor k is not positive definite (LAPACK dpotrf
 * convention).  Ainv (may be NULL) receives L^-1. */
int gpmpc_cholesky(int device, int n, double* A, double* Ainv, int* info);
/* C = alpha * op(A) op(B) + beta * C on the fp64 MFMA GEMM core (row-major, ld = row length).
 * transa/transb as in BLAS ('N' = 0 / 'T' = 1). */
int gpmpc_dgemm(int device, int transa, int transb, int M, int N, int K, double alpha,
                const double* A, int lda, const double* B, int ldb, double beta, double* C, int ldc);

/* The static tile schedule of the persistent products (host code only, no device needed): mode 0 = the predictive variance of
 * gp_functions.py:122-126 (tilesM x tilesN tiles of 128 x 128 per matrix, the tile in block row tm is min(K, 128 (tm + 1)) / 16
 * slabs long), mode 1 = the lower triangle of K^-1 = L^-T L^-1 (optimize.py:489-490; tiles tm >= tn, (K - 128 tm) / 16 slabs),
 * for `batch` matrices on `slots` resident workgroups dealt round-robin to 8 XCDs.  stats[0..5] = tiles, heaviest slot load,
 * mean slot load (half slabs), tiles on their operand panel's home XCD, tiles scheduled more or less than once (0 when
 * correct), longest list.  What the CPU tier checks: every tile exactly once, balance, locality. */
int gpmpc_schedule_stats(int mode, int tilesM, int tilesN, int batch, int K, int slots, double* stats);

/* Diagnostic knobs for tests and tuning runs (no reference counterpart).  "gemm_tile": 0 (automatic), 32, 64 or 128
 * pins the tile of every GEMM launch of the process, so that small problems reach the large-tile kernels.
 * "cu_count": the number of compute units of device 0 the persistent-kernel factorisation plans with (at most the
 * real count on a GPU; the emulated build accepts up to 64 so that the multi-launch worker schedules can be
 * exercised).  "fail_nll_after": n > 0 makes the n-th gpmpc_nll evaluation from now on return GPMPC_EHIP without touching
 * the device (fault injection: how the tests reach the failure paths of the restart shard); 0 switches it off.
 * "worker_courier": 1 / 0 = the tile-owner worker launches of the chained factorisation run with / without the courier
 * workgroup (two instantiations of one kernel; default 1, or GPMPC_COURIER), -1 back to the default.
 * "handoff_write_through": 1 = the tiles that cross workgroups inside the chained factorisation (chain kernel, tile-owner
 * workers, courier) leave as write-through stores followed by a drained flag (default, or GPMPC_CHAIN_WT / GPMPC_WORKER_WT),
 * 0 = plain stores and an agent-scope release (an L2 write-back) per hand-off, -1 back to the default; same results.
 * "vargemm_persist": the large-batch variance product (gp_functions.py:122-126) as 0 = one 128 x 128 tile per workgroup in
 * the dispatcher's order, 1 = one persistent launch over a static schedule when there are at least two tiles per workgroup
 * slot (default, or GPMPC_VARGEMM_PERSIST), 2 = ... at any size (tests), -1 back to the default; same bits either way.
 * "em_chunk": column tiles (64 wide) one workgroup of the exact-moment pair sums sweeps (gp_exact_moment,
 * gp_functions.py:397-414; default 64, or GPMPC_EM_CHUNK); 0 back to the default; results agree to rounding.
 * "em_diag_segs": the a == b pair sums of the same (the ones that stream K^-1): n > 0 = the lower triangle of tiles in n equal
 * ranges per pair (default: four workgroups per CU shared by the outputs, at most one per partial-sum slot; or
 * GPMPC_EM_DIAG_SEGS), 0 = by strips and chunks like the a != b pairs, -1 back to the default; results agree to rounding.
 * "predict_chunk": n = a multiple of 64 in [64, 32768] caps the points per pass of every chunk loop of the predict family
 * (gpmpc_predict_mean_var, gpmpc_mean_jac, gpmpc_predict_jac, gpmpc_predict, gpmpc_predict_sens; the single-chunk limits of
 * gpmpc_covar and of the routes next to a fit follow it), also on a handle whose scratch is already allocated; 0 back to the
 * build's own size (2e9 bytes of cross-covariances, at most 32768 points).  For tests: the multi-chunk paths at small sizes.
 * "em_sens_chunk": n >= 1 caps the inputs per pass of gpmpc_predict_em_sens (default: 512 MB of operands); 0 back to that.
 * Returns GPMPC_EINVAL for an unknown name or value. */
int gpmpc_set_tuning(const char* name, int value);

#ifdef __cplusplus
}
#endif
#endif /* GPMPC_H */
