/*
 * egx_gp.h -- C ABI of libegx_gp_hip.so: MI355X-native (gfx950) kriging hot path.
 *
 * This is the drop-in boundary for egobox-gp's fit / reduced-likelihood /
 * predict / predict_var path.  The reference (relf/egobox 0.34.0) has no FFI
 * today: its seams are Rust traits and one cargo-feature `cfg`.  Every entry
 * point below names the reference interface it replaces (paths relative to the
 * reference checkout).  A Rust `extern "C"` shim implementing those traits on
 * top of this header is shown in INTEGRATION.md.
 *
 * Conventions
 *   - all arrays are caller-owned HOST memory, f64, C-contiguous row-major
 *     (ndarray standard layout); the library owns device memory behind the
 *     opaque handle; no callbacks cross the boundary.
 *   - every function returns an egx_rc (0 = success); on failure
 *     egx_last_error() returns a thread-local message.
 *   - numerical failures of ONE likelihood evaluation are VALUES, not errors:
 *     they come back in the per-candidate `status` (egx_status), exactly as the
 *     reference swallows them into +inf during optimisation
 *     (crates/gp/src/algorithm.rs:885-896).  Only egx_gp_finalize / egx_gp_fit
 *     turn a bad status into an error return, as the reference's final
 *     `reduced_likelihood(...)?` does (algorithm.rs:968).
 *   - a handle is safe to call from several host threads (calls are
 *     serialised per handle); distinct handles are independent.
 *   - there is NO CPU fallback: without a gfx950 device egx_gp_create fails
 *     with EGX_ERR_NO_DEVICE.
 */
#ifndef EGX_GP_H
#define EGX_GP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGX_GP_ABI_VERSION 2

typedef struct egx_gp egx_gp; /* opaque: one training set resident on one GPU */

/* return codes */
typedef enum {
    EGX_SUCCESS = 0,
    EGX_ERR_INVALID_VALUE = 1, /* GpError::InvalidValueError, crates/gp/src/errors.rs:38 (and the
                                  panics of algorithm.rs:835-837, 907-911 turned into errors) */
    EGX_ERR_NO_DEVICE = 2,     /* no gfx950 device / HIP runtime unusable */
    EGX_ERR_HIP = 3,           /* a HIP call failed (message has the HIP error string) */
    EGX_ERR_NOT_FITTED = 4,    /* predict* / get_inner before finalize/fit */
    EGX_ERR_LINALG = 5,        /* GpError::LinalgError (not positive definite), errors.rs:19 */
    EGX_ERR_LIKELIHOOD = 6,    /* GpError::LikelihoodComputationError, errors.rs:12 */
    EGX_ERR_UNSUPPORTED = 7,
    EGX_ERR_PEER = 8,          /* collective calls: another rank failed, or did not answer in time */
    EGX_ERR_NO_FINITE_START = 9 /* egx_infill_optimize: no start ended at a finite value (*f_best = +inf) */
} egx_rc;

/* per-evaluation status (the value channel) */
typedef enum {
    EGX_STATUS_OK = 0,
    EGX_STATUS_NOT_POSITIVE_DEFINITE = 1, /* cholesky()? failed, algorithm.rs:1004 */
    EGX_STATUS_ILL_CONDITIONED_FT = 2,    /* algorithm.rs:1022-1026 */
    EGX_STATUS_ILL_CONDITIONED_F = 3,     /* algorithm.rs:1015-1020 */
    EGX_STATUS_NAN_THETA = 4,             /* algorithm.rs:885-891 */
    EGX_STATUS_RANK_FAILED = 5            /* sweep only: the rank that held this candidate failed (the call returns
                                             EGX_ERR_PEER on every other rank, the failing rank returns its own error) */
} egx_status;

/* crates/gp/src/correlation_models.rs: the four CorrelationModel impls */
typedef enum {
    EGX_CORR_SQUARED_EXPONENTIAL = 0, /* :91-104  */
    EGX_CORR_ABSOLUTE_EXPONENTIAL = 1, /* :185-196 */
    EGX_CORR_MATERN32 = 2,            /* :277-286, :326-353 */
    EGX_CORR_MATERN52 = 3             /* :446-455, :497-523 */
} egx_corr;

/* crates/gp/src/mean_models.rs: the three RegressionModel impls */
typedef enum {
    EGX_MEAN_CONSTANT = 0, /* :42-44   */
    EGX_MEAN_LINEAR = 1,   /* :68-71   */
    EGX_MEAN_QUADRATIC = 2 /* :97-104  */
} egx_mean;

/* Builder state that reaches the hot path: GpValidParams, crates/gp/src/parameters.rs:93-121 */
typedef struct {
    int32_t corr;         /* egx_corr */
    int32_t mean;         /* egx_mean */
    double nugget;        /* default 100*f64::EPSILON, parameters.rs:118 */
    int32_t device;       /* HIP device ordinal; -1 = current device */
    int32_t n_workspaces; /* correlation-matrix workspaces (concurrent likelihood evaluations), >= 1 */
    const double *w_star; /* optional KPLS rotations (d x kpls_dim), algorithm.rs:843-855; NULL = identity */
    int64_t kpls_dim;     /* columns of w_star (ignored when w_star == NULL) */
} egx_gp_config;

/* ---- library level ------------------------------------------------------ */
int32_t egx_abi_version(void);
const char *egx_last_error(void); /* thread-local, never NULL */
int32_t egx_device_count(void);   /* number of visible HIP devices (0 when none) */
void egx_gp_config_default(egx_gp_config *cfg);
/* Destroyed handles leave their device resources (the correlation-matrix workspaces with their streams and pinned
 * buffers, the training-set buffers) in a per-process pool keyed by the handle's shape (device, padded n, d, trend
 * columns, workspaces): the reference creates a new model per fit (GpValidParams::fit is one-shot, algorithm.rs:785-794;
 * egobox-moe trains one per expert, crates/moe/src/algorithm.rs:167-177), and the next egx_gp_create of that shape
 * starts warm instead of paying a multi-GiB allocation and a first factorisation on untouched memory.  Bounded by
 * EGX_POOL_MAX_GB (environment, default 48, 0 = no pool).  egx_trim frees everything cached and returns the bytes.
 * The same holds for GROUPS (egx_gp_create_group): the group's slabs are pooled by their three sizes, every member's workspace
 * and training-set buffers under the member's shape -- the next group of that shape adopts them (hits: k members + 1).
 * Streams carry no shape: idle workspaces (pooled or freed) leave theirs in a per-device free list and a handle of ANY shape
 * takes them from there (the runtime needs ~3 ms to create a stream, a workspace has four); egx_trim destroys the idle ones. */
int64_t egx_trim(void);
void egx_pool_stats(int64_t *cached_bytes, int64_t *hits, int64_t *misses);
/* Chain launches (the serial chain of a factorisation as one persistent launch) bound every device-side
 * wait by EGX_PIPE_TIMEOUT_MS.  A wait that runs out -- waves pre-empted while several processes share the GPU, a debugger --
 * is not a numerical event and the reference's cholesky() (crates/gp/src/algorithm.rs:1004) knows no such failure (the
 * objective only ever sees numerical errors, :893-896): the evaluation is run ONCE more, alone, by separate launches of the
 * same handle, and only a second failure is reported as EGX_ERR_HIP ("pipe_retry" = 0 / EGX_PIPE_RETRY=0: report at once).
 * Process-wide counters since start-up: *aborted = evaluations whose chain launch ran into the bound, *retried = those that
 * were run again.  Either pointer may be NULL. */
void egx_chain_stats(int64_t *aborted, int64_t *retried);
/* The factorisation's scheduling settings at run time (the EGX_* environment variables of DESIGN.md section 4, read
 * once at start-up; here by name without the prefix, lower case):
 *   "potrf_group"      panels per trailing update (0 = by size)          "stream_min"  tiles from which the stream kernel is used
 *   "gemm_small"       tiles below which the 64 x 64 kernel is used      "look_min"    trailing columns down to which the chain looks ahead
 *   "potrf_left"       left-looking updates 0 never / 1 per handle / 2   "lur_side"    look-ahead update beside (1) or in front of (0) the trailing one
 *   "pipe"             chain launches 0 never / 1 per handle / 2 per group of panels only
 *   "pipe_timeout_ms"  bound of every device-side wait of a chain launch (default 2000; exceeded = one retry by separate
 *                      launches, see egx_chain_stats -- never a hang)
 *   "pipe_retry"       1 (default): that retry; 0: EGX_ERR_HIP at once
 *   "trsv_fused"       1 (default): the back-substitution gamma = C^-T rho (crates/gp/src/algorithm.rs:1034) is ONE launch whose
 *                      workgroups hand the blocks' solutions to each other on the device (waits bounded by "pipe_timeout_ms": after a
 *                      wait that ran out the launch-per-block form is run once, counted by egx_chain_stats; EGX_ERR_HIP only if that
 *                      fails too or with "pipe_retry" = 0 -- never a wrong gamma); 0: one launch per 256-column block (rounds 1-5).
 *                      The same sums in the same order either way: the same bits
 *   "trsm_rows_min"    panels of a factorisation with at least this many rows (of ONE matrix; default 4096) are solved by the
 *                      row-owning kernel k_panel_trsm_rows, shorter ones by k_panel_trsm16; a value beyond any n switches the
 *                      kernel off.  The same instructions on the same values either way: the same bits, at launch time
 * (the test hook "pipe_stall" exists only in the test build of the library, -DEGX_TEST_HOOKS).  They move launches between streams and kernels between tile shapes, never the
 * arithmetic inside a kernel; "potrf_group" / "stream_min" / "gemm_small" / "potrf_left" / "pipe" change which kernel
 * updates a block, or the order in which updates are summed, hence the rounding -- and "potrf_left" / "pipe" /
 * "potrf_group" enter a handle's schedule (egx_gp_get_schedule) when it is CREATED or its lock-step width is set, not
 * later.  Process-wide, atomic; meant for A/B runs, not for use while evaluations are in flight.  *previous (optional)
 * receives the old value.  Used by bench.py's roofline leg ("lur_side" = 0: clean per-launch durations) and the tests. */
int32_t egx_set_tuning(const char *knob, int32_t value, int32_t *previous);

/* ---- host-side helpers (no device needed) -------------------------------- */
/* utils.rs:45-54 normalize(): column mean, sample std (ddof=1), zero std -> 1. */
int32_t egx_normalize(const double *x, int64_t n, int64_t d, double *xnorm /*n*d*/,
                      double *mean /*d*/, double *std /*d*/);
/* mean_models.rs value(): number of basis columns p for input dimension d. */
int64_t egx_regression_ncols(int32_t mean, int64_t d);
/* mean_models.rs value(): F (n x p) from (normalised) x (n x d). */
int32_t egx_regression_basis(int32_t mean, const double *x, int64_t n, int64_t d, double *f /*n*p*/);

/* ---- mixed-integer design spaces (host side, no device needed) ------------
 * XType (crates/ego/src/types.rs) and the free functions of crates/ego/src/gpmix/mixint.rs:38-226.  A spec is nx typed
 * columns; its UNFOLDED, continuously relaxed form has d = sum (ENUM ? n : 1) columns, an Enum column of n levels being a
 * one-hot group of n.  The arithmetic (csrc/mixint.h, one text for host and device):
 *   cast      FLOAT unchanged; INT rounds half away from zero (f64::round; the sign of zero is kept, NO clamping to lo / hi, as in the
 *             reference); ORD takes the value with the smallest |x - v|, the FIRST in list order on a tie; an ENUM group becomes the
 *             one-hot of its FIRST maximum.  A NaN / +-inf INT or ORD coordinate stays as it is, an ENUM group with a non-finite
 *             entry becomes all NaN (the reference panics): a non-finite point stays non-finite.
 *   unfold    the enum index (truncated, `as usize`) becomes the one-hot group; an index outside [0, n) or a non-finite one is
 *             EGX_ERR_INVALID_VALUE, the message names row and column
 *   fold      the index of the group's first maximum (NaN for a group with a non-finite entry)
 *   to_discrete = cast, then fold (mixint.rs:220-226); continuous_limits: ORD min / max of its values, ENUM [0, 1] per level
 * Where the reference is not followed: its fold slices the unfolded row at the FOLDED index (:89) and its unfold reads the
 * non-enum columns at the UNFOLDED index (:126), which is right only while no Enum column precedes; here fold reads at the
 * unfolded index and unfold at the folded one (csrc/mixint.h says on which specs the two agree).
 * Every function validates the spec first (EGX_ERR_INVALID_VALUE, the message names the entry): unknown kind, ORD with n < 1 or a
 * non-finite value, ENUM with n < 1, lo > hi; more than EGX_MIXINT_MAX_ORD_VALUES Ord values in all is EGX_ERR_UNSUPPORTED. */
typedef enum { EGX_XTYPE_FLOAT = 0, EGX_XTYPE_INT = 1, EGX_XTYPE_ORD = 2, EGX_XTYPE_ENUM = 3 } egx_xtype_kind;
typedef struct {
    int32_t kind;         /* egx_xtype_kind */
    int32_t n;            /* ORD: number of values, ENUM: number of levels (ignored otherwise) */
    double lo, hi;        /* FLOAT / INT */
    const double *values; /* ORD (n), borrowed during the call only */
} egx_xtype;
#define EGX_MIXINT_MAX_ORD_VALUES 4096 /* Ord values per spec, all columns together: the nearest-value search is a loop per coordinate */
int32_t egx_mixint_unfolded_dim(const egx_xtype *xt, int32_t nx, int64_t *d);
int32_t egx_mixint_continuous_limits(const egx_xtype *xt, int32_t nx, double *xlimits /*d*2*/);
int32_t egx_mixint_unfold(const egx_xtype *xt, int32_t nx, const double *x /*m*nx*/, int64_t m, double *out /*m*d*/);
int32_t egx_mixint_fold(const egx_xtype *xt, int32_t nx, const double *x /*m*d*/, int64_t m, double *out /*m*nx*/);
int32_t egx_mixint_cast(const egx_xtype *xt, int32_t nx, const double *x /*m*d*/, int64_t m, double *out /*m*d, may be x*/);
int32_t egx_mixint_to_discrete(const egx_xtype *xt, int32_t nx, const double *x /*m*d*/, int64_t m, double *out /*m*nx*/);

/* ---- handle lifetime ------------------------------------------------------
 * Replaces the theta-independent part of GpValidParams::fit
 * (crates/gp/src/algorithm.rs:795-866): copies x (n x d) and y (n), normalises
 * both, builds the regression basis, uploads, allocates workspaces. */
int32_t egx_gp_create(const egx_gp_config *cfg, const double *x, const double *y, int64_t n,
                      int64_t d, egx_gp **out);
void egx_gp_destroy(egx_gp *gp);
/* dims: n, d (dims().0, algorithm.rs:437-439), p = basis columns, h = theta length */
int32_t egx_gp_dims(const egx_gp *gp, int64_t *n, int64_t *d, int64_t *p, int64_t *h);
/* the handle's own copy of the raw training set (GaussianProcess::training_data, algorithm.rs:969-978: the fitted model
 * owns copies of x and y); x_out (n*d), y_out (n), either may be NULL */
int32_t egx_gp_get_training_data(const egx_gp *gp, double *x_out, double *y_out);
/* MixintGpMixture (crates/ego/src/gpmix/mixint.rs:589-697): a model that carries xtypes casts every query point to its nearest
 * admissible discrete point before it is used, in EVERY call that takes query points -- egx_gp_predict / _var / _valvar, the three
 * _gradients (the model's gradients at the cast point with respect to the unfolded coordinates, m x d, :656-687),
 * egx_gp_predict_covariance, egx_gp_sample, egx_gp_predict_valvar_multi (every member by its own spec or none),
 * egx_moe_predict_valvar(_gradients) (the experts cast for themselves) and the infill handles built on it -- ON THE DEVICE, in the
 * kernel that reads the raw rows anyway: no extra launch, no host pass over the queries.  The result is bit for bit what the
 * model without xtypes returns on egx_mixint_cast(x).  The spec is copied (host copy and a small device table); its unfolded
 * dimension must equal the handle's d (EGX_ERR_INVALID_VALUE, as every fault of egx_mixint_*; checked before the device is touched).
 * nx == 0 clears: the handle is a continuous model again -- same kernels, same bits as before.  The TRAINING inputs are the
 * caller's business: pass them already cast to egx_gp_create; the handle does not recast them. */
int32_t egx_gp_set_xtypes(egx_gp *gp, const egx_xtype *xt, int32_t nx);
/* the spec back: *nx columns (the first min(cap, *nx) written to xt), *n_ord_values Ord values in column order into ord_values (or
 * NULL: xt[j].values is then NULL); any output may be NULL.  *nx == 0: no xtypes. */
int32_t egx_gp_get_xtypes(egx_gp *gp, egx_xtype *xt /*cap*/, int32_t cap, int32_t *nx, double *ord_values, int64_t *n_ord_values);

/* ---- likelihood (the unit COBYLA multiplies) ------------------------------
 * One evaluation of `reduced_likelihood(fx, corr.value(d, theta, w), ...)`
 * (algorithm.rs:892-896, 988-1056).  theta_len is h or 1 (broadcast,
 * algorithm.rs:829-838).  *lkh is the reduced likelihood (NOT negated);
 * on status != 0 it is -inf (the reference's objective is then +inf).
 * Thread-safe: concurrent callers each take a workspace from the handle's pool (n_workspaces).  The fitted factor
 * lives in workspace 0: with n_workspaces > 1 a fitted model is never disturbed (callers wait for another workspace);
 * with a single workspace an evaluation overwrites it and the handle must be finalized again before predicting. */
int32_t egx_gp_likelihood(egx_gp *gp, const double *theta, int64_t theta_len, double *lkh,
                          int32_t *status);
/* k candidates, thetas is (k x theta_len); the multistart / theta-sweep unit of
 * algorithm.rs:928-945 (rayon par_iter over starts).  Pipelines over the handle's workspaces; a fitted model keeps
 * workspace 0 (and stays fitted) when n_workspaces > 1. */
int32_t egx_gp_likelihood_batch(egx_gp *gp, const double *thetas, int64_t k, int64_t theta_len,
                                double *lkh /*k*/, int32_t *status /*k*/);
/* Width of the LOCK-STEP groups of egx_gp_likelihood_batch / egx_sweep_likelihood: that many candidates (consecutive
 * workspaces) are factored by ONE launch sequence -- the candidates of a sweep have the same n, hence the same
 * schedule; the serial chain of the factorisation then costs its latency once per group and every launch has `width`
 * times the tiles.  1 = every candidate on its own stream set (round 2's pipeline); 0 = the default
 * (min(n_workspaces, 12) below a padded n of 14336 -- one slot: the serial chain is what such an evaluation waits for --,
 * from there on 4, and 8 from 16 workspaces on).  The width is CLAMPED to min(n_workspaces, 16) -- 16 candidates are the
 * most one launch takes; a wider request gives slots of 16 -- and egx_gp_get_lockstep / egx_gp_get_schedule report the
 * width in force.  A candidate's result does
 * not depend on its companions or on how many of them share its launch (same kernels, same arithmetic: bit-identical);
 * it does not depend on the width either, with ONE exception: a handle with a padded n >= 14336 and a width >= 8 factors
 * LEFT-looking over its panel groups (two long-K updates per tile of the factor instead of one per earlier group), a
 * different order of the same sums than the right-looking schedule every other handle uses (EGX_POTRF_LEFT=0 switches
 * it off, 2 forces it everywhere).  Whatever the schedule, it is a property of the HANDLE's shape and setting, so all
 * evaluations of a handle -- and of its replicas on other ranks -- agree bit for bit. */
int32_t egx_gp_set_lockstep(egx_gp *gp, int32_t width);
int32_t egx_gp_get_lockstep(const egx_gp *gp);
/* Which schedule the handle's factorisations follow -- decided when the handle is created or its lock-step width is set,
 * from its padded size, lock-step width and number of workspaces, kept by egx_gp_shrink -- so that a caller can tell two
 * handles that will not give the same bits apart (a sweep on a 16-workspace handle and a re-evaluation of its winner on a
 * 1-workspace handle at n = 16384 differ by 1e-10 relative).  out[0..5] = { left-looking group updates, left-looking
 * C^-T rider, pipelined chain launches (the chain of a panel group -- diagonal blocks, panel solves, in-group updates: the
 * panel step of `cholesky()`, crates/gp/src/algorithm.rs:1004 -- as one persistent launch), whole factorisation as one such
 * launch, panels per group, lock-step width }; out_len >= 6.  out[6] (when out_len >= 7): the whole factorisation as ONE FLOW
 * launch -- critical stage lists + bulk-class rounds per column, csrc/pipe_flow.h; round 6: a lone one-workspace handle that
 * is not a member of a group, padded size 5376 .. 14080 (value 1); from 14336 on (value 2) such a handle factors right-looking by
 * separate launches and hands its LAST 6144 .. 7167 columns, fully updated, to one flow launch.  (An evaluation WITH the
 * theta-gradient factors by separate launches on such a handle too -- the rider C^-T runs beside them, behind a flow launch it
 * would wait: the likelihood egx_gp_likelihood_grad returns there is egx_gp_likelihood's to rounding, 1e-12 relative, not bit for
 * bit.)  Further slots are set to 0. */
int32_t egx_gp_get_schedule(const egx_gp *gp, int32_t *out, int32_t out_len);
/* Give back what only an optimisation needed: the handle keeps its first n_keep (>= 1) workspaces -- workspace 0 holds the
 * fitted factor, which survives -- and frees the others together with the theta-gradient's scratch.  A tuned fit runs its
 * multistart on up to 12 workspaces (2 GiB each at n = 16384); the fitted model that stays resident (an EGO objective, an
 * expert of a mixture) needs one.  The schedule of the handle (egx_gp_get_schedule) does not change -- the model keeps giving
 * the bits it gave before --; the lock-step width is capped by the workspaces that are left. */
int32_t egx_gp_shrink(egx_gp *gp, int32_t n_keep);
/* NEW capability (the reference has no theta-gradient, algorithm.rs:880: the objective closure ignores `_gradient`):
 * the reduced likelihood of algorithm.rs:988-1056 AND dL/dtheta (length h) at one theta; validated against the oracle's
 * closed form and by finite differences of the parity-checked likelihood.  Needs the factor, C^-T (n^2 doubles of
 * scratch per candidate in flight, allocated on first use) and R^-1 (written over the factor).  A fitted model with
 * n_workspaces > 1 keeps workspace 0 and stays fitted; with a single workspace the call un-fits it. */
int32_t egx_gp_likelihood_grad(egx_gp *gp, const double *theta, int64_t theta_len, double *lkh,
                               double *dlkh_dtheta /*h*/, int32_t *status);
/* k candidates at once (thetas is k x theta_len, grads k x h row-major): the gradient counterpart of
 * egx_gp_likelihood_batch -- the objective + gradient evaluations of a gradient-based multistart (the rayon tasks of
 * algorithm.rs:928-945).  Candidates are pipelined over the workspaces; the candidates of a lock-step slot
 * (egx_gp_set_lockstep, at most 16) run EVERY stage -- factorisation, C^-T, R^-1, the trace kernel -- as one launch
 * sequence.  A candidate's (likelihood, gradient) are bit for bit what egx_gp_likelihood_grad returns for it alone. */
int32_t egx_gp_likelihood_grad_batch(egx_gp *gp, const double *thetas, int64_t k, int64_t theta_len,
                                     double *lkh /*k*/, double *dlkh_dtheta /*k x h*/, int32_t *status /*k*/);

/* ---- fit ------------------------------------------------------------------
 * ThetaTuning::Fixed fit (algorithm.rs:869-872, 966-978; python n_start=-1,
 * python/src/gp_mix.rs:202-208): one likelihood evaluation whose factor and
 * inner params stay resident.  Error return when the evaluation fails. */
int32_t egx_gp_finalize(egx_gp *gp, const double *theta, int64_t theta_len);
/* Lock-step across MODELS.  The reference's callers multiply independent models, not only candidates of one model: the
 * expert loop of egobox-moe (crates/moe/src/algorithm.rs:167-177: one GP per cluster, fitted one after the other) and
 * EGO's objective + constraint surrogates (crates/ego/src/solver/solver_impl.rs:370-391) -- whose QUERY side is lock-step too:
 * egx_gp_predict_valvar_multi, egx_gp_predict_valvar_gradients_multi, and the runs of an infill handle (egx_infill_get_runs).
 *   egx_gp_create_group   k models of ONE shape (same n, d, trend, kernel, nugget: `cfg`; training sets x (k x n x d) and
 *                         y (k x n), one after the other) whose matrices live in one slab at the strides a lock-step launch
 *                         needs.  out[0..k) are ordinary handles with one workspace each -- every entry point works on them
 *                         and each is destroyed on its own (the slab goes with the last one).
 *   egx_gp_finalize_multi `fit` at fixed theta (thetas: k x theta_len, row j for gps[j]) of k DISTINCT handles: members of
 *                         one group in consecutive slots are factored by ONE launch sequence (up to 12 per sequence), any
 *                         other handle on its own -- the fitted models are bit for bit what egx_gp_finalize gives each of them
 *                         (the same kernels on the same values: a matrix never sees its companions).  The first error of
 *                         any model is returned after all of them have been finished.
 *   egx_gp_likelihood_multi  the same for the reduced likelihood alone (algorithm.rs:988-1056); status as egx_gp_likelihood.
 *                         NOTE: both calls evaluate on every member's workspace 0, where a fitted model's factor lives: a fitted
 *                         member is UN-FITTED by egx_gp_likelihood_multi too (egx_gp_likelihood keeps a fitted handle with spare
 *                         workspaces fitted; call egx_gp_finalize[_multi] again before predicting). */
int32_t egx_gp_create_group(const egx_gp_config *cfg, const double *x, const double *y, int64_t n, int64_t d, int32_t k,
                            egx_gp **out /*k*/);
int32_t egx_gp_finalize_multi(egx_gp *const *gps, int32_t k, const double *thetas /*k x theta_len*/, int64_t theta_len);
int32_t egx_gp_likelihood_multi(egx_gp *const *gps, int32_t k, const double *thetas /*k x theta_len*/, int64_t theta_len,
                                double *lkh /*k*/, int32_t *status /*k*/);
/* ThetaTuning::Full across MODELS (round 6): the tuned fit the expert loop runs per cluster (crates/moe/src/algorithm.rs:167-177
 * -> find_best_expert :209-262 -> GpValidParams::fit -> the multistart COBYLA of crates/gp/src/algorithm.rs:921-945), and EGO's
 * per-output surrogates (crates/ego/src/solver/solver_impl.rs:370-391), for k DISTINCT handles with the same number of
 * hyperparameters -- the members of a group (egx_gp_create_group) in consecutive slots are evaluated in lock-step: per round
 * of the k x n_starts COBYLA machines and per start index, the trial points of all models are ONE launch sequence.
 * theta0s is (k x n_starts x h) in linear theta units (model-major), lo / hi / bounds_len / max_eval as egx_gp_fit,
 * n_evals_out (k, optional) the evaluations per model.  Every member ends fitted exactly as egx_gp_fit on a one-workspace
 * handle of its training set would leave it (a machine only sees its own model's values, an evaluation never its companions):
 * theta*, likelihood and predictions are the same bits. */
int32_t egx_gp_fit_multi(egx_gp *const *gps, int32_t k, const double *theta0s /*k x n_starts x h*/, int64_t n_starts,
                         const double *lo, const double *hi, int64_t bounds_len, int64_t max_eval, int64_t *n_evals_out /*k*/);
/* The theta-gradient across MODELS (new, like egx_gp_likelihood_grad itself): likelihood and dL/dtheta of k DISTINCT handles with
 * the same number of hyperparameters h, row j of thetas (k x theta_len) for gps[j]; lkh (k), dlkh_dtheta (k x h), status (k).
 *   Handles  Members of one group (egx_gp_create_group) in consecutive slots form runs (at most 12) and run EVERY stage -- the
 *            factorisation, the C^-T rider, R^-1 = C^-T C^-1, the trace kernel -- in lock-step, the member a grid coordinate;
 *            their C^-T buffers are the group's (one n_pad^2 slot per member, shared with the x-gradients' cache: no buffer per
 *            handle).  Every other handle -- a lone handle, a member out of order, a handle with w_star -- goes one by one.
 *            The result never depends on which route was taken.
 *   Bits     Row j is bit for bit what egx_gp_likelihood_grad(gps[j], thetas + j theta_len, ...) returns on that handle alone:
 *            a matrix never sees its companions, and the form of the trace kernel depends on one member's shape and its OWN
 *            coefficients only.
 *   Status   as egx_gp_likelihood_grad_batch: a NaN theta row gives -inf, EGX_STATUS_NAN_THETA and a zero gradient -- not an
 *            error return --, a member that is not positive definite its status and a zero gradient; neighbours are unaffected.
 *   NOTE     like egx_gp_likelihood_multi the call evaluates on every member's workspace 0: a fitted member is UN-FITTED (also
 *            one with spare workspaces, which egx_gp_likelihood_grad would keep fitted), and its cached C^-T is dropped; call
 *            egx_gp_finalize[_multi] again before predicting.  A fitted model that is not part of the call keeps its state. */
int32_t egx_gp_likelihood_grad_multi(egx_gp *const *gps, int32_t k, const double *thetas /*k x theta_len*/,
                                     int64_t theta_len, double *lkh /*k*/, double *dlkh_dtheta /*k x h*/,
                                     int32_t *status /*k*/);
/* egx_gp_fit_lbfgs across MODELS: k x n_starts projected L-BFGS machines, start-major and model-minor as egx_gp_fit_multi lays
 * out its COBYLA machines; per round and start index, the trial points of the models whose machine still asks are ONE
 * egx_gp_likelihood_grad_multi evaluation.  The best start per model wins (the first on ties), then ONE egx_gp_finalize_multi
 * of the winners.  theta0s is (k x n_starts x h) in linear theta units (model-major), lo / hi / bounds_len / max_iter as
 * egx_gp_fit_lbfgs, n_evals_out (k, optional) the likelihood + gradient evaluations per model.  Every member ends exactly as
 * egx_gp_fit_lbfgs leaves a one-workspace handle of its training set -- theta*, likelihood, evaluations and predictions are the
 * same bits -- wherever the two handles factor by the same schedule (egx_gp_get_schedule): every padded size below 5376. */
int32_t egx_gp_fit_lbfgs_multi(egx_gp *const *gps, int32_t k, const double *theta0s /*k x n_starts x h*/, int64_t n_starts,
                               const double *lo, const double *hi, int64_t bounds_len, int64_t max_iter,
                               int64_t *n_evals_out /*k*/);
/* ThetaTuning::Full fit (algorithm.rs:874-948): multistart derivative-free
 * maximisation of the likelihood over log10(theta) in [lo,hi], then finalize.
 * theta0s is (n_starts x h) in LINEAR theta units: the caller supplies the
 * starts (prepare_multistart, optimization.rs:26-71, stays on the caller's side
 * because its LHS stream is the caller's RNG).  bounds_len is h or 1. */
int32_t egx_gp_fit(egx_gp *gp, const double *theta0s, int64_t n_starts, const double *lo,
                   const double *hi, int64_t bounds_len, int64_t max_eval, int64_t *n_evals_out);

/* ThetaTuning::Partial (parameters.rs:24-32, algorithm.rs:822-826, 873-960): only the components listed in
 * active_idx (strictly increasing, n_active of them) are optimised, the others stay at theta_init (h values).
 * theta0s is (n_starts x n_active) in theta space, lo/hi have 1 or n_active entries;
 * maxeval per start = clamp(10 n_active, 25, max_eval). */
int32_t egx_gp_fit_partial(egx_gp *gp, const double *theta_init, const int64_t *active_idx, int64_t n_active,
                           const double *theta0s, int64_t n_starts, const double *lo, const double *hi,
                           int64_t bounds_len, int64_t max_eval, int64_t *n_evals_out);

/* Gradient-based variant (NEW: consumes the theta-gradient; same contract as egx_gp_fit otherwise):
 * projected L-BFGS on log10(theta) per start, ALL starts advanced in lock-step (a round's trial points are one
 * egx_gp_likelihood_grad_batch), best start wins, then finalize.  max_iter bounds the iterations per start;
 * *n_evals_out counts likelihood+gradient evaluations. */
int32_t egx_gp_fit_lbfgs(egx_gp *gp, const double *theta0s, int64_t n_starts, const double *lo,
                         const double *hi, int64_t bounds_len, int64_t max_iter, int64_t *n_evals_out);

/* ---- prediction (GaussianProcess::{predict, predict_var, predict_valvar},
 * algorithm.rs:253-307).  xq is (m x d) in ORIGINAL units. */
int32_t egx_gp_predict(egx_gp *gp, const double *xq, int64_t m, double *y /*m*/);
int32_t egx_gp_predict_var(egx_gp *gp, const double *xq, int64_t m, double *var /*m*/);
int32_t egx_gp_predict_valvar(egx_gp *gp, const double *xq, int64_t m, double *y, double *var);
/* The posterior of k DISTINCT fitted models in one call: gps[j] answers ITS OWN block of m queries, rows [j m, (j + 1) m) of
 * xq (original units, normalised with gps[j]'s x_mean | x_std), into rows of y and var likewise (either may be NULL, not
 * both).  What a k-fold cross-validation asks of the k fits of its folds (GpMetrics, crates/moe/src/metrics.rs:19-144;
 * find_best_expert, crates/moe/src/algorithm.rs:209-347).  Members of one group (egx_gp_create_group) in consecutive slots
 * answer in lock-step: one launch sequence, one upload, one read-back and one host synchronisation per run of members (the
 * runs of egx_gp_finalize_multi) and chunk of queries, the member a grid coordinate of the kernels.  Any other handle is
 * served on its own as by egx_gp_predict_valvar.  The lock-step route is the batched one for every m (no C^-T cache per
 * member).  CONTRACT: for every member, y and var are bit for bit what egx_gp_predict_valvar(gps[j], block j, m, ..) returns
 * on its batched route, which that call takes for m > 8; for m <= 8 the lone call may answer from its cached C^-T, and the
 * two agree to rounding only.  Arguments as for the other _multi calls: NULL / k <= 0 / duplicate handles / unequal d are
 * EGX_ERR_INVALID_VALUE before any work, the locks are taken in a fixed order, an unfitted member is EGX_ERR_NOT_FITTED; the
 * first error is returned after every member has been served. */
int32_t egx_gp_predict_valvar_multi(egx_gp *const *gps, int32_t k, const double *xq /*k x m x d, block j for gps[j]*/,
                                    int64_t m, double *y /*k x m or NULL*/, double *var /*k x m or NULL*/);

/* ---- x-gradients of the predictions (what EGO's infill optimiser asks per point):
 * GaussianProcess::predict_gradients algorithm.rs:510-549, predict_var_gradients(_single) :555-617, 702-709,
 * predict_valvar_gradients :711-727; kernels' jacobian correlation_models.rs:106-123, 198-214, 355-413, 524-586,
 * trend jacobian mean_models.rs:50-52, 76-81, 110-128.  xq is (m x d) in ORIGINAL units, grad is (m x d)
 * row-major, d out / d xq_k in original units.  Batched over m (the reference loops point by point and redoes
 * R^-1 F and chol(F^T R^-1 F) for every point); the first variance-gradient call after a fit caches C^-T. */
int32_t egx_gp_predict_gradients(egx_gp *gp, const double *xq, int64_t m, double *grad /*m*d*/);
int32_t egx_gp_predict_var_gradients(egx_gp *gp, const double *xq, int64_t m, double *grad /*m*d*/);
int32_t egx_gp_predict_valvar_gradients(egx_gp *gp, const double *xq, int64_t m, double *grad_y /*m*d*/,
                                        double *grad_var /*m*d*/);
/* The x-gradients of k DISTINCT fitted models in one call -- the query side of egx_gp_create_group's client, an optimiser's
 * objective and constraint surrogates (solver_impl.rs:370-391): gps[j] answers ITS OWN block of m queries, rows [j m, (j + 1) m)
 * of xq, into block j (m x d) of grad_y and grad_var (either may be NULL, not both).  Runs of fitted members of one group in
 * consecutive slots with one n and trend (and a correlation with one coefficient column per input: not KPLS + Matern) answer
 * in lock-step: one launch sequence per run, chunk of queries and half, the member a grid coordinate of the x-gradient kernels
 * and of the weight GEMMs, whose C^-T and -R^-1 F the group holds for all its members at one stride (allocated on the first
 * such call or the first variance-gradient call of any member; per member what a lone handle holds).  A run is at most 16
 * members and is cut where its blocks pass the bound of egx_gp_predict_valvar_multi; any other handle is served on its own
 * as by egx_gp_predict_valvar_gradients.  CONTRACT: for every member and m > 8, both arrays are bit for bit what
 * egx_gp_predict_valvar_gradients(gps[j], block j, m, ..) returns; for m <= 8 the lone call may take its few-query route, a
 * run never does, and the two agree to rounding only.  Arguments, locking and errors as for egx_gp_predict_valvar_multi. */
int32_t egx_gp_predict_valvar_gradients_multi(egx_gp *const *gps, int32_t k, const double *xq /*k x m x d, block j for gps[j]*/,
                                              int64_t m, double *grad_y /*k x m x d or NULL*/,
                                              double *grad_var /*k x m x d or NULL*/);

/* ---- posterior covariance and trajectories (GpSurrogateExt::sample, crates/moe/src/surrogates.rs:66-81;
 * GaussianProcess::_compute_covariance algorithm.rs:310-326, sample_chol / sample_eig / sample :383-395, helper
 * sample :1153-1193).  xq is (m x d) in ORIGINAL units; every array is host memory, row-major.
 *
 * egx_gp_predict_covariance: cov (m x m) = sigma2 (K(xq, xq) - rt^T rt + u^T u), K without nugget (diagonal 1), rt / u those
 * of predict_var: the diagonal is predict_var before its clamp at 0.  Exactly symmetric.
 *
 * egx_gp_sample: traj (m x n_traj) = predict(xq) 1^T + F Z, F the lower Cholesky factor of
 *   EGX_SAMPLE_CHOLESKY  cov itself (sample_chol); EGX_ERR_LINALG, naming the 1-based pivot, when it is not positive definite
 *   EGX_SAMPLE_PSD       cov + tau I (sample / sample_eig), tau0 = max(1e-9, 1e-12 max_i cov_ii), times 10 after every failed
 *                        factorisation, at most six retries, then EGX_ERR_LINALG.
 * DEVIATION from the reference's sample_eig: no eigendecomposition.  The reference samples with the eigenvalues below 1e-9
 * clipped to 0 (Sigma_+); the covariance sampled here, F F^T = Sigma + tau I, differs from Sigma_+ by at most
 * tau + max(1e-9, |lambda_min(Sigma)|) in 2-norm.  The tau used is written to *tau_out (0 for EGX_SAMPLE_CHOLESKY; may be NULL).
 * z: (m x n_traj) normals supplied by the caller (with z = I, n_traj = m, traj - predict(xq) is F), or NULL: the library's
 * stream, egx_random_normals(seed).  m = 0 or n_traj = 0 succeeds and does nothing; serialised per handle like predict*. */
typedef enum { EGX_SAMPLE_CHOLESKY = 0, EGX_SAMPLE_PSD = 1 } egx_sample_method;
int32_t egx_gp_predict_covariance(egx_gp *gp, const double *xq, int64_t m, double *cov /*m*m*/);
int32_t egx_gp_sample(egx_gp *gp, const double *xq, int64_t m, int64_t n_traj, int32_t method, uint64_t seed,
                      const double *z /*m*n_traj or NULL*/, double *traj /*m*n_traj*/, double *tau_out /*1 or NULL*/);
/* The normals egx_gp_sample draws for `seed` when z is NULL, (m x n_traj), computed on `device` (-1: the current one):
 * Philox4x64-10 with numpy.random.Philox's constants, key (seed, 0); Z[i, j] is normal (i mod 4) of the block with counter
 * (i / 4, j, 0, 0), by Box-Muller over u = ((w >> 11) + 0.5) 2^-53 -- it depends on (seed, i, j) only
 * (egobox_amd/csrc/philox.h). */
int32_t egx_random_normals(int32_t device, uint64_t seed, int64_t m, int64_t n_traj, double *z /*m*n_traj*/);

/* ---- fitted state download (GpInnerParams algorithm.rs:47-60 + accessors
 * theta()/variance()/likelihood() :413-431), for serde parity.  Any pointer may
 * be NULL (skipped).  r_chol is (n x n) lower with zero upper triangle;
 * ft_qr_r has a positive diagonal. */
typedef struct {
    double *theta;      /* h */
    double *likelihood; /* 1 */
    double *sigma2;     /* 1 : variance() = sigma2 * y_std^2 */
    double *beta;       /* p */
    double *gamma;      /* n */
    double *r_chol;     /* n*n */
    double *ft;         /* n*p */
    double *ft_qr_r;    /* p*p */
    double *x_mean;     /* d */
    double *x_std;      /* d */
    double *y_mean;     /* 1 */
    double *y_std;      /* 1 */
    double *xt_norm;    /* n*d */
    double *yt_norm;    /* n */
} egx_gp_inner_view;
int32_t egx_gp_get_inner(egx_gp *gp, const egx_gp_inner_view *view);
/* Inverse of egx_gp_get_inner: install a fitted state produced elsewhere (e.g. deserialised from the
 * reference's serde JSON, crates/moe/src/surrogates.rs:426-441 `load`) WITHOUT re-factoring: theta (h),
 * likelihood, sigma2, beta (p), gamma (n), r_chol (n*n, lower), ft (n*p), ft_qr_r (p*p) are read;
 * normalisation fields of the view are ignored (they are recomputed from the training data given to
 * egx_gp_create and must agree).  All eight pointers are required. */
int32_t egx_gp_set_inner(egx_gp *gp, const egx_gp_inner_view *view);

/* ---- kernel-level entry points ---------------------------------------------
 * The CorrelationModel::value seam (correlation_models.rs:19-58) fused with
 * DiffMatrix (utils.rs:80-104) and the scatter loop (algorithm.rs:997-1001):
 * r (n x n, full symmetric, diagonal 1+nugget) straight from normalised x.
 * theta is the per-input-dimension scale vector (length d, w = I). */
int32_t egx_corr_matrix(int32_t corr, const double *xnorm, int64_t n, int64_t d,
                        const double *theta, double nugget, double *r /*n*n*/);
/* _compute_correlation (algorithm.rs:372-380): r (m x n) between normalised
 * query points and normalised training points. */
int32_t egx_cross_corr(int32_t corr, const double *xq_norm, int64_t m, const double *xt_norm,
                       int64_t n, int64_t d, const double *theta, double *r /*m*n*/);
/* cholesky() (algorithm.rs:1004; LAPACK dpotrf with the blas feature :1077):
 * a (n x n, symmetric, lower triangle read) -> lower factor in place (upper
 * zeroed).  *info = 0, or 1-based index of the first non-positive pivot. */
int32_t egx_potrf(double *a, int64_t n, int32_t *info);

/* ==== multi-GPU theta sweep (BASELINE config 4) ================================
 * Replaces the rayon multistart of crates/gp/src/algorithm.rs:928-945 (independent likelihood evaluations, one
 * per start, arg-min reduce :942-945) and the serial expert loop of crates/moe/src/algorithm.rs:167-177 at node
 * scale: ONE PROCESS PER GPU, the training set replicated on every rank (4 MiB at n = 16384, d = 32), candidate
 * k evaluated by rank k mod world through egx_gp_likelihood_batch, and one RCCL all-gather (ncclAllGather over xGMI)
 * of {likelihood f64, status} -- 16 B per candidate -- so that every rank returns the full (k) result.
 * RCCL (librccl.so.1) is bound at run time on the first egx_sweep_* call; a single-GPU user never loads it.
 *
 * Rendezvous: rank 0 calls egx_sweep_unique_id and hands the EGX_SWEEP_ID_BYTES bytes to the other ranks by any
 * out-of-band channel (MPI_Bcast, a file, torch.distributed's store ...); all ranks then call egx_sweep_create
 * collectively.  world == 1 with nccl_id == NULL needs no RCCL at all; world == 1 WITH an id builds a one-rank
 * communicator (the same code path as world > 1). */
#define EGX_SWEEP_ID_BYTES 128 /* sizeof(ncclUniqueId) */
typedef struct egx_sweep egx_sweep;
int32_t egx_sweep_unique_id(void *id_out /*EGX_SWEEP_ID_BYTES*/);
/* cfg / x / y / n / d as egx_gp_create (cfg->device selects this rank's GPU; n_workspaces is raised to 2). */
int32_t egx_sweep_create(const egx_gp_config *cfg, const double *x, const double *y, int64_t n, int64_t d,
                         const void *nccl_id /*EGX_SWEEP_ID_BYTES or NULL*/, int32_t rank, int32_t world,
                         egx_sweep **out);
void egx_sweep_destroy(egx_sweep *sw);
/* this rank's GP handle (owned by the sweep): finalize / predict with the winning theta on it */
egx_gp *egx_sweep_handle(egx_sweep *sw);
/* rccl_ranks = ranks of the RCCL communicator (0 when none was built), rccl_version = ncclGetVersion code */
int32_t egx_sweep_info(const egx_sweep *sw, int32_t *rank, int32_t *world, int32_t *rccl_ranks, int32_t *rccl_version,
                       int64_t *n_allgathers);
/* COLLECTIVE: every rank passes the same thetas (k x theta_len); lkh / status (k) are complete on every rank.
 * Semantics per candidate as egx_gp_likelihood_batch (status is the value channel, failures are not errors). */
int32_t egx_sweep_likelihood(egx_sweep *sw, const double *thetas, int64_t k, int64_t theta_len, double *lkh /*k*/,
                             int32_t *status /*k*/);
/* Assignment of candidates to ranks for the following egx_sweep_likelihood calls: 0 = static (candidate c -> rank
 * c mod world; the default), 1 = dynamic (ranks pull the next candidate from a node-wide counter in POSIX shared
 * memory as their workspaces free up: candidates that are not positive definite return ~10x sooner than the others,
 * SURVEY 8e).  The results are identical either way (every evaluation is deterministic and independent of the rank
 * that runs it).  Every rank must select the same mode.  EGX_ERR_UNSUPPORTED when the shared memory is unavailable. */
int32_t egx_sweep_set_assignment(egx_sweep *sw, int32_t dynamic);
/* Balance of the last egx_sweep_likelihood: candidates evaluated by every rank (world entries, NULL = skip) and the
 * wall time this rank spent in its own evaluations (seconds, NULL = skip). */
int32_t egx_sweep_last_balance(const egx_sweep *sw, int64_t *per_rank /*world*/, double *local_eval_s);
/* FAILURE SAFETY of the collectives: a rank whose local work fails (HIP error, out of memory, ...) still takes part
 * in the all-gather with a poisoned payload and returns its own error afterwards; every other rank returns
 * EGX_ERR_PEER (the candidates of the failed rank come back with status EGX_STATUS_RANK_FAILED, all others are
 * valid).  A peer that never arrives is given EGX_SWEEP_TIMEOUT_S seconds (environment, default 1800), then the
 * communicator is aborted and the call returns EGX_ERR_PEER instead of blocking for ever. */
/* COLLECTIVE helper for the mixture-of-experts path (expert e on rank e mod world): recv (world x count) <- the
 * concatenation over ranks of send (count), e.g. per-expert mean / variance vectors before the recombination of
 * crates/moe/src/algorithm.rs:670-685. */
int32_t egx_sweep_allgather(egx_sweep *sw, const double *send, int64_t count, double *recv /*world*count*/);

/* COLLECTIVE tuned fit: egx_gp_fit with the starts sharded over the ranks (start s on rank s mod world; the reference runs
 * them as rayon tasks on one host, crates/gp/src/algorithm.rs:928-945).  Every rank passes the same arguments; one
 * all-gather carries each start's (objective, evaluations, minimiser); every rank reduces in start order (:942-945) and
 * finalizes ITS replica at the winner, so afterwards egx_sweep_handle(sw) is the same fitted model on every rank -- bit
 * for bit the model egx_gp_fit returns on one GPU (an evaluation gives the same bits wherever it runs).  n_evals_out: the
 * evaluations of all starts.  Failure semantics as egx_sweep_likelihood. */
int32_t egx_sweep_fit(egx_sweep *sw, const double *theta0s /*n_starts x h*/, int64_t n_starts, const double *lo,
                      const double *hi, int64_t bounds_len, int64_t max_eval, int64_t *n_evals_out);

/* ---- mixture-of-experts recombination (BASELINE config 5) ----------------------------------
 * GpMixture::predict_smooth / predict_var_smooth (crates/moe/src/algorithm.rs:411-423, 670-685):
 *     val = sum_e p_e y_e,  var = sum_e p_e^2 v_e        over all m points, every expert sees every point;
 * GpMixture::predict_hard / predict_var_hard (:879-935): a point is answered by the expert of its cluster,
 * argmax_e p_e (first maximum) -- routed once, ONE batched call per expert (the reference calls the expert per row).
 * `experts` are this process' fitted handles, expert_ids[e] in [0, n_experts) their columns in `probas`
 * (m x n_experts row-major: the responsibilities GaussianMixture::predict_probas returns, gaussian_mixture.rs:114-121).
 * xq is (m x d) in ORIGINAL units.  val / var (m): either may be NULL.
 * sw == NULL: single process, every expert is local.  sw != NULL: COLLECTIVE -- every rank passes the same probas /
 * xq and ITS OWN experts (expert e on rank e mod world in config 5; a rank may own none); the partial sums are exchanged
 * by one all-gather on the sweep's communicator and added in rank order, so every rank returns the same bits.  Failure
 * safety as for egx_sweep_likelihood (a failing rank still arrives, the others return EGX_ERR_PEER). */
int32_t egx_moe_predict_valvar(egx_sweep *sw, egx_gp *const *experts, const int32_t *expert_ids, int64_t n_local,
                               int64_t n_experts, const double *probas /*m*n_experts*/, const double *xq /*m*d*/,
                               int64_t m, int64_t d, int32_t smooth, double *val /*m*/, double *var /*m*/);

/* Responsibilities of a fitted Gaussian mixture at m points: GaussianMixture::predict_probas (crates/moe/src/
 * gaussian_mixture.rs:114-121, with compute_log_prob_resp :231-251 and compute_log_gaussian_prob :253-283) -- the `probas`
 * egx_moe_predict_valvar consumes.  weights (k), means (k x d), precisions_chol (k x d x d row-major: (chol(cov_c)^-1)^T as
 * the reference stores it, :182-205; egx_gmx_precisions_chol builds it from covariances (k x d x d), EGX_ERR_LINALG for a
 * covariance that is not positive definite), heaviside_factor > 0 (:105-110: scales the precision factors by its power
 * -1/2; 1 = none).  xq (m x d) in original units, probas (m x k).  One cluster: all ones (:115-116).  Runs on `device`
 * (< 0: the calling thread's current device); the d x d factorisations of egx_gmx_precisions_chol are host arithmetic. */
int32_t egx_gmx_precisions_chol(const double *covariances, int64_t k, int64_t d, double *precisions_chol);
int32_t egx_gmx_predict_probas(int32_t device, const double *weights, const double *means, const double *precisions_chol,
                               int64_t k, int64_t d, double heaviside_factor, const double *xq, int64_t m, double *probas);

/* Training of that mixture: full-covariance EM on data (n x dim, row-major; egobox-moe passes the joined [x, y]) with
 * n_runs restarts in lock-step on the GPU -- GaussianMixtureModel::params(n_clusters).n_runs(20).fit(..), crates/moe/src/
 * algorithm.rs:120-123 and clustering.rs:126-130.  Restart r starts from init_means[r] (k x dim): iteration 0 assigns every
 * row to its nearest initial mean (squared Euclidean distance, ties to the lowest cluster) and runs the M-step on these
 * one-hot responsibilities; every later iteration is an E-step and an M-step (nk = sum resp + 10 eps, weights = nk / sum nk,
 * covariance = weighted scatter about the new mean + reg_covar I), its lower bound the mean log-prob-norm of the E-step.  A
 * restart stops when |lb - lb_prev| < tol (status 0) or after max_iter iterations (status 1, still a candidate); a
 * covariance that is not positive definite or a value that is not finite fails that restart alone (status 2, excluded, its
 * lower bound NaN).  The result is the restart with the greatest final lower bound (the lowest index among equals).  A
 * restart computes the same bits alone and in any batch.  dim <= 36 and n_clusters <= 16, beyond: EGX_ERR_INVALID_VALUE, as
 * for n < n_clusters, a value of data / init_means that is not finite, n_runs < 1 (all checked before the device is
 * touched).  EGX_ERR_LINALG when every restart failed (the per-restart outputs are filled).  The all_* outputs (every
 * restart's parameters; those of a failed restart are not meaningful) may be NULL. */
typedef struct {
    int32_t n_clusters, n_runs, max_iter, device; /* device < 0: the calling thread's current device */
    double tol, reg_covar;
} egx_gmm_config;
void egx_gmm_config_default(egx_gmm_config *cfg); /* n_clusters 1, n_runs 20, max_iter 100, tol 1e-3, reg_covar 1e-6, device -1 */
int32_t egx_gmm_fit(const egx_gmm_config *cfg, const double *data, int64_t n, int32_t dim,
                    const double *init_means /*n_runs*k*dim*/, double *weights /*k*/, double *means /*k*dim*/,
                    double *covariances /*k*dim*dim*/, double *lower_bounds /*n_runs*/, int32_t *n_iters /*n_runs*/,
                    int32_t *statuses /*n_runs*/, int32_t *best_run, double *all_weights /*n_runs*k*/,
                    double *all_means /*n_runs*k*dim*/, double *all_covariances /*n_runs*k*dim*dim*/);
/* The same training for rows up to 128 wide: arguments, outputs, statuses and errors are exactly those of egx_gmm_fit, with
 * dim <= 128 and n_clusters <= 16 (beyond: EGX_ERR_INVALID_VALUE, checked before the device is touched).  The two products
 * per row that cost O(dim^2) run on the FP64 matrix unit; narrow rows are taken too, and agree with egx_gmm_fit to rounding
 * (the sums have another order, so not to the bit).  A restart computes the same bits alone and in any batch here as well.
 * The mixture's x-derivatives and the infill handles on mixtures still need 3 d + k <= 320 (below). */
int32_t egx_gmm_fit_wide(const egx_gmm_config *cfg, const double *data, int64_t n, int32_t dim,
                         const double *init_means /*n_runs*k*dim*/, double *weights /*k*/, double *means /*k*dim*/,
                         double *covariances /*k*dim*dim*/, double *lower_bounds /*n_runs*/, int32_t *n_iters /*n_runs*/,
                         int32_t *statuses /*n_runs*/, int32_t *best_run, double *all_weights /*n_runs*k*/,
                         double *all_means /*n_runs*k*dim*/, double *all_covariances /*n_runs*k*dim*dim*/);

/* d p_c(x) / d x of those responsibilities: GaussianMixture::predict_probas_derivatives (gaussian_mixture.rs:127-170),
 * dprobas is (m x k x d) row-major; on the device, one lane per point (needs 3 d + k <= 320). */
int32_t egx_gmx_predict_probas_derivatives(int32_t device, const double *weights, const double *means,
                                           const double *precisions_chol, int64_t k, int64_t d, double heaviside_factor,
                                           const double *xq, int64_t m, double *dprobas /*m*k*d*/);
/* The typed forms of the two stateless mixture calls: the same arguments plus a spec whose unfolded dimension is d; the points are
 * cast (egx_mixint_cast) on the device as the kernel stages them.  nx == 0 is the untyped call. */
int32_t egx_gmx_predict_probas_mixint(int32_t device, const double *weights, const double *means, const double *precisions_chol,
                                      int64_t k, int64_t d, double heaviside_factor, const double *xq, int64_t m,
                                      double *probas /*m*k*/, const egx_xtype *xt, int32_t nx);
int32_t egx_gmx_predict_probas_derivatives_mixint(int32_t device, const double *weights, const double *means,
                                                  const double *precisions_chol, int64_t k, int64_t d, double heaviside_factor,
                                                  const double *xq, int64_t m, double *dprobas /*m*k*d*/, const egx_xtype *xt,
                                                  int32_t nx);
/* x-gradients of the mixture's mean and variance: GpMixture::predict_gradients_smooth / predict_var_gradients_smooth
 * (crates/moe/src/algorithm.rs:691-783:  sum_e p_e grad y_e + p'_e y_e ,  sum_e p_e^2 grad v_e + 2 p_e p'_e v_e) and
 * predict_gradients_hard / predict_var_gradients_hard (:942-1010: the expert of argmax_e p_e) -- what EGO's infill
 * optimiser asks of a mixture surrogate.  Arguments and sharding as egx_moe_predict_valvar (a rank passes its own
 * experts; one all-gather of the partial (m x d) sums, added in rank order); dprobas (m x n_experts x d, from
 * egx_gmx_predict_probas_derivatives) is read in smooth mode only and may be NULL for a single expert.  grad_val /
 * grad_var are (m x d) row-major in original units; either may be NULL.  Every expert gets ONE batched call per
 * quantity (the reference calls it once per row). */
int32_t egx_moe_predict_valvar_gradients(egx_sweep *sw, egx_gp *const *experts, const int32_t *expert_ids, int64_t n_local,
                                         int64_t n_experts, const double *probas /*m*n_experts*/,
                                         const double *dprobas /*m*n_experts*d*/, const double *xq /*m*d*/, int64_t m,
                                         int64_t d, int32_t smooth, double *grad_val /*m*d*/, double *grad_var /*m*d*/);

/* ---- measurement ------------------------------------------------------------
 * HIP-event durations (ms) of the stages of the most recent likelihood /
 * finalize call on workspace 0, measured on the stream the kernels ran on. */
typedef struct {
    double corr_build_ms; /* K1 */
    double potrf_ms;      /* K3 incl. fused forward solves (K4) */
    double potrf_syrk_ms; /* sum of the HIP-event durations of the big-tile trailing-update launches */
    double solve_ms;      /* gamma back-substitution */
    double host_ms;       /* GLS / QR / reductions on the host */
    double total_ms;
    int64_t potrf_flops;  /* n^3/3 algorithmic */
    int64_t corr_bytes;   /* 8*n*d + 8*n(n+1)/2 algorithmic */
    int64_t syrk_launches; /* number of big-tile (128x128, 512-thread) trailing-update launches timed */
    int64_t syrk_flops;    /* their algorithmic flops: sum of 2*K*ncols*(ncols+1)/2 (lower triangle) */
} egx_timings;
int32_t egx_gp_last_timings(const egx_gp *gp, egx_timings *t);

/* self-test of the FP64 MFMA fragment layout (16x16x4): returns max abs error of
 * a 16x16x16 product computed with v_mfma_f64_16x16x4_f64 vs the host. */
int32_t egx_mfma_probe(double *max_abs_err);


/* ==== sparse Gaussian process (FITC / VFE), SURVEY 8f rank 4 =================================
 * SparseGaussianProcess / SgpValidParams, crates/gp/src/sparse_algorithm.rs:145-168, 422-831 and
 * sparse_parameters.rs.  Works on RAW x / y (the reference does not normalise here) with a zero trend;
 * parameters are theta (d, or 1 broadcast), the process variance sigma2 and the homoscedastic noise variance.
 * z are the nz inducing points (Inducings::Located; a Randomized(n) draw is the caller's shuffle of x). */
typedef struct egx_sgp egx_sgp;
typedef enum { EGX_SGP_FITC = 0, EGX_SGP_VFE = 1 } egx_sgp_method; /* SparseMethod, sparse_parameters.rs:59-67 */
typedef struct {
    int32_t corr;   /* egx_corr */
    int32_t method; /* egx_sgp_method */
    double nugget;  /* added to diag(Kmm); default 100 * f64::EPSILON */
    int32_t device; /* HIP ordinal, -1 = current */
} egx_sgp_config;
void egx_sgp_config_default(egx_sgp_config *cfg);
int32_t egx_sgp_create(const egx_sgp_config *cfg, const double *x /*n*d*/, const double *y /*n*/, int64_t n, int64_t d,
                       const double *z /*nz*d*/, int64_t nz, egx_sgp **out);
void egx_sgp_destroy(egx_sgp *sgp);
int32_t egx_sgp_dims(const egx_sgp *sgp, int64_t *n, int64_t *d, int64_t *nz);
/* reduced_likelihood (fitc :695-766 / vfe :769-831) at given parameters; status as for egx_gp_likelihood
 * (1: Kmm or I + V diag(beta) V^T not positive definite -- the reference unwraps; 4: NaN / non-positive parameters) */
int32_t egx_sgp_likelihood(egx_sgp *sgp, const double *theta, int64_t theta_len, double sigma2, double noise,
                           double *lkh, int32_t *status);
/* keep the state of one evaluation resident = a fit at fixed parameters */
int32_t egx_sgp_finalize(egx_sgp *sgp, const double *theta, int64_t theta_len, double sigma2, double noise);
/* SgpValidParams::fit :488-650: multistart derivative-free maximisation over log10 [theta.., sigma2, (noise)];
 * params0s (n_starts x np), lo / hi (np), np = d + 1 + (estimate_noise != 0); maxeval = clamp(10 d, 25, max_eval).
 * An evaluation that fails with a HIP or argument error ends the fit at once with that code. */
int32_t egx_sgp_fit(egx_sgp *sgp, const double *params0s, int64_t n_starts, const double *lo, const double *hi,
                    int32_t estimate_noise, double noise_fixed, int64_t max_eval, int64_t *n_evals_out);
/* No counterpart in the reference (it tunes the sparse model derivative-free): the likelihood of egx_sgp_likelihood -- the same
 * bits -- and its CLOSED-FORM gradient, grad (d + 2) = dL/dtheta_0..d-1 (of the broadcast theta when theta_len == 1),
 * dL/dsigma2, dL/dnoise (VFE: dL/dnoise is exactly 0 while noise <= nugget, where the likelihood does not depend on it).
 * Status and failure as egx_sgp_likelihood; whenever *status != 0, *lkh = -inf and grad is zeros.  Like egx_sgp_likelihood it
 * un-fits the handle.  The first call allocates one more n_pad x z_pad buffer, which the handle keeps. */
int32_t egx_sgp_likelihood_grad(egx_sgp *sgp, const double *theta, int64_t theta_len, double sigma2, double noise, double *lkh,
                                double *grad /* d + 2: dL/dtheta_0..d-1, dL/dsigma2, dL/dnoise */, int32_t *status);
/* egx_sgp_fit by a projected L-BFGS on x = log10(params) driven by egx_sgp_likelihood_grad: the same parameter layout, box and
 * checks; the starts run one after the other, the best wins (the first on ties), one keeping evaluation follows.
 * max_iter < 1: 50 iterations per start.  *n_evals_out counts likelihood + gradient evaluations. */
int32_t egx_sgp_fit_lbfgs(egx_sgp *sgp, const double *params0s, int64_t n_starts, const double *lo, const double *hi,
                          int32_t estimate_noise, double noise_fixed, int64_t max_iter, int64_t *n_evals_out);
/* No counterpart in the reference (its inducing points never move): egx_sgp_likelihood_grad -- *lkh and grad bit for bit -- and,
 * from the same pair weights, the gradient in the inducing points, grad_z (nz x d, row-major like z) = dL/dz_{j,k}.  Under the
 * absolute exponential a coordinate where z_j meets a training point or another inducing point (the kernel's kink) contributes 0,
 * what the central difference gives there.  Whenever *status != 0, grad_z is zeros too.  Un-fits the handle like its sibling. */
int32_t egx_sgp_likelihood_grad_z(egx_sgp *sgp, const double *theta, int64_t theta_len, double sigma2, double noise, double *lkh,
                                  double *grad /* d + 2 */, double *grad_z /* nz*d */, int32_t *status);
/* Replace the inducing points by z (the same nz; finite values, else EGX_ERR_INVALID_VALUE and the handle stays as it was).
 * Un-fits the handle: finalize or fit again before predicting.  egx_sgp_get_inducings returns the current points. */
int32_t egx_sgp_set_inducings(egx_sgp *sgp, const double *z /*nz*d*/);
int32_t egx_sgp_get_inducings(egx_sgp *sgp, double *z /*nz*d*/);
/* KPLS dimension reduction of the sparse model (SgpValidParams::fit computes the PLS rotations on the raw (x, y) and carries
 * w_star through compute_k, fitc, vfe, predict* and sample: sparse_algorithm.rs:429-455, 222-229, 659-687).  w is d x h row-major,
 * 1 <= h <= d, finite values; otherwise EGX_ERR_INVALID_VALUE ("`kpls_dim` canot be 0!", "Dimension reduction ... should be
 * smaller than actual training input dimensions ...") and the handle stays as it was.  An all-zero w is accepted (the reference
 * passes it on a constant PLS residual); evaluations then report their status as values.  Un-fits the handle.  w == NULL with
 * h == 0 clears the weights: every output is again bit for bit that of a handle that never had any.  While weights are set
 *   - theta has h components: theta_len is 1 or h in egx_sgp_likelihood / _finalize / _likelihood_grad / _likelihood_grad_z
 *     ("theta should be either 1-dim or dim of xtrain (w_star.ncols()), got ..."), egx_sgp_get_state writes h thetas;
 *   - grad of egx_sgp_likelihood_grad / _grad_z is h + 2 long: dL/dtheta_0..h-1, dL/dsigma2, dL/dnoise;
 *   - egx_sgp_fit / _fit_lbfgs / _fit_lbfgs_z take np = h + 1 + (estimate_noise != 0), and the evaluation budget of egx_sgp_fit
 *     is clamp(10 h, 25, max_eval);
 *   - grad_z, the inducing points and their box stay nz x d / d: the points live in the input space;
 *   - the x-gradients need d * (hcols + 5) <= 20480 with hcols = h for the Matern correlations and 1 otherwise
 *     (the squared and the absolute exponential collapse theta and w into one coefficient per input).
 * egx_sgp_get_w_star writes *h (d when no weights are set) and, where w != NULL and weights are set, the d x h weights. */
int32_t egx_sgp_set_w_star(egx_sgp *sgp, const double *w /*d*h row-major, or NULL*/, int64_t h);
int32_t egx_sgp_get_w_star(egx_sgp *sgp, double *w /*d*h or NULL*/, int64_t *h);

/* ---- PLS rotations on the device (the weights w_star of KPLS) ------------------------------------------------------------------
 * The x rotations W (P^T W)^-1 (d x k, row-major) of a PLS1 regression of y on x, both centred and scaled to unit variance
 * (ddof = 1; a column of zero spread is scaled by 1 and gets a zero row): what linfa-pls' PlsRegression::params(k).fit(..)
 * .rotations().0 gives the reference (algorithm.rs:843-855) and egobox_amd/kpls.py restates on the host.  The signs of the columns
 * are those of the NIPALS recursion; every consumer reads |w| or w^2.
 *
 * Two launches read the data: the column means, then the centred Gram matrix of [x | y] on the FP64 matrix unit, the rows split
 * into chunks whose partial sums are added in chunk order (a third, tiny launch).  The O(d^2 k) deflation runs on the host from
 * that matrix.  No atomics: the result depends on (x, y, n, d, k) alone -- the same bits on every call, for every leading
 * dimension of the device copy, from egx_pls_rotations and from egx_sgp_compute_w_star.
 *
 * *status = 0, or 1 with w all zeros where the response (or the residual left by an earlier component) is constant up to
 * rounding -- where the reference hands zeros on after PowerMethodConstantResidualError.  status may be NULL.
 *
 * Checked before a device is touched, EGX_ERR_INVALID_VALUE: NULL x / y / w; k < 1 ("`kpls_dim` canot be 0!"); k > d ("Dimension
 * reduction k should be smaller than actual training input dimensions d"); n < 2; d < 1; a non-finite entry of x or y.
 * Then EGX_ERR_NO_DEVICE without a device, EGX_ERR_INVALID_VALUE for a device ordinal out of range (device < 0: the current one). */
int32_t egx_pls_rotations(int32_t device, const double *x /*n*d row-major*/, const double *y /*n*/, int64_t n, int64_t d, int64_t k,
                          double *w /*d*k row-major*/, int32_t *status);
/* The same rotations from the training set the handle holds on the device (no upload), installed exactly as
 * egx_sgp_set_w_star(sgp, w, k) installs them: the handle is un-fitted, theta has k components, egx_sgp_get_w_star returns the
 * weights.  A constant response installs zeros (accepted as from egx_sgp_set_w_star; evaluations then report their status as
 * values); egx_sgp_get_w_star shows them.  k < 1 / k > d: EGX_ERR_INVALID_VALUE with the messages above, and the handle stays
 * as it was (a NULL handle is refused after k < 1, as egx_sgp_set_w_star does). */
int32_t egx_sgp_compute_w_star(egx_sgp *sgp, int64_t k);
/* A measurement aid (tools/pls_bench.py): the launches of egx_sgp_compute_w_star on the handle's data, once, between two HIP
 * events; *ms their elapsed time.  The handle is left as it was. */
int32_t egx_sgp_pls_launch_ms(egx_sgp *sgp, double *ms);
/* How the two launches above cut an (n x d) training set (host only, no device; csrc/pls_host.h is the one place that decides):
 * chunk c < n_chunks owns the rows [c chunk_rows, min(n, (c + 1) chunk_rows)) -- every row once, no chunk empty; chunk_rows is a
 * multiple of 64 and does not shrink as n grows.  [x | y] has d + 1 columns in `tiles` tiles of 16; out_tiles = the 16 x 16
 * tiles of the lower triangle, the only ones computed; a workgroup owns one of `blocks` 64 x 64 blocks (block_side per side) of
 * one chunk.  None of them shrinks as d grows.  n < 1, d < 1 or out == NULL: EGX_ERR_INVALID_VALUE. */
typedef struct {
    int64_t n, d;
    int64_t chunk_rows, n_chunks;
    int64_t tiles, out_tiles;
    int64_t block_side, blocks;
} egx_pls_plan;
int32_t egx_pls_get_plan(int64_t n, int64_t d, egx_pls_plan *out);
/* egx_sgp_fit_lbfgs (phase 1, exactly), then ONE more projected L-BFGS from its winner over [log10 params (np), u (nz*d)],
 * u = (z - z_lo) / (z_hi - z_lo) in [0, 1]: the inducing points move with the parameters, driven by egx_sgp_likelihood_grad_z.
 * z_lo / z_hi (d each) box every inducing point; NULL: the per-column min / max of the training x.  A column with z_hi == z_lo
 * is held where it is; points outside the box start from its nearest face.  An evaluation that fails (two points merged) counts
 * as +inf and the line search backs off.  Phase 2 is kept only where it ends at a strictly higher likelihood than phase 1, so
 * the result is never worse than egx_sgp_fit_lbfgs; the accepted points stay on the handle (egx_sgp_get_inducings) and one keeping
 * evaluation follows.  max_iter_z == 0: no phase 2, the handle is left bit for bit as egx_sgp_fit_lbfgs leaves it; < 0: 50.
 * *n_evals_out counts the evaluations of both phases. */
int32_t egx_sgp_fit_lbfgs_z(egx_sgp *sgp, const double *params0s, int64_t n_starts, const double *lo, const double *hi,
                            int32_t estimate_noise, double noise_fixed, int64_t max_iter, const double *z_lo /*d or NULL*/,
                            const double *z_hi /*d or NULL*/, int64_t max_iter_z, int64_t *n_evals_out);
/* SparseGaussianProcess::predict :237-241, predict_var :245-257 (clamp at 1e-15, + noise) */
int32_t egx_sgp_predict(egx_sgp *sgp, const double *xq, int64_t m, double *y /*m*/);
int32_t egx_sgp_predict_var(egx_sgp *sgp, const double *xq, int64_t m, double *var /*m*/);
/* Mean and variance of the same points in one call: one upload, one launch sequence, one synchronisation; the same bits as
 * the two calls above.  (The mean keeps its own kernel, which evaluates r(xq, z) on the fly: a row-dot of the K(xq, z) block
 * formed for the variance would have to repeat that kernel's summation order to keep the bits, and was not attempted.) */
int32_t egx_sgp_predict_valvar(egx_sgp *sgp, const double *xq, int64_t m, double *y /*m*/, double *var /*m*/);
/* ANALYTIC x-gradients (what a SgpSurrogate shim binds for predict_gradients / predict_var_gradients /
 * predict_valvar_gradients; the reference takes central differences of predict / predict_var, :298-336, which these are the
 * limit of).  With kx = sigma2 r(x, z), W / vec the WoodburyData of egx_sgp_get_state:
 *   d mean / d x_k = sigma2 sum_j vec_j d r(x, z_j) / d x_k
 *   d var  / d x_k = -2 sigma2 sum_j (W kx)_j d r(x, z_j) / d x_k  where sigma2 - kx^T W kx >= 1e-15, and exactly 0 where
 *                    predict_var clamps (the derivative of the clamped function, as the central difference gives there).
 * xq (m x d) in the units of the training inputs; m = 0 succeeds and does nothing; EGX_ERR_UNSUPPORTED when 6 d > 20480
 * (d * (hcols + 5) > 20480 with KPLS weights, egx_sgp_set_w_star). */
int32_t egx_sgp_predict_gradients(egx_sgp *sgp, const double *xq, int64_t m, double *grad /*m*d*/);
int32_t egx_sgp_predict_var_gradients(egx_sgp *sgp, const double *xq, int64_t m, double *grad /*m*d*/);
int32_t egx_sgp_predict_valvar_gradients(egx_sgp *sgp, const double *xq, int64_t m, double *grad_y /*m*d*/,
                                         double *grad_var /*m*d*/);
/* SparseGaussianProcess::sample :338-362 AS THE REFERENCE DEFINES IT: traj (m x n_traj) = predict(xq) 1^T + F Z with
 * F F^T = sigma2 r(xq, xq) (+ tau I): the PRIOR covariance, without the noise and without the Woodbury term.  That is a
 * quirk of the reference, kept on purpose: the trajectories scatter around the posterior mean with the prior's spread.
 * method, seed, z, tau_out, the normals, the EGX_SAMPLE_PSD jitter rule and the deviation from sample_eig are those of
 * egx_gp_sample (above); nothing m x m leaves the device. */
int32_t egx_sgp_sample(egx_sgp *sgp, const double *xq, int64_t m, int64_t n_traj, int32_t method, uint64_t seed,
                       const double *z /*m*n_traj or NULL*/, double *traj /*m*n_traj*/, double *tau_out /*1 or NULL*/);
/* fitted state: theta (d), sigma2, noise, likelihood, WoodburyData vec (nz) and inv (nz*nz) :32-36; NULL = skip */
int32_t egx_sgp_get_state(egx_sgp *sgp, double *theta, double *sigma2, double *noise, double *likelihood,
                          double *w_vec, double *w_inv);

/* ---- EGO's infill criterion on fitted models -------------------------------------------------------------------------
 * What EGO asks of its surrogates, "where next?" (crates/ego/src): the objective its infill optimiser MINIMISES,
 *   obj(x) = -crit(x) / scale                    crit: criteria/ei.rs:22-170 (EI, LogEI), criteria/wb2.rs:21-49 (WB2, WB2S)
 *   obj(x) * pofs(x)  (EI, WB2, WB2S)  or  obj(x) - logpofs(x)  (LogEI)   with constraint models (cstr_infill = true):
 *                                                utils/cstr_pof.rs, solver/solver_computations.rs:356-475
 * and its x-gradient, for m points per call, from ONE objective model and n_cstr >= 0 constraint models (dense GPs, all
 * fitted, same d, same device; n may differ) -- or, through egx_infill_create_mix below, from surrogates that are mixtures
 * of such GPs.  The models are BORROWED: they must outlive the handle, and a call always reads
 * their CURRENT fitted state -- and their CURRENT xtypes (egx_gp_set_xtypes), checked at creation and again at every call: all
 * models (every expert of every surrogate) carry the same spec, or none does, else EGX_ERR_INVALID_VALUE naming the two.  With
 * xtypes every point of every call below -- egx_infill_eval, _eval_cstr, _eval_experts, _scaling, and the trial points
 * egx_infill_optimize / _optimize_cstr generate themselves -- is cast on the device before it is evaluated, the mixtures'
 * responsibilities included; the optimisers work in the unfolded continuous box, x_best is the evaluated point as proposed (fold
 * it with egx_mixint_to_discrete) and *f_best is bit for bit egx_infill_eval there.  feasibility == 0 replaces obj by -1 (0 for LogEI) and its gradient by 0 (:410-416, 441-466).
 * The reference evaluates this one point at a time with 2 (1 + n_cstr) predict calls per evaluation; here a call is one
 * upload, one launch sequence per 128-point tile and model, one synchronisation, and nothing is computed on the host.
 *
 * A point's results do not depend on its companions: value[i], grad[i, :] and the parts of point i are bit for bit the same
 * whether the point is evaluated alone, at another position, or among others; value is bit for bit the same with and
 * without grad.
 *
 * Four DEVIATIONS from the reference (egobox_amd/csrc/infill_math.h):
 *   1. log_ei_helper (utils/logei_helper.rs) is exact on the whole line: below u = -20 the asymptotic series replaces
 *      exp(z^2) erfc(z), which leaves double range near u = -37.6 in the reference (wrong or NaN down to u = -1e6).
 *   2. pof_grad (cstr_pof.rs:42-43) is the derivative of Phi((tol - mu) / sigma) for every tol, not only for tol = 0.
 *   3. the gradient uses the same sigma_weight as the value (solver_computations.rs:387-391 passes None).
 *   4. the gradient of the upper trust bound of a constraint (egx_infill_eval_cstr under EGX_CSTR_UTB) uses every coordinate's
 *      own d var / d x_c; upper_trust_bound_cstr (:242) takes the first coordinate's for all of them.
 * NaN in a point: value = +inf, gradient 0, for that point only (solver_infill_optim.rs:87-90).  m = 0 succeeds. */
typedef struct egx_infill egx_infill;
typedef enum { EGX_INFILL_EI = 0, EGX_INFILL_LOG_EI = 1, EGX_INFILL_WB2 = 2, EGX_INFILL_WB2S = 3 } egx_infill_criterion;
typedef struct {
    int32_t criterion;   /* egx_infill_criterion; default EGX_INFILL_LOG_EI */
    int32_t feasibility; /* 0: no feasible point known yet (see above); default 1 */
    double fmin;         /* current best objective value */
    double sigma_weight; /* k in sigma_k = k sqrt(var) (EI, WB2, WB2S; LogEI ignores it, as the reference); default 1 */
    double scale_ic;     /* WB2S's factor on EI (wb2.rs:29); ignored by the other criteria; default 1 */
    double scale;        /* obj = -crit / scale; default 1 */
} egx_infill_config;
void egx_infill_config_default(egx_infill_config *cfg);
/* EGX_ERR_INVALID_VALUE naming the model's index (0 = objective, 1.. = constraints) when d or the device differ;
 * EGX_ERR_NOT_FITTED when a model is not fitted (here and in every later call). */
int32_t egx_infill_create(const egx_infill_config *cfg, egx_gp *obj_model, egx_gp *const *cstr_models /*n_cstr*/,
                          const double *cstr_tols /*n_cstr*/, int32_t n_cstr, egx_infill **out);
void egx_infill_destroy(egx_infill *h);
/* between EGO iterations, without rebuilding the handle */
int32_t egx_infill_set_params(egx_infill *h, double fmin, double sigma_weight, double scale_ic, double scale,
                              int32_t feasibility);
int32_t egx_infill_get_params(egx_infill *h, egx_infill_config *cfg);
/* what the criterion was computed FROM, model-major (model 0 = objective): any pointer may be NULL (skipped) */
typedef struct {
    double *mean;      /* (1 + n_cstr) * m     */
    double *var;       /* (1 + n_cstr) * m     */
    double *grad_mean; /* (1 + n_cstr) * m * d */
    double *grad_var;  /* (1 + n_cstr) * m * d */
} egx_infill_parts;
/* xq (m x d) in ORIGINAL units.  grad == NULL skips the gradient work (unless parts asks for gradients); the cached C^-T
 * the gradients need is built on the first gradient call after a fit -- values need the factor alone. */
int32_t egx_infill_eval(egx_infill *h, const double *xq, int64_t m, double *value /*m*/, double *grad /*m*d or NULL*/,
                        const egx_infill_parts *parts /*or NULL*/);
/* compute_scaling (solver_computations.rs:132-193) on the caller's points (the reference draws min(100 d, 1000) LHS points):
 * scale_ic = compute_wb2s_scale (wb2.rs:67-88; 1 unless the criterion is WB2S), scale = compute_infill_obj_scale (:297-351),
 * scale_cstr[j] = compute_cstr_scales (utils/misc.rs:10-28; may be NULL).  One values-only pass over the points.  The criterion's
 * terms are formed on the device with the text of egx_infill_eval: scale is bit for bit the largest |value| egx_infill_eval
 * returns for these points at scale = 1 (a NaN / infinite objective counting as 1.0 before the feasibility factor).  scale_ic
 * and scale are stored in the handle and returned (either pointer may be NULL). */
int32_t egx_infill_scaling(egx_infill *h, const double *pts /*npts*d*/, int64_t npts, double *scale_ic, double *scale,
                           double *scale_cstr /*n_cstr or NULL*/);
/* The bound-constrained multistart of solver_infill_optim.rs:148-236 (no constraint models, or cstr_infill = true): one
 * COBYLA per start (rhobeg 0.5, ftol_rel = ftol_abs = 1e-4, at most max_eval evaluations each; max_eval <= 0:
 * min(10 n_start d, 2000)), all starts advanced in LOCK-STEP -- a round's trial points are one values-only evaluation, and
 * every start walks bit for bit the points it walks alone.  Returns the best EVALUATED point over all starts (the first start
 * wins ties): *f_best is bit for bit egx_infill_eval at x_best.  Values at or beyond 1e30 (COBYLA's barrier; LogEI's f64::MAX at
 * a point of zero variance) count as +inf.  No start finite: *f_best = +inf, x_best = start 0 clamped into the box, and
 * EGX_ERR_NO_FINITE_START.  NaN / infinite start rows or bounds, lo > hi: EGX_ERR_INVALID_VALUE. */
typedef struct {
    int64_t rounds;     /* lock-step rounds = evaluations of the start that ran longest */
    int64_t best_start; /* index of the start that won */
    int64_t *evals;     /* n_start evaluation counts, or NULL */
} egx_infill_stats;
int32_t egx_infill_optimize(egx_infill *h, const double *lo /*d*/, const double *hi /*d*/, const double *x_start /*n_start*d*/,
                            int64_t n_start, int64_t max_eval, double *f_best, double *x_best /*d*/, egx_infill_stats *stats);

/* ---- the constraint surrogates as constraints of the optimiser ---------------------------------------------------------
 * EgorConfig defaults to cstr_infill = false, cstr_strategy = MeanConstraint (solver/egor_config.rs:255-256): the criterion is
 * optimised WITHOUT the probability-of-feasibility factor (eval_infill_obj, solver_computations.rs:356-374) and every
 * constraint surrogate is handed to the optimiser as a nonlinear inequality constraint c_j(x) <= 0
 * (solver_infill_optim.rs:148-204): its scaled mean mu_j / scale_cstr_j (mean_cstr, :196-220) or its scaled upper trust bound
 * (mu_j + 3 sigma_j) / scale_cstr_j (upper_trust_bound_cstr, :224-257).  A handle starts in EGX_CSTR_INFILL (everything above);
 * in EGX_CSTR_MEAN / _UTB
 *   - egx_infill_eval's value / grad are the objective model's criterion alone, -crit / scale: no factor, and `feasibility` is
 *     not consulted (as eval_infill_obj); parts stay as they are.  The constraint surrogates run only when parts are asked
 *     for, and under MEAN only their MEAN-ONLY launch sequence (no solve against the factor) unless parts->var or
 *     parts->grad_var is asked for.  Their means keep the bits of the full sequence.
 *   - egx_infill_scaling skips the factor (compute_infill_obj_scale with cstr_infill = false, :322-330) and stores the
 *     scale_cstr it computes in the handle (an entry that is not positive and finite leaves the stored one).
 *   - egx_infill_optimize is unchanged: it optimises whatever egx_infill_eval returns.
 * scale_cstr: n_cstr positive finite values (EGX_ERR_INVALID_VALUE otherwise), or NULL to keep the stored ones (ones at first). */
typedef enum { EGX_CSTR_INFILL = 0 /* pofs / logpofs in the objective */, EGX_CSTR_MEAN = 1, EGX_CSTR_UTB = 2 } egx_cstr_strategy;
int32_t egx_infill_set_cstr_strategy(egx_infill *h, int32_t strategy, const double *scale_cstr /*n_cstr, or NULL: keep*/);
int32_t egx_infill_get_cstr_strategy(egx_infill *h, int32_t *strategy, double *scale_cstr /*n_cstr or NULL*/);
/* What the optimiser sees at m points: value (m) as egx_infill_eval's in these modes, cstr[i * n_cstr + j] the constraint values,
 * and optionally their x-gradients grad (m x d), grad_cstr[(i * n_cstr + j) * d + c].  Under MEAN the constraint surrogates'
 * experts run the mean-only sequence; under UTB the full one.  A NaN / infinite point: value = +inf, cstr = +inf, zero
 * gradients.  A point's bits do not depend on its companions or its position.  EGX_ERR_INVALID_VALUE on an EGX_CSTR_INFILL
 * handle.  n_cstr = 0 is allowed (cstr / grad_cstr untouched, may be NULL); m = 0 succeeds. */
int32_t egx_infill_eval_cstr(egx_infill *h, const double *xq, int64_t m, double *value /*m*/, double *cstr /*m*n_cstr*/,
                             double *grad /*m*d or NULL*/, double *grad_cstr /*m*n_cstr*d or NULL*/);
/* The multistart of solver_infill_optim.rs:217-236 with the constraints: one general-constraint COBYLA per start (Powell's
 * method with his full trust-region subproblem, egobox_amd/csrc/cobyla.h; rhobeg 0.5, ftol_rel = ftol_abs = 1e-4, no
 * constraint tolerances given to it -- optimizers/optimizer.rs:123-126 --, at most max_eval evaluations each; max_eval <= 0:
 * min(10 n_start d, 2000)), all starts in LOCK-STEP: a round is ONE values-only egx_infill_eval_cstr of the trial points, and
 * every start walks bit for bit the points it walks alone.
 * DEVIATION in what is returned.  The reference takes every run's final vertex and the smallest objective over the starts,
 * feasible or not (:229-232).  Here the best EVALUATED point is returned under this ordering: a point is feasible when
 * c_j <= cstr_tol_j / scale_cstr_j for every j (the handle's cstr_tols, Egor's acceptance tolerance); feasible beats infeasible;
 * among feasible points the smaller objective wins (a value at or beyond 1e30 counting as +inf), among infeasible ones the
 * smaller max_j (c_j - cstr_tol_j / scale_cstr_j); the first point within a start and the first start win ties.
 * *f_best and c_best are bit for bit egx_infill_eval_cstr at x_best; stats->feasible / violation (that maximum; 0 without
 * constraints) describe the returned point.  An infeasible best point is EGX_SUCCESS with feasible = 0; no finite objective
 * value at all: *f_best = +inf and EGX_ERR_NO_FINITE_START.  EGX_ERR_INVALID_VALUE on an EGX_CSTR_INFILL handle and for the
 * arguments egx_infill_optimize refuses.  n_cstr = 0: a bound-constrained run of the same class (c_best may be NULL). */
typedef struct {
    int64_t rounds, best_start;
    int32_t feasible;
    double violation;
    int64_t *evals; /* n_start evaluation counts, or NULL */
} egx_infill_cstr_stats;
int32_t egx_infill_optimize_cstr(egx_infill *h, const double *lo /*d*/, const double *hi /*d*/, const double *x_start /*n_start*d*/,
                                 int64_t n_start, int64_t max_eval, double *f_best, double *x_best /*d*/, double *c_best /*n_cstr*/,
                                 egx_infill_cstr_stats *stats);
/* The same multistart with the reference's DEFAULT inner optimiser, InfillOptimizer::Slsqp (solver/egor_config.rs:246): one
 * SLSQP per start (Kraft's algorithm, egobox_amd/csrc/slsqp.h; ftol_rel = ftol_abs = 1e-4, solver_infill_optim.rs:225-226, at
 * most max_eval evaluations each; max_eval <= 0: min(10 n_start d, 2000)), all starts in LOCK-STEP: a round collects the point
 * of every start that still runs -- a line-search trial point as much as an iterate -- and is ONE evaluation WITH gradients,
 * egx_infill_eval (EGX_CSTR_INFILL, or n_cstr = 0) or egx_infill_eval_cstr (EGX_CSTR_MEAN / _UTB); no point is evaluated
 * twice, and every start walks bit for bit the points it walks alone.  Works in all three strategies:
 *   EGX_CSTR_INFILL, or n_cstr = 0   a bound-constrained run; c_best is untouched (may be NULL), feasible = 1, violation = 0;
 *   EGX_CSTR_MEAN / _UTB             subject to c_j(x) - cstr_tol_j / scale_cstr_j <= 0 (optimizers/optimizer.rs:188-199).
 * Returned: the best EVALUATED point in egx_infill_optimize_cstr's ordering (the same deviation from :229-232): feasible
 * (c_j <= cstr_tol_j / scale_cstr_j for all j) beats infeasible, then the smaller objective, or the smaller violation; the
 * first point and the first start win ties.  *f_best and c_best are bit for bit the evaluation at x_best.  On a handle with
 * xtypes the trial points are cast on the device and the machine works in the unfolded box with the gradients at the cast
 * point (gpmix/mixint.rs:656-687); x_best is the point as proposed.  A value that is NaN, or at or beyond 1e30, counts as
 * +inf: at a trial point it shortens the step, at a start point it ends that start.  No finite objective at all:
 * *f_best = +inf, x_best = start 0 clamped into the box, EGX_ERR_NO_FINITE_START.  The argument checks are
 * egx_infill_optimize_cstr's.  stop[s]: why start s ended -- 1 the evaluation budget, 2 Kraft's convergence test, 3 the line
 * search could not move (no descent direction after the resets of the Hessian, or only non-finite values), 4 no finite value
 * at the start point, 5 the quadratic subproblem stayed inconsistent. */
typedef struct {
    int64_t rounds, best_start;
    int32_t feasible;
    double violation;
    int64_t *evals; /* n_start counts of distinct points evaluated, or NULL */
    int32_t *stop;  /* n_start stop codes, or NULL */
} egx_infill_slsqp_stats;
int32_t egx_infill_optimize_slsqp(egx_infill *h, const double *lo /*d*/, const double *hi /*d*/, const double *x_start /*n_start*d*/,
                                  int64_t n_start, int64_t max_eval, double *f_best, double *x_best /*d*/,
                                  double *c_best /*n_cstr, or NULL*/, egx_infill_slsqp_stats *stats);

/* ---- ... on mixtures of experts -------------------------------------------------------------------------------------
 * What EGO holds for its objective and every constraint is a clustered surrogate (GpMixture, crates/moe/src/algorithm.rs):
 * one GP expert per cluster and the Gaussian mixture of the x-space that weighs them.  A handle of egx_infill_create_mix takes
 * such SURROGATES: the experts (borrowed egx_gp*, all fitted, same d and device; n may differ) and a copy of the mixture, given
 * as to egx_gmx_predict_probas -- weights (k), means (k x d), precisions_chol (k x d x d) and the heaviside factor.  Per
 * 128-point tile every expert runs the launch sequence of a single model; one more launch per (tile, surrogate with k >= 2)
 * computes the responsibilities p_e(x), their x-derivatives (the arithmetic of egx_gmx_predict_probas / _derivatives, bit for
 * bit) and recombines the experts on the device:
 *   smooth (:411-423, 670-685, 691-783)  mean = sum p_e mu_e, var = sum p_e^2 v_e,
 *                                        grad mean = sum p_e grad mu_e + p'_e mu_e, grad var = sum p_e^2 grad v_e + 2 p_e p'_e v_e
 *   hard   (:879-935, 942-1010)          the four quantities of the expert of the FIRST maximum of p_e
 * (the experts in index order).  In hard mode every expert still evaluates every point and the kernel selects: a call costs k
 * expert sequences per surrogate in both modes, and a point's bits stay independent of its companions.  A surrogate with ONE
 * expert is that expert (the responsibilities are ones, gaussian_mixture.rs:115-116): its mixture is not read and may be NULL.
 * egx_infill_eval, _scaling, _optimize, _set_params and _get_params work on such a handle unchanged; egx_infill_parts stays
 * per SURROGATE, (1 + n_cstr) entries.  A NaN / infinite point: value +inf, gradient 0, for that point only.
 * Checked before the device is touched, EGX_ERR_INVALID_VALUE naming the surrogate (and the expert): NULL pointers,
 * n_experts < 1, and for k >= 2 a heaviside factor that is not positive and finite, non-finite weights / means / factors,
 * weights that are not positive, differing d or device.  EGX_ERR_NOT_FITTED names surrogate and expert, here and in every
 * later call.  EGX_ERR_UNSUPPORTED when 3 (d | 1) + 2 (k | 1) > 320 (the recombination keeps that many doubles of LDS per
 * point; every mixture egx_gmm_fit can train, d <= 35 and k <= 16, fits; one of egx_gmm_fit_wide beyond d of about 100
 * does not).
 * Out of scope: mixtures whose experts live on several ranks (egx_sweep).  Sparse-GP experts (egx_sgp): egx_infill_create_any below. */
typedef struct {
    egx_gp *const *experts; int32_t n_experts;       /* one per cluster, fitted, same d and device */
    const double *weights /*k*/, *means /*k*d*/, *precisions_chol /*k*d*d*/;  /* as egx_gmx_predict_probas; may be NULL when n_experts == 1 */
    double heaviside_factor;                          /* > 0 */
    int32_t smooth;                                   /* 1 smooth, 0 hard */
} egx_infill_surrogate;
int32_t egx_infill_create_mix(const egx_infill_config *cfg, const egx_infill_surrogate *surrogates /*1 + n_cstr, [0] = objective*/,
                              const double *cstr_tols, int32_t n_cstr, egx_infill **out);
/* diagnostics: what surrogate j was recombined FROM; any pointer may be NULL.  Expert-major parts of its k experts, the
 * responsibilities (bit for bit egx_gmx_predict_probas at xq) and their derivatives (... _derivatives); k = 1: ones and zeros.
 * Works on a handle of egx_infill_create as well (every surrogate one expert). */
int32_t egx_infill_eval_experts(egx_infill *h, int32_t j, const double *xq, int64_t m,
                                double *mean /*k*m*/, double *var /*k*m*/, double *grad_mean /*k*m*d*/, double *grad_var /*k*m*d*/,
                                double *probas /*m*k*/, double *dprobas /*m*k*d*/);

/* ---- ... with SPARSE experts ------------------------------------------------------------------------------------------
 * The same handle from TAGGED model references: an expert is a dense model (egx_gp*) or a fitted sparse one (egx_sgp*), mixed
 * freely across the surrogates and inside one mixture; everything else as egx_infill_surrogate / egx_infill_create_mix, and a
 * handle of dense experts only returns the bits of egx_infill_create / _create_mix.  Every egx_infill_* call works on such a
 * handle unchanged (eval, eval_experts, eval_cstr, scaling, optimize, optimize_cstr, set / get_params, set / get_cstr_strategy).
 * A sparse expert runs, per 128-point tile and at the padded batch of 128 whatever m is, the BATCHED sequence of
 * egx_sgp_predict_valvar / _valvar_gradients (never their few-query route: a point's bits do not depend on its companions or
 * its position): raw x (the sparse model does not normalise), K(x, z), the two block solves with their row reductions, the
 * mean; with gradients the two transposed products with the cached inverse factors and the two contractions.  Semantics:
 *   - the `var` of a sparse model (egx_infill_parts, egx_infill_eval_experts) is egx_sgp_predict_var's: the raw variance
 *     clamped at 1e-15, THEN + noise; its gradient is egx_sgp_predict_var_gradients': exactly 0 where the clamp holds;
 *   - the mean is the sum, in split order, of the partial sums of K(x, z) . (sigma2 vec) over a split of the inducing points
 *     that depends on nz alone (within rounding of egx_sgp_predict, not bit for bit); a constraint surrogate under
 *     EGX_CSTR_MEAN runs no solve and its means keep the bits of the full sequence;
 *   - the model's fitted state is read at every call, as for dense models (a refit between two calls is followed);
 *   - sparse handles carry no xtypes: a handle that mixes typed dense models with sparse ones is refused (all or none);
 *   - the limit of the sparse x-gradients, 6 d <= 20480, is checked at creation: EGX_ERR_UNSUPPORTED.
 * Checked before the device is touched, EGX_ERR_INVALID_VALUE naming surrogate and expert: NULL experts / handles, a kind that
 * is neither EGX_MODEL_GP nor EGX_MODEL_SGP, n_experts < 1, the mixture data as for egx_infill_create_mix.
 * Out of scope: mixtures whose experts live on several ranks (egx_sweep), xtypes on sparse models. */
typedef enum { EGX_MODEL_GP = 0, EGX_MODEL_SGP = 1 } egx_model_kind;
typedef struct { int32_t kind; void *handle; } egx_model_ref;        /* egx_gp* or egx_sgp*, borrowed */
typedef struct {
    const egx_model_ref *experts; int32_t n_experts;
    const double *weights /*k*/, *means /*k*d*/, *precisions_chol /*k*d*d*/;
    double heaviside_factor;
    int32_t smooth;
} egx_infill_surrogate_any;
int32_t egx_infill_create_any(const egx_infill_config *cfg, const egx_infill_surrogate_any *surrogates /*1 + n_cstr*/,
                              const double *cstr_tols, int32_t n_cstr, egx_infill **out);

/* egx_moe_predict_valvar / _valvar_gradients for a mixture of SPARSE experts: the same arguments, routing, workers, order of
 * additions, failure semantics and sw == NULL; every expert answers through egx_sgp_predict* on its points. */
int32_t egx_moe_predict_valvar_sgp(egx_sweep *sw, egx_sgp *const *experts, const int32_t *expert_ids, int64_t n_local,
                                   int64_t n_experts, const double *probas /*m*n_experts*/, const double *xq /*m*d*/,
                                   int64_t m, int64_t d, int32_t smooth, double *val /*m*/, double *var /*m*/);
int32_t egx_moe_predict_valvar_gradients_sgp(egx_sweep *sw, egx_sgp *const *experts, const int32_t *expert_ids, int64_t n_local,
                                             int64_t n_experts, const double *probas /*m*n_experts*/,
                                             const double *dprobas /*m*n_experts*d*/, const double *xq /*m*d*/, int64_t m,
                                             int64_t d, int32_t smooth, double *grad_val /*m*d*/, double *grad_var /*m*d*/);

/* ---- q points per iteration: PENDING points on the infill handle ----------------------------------------------------------
 * The reference's q_points > 1 loop (crates/ego/src/solver/solver_impl.rs:622-791) appends a VIRTUAL observation at the point
 * it just found (compute_virtual_point, solver_computations.rs:261-292) and refits every surrogate before it looks for the
 * next one.  Here the handle keeps up to EGX_INFILL_MAX_PENDING virtual observations and CONDITIONS its models on them in closed
 * form (csrc/pending_math.h): no model is refitted or touched.  While q > 0 every evaluation of the handle -- egx_infill_eval,
 * _eval_cstr, _scaling, the three optimisers, the parts tables, a lone expert's row of _eval_experts -- runs on the
 * conditioned models; with q = 0 (never pushed, or after egx_infill_clear_pending) the handle launches exactly what it
 * launched before, bit for bit.  What the conditioning equals: a refit of each model on its n + q points at its theta with its
 * normalisation (x_mean, x_std, y_mean, y_std) FROZEN; the reference's refit re-normalises.  fmin stays what the caller set.
 * push_pending: x is cast with the models' xtypes first, as a query would be; y holds one raw value per surrogate (objective,
 * then the constraints).  Errors: a 17th point, a non-finite coordinate or value: EGX_ERR_INVALID_VALUE; a mixture (two or more
 * experts) or a sparse expert among the surrogates: EGX_ERR_UNSUPPORTED naming the surrogate; d > 1024: EGX_ERR_UNSUPPORTED; a
 * pivot of S = k(X_v, X_v) + nugget I that is not positive: EGX_ERR_LINALG -- and the handle is as it was before the call.
 * Pending points belong to ONE fitted state of every model: after a model was refitted every evaluation returns
 * EGX_ERR_INVALID_VALUE saying so, until egx_infill_clear_pending.
 * Up to d = 64 the cross-covariances of a tile come from one fused contraction (csrc/kernels_pending.hip); beyond, and everywhere
 * with egx_set_tuning("pending_composed", 1), from q launches of the existing mean / x-gradient contractions (the same values to
 * rounding, not the same bits). */
#define EGX_INFILL_MAX_PENDING 16
typedef enum { EGX_QEI_KB = 0, EGX_QEI_KB_LB = 1, EGX_QEI_KB_UB = 2, EGX_QEI_CL_MIN = 3 } egx_qei_strategy;
int32_t egx_infill_push_pending(egx_infill *h, const double *x /*d*/, const double *y /*1 + n_cstr*/);
int32_t egx_infill_clear_pending(egx_infill *h);
/* *q; optionally (any may be NULL) the points as stored (q x d, cast), their values (q x (1 + n_cstr)) and the conditioned
 * process variance of every surrogate (1 + n_cstr; the fitted one while q = 0) */
int32_t egx_infill_get_pending(egx_infill *h, int32_t *q, double *x, double *y, double *sigma2);
/* compute_virtual_point at x on the handle's CURRENT (conditioned) models: y (1 + n_cstr).  KB / KB_LB / KB_UB: the objective's
 * mean + {0, -3, +3} sqrt(var), the mean of every constraint.  CL_MIN: the training row with the smallest objective value, every
 * model's y at that row (x is not read); all models must hold the same number of rows, else EGX_ERR_INVALID_VALUE. */
int32_t egx_infill_virtual_point(egx_infill *h, const double *x /*d*/, int32_t strategy, double *y);
typedef enum { EGX_BATCH_COBYLA = 0, EGX_BATCH_SLSQP = 1 } egx_infill_batch_optimizer;
typedef struct {
    int32_t strategy;  /* egx_qei_strategy */
    int32_t optimizer; /* COBYLA: egx_infill_optimize (EGX_CSTR_INFILL) or _optimize_cstr; SLSQP: egx_infill_optimize_slsqp */
    int64_t max_eval;  /* as the optimisers' (<= 0: their default) */
    const double *scaling_points; /* n_scaling x d, or NULL: egx_infill_scaling on the conditioned models before every step */
    int64_t n_scaling;
} egx_infill_batch_config;
void egx_infill_batch_config_default(egx_infill_batch_config *cfg); /* KB, SLSQP, 0, NULL, 0 */
/* The q loop in one call: optimise from the step's own starts, compute the virtual point there, push it, again.  The pending
 * points already on the handle stay and count towards the 16.  Stops at the first step whose optimiser or push fails and
 * returns that error with the steps completed so far in *n_found (their points stay pending); f_out[i] is the criterion of
 * step i at x_out[i] on the models conditioned on the steps before it. */
int32_t egx_infill_optimize_batch(egx_infill *h, const egx_infill_batch_config *cfg, const double *lo /*d*/, const double *hi /*d*/,
                                  const double *x_start /*q*n_start*d*/, int64_t n_start, int32_t q, double *x_out /*q*d*/,
                                  double *y_virtual /*q*(1+n_cstr)*/, double *f_out /*q*/, int32_t *n_found);

/* ---- ACTIVE COORDINATES on the infill handle (CoEGO, crates/ego/src/solver/coego.rs, solver_infill_optim.rs:67-271) ---------
 * CoEGO optimises the criterion over one group of coordinates at a time, the others held at the current best point.  While an
 * activity is set a trial point is a COMPACT row of n_active values: value j of the row replaces x_base[active[j]], every other
 * column is x_base's.  `active`: n_active DISTINCT column indices in [0, d), 1 <= n_active <= d, in any order (CoEGO's groups
 * are shuffled); x_base: d finite values.  Anything else: EGX_ERR_INVALID_VALUE naming the offending entry, before the device is
 * touched, and the handle keeps what it had.  On a handle with xtypes the indices count the unfolded columns and x_base is a raw
 * unfolded row: the cast happens where it happens without an activity.
 * Width n_active instead of d while an activity is set:
 *   egx_infill_eval           xq, grad, parts->grad_mean / grad_var
 *   egx_infill_eval_cstr      xq, grad, grad_cstr
 *   egx_infill_optimize, _optimize_cstr, _optimize_slsqp    lo, hi, x_start, x_best; the machines run in n_active dimensions
 *                             and the default budget is min(10 n_start n_active, 2000)
 * Width d as ever, the activity is not read: egx_infill_scaling, _eval_experts, _push_pending, _get_pending, _virtual_point.
 * egx_infill_optimize_batch returns EGX_ERR_UNSUPPORTED while an activity is set.
 * The value of a compact point is bit for bit the full-width call's at the expanded row, its gradient bit for bit that call's
 * columns active[0 .. n_active) -- on every kind of handle (lone dense models, mixtures, sparse experts, typed models, pending
 * points); a non-finite value in a compact row gives +inf and a zero gradient for that point only.  Rows are expanded and
 * columns gathered on the host (csrc/infill_active.h); the experts' x-gradient contractions compute the listed columns alone
 * (k_xgrad<LIST>, csrc/kernels_corr.hip).  Without an activity every entry point returns the bits it returned before. */
int32_t egx_infill_set_active(egx_infill *h, const int32_t *active /*n_active*/, int32_t n_active, const double *x_base /*d*/);
int32_t egx_infill_clear_active(egx_infill *h);
/* *n_active (0: no activity); optionally the indices and the base point (each d long at most, or NULL) */
int32_t egx_infill_get_active(egx_infill *h, int32_t *n_active, int32_t *active /*d, or NULL*/, double *x_base /*d, or NULL*/);

/* ---- runs.  An evaluation walks the points in tiles and, per tile, the surrogates in RUNS: consecutive surrogates that go through
 * ONE launch sequence, the member a grid coordinate of every kernel of it, instead of one sequence each.  Surrogates js .. js +
 * len - 1 form a run when each is a lone dense model; all have the same n, kernel, trend and coefficient columns; all take the same
 * sequence kind (the objective always the full one; the constraints the mean-only one exactly under EGX_CSTR_MEAN, when no
 * variance of theirs is asked for); the handle has no pending points; len <= 16.  A mean-only run needs nothing more (separately
 * created models of one shape qualify); a full-sequence run also needs its members to be members of ONE group in consecutive
 * slots (egx_gp_create_group), whose factors and C^-T sit at one stride.  Surrogates are never reordered.  CONTRACT: every
 * output of every entry point of a handle is bit for bit what the same surrogates give with all runs of length 1.
 * egx_infill_get_runs reports the runs of a walk over all surrogates under the current strategy and pending state: *n_runs, and
 * their lengths in order (they sum to 1 + n_cstr). */
int32_t egx_infill_get_runs(egx_infill *h, int32_t *n_runs, int32_t *run_len /* 1 + n_cstr, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* EGX_GP_H */
