// Header-only C++17 host API over the C ABI of egx_gp.h, shaped like the reference's Rust builder
// (crates/gp/src/parameters.rs:167-313, crates/gp/src/algorithm.rs:200-440):
//
//     auto gp = egobox::GaussianProcess::params(egobox::Mean::Constant, egobox::Corr::SquaredExponential)
//                   .theta_tuning(egobox::ThetaTuning::Fixed({1.83209405}))
//                   .fit(xt, n, d, yt);                     // Err(GpError::..) of the reference -> C++ exceptions
//     auto y = gp.predict(xq, m);  auto v = gp.predict_var(xq, m);  gp.theta(); gp.variance(); gp.likelihood();
//
// This image has no Rust toolchain; this is the compiled-language mirror of the reference interface (INTEGRATION.md
// shows the Rust `extern "C"` shim).  Everything numerical happens behind the C ABI on the GPU.
#ifndef EGX_GP_HPP
#define EGX_GP_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <array>
#include <vector>

#include "egx_gp.h"

namespace egobox {

enum class Mean { Constant = EGX_MEAN_CONSTANT, Linear = EGX_MEAN_LINEAR, Quadratic = EGX_MEAN_QUADRATIC };
enum class Corr {
    SquaredExponential = EGX_CORR_SQUARED_EXPONENTIAL,
    AbsoluteExponential = EGX_CORR_ABSOLUTE_EXPONENTIAL,
    Matern32 = EGX_CORR_MATERN32,
    Matern52 = EGX_CORR_MATERN52
};

// crates/gp/src/errors.rs:8-40
struct GpError : std::runtime_error {
    int rc;
    GpError(int rc_, const std::string &m) : std::runtime_error(m), rc(rc_) {}
};
struct InvalidValueError : GpError { using GpError::GpError; };
struct LinalgError : GpError { using GpError::GpError; };
struct LikelihoodComputationError : GpError { using GpError::GpError; };
struct PeerError : GpError { using GpError::GpError; };  // another rank of a collective failed (EGX_ERR_PEER)

inline void check(int32_t rc) {
    if (rc == EGX_SUCCESS) return;
    const std::string msg = egx_last_error();
    switch (rc) {
        case EGX_ERR_INVALID_VALUE: throw InvalidValueError(rc, msg);
        case EGX_ERR_LINALG: throw LinalgError(rc, msg);
        case EGX_ERR_LIKELIHOOD: throw LikelihoodComputationError(rc, msg);
        case EGX_ERR_PEER: throw PeerError(rc, msg);
        default: throw GpError(rc, msg);
    }
}

// crates/gp/src/parameters.rs:11-78
struct ThetaTuning {
    enum class Kind { Fixed, Full, Partial } kind = Kind::Full;
    std::vector<double> init{DEFAULT_INIT};
    std::vector<std::pair<double, double>> bounds{{DEFAULT_LO, DEFAULT_HI}};
    std::vector<int64_t> active;
    static constexpr double DEFAULT_INIT = 1e-1, DEFAULT_LO = 1e-2, DEFAULT_HI = 1e1;
    static ThetaTuning Fixed(std::vector<double> v) {
        ThetaTuning t;
        t.kind = Kind::Fixed;
        t.init = std::move(v);
        return t;
    }
    static ThetaTuning Full(std::vector<double> i, std::vector<std::pair<double, double>> b) {
        ThetaTuning t;
        t.init = std::move(i);
        t.bounds = std::move(b);
        return t;
    }
    static ThetaTuning Partial(std::vector<double> i, std::vector<std::pair<double, double>> b, std::vector<int64_t> a) {
        ThetaTuning t = Full(std::move(i), std::move(b));
        t.kind = Kind::Partial;
        t.active = std::move(a);
        return t;
    }
};

// XType (crates/ego/src/types.rs) and the free functions of crates/ego/src/gpmix/mixint.rs:38-226 over the egx_mixint_* helpers
struct XType {
    int32_t kind = EGX_XTYPE_FLOAT;
    double lo = 0.0, hi = 0.0;
    std::vector<double> values;  // Ord
    int32_t n = 0;               // Enum levels
    static XType Float(double lo, double hi) { XType t; t.lo = lo, t.hi = hi; return t; }
    static XType Int(double lo, double hi) { XType t; t.kind = EGX_XTYPE_INT, t.lo = lo, t.hi = hi; return t; }
    static XType Ord(std::vector<double> v) { XType t; t.kind = EGX_XTYPE_ORD, t.n = (int32_t)v.size(), t.values = std::move(v); return t; }
    static XType Enum(int32_t n) { XType t; t.kind = EGX_XTYPE_ENUM, t.n = n; return t; }
};
namespace mixint {
// the C structs of a spec; they borrow the Ord values of `xt`, which must outlive them
inline std::vector<egx_xtype> c_xtypes(const std::vector<XType> &xt) {
    std::vector<egx_xtype> c(xt.size());
    for (size_t j = 0; j < xt.size(); j++) c[j] = egx_xtype{xt[j].kind, xt[j].n, xt[j].lo, xt[j].hi, xt[j].values.empty() ? nullptr : xt[j].values.data()};
    return c;
}
inline int64_t unfolded_dim(const std::vector<XType> &xt) {
    const auto c = c_xtypes(xt);
    int64_t d = 0;
    check(egx_mixint_unfolded_dim(c.data(), (int32_t)c.size(), &d));
    return d;
}
inline std::vector<double> as_continuous_limits(const std::vector<XType> &xt) {  // d x 2
    const auto c = c_xtypes(xt);
    std::vector<double> lim((size_t)unfolded_dim(xt) * 2);
    check(egx_mixint_continuous_limits(c.data(), (int32_t)c.size(), lim.data()));
    return lim;
}
namespace detail {
using RowFn = int32_t (*)(const egx_xtype *, int32_t, const double *, int64_t, double *);
inline std::vector<double> rows(RowFn fn, const std::vector<XType> &xt, const double *x, int64_t m, int64_t cols_out) {
    const auto c = c_xtypes(xt);
    std::vector<double> out((size_t)(m * cols_out));
    check(fn(c.data(), (int32_t)c.size(), x, m, out.data()));
    return out;
}
}  // namespace detail
// x: m rows of the folded (nx columns) or unfolded (d columns) space, as the C functions take them
inline std::vector<double> unfold_with_enum_mask(const std::vector<XType> &xt, const double *x, int64_t m) {
    return detail::rows(egx_mixint_unfold, xt, x, m, unfolded_dim(xt));
}
inline std::vector<double> to_continuous_space(const std::vector<XType> &xt, const double *x, int64_t m) { return unfold_with_enum_mask(xt, x, m); }
inline std::vector<double> fold_with_enum_index(const std::vector<XType> &xt, const double *x, int64_t m) {
    return detail::rows(egx_mixint_fold, xt, x, m, (int64_t)xt.size());
}
inline std::vector<double> cast_to_discrete_values(const std::vector<XType> &xt, const double *x, int64_t m) {
    return detail::rows(egx_mixint_cast, xt, x, m, unfolded_dim(xt));
}
inline std::vector<double> to_discrete_space(const std::vector<XType> &xt, const double *x, int64_t m) {
    return detail::rows(egx_mixint_to_discrete, xt, x, m, (int64_t)xt.size());
}
}  // namespace mixint

// The x rotations (d x k, row-major) of a PLS1 regression of y on x (n x d row-major), centred and scaled to unit variance, computed
// on the device (egx_pls_rotations): the KPLS weights w_star.  status (optional): 1 with all zeros on a constant response.
inline std::vector<double> pls_rotations(const double *x, const double *y, int64_t n, int64_t d, int64_t k, int device = -1,
                                         int32_t *status = nullptr) {
    std::vector<double> w((size_t)(d > 0 ? d : 0) * (size_t)(k > 0 ? k : 0));
    check(egx_pls_rotations(device, x, y, n, d, k, w.empty() ? nullptr : w.data(), status));
    return w;
}

class GaussianProcess;

// GpParams / GpValidParams, parameters.rs:80-313
class GpParams {
  public:
    GpParams(Mean m, Corr c) : mean_(m), corr_(c) {}
    GpParams &theta_tuning(ThetaTuning t) { tuning_ = std::move(t); return *this; }
    GpParams &theta_init(std::vector<double> v) { tuning_.init = std::move(v); return *this; }
    GpParams &theta_bounds(std::vector<std::pair<double, double>> b) { tuning_.bounds = std::move(b); return *this; }
    // KPLS (parameters.rs:214-218, algorithm.rs:798-855): fit on k PLS components of the inputs.  `fit` computes the rotations on
    // the device (pls_rotations) and hands them to the model as w_star / kpls_dim of egx_gp_config; theta, its initial guess and
    // its bounds then have k components (a single value is broadcast).  k = 0 is refused by `fit` ("`kpls_dim` canot be 0!"), as
    // is k > d.  w_star(w, k): the caller's own rotations (d x k, row-major) instead.  fit_group refuses both: the members of a
    // lock-step group share no rotations (InvalidValueError).
    GpParams &kpls_dim(int64_t k) { kpls_dim_ = k; has_kpls_ = true; w_star_.clear(); return *this; }
    GpParams &w_star(std::vector<double> w, int64_t k) { w_star_ = std::move(w); kpls_dim_ = k; has_kpls_ = true; return *this; }
    GpParams &n_start(int n) { n_start_ = n; return *this; }
    GpParams &max_eval(int n) { max_eval_ = n; return *this; }
    GpParams &nugget(double v) { nugget_ = v; return *this; }
    GpParams &seed(uint64_t s) { seed_ = s; return *this; }
    GpParams &device(int dev) { device_ = dev; return *this; }
    GpParams &n_workspaces(int n) { n_workspaces_ = n; return *this; }
    // Fit<..>::fit, algorithm.rs:785-980.  x is (n x d) row-major, y has n entries.
    GaussianProcess fit(const double *x, int64_t n, int64_t d, const double *y) const;
    // `fit` (ThetaTuning::Fixed or ::Full) for k training sets of one shape at once: x (k x n x d), y (k x n).  The expert loop of
    // egobox-moe (crates/moe/src/algorithm.rs:167-177) with the experts factored in LOCK-STEP (egx_gp_create_group +
    // egx_gp_finalize_multi / egx_gp_fit_multi); each model is what `fit` returns for its training set on one workspace.
    std::vector<GaussianProcess> fit_group(const double *x, const double *y, int64_t n, int64_t d, int32_t k) const;

  private:
    Mean mean_;
    Corr corr_;
    ThetaTuning tuning_;
    int n_start_ = 10, max_eval_ = 50;  // GP_OPTIM_N_START, GP_COBYLA_MAX_EVAL (parameters.rs:107-121)
    double nugget_ = 100.0 * 2.220446049250313e-16;
    uint64_t seed_ = 42;
    int device_ = -1, n_workspaces_ = 1;
    bool has_kpls_ = false;
    int64_t kpls_dim_ = 0;
    std::vector<double> w_star_;
};

// GaussianProcess, algorithm.rs:174-440
class GaussianProcess {
  public:
    static GpParams params(Mean m, Corr c) { return GpParams(m, c); }

    // egx_gp_set_xtypes: every query point is cast to its nearest admissible discrete point on the device from now on; {} clears
    void set_xtypes(const std::vector<XType> &xt) {
        const auto c = mixint::c_xtypes(xt);
        check(egx_gp_set_xtypes(h_.get(), c.empty() ? nullptr : c.data(), (int32_t)c.size()));
    }

    std::vector<double> predict(const double *x, int64_t m) const {
        std::vector<double> y((size_t)m);
        check(egx_gp_predict(h_.get(), x, m, y.data()));
        return y;
    }
    std::vector<double> predict_var(const double *x, int64_t m) const {
        std::vector<double> v((size_t)m);
        check(egx_gp_predict_var(h_.get(), x, m, v.data()));
        return v;
    }
    std::pair<std::vector<double>, std::vector<double>> predict_valvar(const double *x, int64_t m) const {
        std::vector<double> y((size_t)m), v((size_t)m);
        check(egx_gp_predict_valvar(h_.get(), x, m, y.data(), v.data()));
        return {std::move(y), std::move(v)};
    }
    std::vector<double> predict_gradients(const double *x, int64_t m) const {  // (m x d) row-major
        std::vector<double> g((size_t)(m * d_));
        check(egx_gp_predict_gradients(h_.get(), x, m, g.data()));
        return g;
    }
    std::vector<double> predict_var_gradients(const double *x, int64_t m) const {
        std::vector<double> g((size_t)(m * d_));
        check(egx_gp_predict_var_gradients(h_.get(), x, m, g.data()));
        return g;
    }
    // algorithm.rs:711-727 -> the two (m x d) row-major gradients from one pass
    std::pair<std::vector<double>, std::vector<double>> predict_valvar_gradients(const double *x, int64_t m) const {
        std::vector<double> gy((size_t)(m * d_)), gv((size_t)(m * d_));
        check(egx_gp_predict_valvar_gradients(h_.get(), x, m, gy.data(), gv.data()));
        return {std::move(gy), std::move(gv)};
    }
    // _compute_covariance, algorithm.rs:310-326 -> (m x m) row-major
    std::vector<double> predict_covariance(const double *x, int64_t m) const {
        std::vector<double> c((size_t)(m * m));
        check(egx_gp_predict_covariance(h_.get(), x, m, c.data()));
        return c;
    }
    // sample (EGX_SAMPLE_PSD: Cholesky of Sigma + tau I, the deviation from sample_eig documented in egx_gp.h) / sample_chol
    // (EGX_SAMPLE_CHOLESKY), algorithm.rs:383-395 -> (m x n_traj) row-major; z (m x n_traj) or nullptr: the stream of `seed`
    std::vector<double> sample(const double *x, int64_t m, int64_t n_traj, egx_sample_method method = EGX_SAMPLE_PSD,
                               uint64_t seed = 0, const double *z = nullptr, double *tau = nullptr) const {
        std::vector<double> t((size_t)(m * n_traj));
        check(egx_gp_sample(h_.get(), x, m, n_traj, method, seed, z, t.data(), tau));
        return t;
    }
    std::vector<double> sample_chol(const double *x, int64_t m, int64_t n_traj, uint64_t seed = 0) const {
        return sample(x, m, n_traj, EGX_SAMPLE_CHOLESKY, seed);
    }
    // reduced likelihood at k candidate thetas (k x theta_len row-major) -> (values, status per candidate): the evaluations
    // the reference's multistart closures make (algorithm.rs:880-897, 928-945), factored in lock-step groups on the GPU
    std::pair<std::vector<double>, std::vector<int32_t>> likelihood_batch(const double *thetas, int64_t k, int64_t theta_len) {
        std::vector<double> lk((size_t)k);
        std::vector<int32_t> st((size_t)k);
        check(egx_gp_likelihood_batch(h_.get(), thetas, k, theta_len, lk.data(), st.data()));
        return {std::move(lk), std::move(st)};
    }
    // the same with dL/dtheta (new: the reference's objective has no gradient, algorithm.rs:880): likelihoods (k), gradients
    // (k x h row-major), statuses (k); every stage in lock-step over a slot's candidates, bit for bit the single call
    struct LikelihoodGrad {
        std::vector<double> likelihood, gradient;
        std::vector<int32_t> status;
    };
    LikelihoodGrad likelihood_grad_batch(const double *thetas, int64_t k, int64_t theta_len) {
        int64_t h = 0;
        check(egx_gp_dims(h_.get(), nullptr, nullptr, nullptr, &h));
        LikelihoodGrad out;
        out.likelihood.resize((size_t)k);
        out.gradient.assign((size_t)(k * h), 0.0);
        out.status.resize((size_t)k);
        check(egx_gp_likelihood_grad_batch(h_.get(), thetas, k, theta_len, out.likelihood.data(), out.gradient.data(),
                                           out.status.data()));
        return out;
    }
    // a tuned model ran its multistart on several workspaces; the resident model needs one (plus one for likelihood
    // evaluations that must not un-fit it)
    void shrink(int32_t n_keep = 1) { check(egx_gp_shrink(h_.get(), n_keep)); }
    // { left-looking, left-looking rider, pipelined chain launches, whole-factorisation launch, panels per group, lock-step width,
    //   flow launch }
    std::array<int32_t, 7> schedule() const {
        std::array<int32_t, 7> s{};
        check(egx_gp_get_schedule(h_.get(), s.data(), 7));
        return s;
    }
    int32_t set_lockstep(int32_t width) {  // candidates per launch sequence (0 = the library's choice); returns the width in force
        check(egx_gp_set_lockstep(h_.get(), width));
        return egx_gp_get_lockstep(h_.get());
    }
    // GaussianProcess::training_data (algorithm.rs:969-978): the (n x d) inputs and (n) outputs the model was trained on
    std::pair<std::vector<double>, std::vector<double>> training_data(int64_t n) const {
        std::vector<double> x((size_t)(n * d_)), y((size_t)n);
        check(egx_gp_get_training_data(h_.get(), x.data(), y.data()));
        return {std::move(x), std::move(y)};
    }
    const std::vector<double> &theta() const { return theta_; }   // :413-416
    double variance() const { return sigma2_; }                   // :418-421
    double likelihood() const { return likelihood_; }             // :428-431
    std::pair<int64_t, int64_t> dims() const { return {d_, 1}; }  // :436-439
    int64_t n_evals() const { return n_evals_; }
    int64_t kpls_dim() const { return kpls_dim_; }  // the PLS components the model was fitted on; 0: none
    egx_gp *handle() const { return h_.get(); }
    // theta() / variance() / likelihood() read again from the handle after a fit that ran on it from outside (fit_lbfgs_group)
    void adopt_fit(int64_t n_evals) {
        int64_t hh = 0;
        check(egx_gp_dims(h_.get(), nullptr, nullptr, nullptr, &hh));
        theta_.resize((size_t)hh);
        egx_gp_inner_view view{};
        view.theta = theta_.data();
        view.sigma2 = &sigma2_;
        view.likelihood = &likelihood_;
        check(egx_gp_get_inner(h_.get(), &view));
        n_evals_ = n_evals;
    }

  private:
    friend class GpParams;
    struct Deleter {
        void operator()(egx_gp *p) const { egx_gp_destroy(p); }
    };
    std::unique_ptr<egx_gp, Deleter> h_;
    std::vector<double> theta_;
    double sigma2_ = 0.0, likelihood_ = 0.0;
    int64_t d_ = 0, n_evals_ = 0, kpls_dim_ = 0;
};

// SparseGaussianProcess at given parameters, sparse_algorithm.rs:145-362 (the predict side; the multistart fit is egx_sgp_fit):
// x (n x d), y (n), z (nz x d) row-major, raw units, zero trend.  Everything a SgpSurrogate (FullGpSurrogate) needs.
class SparseGaussianProcess {
  public:
    SparseGaussianProcess(const double *x, const double *y, int64_t n, int64_t d, const double *z, int64_t nz,
                          const egx_sgp_config *cfg = nullptr)
        : d_(d) {
        egx_sgp *h = nullptr;
        check(egx_sgp_create(cfg, x, y, n, d, z, nz, &h));
        h_.reset(h);
    }
    void finalize(const double *theta, int64_t theta_len, double sigma2, double noise) {
        check(egx_sgp_finalize(h_.get(), theta, theta_len, sigma2, noise));
    }
    // KPLS weights (d x h row-major, 1 <= h <= d; nullptr with h = 0 clears them): egx_sgp_set_w_star.  Un-fits the model; theta
    // then has h components.  w_star(): (the weights, h); no weights and h = d when none are set.
    void set_w_star(const double *w, int64_t h) { check(egx_sgp_set_w_star(h_.get(), w, h)); }
    // ... computed on the device from the training set the handle holds (egx_sgp_compute_w_star: no upload) and installed as
    // set_w_star installs them; zeros on a constant response.  Returns the weights (d x k).
    std::vector<double> compute_w_star(int64_t k) {
        check(egx_sgp_compute_w_star(h_.get(), k));
        return w_star().first;
    }
    std::pair<std::vector<double>, int64_t> w_star() const {
        int64_t h = 0;
        check(egx_sgp_get_w_star(h_.get(), nullptr, &h));
        std::vector<double> w((size_t)(d_ * h), std::nan(""));  // (weights are finite: NaN left behind means none are set)
        check(egx_sgp_get_w_star(h_.get(), w.data(), &h));
        if (std::isnan(w[0])) w.clear();
        return {std::move(w), h};
    }
    // the number of theta components: h with KPLS weights, else d
    int64_t n_theta() const {
        int64_t h = 0;
        check(egx_sgp_get_w_star(h_.get(), nullptr, &h));
        return h;
    }
    // the likelihood and its closed-form gradient (h + 2: theta.., sigma2, noise; zeros when status != 0): egx_sgp_likelihood_grad
    struct LikelihoodGrad {
        double likelihood;
        std::vector<double> grad;
        int32_t status;
    };
    LikelihoodGrad likelihood_grad(const double *theta, int64_t theta_len, double sigma2, double noise) {
        LikelihoodGrad r{0.0, std::vector<double>((size_t)(w_star().second + 2)), 0};
        check(egx_sgp_likelihood_grad(h_.get(), theta, theta_len, sigma2, noise, &r.likelihood, r.grad.data(), &r.status));
        return r;
    }
    // multistart L-BFGS fit on that gradient (egx_sgp_fit_lbfgs); returns the number of likelihood + gradient evaluations
    int64_t fit_lbfgs(const double *params0s, int64_t n_starts, const double *lo, const double *hi, bool estimate_noise,
                      double noise_fixed, int64_t max_iter = 50) {
        int64_t n_evals = 0;
        check(egx_sgp_fit_lbfgs(h_.get(), params0s, n_starts, lo, hi, estimate_noise ? 1 : 0, noise_fixed, max_iter, &n_evals));
        return n_evals;
    }
    // likelihood_grad and, from the same pair weights, dL/dz (nz x d row-major): egx_sgp_likelihood_grad_z
    struct LikelihoodGradZ {
        double likelihood;
        std::vector<double> grad, grad_z;
        int32_t status;
    };
    LikelihoodGradZ likelihood_grad_z(const double *theta, int64_t theta_len, double sigma2, double noise) {
        LikelihoodGradZ r{0.0, std::vector<double>((size_t)(w_star().second + 2)), std::vector<double>((size_t)(nz() * d_)), 0};
        check(egx_sgp_likelihood_grad_z(h_.get(), theta, theta_len, sigma2, noise, &r.likelihood, r.grad.data(), r.grad_z.data(),
                                        &r.status));
        return r;
    }
    // the inducing points (nz x d row-major): replace them (un-fits the model) / read the current ones
    void set_inducings(const double *z) { check(egx_sgp_set_inducings(h_.get(), z)); }
    std::vector<double> inducings() const {
        std::vector<double> z((size_t)(nz() * d_));
        check(egx_sgp_get_inducings(h_.get(), z.data()));
        return z;
    }
    // fit_lbfgs, then one more L-BFGS in which the inducing points move inside [z_lo, z_hi] (d each; nullptr: the range of the
    // training inputs): egx_sgp_fit_lbfgs_z.  max_iter_z == 0 is fit_lbfgs.
    int64_t fit_lbfgs_z(const double *params0s, int64_t n_starts, const double *lo, const double *hi, bool estimate_noise,
                        double noise_fixed, int64_t max_iter = 50, const double *z_lo = nullptr, const double *z_hi = nullptr,
                        int64_t max_iter_z = 50) {
        int64_t n_evals = 0;
        check(egx_sgp_fit_lbfgs_z(h_.get(), params0s, n_starts, lo, hi, estimate_noise ? 1 : 0, noise_fixed, max_iter, z_lo, z_hi,
                                  max_iter_z, &n_evals));
        return n_evals;
    }
    int64_t nz() const {
        int64_t v = 0;
        check(egx_sgp_dims(h_.get(), nullptr, nullptr, &v));
        return v;
    }
    std::vector<double> predict(const double *x, int64_t m) const {
        std::vector<double> y((size_t)m);
        check(egx_sgp_predict(h_.get(), x, m, y.data()));
        return y;
    }
    std::vector<double> predict_var(const double *x, int64_t m) const {
        std::vector<double> v((size_t)m);
        check(egx_sgp_predict_var(h_.get(), x, m, v.data()));
        return v;
    }
    std::pair<std::vector<double>, std::vector<double>> predict_valvar(const double *x, int64_t m) const {
        std::vector<double> y((size_t)m), v((size_t)m);
        check(egx_sgp_predict_valvar(h_.get(), x, m, y.data(), v.data()));
        return {std::move(y), std::move(v)};
    }
    // analytic (m x d) row-major gradients: the closed form the reference's central differences (:298-336) approximate
    std::vector<double> predict_gradients(const double *x, int64_t m) const {
        std::vector<double> g((size_t)(m * d_));
        check(egx_sgp_predict_gradients(h_.get(), x, m, g.data()));
        return g;
    }
    std::vector<double> predict_var_gradients(const double *x, int64_t m) const {
        std::vector<double> g((size_t)(m * d_));
        check(egx_sgp_predict_var_gradients(h_.get(), x, m, g.data()));
        return g;
    }
    std::pair<std::vector<double>, std::vector<double>> predict_valvar_gradients(const double *x, int64_t m) const {
        std::vector<double> gy((size_t)(m * d_)), gv((size_t)(m * d_));
        check(egx_sgp_predict_valvar_gradients(h_.get(), x, m, gy.data(), gv.data()));
        return {std::move(gy), std::move(gv)};
    }
    // :338-362 -> (m x n_traj) row-major around predict(x) with the PRIOR covariance sigma2 r(x, x) (the reference's definition)
    std::vector<double> sample(const double *x, int64_t m, int64_t n_traj, egx_sample_method method = EGX_SAMPLE_PSD,
                               uint64_t seed = 0, const double *z = nullptr, double *tau = nullptr) const {
        std::vector<double> t((size_t)(m * n_traj));
        check(egx_sgp_sample(h_.get(), x, m, n_traj, method, seed, z, t.data(), tau));
        return t;
    }
    std::vector<double> sample_chol(const double *x, int64_t m, int64_t n_traj, uint64_t seed = 0) const {
        return sample(x, m, n_traj, EGX_SAMPLE_CHOLESKY, seed);
    }
    std::pair<int64_t, int64_t> dims() const { return {d_, 1}; }
    egx_sgp *handle() const { return h_.get(); }

  private:
    struct Deleter {
        void operator()(egx_sgp *p) const { egx_sgp_destroy(p); }
    };
    std::unique_ptr<egx_sgp, Deleter> h_;
    int64_t d_ = 0;
};

inline std::vector<GaussianProcess> GpParams::fit_group(const double *x, const double *y, int64_t n, int64_t d, int32_t k) const {
    if (tuning_.kind == ThetaTuning::Kind::Partial)
        throw InvalidValueError(EGX_ERR_INVALID_VALUE, "fit_group: ThetaTuning::Fixed or ::Full");
    if (has_kpls_) throw InvalidValueError(EGX_ERR_INVALID_VALUE, "fit_group: kpls_dim / w_star are not supported, fit the members one by one");
    egx_gp_config cfg;
    egx_gp_config_default(&cfg);
    cfg.corr = (int32_t)corr_;
    cfg.mean = (int32_t)mean_;
    cfg.nugget = nugget_;
    cfg.device = device_;
    std::vector<egx_gp *> raw((size_t)k, nullptr);
    check(egx_gp_create_group(&cfg, x, y, n, d, k, raw.data()));
    std::vector<GaussianProcess> out((size_t)k);
    for (int32_t j = 0; j < k; j++) {
        out[(size_t)j].h_.reset(raw[(size_t)j]);
        out[(size_t)j].d_ = d;
        out[(size_t)j].n_evals_ = 1;
    }
    int64_t hh = 0;
    check(egx_gp_dims(raw[0], nullptr, nullptr, nullptr, &hh));
    if (tuning_.init.size() != 1 && tuning_.init.size() != (size_t)hh)
        throw InvalidValueError(EGX_ERR_INVALID_VALUE, "Initial guess for theta should be either 1-dim or dim of xtrain, got " +
                                                           std::to_string(tuning_.init.size()));
    std::vector<double> thetas((size_t)k * (size_t)hh);
    for (size_t i = 0; i < thetas.size(); i++) thetas[i] = tuning_.init[tuning_.init.size() == 1 ? 0 : i % (size_t)hh];
    if (tuning_.kind == ThetaTuning::Kind::Fixed) {
        check(egx_gp_finalize_multi(raw.data(), k, thetas.data(), hh));
    } else {
        // ThetaTuning::Full for every member (round 6, egx_gp_fit_multi): the tuned fit the expert loop runs per cluster
        // (crates/moe/src/algorithm.rs:209-262 -> crates/gp/src/algorithm.rs:921-945), all models' COBYLA machines in lock-step;
        // the same starts for every model, as the reference's fits draw theirs from one fixed seed (optimization.rs:49-66)
        const size_t h = (size_t)hh;
        if (tuning_.bounds.size() != 1 && tuning_.bounds.size() != h)
            throw InvalidValueError(EGX_ERR_INVALID_VALUE, "Bounds for theta should be either 1-dim or dim of xtrain (" + std::to_string(h) +
                                                               "), got " + std::to_string(tuning_.bounds.size()));
        std::vector<double> lo(h), hi(h);
        for (size_t i = 0; i < h; i++) {
            const auto &b = tuning_.bounds[tuning_.bounds.size() == 1 ? 0 : i];
            lo[i] = b.first, hi[i] = b.second;
        }
        const size_t ns = (size_t)std::max(0, n_start_) + 1;
        std::vector<double> starts(ns * h);
        for (size_t i = 0; i < h; i++) starts[i] = thetas[i];
        std::mt19937_64 rng(seed_);  // (the draw of GpParams::fit: a fit_group member gets the starts its lone fit gets)
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        for (size_t j = 0; j < h && ns > 1; j++) {
            std::vector<size_t> perm(ns - 1);
            for (size_t r = 0; r < ns - 1; r++) perm[r] = r;
            std::shuffle(perm.begin(), perm.end(), rng);
            for (size_t r = 0; r < ns - 1; r++) {
                const double u = ((double)perm[r] + u01(rng)) / (double)(ns - 1);
                starts[(r + 1) * h + j] = std::pow(10.0, std::log10(lo[j]) + u * (std::log10(hi[j]) - std::log10(lo[j])));
            }
        }
        std::vector<double> all((size_t)k * ns * h);
        for (int32_t j = 0; j < k; j++) std::copy(starts.begin(), starts.end(), all.begin() + (size_t)j * ns * h);
        std::vector<int64_t> ne((size_t)k, 0);
        check(egx_gp_fit_multi(raw.data(), k, all.data(), (int64_t)ns, lo.data(), hi.data(), (int64_t)h, max_eval_, ne.data()));
        for (int32_t j = 0; j < k; j++) out[(size_t)j].n_evals_ = ne[(size_t)j];
    }
    for (int32_t j = 0; j < k; j++) {  // theta() / variance() / likelihood() of every member, as `fit` leaves them
        GaussianProcess &gp = out[(size_t)j];
        gp.theta_.resize((size_t)hh);
        egx_gp_inner_view view{};
        view.theta = gp.theta_.data();
        view.sigma2 = &gp.sigma2_;
        view.likelihood = &gp.likelihood_;
        check(egx_gp_get_inner(raw[(size_t)j], &view));
    }
    return out;
}

inline GaussianProcess GpParams::fit(const double *x, int64_t n, int64_t d, const double *y) const {
    egx_gp_config cfg;
    egx_gp_config_default(&cfg);
    cfg.corr = (int32_t)corr_;
    cfg.mean = (int32_t)mean_;
    cfg.nugget = nugget_;
    cfg.device = device_;
    const bool tuned = tuning_.kind != ThetaTuning::Kind::Fixed;
    cfg.n_workspaces = tuned ? std::max(1, std::min(n_workspaces_, n_start_ + 1)) : std::max(1, n_workspaces_);
    std::vector<double> w;  // outlives egx_gp_create, which copies it
    if (has_kpls_) {
        if (w_star_.empty()) {
            w = pls_rotations(x, y, n, d, kpls_dim_, device_);
        } else {
            if (kpls_dim_ < 1 || kpls_dim_ > d || w_star_.size() != (size_t)(d * kpls_dim_))
                throw InvalidValueError(EGX_ERR_INVALID_VALUE, "w_star must hold d x kpls_dim values, 1 <= kpls_dim <= d");
            w = w_star_;
        }
        cfg.w_star = w.data();
        cfg.kpls_dim = kpls_dim_;
    }
    egx_gp *raw = nullptr;
    check(egx_gp_create(&cfg, x, y, n, d, &raw));
    GaussianProcess gp;
    gp.h_.reset(raw);
    gp.d_ = d;
    gp.kpls_dim_ = has_kpls_ ? kpls_dim_ : 0;
    int64_t hh = 0;
    check(egx_gp_dims(raw, nullptr, nullptr, nullptr, &hh));
    const size_t h = (size_t)hh;
    if (tuning_.init.size() != 1 && tuning_.init.size() != h)  // a panic in the reference, algorithm.rs:829-838
        throw InvalidValueError(EGX_ERR_INVALID_VALUE,
                                "Initial guess for theta should be either 1-dim or dim of xtrain (w_star.ncols()), got " +
                                    std::to_string(tuning_.init.size()));
    std::vector<double> theta0(h);
    for (size_t i = 0; i < h; i++) theta0[i] = tuning_.init[tuning_.init.size() == 1 ? 0 : i];
    if (!tuned) {
        check(egx_gp_finalize(raw, theta0.data(), (int64_t)h));
        gp.n_evals_ = 1;
    } else {
        if (tuning_.bounds.size() != 1 && tuning_.bounds.size() != h)  // algorithm.rs:901-912
            throw InvalidValueError(EGX_ERR_INVALID_VALUE, "Bounds for theta should be either 1-dim or dim of xtrain (" +
                                                               std::to_string(h) + "), got " +
                                                               std::to_string(tuning_.bounds.size()));
        std::vector<int64_t> active;
        if (tuning_.kind == ThetaTuning::Kind::Partial) active = tuning_.active;
        else for (size_t i = 0; i < h; i++) active.push_back((int64_t)i);
        std::sort(active.begin(), active.end());
        const size_t k = active.size();
        std::vector<double> lo(k), hi(k);
        for (size_t i = 0; i < k; i++) {
            const auto &b = tuning_.bounds[tuning_.bounds.size() == 1 ? 0 : (size_t)active[i]];
            lo[i] = b.first;
            hi[i] = b.second;
        }
        // prepare_multistart, optimization.rs:26-71: row 0 = the user's theta0, rows 1.. a Latin hypercube in log10
        // bounds (the reference's maximin-optimised, Xoshiro-seeded design is not reproducible here: parity-unpinned)
        const size_t ns = (size_t)std::max(0, n_start_) + 1;
        std::vector<double> starts(ns * k);
        for (size_t i = 0; i < k; i++) starts[i] = theta0[(size_t)active[i]];
        std::mt19937_64 rng(seed_);
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        for (size_t j = 0; j < k && ns > 1; j++) {
            std::vector<size_t> perm(ns - 1);
            for (size_t r = 0; r < ns - 1; r++) perm[r] = r;
            std::shuffle(perm.begin(), perm.end(), rng);
            for (size_t r = 0; r < ns - 1; r++) {
                const double u = ((double)perm[r] + u01(rng)) / (double)(ns - 1);
                starts[(r + 1) * k + j] = std::pow(10.0, std::log10(lo[j]) + u * (std::log10(hi[j]) - std::log10(lo[j])));
            }
        }
        int64_t ne = 0;
        if (tuning_.kind == ThetaTuning::Kind::Partial)
            check(egx_gp_fit_partial(raw, theta0.data(), active.data(), (int64_t)k, starts.data(), (int64_t)ns, lo.data(),
                                     hi.data(), (int64_t)k, max_eval_, &ne));
        else
            check(egx_gp_fit(raw, starts.data(), (int64_t)ns, lo.data(), hi.data(), (int64_t)k, max_eval_, &ne));
        gp.n_evals_ = ne;
    }
    gp.theta_.resize(h);
    egx_gp_inner_view view{};
    view.theta = gp.theta_.data();
    view.sigma2 = &gp.sigma2_;
    view.likelihood = &gp.likelihood_;
    check(egx_gp_get_inner(raw, &view));
    return gp;
}

// The posterior of k fitted models in one call (egx_gp_predict_valvar_multi): model j answers rows [j m, (j + 1) m) of xq
// (k x m x d, original units).  Members of one group (GpParams::fit_group) answer in lock-step, each bit for bit as its own
// batched predict_valvar: what the folds of a cross-validation ask (crates/moe/src/metrics.rs:19-144).  Returns (y, var), k x m.
inline std::pair<std::vector<double>, std::vector<double>> predict_valvar_group(const std::vector<const GaussianProcess *> &models,
                                                                                const double *xq, int64_t m) {
    std::vector<egx_gp *> hs;
    for (const GaussianProcess *g : models) hs.push_back(g->handle());
    std::vector<double> y(hs.size() * (size_t)m), v(hs.size() * (size_t)m);
    check(egx_gp_predict_valvar_multi(hs.data(), (int32_t)hs.size(), xq, m, y.data(), v.data()));
    return {std::move(y), std::move(v)};
}

// The x-gradients of k fitted models in one call (egx_gp_predict_valvar_gradients_multi): model j answers rows [j m, (j + 1) m)
// of xq.  Members of one group answer in lock-step, each bit for bit as its own predict_valvar_gradients (m > 8): what an
// optimiser asks of its objective and constraint surrogates.  Returns (grad_y, grad_var), k x m x d each.
inline std::pair<std::vector<double>, std::vector<double>> predict_valvar_gradients_group(
    const std::vector<const GaussianProcess *> &models, const double *xq, int64_t m, int64_t d) {
    std::vector<egx_gp *> hs;
    for (const GaussianProcess *g : models) hs.push_back(g->handle());
    std::vector<double> gy(hs.size() * (size_t)m * (size_t)d), gv(hs.size() * (size_t)m * (size_t)d);
    check(egx_gp_predict_valvar_gradients_multi(hs.data(), (int32_t)hs.size(), xq, m, gy.data(), gv.data()));
    return {std::move(gy), std::move(gv)};
}

// The likelihood and dL/dtheta of k models in one call (egx_gp_likelihood_grad_multi): row j of thetas (k x theta_len) for
// models[j].  Members of one group (GpParams::fit_group) run every stage in lock-step, each row bit for bit the model's own
// egx_gp_likelihood_grad.  The call UN-FITS the models: fit them again (fit_lbfgs_group, egx_gp_finalize_multi) before predicting.
inline GaussianProcess::LikelihoodGrad likelihood_grad_group(const std::vector<GaussianProcess *> &models, const double *thetas,
                                                             int64_t theta_len) {
    std::vector<egx_gp *> hs;
    for (const GaussianProcess *g : models) hs.push_back(g->handle());
    int64_t h = 0;
    if (!hs.empty()) check(egx_gp_dims(hs[0], nullptr, nullptr, nullptr, &h));
    GaussianProcess::LikelihoodGrad out;
    out.likelihood.resize(hs.size());
    out.gradient.assign(hs.size() * (size_t)h, 0.0);
    out.status.resize(hs.size());
    check(egx_gp_likelihood_grad_multi(hs.data(), (int32_t)hs.size(), thetas, theta_len, out.likelihood.data(), out.gradient.data(),
                                       out.status.data()));
    return out;
}

// The projected L-BFGS multistart on the theta-gradient for k models in one call (egx_gp_fit_lbfgs_multi): theta0s
// (k x n_starts x h, linear theta units), lo / hi (bounds_len = 1 or h).  Members of one group advance in lock-step; every model
// ends as egx_gp_fit_lbfgs leaves a one-workspace handle of its training set, and its theta() / variance() / likelihood() /
// n_evals() are those of the new fit.  Returns the evaluations per model.
inline std::vector<int64_t> fit_lbfgs_group(const std::vector<GaussianProcess *> &models, const double *theta0s, int64_t n_starts,
                                            const double *lo, const double *hi, int64_t bounds_len, int64_t max_iter = 50) {
    std::vector<egx_gp *> hs;
    for (const GaussianProcess *g : models) hs.push_back(g->handle());
    std::vector<int64_t> ne(hs.size(), 0);
    check(egx_gp_fit_lbfgs_multi(hs.data(), (int32_t)hs.size(), theta0s, n_starts, lo, hi, bounds_len, max_iter, ne.data()));
    for (size_t j = 0; j < models.size(); j++) models[j]->adopt_fit(ne[j]);
    return ne;
}

// GpMixture::predict / predict_var over fitted experts of THIS process (crates/moe/src/algorithm.rs:411-423, 670-685 smooth;
// :879-935 hard): probas (m x n_experts row-major) are the responsibilities, xq (m x d) in original units.
inline std::pair<std::vector<double>, std::vector<double>> moe_predict_valvar(const std::vector<const GaussianProcess *> &experts,
                                                                              const double *probas, const double *xq,
                                                                              int64_t m, int64_t d, bool smooth) {
    std::vector<egx_gp *> hs;
    std::vector<int32_t> ids;
    for (size_t e = 0; e < experts.size(); e++) {
        hs.push_back(experts[e]->handle());
        ids.push_back((int32_t)e);
    }
    std::vector<double> val((size_t)m), var((size_t)m);
    check(egx_moe_predict_valvar(nullptr, hs.data(), ids.data(), (int64_t)hs.size(), (int64_t)hs.size(), probas, xq, m, d,
                                 smooth ? 1 : 0, val.data(), var.data()));
    return {std::move(val), std::move(var)};
}

// GpMixture::predict_gradients / predict_var_gradients (crates/moe/src/algorithm.rs:691-783 smooth, :942-1010 hard) over
// fitted experts of THIS process: dprobas (m x n_experts x d, GaussianMixture::predict_probas_derivatives) is read by the
// smooth recombination only.  Returns (d val / dx, d var / dx), each (m x d) row-major.
inline std::pair<std::vector<double>, std::vector<double>> moe_predict_valvar_gradients(
    const std::vector<const GaussianProcess *> &experts, const double *probas, const double *dprobas, const double *xq, int64_t m,
    int64_t d, bool smooth) {
    std::vector<egx_gp *> hs;
    std::vector<int32_t> ids;
    for (size_t e = 0; e < experts.size(); e++) {
        hs.push_back(experts[e]->handle());
        ids.push_back((int32_t)e);
    }
    std::vector<double> gy((size_t)(m * d)), gv((size_t)(m * d));
    check(egx_moe_predict_valvar_gradients(nullptr, hs.data(), ids.data(), (int64_t)hs.size(), (int64_t)hs.size(), probas, dprobas,
                                           xq, m, d, smooth ? 1 : 0, gy.data(), gv.data()));
    return {std::move(gy), std::move(gv)};
}

// GaussianMixtureModel::params(n_clusters).n_runs(n_runs).fit(data) (crates/moe/src/algorithm.rs:120-123) through egx_gmm_fit:
// full-covariance EM on data (n x dim row-major), restart r from init_means[r] (n_clusters x dim), the restarts in lock-step
// on the GPU.  LinalgError when every restart failed.
struct GmmFit {
    std::vector<double> weights, means, covariances;  // the best restart: (k), (k x dim), (k x dim x dim)
    std::vector<double> lower_bounds;                 // per restart (NaN: failed)
    std::vector<int32_t> n_iters, statuses;           // per restart; 0 converged, 1 stopped at max_iter, 2 failed
    int32_t best_run = -1;
};
using GmmFitFn = decltype(&egx_gmm_fit);
inline GmmFit gmm_fit_with(GmmFitFn fit, const double *data, int64_t n, int32_t dim, int32_t n_clusters,
                           const std::vector<double> &init_means, const egx_gmm_config *config) {
    egx_gmm_config cfg;
    if (config)
        cfg = *config;
    else
        egx_gmm_config_default(&cfg);
    cfg.n_clusters = n_clusters;
    const size_t per = (size_t)(n_clusters > 0 ? n_clusters : 1) * (size_t)(dim > 0 ? dim : 1);
    cfg.n_runs = (int32_t)(init_means.size() / per);
    if (cfg.n_runs < 1 || (size_t)cfg.n_runs * per != init_means.size())
        throw InvalidValueError(EGX_ERR_INVALID_VALUE, "gmm_fit: init_means must hold n_runs x n_clusters x dim values");
    GmmFit f;
    f.weights.resize((size_t)n_clusters);
    f.means.resize(per);
    f.covariances.resize(per * (size_t)dim);
    f.lower_bounds.resize((size_t)cfg.n_runs);
    f.n_iters.resize((size_t)cfg.n_runs);
    f.statuses.resize((size_t)cfg.n_runs);
    check(fit(&cfg, data, n, dim, init_means.data(), f.weights.data(), f.means.data(), f.covariances.data(),
              f.lower_bounds.data(), f.n_iters.data(), f.statuses.data(), &f.best_run, nullptr, nullptr, nullptr));
    return f;
}
inline GmmFit gmm_fit(const double *data, int64_t n, int32_t dim, int32_t n_clusters, const std::vector<double> &init_means,
                      const egx_gmm_config *config = nullptr) {
    return gmm_fit_with(&egx_gmm_fit, data, n, dim, n_clusters, init_means, config);
}
// ... through egx_gmm_fit_wide: rows up to 128 wide (dim <= 128), the same outputs and errors
inline GmmFit gmm_fit_wide(const double *data, int64_t n, int32_t dim, int32_t n_clusters, const std::vector<double> &init_means,
                           const egx_gmm_config *config = nullptr) {
    return gmm_fit_with(&egx_gmm_fit_wide, data, n, dim, n_clusters, init_means, config);
}

// EGO's infill criterion on fitted models (egx_infill_*, egx_gp.h): the objective the infill optimiser minimises and its
// x-gradient for m points per call (crates/ego/src/criteria, utils/cstr_pof.rs, solver/solver_computations.rs:356-475), the
// scaling pass (:132-193) and the lock-step multistart (solver_infill_optim.rs:148-236).  The models are borrowed and must
// outlive the object.
//
// A surrogate of the mixture form (egx_infill_create_mix): the experts of a GpMixture (borrowed) and a copy of its Gaussian
// mixture, as egx_gmx_predict_probas takes it.  One expert: the mixture is not read and may stay empty.
// With SPARSE experts (egx_infill_create_any): build the surrogate from a SparseGaussianProcess, or add() experts of either
// kind in cluster order; `models` then holds the tagged references and `experts` stays empty.
struct InfillSurrogate {
    std::vector<const GaussianProcess *> experts;  // one per cluster
    std::vector<double> weights, means, precisions_chol;  // k, k x d, k x d x d
    double heaviside_factor = 1.0;
    bool smooth = true;  // false: hard recombination
    std::vector<egx_model_ref> models;  // dense and sparse experts, one per cluster (non-empty: used instead of `experts`)
    int64_t d = 0;                      // inputs of the models added

    InfillSurrogate() = default;
    explicit InfillSurrogate(const SparseGaussianProcess &sgp) { add(sgp); }  // one sparse expert, no mixture
    InfillSurrogate &add(const GaussianProcess &gp) {
        models.push_back(egx_model_ref{EGX_MODEL_GP, gp.handle()});
        d = gp.dims().first;
        return *this;
    }
    InfillSurrogate &add(const SparseGaussianProcess &sgp) {
        models.push_back(egx_model_ref{EGX_MODEL_SGP, sgp.handle()});
        d = sgp.dims().first;
        return *this;
    }
};

// QEiStrategy, crates/ego/src/types.rs:59-68
enum class QEiStrategy {
    KrigingBeliever = EGX_QEI_KB,
    KrigingBelieverLowerBound = EGX_QEI_KB_LB,
    KrigingBelieverUpperBound = EGX_QEI_KB_UB,
    ConstantLiarMinimum = EGX_QEI_CL_MIN
};

class InfillObjective {
  public:
    // what surrogate j was recombined from (egx_infill_eval_experts): expert-major parts, responsibilities, their derivatives
    struct ExpertParts {
        std::vector<double> mean, var, grad_mean, grad_var, probas, dprobas;  // k m, k m, k m d, k m d, m k, m k d
    };
    // surrogates[0] is the objective, the others the constraints (one tolerance each)
    InfillObjective(const std::vector<InfillSurrogate> &surrogates, const std::vector<double> &cstr_tols,
                    egx_infill_criterion criterion, double fmin, double sigma_weight = 1.0, bool feasibility = true) {
        if (surrogates.empty() || surrogates.size() != cstr_tols.size() + 1)
            throw InvalidValueError(EGX_ERR_INVALID_VALUE, "InfillObjective: an objective surrogate and one tolerance per constraint");
        egx_infill_config cfg;
        egx_infill_config_default(&cfg);
        cfg.criterion = criterion;
        cfg.fmin = fmin;
        cfg.sigma_weight = sigma_weight;
        cfg.feasibility = feasibility ? 1 : 0;
        bool tagged = false;
        for (const InfillSurrogate &sv : surrogates) tagged |= !sv.models.empty();
        if (tagged) {  // sparse experts somewhere: every surrogate as tagged references (egx_infill_create_any)
            std::vector<std::vector<egx_model_ref>> refs(surrogates.size());
            std::vector<egx_infill_surrogate_any> raw_a(surrogates.size());
            for (size_t j = 0; j < surrogates.size(); j++) {
                const InfillSurrogate &sv = surrogates[j];
                refs[j] = sv.models;
                if (refs[j].empty())
                    for (const GaussianProcess *e : sv.experts) refs[j].push_back(egx_model_ref{EGX_MODEL_GP, e ? e->handle() : nullptr});
                n_experts_.push_back((int64_t)refs[j].size());
                raw_a[j].experts = refs[j].data();
                raw_a[j].n_experts = (int32_t)refs[j].size();
                raw_a[j].weights = sv.weights.empty() ? nullptr : sv.weights.data();
                raw_a[j].means = sv.means.empty() ? nullptr : sv.means.data();
                raw_a[j].precisions_chol = sv.precisions_chol.empty() ? nullptr : sv.precisions_chol.data();
                raw_a[j].heaviside_factor = sv.heaviside_factor;
                raw_a[j].smooth = sv.smooth ? 1 : 0;
            }
            egx_infill *raw = nullptr;
            check(egx_infill_create_any(&cfg, raw_a.data(), cstr_tols.data(), (int32_t)cstr_tols.size(), &raw));
            h_.reset(raw);
            d_ = !surrogates[0].models.empty() ? surrogates[0].d : surrogates[0].experts[0]->dims().first;
            k_ = (int64_t)cstr_tols.size();
            return;
        }
        std::vector<std::vector<egx_gp *>> hs(surrogates.size());
        std::vector<egx_infill_surrogate> raw_s(surrogates.size());
        for (size_t j = 0; j < surrogates.size(); j++) {
            const InfillSurrogate &sv = surrogates[j];
            for (const GaussianProcess *e : sv.experts) hs[j].push_back(e ? e->handle() : nullptr);
            n_experts_.push_back((int64_t)hs[j].size());
            raw_s[j].experts = hs[j].data();
            raw_s[j].n_experts = (int32_t)hs[j].size();
            raw_s[j].weights = sv.weights.empty() ? nullptr : sv.weights.data();
            raw_s[j].means = sv.means.empty() ? nullptr : sv.means.data();
            raw_s[j].precisions_chol = sv.precisions_chol.empty() ? nullptr : sv.precisions_chol.data();
            raw_s[j].heaviside_factor = sv.heaviside_factor;
            raw_s[j].smooth = sv.smooth ? 1 : 0;
        }
        egx_infill *raw = nullptr;
        check(egx_infill_create_mix(&cfg, raw_s.data(), cstr_tols.data(), (int32_t)cstr_tols.size(), &raw));
        h_.reset(raw);
        d_ = surrogates[0].experts[0]->dims().first;
        k_ = (int64_t)cstr_tols.size();
    }
    ExpertParts eval_experts(int32_t j, const double *x, int64_t m) const {
        if (j < 0 || (size_t)j >= n_experts_.size()) throw InvalidValueError(EGX_ERR_INVALID_VALUE, "InfillObjective: no such surrogate");
        const size_t k = (size_t)n_experts_[(size_t)j], mm = (size_t)m, d = (size_t)d_;
        ExpertParts p;
        p.mean.resize(k * mm), p.var.resize(k * mm), p.grad_mean.resize(k * mm * d), p.grad_var.resize(k * mm * d);
        p.probas.resize(mm * k), p.dprobas.resize(mm * k * d);
        check(egx_infill_eval_experts(h_.get(), j, x, m, p.mean.data(), p.var.data(), p.grad_mean.data(), p.grad_var.data(),
                                      p.probas.data(), p.dprobas.data()));
        return p;
    }
    InfillObjective(const GaussianProcess &obj_model, const std::vector<const GaussianProcess *> &cstr_models,
                    const std::vector<double> &cstr_tols, egx_infill_criterion criterion, double fmin, double sigma_weight = 1.0,
                    bool feasibility = true) {
        if (cstr_models.size() != cstr_tols.size())
            throw InvalidValueError(EGX_ERR_INVALID_VALUE, "InfillObjective: one tolerance per constraint model");
        egx_infill_config cfg;
        egx_infill_config_default(&cfg);
        cfg.criterion = criterion;
        cfg.fmin = fmin;
        cfg.sigma_weight = sigma_weight;
        cfg.feasibility = feasibility ? 1 : 0;
        std::vector<egx_gp *> hs;
        for (const GaussianProcess *m : cstr_models) hs.push_back(m->handle());
        egx_infill *raw = nullptr;
        check(egx_infill_create(&cfg, obj_model.handle(), hs.data(), cstr_tols.data(), (int32_t)hs.size(), &raw));
        h_.reset(raw);
        d_ = obj_model.dims().first;
        k_ = (int64_t)hs.size();
        n_experts_.assign((size_t)k_ + 1, 1);
    }
    // InfillCriterion::value through eval_infill_obj_with_cstrs: (m) values of the minimised objective
    std::vector<double> value(const double *x, int64_t m) const {
        std::vector<double> v((size_t)m);
        check(egx_infill_eval(h_.get(), x, m, v.data(), nullptr, nullptr));
        return v;
    }
    // ... and eval_grad_infill_obj_with_cstrs: (m) values, (m x d) gradients
    std::pair<std::vector<double>, std::vector<double>> value_and_grad(const double *x, int64_t m) const {
        std::vector<double> v((size_t)m), g((size_t)(m * width()));
        check(egx_infill_eval(h_.get(), x, m, v.data(), g.data(), nullptr));
        return {std::move(v), std::move(g)};
    }
    struct Scaling {
        double scale_ic = 1.0, scale = 1.0;
        std::vector<double> scale_cstr;
    };
    Scaling scaling(const double *pts, int64_t npts) {  // compute_scaling; scale_ic and scale are stored in the object
        Scaling s;
        s.scale_cstr.assign((size_t)(k_ > 0 ? k_ : 1), 0.0);
        check(egx_infill_scaling(h_.get(), pts, npts, &s.scale_ic, &s.scale, s.scale_cstr.data()));
        s.scale_cstr.resize((size_t)k_);
        return s;
    }
    void set_params(double fmin, double sigma_weight, double scale_ic, double scale, bool feasibility) {
        check(egx_infill_set_params(h_.get(), fmin, sigma_weight, scale_ic, scale, feasibility ? 1 : 0));
    }
    struct Optimum {
        double f = 0.0;
        std::vector<double> x;
        std::vector<int64_t> evals;
        int64_t rounds = 0, best_start = 0;
        bool finite = true;  // false: no start ended at a finite value (f = +inf)
    };
    Optimum optimize(const double *lo, const double *hi, const double *x_start, int64_t n_start, int64_t max_eval = 0) {
        Optimum o;
        o.x.assign((size_t)width(), 0.0);
        o.evals.assign((size_t)n_start, 0);
        egx_infill_stats st{0, 0, o.evals.data()};
        const int32_t rc = egx_infill_optimize(h_.get(), lo, hi, x_start, n_start, max_eval, &o.f, o.x.data(), &st);
        if (rc != EGX_ERR_NO_FINITE_START) check(rc);
        o.finite = rc == EGX_SUCCESS;
        o.rounds = st.rounds;
        o.best_start = st.best_start;
        return o;
    }
    // ---- the constraint surrogates as constraints of the optimiser (cstr_infill = false; solver_infill_optim.rs:148-204)
    void set_cstr_strategy(egx_cstr_strategy strategy, const std::vector<double> &scale_cstr = {}) {
        if (!scale_cstr.empty() && (int64_t)scale_cstr.size() != k_)
            throw InvalidValueError(EGX_ERR_INVALID_VALUE, "InfillObjective: one scale per constraint");
        check(egx_infill_set_cstr_strategy(h_.get(), strategy, scale_cstr.empty() ? nullptr : scale_cstr.data()));
    }
    std::pair<egx_cstr_strategy, std::vector<double>> cstr_strategy() const {
        int32_t s = 0;
        std::vector<double> sc((size_t)(k_ > 0 ? k_ : 1), 1.0);
        check(egx_infill_get_cstr_strategy(h_.get(), &s, sc.data()));
        sc.resize((size_t)k_);
        return {(egx_cstr_strategy)s, std::move(sc)};
    }
    struct Constraints {
        std::vector<double> value, cstr, grad, grad_cstr;  // m, m k, m d, m k d (the gradients empty unless asked for)
    };
    Constraints constraints(const double *x, int64_t m, bool grad = false) const {
        Constraints c;
        const size_t mm = (size_t)m, k = (size_t)k_, d = (size_t)width();
        c.value.resize(mm), c.cstr.resize(mm * k + 1);
        if (grad) c.grad.resize(mm * d), c.grad_cstr.resize(mm * k * d + 1);
        check(egx_infill_eval_cstr(h_.get(), x, m, c.value.data(), c.cstr.data(), grad ? c.grad.data() : nullptr,
                                   grad ? c.grad_cstr.data() : nullptr));
        c.cstr.resize(mm * k);
        if (grad) c.grad_cstr.resize(mm * k * d);
        return c;
    }
    struct ConstrainedOptimum {
        double f = 0.0, violation = 0.0;
        std::vector<double> x, c;
        std::vector<int64_t> evals;
        int64_t rounds = 0, best_start = 0;
        bool feasible = false, finite = true;
    };
    ConstrainedOptimum optimize_constrained(const double *lo, const double *hi, const double *x_start, int64_t n_start,
                                            int64_t max_eval = 0) {
        ConstrainedOptimum o;
        o.x.assign((size_t)width(), 0.0);
        o.c.assign((size_t)k_ + 1, 0.0);
        o.evals.assign((size_t)n_start, 0);
        egx_infill_cstr_stats st{0, 0, 0, 0.0, o.evals.data()};
        const int32_t rc = egx_infill_optimize_cstr(h_.get(), lo, hi, x_start, n_start, max_eval, &o.f, o.x.data(), o.c.data(), &st);
        if (rc != EGX_ERR_NO_FINITE_START) check(rc);
        o.c.resize((size_t)k_);
        o.finite = rc == EGX_SUCCESS;
        o.rounds = st.rounds, o.best_start = st.best_start;
        o.feasible = st.feasible != 0, o.violation = st.violation;
        return o;
    }
    // InfillOptimizer::Slsqp, the reference's default, as one call (egx_infill_optimize_slsqp); works in every strategy
    struct SlsqpOptimum : ConstrainedOptimum {
        std::vector<int32_t> stop;  // per start: 1 budget, 2 converged, 3 line search, 4 no finite start value, 5 inconsistent
    };
    SlsqpOptimum optimize_slsqp(const double *lo, const double *hi, const double *x_start, int64_t n_start, int64_t max_eval = 0) {
        SlsqpOptimum o;
        o.x.assign((size_t)width(), 0.0);
        o.c.assign((size_t)k_ + 1, 0.0);
        o.evals.assign((size_t)n_start, 0);
        o.stop.assign((size_t)n_start, 0);
        egx_infill_slsqp_stats st{0, 0, 0, 0.0, o.evals.data(), o.stop.data()};
        const int32_t rc = egx_infill_optimize_slsqp(h_.get(), lo, hi, x_start, n_start, max_eval, &o.f, o.x.data(), o.c.data(), &st);
        if (rc != EGX_ERR_NO_FINITE_START) check(rc);
        o.c.resize(cstr_strategy().first == EGX_CSTR_INFILL ? 0 : (size_t)k_);  // folded constraints: none are returned
        o.finite = rc == EGX_SUCCESS;
        o.rounds = st.rounds, o.best_start = st.best_start;
        o.feasible = st.feasible != 0, o.violation = st.violation;
        return o;
    }
    // ---- q points per iteration (solver_impl.rs:622-791): pending virtual observations the models are conditioned on, no refit
    void push_pending(const double *x, const double *y) { check(egx_infill_push_pending(h_.get(), x, y)); }
    void clear_pending() { check(egx_infill_clear_pending(h_.get())); }
    int32_t n_pending() const {
        int32_t q = 0;
        check(egx_infill_get_pending(h_.get(), &q, nullptr, nullptr, nullptr));
        return q;
    }
    // compute_virtual_point on the current (conditioned) models: 1 + n_cstr values
    std::vector<double> virtual_point(const double *x, QEiStrategy strategy = QEiStrategy::KrigingBeliever) const {
        std::vector<double> y((size_t)k_ + 1);
        check(egx_infill_virtual_point(h_.get(), x, (int32_t)strategy, y.data()));
        return y;
    }
    struct Batch {
        std::vector<double> x, y_virtual, f;  // n_found d, n_found (1 + n_cstr), n_found
        int32_t n_found = 0;
    };
    // x_start: q x n_start x d; an error at a later step returns the steps before it (their points stay pending)
    Batch optimize_batch(const double *lo, const double *hi, const double *x_start, int64_t n_start, int32_t q,
                         QEiStrategy strategy = QEiStrategy::KrigingBeliever, bool slsqp = true, int64_t max_eval = 0,
                         const double *scaling_points = nullptr, int64_t n_scaling = 0) {
        egx_infill_batch_config cfg;
        egx_infill_batch_config_default(&cfg);
        cfg.strategy = (int32_t)strategy;
        cfg.optimizer = slsqp ? EGX_BATCH_SLSQP : EGX_BATCH_COBYLA;
        cfg.max_eval = max_eval;
        cfg.scaling_points = scaling_points, cfg.n_scaling = n_scaling;
        Batch b;
        const size_t qq = (size_t)(q > 0 ? q : 0), nm = (size_t)k_ + 1;
        b.x.assign(qq * (size_t)d_ + 1, 0.0), b.y_virtual.assign(qq * nm + 1, 0.0), b.f.assign(qq + 1, 0.0);
        const int32_t rc = egx_infill_optimize_batch(h_.get(), &cfg, lo, hi, x_start, n_start, q, b.x.data(), b.y_virtual.data(),
                                                     b.f.data(), &b.n_found);
        if (rc != EGX_SUCCESS && b.n_found == 0) check(rc);
        b.x.resize((size_t)b.n_found * (size_t)d_), b.y_virtual.resize((size_t)b.n_found * nm), b.f.resize((size_t)b.n_found);
        return b;
    }
    // ---- active coordinates (CoEGO): while set, points, limits and gradients above are n_active wide (egx_infill_set_active);
    // value j of a compact row stands for column active[j], the other columns are x_base's
    void set_active(const std::vector<int> &active, const std::vector<double> &x_base) {
        if ((int64_t)x_base.size() != d_) throw InvalidValueError(EGX_ERR_INVALID_VALUE, "InfillObjective: x_base must hold d values");
        const std::vector<int32_t> idx(active.begin(), active.end());
        check(egx_infill_set_active(h_.get(), idx.data(), (int32_t)idx.size(), x_base.data()));
        w_ = (int64_t)idx.size();
    }
    void clear_active() {
        check(egx_infill_clear_active(h_.get()));
        w_ = 0;
    }
    struct Active {
        std::vector<int> indices;    // empty: no activity
        std::vector<double> x_base;
    };
    Active active() const {
        int32_t n = 0;
        std::vector<int32_t> idx((size_t)d_);
        std::vector<double> xb((size_t)d_);
        check(egx_infill_get_active(h_.get(), &n, idx.data(), xb.data()));
        Active a;
        if (n > 0) a.indices.assign(idx.begin(), idx.begin() + n), a.x_base = std::move(xb);
        return a;
    }
    int64_t width() const { return w_ > 0 ? w_ : d_; }  // of a point, a limit, a gradient row
    // the lengths of the runs an evaluation walks (egx_infill_get_runs); they sum to 1 + n_cstr
    std::vector<int32_t> runs() const {
        int32_t n = 0;
        std::vector<int32_t> len((size_t)k_ + 1, 0);
        check(egx_infill_get_runs(h_.get(), &n, len.data()));
        len.resize((size_t)n);
        return len;
    }
    egx_infill *handle() const { return h_.get(); }

  private:
    struct Deleter {
        void operator()(egx_infill *p) const { egx_infill_destroy(p); }
    };
    std::unique_ptr<egx_infill, Deleter> h_;
    int64_t d_ = 0, k_ = 0, w_ = 0;   // w_: n_active while an activity is set
    std::vector<int64_t> n_experts_;  // per surrogate
};

// device resources destroyed models left in the library's pool (a model of the same shape created next reuses them)
inline int64_t trim() { return egx_trim(); }  // bytes freed
struct PoolStats { int64_t cached_bytes = 0, hits = 0, misses = 0; };
inline PoolStats pool_stats() {
    PoolStats s;
    egx_pool_stats(&s.cached_bytes, &s.hits, &s.misses);
    return s;
}

// chain launches that ran into their wait bound, and how many of those evaluations were run again by separate launches
struct ChainStats { int64_t aborted = 0, retried = 0; };
inline ChainStats chain_stats() {
    ChainStats s;
    egx_chain_stats(&s.aborted, &s.retried);
    return s;
}

// Kriging = constant mean + squared exponential, algorithm.rs:244-249
struct Kriging {
    static GpParams params() { return GpParams(Mean::Constant, Corr::SquaredExponential); }
};

}  // namespace egobox
#endif  // EGX_GP_HPP
