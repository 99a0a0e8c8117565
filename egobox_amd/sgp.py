"""Sparse Gaussian process (FITC / VFE) on the GPU -- mirror of the reference's two surfaces for it:

    Rust    SparseGaussianProcess::params(Inducings::Located(z) | Randomized(n)).sparse_method(..).noise_variance(..)
            .theta_init(..).theta_bounds(..).n_start(..).max_eval(..).seed(..).fit(x, y)
            -> predict / predict_var / theta / variance / noise_variance / likelihood / inducings
            (crates/gp/src/sparse_parameters.rs, sparse_algorithm.rs:145-300, 422-650)
    Python  SparseGpx.builder(corr_spec, theta_init, theta_bounds, n_start, nz | z, method, seed).fit(xt, yt)
            (python/src/sparse_gp_mix.rs)

The sparse GP works on raw x / y (no normalisation) with a zero trend.  Inducings.Randomized(n) draws rows of x with
numpy's generator: the reference shuffles with Rust's Xoshiro256Plus, so the drawn points (and everything fitted from
them) are not comparable digit by digit; with Located(z) the likelihood at given parameters is.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import gp as G
from .multistart import prepare_multistart

FITC, VFE = 0, 1
DEFAULT_NOISE_INIT = 1e-2                                   # ParamTuning::default, sparse_parameters.rs:33-39
DEFAULT_NOISE_BOUNDS = (100.0 * np.finfo(float).eps, 1e10)
DEFAULT_THETA_BOUNDS = (1e-2, 1e2)                          # sparse_parameters.rs:160-163


class Inducings:
    def __init__(self, kind, value):
        self.kind, self.value = kind, value

    @classmethod
    def Randomized(cls, n):
        return cls("Randomized", int(n))

    @classmethod
    def Located(cls, z):
        return cls("Located", np.atleast_2d(np.asarray(z, dtype=np.float64)))


class ParamTuning:
    """Noise variance: Fixed(c) or Optimized{init, bounds} (sparse_parameters.rs:13-40)."""

    def __init__(self, kind, init, bounds=None):
        self.kind, self.init, self.bounds = kind, float(init), bounds

    @classmethod
    def Fixed(cls, c):
        return cls("Fixed", c)

    @classmethod
    def Optimized(cls, init=DEFAULT_NOISE_INIT, bounds=DEFAULT_NOISE_BOUNDS):
        return cls("Optimized", init, tuple(bounds))


class SgpHandle:
    """Thin owner of an `egx_sgp*`."""

    def __init__(self, x, y, z, corr=0, method=FITC, nugget=G.DEFAULT_NUGGET, device=-1, w_star=None):
        self._lib = L.load()
        x = L.as_f64(x)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        y = L.as_f64(np.asarray(y, dtype=np.float64).reshape(-1))
        z = L.as_f64(z)
        if z.ndim == 1:
            z = z.reshape(-1, x.shape[1])
        if x.ndim != 2 or z.ndim != 2 or z.shape[1] != x.shape[1] or y.shape[0] != x.shape[0]:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, "x (n, d), y (n), z (nz, d) expected")
        cfg = L.SgpConfig()
        self._lib.egx_sgp_config_default(C.byref(cfg))
        cfg.corr, cfg.method, cfg.nugget, cfg.device = int(corr), int(method), float(nugget), int(device)
        h = C.c_void_p()
        L.check(self._lib.egx_sgp_create(C.byref(cfg), L.dptr(x), L.dptr(y), x.shape[0], x.shape[1], L.dptr(z),
                                         z.shape[0], C.byref(h)))
        self._h = h
        self.n, self.d, self.nz = x.shape[0], x.shape[1], z.shape[0]
        self.h = self.d  # theta components: the columns of the KPLS weights once `set_w_star` has set some
        self.z = z.copy()
        if w_star is not None:
            try:
                self.set_w_star(w_star)
            except Exception:
                self.close()
                raise

    def set_w_star(self, w):
        """KPLS weights (d, h), 1 <= h <= d, finite; None clears them (egx_sgp_set_w_star).  Un-fits the handle; theta then has
        h components everywhere, gradients are h + 2 long; `grad_z` and the inducing points stay (nz, d)."""
        if w is None:
            L.check(self._lib.egx_sgp_set_w_star(self._h, None, 0))
            self.h = self.d
            return
        w = np.ascontiguousarray(L.as_f64(w))
        if w.ndim != 2 or w.shape[0] != self.d:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"w_star must be ({self.d}, h), got {w.shape}")
        L.check(self._lib.egx_sgp_set_w_star(self._h, L.dptr(w), w.shape[1]))
        self.h = w.shape[1]

    def compute_w_star(self, k):
        """The PLS rotations (d, k) of the training set the handle holds, computed on the device (egx_sgp_compute_w_star: no
        upload) and installed as `set_w_star` installs them.  A constant response installs zeros.  Returns the weights."""
        L.check(self._lib.egx_sgp_compute_w_star(self._h, int(k)))
        self.h = int(k)
        return self.w_star()

    def w_star(self):
        """The KPLS weights (d, h), or None when none are set (egx_sgp_get_w_star)."""
        h = C.c_int64()
        L.check(self._lib.egx_sgp_get_w_star(self._h, None, C.byref(h)))
        w = np.full((self.d, h.value), np.nan)
        L.check(self._lib.egx_sgp_get_w_star(self._h, L.dptr(w), C.byref(h)))
        return None if np.isnan(w[0, 0]) else w

    def close(self):
        if getattr(self, "_h", None):
            self._lib.egx_sgp_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def likelihood(self, theta, sigma2, noise):
        th = L.as_f64(np.atleast_1d(theta), 1)
        lk, st = C.c_double(), C.c_int32()
        L.check(self._lib.egx_sgp_likelihood(self._h, L.dptr(th), th.size, float(sigma2), float(noise), C.byref(lk),
                                             C.byref(st)))
        return lk.value, st.value

    def likelihood_grad(self, theta, sigma2, noise):
        """(likelihood, gradient, status): the likelihood of `likelihood` (same bits) and its closed-form gradient
        (h + 2, h = d without KPLS weights: dL/dtheta_0..h-1 -- of the broadcast theta when one value is given --, dL/dsigma2,
        dL/dnoise), zeros whenever status != 0 (egx_sgp_likelihood_grad)."""
        th = L.as_f64(np.atleast_1d(theta), 1)
        lk, st = C.c_double(), C.c_int32()
        grad = np.zeros(self.h + 2)
        L.check(self._lib.egx_sgp_likelihood_grad(self._h, L.dptr(th), th.size, float(sigma2), float(noise), C.byref(lk),
                                                  L.dptr(grad), C.byref(st)))
        return lk.value, grad, st.value

    def finalize(self, theta, sigma2, noise):
        th = L.as_f64(np.atleast_1d(theta), 1)
        L.check(self._lib.egx_sgp_finalize(self._h, L.dptr(th), th.size, float(sigma2), float(noise)))

    def fit(self, params0s, lo, hi, estimate_noise, noise_fixed, max_eval):
        p0 = L.as_f64(params0s, 2)
        lo, hi = L.as_f64(lo, 1), L.as_f64(hi, 1)
        ne = C.c_int64()
        L.check(self._lib.egx_sgp_fit(self._h, L.dptr(p0), p0.shape[0], L.dptr(lo), L.dptr(hi), int(bool(estimate_noise)),
                                      float(noise_fixed), int(max_eval), C.byref(ne)))
        return ne.value

    def fit_lbfgs(self, params0s, lo, hi, estimate_noise, noise_fixed, max_iter=50):
        """As `fit` (same starts, box and parameter layout) by a projected L-BFGS on log10(params) driven by
        `likelihood_grad` (egx_sgp_fit_lbfgs); returns the number of likelihood + gradient evaluations."""
        p0 = L.as_f64(params0s, 2)
        lo, hi = L.as_f64(lo, 1), L.as_f64(hi, 1)
        ne = C.c_int64()
        L.check(self._lib.egx_sgp_fit_lbfgs(self._h, L.dptr(p0), p0.shape[0], L.dptr(lo), L.dptr(hi),
                                            int(bool(estimate_noise)), float(noise_fixed), int(max_iter), C.byref(ne)))
        return ne.value

    def likelihood_grad_z(self, theta, sigma2, noise):
        """(likelihood, gradient, grad_z, status): `likelihood_grad` (same bits) and dL/dz, (nz, d) like `z`, the gradient in
        the inducing points; zeros whenever status != 0 (egx_sgp_likelihood_grad_z)."""
        th = L.as_f64(np.atleast_1d(theta), 1)
        lk, st = C.c_double(), C.c_int32()
        grad, grad_z = np.zeros(self.h + 2), np.zeros((self.nz, self.d))
        L.check(self._lib.egx_sgp_likelihood_grad_z(self._h, L.dptr(th), th.size, float(sigma2), float(noise), C.byref(lk),
                                                    L.dptr(grad), L.dptr(grad_z), C.byref(st)))
        return lk.value, grad, grad_z, st.value

    def inducings(self):
        """The current inducing points (nz, d), read from the library (egx_sgp_get_inducings)."""
        z = np.empty((self.nz, self.d))
        L.check(self._lib.egx_sgp_get_inducings(self._h, L.dptr(z)))
        return z

    def set_inducings(self, z):
        """Replace the inducing points (same nz; finite values).  Un-fits the handle (egx_sgp_set_inducings)."""
        z = np.ascontiguousarray(L.as_f64(z))
        if z.shape != (self.nz, self.d):
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"z must be ({self.nz}, {self.d}), got {z.shape}")
        L.check(self._lib.egx_sgp_set_inducings(self._h, L.dptr(z)))
        self.z = self.inducings()

    def fit_lbfgs_z(self, params0s, lo, hi, estimate_noise, noise_fixed, max_iter=50, max_iter_z=50, z_lo=None, z_hi=None):
        """`fit_lbfgs`, then one more L-BFGS from its winner over the parameters AND the inducing points, each boxed in
        [z_lo, z_hi] (d values each; None: the range of the training inputs), driven by `likelihood_grad_z`
        (egx_sgp_fit_lbfgs_z).  Never ends below `fit_lbfgs`; max_iter_z=0 is `fit_lbfgs`.  `z` / `inducings()` hold the
        moved points afterwards.  Returns the number of evaluations of both phases."""
        p0 = L.as_f64(params0s, 2)
        lo, hi = L.as_f64(lo, 1), L.as_f64(hi, 1)
        if (z_lo is None) != (z_hi is None):
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, "z_lo and z_hi must be given together")
        zl = zh = None
        if z_lo is not None:
            zl = np.ascontiguousarray(np.broadcast_to(L.as_f64(np.atleast_1d(z_lo), 1), (self.d,)))
            zh = np.ascontiguousarray(np.broadcast_to(L.as_f64(np.atleast_1d(z_hi), 1), (self.d,)))
        ne = C.c_int64()
        try:
            L.check(self._lib.egx_sgp_fit_lbfgs_z(self._h, L.dptr(p0), p0.shape[0], L.dptr(lo), L.dptr(hi),
                                                  int(bool(estimate_noise)), float(noise_fixed), int(max_iter),
                                                  L.dptr(zl) if zl is not None else None, L.dptr(zh) if zh is not None else None,
                                                  int(max_iter_z), C.byref(ne)))
        finally:
            self.z = self.inducings()
        return ne.value

    def _q(self, x):
        x = L.as_f64(x)
        if x.ndim == 1:
            x = x.reshape(-1, self.d)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"query points must be (m, {self.d}), got {x.shape}")
        return np.ascontiguousarray(x)

    def predict(self, x):
        x = self._q(x)
        out = np.empty(x.shape[0])
        L.check(self._lib.egx_sgp_predict(self._h, L.dptr(x), x.shape[0], L.dptr(out)))
        return out

    def predict_var(self, x):
        x = self._q(x)
        out = np.empty(x.shape[0])
        L.check(self._lib.egx_sgp_predict_var(self._h, L.dptr(x), x.shape[0], L.dptr(out)))
        return out

    def predict_valvar(self, x):
        """(mean, variance) from one call (one upload, one synchronisation): the bits of `predict` and `predict_var`."""
        x = self._q(x)
        y, v = np.empty(x.shape[0]), np.empty(x.shape[0])
        L.check(self._lib.egx_sgp_predict_valvar(self._h, L.dptr(x), x.shape[0], L.dptr(y), L.dptr(v)))
        return y, v

    def predict_gradients(self, x):
        """(m, d) analytic d mean / d x (egx_sgp_predict_gradients)."""
        x = self._q(x)
        out = np.empty(x.shape)
        L.check(self._lib.egx_sgp_predict_gradients(self._h, L.dptr(x), x.shape[0], L.dptr(out)))
        return out

    def predict_var_gradients(self, x):
        """(m, d) analytic d var / d x, exactly 0 where `predict_var` clamps (egx_sgp_predict_var_gradients)."""
        x = self._q(x)
        out = np.empty(x.shape)
        L.check(self._lib.egx_sgp_predict_var_gradients(self._h, L.dptr(x), x.shape[0], L.dptr(out)))
        return out

    def predict_valvar_gradients(self, x):
        """Both analytic gradients from one K(x, z) block and one pair of forward solves."""
        x = self._q(x)
        gy, gv = np.empty(x.shape), np.empty(x.shape)
        L.check(self._lib.egx_sgp_predict_valvar_gradients(self._h, L.dptr(x), x.shape[0], L.dptr(gy), L.dptr(gv)))
        return gy, gv

    def sample(self, x, n_traj, method="psd", seed=None, z=None, return_tau=False):
        """(m, n_traj) trajectories predict(x) 1^T + F Z (egx_sgp_sample), F F^T = sigma2 r(x, x) (+ tau I): the PRIOR
        covariance, as the reference samples its sparse GP.  Arguments and return convention of `GpHandle.sample`."""
        x = self._q(x)
        m, n_traj = x.shape[0], int(n_traj)
        meth = {"cholesky": L.SAMPLE_CHOLESKY, "psd": L.SAMPLE_PSD}.get(method, method)
        if not isinstance(meth, int):
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"unknown sampling method {method!r}")
        if seed is None:
            seed = int(np.random.default_rng().integers(0, 2 ** 63))
        zp = None
        if z is not None:
            z = L.as_f64(z, 2)
            if z.shape != (m, n_traj):
                raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"z must be ({m}, {n_traj}), got {z.shape}")
            zp = L.dptr(z)
        out = np.empty((m, n_traj))
        tau = C.c_double()
        L.check(self._lib.egx_sgp_sample(self._h, L.dptr(x), m, n_traj, int(meth), int(seed) & (2 ** 64 - 1), zp, L.dptr(out),
                                         C.byref(tau)))
        return (out, tau.value) if return_tau else out

    def state(self, with_inv=False):
        th, vec = np.empty(self.h), np.empty(self.nz)
        s2, nv, lk = C.c_double(), C.c_double(), C.c_double()
        inv = np.empty((self.nz, self.nz)) if with_inv else None
        L.check(self._lib.egx_sgp_get_state(self._h, L.dptr(th), C.byref(s2), C.byref(nv), C.byref(lk), L.dptr(vec),
                                            L.dptr(inv) if with_inv else None))
        out = dict(theta=th, sigma2=s2.value, noise=nv.value, likelihood=lk.value, w_vec=vec)
        if with_inv:
            out["w_inv"] = inv
        return out


class SgpParams:
    """Builder, crates/gp/src/sparse_parameters.rs:150-300."""

    def __init__(self, corr, inducings):
        self._corr = corr
        self._inducings = inducings
        self._method = FITC
        self._noise = ParamTuning.Optimized()
        self._theta_tuning = G.ThetaTuning.Full([G.ThetaTuning.DEFAULT_INIT], [DEFAULT_THETA_BOUNDS])
        self._n_start, self._max_eval = G.GP_OPTIM_N_START, G.GP_COBYLA_MAX_EVAL
        self._nugget, self._seed, self._device = G.DEFAULT_NUGGET, None, -1
        self._optimizer = "cobyla"  # the reference's optimiser; "lbfgs" uses the closed-form likelihood gradient
        self._opt_z = None          # optimize_inducings: (max_iter, (z_lo, z_hi) or None)
        self._kpls_dim = None
        self._pls = "host"

    def kpls_dim(self, k):
        """SgpParams::kpls_dim (sparse_parameters.rs:216-220, checked as :304-322): fit on k PLS components of the inputs.  The
        rotations w_star (d, k) are those of a PLS regression of the raw y on the raw x (`kpls.pls_rotations`, on the host, as
        sparse_algorithm.rs:429-455 takes them from linfa-pls; `pls("device")`: computed by the handle on the GPU); theta, its
        initial guess and its bounds then have k components, with every optimiser.  None switches it off."""
        if k is not None:
            k = int(k)
            if k == 0:
                raise L.InvalidValueError(L.ERR_INVALID_VALUE, "`kpls_dim` canot be 0!")
            th = np.asarray(self._theta_tuning.init, dtype=np.float64).reshape(-1)
            if th.size > 1 and k > th.size:
                raise L.InvalidValueError(
                    L.ERR_INVALID_VALUE,
                    f"Dimension reduction ({k}) should be smaller than expected training input size "
                    f"infered from given initial theta length ({th.size})")
        self._kpls_dim = k
        return self

    def pls(self, where):
        """Where `kpls_dim` computes its rotations: "host" (default: `kpls.pls_rotations`, the oracle) or "device" (the handle is
        created without weights and computes them from its resident training set, `SgpHandle.compute_w_star`)."""
        if where not in ("host", "device"):
            raise ValueError("pls must be 'host' or 'device'")
        self._pls = where
        return self

    def sparse_method(self, m):
        self._method = {"fitc": FITC, "vfe": VFE}[m.lower()] if isinstance(m, str) else int(m)
        return self

    def noise_variance(self, tuning):
        self._noise = tuning
        return self

    def theta_init(self, init):
        t = self._theta_tuning
        self._theta_tuning = G.ThetaTuning(t.kind, init, t.bounds)
        return self

    def theta_bounds(self, bounds):
        t = self._theta_tuning
        self._theta_tuning = G.ThetaTuning(t.kind, t.init, [tuple(b) for b in bounds])
        return self

    def theta_tuning(self, t):
        self._theta_tuning = t
        return self

    def n_start(self, n):
        self._n_start = int(n)
        return self

    def max_eval(self, n):
        self._max_eval = int(n)
        return self

    def nugget(self, v):
        self._nugget = float(v)
        return self

    def optimizer(self, name):
        """"cobyla" (default, as the reference tunes the sparse model), or the extension "lbfgs" (projected L-BFGS on
        log10(params) driven by the closed-form likelihood gradient), as `GpParams.optimizer`."""
        if name not in ("cobyla", "lbfgs"):
            raise ValueError("optimizer must be 'cobyla' or 'lbfgs'")
        self._optimizer = name
        return self

    def optimize_inducings(self, max_iter=50, bounds=None):
        """Extension (the reference's inducing points never move): after the "lbfgs" fit, one more L-BFGS from its winner in
        which the inducing points move with the parameters (`SgpHandle.fit_lbfgs_z`), `max_iter` iterations at the most.
        bounds: (z_lo, z_hi), d values each (or one for all), the box of every point; None: the range of the training
        inputs.  Needs optimizer("lbfgs"); max_iter=0 switches it off again."""
        self._opt_z = (int(max_iter), None if bounds is None else (bounds[0], bounds[1]))
        return self

    def seed(self, s):
        self._seed = s
        return self

    def device(self, dev):
        self._device = int(dev)
        return self

    def fit(self, x, y):
        """SgpValidParams::fit, sparse_algorithm.rs:422-650."""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        opt_z = self._opt_z is not None and self._opt_z[0] != 0
        if opt_z and self._optimizer != "lbfgs":
            raise L.InvalidValueError(L.ERR_INVALID_VALUE,
                                      'optimize_inducings moves the inducing points by the likelihood gradient: it needs '
                                      'optimizer("lbfgs")')
        if self._inducings.kind == "Located":
            z = self._inducings.value
        else:  # make_inducings :833-848 (numpy shuffle instead of Xoshiro256Plus)
            rng = np.random.default_rng(self._seed)
            z = x[rng.permutation(x.shape[0])[:min(self._inducings.value, x.shape[0])]].copy()
        w_star = None
        if self._kpls_dim is not None:
            if self._kpls_dim > x.shape[1]:  # sparse_algorithm.rs:430-438
                raise L.InvalidValueError(
                    L.ERR_INVALID_VALUE,
                    f"Dimension reduction {self._kpls_dim} should be smaller than actual training input dimensions {x.shape[1]}")
            if self._pls == "host":
                from .kpls import pls_rotations
                w_star = pls_rotations(x, y, self._kpls_dim)  # on the raw data, as the reference does (:440-455)
        h = SgpHandle(x, y, z, corr=self._corr.code, method=self._method, nugget=self._nugget, device=self._device,
                      w_star=w_star)
        if self._kpls_dim is not None and w_star is None:  # pls("device"): from the training set the handle just uploaded
            try:
                w_star = h.compute_w_star(self._kpls_dim)
            except Exception:
                h.close()
                raise
        d = h.h  # theta components: kpls_dim with KPLS, else the number of inputs
        t = self._theta_tuning
        init = np.asarray(t.init, dtype=np.float64).reshape(-1)
        if init.size not in (1, d):
            h.close()
            raise L.InvalidValueError(L.ERR_INVALID_VALUE,
                                      "Initial guess for theta should be either 1-dim or dim of xtrain" +
                                      (" (w_star.ncols())" if w_star is not None else "") + f", got {init.size}")
        theta0 = np.full(d, init[0]) if init.size == 1 else init
        sigma2_0 = float(np.std(y, ddof=1) ** 2)                      # :503-505
        est = self._noise.kind == "Optimized"
        if t.kind == "Fixed":                                          # :479: bounds collapse onto the value
            tb = [(v, v) for v in theta0]
        else:
            tb = list(t.bounds) * d if len(t.bounds) == 1 else list(t.bounds)
            if w_star is not None and len(tb) != d:
                h.close()
                raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"theta bounds: one pair or {d} pairs expected, got {len(tb)}")
        params0 = np.concatenate([theta0, [sigma2_0], [self._noise.init] if est else []])
        bounds = tb + [(1e-12, 9.0 * sigma2_0)] + ([tuple(self._noise.bounds)] if est else [])  # :580-592
        for i, (lo, hi) in enumerate(bounds):   # keep every start inside its box
            params0[i] = min(max(params0[i], lo), hi)
        starts_log10, _ = prepare_multistart(self._n_start, params0, bounds, seed=42 if self._seed is None else self._seed)
        lo, hi = [b[0] for b in bounds], [b[1] for b in bounds]
        if self._optimizer == "lbfgs":  # iterations per start from max_eval as GpParams.fit does
            max_iter = max(5, min(100, self._max_eval // 4))
            if opt_z:
                zb = self._opt_z[1] or (None, None)
                try:
                    n_evals = h.fit_lbfgs_z(10.0 ** starts_log10, lo, hi, est, self._noise.init, max_iter,
                                            max_iter_z=self._opt_z[0], z_lo=zb[0], z_hi=zb[1])
                except Exception:
                    h.close()
                    raise
            else:
                n_evals = h.fit_lbfgs(10.0 ** starts_log10, lo, hi, est, self._noise.init, max_iter)
        else:
            n_evals = h.fit(10.0 ** starts_log10, lo, hi, est, self._noise.init, self._max_eval)
        sgp = SparseGaussianProcess(h, self, n_evals)
        sgp._xy = (x, y)
        return sgp


class SparseGaussianProcess:
    """crates/gp/src/sparse_algorithm.rs:145-300 (predict side)."""

    def __init__(self, handle, params, n_evals=0):
        self._h, self.params_, self.n_evals = handle, params, n_evals
        self._xy = None

    @staticmethod
    def params(inducings, corr=None):
        return SgpParams(corr if corr is not None else G.SquaredExponentialCorr(), inducings)

    def predict(self, x):
        return self._h.predict(x)

    def predict_var(self, x):
        return self._h.predict_var(x)

    def _central_diff(self, fn, x):
        """sparse_algorithm.rs:298-336: the reference differentiates the sparse predictions NUMERICALLY
        (finitediff's central_diff, step sqrt(f64::EPSILON)); here all 2 nx shifted batches go to the GPU at once."""
        x = self._h._q(x)
        m, nx = x.shape
        h = float(np.sqrt(np.finfo(float).eps))
        shifted = np.repeat(x[None, :, :], 2 * nx, axis=0)
        for k in range(nx):
            shifted[2 * k, :, k] += h
            shifted[2 * k + 1, :, k] -= h
        v = fn(shifted.reshape(-1, nx)).reshape(2 * nx, m)
        return ((v[0::2] - v[1::2]) / (2.0 * h)).T.copy()

    def predict_valvar(self, x):
        return self._h.predict_valvar(x)

    def predict_gradients(self, x, analytic=False):
        """Default: the reference's central differences.  analytic=True: the closed form they approximate, evaluated on
        the GPU (egx_sgp_predict_gradients) -- what a Rust shim behind `SgpSurrogate::predict_gradients` should bind."""
        if analytic:
            return self._h.predict_gradients(x)
        return self._central_diff(self._h.predict, x)

    def predict_var_gradients(self, x, analytic=False):
        """As `predict_gradients`; the analytic form (egx_sgp_predict_var_gradients) is exactly 0 where the variance is
        clamped at 1e-15, which is what the central difference of the clamped function gives there."""
        if analytic:
            return self._h.predict_var_gradients(x)
        return self._central_diff(self._h.predict_var, x)

    def predict_valvar_gradients(self, x):
        """(d mean / d x, d var / d x), analytic only (egx_sgp_predict_valvar_gradients): what a shim should bind for
        `predict_valvar_gradients`."""
        return self._h.predict_valvar_gradients(x)

    def sample_chol(self, x, n_traj, seed=None):
        """sparse_algorithm.rs:338-362 with the plain Cholesky factor: (m, n_traj) trajectories predict(x) + F Z with
        F F^T = sigma2 r(x, x), the PRIOR covariance (no noise, no Woodbury term: the reference's definition, kept as it
        is); LinalgError when it is not positive definite."""
        return self._h.sample(x, n_traj, "cholesky", seed)

    def sample_eig(self, x, n_traj, seed=None):
        """As `GaussianProcess.sample_eig` (same deviation: Cholesky of the covariance + tau I, no eigendecomposition),
        on the prior covariance of `sample_chol`."""
        return self._h.sample(x, n_traj, "psd", seed)

    def sample(self, x, n_traj, seed=None):
        """Alias of `sample_eig`, as in the reference."""
        return self.sample_eig(x, n_traj, seed)

    def theta(self):
        return self._h.state()["theta"]

    def variance(self):
        return self._h.state()["sigma2"]

    def noise_variance(self):
        return self._h.state()["noise"]

    def likelihood(self):
        return self._h.state()["likelihood"]

    def inducings(self):
        return self._h.z

    def dims(self):
        """(the number of theta components -- kpls_dim under KPLS, else the inputs --, 1), sparse_algorithm.rs:283-285"""
        return self._h.h, 1

    def w_star(self):
        """The KPLS weights (d, h) the model was fitted with; the identity without KPLS, as the reference stores it."""
        w = self._h.w_star()
        return np.eye(self._h.d) if w is None else w

    def woodbury(self):
        s = self._h.state(with_inv=True)
        return s["w_vec"], s["w_inv"]

    def close(self):
        self._h.close()

    def __str__(self):  # "SGP(corr=..., theta=..., variance=..., noise variance=..., likelihood=...)" :200-208
        s = self._h.state()
        return (f"SGP(corr={self.params_._corr}, theta={s['theta'].tolist()}, variance={s['sigma2']}, "
                f"noise variance={s['noise']}, likelihood={s['likelihood']})")


class SparseMethod:
    FITC = FITC
    VFE = VFE


class SparseGpMix:
    """python/src/sparse_gp_mix.rs: SparseGpx.builder(...) -> SparseGpMix, .fit(xt, yt) -> SparseGpx.

    n_clusters = 1 is one sparse expert.  n_clusters = k >= 2 trains as GpMixtureValidParams::train does for GpType::SparseGp
    (crates/moe/src/algorithm.rs:72-205, 306-339): the Gaussian mixture of [x, y] (`GaussianMixture.fit`, on the GPU), one
    sparse expert per cluster -- Located(z): every expert the same z; Randomized(nz): nz rows of the expert's own cluster, drawn
    with the seed --, and `recombination` "hard" or "smooth"; smooth with heaviside_factor=None (the reference's Smooth(None))
    chooses the factor on one row out of five (`optimize_heaviside_factor`) and retrains on all rows.  n_clusters = 0 (automatic)
    and kpls_dim are not implemented HERE: a single sparse model takes KPLS through `SgpParams.kpls_dim` (the Rust-shaped
    builder), and this builder keeps refusing kpls_dim with NotImplementedError("KPLS ...") -- lifting that is a follow-up, which
    has to edit the test that pins the refusal (tests/test_infill_sparse_cpu.py).  optimize_inducings (an extension, with optimizer="lbfgs"): every expert moves its
    inducing points by the likelihood gradient after its fit (`SgpParams.optimize_inducings`)."""

    def __init__(self, corr_spec=1, theta_init=None, theta_bounds=None, kpls_dim=None, n_start=G.GP_OPTIM_N_START, nz=None,
                 z=None, method=FITC, seed=None, max_eval=G.GP_COBYLA_MAX_EVAL, device=-1, optimizer="cobyla", n_clusters=1,
                 recombination="smooth", heaviside_factor=None, n_runs=20, optimize_inducings=False):
        if kpls_dim is not None:
            raise NotImplementedError("KPLS rotations come from linfa-pls (outside the accelerated path)")
        if int(n_clusters) == 0:
            raise NotImplementedError("n_clusters = 0 (the automatic choice of the number of clusters) is not implemented")
        if int(n_clusters) < 0:
            raise ValueError("n_clusters must be positive")
        if nz is None and z is None:
            raise ValueError("either nz or z has to be specified")  # sparse_gp_mix.rs builder check
        recombination = getattr(recombination, "name", recombination)  # gpx.Recombination.HARD / SMOOTH, or a string
        if str(recombination).lower() not in ("hard", "smooth"):
            raise ValueError("recombination must be 'hard' or 'smooth'")
        self.corr_spec, self.theta_init, self.theta_bounds = int(corr_spec), theta_init, theta_bounds
        self.n_start, self.nz, self.z, self.method, self.seed = n_start, nz, z, method, seed
        self.max_eval, self.device, self.optimizer = max_eval, device, optimizer
        self.n_clusters, self.recombination, self.heaviside_factor = int(n_clusters), str(recombination).lower(), heaviside_factor
        self.n_runs = int(n_runs)
        # False, True (50 iterations) or the number of iterations of `SgpParams.optimize_inducings`, per expert
        self.optimize_inducings = optimize_inducings

    def _expert_params(self):
        corrs = {1: G.SquaredExponentialCorr, 2: G.AbsoluteExponentialCorr, 4: G.Matern32Corr, 8: G.Matern52Corr}
        if self.corr_spec not in corrs:
            raise NotImplementedError("pass exactly one correlation spec (expert selection belongs to egobox-moe)")
        ind = Inducings.Located(self.z) if self.z is not None else Inducings.Randomized(self.nz)
        p = SgpParams(corrs[self.corr_spec](), ind).sparse_method(self.method).n_start(self.n_start) \
            .max_eval(self.max_eval).seed(self.seed).device(self.device).optimizer(self.optimizer)
        if self.theta_init is not None:
            p.theta_init(self.theta_init)
        if self.theta_bounds is not None:
            p.theta_bounds(self.theta_bounds)
        if self.optimize_inducings:
            p.optimize_inducings(50 if self.optimize_inducings is True else int(self.optimize_inducings))
        return p

    def fit(self, xt, yt):
        yt = np.asarray(yt, dtype=np.float64)
        if yt.ndim == 2 and yt.shape[1] != 1:
            raise ValueError("sparse GP mixture handles a single output")  # test_sgp_multi_outputs_exception
        p = self._expert_params()
        if self.n_clusters == 1:
            return SparseGpx(p.fit(xt, yt.reshape(-1)))
        x = np.asarray(xt, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        return SparseGpx(None, self._fit_clusters(x, yt.reshape(-1), self.heaviside_factor))

    def _fit_clusters(self, x, y, factor):
        """train / train_on_clusters (algorithm.rs:72-205) with sparse experts (:306-339)."""
        from . import moe as M
        k, nx = self.n_clusters, x.shape[1]
        if k > x.shape[0]:
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"n_clusters ({k}) exceeds the number of training points ({x.shape[0]})")
        data = np.column_stack([x, y])
        smooth_none = self.recombination == "smooth" and factor is None
        training = M.extract_part(data, 5)[1] if smooth_none else data
        gmm = M.train_mixture(training, k, n_runs=self.n_runs, seed=42 if self.seed is None else self.seed,
                              device=self.device)
        gmx = gmm.marginal(nx, 1.0 if factor is None else float(factor))
        clusters = M.sort_by_cluster(k, data, gmx.predict(x))
        M.check_three_points(clusters)
        experts = [self._expert_params().fit(c[:, :nx], c[:, nx]) for c in clusters]
        moe = M.GpMixture(experts, gmx, self.recombination)
        if smooth_none:
            test = M.extract_part(data, 5)[0]
            best = M.optimize_heaviside_factor(moe.experts, gmx, test[:, :nx], test[:, nx], "smooth")
            final = self._fit_clusters(x, y, best)  # the mixture on ALL rows, algorithm.rs:188-193
            for e in experts:
                e.close()
            return final
        moe.training_data = (x, y)
        return moe


class SparseGpx:
    """One sparse expert (`_sgp`), or a trained mixture of sparse experts (`_moe`, an `egobox_amd.moe.GpMixture` whose
    recombination runs inside the library: egx_moe_predict_valvar_sgp / _gradients_sgp)."""

    def __init__(self, sgp, moe=None):
        self._sgp, self._moe = sgp, moe

    @staticmethod
    def builder(**kw):
        return SparseGpMix(**kw)

    @property
    def experts(self):
        return [self._sgp] if self._moe is None else list(self._moe.experts)

    def _need_single(self, what):
        if self._moe is not None:
            raise L.SampleError(L.ERR_INVALID_VALUE, f"Can not {what} when several clusters {len(self._moe.experts)}")

    def predict(self, x):
        return self._sgp.predict(x) if self._moe is None else self._moe.predict(x)

    def predict_var(self, x):
        return self._sgp.predict_var(x) if self._moe is None else self._moe.predict_var(x)

    def predict_valvar(self, x):
        return self._sgp.predict_valvar(x) if self._moe is None else self._moe.predict_valvar(x)

    def predict_gradients(self, x, analytic=False):
        """(A mixture of several experts recombines the experts' ANALYTIC gradients whatever `analytic` says.)"""
        return self._sgp.predict_gradients(x, analytic=analytic) if self._moe is None else self._moe.predict_gradients(x)

    def predict_var_gradients(self, x, analytic=False):
        return self._sgp.predict_var_gradients(x, analytic=analytic) if self._moe is None else self._moe.predict_var_gradients(x)

    def predict_valvar_gradients(self, x):
        return self._sgp.predict_valvar_gradients(x) if self._moe is None else self._moe.predict_valvar_gradients(x)

    def sample(self, x, n_traj, seed=None):
        self._need_single("sample")
        return self._sgp.sample(x, n_traj, seed)

    def sample_chol(self, x, n_traj, seed=None):
        self._need_single("sample")
        return self._sgp.sample_chol(x, n_traj, seed)

    def sample_eig(self, x, n_traj, seed=None):
        self._need_single("sample")
        return self._sgp.sample_eig(x, n_traj, seed)

    def thetas(self):
        """(n_clusters, d)"""
        return np.stack([e.theta() for e in self.experts])

    def variances(self):
        """(n_clusters,)"""
        return np.array([e.variance() for e in self.experts])

    def likelihoods(self):
        """(n_clusters,)"""
        return np.array([e.likelihood() for e in self.experts])

    def __str__(self):
        if self._moe is None:
            return f"Mixture[Smooth(1)]({self._sgp.params_._corr}{self._sgp})"
        mode = "Hard" if self._moe.recombination == "hard" else f"Smooth({self._moe.gmx.heaviside_factor})"
        return f"Mixture[{mode}](" + ", ".join(f"{e.params_._corr}{e}" for e in self.experts) + ")"

    # ---- JSON dump in the field layout of the reference's serde structs (SparseGaussianProcess :145-168, WoodburyData
    #      :32-36; typetag "type_sgp" crates/moe/src/surrogates.rs:101): theta, sigma2, noise, likelihood, w_star,
    #      inducings, w_data{vec, inv}, training_data, corr, method
    def to_dict(self):
        if self._moe is not None:
            raise NotImplementedError("only a single-expert sparse model is serialised")
        g = self._sgp
        h = g._h
        st = h.state(with_inv=True)

        def nd(a):
            a = np.asarray(a, dtype=np.float64)
            return {"v": 1, "dim": list(a.shape), "data": a.ravel().tolist()}

        corr = str(g.params_._corr)
        expert = {"type_sgp": f"Sgp{corr}Surrogate", "corr": corr, "method": "Fitc" if g.params_._method == FITC else "Vfe",
                  "theta": nd(st["theta"]), "sigma2": st["sigma2"], "noise": st["noise"], "likelihood": st["likelihood"],
                  "w_star": nd(g.w_star()), "inducings": nd(h.z),
                  "w_data": {"vec": nd(st["w_vec"].reshape(-1, 1)), "inv": nd(st["w_inv"])},
                  "training_data": [nd(g._xy[0]), nd(g._xy[1])], "nugget": g.params_._nugget}
        return {"recombination": {"Smooth": 1.0}, "experts": [expert], "gp_type": "SparseGp"}

    def save(self, filename):
        import json
        if not str(filename).endswith(".json"):
            raise NotImplementedError("only the JSON format is written (the reference's .bin is bincode)")
        with open(filename, "w") as f:
            json.dump(self.to_dict(), f)
        return True

    @staticmethod
    def load(filename):
        """Rebuild on the GPU from a JSON dump: the stored (theta, sigma2, noise, inducings) are re-evaluated (one
        likelihood evaluation, milliseconds) and the stored likelihood is checked against the recomputed one."""
        import json
        with open(filename) as f:
            e = json.load(f)["experts"][0]

        def arr(o):
            return np.asarray(o["data"], dtype=np.float64).reshape(o["dim"])

        corr = G.CORRS[e["corr"]]()
        x, y = arr(e["training_data"][0]), arr(e["training_data"][1])
        z, theta = arr(e["inducings"]), arr(e["theta"])
        method = FITC if e["method"] == "Fitc" else VFE
        params = SgpParams(corr, Inducings.Located(z)).sparse_method(method).nugget(e.get("nugget", G.DEFAULT_NUGGET))
        h = SgpHandle(x, y, z, corr=corr.code, method=method, nugget=params._nugget)
        w = arr(e["w_star"]) if "w_star" in e else None
        if w is not None and not (w.shape[0] == w.shape[1] and np.array_equal(w, np.eye(w.shape[0]))):
            try:  # real KPLS weights: restored before the state goes in (a file with eye(d) loads exactly as it always did)
                h.set_w_star(w)
                params.kpls_dim(w.shape[1])
            except Exception:
                h.close()
                raise
        h.finalize(theta, e["sigma2"], e["noise"])
        lk = h.state()["likelihood"]
        if not np.isclose(lk, e["likelihood"], rtol=1e-6, atol=1e-9):
            h.close()
            raise L.EgxError(L.ERR_LIKELIHOOD, f"stored likelihood {e['likelihood']} != recomputed {lk}")
        sgp = SparseGaussianProcess(h, params, n_evals=1)
        sgp._xy = (x, y)
        return SparseGpx(sgp)
