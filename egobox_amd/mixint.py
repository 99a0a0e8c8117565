"""Mixed-integer design spaces (crates/ego/src/types.rs `XType`, crates/ego/src/gpmix/mixint.rs): typed columns, the fold /
unfold / cast between the user's columns and their continuous relaxation, and surrogates that cast every query point to its
nearest admissible discrete point before they answer -- on the GPU, in the kernels that read the query rows anyway
(include/egx_gp.h `egx_mixint_*`, `egx_gp_set_xtypes`).  Every function here goes through the C ABI; the arithmetic and the
places where the reference is not followed are those of egobox_amd/csrc/mixint.h."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .cv import GpMetrics

FLOAT, INT, ORD, ENUM = 0, 1, 2, 3


class XType:
    """One typed column: `XType.Float(lo, hi)`, `XType.Int(lo, hi)`, `XType.Ord(values)`, `XType.Enum(n)`."""

    __slots__ = ("kind", "lo", "hi", "values", "n")

    def __init__(self, kind, lo=0.0, hi=0.0, values=(), n=0):
        self.kind, self.lo, self.hi = int(kind), float(lo), float(hi)
        self.values = tuple(float(v) for v in values)
        self.n = int(n)

    @classmethod
    def Float(cls, lo, hi):
        return cls(FLOAT, lo, hi)

    @classmethod
    def Int(cls, lo, hi):
        return cls(INT, lo, hi)

    @classmethod
    def Ord(cls, values):
        values = tuple(values)
        return cls(ORD, values=values, n=len(values))

    @classmethod
    def Enum(cls, n):
        return cls(ENUM, n=n)

    def __eq__(self, other):
        return isinstance(other, XType) and (self.kind, self.lo, self.hi, self.values, self.n) == (
            other.kind, other.lo, other.hi, other.values, other.n)

    def __hash__(self):
        return hash((self.kind, self.lo, self.hi, self.values, self.n))

    def __repr__(self):
        if self.kind == FLOAT:
            return f"XType.Float({self.lo}, {self.hi})"
        if self.kind == INT:
            return f"XType.Int({self.lo:g}, {self.hi:g})"
        if self.kind == ORD:
            return f"XType.Ord({list(self.values)})"
        if self.kind == ENUM:
            return f"XType.Enum({self.n})"
        return f"XType(kind={self.kind})"


def _c_xtypes(xtypes):
    """(egx_xtype array, nx, keep-alive) of a sequence of XType."""
    xtypes = list(xtypes)
    arr = (L.XTypeC * max(1, len(xtypes)))()
    keep = []
    for c, t in zip(arr, xtypes):
        if not isinstance(t, XType):
            raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"xtypes: expected XType, got {type(t).__name__}")
        c.kind, c.n, c.lo, c.hi = t.kind, t.n, t.lo, t.hi
        if t.kind == ORD:
            v = np.ascontiguousarray(t.values, dtype=np.float64)
            keep.append(v)
            c.values = L.dptr(v) if v.size else None
    return arr, len(xtypes), keep


def unfolded_dim(xtypes):
    """compute_continuous_dim (mixint.rs:99-108): sum of (Enum(v) ? v : 1)."""
    arr, nx, _keep = _c_xtypes(xtypes)
    d = C.c_int64()
    L.check(L.load().egx_mixint_unfolded_dim(arr, nx, C.byref(d)))
    return int(d.value)


def as_continuous_limits(xtypes):
    """(d, 2) limits of the relaxed space (mixint.rs:38-67)."""
    arr, nx, _keep = _c_xtypes(xtypes)
    out = np.empty((unfolded_dim(xtypes), 2))
    L.check(L.load().egx_mixint_continuous_limits(arr, nx, L.dptr(out)))
    return out


def _rows(fn, xtypes, x, cols_in, cols_out):
    arr, nx, _keep = _c_xtypes(xtypes)
    d = unfolded_dim(xtypes)  # (validates the spec)
    dims = {"nx": nx, "d": d}
    x = L.as_f64(x)
    if x.ndim == 1:
        x = x.reshape(1, -1) if dims[cols_in] > 1 or x.shape[0] == 1 else x.reshape(-1, 1)
    if x.ndim != 2 or x.shape[1] != dims[cols_in]:
        raise L.InvalidValueError(L.ERR_INVALID_VALUE, f"{fn}: x must be (m, {dims[cols_in]}), got {x.shape}")
    x = np.ascontiguousarray(x)
    out = np.empty((x.shape[0], dims[cols_out]))
    L.check(getattr(L.load(), fn)(arr, nx, L.dptr(x), x.shape[0], L.dptr(out)))
    return out


def unfold_with_enum_mask(xtypes, x):
    """(m, nx) -> (m, d): an enum index becomes its one-hot group (mixint.rs:116-144); an index outside [0, v) raises."""
    return _rows("egx_mixint_unfold", xtypes, x, "nx", "d")


to_continuous_space = unfold_with_enum_mask  # mixint.rs:148-153


def fold_with_enum_index(xtypes, x):
    """(m, d) -> (m, nx): a group becomes the index of its first maximum (mixint.rs:77-96)."""
    return _rows("egx_mixint_fold", xtypes, x, "d", "nx")


def cast_to_discrete_values(xtypes, x):
    """(m, d) -> (m, d): every coordinate to its nearest admissible value (mixint.rs:167-217)."""
    return _rows("egx_mixint_cast", xtypes, x, "d", "d")


def to_discrete_space(xtypes, x):
    """cast, then fold (mixint.rs:220-226)."""
    return _rows("egx_mixint_to_discrete", xtypes, x, "d", "nx")


def set_handle_xtypes(handle, xtypes):
    """egx_gp_set_xtypes on a GpHandle; None or () clears."""
    xtypes = list(xtypes or ())
    arr, nx, _keep = _c_xtypes(xtypes)
    L.check(handle._lib.egx_gp_set_xtypes(handle._h, arr if nx else None, nx))


def get_handle_xtypes(handle):
    """The XTypes a GpHandle carries (egx_gp_get_xtypes); [] when none."""
    nx, nv = C.c_int32(), C.c_int64()
    L.check(handle._lib.egx_gp_get_xtypes(handle._h, None, 0, C.byref(nx), None, C.byref(nv)))
    if nx.value == 0:
        return []
    arr = (L.XTypeC * nx.value)()
    vals = np.empty(max(1, nv.value))
    L.check(handle._lib.egx_gp_get_xtypes(handle._h, arr, nx.value, None, L.dptr(vals), None))
    out, off = [], 0
    for c in arr:
        if c.kind == ORD:
            out.append(XType.Ord(vals[off:off + c.n]))
            off += c.n
        elif c.kind == ENUM:
            out.append(XType.Enum(c.n))
        else:
            out.append(XType(c.kind, c.lo, c.hi))
    return out


class MixintSampling:
    """An LHS in the continuous limits of a spec, returned in the discrete folded space."""

    def __init__(self, xtypes, seed=None):
        self.xtypes, self.rng = list(xtypes), np.random.default_rng(seed)

    def sample(self, n):
        from .multistart import lhs_classic
        lim = as_continuous_limits(self.xtypes)
        u = lhs_classic(int(n), lim.shape[0], self.rng)
        return to_discrete_space(self.xtypes, lim[:, 0] + u * (lim[:, 1] - lim[:, 0]))


class MixintContext:
    """MixintContext (mixint.rs:781-870): a spec and what is built from it."""

    def __init__(self, xtypes, work_in_folded_space=True):
        self.xtypes = list(xtypes)
        self.work_in_folded_space = bool(work_in_folded_space)
        self._d = unfolded_dim(self.xtypes)

    def get_unfolded_dim(self):
        return self._d

    def create_lhs_sampling(self, seed=None):
        """The project's own numpy LHS (multistart.lhs_classic) in the continuous limits, then `to_discrete_space`.  It is NOT the
        reference's Xoshiro stream: the points differ from `test_mixint_lhs`' (mixint.rs:883-908), their admissibility does not."""
        return MixintSampling(self.xtypes, seed)

    def create_surrogate(self, params, x, y):
        """MixintGpMixtureParams(xtypes, params).work_in_folded_space(..).fit(x, y) (mixint.rs:842-856)."""
        return MixintGpMixtureParams(self.xtypes, params).work_in_folded_space(self.work_in_folded_space).fit(x, y)


class MixintGpMixtureParams:
    """MixintGpMixtureParams (mixint.rs:238-330): a spec around the parameters of a `GpMixture`."""

    def __init__(self, xtypes, gp_mixture_params=None):
        from .moe import GpMixtureParams
        self.xtypes = list(xtypes)
        self.params = gp_mixture_params if gp_mixture_params is not None else GpMixtureParams()
        self._folded = False
        unfolded_dim(self.xtypes)  # validates

    def work_in_folded_space(self, flag):
        self._folded = bool(flag)
        return self

    def fit(self, x, y):
        """Unfolds when working in folded space, casts the training inputs once (on the host), fits the mixture, and sets the
        xtypes on every expert's handle: from then on the queries are cast on the device."""
        x = L.as_f64(x)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        xu = unfold_with_enum_mask(self.xtypes, x) if self._folded else x
        xc = cast_to_discrete_values(self.xtypes, xu)
        moe = self.params.fit(xc, y)
        return MixintGpMixture(moe, self.xtypes, self._folded)


class MixintGpMixture(GpMetrics):
    """MixintGpMixture (mixint.rs:332-697): a `GpMixture` whose experts carry the xtypes.  A query in the unfolded space goes to
    the device as it is and is cast there; in folded space it is unfolded on the host first (the enum indices are validated)."""

    def __init__(self, moe, xtypes, work_in_folded_space=False):
        self.moe, self.xtypes, self.work_in_folded_space = moe, list(xtypes), bool(work_in_folded_space)
        self._d = unfolded_dim(self.xtypes)
        handles = []
        for e in moe.experts:
            h = getattr(e, "handle", e)
            if e is None or not hasattr(h, "_h"):
                raise L.InvalidValueError(L.ERR_INVALID_VALUE, "MixintGpMixture: every expert must be a library-backed model on this rank")
            handles.append(h)
        for h in handles:
            set_handle_xtypes(h, self.xtypes)
        moe.xtypes = self.xtypes  # the mixture's responsibilities are taken at the cast point as well

    @property
    def dims(self):
        """(nx, 1) in folded space, (d, 1) otherwise."""
        return (len(self.xtypes) if self.work_in_folded_space else self._d, 1)

    def _q(self, x):
        x = L.as_f64(x)
        if x.ndim == 1:
            x = x.reshape(-1, 1) if self.dims[0] == 1 else x.reshape(1, -1)
        return unfold_with_enum_mask(self.xtypes, x) if self.work_in_folded_space else np.ascontiguousarray(x)

    def predict(self, x):
        return self.moe.predict(self._q(x))

    def predict_var(self, x):
        return self.moe.predict_var(self._q(x))

    def predict_valvar(self, x):
        return self.moe.predict_valvar(self._q(x))

    def predict_gradients(self, x):
        """d mean / d x at the cast point, with respect to the UNFOLDED coordinates: (m, d) (mixint.rs:656-687)."""
        return self.moe.predict_gradients(self._q(x))

    def predict_var_gradients(self, x):
        return self.moe.predict_var_gradients(self._q(x))

    def predict_valvar_gradients(self, x):
        return self.moe.predict_valvar_gradients(self._q(x))

    def sample(self, x, n_traj):
        return self.moe.sample(self._q(x), n_traj)

    # GpMetrics: the scores of the inner mixture, whose training data are the cast ones
    def _cv_targets(self):
        return self.moe._cv_targets()

    def _cv_folds(self, kfold, want_var):
        return self.moe._cv_folds(kfold, want_var)

    @property
    def training_data(self):
        return self.moe.training_data

    @property
    def experts(self):
        return self.moe.experts
