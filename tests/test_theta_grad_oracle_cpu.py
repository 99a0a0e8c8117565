"""The closed-form theta-gradient of tests/theta_grad_oracle.py, on the CPU alone: it is oracle.gp_oracle.likelihood_grad at
w = I, it is the derivative of oracle.gp_oracle.fit_fixed(...).likelihood for weights with zeros, every trend and a theta
component at zero, its D_l is the derivative of log corr_value -- and every row of tests/theta_grad_cases.py is well posed, so
that the 1e-6 bar of tests/test_gpu_theta_grad.py means something on each of them."""
import numpy as np
import pytest

import theta_grad_cases as TC
import theta_grad_oracle as TO
from oracle import gp_oracle as GO


def _set(n, d, seed):
    x = GO.lhs_classic(n, d, seed)
    return x, GO.griewank(x)


@pytest.mark.parametrize("corr", range(4))
def test_equals_the_identity_weight_oracle(corr):
    """w = I, explicitly and by default: the older closed form to rounding (1e-12 of the largest component)"""
    x, y = _set(150, 3, 6)
    theta = np.array([0.8, 1.3, 0.5]) * (4.0 if corr == 0 else 1.0)
    lk_ref, g_ref = GO.likelihood_grad(x, y, theta, corr=TC.KINDS[corr])
    for w in (None, np.eye(3)):
        lk, g, piv = TO.likelihood_grad(x, y, theta, corr=TC.KINDS[corr], w_star=w)
        assert lk == lk_ref and piv > 0.0
        np.testing.assert_allclose(g, g_ref, rtol=1e-12, atol=1e-12 * np.abs(g_ref).max())


def _richardson(f, theta, l, step):
    """d f / d theta_l by central differences at step and step / 2, extrapolated (error O(step^4))"""
    def cd(s):
        e = np.zeros_like(theta)
        e[l] = s
        return (f(theta + e) - f(theta - e)) / (2.0 * s)
    return (4.0 * cd(step / 2.0) - cd(step)) / 3.0


# weights 6 x 3 with a zero row and a zero entry; theta[1] = 0 exactly in the last rows, where only the OTHER components are
# differenced (a negative theta is outside every kernel's domain, so the zero component has no central difference)
@pytest.mark.parametrize("corr", range(4))
@pytest.mark.parametrize("mean,zero", [(0, False), (1, False), (2, False), (0, True), (1, True)])
def test_is_the_derivative_of_the_likelihood(corr, mean, zero):
    n, d, h = 60, 6, 3
    x, y = _set(n, d, 21)
    w = np.random.default_rng(5).standard_normal((d, h))
    w[1, :] = 0.0
    w[0, h - 1] = 0.0
    w /= np.linalg.norm(w, axis=0)
    theta = np.array([0.9, 1.4, 0.6]) * (2.0 if corr == 0 else 1.0)
    if zero:
        theta[1] = 0.0
    kw = dict(mean=TC.MEANS[mean], corr=TC.KINDS[corr], w_star=w)
    lk, g, piv = TO.likelihood_grad(x, y, theta, **kw)
    assert piv >= 1e-2  # (so that differences of the likelihood carry nine digits)
    assert lk == GO.fit_fixed(x, y, theta, **kw).likelihood

    def f(th):
        return GO.fit_fixed(x, y, th, **kw).likelihood
    for l in range(h):
        if zero and l == 1:
            continue
        fd = _richardson(f, theta, l, 1e-3 * theta[l])
        print(f"{TC.KINDS[corr]} {TC.MEANS[mean]} zero {zero} l {l}: closed {g[l]:.12e} differences {fd:.12e}")
        assert abs(g[l] - fd) <= 1e-7 * np.abs(g).max()
    if zero and corr != 1:
        assert g[1] == 0.0  # sq-exp and the Materns are flat in a component at zero; abs-exp is not
    if zero and corr == 1:
        assert g[1] != 0.0


@pytest.mark.parametrize("corr", range(4))
def test_d_l_is_the_derivative_of_log_corr_value(corr):
    rng = np.random.default_rng(3)
    d, h = 5, 3
    w = rng.standard_normal((d, h))
    w[2, :] = 0.0
    w[0, 1] = 0.0
    theta = np.array([0.7, 1.1, 0.4])
    a = rng.random((7, d))  # a handful of pairs
    for l in range(h):
        def f(th):
            return np.log(GO.corr_value(TC.KINDS[corr], a, th, w)[:, 0])
        fd = _richardson(f, theta, l, 1e-3)
        got = TO.dlog_dtheta(TC.KINDS[corr], a, theta, w, l)
        np.testing.assert_allclose(got, fd, rtol=1e-9, atol=1e-9 * np.abs(fd).max())


def test_table_covers_the_branches():
    """the shapes the table is there for, by name (so that an edit of the table cannot drop one silently)"""
    ks = ("sqexp", "absexp", "matern32", "matern52")
    want = [f"A-n{n}-{k}" for n in (5, 63, 64, 65, 128, 129) for k in ks]
    want += [f"B-d{d}-{k}" for d in (1, 8, 9, 16, 17, 32, 33, 64, 65, 97, 129) for k in ks]
    want += [f"C-d{d}-{k}" for d in (6, 40, 70) for k in ks]
    want += [f"D-d{d}-h{h}-{k}" for d, h in ((6, 3), (12, 9), (20, 17), (40, 33), (70, 3), (70, 33)) for k in ks]
    want += [f"D-d{d}-h{h}-wzero-{k}" for d, h in ((6, 3), (40, 33), (70, 3)) for k in ks]
    want += [f"E-{m}-{k}" for m in ("linear", "quadratic") for k in ks]
    assert sorted(want) == sorted(TC.BY_NAME)
    for c in TC.CASES:
        assert c.n == (int(c.name.split("-")[1][1:]) if c.name.startswith("A-") else TC.N_DEFAULT)
        th, w = TC.case_theta(c), TC.case_weights(c)
        assert th.shape == (c.d if c.h is None else c.h,) and np.all(th >= 0.0)
        assert np.flatnonzero(th == 0.0).tolist() == ([1] if c.zero_component else [])
        if w is not None:
            assert w.shape == (c.d, c.h)
            np.testing.assert_allclose(np.linalg.norm(w, axis=0), 1.0, rtol=1e-14)
            zeros = np.argwhere(w == 0.0).tolist()
            assert zeros == ([[0, c.h - 1]] + [[1, l] for l in range(c.h)] if c.w_zero_row else [])


def _assert_well_posed(label, ref):
    lk, g, piv = ref
    print(f"{label}: likelihood {lk:.6e} min pivot {piv:.3e} max |g| {np.abs(g).max():.3e}")
    assert np.isfinite(lk) and np.all(np.isfinite(g))
    assert TC.PIVOT_WINDOW[0] <= piv <= TC.PIVOT_WINDOW[1]
    assert np.abs(g).max() >= TC.MIN_GRAD


@pytest.mark.parametrize("case", TC.CASES, ids=[c.name for c in TC.CASES])
def test_row_is_well_posed(case):
    _assert_well_posed(case.name, TC.reference(case))


@pytest.mark.parametrize("members", [TC.mode0_batch, TC.mixed_group, TC.companions])
def test_entry_point_members_are_well_posed(members):
    ms = members()
    assert len({m.label for m in ms}) == len(ms)
    for m in ms:
        _assert_well_posed(m.label, TC.reference(m))
    if members is TC.mixed_group:
        assert [np.flatnonzero(m.theta == 0.0).tolist() for m in ms] == [[], [], [1], []]
