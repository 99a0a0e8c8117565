"""CPU checks of the pending points (q-point infill without a refit): the closed form of egobox_amd/csrc/pending_math.h against
an actual refit with frozen normalisation (tests/pending_oracle.py, both in numpy on oracle.gp_oracle), pending_math.h itself
compiled with g++ (tests/c_host/pending_math_test.cpp) against numpy on values the oracle supplies, and the C ABI of the feature."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import pending_oracle as PO
from oracle import gp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egobox_amd", "csrc")
KINDS = ["SquaredExponential", "AbsoluteExponential", "Matern32", "Matern52"]
NEW_SYMBOLS = ["egx_infill_push_pending", "egx_infill_clear_pending", "egx_infill_get_pending", "egx_infill_virtual_point",
               "egx_infill_batch_config_default", "egx_infill_optimize_batch"]
# (n, d, q, theta): the shapes of tests/test_gpu_infill_pending.py
CASES = [(600, 4, 3, 1.5), (600, 5, 16, 1.5), (130, 3, 5, 1.5), (130, 2, 2, 4.0)]


def _case(n, d, q, theta, corr, mean, seed=1):
    from egobox_amd import workload
    x, y = workload.make_training_set(n, d, seed=seed)
    g = O.fit_fixed(x, 1e-3 * y, np.full(d, theta), mean=mean, corr=corr)
    rng = np.random.default_rng(100 * n + 10 * d + q)
    lo, hi = x.min(axis=0), x.max(axis=0)
    xv = lo + (hi - lo) * rng.random((q, d))
    xq = lo + (hi - lo) * rng.random((40, d))
    mu, var = g.predict_valvar(xv)
    yv = mu + 3.0 * np.sqrt(var) * rng.standard_normal(q)
    return g, xv, yv, xq


@pytest.mark.parametrize("mean", ["Constant", "Quadratic"])
@pytest.mark.parametrize("corr", KINDS)
@pytest.mark.parametrize("n,d,q,theta", CASES)
def test_closed_form_is_the_frozen_refit(n, d, q, theta, corr, mean):
    g, xv, yv, xq = _case(n, d, q, theta, corr, mean)
    ref = PO.refit_frozen(g, xv, yv)
    rm, rv = ref.predict_valvar(xq)
    cm, cv, cs2, _ = PO.closed_form(g, xv, yv, xq)
    em = float(np.max(np.abs(cm - rm)) / np.max(np.abs(rm)))
    ev = float(np.max(np.abs(cv - rv)) / ref.inner.sigma2)
    es = abs(cs2 - ref.inner.sigma2) / ref.inner.sigma2
    print(f"n {n} d {d} q {q} {corr} {mean}: mean {em:.2e} var {ev:.2e} sigma2 {es:.2e}")
    assert em <= 1e-10 and ev <= 1e-10 and es <= 1e-10


def test_the_case_tables_data_is_the_workloads():
    """tests/pending_cases.py imports without the library, so it takes its data from the oracle: the same numbers"""
    from egobox_amd import workload
    import pending_cases as PC
    for n, d in ((130, 9), (260, 17)):
        x, y = workload.make_training_set(n, d, seed=1)
        got = PC._draw(n, d, 2, 3)
        np.testing.assert_array_equal(got[0], x)
        np.testing.assert_array_equal(got[1], y)


# ---- pending_math.h on the host -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("pending") / "pending_math_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "c_host", "pending_math_test.cpp"), "-o", str(out)], check=True)
    return str(out)


def _line(q, n, sigma2, y_std, s, delta, c, mean, var, x_std, gmean, gvar, dc):
    tok = ["P", q, n] + [repr(float(v)) for v in [sigma2, y_std, *np.ravel(s), *delta, *c, mean, var, x_std, gmean, gvar, *dc]]
    return " ".join(str(t) for t in tok)


@pytest.mark.parametrize("n,d,q,theta,corr,mean", [(130, 3, 5, 1.5, "Matern52", "Quadratic"), (130, 2, 2, 4.0, "SquaredExponential", "Constant"),
                                                   (130, 3, 16, 1.5, "AbsoluteExponential", "Constant"),
                                                   (130, 1, 1, 30.0, "AbsoluteExponential", "Constant")])
def test_pending_math_header(exe, n, d, q, theta, corr, mean):
    """bordered Cholesky, alpha, the sigma2 recursion and the per-point finish: the header against numpy, and through the
    oracle's cross-covariances against the refit"""
    g, xv, yv, xq = _case(n, d, q, theta, corr, mean)
    xn, s, delta = PO._system(g, xv, yv)
    xqn = (xq - g.x_mean) / g.x_std
    cq = PO.unit_cov(g, xqn, xn)
    bm, bv = g.predict_valvar(xq)
    ref = PO.refit_frozen(g, xv, yv)
    rm, rv = ref.predict_valvar(xq)
    y_std, sigma2 = float(g.y_std[0]), g.inner.sigma2
    rng = np.random.default_rng(5)
    dcs = rng.standard_normal((xq.shape[0], q))
    lines = [_line(q, n, sigma2, y_std, s, delta, cq[i], bm[i], bv[i], 0.7, 0.3, -0.2, dcs[i]) for i in range(xq.shape[0])]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [[float(v) for v in ln.split()] for ln in out.strip().splitlines()]
    assert len(rows) == len(lines)
    chol = sla.cholesky(s, lower=True)
    alpha = sla.cho_solve((chol, True), delta)
    s2c = (n * sigma2 + y_std * y_std * delta.dot(alpha)) / (n + q)
    np.testing.assert_allclose(s2c, ref.inner.sigma2, rtol=1e-10)
    for i, row in enumerate(rows):
        got_l = np.array(row[:q * q]).reshape(q, q)
        np.testing.assert_allclose(got_l, chol, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(row[q * q:q * q + q], alpha, rtol=1e-9, atol=1e-12 * np.abs(alpha).max())
        got_s2, got_m, got_v, got_gm, got_gv = row[q * q + q:]
        np.testing.assert_allclose(got_s2, s2c, rtol=1e-12)
        b = sla.cho_solve((chol, True), cq[i])
        np.testing.assert_allclose(got_gm, 0.3 + y_std * dcs[i].dot(alpha) / 0.7, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(got_gv, -0.2 * s2c / sigma2 - 2.0 * s2c * dcs[i].dot(b) / 0.7, rtol=1e-9, atol=1e-12 * s2c)
        # ... and the point's mean and variance are the refit's
        np.testing.assert_allclose(got_m, rm[i], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(got_v, rv[i], rtol=0, atol=1e-9 * ref.inner.sigma2)


def test_pending_math_failed_pivot(exe):
    """the same point twice without a nugget: the second pivot is 0 -- reported, never a NaN factor"""
    s = np.array([[1.0, 1.0], [1.0, 1.0]])
    line = _line(2, 10, 1.0, 1.0, s, [0.0, 0.0], [0.0, 0.0], 0.0, 1.0, 1.0, 0.0, 0.0, [0.0, 0.0])
    out = subprocess.run([exe], input=line + "\n", capture_output=True, text=True, check=True).stdout
    assert out.strip() == "FAIL 1"


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_headers_declare_and_the_library_exports_the_entry_points():
    import egobox_amd as egx
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egx_gp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egx_[a-z0-9_]+)\s*\(", txt))
    lib = C.CDLL(egx._lib.LIB_PATH)
    bound = {s[0] for s in egx._lib.SIGNATURES}
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in bound, name
    assert "#define EGX_INFILL_MAX_PENDING 16" in open(os.path.join(ROOT, "include", "egx_gp.h")).read()
    assert re.search(r"#define EGX_GP_ABI_VERSION 2\b", open(os.path.join(ROOT, "include", "egx_gp.h")).read())
    assert [int(s) for s in egx.QEiStrategy] == [0, 1, 2, 3]
    cfg = egx._lib.InfillBatchConfig()
    egx._lib.load().egx_infill_batch_config_default(C.byref(cfg))
    assert (cfg.strategy, cfg.optimizer, cfg.max_eval, cfg.n_scaling) == (0, 1, 0, 0) and not cfg.scaling_points


def test_headers_compile_with_the_new_entries(tmp_path):
    inc = os.path.join(ROOT, "include")
    c = tmp_path / "t.c"
    c.write_text('#include "egx_gp.h"\nint use(egx_infill *h, const double *x, double *y) {\n'
                 '    egx_infill_batch_config cfg;\n    int32_t q = 0, nf = 0;\n    egx_infill_batch_config_default(&cfg);\n'
                 '    cfg.strategy = EGX_QEI_KB_UB;\n    cfg.optimizer = EGX_BATCH_COBYLA;\n'
                 '    if (egx_infill_virtual_point(h, x, EGX_QEI_CL_MIN, y)) return 1;\n'
                 '    if (egx_infill_push_pending(h, x, y) || egx_infill_get_pending(h, &q, 0, 0, 0)) return 2;\n'
                 '    if (egx_infill_optimize_batch(h, &cfg, x, x, x, 1, 1, y, y, y, &nf)) return 3;\n'
                 '    return egx_infill_clear_pending(h) + q + nf + EGX_INFILL_MAX_PENDING;\n}\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{inc}", str(c)], check=True)
    cpp = tmp_path / "t.cpp"
    cpp.write_text('#include "egx_gp.hpp"\nint use(egobox::GaussianProcess &gp) {\n'
                   '    egobox::InfillObjective o(gp, {}, {}, EGX_INFILL_EI, 0.0);\n    double x[1] = {0.0}, lo[1] = {0.0}, hi[1] = {1.0};\n'
                   '    auto y = o.virtual_point(x, egobox::QEiStrategy::KrigingBelieverUpperBound);\n    o.push_pending(x, y.data());\n'
                   '    auto b = o.optimize_batch(lo, hi, x, 1, 1, egobox::QEiStrategy::ConstantLiarMinimum);\n    o.clear_pending();\n'
                   '    return b.n_found + o.n_pending();\n}\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{inc}", str(cpp)], check=True)
