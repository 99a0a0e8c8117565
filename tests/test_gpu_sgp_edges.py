"""The sparse GP's forward path on the GPU -- likelihood, fitted state, predict, predict_var and the query loop of sgp_query --
against the CPU oracle at the padding, block, split and chunk edges of tests/sgp_edge_cases.py.  tests/test_sgp_edges_cpu.py
shows on the oracle alone that it can vouch for every row at these bars, so a failure here is the kernels'.
Bars (the project's own: BASELINE.json, the header of tests/test_sgp_gpu.py): likelihood 1e-8 relative; mean rtol 1e-6 with
atol 1e-8; variance rtol 1e-6 with atol 1e-9, queries within 1e-7 sigma2 of the clamp left out of the variance comparison only
and clamped queries equal to 1e-15 + noise exactly; w_vec / w_inv rtol 1e-6 with atol 1e-6 max |ref|; x-gradients the bars of
tests/test_gpu_sgp_surrogate.py (PRED_RTOL with atol 1e-6 max |ref|, exactly 0 under the clamp).

What this file cannot see, by construction: the mask `i < nz` of k_sgp_transpose_scale.  Without it the padded rows of W carry the
correlations with z = 0, so G and A = I + G change beyond row nz -- but the first nz rows of a Cholesky factor, of a forward
substitution and of a row reduction over nz columns depend on the leading nz x nz block alone, and the backward substitutions
start from a right-hand side that is zero beyond nz: likelihood, w_vec, w_inv and every prediction keep their bits (measured with
a scratch build: all 112 forward cases pass unchanged).  The mask is needed by the likelihood's gradient, which forms A^-1 over
z_pad, and is guarded there: tests/test_gpu_sgp_grad.py::test_gradient_matches_the_restatement fails 47 of 48 with that build."""
import numpy as np
import pytest

import sgp_edge_cases as EC
from test_gpu_sgp_surrogate import PRED_RTOL
from test_sgp_surrogate_cpu import analytic_gradients

pytestmark = pytest.mark.gpu

S2, NV = EC.SIGMA2, EC.NOISE


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _handle(egx, cid, corr, method):
    x, y, z, w = EC.data(cid)
    return egx.SgpHandle(x, y, z, corr=corr, method=method, w_star=w)


def _dev(got, ref):
    """max |got - ref| relative to max |ref| (1 where the reference is all zero)."""
    scale = np.abs(ref).max() if np.size(ref) else 0.0
    return float(np.abs(got - ref).max() / (scale if scale > 0.0 else 1.0)) if np.size(ref) else 0.0


def _check_valvar(mean, var, ref_mean, ref_var, var_raw, label):
    """Mean (if given) and variance against the oracle's rows; returns the two relative deviations for the printed line."""
    sure = ~EC.unsure(var_raw)
    clamped = sure & (var_raw < 1e-15)
    devs = (_dev(mean, ref_mean) if mean is not None else 0.0, _dev(var[sure], ref_var[sure]))
    print(f"{label}: mean {devs[0]:.3g}, var {devs[1]:.3g}, left out {(~sure).sum()} of {sure.size}, clamped {clamped.sum()}")
    if mean is not None:
        np.testing.assert_allclose(mean, ref_mean, rtol=1e-6, atol=1e-8, err_msg=label)
    np.testing.assert_allclose(var[sure], ref_var[sure], rtol=1e-6, atol=1e-9, err_msg=label)
    assert np.all(var[clamped] == 1e-15 + NV), label
    return devs


def _check_gradients(gy, gv, gy_ref, gv_ref, var_raw, label):
    """compare_gradients of tests/test_gpu_sgp_surrogate.py on given rows (its bars and its unsure-row rule; the share of unsure
    rows is capped on the CPU, tests/test_sgp_edges_cpu.py)."""
    keep = ~EC.unsure(var_raw)
    clamped = keep & (var_raw < 1e-15)
    print(f"{label}: dmean {_dev(gy, gy_ref):.3g}, dvar {_dev(gv[keep], gv_ref[keep]):.3g}, left out {(~keep).sum()} of {keep.size}, "
          f"clamped {clamped.sum()}")
    np.testing.assert_allclose(gy, gy_ref, rtol=PRED_RTOL, atol=1e-6 * np.abs(gy_ref).max(), err_msg=label)
    np.testing.assert_allclose(gv[keep], gv_ref[keep], rtol=PRED_RTOL, atol=1e-6 * np.abs(gv_ref).max(), err_msg=label)
    assert np.all(gv[clamped] == 0.0), label


# ------------------------------------------------------------------ a. the forward path, every row
_worst = {}


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
@pytest.mark.parametrize("cid", list(EC.CASES))
def test_forward_path_vs_oracle(egx, cid, corr, method):
    ref = EC.oracle(cid, corr, method)
    th, nz = EC.theta(cid), EC.CASES[cid][1]
    xq = EC.queries(cid, EC.M_FORWARD)
    with _handle(egx, cid, corr, method) as h:
        lk, st = h.likelihood(th, S2, NV)
        h.finalize(th, S2, NV)
        s = h.state(with_inv=True)
        mean, var = h.predict(xq), h.predict_var(xq)
    label = f"{cid} corr {corr} method {method}"
    d_lk = abs(lk - ref.likelihood) / abs(ref.likelihood)
    d_vec, d_inv = _dev(s["w_vec"], ref.w_vec[:, 0]), _dev(s["w_inv"], ref.w_inv)
    print(f"{label}: likelihood {d_lk:.3g}, w_vec {d_vec:.3g}, w_inv {d_inv:.3g}")
    assert st == 0 and lk == pytest.approx(ref.likelihood, rel=1e-8)
    assert s["likelihood"] == lk and s["sigma2"] == S2 and s["noise"] == NV
    np.testing.assert_array_equal(s["theta"], th)
    # the state is handed out without its padding: nz values, nz x nz
    assert s["w_vec"].shape == (nz,) and s["w_inv"].shape == (nz, nz)
    np.testing.assert_allclose(s["w_vec"], ref.w_vec[:, 0], rtol=1e-6, atol=1e-6 * np.abs(ref.w_vec).max())
    np.testing.assert_allclose(s["w_inv"], ref.w_inv, rtol=1e-6, atol=1e-6 * np.abs(ref.w_inv).max())
    d_mean, d_var = _check_valvar(mean, var, ref.predict(xq), ref.predict_var(xq), EC.raw_variance(ref, xq), label)
    w = _worst.setdefault(cid, [0.0] * 5)
    w[:] = [max(a, b) for a, b in zip(w, (d_lk, d_vec, d_inv, d_mean, d_var))]
    print(f"worst so far, row {cid}: likelihood {w[0]:.3g}, w_vec {w[1]:.3g}, w_inv {w[2]:.3g}, mean {w[3]:.3g}, var {w[4]:.3g}")


# ------------------------------------------------------------------ b. query counts, each against the oracle itself
_count_ref = {}


def _count_reference(corr, method):
    """Oracle rows of the nz129 row's largest query set, computed once; every count is a prefix of it."""
    key = (corr, method)
    if key not in _count_ref:
        ref = EC.oracle("nz129", corr, method)
        xq = EC.queries("nz129", max(EC.M_COUNTS))
        _count_ref[key] = (ref.predict(xq), ref.predict_var(xq)) + analytic_gradients(ref, xq)
    return _count_ref[key]


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", [0, 3])
def test_query_counts_vs_oracle(egx, corr, method):
    """m around the few-query switch (16 / 17) and around one and two tiles of 128 queries, on the model whose inducing points
    reach one column into a second block: predict, predict_var, predict_valvar and both x-gradients."""
    r_mean, r_var, r_gy, r_gv, var_raw = _count_reference(corr, method)
    th = EC.theta("nz129")
    with _handle(egx, "nz129", corr, method) as h:
        h.finalize(th, S2, NV)
        for m in EC.M_COUNTS:
            xq = EC.queries("nz129", m)
            label = f"nz129 corr {corr} method {method} m {m}"
            _check_valvar(h.predict(xq), h.predict_var(xq), r_mean[:m], r_var[:m], var_raw[:m], label + " two calls")
            _check_valvar(*h.predict_valvar(xq), r_mean[:m], r_var[:m], var_raw[:m], label + " valvar")
            gy, gv = h.predict_valvar_gradients(xq)
            assert gy.shape == gv.shape == (m, 4)
            _check_gradients(gy, gv, r_gy[:m], r_gv[:m], var_raw[:m], label)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", [0, 3])
def test_few_query_route_nz257_two_partial_sums_sgp_predict_hip_line_171(egx, corr, method):
    """sgp_predict.hip:171, nblk = (nz + 255) / 256: with more than 256 inducing points the few-query contraction
    (launch_xgrad_point) leaves two partial sums per query for k_sgp_grad_finish; no other few-query test has nz > 256."""
    ref = EC.oracle("nz257", corr, method)
    xq = EC.queries("nz257", 3)
    gy_ref, gv_ref, var_raw = analytic_gradients(ref, xq)
    with _handle(egx, "nz257", corr, method) as h:
        h.finalize(EC.theta("nz257"), S2, NV)
        label = f"nz257 corr {corr} method {method} m 3"
        _check_valvar(*h.predict_valvar(xq), ref.predict(xq), ref.predict_var(xq), var_raw, label)
        _check_gradients(*h.predict_valvar_gradients(xq), gy_ref, gv_ref, var_raw, label)
        _check_gradients(h.predict_gradients(xq[:1]), h.predict_var_gradients(xq[:1]), gy_ref[:1], gv_ref[:1], var_raw[:1], label + ", one")


# ------------------------------------------------------------------ c. the 65536-query chunk
_chunk_ref = {}
G0 = EC.CHUNK - 8  # gradients: the last 8 rows of the first chunk and every row of the second


def _chunk_reference(method):
    key = method
    if key not in _chunk_ref:
        ref = EC.oracle("A", 3, method)
        xq = EC.queries("A", max(EC.M_CHUNK))
        _chunk_ref[key] = (ref.predict(xq), ref.predict_var(xq), EC.raw_variance(ref, xq)) + analytic_gradients(ref, xq[G0:])[:2]
    return _chunk_ref[key]


@pytest.mark.parametrize("method", [0, 1])
def test_chunk_edges_vs_oracle(egx, method):
    """One fresh handle, calls in this order: m = 1 (small workspaces exist and must grow), 65537 (a second chunk of one row,
    m_pad = 128), 130 (a large workspace reused by a small call), then 65536 (exactly one chunk) and 65536 + 129.  Every row of
    every call against the oracle; the chunk loop is shared by all entry points, so comparing them with each other shows nothing."""
    r_mean, r_var, var_raw, r_gy, r_gv = _chunk_reference(method)
    with _handle(egx, "A", 3, method) as h:
        h.finalize(EC.theta("A"), S2, NV)
        for m in (1, EC.CHUNK + 1, 130, EC.CHUNK, EC.CHUNK + 129):
            xq = EC.queries("A", m)
            label = f"A corr 3 method {method} m {m}"
            _check_valvar(*h.predict_valvar(xq), r_mean[:m], r_var[:m], var_raw[:m], label + " valvar")
            if m != EC.CHUNK + 1:
                _check_valvar(h.predict(xq), h.predict_var(xq), r_mean[:m], r_var[:m], var_raw[:m], label + " two calls")
            gy, gv = h.predict_valvar_gradients(xq)
            assert gy.shape == gv.shape == (m, 3)
            if m > G0:
                _check_gradients(gy[G0:], gv[G0:], r_gy[:m - G0], r_gv[:m - G0], var_raw[G0:m], label + f" rows {G0}..")
            else:
                gy_ref, gv_ref, _ = analytic_gradients(EC.oracle("A", 3, method), xq)
                _check_gradients(gy, gv, gy_ref, gv_ref, var_raw[:m], label)
