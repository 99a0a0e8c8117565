"""PLS rotations on the GPU (egx_pls_rotations, egx_sgp_compute_w_star, the builders' pls("device")) against the long-double
NIPALS of tests/pls_oracle.py.

The rule, per row (n, d, k) of pls_oracle.CASES: with e_dev, e_host, e_gram the sign-insensitive column errors of the device
result, of `kpls.pls_rotations` and of the numpy Gram form against the long-double oracle,
    e_dev <= 8 max(e_host, e_gram, 16 eps).
The rows are the smallest shapes at which each way the kernels can go wrong shows: one chunk, two chunks with a ragged last one,
three chunks (from egx_pls_get_plan), n in {2, 5, 17, 127, 129} for the K tail and the padding, d + 1 on and off a 16-wide tile
and a 64-wide block, k up to d, a mean 1e8 times the spread, a constant column, scales spread over 1e4.
EGX_PLS_PARITY_OUT=<file>: the measured ratios per row are written there as well (profiles/pls_parity.txt is such a file)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pls_oracle as PO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    import egobox_amd.kpls  # noqa: F401  (egx.kpls)
    return egobox_amd


@pytest.fixture(scope="module")
def rows(egx):
    return PO.rows(egx.kpls.pls_plan)


def _data(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3.0 * x[:, 0]) + x @ rng.standard_normal(d) + 0.05 * rng.standard_normal(n)
    return x, y


# ---- parity
def test_parity_with_the_long_double_oracle(egx, rows):
    lines, bad = [], []
    for name, n, d, k, kind, x, y, ref, e_host, e_gram in rows:
        w, status = egx.kpls.pls_rotations_device(x, y, k, return_status=True)
        e_dev = PO.col_err(w, ref)
        bound = PO.bound(e_host, e_gram)
        lines.append(f"{name:14s} n {n:4d} d {d:3d} k {k:2d}  e_dev {e_dev:.3e}  e_host {e_host:.3e}  e_gram {e_gram:.3e}  "
                     f"e_dev / max(e_host, e_gram, 16 eps) {e_dev / (bound / PO.FACTOR):.3f}  (allowed {PO.FACTOR:g})")
        print(lines[-1])
        if status != 0 or w.shape != (d, k) or not e_dev <= bound:
            bad.append((name, status, e_dev, bound))
        if kind == "constcol" and np.any(w[PO.CONST_COLUMN] != 0.0):
            bad.append((name, "the constant column's row is not zero", w[PO.CONST_COLUMN]))
    out = os.environ.get("EGX_PLS_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert not bad, bad


# ---- same bits
def test_same_bits_on_every_call_and_for_every_leading_dimension(egx):
    """Two calls of egx_pls_rotations; egx_pls_rotations (leading dimension n rounded up to 16) against egx_sgp_compute_w_star
    (the handle's n rounded up to 128): the same kernels in the same order."""
    for n, d, k in ((300, 17, 3), (600, 65, 4), (129, 5, 5)):
        x, y = _data(n, d, seed=n + d)
        a = egx.kpls.pls_rotations_device(x, y, k)
        b = egx.kpls.pls_rotations_device(x, y, k)
        np.testing.assert_array_equal(a, b)
        with egx.SgpHandle(x, y, x[:4].copy(), corr=0) as h:
            c = h.compute_w_star(k)
            assert h.h == k
            np.testing.assert_array_equal(c, a)
            np.testing.assert_array_equal(h.compute_w_star(k), a)


# ---- a constant response
def test_constant_response_gives_zeros_and_status_1(egx):
    x, _ = _data(70, 4, seed=5)
    for const in (0.0, 3.7, -1e6):
        y = np.full(70, const)
        w, status = egx.kpls.pls_rotations_device(x, y, 2, return_status=True)
        assert status == 1 and w.shape == (4, 2) and not np.any(w)
        np.testing.assert_array_equal(egx.kpls.pls_rotations(x, y, 2), w)
    with egx.SgpHandle(x, np.full(70, 3.7), x[:6].copy(), corr=0) as h:
        w = h.compute_w_star(2)
        assert w is not None and w.shape == (4, 2) and not np.any(w) and h.h == 2
        lk, st = h.likelihood(np.array([1.0, 1.0]), 0.5, 0.01)  # still evaluates: the status is a value, not an exception
        assert isinstance(st, int) and (st != 0 or np.isfinite(lk))


# ---- fit parity, sparse
def test_sparse_handle_computes_and_installs_its_weights(egx):
    n, d, k = 300, 8, 3
    x, y = _data(n, d, seed=11)
    z = x[:20].copy()
    th, s2, noise = np.array([0.8, 1.1, 0.6]), 0.7, 0.02
    w_host = egx.kpls.pls_rotations(x, y, k)
    with egx.SgpHandle(x, y, z, corr=0) as h, egx.SgpHandle(x, y, z, corr=0) as h2, egx.SgpHandle(x, y, z, corr=0, w_star=w_host) as h3:
        h.finalize(np.full(d, 1.0), s2, noise)
        h.predict_valvar(x[:3])
        w = h.compute_w_star(k)
        with pytest.raises(egx.NotFittedError):  # un-fitted, as after set_w_star
            h.predict_valvar(x[:3])
        assert w.shape == (d, k) and h.h == k
        np.testing.assert_array_equal(h.w_star(), w)
        with pytest.raises(egx.InvalidValueError, match=r"w_star\.ncols\(\)"):  # theta is k long now
            h.likelihood(np.full(d, 1.0), s2, noise)
        h2.set_w_star(w)
        lk, st = h.likelihood(th, s2, noise)
        lk2, st2 = h2.likelihood(th, s2, noise)
        assert st == 0 and st2 == 0 and lk == lk2
        h.finalize(th, s2, noise)
        h2.finalize(th, s2, noise)
        for a, b in zip(h.predict_valvar(x[:9] + 0.01), h2.predict_valvar(x[:9] + 0.01)):
            np.testing.assert_array_equal(a, b)
        lk3, st3 = h3.likelihood(th, s2, noise)  # under the host weights: the project's likelihood bar
        assert st3 == 0 and abs(lk - lk3) <= 1e-8 * abs(lk3), (lk, lk3)
        with pytest.raises(egx.InvalidValueError, match="canot be 0"):
            h.compute_w_star(0)
        with pytest.raises(egx.InvalidValueError, match=f"Dimension reduction {d + 1}"):
            h.compute_w_star(d + 1)
        assert h.h == k  # a refused call leaves the handle as it was
        np.testing.assert_array_equal(h.w_star(), w)


def test_sparse_builder_with_pls_device(egx):
    n, d, k = 300, 8, 3
    x, y = _data(n, d, seed=12)

    def params():
        return egx.SparseGaussianProcess.params(egx.Inducings.Located(x[:20].copy())).kpls_dim(k) \
            .theta_tuning(egx.ThetaTuning.Fixed([0.9])).noise_variance(egx.ParamTuning.Fixed(0.02)).n_start(0)

    host0, host, dev = params().fit(x, y), params().pls("host").fit(x, y), params().pls("device").fit(x, y)
    np.testing.assert_array_equal(host0.w_star(), egx.kpls.pls_rotations(x, y, k))
    np.testing.assert_array_equal(host.w_star(), host0.w_star())
    assert host.likelihood() == host0.likelihood()
    # the device weights are installed and the fit (sigma2 by the optimiser, whose path the test does not pin) went through on them
    np.testing.assert_array_equal(dev.w_star(), egx.kpls.pls_rotations_device(x, y, k))
    assert len(np.atleast_1d(dev.theta())) == k and np.isfinite(dev.likelihood())
    assert np.all(np.isfinite(dev.predict(x[:7] + 0.01)))


# ---- fit parity, dense
def test_dense_builder_with_pls_device(egx):
    n, d, k = 120, 10, 3
    x, y = _data(n, d, seed=13)
    xq = np.random.default_rng(3).random((33, d))

    def params():
        return egx.GaussianProcess.params(egx.ConstantMean(), egx.SquaredExponentialCorr()).kpls_dim(k) \
            .theta_tuning(egx.ThetaTuning.Fixed([1.2]))

    plain, host, dev = params().fit(x, y), params().pls("host").fit(x, y), params().pls("device").fit(x, y)
    assert host.likelihood() == plain.likelihood()  # pls("host") and no call at all: bit for bit
    for a, b in zip(host.predict_valvar(xq), plain.predict_valvar(xq)):
        np.testing.assert_array_equal(a, b)
    assert len(np.atleast_1d(dev.theta())) == k
    assert abs(dev.likelihood() - host.likelihood()) <= 1e-8 * abs(host.likelihood()), (dev.likelihood(), host.likelihood())
    yd, vd = dev.predict_valvar(xq)
    yh, vh = host.predict_valvar(xq)
    np.testing.assert_allclose(yd, yh, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(vd, vh, rtol=1e-6, atol=1e-9)


# ---- C++
def test_cpp_builder_fits_with_kpls_dim(egx, tmp_path):
    """tests/c_host/kpls_params.cpp: GpParams::kpls_dim(2) through include/egx_gp.hpp; theta has 2 components and the prediction
    is that of the Python device path on the same data."""
    exe = tmp_path / "kpls_params"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "kpls_params.cpp"), f"-L{libdir}", "-legx_gp_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = out.stdout.strip().splitlines()
    assert lines[0] == "OK", lines
    got = {ln.split()[0]: np.array(ln.split()[1:], dtype=np.float64) for ln in lines[1:]}
    assert got["theta_len"][0] == 2 and got["kpls_dim"][0] == 2
    n, d, m = 60, 5, 3
    i, k = np.arange(n)[:, None], np.arange(d)[None, :]
    x = ((7 * i + 13 * k + 3 * i * k) % 32) / 16.0 - 1.0
    y = 0.5 * x[:, 0] - 0.25 * x[:, 2] * x[:, 1] + ((5 * np.arange(n)) % 17) / 64.0
    xq = ((11 * np.arange(m)[:, None] + 5 * k) % 16) / 8.0 - 0.9375
    np.testing.assert_array_equal(got["w"].reshape(d, 2), egx.kpls.pls_rotations_device(x, y, 2))
    gp = egx.GaussianProcess.params(egx.ConstantMean(), egx.SquaredExponentialCorr()).kpls_dim(2).pls("device") \
        .theta_tuning(egx.ThetaTuning.Fixed([0.75])).fit(x, y)
    np.testing.assert_array_equal(got["predict"], np.asarray(gp.predict(xq)).reshape(-1))
