"""egx_gmm_fit on the GPU (EM of a full-covariance Gaussian mixture, the restarts in lock-step) against the numpy oracle of
tests/gmm_oracle.py: parity at the project's 1e-8 bar on every restart, the default stopping rule, bit-for-bit independence
of a restart from its batch, offset data, failed restarts as values, and a C99 host on the C ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gmm_oracle as GO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def close(a, b, tol=1e-8):
    """The project's parity bar: `tol` relative, absolute where the value is below 1."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert err.size and np.all(err <= tol), f"max error {err.max():.3e} > {tol:g}"
    return float(err.max())


def check_against_oracle(gm, runs, best):
    """Every restart's status, iteration count and lower bound, the parameters of the restarts that did not fail, the best
    restart and its parameters."""
    assert [int(s) for s in gm.statuses_] == [r["status"] for r in runs]
    assert [int(i) for i in gm.n_iters_] == [r["n_iter"] for r in runs]
    assert gm.best_run_ == best
    worst = 0.0
    for j, r in enumerate(runs):
        if r["status"] == GO.FAILED:
            assert np.isnan(gm.lower_bounds_[j])
            continue
        worst = max(worst, close(gm.lower_bounds_[j], r["lower_bound"]), close(gm.all_weights_[j], r["weights"]),
                    close(gm.all_means_[j], r["means"]), close(gm.all_covariances_[j], r["covariances"]))
    close(gm.weights, runs[best]["weights"])
    close(gm.means, runs[best]["means"])
    close(gm.covariances, runs[best]["covariances"])
    assert gm.lower_bound_ == gm.lower_bounds_[best] and gm.n_iter_ == runs[best]["n_iter"]
    return worst


def starts_with_a_unique_best(x, n_runs, k, iters, seed):
    """Seeded starts (k distinct rows per restart) under which the ORACLE's two greatest lower bounds are 1e-6 apart, so that
    rounding cannot decide best_run: on well-separated blobs two restarts that each hit every blob end in the same mixture
    to the last bit.  The first seed from `seed` on that qualifies; the library is not consulted."""
    for s in range(seed, seed + 64):
        st = GO.starts(x, n_runs, k, seed=s)
        runs, best = GO.fit(x, st, max_iter=iters, tol=0.0)
        lbs = sorted(r["lower_bound"] for r in runs if r["status"] != GO.FAILED)
        if len(lbs) == n_runs and (n_runs == 1 or lbs[-1] - lbs[-2] > 1e-6 * max(1.0, abs(lbs[-1]))):
            return st, runs, best
    raise AssertionError("no seed gives a unique best restart")


# (n, D, k, R, iterations): below one wave, exactly one, one over, a ragged last tile; nx = 1, a D that is no multiple of 4,
# D = 17 and D = 33; one cluster and eight; several workgroups per restart with the whole batch of 20
CASES = [(7, 3, 3, 3, 4), (64, 3, 3, 3, 4), (65, 3, 3, 3, 4), (257, 3, 3, 3, 4),
         (257, 2, 2, 3, 4), (257, 5, 2, 3, 4), (257, 17, 2, 3, 4), (257, 33, 2, 3, 4),
         (257, 3, 1, 2, 4), (257, 3, 8, 3, 4),
         (4099, 17, 8, 20, 3)]


@pytest.mark.parametrize("n,d,k,n_runs,iters", CASES)
def test_em_matches_the_oracle(egx, n, d, k, n_runs, iters):
    """tol = 0 and a fixed max_iter: the iteration counts cannot differ.  The starts are such that rounding cannot decide
    best_run (starts_with_a_unique_best); with one cluster every start gives the same mixture, so there both restarts get
    the SAME start and the tie goes to the lowest index."""
    x = GO.blobs(n, d, k, seed=100 + n + d + k)
    if k == 1:
        st = np.repeat(GO.starts(x, 1, k, seed=n), n_runs, axis=0)
        runs, best = GO.fit(x, st, max_iter=iters, tol=0.0)
    else:
        st, runs, best = starts_with_a_unique_best(x, n_runs, k, iters, seed=n + 7 * d + k)
    gm = egx.GaussianMixture.fit(x, k, n_runs=n_runs, max_iter=iters, tol=0.0, init_means=st)
    worst = check_against_oracle(gm, runs, best)
    print(f"n {n} D {d} k {k} R {n_runs}: max error {worst:.2e}")
    assert [r["status"] for r in runs] == [GO.MAX_ITER] * n_runs
    if k == 1:
        assert best == 0 and gm.lower_bounds_[0] == gm.lower_bounds_[1]


def test_default_stopping_rule(egx):
    """n = 301, D = 3, k = 3: the oracle stops after 5 iterations under the defaults (tol 1e-3), and so does the library.  No
    |delta lb| of the oracle's trace lies within a factor 10 of tol, so rounding cannot flip the comparison."""
    x = GO.blobs(301, 3, 3, seed=12, separation=6.0)
    st = GO.starts(x, 1, 3, seed=3)
    runs, best = GO.fit(x, st)
    delta = np.abs(np.diff(np.array(runs[0]["trace"])))
    assert runs[0]["status"] == GO.CONVERGED and runs[0]["n_iter"] == 5
    assert not np.any((delta >= 1e-4) & (delta <= 1e-2)), delta
    gm = egx.GaussianMixture.fit(x, 3, n_runs=1, init_means=st)
    assert gm.n_iter_ == 5 and int(gm.statuses_[0]) == GO.CONVERGED
    check_against_oracle(gm, runs, best)


def _params(gm, j=None):
    if j is None:
        return [gm.weights, gm.means, gm.covariances, np.float64(gm.lower_bound_)]
    return [gm.all_weights_[j], gm.all_means_[j], gm.all_covariances_[j], gm.lower_bounds_[j]]


def test_a_restart_does_not_depend_on_its_batch(egx):
    """Restart j of 20 is bit for bit the call with that start alone (several workgroups per restart: n = 1030); two
    identical calls are bit-identical."""
    x = GO.blobs(1030, 5, 3, seed=4, separation=4.0)
    st = GO.starts(x, 20, 3, seed=9)
    kw = dict(max_iter=4, tol=0.0)
    a = egx.GaussianMixture.fit(x, 3, n_runs=20, init_means=st, **kw)
    b = egx.GaussianMixture.fit(x, 3, n_runs=20, init_means=st, **kw)
    for j in range(20):
        for u, v in zip(_params(a, j), _params(b, j)):
            np.testing.assert_array_equal(u, v)
    assert a.best_run_ == b.best_run_
    for j in (0, 7, 19):
        one = egx.GaussianMixture.fit(x, 3, n_runs=1, init_means=st[j:j + 1], **kw)
        for u, v in zip(_params(a, j), _params(one)):
            np.testing.assert_array_equal(u, v)
        assert int(one.statuses_[0]) == int(a.statuses_[j]) and int(one.n_iters_[0]) == int(a.n_iters_[j])


def test_offset_data(egx):
    """Moments about the previous mean, not about zero: a shift of 1e6 moves the means and nothing else (the two-pass oracle
    itself holds 7e-10 on such data, raw moments 1.7e-3)."""
    x = GO.blobs(301, 3, 3, seed=5)
    st = starts_with_a_unique_best(x, 2, 3, 5, seed=1)[0]
    kw = dict(max_iter=5, tol=0.0)
    a = egx.GaussianMixture.fit(x, 3, n_runs=2, init_means=st, **kw)
    b = egx.GaussianMixture.fit(x + 1e6, 3, n_runs=2, init_means=st + 1e6, **kw)
    for j in range(2):
        close(b.all_means_[j] - 1e6, a.all_means_[j])
        close(b.all_covariances_[j], a.all_covariances_[j])
        close(b.all_weights_[j], a.all_weights_[j])
        close(b.lower_bounds_[j], a.lower_bounds_[j])
    assert a.best_run_ == b.best_run_


def test_blobs_a_thousand_spreads_apart(egx):
    x = GO.blobs(301, 3, 3, seed=6, separation=1e3, spread=1.0)
    st, runs, best = starts_with_a_unique_best(x, 3, 3, 5, seed=2)
    gm = egx.GaussianMixture.fit(x, 3, n_runs=3, max_iter=5, tol=0.0, init_means=st)
    check_against_oracle(gm, runs, best)


def test_failed_restarts_are_values(egx):
    """reg_covar = 0 and a restart whose two initial means are the same row: cluster 1 gets no rows, its covariance is the
    zero matrix, the restart reports status 2 and the other one wins; with every restart built that way the call returns an
    error code (ClusteringError in Python).  A numerical status: nothing faults."""
    x = GO.blobs(64, 2, 2, seed=2)
    dead, live = np.stack([x[0], x[0]]), np.stack([x[0], x[1]])
    st = np.stack([dead, live])
    runs, best = GO.fit(x, st, max_iter=5, tol=0.0, reg_covar=0.0)
    assert [r["status"] for r in runs] == [GO.FAILED, GO.MAX_ITER] and best == 1
    gm = egx.GaussianMixture.fit(x, 2, n_runs=2, max_iter=5, tol=0.0, reg_covar=0.0, init_means=st)
    assert int(gm.statuses_[0]) == GO.FAILED and gm.best_run_ == 1
    check_against_oracle(gm, runs, best)
    with pytest.raises(egx.ClusteringError, match="every restart failed"):
        egx.GaussianMixture.fit(x, 2, n_runs=2, max_iter=5, tol=0.0, reg_covar=0.0, init_means=np.stack([dead, dead]))
    # the same through the C ABI: an error code and a message, the per-restart outputs filled
    L = egx._lib
    lib = L.load()
    cfg = L.GmmConfig()
    lib.egx_gmm_config_default(cfg)
    cfg.n_clusters, cfg.n_runs, cfg.max_iter, cfg.tol, cfg.reg_covar = 2, 2, 5, 0.0, 0.0
    xs, sd = np.ascontiguousarray(x), np.ascontiguousarray(np.stack([dead, dead]))
    w, m, c, lb = np.empty(2), np.empty((2, 2)), np.empty((2, 2, 2)), np.empty(2)
    it, stt, best_c = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), C.c_int32(7)
    rc = lib.egx_gmm_fit(cfg, L.dptr(xs), 64, 2, L.dptr(sd), L.dptr(w), L.dptr(m), L.dptr(c), L.dptr(lb),
                         it.ctypes.data_as(L.c_int32_p), stt.ctypes.data_as(L.c_int32_p), C.byref(best_c), None, None, None)
    assert rc == L.ERR_LINALG and b"every restart failed" in lib.egx_last_error()
    assert list(stt) == [2, 2] and best_c.value == -1 and list(it) == [0, 0]
    # the library still works afterwards
    again = egx.GaussianMixture.fit(x, 2, n_runs=1, max_iter=5, tol=0.0, reg_covar=0.0, init_means=st[1:])
    np.testing.assert_array_equal(again.means, gm.means)


def test_limits_are_errors(egx):
    rng = np.random.default_rng(0)
    with pytest.raises(egx.InvalidValueError, match="dim <= 36"):
        egx.GaussianMixture.fit(rng.random((100, 37)), 2, n_runs=1)
    with pytest.raises(egx.InvalidValueError, match="n_clusters <= 16"):
        egx.GaussianMixture.fit(rng.random((100, 3)), 17, n_runs=1)


def test_plain_c_host_trains_a_mixture(tmp_path):
    """tests/c_host/gmm_driver.c: a C99 program trains a 64 x 3 mixture through egx_gmm_fit."""
    exe = tmp_path / "gmm_driver"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "gmm_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK")
