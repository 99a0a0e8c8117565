"""egx_gmm_fit_wide on the GPU (the mixture's EM for rows up to 128 wide, its two O(D^2) products per row on the FP64 matrix
unit) against the numpy oracle of tests/gmm_oracle.py at the project's 1e-8 bar: every restart at the row-count, tile and
width edges, beside the narrow path where both run, the default stopping rule, bit-for-bit independence of a restart from
its batch, offset data, failed restarts as values, the limits, and a C99 host on the C ABI."""
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
    rounding cannot decide best_run.  The first seed from `seed` on that qualifies; the library is not consulted."""
    for s in range(seed, seed + 64):
        st = GO.starts(x, n_runs, k, seed=s)
        runs, best = GO.fit(x, st, max_iter=iters, tol=0.0)
        lbs = sorted(r["lower_bound"] for r in runs if r["status"] != GO.FAILED)
        if len(lbs) == n_runs and (n_runs == 1 or lbs[-1] - lbs[-2] > 1e-6 * max(1.0, abs(lbs[-1]))):
            return st, runs, best
    raise AssertionError("no seed gives a unique best restart")


# (n, D, k, R, iterations): the row-count edges through the wide kernels (below one 64-row tile, exactly one, one over, a
# ragged fifth); the first width the narrow path refuses; a D that is no multiple of 4 or 16; exactly four MFMA tiles and one
# column over; the limit with several row tiles; eight clusters; one cluster; the whole batch of 20 with a ragged last tile
CASES = [(7, 3, 3, 3, 4), (64, 3, 3, 3, 4), (65, 3, 3, 3, 4), (257, 3, 3, 3, 4),
         (300, 37, 2, 2, 3),
         (400, 50, 2, 2, 3),
         (520, 64, 2, 2, 3), (530, 65, 2, 2, 3),
         (1030, 128, 2, 2, 3),
         (1300, 40, 8, 3, 3),
         (257, 100, 1, 2, 3),
         (4099, 48, 4, 20, 3)]


@pytest.mark.parametrize("n,d,k,n_runs,iters", CASES)
def test_wide_em_matches_the_oracle(egx, n, d, k, n_runs, iters):
    """tol = 0 and a fixed max_iter: the iteration counts cannot differ.  With one cluster both restarts get the SAME start
    and the tie goes to the lowest index."""
    x = GO.blobs(n, d, k, seed=100 + n + d + k)
    if k == 1:
        st = np.repeat(GO.starts(x, 1, k, seed=n), n_runs, axis=0)
        runs, best = GO.fit(x, st, max_iter=iters, tol=0.0)
    else:
        st, runs, best = starts_with_a_unique_best(x, n_runs, k, iters, seed=n + 7 * d + k)
    gm = egx.GaussianMixture.fit_wide(x, k, n_runs=n_runs, max_iter=iters, tol=0.0, init_means=st)
    worst = check_against_oracle(gm, runs, best)
    print(f"n {n} D {d} k {k} R {n_runs}: max error {worst:.2e}")
    assert [r["status"] for r in runs] == [GO.MAX_ITER] * n_runs
    if k == 1:
        assert best == 0 and gm.lower_bounds_[0] == gm.lower_bounds_[1]


@pytest.mark.parametrize("d", [17, 33])
def test_wide_beside_narrow(egx, d):
    """The two paths from the same starts: the same bar (the sums have another order, so no bits), the same statuses,
    iteration counts and best run."""
    n, k, n_runs, iters = 257, 2, 3, 4
    x = GO.blobs(n, d, k, seed=100 + n + d + k)
    st = starts_with_a_unique_best(x, n_runs, k, iters, seed=n + 7 * d + k)[0]
    kw = dict(n_runs=n_runs, max_iter=iters, tol=0.0, init_means=st)
    a, b = egx.GaussianMixture.fit(x, k, **kw), egx.GaussianMixture.fit_wide(x, k, **kw)
    assert list(a.statuses_) == list(b.statuses_) and list(a.n_iters_) == list(b.n_iters_) and a.best_run_ == b.best_run_
    for j in range(n_runs):
        close(b.lower_bounds_[j], a.lower_bounds_[j])
        close(b.all_weights_[j], a.all_weights_[j])
        close(b.all_means_[j], a.all_means_[j])
        close(b.all_covariances_[j], a.all_covariances_[j])


def test_default_stopping_rule_at_width(egx):
    """n = 400, D = 40, k = 2: the oracle stops after 13 iterations under the defaults (tol 1e-3), and so does the library.
    No |delta lb| of the oracle's trace lies within a factor 10 of tol, so rounding cannot flip the comparison."""
    x = GO.blobs(400, 40, 2, seed=12, separation=6.0)
    st = GO.starts(x, 1, 2, seed=3)
    runs, best = GO.fit(x, st)
    delta = np.abs(np.diff(np.array(runs[0]["trace"])))
    assert runs[0]["status"] == GO.CONVERGED and runs[0]["n_iter"] == 13
    assert not np.any((delta >= 1e-4) & (delta <= 1e-2)), delta
    gm = egx.GaussianMixture.fit_wide(x, 2, n_runs=1, init_means=st)
    assert gm.n_iter_ == 13 and int(gm.statuses_[0]) == GO.CONVERGED
    check_against_oracle(gm, runs, best)


def _params(gm, j=None):
    if j is None:
        return [gm.weights, gm.means, gm.covariances, np.float64(gm.lower_bound_)]
    return [gm.all_weights_[j], gm.all_means_[j], gm.all_covariances_[j], gm.lower_bounds_[j]]


def test_a_wide_restart_does_not_depend_on_its_batch(egx):
    """Restart j of 20 is bit for bit the call with that start alone (n = 1030: 17 tiles, D = 40); two identical calls are
    bit-identical."""
    x = GO.blobs(1030, 40, 3, seed=4, separation=4.0)
    st = GO.starts(x, 20, 3, seed=9)
    kw = dict(max_iter=4, tol=0.0)
    a = egx.GaussianMixture.fit_wide(x, 3, n_runs=20, init_means=st, **kw)
    b = egx.GaussianMixture.fit_wide(x, 3, n_runs=20, init_means=st, **kw)
    for j in range(20):
        for u, v in zip(_params(a, j), _params(b, j)):
            np.testing.assert_array_equal(u, v)
    assert a.best_run_ == b.best_run_
    for j in (0, 7, 19):
        one = egx.GaussianMixture.fit_wide(x, 3, n_runs=1, init_means=st[j:j + 1], **kw)
        for u, v in zip(_params(a, j), _params(one)):
            np.testing.assert_array_equal(u, v)
        assert int(one.statuses_[0]) == int(a.statuses_[j]) and int(one.n_iters_[0]) == int(a.n_iters_[j])


def test_offset_data_at_width(egx):
    """Moments about the previous mean, not about zero: a shift of 1e5 at D = 40 moves the means and nothing else.  (At 1e6
    the ulp of x is 1.2e-10 and the oracle's own shifted and unshifted runs differ by 1.5e-9: no margin under 1e-8; at 1e5
    raw moments would still be wrong by about 1e-6.)  The oracle's two runs agree to 1e-9 here, which is asserted first."""
    shift = 1e5
    x = GO.blobs(301, 40, 3, seed=5)
    st = starts_with_a_unique_best(x, 2, 3, 5, seed=1)[0]
    kw = dict(max_iter=5, tol=0.0)
    ra, _ = GO.fit(x, st, **kw)
    rb, _ = GO.fit(x + shift, st + shift, **kw)
    for u, v in zip(ra, rb):
        close(v["means"] - shift, u["means"], 1e-9)
        close(v["covariances"], u["covariances"], 1e-9)
        close(v["weights"], u["weights"], 1e-9)
        close(v["lower_bound"], u["lower_bound"], 1e-9)
    a = egx.GaussianMixture.fit_wide(x, 3, n_runs=2, init_means=st, **kw)
    b = egx.GaussianMixture.fit_wide(x + shift, 3, n_runs=2, init_means=st + shift, **kw)
    for j in range(2):
        close(b.all_means_[j] - shift, a.all_means_[j])
        close(b.all_covariances_[j], a.all_covariances_[j])
        close(b.all_weights_[j], a.all_weights_[j])
        close(b.lower_bounds_[j], a.lower_bounds_[j])
    assert a.best_run_ == b.best_run_


def test_failed_restarts_are_values_at_width(egx):
    """reg_covar = 0 and a restart whose two initial means are the same row: cluster 1 gets no rows, its covariance is the
    zero matrix, the restart reports status 2 and the other one wins; with every restart built that way the call returns an
    error code (ClusteringError in Python).  A numerical status: nothing faults."""
    x = GO.blobs(400, 40, 2, seed=2)
    dead, live = np.stack([x[0], x[0]]), np.stack([x[0], x[1]])
    st = np.stack([dead, live])
    runs, best = GO.fit(x, st, max_iter=5, tol=0.0, reg_covar=0.0)
    assert [r["status"] for r in runs] == [GO.FAILED, GO.MAX_ITER] and best == 1
    gm = egx.GaussianMixture.fit_wide(x, 2, n_runs=2, max_iter=5, tol=0.0, reg_covar=0.0, init_means=st)
    assert int(gm.statuses_[0]) == GO.FAILED and gm.best_run_ == 1
    check_against_oracle(gm, runs, best)
    with pytest.raises(egx.ClusteringError, match="every restart failed"):
        egx.GaussianMixture.fit_wide(x, 2, n_runs=2, max_iter=5, tol=0.0, reg_covar=0.0, init_means=np.stack([dead, dead]))
    # the same through the C ABI: an error code and a message, the per-restart outputs filled
    L = egx._lib
    lib = L.load()
    cfg = L.GmmConfig()
    lib.egx_gmm_config_default(cfg)
    cfg.n_clusters, cfg.n_runs, cfg.max_iter, cfg.tol, cfg.reg_covar = 2, 2, 5, 0.0, 0.0
    xs, sd = np.ascontiguousarray(x), np.ascontiguousarray(np.stack([dead, dead]))
    w, m, c, lb = np.empty(2), np.empty((2, 40)), np.empty((2, 40, 40)), np.empty(2)
    it, stt, best_c = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), C.c_int32(7)
    rc = lib.egx_gmm_fit_wide(cfg, L.dptr(xs), 400, 40, L.dptr(sd), L.dptr(w), L.dptr(m), L.dptr(c), L.dptr(lb),
                              it.ctypes.data_as(L.c_int32_p), stt.ctypes.data_as(L.c_int32_p), C.byref(best_c), None, None, None)
    assert rc == L.ERR_LINALG and b"every restart failed" in lib.egx_last_error()
    assert list(stt) == [2, 2] and best_c.value == -1 and list(it) == [0, 0]
    # the library still works afterwards
    again = egx.GaussianMixture.fit_wide(x, 2, n_runs=1, max_iter=5, tol=0.0, reg_covar=0.0, init_means=st[1:])
    np.testing.assert_array_equal(again.means, gm.means)


def test_wide_limits_are_errors(egx):
    rng = np.random.default_rng(0)
    with pytest.raises(egx.InvalidValueError, match="dim <= 128"):
        egx.GaussianMixture.fit_wide(rng.random((200, 129)), 2, n_runs=1)
    with pytest.raises(egx.InvalidValueError, match="n_clusters <= 16"):
        egx.GaussianMixture.fit_wide(rng.random((100, 3)), 17, n_runs=1)


def test_plain_c_host_trains_a_wide_mixture(tmp_path):
    """tests/c_host/gmm_wide_driver.c: a C99 program trains a 300 x 40 mixture through egx_gmm_fit_wide."""
    exe = tmp_path / "gmm_wide_driver"
    libdir = os.path.join(ROOT, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c_host", "gmm_wide_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK")
