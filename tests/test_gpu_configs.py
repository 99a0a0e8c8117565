"""Every BASELINE.json configuration at its stated size, against the oracle.

The numpy/scipy oracle needs ~100 s per likelihood at n = 16384, so its outputs at the headline sizes are committed
as data (tests/golden/large_n.json, generated in the build container by tests/golden/make_large_n.py from
oracle/gp_oracle.py, which tests/test_oracle_golden.py pins to the reference's golden vectors).  Inputs are
regenerated here from the same seeds.  Bars: 1e-8 relative on the log-likelihood, 1e-6 relative on predictions
(absolute floor where the reference clamps variances at 0, crates/gp/src/algorithm.rs:278).

  config 2   n = 4096,  d = 8,  sq-exp: the well-posed straight-1e-8 case (oracle run in the test)
  config 3   n = 16384, d = 32, sq-exp and Matern-5/2: likelihood, sigma2, beta, 1000 predictions/variances (fixture);
             theta-gradient at n = 4096 (fixture) and at n = 16384 (two directional central differences)
  config 4   theta sweep at n = 16384: likelihood_batch and the C-ABI sweep (RCCL communicator) on 33 candidates
             incl. not-positive-definite ones; early exit of the failed candidates
  config 5   8 experts x n = 8192, d = 16, predict_var on m = 100 000 points, smooth and hard recombination
"""
import json
import math
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LK_RTOL = 1e-8
PRED_RTOL = 1e-6
KCODE = {"SquaredExponential": 0, "AbsoluteExponential": 1, "Matern32": 2, "Matern52": 3}


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


@pytest.fixture(scope="module")
def large(golden_dir):
    with open(os.path.join(golden_dir, "large_n.json")) as f:
        return json.load(f)


def _data(n, d, seed):
    from egobox_amd import workload
    return workload.make_training_set(n, d, seed=seed)


def _fit_queries(x, d):
    xq = np.random.default_rng(7).random((1000, d))
    xq[:100] = x[:100]
    xq[100:200] = x[100:200] + 1e-4
    return xq


# ------------------------------------------------------------------ config 2
def test_config2_n4096_d8_sqexp_well_posed_straight_bar(egx, O):
    """BASELINE configs[1] shape at a theta where the problem is well posed (oracle min pivot >> sqrt(nugget)): the
    straight 1e-8 / 1e-6 bars, no self-disagreement allowance."""
    n, d = 4096, 8
    x, y = _data(n, d, 42)
    theta = np.full(d, 2.0)
    ref = O.fit_fixed(x, y, theta, corr=O.SQEXP)
    assert np.diag(ref.inner.r_chol).min() > 1e-3
    with egx.GpHandle(x, y, corr=0) as h:
        h.finalize(theta)
        lk, s2 = h.fitted_scalars()
        assert lk == pytest.approx(ref.likelihood, rel=LK_RTOL)
        assert s2 == pytest.approx(ref.inner.sigma2, rel=1e-8)
        xq = np.random.default_rng(3).random((2000, d))
        yp, vp = h.predict_valvar(xq)
        np.testing.assert_allclose(yp, ref.predict(xq), rtol=PRED_RTOL, atol=PRED_RTOL * np.abs(y).max())
        vr = ref.predict_var(xq)
        np.testing.assert_allclose(vp, vr, rtol=PRED_RTOL, atol=1e-9 * ref.inner.sigma2)


# ------------------------------------------------------------------ config 3
@pytest.mark.parametrize("corr", ["SquaredExponential", "Matern52"])
def test_config3_n16384_d32_fit_matches_oracle_fixture(egx, large, corr):
    rec = large[f"fit_n16384_d32_{corr}"]
    n, d = rec["n"], rec["d"]
    x, y = _data(n, d, rec["seed"])
    theta = np.array(rec["theta"])
    assert rec["min_pivot"] > 1e-4  # well posed: the straight bars apply
    with egx.GpHandle(x, y, corr=KCODE[corr]) as h:
        lk0, st0 = h.likelihood(theta)
        assert st0 == 0 and lk0 == pytest.approx(rec["likelihood"], rel=LK_RTOL)
        h.finalize(theta)
        lk, s2 = h.fitted_scalars()
        assert lk == lk0
        assert s2 == pytest.approx(rec["sigma2"], rel=1e-8)
        inner = h.inner(with_chol=False)
        np.testing.assert_allclose(np.ravel(inner["beta"]), rec["beta"], rtol=1e-7, atol=1e-10)
        gam = np.ravel(inner["gamma"])
        assert np.linalg.norm(gam) == pytest.approx(rec["gamma_norm"], rel=1e-6)
        np.testing.assert_allclose(gam[:8], rec["gamma_head"], rtol=1e-5, atol=1e-7 * np.abs(gam).max())
        xq = _fit_queries(x, d)
        yp, vp = h.predict_valvar(xq)
        want_y, want_v = np.array(rec["predict"]), np.array(rec["predict_var"])
        np.testing.assert_allclose(yp, want_y, rtol=PRED_RTOL, atol=PRED_RTOL * np.abs(y).max())
        # variances: relative 1e-6 with an absolute floor of 1e-9 sigma2 (at / next to training points the value is a
        # cancellation 1 - |rt|^2 + |u|^2 ~ 1e-13..1e-8 that the reference clamps at 0)
        np.testing.assert_allclose(vp, want_v, rtol=PRED_RTOL, atol=1e-9 * rec["sigma2"])
        assert np.all(vp >= 0.0)


@pytest.mark.parametrize("corr", ["SquaredExponential", "Matern52"])
def test_config3_theta_gradient_n4096_matches_oracle_fixture(egx, large, corr):
    rec = large[f"grad_n4096_d32_{corr}"]
    x, y = _data(rec["n"], rec["d"], rec["seed"])
    theta = np.array(rec["theta"])
    with egx.GpHandle(x, y, corr=KCODE[corr]) as h:
        lk, g, st = h.likelihood_grad(theta)
    assert st == 0 and lk == pytest.approx(rec["likelihood"], rel=LK_RTOL)
    want = np.array(rec["grad"])
    np.testing.assert_allclose(g, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())


def test_config3_theta_gradient_n16384_matches_oracle_closed_form(egx, large):
    """config 3 proper (n = 16384, d = 32, Matern-5/2, an anisotropic theta): likelihood and ALL 32 gradient components against
    the oracle's closed form (oracle/gp_oracle.py likelihood_grad: R^-1 by LAPACK, tr(R^-1 dR/dtheta_k) dimension by dimension;
    one n^3 CPU job of half an hour, tests/golden/make_large_n.py --only grad16384) at 1e-6 -- SURVEY appendix A.12, the
    objective of algorithm.rs:880-897 -- plus one central difference of the parity-checked likelihood as a cross-check of the
    fixture itself."""
    rec = large["grad_n16384_d32_Matern52"]
    n, d = rec["n"], rec["d"]
    x, y = _data(n, d, rec["seed"])
    theta = np.array(rec["theta"])
    want = np.array(rec["grad"])
    with egx.GpHandle(x, y, corr=3, n_workspaces=2) as h:
        lk, g, st = h.likelihood_grad(theta)
        assert st == 0 and lk == pytest.approx(rec["likelihood"], rel=LK_RTOL)
        np.testing.assert_allclose(g, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
        v = np.random.default_rng(11).standard_normal(d)
        v /= np.linalg.norm(v)
        eps = 1e-4 * theta[0]
        lks, sts = h.likelihood_batch(np.stack([theta + eps * v, theta - eps * v]))
        assert np.all(sts == 0)
        assert float(want @ v) == pytest.approx((lks[0] - lks[1]) / (2 * eps), rel=2e-5, abs=1e-5 * np.linalg.norm(want))


# ------------------------------------------------------------------ config 4
def test_config4_sweep_candidates_n16384(egx, large, arbiter):
    """33 candidates of the theta sweep at size -- 28 rows of theta_sweep_candidates(512, 32) (row 0, the first 13 LHS
    rows, the 14 rows with the smallest sum theta^2) + 5 corner rows -- through likelihood_batch AND the C-ABI sweep
    (egx_sweep_*, one-rank RCCL communicator), against the oracle's likelihoods and statuses:
      * the 28 rows of the sweep are well posed: straight 1e-8 on the likelihood, status 0;
      * all theta = 1e-3 / 1e-4 (R ~ all ones): not positive definite in the oracle and here (status 1, -inf);
      * all theta = 0.01 / 0.02 / 0.03 (the lower-bound corner): cond(R) ~ 1 / nugget -- the oracle's LAPACK factorisation
        happens to go through, but the pivots sit at rounding level, so either outcome is legitimate: status 0 with a
        likelihood within 1e-2 of the oracle's, or status 1."""
    rec = large["sweep_n16384_d32"]
    n, d = rec["n"], rec["d"]
    x, y = _data(n, d, rec["seed"])
    thetas = np.array(rec["thetas"])
    rows = rec["rows"]
    np.testing.assert_array_equal(thetas[:len(rows)], egx.theta_sweep_candidates(512, d)[rows])
    want_st = np.array(rec["status"])
    want_lk = np.array([np.nan if v is None else v for v in rec["likelihood"]])
    assert len(want_st) == len(thetas) == len(rows) + rec["n_extra"], "fixture incomplete: rerun make_large_n.py --only sweep"
    well = np.arange(len(thetas)) < len(rows)
    corner = ~well & (want_st == 0)
    bad = ~well & (want_st == 1)
    assert np.all(want_st[well] == 0) and bad.sum() == 2 and corner.sum() == 3

    def check(lk, st):
        np.testing.assert_array_equal(st[well], 0)
        np.testing.assert_allclose(lk[well], want_lk[well], rtol=LK_RTOL)
        for i in np.flatnonzero(bad):
            # all theta = 1e-3 / 1e-4: R = (all ones) - O(1e-5 .. 1e-7) + nugget.  In exact arithmetic it is positive definite
            # (the arbiter factors it); in double the accumulated rounding of 16384-term dot products is of the size of
            # the nugget, so whether every pivot stays positive depends on the summation order.  LAPACK (the reference's
            # answer: an error, i.e. +inf) fails; the HIP path may fail too, or get through -- then its likelihood has to
            # be near the extended-precision value.
            assert st[i] in (0, 1)
            if st[i] == 1:
                assert np.isneginf(lk[i])
            else:
                truth = arbiter.get(f"sweep_extra_n16384_d32_theta_{thetas[i][0]}")
                assert truth is not None and truth["truth_status"] == 0
                print(f"theta {thetas[i][0]}: LAPACK not positive definite, HIP {lk[i]!r}, long double {truth['truth_likelihood']!r}")
                assert lk[i] == pytest.approx(truth["truth_likelihood"], rel=5e-2)
        for i in np.flatnonzero(corner):
            # all theta = 0.01 / 0.02 / 0.03: cond(R) ~ 1 / nugget, LAPACK gets through with pivots near rounding level.
            # The extended-precision arbiter says how far LAPACK itself is from the exact value; the HIP path has to be
            # within 10x of that distance (or 1e-8), or report not positive definite.
            assert st[i] in (0, 1)
            if st[i] == 0:
                truth = arbiter[f"sweep_extra_n16384_d32_theta_{thetas[i][0]}"]["truth_likelihood"]
                lap_err = abs(want_lk[i] - truth) / abs(truth)
                gpu_err = abs(lk[i] - truth) / abs(truth)
                print(f"corner theta {thetas[i][0]}: long double {truth!r}; LAPACK rel err {lap_err:.2e}, HIP rel err {gpu_err:.2e}")
                assert gpu_err <= max(LK_RTOL, 10.0 * lap_err)
            else:
                assert np.isneginf(lk[i])

    with egx.GpHandle(x, y, corr=0, n_workspaces=2) as h:
        lk, st = h.likelihood_batch(thetas)
        check(lk, st)
    with egx.Sweep(x, y, corr=0, rank=0, world=1, id_bytes="new") as sw:
        info = sw.info()
        assert info["rccl_ranks"] == 1 and info["rccl_version"] > 0
        lk2, st2 = sw.likelihood(thetas)
        check(lk2, st2)
        np.testing.assert_array_equal(st2, st)
        np.testing.assert_array_equal(lk2[st == 0], lk[st == 0])  # same kernels, same order of operations: bit identical
        assert sw.info()["n_allgathers"] == 1
        got = sw.allgather(np.arange(5.0))
        np.testing.assert_array_equal(got, np.arange(5.0)[None, :])


def test_config4_all_512_rows_n16384(egx, large):
    """BASELINE config 4 in full: the 512 log-uniform rows of theta_sweep_candidates(512, 32) (the reference's multistart
    points, crates/gp/src/optimization.rs:49-66) at n = 16384 through the C-ABI sweep with 24 candidates in flight as
    three lock-step groups of eight (a handle of that shape factors left-looking over its panel groups): the 28 rows the
    oracle fixture holds at 1e-8, every other row a finite likelihood with status 0 or (-inf, not positive definite); the
    best row is the fixture's."""
    rec = large["sweep_n16384_d32"]
    n, d = rec["n"], rec["d"]
    x, y = _data(n, d, rec["seed"])
    rows = np.array(rec["rows"])
    cands = egx.theta_sweep_candidates(512, d)
    np.testing.assert_array_equal(np.array(rec["thetas"])[:len(rows)], cands[rows])
    want_lk = np.array([np.nan if v is None else v for v in rec["likelihood"]])[:len(rows)]
    with egx.Sweep(x, y, corr=0, rank=0, world=1, id_bytes="new", n_workspaces=24) as sw:
        assert sw.set_lockstep(0) == 8
        t0 = time.perf_counter()
        lk, st = sw.likelihood(cands)
        dt = time.perf_counter() - t0
    print(f"config 4: 512 evaluations in {dt:.2f} s = {512 / dt:.1f} per second; statuses {np.bincount(st)}")
    np.testing.assert_array_equal(st[rows], 0)
    np.testing.assert_allclose(lk[rows], want_lk, rtol=LK_RTOL)
    ok = st == 0
    assert np.all(np.isin(st, (0, 1))) and np.all(np.isfinite(lk[ok])) and np.all(np.isneginf(lk[~ok]))
    assert ok.sum() >= 500
    assert int(np.argmax(np.where(ok, lk, -np.inf))) == int(rows[np.argmax(want_lk)]) or lk.max() >= want_lk.max()


def test_config4_failed_candidate_exits_early(egx):
    """algorithm.rs:893-896: a failed Cholesky is +inf at once.  Every kernel of the factorisation returns on entry
    once the pivot flag is set, so a not-positive-definite candidate at n = 16384 costs a small fraction of a
    regular evaluation (negative nugget: the first pivot block already fails)."""
    n, d = 16384, 32
    x, y = _data(n, d, 42)
    theta = egx.workload.default_theta(d)
    with egx.GpHandle(x, y, corr=0) as good, egx.GpHandle(x, y, corr=0, nugget=-0.9) as bad:
        good.likelihood(theta)
        bad.likelihood(theta)
        t0 = time.perf_counter()
        for _ in range(3):
            lk, st = good.likelihood(theta)
        t_good = (time.perf_counter() - t0) / 3
        assert st == 0
        t0 = time.perf_counter()
        for _ in range(3):
            lk, st = bad.likelihood(theta)
        t_bad = (time.perf_counter() - t0) / 3
        assert st == 1 and lk == -math.inf
        print(f"n=16384 evaluation: ok {t_good * 1e3:.2f} ms, not positive definite {t_bad * 1e3:.2f} ms")
        assert t_bad < 0.25 * t_good
        assert t_bad < 4e-3


def test_sweep_c_host_drives_the_collective(tmp_path):
    """tests/c_host/sweep_driver.c: a C99 host (no Python) creates the one-rank sweep with a fresh RCCL unique id
    through the C ABI and checks egx_sweep_likelihood against egx_gp_likelihood_batch."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "sweep_driver"
    libdir = os.path.join(root, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(root, 'include')}",
                    os.path.join(root, "tests", "c_host", "sweep_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK"), out.stdout  # RCCL's version banner goes to stderr (sweep.hip)


def test_sweep_dynamic_assignment_gives_the_static_results(egx):
    """egx_sweep_set_assignment(1): candidates are pulled from the node-wide counter instead of the c mod world shard.
    On one rank the counter is process-local; the results must be those of the static assignment bit for bit, call after
    call (the counter slots rotate), NaN thetas included, and the balance report must account for every candidate."""
    x, y = _data(900, 5, 3)
    thetas = egx.theta_sweep_candidates(13, 5, seed=2)
    thetas[4] = np.nan
    with egx.Sweep(x, y, corr=0, rank=0, world=1, id_bytes="new", n_workspaces=4) as sw:
        lk0, st0 = sw.likelihood(thetas)
        assert st0[4] == egx._lib.STATUS_NAN_THETA and (st0 == 0).sum() >= 8
        sw.set_assignment(True)
        for _ in range(70):  # more calls than counter slots (64): the slots are recycled
            lk1, st1 = sw.likelihood(thetas[:5])
            np.testing.assert_array_equal(st1, st0[:5])
            np.testing.assert_array_equal(lk1[st1 == 0], lk0[:5][st0[:5] == 0])
        lk1, st1 = sw.likelihood(thetas)
        np.testing.assert_array_equal(st1, st0)
        np.testing.assert_array_equal(lk1[st1 == 0], lk0[st0 == 0])
        per, sec = sw.last_balance()
        assert per.tolist() == [13] and sec > 0.0
        sw.set_assignment(False)
        lk2, st2 = sw.likelihood(thetas)
        np.testing.assert_array_equal(lk2[st2 == 0], lk0[st0 == 0])


def _two_rank_worker(rank, token, q):
    """One rank of a world = 2 sweep on the ONE GPU of the test box (host transport, see sweep.hip)."""
    os.environ["EGX_SWEEP_TRANSPORT"] = "shm"
    os.environ["EGX_SWEEP_TIMEOUT_S"] = "8"
    import numpy as np
    import egobox_amd as egx
    from egobox_amd import workload
    x, y = workload.make_training_set(900, 5, seed=3)
    thetas = egx.theta_sweep_candidates(14, 5, seed=2)
    thetas[4] = np.nan
    thetas[9] = 1e-4  # R ~ all ones: kept positive definite by its nugget alone
    out = {}
    sw = egx.Sweep(x, y, corr=0, device=0, rank=rank, world=2, id_bytes=token, n_workspaces=4)
    try:
        out["info"] = sw.info()
        out["static"] = sw.likelihood(thetas)
        out["balance_static"] = sw.last_balance()[0].tolist()
        sw.set_assignment(True)
        out["dynamic"] = [sw.likelihood(thetas) for _ in range(3)][-1]
        out["balance_dynamic"] = sw.last_balance()[0].tolist()
        sw.set_assignment(False)
        out["allgather"] = sw.allgather(np.arange(5.0) + 10.0 * rank)
        # the mixture recombination sharded over the two ranks (expert e on rank e mod 2), both recombinations
        from egobox_amd.moe import GaussianMixture, GpMixture
        experts = []
        for e in range(3):
            xe, ye = workload.make_training_set(400, 2, seed=20 + e)
            experts.append(egx.GaussianProcess.params(egx.ConstantMean(), egx.Matern52Corr())
                           .theta_tuning(egx.ThetaTuning.Fixed([1.2, 0.9])).fit(xe, ye) if e % 2 == rank else None)
        gmx = GaussianMixture([0.3, 0.3, 0.4], [[0.2, 0.5], [0.5, 0.5], [0.8, 0.5]], [np.eye(2) * 0.05] * 3, 0.8)
        xq = np.random.default_rng(2).random((333, 2))
        for recomb in ("smooth", "hard"):
            mixr = GpMixture(experts, gmx, recomb, rank=rank, world=2, sweep=sw)
            out["moe_" + recomb] = mixr.predict_valvar(xq)
            out["moe_grad_" + recomb] = mixr.predict_valvar_gradients(xq[:100])  # egx_moe_predict_valvar_gradients, sharded
        for e in experts:
            if e is not None:
                e.close()
        # the tuned fit with its five starts sharded over the two ranks (egx_sweep_fit), then predictions on the replica
        starts = egx.theta_sweep_candidates(5, 5, seed=11)
        out["fit_evals"] = sw.fit(starts, [1e-2], [1e1], max_eval=60)
        mdl = sw.model()
        out["fit"] = ({k_: v for k_, v in mdl.inner().items() if k_ in ("theta", "likelihood", "sigma2", "beta", "gamma")},
                      mdl.predict_valvar(x[:50] + 0.01))
        # a LOCAL failure on rank 1 only (its theta matrix has one column too many): both ranks must come back
        bad = thetas if rank == 0 else np.hstack([thetas, thetas[:, :1]])
        try:
            lk, st = sw.likelihood(bad, raise_on_peer_failure=False)
            out["fail"] = ("returned", lk, st, egx._lib.load().egx_last_error().decode())
        except egx.EgxError as e:
            out["fail"] = (type(e).__name__, e.rc, str(e))
        out["after"] = sw.likelihood(thetas)  # the collective completed on both ranks: the sweep is still usable
        if rank == 0:  # rank 1 never arrives at this call: the deadline (8 s) must end it
            import time
            t0 = time.time()
            try:
                sw.likelihood(thetas)
                out["deadline"] = ("returned", time.time() - t0)
            except egx.EgxError as e:
                out["deadline"] = (type(e).__name__, e.rc, time.time() - t0)
    finally:
        q.put((rank, out))
        sw.close()


@pytest.mark.timeout(300)
def test_sweep_two_ranks_share_one_gpu_through_the_host_transport(egx):
    """The world > 1 logic of csrc/sweep.hip EXECUTED on the one-GPU box: two processes, both on GPU 0, rendezvous
    through the shared-memory segment (EGX_SWEEP_TRANSPORT=shm: RCCL refuses two ranks on one device; the payload and
    everything around the all-gather are the product's).  Static and dynamic assignment return the single-process
    results bit for bit on both ranks; a rank that fails locally still arrives (the survivor gets EGX_ERR_PEER with the
    failed rank's candidates marked, its own valid); a rank that never arrives is given up after the deadline."""
    import torch.multiprocessing as mp
    x, y = _data(900, 5, 3)
    thetas = egx.theta_sweep_candidates(14, 5, seed=2)
    thetas[4] = np.nan
    thetas[9] = 1e-4
    with egx.GpHandle(x, y, corr=0, n_workspaces=4) as h:
        ref_lk, ref_st = h.likelihood_batch(thetas)
    assert ref_st[4] == egx._lib.STATUS_NAN_THETA
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    token = os.urandom(128)
    procs = [ctx.Process(target=_two_rank_worker, args=(r, token, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ok = ref_st == 0
    for r in range(2):
        assert res[r]["info"]["world"] == 2 and res[r]["info"]["rccl_ranks"] == 0
        for mode in ("static", "dynamic", "after"):
            lk, st = res[r][mode]
            np.testing.assert_array_equal(st, ref_st)
            np.testing.assert_array_equal(lk[ok], ref_lk[ok])
        assert res[r]["balance_static"] == [7, 7]
        assert sum(res[r]["balance_dynamic"]) == 14 and min(res[r]["balance_dynamic"]) >= 1
        np.testing.assert_array_equal(res[r]["allgather"], [[0, 1, 2, 3, 4], [10, 11, 12, 13, 14]])
    print("dynamic balance:", res[0]["balance_dynamic"])
    # the sharded mixture against the same three experts in this process
    from egobox_amd.moe import GaussianMixture, GpMixture
    experts = []
    for e in range(3):
        xe, ye = _data(400, 2, 20 + e)
        experts.append(egx.GaussianProcess.params(egx.ConstantMean(), egx.Matern52Corr())
                       .theta_tuning(egx.ThetaTuning.Fixed([1.2, 0.9])).fit(xe, ye))
    gmx = GaussianMixture([0.3, 0.3, 0.4], [[0.2, 0.5], [0.5, 0.5], [0.8, 0.5]], [np.eye(2) * 0.05] * 3, 0.8)
    xq = np.random.default_rng(2).random((333, 2))
    for recomb in ("smooth", "hard"):
        want = GpMixture(experts, gmx, recomb).predict_valvar(xq)
        for r in range(2):
            np.testing.assert_allclose(res[r]["moe_" + recomb][0], want[0], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(res[r]["moe_" + recomb][1], want[1], rtol=1e-12, atol=1e-14)
        np.testing.assert_array_equal(res[0]["moe_" + recomb][0], res[1]["moe_" + recomb][0])  # the same bits on both ranks
        wantg = GpMixture(experts, gmx, recomb).predict_valvar_gradients(xq[:100])
        for r in range(2):
            for q in range(2):
                np.testing.assert_allclose(res[r]["moe_grad_" + recomb][q], wantg[q], rtol=1e-10,
                                           atol=1e-12 * max(1.0, np.abs(wantg[q]).max()))
        for q in range(2):
            np.testing.assert_array_equal(res[0]["moe_grad_" + recomb][q], res[1]["moe_grad_" + recomb][q])
    for e in experts:
        e.close()
    # the sharded tuned fit IS the one-GPU tuned fit: same evaluations, same theta, same predictions, bit for bit, on both ranks
    starts = egx.theta_sweep_candidates(5, 5, seed=11)
    with egx.GpHandle(x, y, corr=0, n_workspaces=4) as h:
        ne = h.fit(starts, [1e-2], [1e1], max_eval=60)
        want_sc, want_pred = h.inner(), h.predict_valvar(x[:50] + 0.01)
    for r in range(2):
        assert res[r]["fit_evals"] == ne
        got_sc, got_pred = res[r]["fit"]
        for key in ("theta", "likelihood", "sigma2", "beta", "gamma"):
            np.testing.assert_array_equal(np.asarray(got_sc[key]), np.asarray(want_sc[key]))
        np.testing.assert_array_equal(got_pred[0], want_pred[0])
        np.testing.assert_array_equal(got_pred[1], want_pred[1])
    # the failing rank reports ITS error, the survivor a peer error with the survivors' candidates intact
    assert res[1]["fail"][0] == "InvalidValueError"
    kind, lk, st, msg = res[0]["fail"]
    assert kind == "returned" and "rank 1 failed" in msg
    mine = np.arange(14) % 2 == 0
    np.testing.assert_array_equal(st[mine], ref_st[mine])
    np.testing.assert_array_equal(lk[mine & ok], ref_lk[mine & ok])
    assert np.all(st[~mine] == egx._lib.STATUS_RANK_FAILED) and np.all(np.isneginf(lk[~mine]))
    kind, rc, waited = res[0]["deadline"]
    assert kind == "PeerError" and rc == egx._lib.ERR_PEER and 6.0 < waited < 40.0


def test_sweep_fit_on_one_rank_is_the_handle_fit(egx):
    """egx_sweep_fit with world = 1 (a one-rank RCCL communicator): the same machines, evaluations and fitted model as
    egx_gp_fit; more starts than workspaces, a trend with p > 1 and a Matern kernel."""
    x, y = _data(700, 3, 5)
    starts = egx.theta_sweep_candidates(7, 3, seed=4)
    with egx.GpHandle(x, y, mean=1, corr=3, n_workspaces=3) as h:
        ne = h.fit(starts, [1e-2], [1e1], max_eval=40)
        want_sc, want_pred = h.inner(), h.predict_valvar(x[:40] * 0.99)
    with egx.Sweep(x, y, mean=1, corr=3, device=0, rank=0, world=1, id_bytes="new", n_workspaces=3) as sw:
        assert sw.fit(starts, [1e-2], [1e1], max_eval=40) == ne
        m = sw.model()
        got_sc, got_pred = m.inner(), m.predict_valvar(x[:40] * 0.99)
        m.close()  # a view: the sweep still owns the handle
        assert sw.model().fitted_scalars()[0] == got_sc["likelihood"]
    for key in ("theta", "likelihood", "sigma2", "beta", "gamma", "ft_qr_r"):
        np.testing.assert_array_equal(np.asarray(got_sc[key]), np.asarray(want_sc[key]))
    np.testing.assert_array_equal(got_pred[0], want_pred[0])
    np.testing.assert_array_equal(got_pred[1], want_pred[1])
    assert ne >= 7 * 25  # every start ran at least GP_COBYLA_MIN_EVAL evaluations


_COEXIST = r"""
import os, sys, json
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["EGX_ROOT"])
import egobox_amd as egx
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
x, y = egx.workload.make_training_set(600, 4, seed=3)
thetas = egx.theta_sweep_candidates(6, 4, seed=1)
t = torch.arange(1024, dtype=torch.float64, device="cuda")
side = torch.cuda.Stream()
with egx.GpHandle(x, y, n_workspaces=2) as h:
    want_lk, want_st = h.likelihood_batch(thetas)
with egx.Sweep(x, y, device=0, rank=0, world=1, id_bytes="new", n_workspaces=2) as sw:
    assert sw.info()["rccl_ranks"] == 1, "the sweep must hold a real RCCL communicator"
    n_ok = 0
    for it in range(100):
        # torch's collective and the library's all-gather in flight together: torch's on a side stream every other
        # round, the library's on its own stream, neither synchronised against the other before both are enqueued
        with torch.cuda.stream(side if it % 2 else torch.cuda.current_stream()):
            a = t * (it + 1)
            work = dist.all_reduce(a, async_op=True)
        if it % 3 == 2:
            got = sw.allgather(np.array([float(it), -float(it)]))
            assert got.shape[-1] == 2 and float(np.ravel(got)[0]) == float(it)
        else:
            lk, st = sw.likelihood(thetas)
            assert np.array_equal(lk, want_lk) and np.array_equal(st, want_st)
        work.wait()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(a, t * (it + 1))
        g = [torch.empty_like(t)]
        dist.all_gather(g, a)
        assert torch.equal(g[0], a)
        n_ok += 1
dist.barrier()
dist.destroy_process_group()
print(json.dumps({"rounds": n_ok}))
"""


@pytest.mark.timeout(600)
def test_library_rccl_communicator_coexists_with_torch_distributed(tmp_path):
    """Round-4 review, item 9: the library's OWN RCCL communicator (dlopen'ed librccl, ncclAllGather on the sweep's
    stream) and torch.distributed's NCCL process group in ONE process on one GPU at world = 1: 100 rounds with a torch
    all-reduce in flight (alternating streams) while the library runs its sharded sweep + all-gather, every result
    checked, both torn down in order.  (bench.py at N > 1 is exactly this process layout.)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EGX_ROOT=root, MASTER_ADDR="127.0.0.1", MASTER_PORT="29647", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "EGX_SWEEP_TRANSPORT"):
        env.pop(k, None)
    script = tmp_path / "coexist.py"
    script.write_text(_COEXIST)
    out = subprocess.run([sys.executable, str(script)], cwd=root, env=env, capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["rounds"] == 100


@pytest.mark.timeout(600)
def test_bench_gpus_2_rehearsal_on_one_gpu():
    """`python bench.py --gpus 2` end to end on the one-GPU box: bench.py starts its two ranks itself, both on GPU 0, the
    library's all-gather goes through the host transport (EGX_SWEEP_TRANSPORT=shm; RCCL refuses two ranks on one device),
    torch.distributed on gloo.  Every statement of the N > 1 path runs: rendezvous, sharded sweep, per-rank times, the
    sharded mixture leg (expert e on rank e mod 2).  The line is marked as a rehearsal and carries no performance claim."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EGX_SWEEP_TRANSPORT="shm")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--sweep-batch", "10", "--in-flight", "4", "--npoints", "2048", "--dim", "6", "--no-cpu-baseline",
                          "--assignment", "dynamic", "--full"], cwd=root, env=env, capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and "rehearsal" in rec and rec["rccl_ranks"] == 0 and rec["assignment"] == "dynamic"
    assert rec["candidates_ok"] == 20 and rec["candidates_failed"] == 0 and len(rec["rank_seconds"]) == 2
    assert sum(rec["last_step_balance"]["candidates_per_rank"]) == 10
    moe = rec["other_configs"]["config5_mixture_8_experts_sharded"]
    assert "error" not in moe and moe["experts_on_rank_0"] == 4 and math.isfinite(moe["checksum"])
    # the sharded mixture is the single-process mixture (bench.py's other_configs at N = 1 prints the same checksum)
    assert moe["checksum"] == pytest.approx(5774.94659384006, rel=1e-9)
    tuned = rec["other_configs"]["tuned_fit_11_starts_sharded"]
    assert "error" not in tuned and tuned["evaluations"] >= 11 * 25 and math.isfinite(tuned["likelihood"])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("how", ["flag", "probe_failure"])
def test_bench_gpus_2_falls_back_to_torch_collective(how):
    """The N > 1 line must survive a library collective that does not work on the driver's node: `--collective torch`
    gathers through torch.distributed around egx_gp_likelihood_batch, and a failed PROBE of the library's all-gather on one
    rank (injected here) switches every rank to that path.  Same likelihood checksum as the library's collective."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EGX_SWEEP_TRANSPORT="shm")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--sweep-batch", "10",
            "--in-flight", "4", "--npoints", "2048", "--dim", "6", "--no-cpu-baseline", "--no-extra-configs"]
    recs = {}
    for name, extra, e in (("library", [], env),
                           ("fallback", ["--collective", "torch"] if how == "flag" else [],
                            env if how == "flag" else dict(env, EGX_BENCH_FAIL_PROBE="1"))):
        out = subprocess.run(base + extra, cwd=root, env=e, capture_output=True, text=True, timeout=280)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        recs[name] = json.loads(lines[0])
    lib, fb = recs["library"], recs["fallback"]
    assert lib["collective"].startswith("library") and fb["collective"].startswith("torch.distributed")
    if how == "probe_failure":
        assert "injected probe failure" in fb["collective"]
    assert fb["n_gpus"] == 2 and fb["candidates_ok"] == 20 and len(fb["rank_seconds"]) == 2
    assert fb["last_step_balance"]["candidates_per_rank"] == [5, 5]
    assert fb["likelihood_checksum"] == lib["likelihood_checksum"]


@pytest.mark.timeout(300)
def test_bench_plain_run_dumps_what_its_last_step_computed(egx, tmp_path):
    """A plain `bench.py --gpus 1` line carries the headline keys and none of the --full legs; --dump-outputs writes the
    last timed step's likelihoods and statuses, which are what likelihood_batch gives for the same seeded candidates."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "EGX_SWEEP_TRANSPORT"):
        env.pop(k, None)
    steps, warmup, nb, n, d = 3, 1, 8, 2048, 6
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                          str(warmup), "--sweep-batch", str(nb), "--in-flight", "4", "--npoints", str(n), "--dim", str(d),
                          "--dump-outputs", str(tmp_path / "dump")], cwd=root, env=env, capture_output=True, text=True,
                         timeout=280)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["metric"] == "gp_fixed_theta_fits_per_sec" and rec["unit"] == "fits/s" and rec["dtype"] == "f64"
    assert rec["higher_is_better"] is True and rec["steps"] == steps and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(nb * 1e3 / rec["ms_per_step"], rel=1e-3)
    assert not {"roofline", "other_configs", "cpu_baseline", "pcie_inclusive", "details"} & set(rec)
    lk = np.load(tmp_path / "dump" / "likelihood.npy")
    st = np.load(tmp_path / "dump" / "status.npy")
    assert lk.dtype == np.float64 and st.dtype == np.float64 and lk.shape == st.shape == (nb,)
    x, y = _data(n, d, 42)
    cands = egx.workload.default_theta(d) * 10.0 ** np.random.default_rng(1234).uniform(-0.15, 0.15,
                                                                                          size=((steps + warmup) * nb, d))
    with egx.GpHandle(x, y, n_workspaces=4) as h:
        want_lk, want_st = h.likelihood_batch(cands[-nb:])
    np.testing.assert_array_equal(st, want_st)
    np.testing.assert_allclose(lk, want_lk, rtol=LK_RTOL)


@pytest.mark.parametrize("k,nx,hf", [(1, 3, 1.0), (2, 1, 1.0), (3, 2, 0.99), (8, 16, 0.9), (8, 16, 0.3), (4, 64, 1.0)])
def test_gmx_responsibilities_on_the_device(k, nx, hf):
    """egx_gmx_predict_probas (one lane per point) against the oracle's GaussianMixture::predict_probas
    (crates/moe/src/gaussian_mixture.rs:114-121, 231-283), including points so far out that every weighted log probability is
    below f64::MIN_10_EXP (the reference then leaves the normaliser at 0, :244-250) and a ragged last workgroup."""
    from egobox_amd.moe import GaussianMixture
    from oracle import moe_oracle as MO
    rng = np.random.default_rng(100 * k + nx)
    means = rng.standard_normal((k, nx)) * 2
    a = rng.standard_normal((k, nx, nx))
    covs = np.einsum("kij,klj->kil", a, a) / nx + 0.5 * np.eye(nx)
    w = rng.random(k) + 0.2
    w /= w.sum()
    x = rng.standard_normal((1000 + 37, nx)) * 3
    x[:5] *= 40.0  # far outside every cluster
    g, go = GaussianMixture(w, means, covs, hf), MO.GaussianMixtureOracle(w, means, covs, hf)
    got = g.predict_probas_device(x)
    want = go.predict_probas(x)
    np.testing.assert_allclose(got, want, rtol=2e-11, atol=1e-300)
    if k > 1:
        np.testing.assert_array_equal(np.argmax(got, axis=1), go.predict(x))
    assert g.predict_probas_device(x[:0]).shape == (0, k)


@pytest.mark.parametrize("k,nx,hf", [(1, 3, 1.0), (2, 1, 1.0), (3, 2, 0.8), (8, 16, 0.9), (5, 40, 1.0)])
def test_gmx_responsibility_derivatives_on_the_device(k, nx, hf):
    """egx_gmx_predict_probas_derivatives (one lane per point) against the oracle's
    GaussianMixture::predict_probas_derivatives (crates/moe/src/gaussian_mixture.rs:127-170) and the numpy form of
    egobox_amd.moe; the rows of every point's (k x nx) block sum to zero over the clusters (the responsibilities sum to 1)."""
    from egobox_amd.moe import GaussianMixture
    from oracle import moe_oracle as MO
    rng = np.random.default_rng(7 * k + nx)
    means = rng.standard_normal((k, nx))
    a = rng.standard_normal((k, nx, nx))
    covs = np.einsum("kij,klj->kil", a, a) / nx + 0.5 * np.eye(nx)
    w = rng.random(k) + 0.2
    w /= w.sum()
    x = rng.standard_normal((200 + 13, nx))
    g, go = GaussianMixture(w, means, covs, hf), MO.GaussianMixtureOracle(w, means, covs, hf)
    got = g.predict_probas_derivatives_device(x)
    want = go.predict_probas_derivatives(x[:40])
    assert got.shape == (x.shape[0], k, nx)
    # (one cluster: the derivative is (u' v - u v') / v^2 with v = u -- zero up to the rounding of the two products)
    scale = max(np.abs(want).max(), 1.0 if k == 1 else 1e-300)
    np.testing.assert_allclose(got[:40], want, rtol=1e-9, atol=1e-12 * scale)
    np.testing.assert_allclose(got, g.predict_probas_derivatives(x), rtol=1e-9, atol=1e-12 * scale)
    np.testing.assert_allclose(got.sum(axis=1), 0.0, atol=1e-10 * scale)
    assert g.predict_probas_derivatives_device(x[:0]).shape == (0, k, nx)


def test_moe_c_host_drives_the_recombination(tmp_path):
    """tests/c_host/moe_driver.c: a C99 host (no Python) trains three experts, then calls egx_moe_predict_valvar -- the
    mixture recombination inside the library -- in both recombinations, single-process and through a one-rank RCCL
    communicator, against crates/moe/src/algorithm.rs:411-423, 670-685, 879-935 applied to the experts' own outputs."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "moe_driver"
    libdir = os.path.join(root, "egobox_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{os.path.join(root, 'include')}",
                    os.path.join(root, "tests", "c_host", "moe_driver.c"), f"-L{libdir}", "-legx_gp_hip", "-lm",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert out.stdout.startswith("OK"), out.stdout


# ------------------------------------------------------------------ config 5
def test_config5_eight_experts_n8192_d16_m100000(egx, large):
    """8 experts x n = 8192, d = 16 (disjoint LHS draws, seeds 7..14), m = 100 000 query points, smooth and hard
    recombination (crates/moe/src/algorithm.rs:670-685, 894-910).  EVERY expert is pinned to the oracle: expert 0 on the
    first 1000 queries, experts 1..7 on the first 100 (likelihood, variance, predictions, variances); both
    recombinations are pinned to the mixture of the eight ORACLE experts on those 100 points, and at m = 100 000 to the
    recombination formulas applied to the experts' own outputs with the oracle's responsibilities (whose pdfs are pinned
    to gaussian_mixture.rs KATs).  The recombination itself runs inside the library (egx_moe_predict_valvar)."""
    from egobox_amd.moe import GaussianMixture, GpMixture
    from oracle import moe_oracle as MO
    rec = large["expert_n8192_d16"]
    n, d, m, k = rec["n"], rec["d"], 100000, 8
    theta = np.array(rec["theta"])
    xq = np.random.default_rng(7).random((m, d))
    # round 6: the eight experts are created as ONE group and fitted in lock-step (GpParams.fit_group -> egx_gp_create_group +
    # egx_gp_finalize_multi: the expert loop of crates/moe/src/algorithm.rs:167-177 as one launch sequence), so every assertion
    # below -- all against the ORACLE experts of large_n.json -- pins the group path at config 5's full size
    sets = [_data(n, d, 7 + e) for e in range(k)]
    experts = (egx.GaussianProcess.params(egx.ConstantMean(), egx.SquaredExponentialCorr())
               .theta_tuning(egx.ThetaTuning.Fixed(theta)).fit_group(np.stack([s_[0] for s_ in sets]), np.stack([s_[1] for s_ in sets])))
    try:
        # ... and one of them once more on its own.  (A lone one-workspace handle of this size factors as ONE flow launch since
        # round 6 -- schedule()["flow"] -- the members of a group in lock-step by separate launches: two rows of csrc/schedule.h,
        # the same sums in another order, 1e-10 apart; the bit-for-bit identity of group and lone fits holds where both take
        # the same row: tests/test_gpu_pipe.py.)
        lone = egx.GaussianProcess.params(egx.ConstantMean(), egx.SquaredExponentialCorr()) \
            .theta_tuning(egx.ThetaTuning.Fixed(theta)).fit(*sets[3])
        try:
            assert lone.handle.schedule()["flow"] == 1 and experts[3].handle.schedule()["flow"] == 0
            assert lone.likelihood() == pytest.approx(experts[3].likelihood(), rel=1e-10)
            assert lone.variance() == pytest.approx(experts[3].variance(), rel=1e-9)
            np.testing.assert_allclose(lone.predict(xq[:64]), experts[3].predict(xq[:64]), rtol=1e-8)
        finally:
            lone.close()
        assert experts[0].likelihood() == pytest.approx(rec["likelihood"], rel=LK_RTOL)
        assert experts[0].variance() == pytest.approx(rec["sigma2"], rel=1e-8)
        # experts 1..7: the oracle's likelihood, variance and 100 predictions each (tests/golden/make_large_n.py --only experts)
        rec17 = large["experts_1_to_7_n8192_d16"]
        mq = rec17["m"]
        for e in range(1, k):
            re_ = rec17["experts"][str(e)]
            assert re_["seed"] == 7 + e
            assert experts[e].likelihood() == pytest.approx(re_["likelihood"], rel=LK_RTOL)
            assert experts[e].variance() == pytest.approx(re_["sigma2"], rel=1e-8)
            ye, ve = experts[e].predict_valvar(xq[:mq])
            np.testing.assert_allclose(ye, re_["predict"], rtol=PRED_RTOL, atol=PRED_RTOL * max(np.abs(re_["predict"]).max(), 1.0))
            np.testing.assert_allclose(ve, re_["predict_var"], rtol=PRED_RTOL, atol=1e-9 * re_["sigma2"])
        t0 = time.perf_counter()
        per_y, per_v = zip(*[e.predict_valvar(xq) for e in experts])
        dt = time.perf_counter() - t0
        print(f"8 experts x predict_valvar(m = {m}): {dt:.2f} s = {k * m / dt / 1e3:.0f} k expert-points/s")
        per_y, per_v = np.array(per_y), np.array(per_v)
        ymax = max(np.abs(per_y).max(), 1.0)
        np.testing.assert_allclose(per_y[0][:1000], rec["predict"], rtol=PRED_RTOL, atol=PRED_RTOL * ymax)
        np.testing.assert_allclose(per_v[0][:1000], rec["predict_var"], rtol=PRED_RTOL, atol=1e-9 * rec["sigma2"])
        assert np.all(np.isfinite(per_v)) and np.all(per_v >= 0.0)
        rng = np.random.default_rng(5)
        w = rng.random(k) + 0.5
        w /= w.sum()
        means = rng.random((k, d))
        covs = np.array([np.eye(d) * 0.3] * k)
        gmo = MO.GaussianMixtureOracle(w, means, covs, 0.9)
        p = gmo.predict_probas(xq)
        c = gmo.predict(xq)
        assert len(np.unique(c)) > 1
        smooth = GpMixture(experts, GaussianMixture(w, means, covs, 0.9), "smooth")
        val, var = smooth.predict_valvar(xq)
        np.testing.assert_allclose(val, (per_y * p.T).sum(axis=0), rtol=1e-9, atol=1e-9 * ymax)
        np.testing.assert_allclose(var, (per_v * p.T * p.T).sum(axis=0), rtol=1e-9, atol=1e-12 * per_v.max())
        # ... and against the mixture of the eight ORACLE experts on the fixture's 100 points (both recombinations)
        mixr = rec17["mixture"]
        np.testing.assert_array_equal(c[:mq], mixr["clusters"])
        np.testing.assert_allclose(val[:mq], mixr["smooth_predict"], rtol=PRED_RTOL, atol=PRED_RTOL * ymax)
        np.testing.assert_allclose(var[:mq], mixr["smooth_predict_var"], rtol=PRED_RTOL, atol=1e-9 * rec["sigma2"])
        hard = GpMixture(experts, GaussianMixture(w, means, covs, 0.9), "hard")
        val_h, var_h = hard.predict_valvar(xq)
        np.testing.assert_allclose(val_h[:mq], mixr["hard_predict"], rtol=PRED_RTOL, atol=PRED_RTOL * ymax)
        np.testing.assert_allclose(var_h[:mq], mixr["hard_predict_var"], rtol=PRED_RTOL, atol=1e-9 * rec["sigma2"])
        rows = np.arange(m)
        # routed subsets run through the same kernels in a different batch composition: values agree to rounding
        np.testing.assert_allclose(val_h, per_y[c, rows], rtol=1e-9, atol=1e-9 * ymax)
        np.testing.assert_allclose(var_h, per_v[c, rows], rtol=1e-7, atol=1e-10 * per_v.max())
    finally:
        for e in experts:
            e.close()


@pytest.mark.parametrize("eps_col", [1e-8, 1e-10, 1e-12, 1e-13, 1e-15, 0.0])
def test_nearly_collinear_trend_is_decided_as_the_reference_decides(egx, O, eps_col):
    """algorithm.rs:1010-1027: the fit fails when sigma_min / sigma_max of the p x p QR factor of ft drops below 1e-10.
    A Linear trend whose last two input columns agree to eps_col makes ft that ill conditioned.  The device GLS route
    (Gram matrix, normal equations) may only be taken with margin -- the singular values of the factor are computed
    exactly for p <= 64 -- and the status must be the oracle's in every regime (sigma_min / sigma_max of the oracle's
    factor in brackets): comfortably fine (1e-8 [1.5e-4], 1e-10 [1.5e-6]), fine but too ill conditioned for normal
    equations (1e-12 [1.5e-8], 1e-13 [1.5e-9]: the Householder route answers), failed with "ft is too ill conditioned"
    (1e-15) and with "F is too ill conditioned" (0: a duplicated column)."""
    rng = np.random.default_rng(12)
    n, d = 600, 3
    x = rng.random((n, d))
    x[:, 2] = x[:, 1] + eps_col * rng.standard_normal(n)
    y = np.sin(3.0 * x[:, 0]) + 2.0 * x[:, 1] + 0.1 * rng.standard_normal(n)
    theta = np.array([1.0, 0.8, 0.8])
    ref_lk, ref_st = O.likelihood_at(x, y, theta, mean=O.LINEAR, corr=O.MATERN52)
    with egx.GpHandle(x, y, mean=1, corr=3) as h:
        lk, st = h.likelihood(theta)
    print(f"eps_col {eps_col:g}: oracle status {ref_st} lkh {ref_lk!r}; HIP status {st} lkh {lk!r}")
    if eps_col >= 1e-13:
        assert ref_st == 0
    else:
        assert ref_st in (2, 3)
    assert (st == 0) == (ref_st == 0)
    if st == 0:
        # ft = C^-1 F differs between two double-precision factorisations by ~1e-13 relative; along the nearly collinear
        # pair that difference is amplified by sigma_max / sigma_min (~ 1 / (1.5e4 eps_col) here) before it reaches the
        # residual, whatever route solves the least-squares problem: the bar scales with it
        assert lk == pytest.approx(ref_lk, rel=max(1e-8, 3e-12 / (1.5e4 * eps_col)))
    else:
        assert st in (egx._lib.STATUS_ILL_CONDITIONED_F, egx._lib.STATUS_ILL_CONDITIONED_FT) and np.isneginf(lk)


# ------------------------------------------------------------------ device-side GLS for p > 1 trend columns
@pytest.mark.parametrize("mean,d,n", [(1, 32, 3000), (2, 32, 4096), (2, 6, 1500)])
def test_device_gls_matches_host_householder_route(egx, O, mean, d, n):
    """algorithm.rs:1006-1043 with a Linear / Quadratic trend (p = 33 / 561 / 28 columns): the device route (Gram matrix of
    [ft | yt] by split-K MFMA, its Cholesky factor = the QR factor R, beta = R^-1 z, rho and sum rho^2 on the device)
    against the host Householder-QR route on the same factorisation, and against the oracle where it is quick."""
    x, y = _data(n, d, 5)
    y = y + 3.0 * x[:, 0] - 2.0 * x[:, 1] ** 2
    theta = np.full(d, 2.0 / math.sqrt(d))
    res = {}
    for route in ("1", "0"):
        os.environ["EGX_GLS_DEVICE"] = route
        try:
            with egx.GpHandle(x, y, mean=mean, corr=3) as h:
                lk, st = h.likelihood(theta)
                assert st == 0
                h.finalize(theta)
                inner = h.inner()
                xq = np.random.default_rng(1).random((300, d))
                res[route] = (lk, h.fitted_scalars(), np.ravel(inner["beta"]), inner["ft_qr_r"], h.predict(xq),
                              h.predict_var(xq), np.ravel(inner["gamma"]))
        finally:
            os.environ.pop("EGX_GLS_DEVICE", None)
    dev, host = res["1"], res["0"]
    assert dev[0] == pytest.approx(host[0], rel=1e-9)
    assert dev[1][0] == dev[0] and dev[1][1] == pytest.approx(host[1][1], rel=1e-8)
    np.testing.assert_allclose(dev[2], host[2], rtol=1e-6, atol=1e-8 * np.abs(host[2]).max())
    np.testing.assert_allclose(dev[3], host[3], rtol=1e-7, atol=1e-9 * np.abs(host[3]).max())  # R of the QR, positive diagonal
    np.testing.assert_allclose(dev[4], host[4], rtol=PRED_RTOL, atol=PRED_RTOL * np.abs(y).max())
    np.testing.assert_allclose(dev[5], host[5], rtol=1e-5, atol=1e-8 * dev[1][1])
    np.testing.assert_allclose(dev[6], host[6], rtol=1e-5, atol=1e-7 * np.abs(host[6]).max())
    if n <= 3000:
        ref = O.fit_fixed(x, y, theta, mean=("Constant", "Linear", "Quadratic")[mean], corr="Matern52")
        assert dev[0] == pytest.approx(ref.likelihood, rel=LK_RTOL)


def test_device_gls_quadratic_trend_costs_like_the_constant_one(egx):
    """Quadratic mean at d = 32 (p = 561) and n = 16384 -- one likelihood evaluation within 1.2x of
    the Constant-mean time (the host route needed a 16384 x 561 Householder QR per evaluation)."""
    n, d = 16384, 32
    x, y = _data(n, d, 42)
    theta = egx.workload.default_theta(d)
    times = {}
    for mean in (0, 2):
        with egx.GpHandle(x, y, mean=mean, corr=0) as h:
            h.likelihood(theta)
            t0 = time.perf_counter()
            for _ in range(3):
                lk, st = h.likelihood(theta)
            times[mean] = (time.perf_counter() - t0) / 3
            assert st == 0 and np.isfinite(lk)
    print(f"likelihood at n=16384, d=32: constant {times[0] * 1e3:.1f} ms, quadratic (p=561) {times[2] * 1e3:.1f} ms")
    assert times[2] < 1.3 * times[0]


# ------------------------------------------------------------------ theta-gradient with KPLS weights
@pytest.mark.parametrize("corr", range(4))
def test_theta_gradient_with_kpls_weights_vs_finite_differences(egx, corr):
    """dL/dtheta_l through the coefficient table make_coef builds from w_star (correlation_models.rs:97-101 sq-exp,
    :191 abs-exp, :333 / :505 Matern): against central differences of the parity-checked likelihood, and for the
    identity rotation against the plain gradient."""
    rng = np.random.default_rng(40 + corr)
    n, d, hk = 700, 6, 3
    x, y = _data(n, d, 9)
    w = rng.standard_normal((d, hk))
    w /= np.linalg.norm(w, axis=0)
    theta = np.array([0.9, 1.4, 0.6]) * (2.0 if corr in (1, 2, 3) else 1.0)
    with egx.GpHandle(x, y, corr=corr, w_star=w, n_workspaces=2) as h:
        assert h.h == hk
        lk, g, st = h.likelihood_grad(theta)
        assert st == 0 and g.shape == (hk,)
        for l in range(hk):
            e = np.zeros(hk)
            e[l] = 1e-5 * theta[l]
            lks, sts = h.likelihood_batch(np.stack([theta + e, theta - e]))
            assert np.all(sts == 0)
            fd = (lks[0] - lks[1]) / (2 * e[l])
            assert g[l] == pytest.approx(fd, rel=2e-5, abs=1e-6 * np.abs(g).max())
    th6 = np.array([0.5, 0.9, 1.3, 0.7, 1.1, 0.8]) * (2.0 if corr else 1.0)
    with egx.GpHandle(x, y, corr=corr, w_star=np.eye(d)) as hw, egx.GpHandle(x, y, corr=corr) as h0:
        lw, gw, _ = hw.likelihood_grad(th6)
        l0, g0, _ = h0.likelihood_grad(th6)
        assert lw == pytest.approx(l0, rel=1e-12)
        np.testing.assert_allclose(gw, g0, rtol=1e-9, atol=1e-9 * np.abs(g0).max())


def test_lbfgs_fit_with_kpls_weights(egx):
    """egx_gp_fit_lbfgs on a KPLS-reduced model (kpls_dim = 2 of d = 8): ends at a likelihood no worse than the start's
    and with a small projected gradient."""
    x, y = _data(600, 8, 21)
    base = lambda: egx.GaussianProcess.params(egx.ConstantMean(), egx.Matern52Corr()).kpls_dim(2).n_start(0)
    gp = base().optimizer("lbfgs").max_eval(120).fit(x, y)
    th = gp.theta()
    assert th.shape == (2,) and np.all(th >= 1e-2 * (1 - 1e-9)) and np.all(th <= 1e1 * (1 + 1e-9))
    with egx.GpHandle(x, y, corr=3, w_star=gp.handle._w) as h:
        l0, _ = h.likelihood(np.full(2, 0.1))
        l1, g1, st = h.likelihood_grad(th)
        assert st == 0 and l1 == pytest.approx(gp.likelihood(), rel=1e-10) and l1 >= l0
        gx = th * np.log(10.0) * g1
        free = (th > 1e-2 * 1.001) & (th < 1e1 * 0.999)
        assert np.all(np.abs(gx[free]) <= 1e-2 * max(1.0, abs(l1)))
    gp.close()


# ------------------------------------------------------------------ the stream kernel inside egx_potrf, against LAPACK
@pytest.mark.parametrize("n", [5700, 6144, 7050, 14400])
def test_potrf_with_stream_kernel_launches_vs_lapack(egx, n):
    """egx_potrf at sizes whose trailing updates cross the 512-tile threshold of k_gemm_stream (LDS-DMA ring, mid-chunk
    barrier, store-only epilogue; n >= 14336 also takes the groups of four panels): the factor against LAPACK's, and
    L L^T against the matrix.  A kernel-shaped matrix (smooth, decaying off-diagonals) rather than a Wishart one: its
    factor has the wide dynamic range of a correlation matrix."""
    rng = np.random.default_rng(n)
    t = np.sort(rng.random(n)) * 40.0
    spd = np.exp(-np.abs(t[:, None] - t[None, :])) + 1e-3 * np.eye(n)  # Ornstein-Uhlenbeck kernel: well conditioned
    spd = spd[np.ix_(p := rng.permutation(n), p)]
    got, info = egx.potrf(spd)
    assert info == 0
    want = np.linalg.cholesky(spd)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)
    assert np.all(np.triu(got, 1) == 0.0)
    idx = rng.integers(0, n, 300)
    np.testing.assert_allclose((got[idx] @ got.T)[:, idx], spd[np.ix_(idx, idx)], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ round 4: the theta-gradient in lock-step batches
@pytest.mark.parametrize("n,d,corr,nws,width", [
    (600, 5, 0, 4, 4),      # n_pad 640: C^-T C^-1 by the register-staged kernel (n_pad % 256 != 0)
    (1000, 7, 3, 6, 3),     # n_pad 1024: the LDS-DMA stream kernel with per-tile K ranges, two slots
    (1000, 40, 2, 3, 2),    # two output chunks of the trace kernel (d > 32), ragged last slot
    (4200, 6, 3, 5, 4),     # n_pad 4352: several panel groups in the solve, slots of 4 + 1
])
def test_theta_gradient_batch_is_bit_identical_to_single_candidates(egx, n, d, corr, nws, width):
    """egx_gp_likelihood_grad_batch: every candidate gets, bit for bit, the likelihood and the gradient
    egx_gp_likelihood_grad returns for it alone -- whatever the lock-step width, its companions (a NaN theta, a
    candidate that is not positive definite) or the workspace it lands on; and twice the same call gives the same bits
    (the trace kernel's reduction order is fixed)."""
    x, y = _data(n, d, 21)
    rng = np.random.default_rng(5)
    base = egx.workload.default_theta(d) * (3.0 if corr == 0 else 1.5)
    thetas = base * 10.0 ** rng.uniform(-0.15, 0.15, (7, d))
    thetas[2, 0] = np.nan                      # answered at once (algorithm.rs:885-891)
    thetas[4] = 1e-7                           # R = ones + nugget: not positive definite in floating point (if the size allows)
    # (another handle of the SAME shape: the schedule -- hence the bits -- is a property of (size, workspaces, lock-step width),
    #  egx_gp_get_schedule; a one-workspace handle of 4352 columns factors as one chain launch, this one by separate launches)
    with egx.GpHandle(x, y, corr=corr, n_workspaces=nws) as h1:
        h1.set_lockstep(width)
        single = [h1.likelihood_grad(t) for t in thetas]
        again = [h1.likelihood_grad(t) for t in thetas[:2]]
    for a, b in zip(single[:2], again):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    with egx.GpHandle(x, y, corr=corr, n_workspaces=nws) as h:
        h.set_lockstep(width)
        lk, g, st = h.likelihood_grad_batch(thetas)
        lk2, g2, st2 = h.likelihood_grad_batch(thetas[::-1].copy())
    assert st[2] == 4 and lk[2] == -np.inf and np.all(g[2] == 0.0)  # EGX_STATUS_NAN_THETA
    for c in range(7):
        assert st[c] == single[c][2]
        if st[c] != 0:
            assert np.all(g[c] == 0.0)
        else:
            assert lk[c] == single[c][0], (c, lk[c], single[c][0])
            assert np.array_equal(g[c], single[c][1]), (c, np.abs(g[c] - single[c][1]).max())
            assert lk2[6 - c] == lk[c] and np.array_equal(g2[6 - c], g[c])
    ok = [c for c in range(7) if st[c] == 0]
    assert len(ok) >= 5 and all(np.all(np.isfinite(g[c])) and np.abs(g[c]).max() > 0 for c in ok)


@pytest.mark.parametrize("corr,d,kpls", [
    (3, 6, 2),     # Matern 5/2 with KPLS weights: two coefficient columns per dimension (hcols > 1)
    (0, 70, 0),    # squared exponential, more input dimensions than the scalar-row kernels stage (64)
])
def test_fallback_front_end_in_lock_step_is_bit_identical_to_single_candidates(egx, corr, d, kpls):
    """The shapes the batched front end refuses -- Matern with KPLS weights, d > 64 -- build their matrices launch by launch
    (launch_corr_sym, launch_fill_rows) and then share the slot's ONE tail launch: in slots of four (7 candidates, one a NaN
    theta that takes no slot: 4 + 2) every candidate gets the bits of a slot of one, and likelihood_grad_batch the bits of
    likelihood_grad."""
    n = 300
    x, y = _data(n, d, 17)
    rng = np.random.default_rng(60 + corr)
    w = None
    if kpls:
        w = rng.standard_normal((d, kpls))
        w /= np.linalg.norm(w, axis=0)
        base = np.array([1.8, 2.8])
    else:
        base = egx.workload.default_theta(d) * 3.0
    thetas = base * 10.0 ** rng.uniform(-0.15, 0.15, (7, base.size))
    thetas[3, 0] = np.nan
    with egx.GpHandle(x, y, corr=corr, w_star=w, n_workspaces=4) as h:
        assert h.set_lockstep(1) == 1
        ref_lk, ref_st = h.likelihood_batch(thetas)
        single = [h.likelihood_grad(t) for t in thetas]
        assert h.set_lockstep(4) == 4
        lk, st = h.likelihood_batch(thetas)
        lkg, g, stg = h.likelihood_grad_batch(thetas)
    ok = np.arange(7) != 3
    assert ref_st[3] == egx._lib.STATUS_NAN_THETA and np.all(ref_st[ok] == 0)
    np.testing.assert_array_equal(st, ref_st)
    np.testing.assert_array_equal(lk, ref_lk)      # bit identical (-inf for the NaN theta in both)
    np.testing.assert_array_equal(stg, ref_st)
    np.testing.assert_array_equal(lkg, ref_lk)
    for c in range(7):
        assert single[c][2] == ref_st[c] and (single[c][0] == ref_lk[c])
        np.testing.assert_array_equal(g[c], single[c][1])
    assert all(np.all(np.isfinite(g[c])) and np.abs(g[c]).max() > 0 for c in range(7) if ok[c]) and np.all(g[3] == 0.0)


def test_lockstep_width_is_clamped_to_what_one_launch_takes(egx):
    """egx_gp_set_lockstep clamps the width to min(n_workspaces, 16): a request for 20 on 20 workspaces gives slots of 16 + 4,
    the handle reports what runs (width and schedule as after a request for 16), and 40 candidates -- 16 + 4, 16 + 4 -- get the
    bits of slots of one, likelihoods and theta-gradients."""
    n, d = 200, 3
    x, y = _data(n, d, 5)
    rng = np.random.default_rng(12)
    thetas = 4.0 * 10.0 ** rng.uniform(-0.2, 0.2, (40, d))  # (short correlation lengths: every R well conditioned)
    with egx.GpHandle(x, y, corr=0, n_workspaces=20) as h:
        assert h.set_lockstep(1) == 1
        ref_lk, ref_st = h.likelihood_batch(thetas)
        ref_lkg, ref_g, ref_stg = h.likelihood_grad_batch(thetas)
        assert h.set_lockstep(16) == 16
        sched16 = h.schedule()
        assert h.set_lockstep(20) == 16
        assert h.schedule() == sched16
        lk, st = h.likelihood_batch(thetas)
        lkg, g, stg = h.likelihood_grad_batch(thetas)
    assert np.all(ref_st == 0) and np.all(ref_stg == 0)
    np.testing.assert_array_equal(st, ref_st)
    np.testing.assert_array_equal(lk, ref_lk)
    np.testing.assert_array_equal(stg, ref_stg)
    np.testing.assert_array_equal(lkg, ref_lkg)
    np.testing.assert_array_equal(g, ref_g)
    np.testing.assert_array_equal(lkg, lk)
    assert np.all(np.isfinite(g)) and np.all(np.abs(g).max(axis=1) > 0)


def test_theta_gradient_batch_matches_oracle_and_keeps_a_fitted_model(egx, O):
    """The batch against the oracle's closed form (gp_oracle.likelihood_grad), on a FITTED handle: with more than one
    workspace the fit stays in workspace 0 and predictions are unchanged afterwards."""
    n, d = 500, 4
    x, y = _data(n, d, 8)
    theta0 = np.array([0.9, 1.2, 0.7, 1.5])
    rng = np.random.default_rng(1)
    thetas = theta0 * 10.0 ** rng.uniform(-0.2, 0.2, (5, d))
    xq = rng.random((50, d))
    with egx.GpHandle(x, y, corr=3, n_workspaces=3) as h:
        h.finalize(theta0)
        before = h.predict_valvar(xq)
        lk, g, st = h.likelihood_grad_batch(thetas)
        after = h.predict_valvar(xq)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for c in range(5):
        lk_ref, g_ref = O.likelihood_grad(x, y, thetas[c], corr="Matern52")
        assert st[c] == 0 and lk[c] == pytest.approx(lk_ref, rel=LK_RTOL)
        np.testing.assert_allclose(g[c], g_ref, rtol=1e-6, atol=1e-6 * np.abs(g_ref).max())


def test_lbfgs_starts_in_lock_step_walk_their_own_trajectories(egx):
    """egx_gp_fit_lbfgs advances all starts through one likelihood + gradient batch per round: the fitted model is the
    one the best start reaches alone (each start sees exactly the evaluations it would see alone)."""
    n, d = 400, 3
    x, y = _data(n, d, 3)
    starts = np.array([[0.3, 0.3, 0.3], [2.0, 0.5, 1.0], [0.05, 4.0, 0.7]])
    lo, hi = [1e-3], [50.0]
    fits = []
    for s in range(3):
        with egx.GpHandle(x, y, corr=0, n_workspaces=1) as h:
            ne = h.fit_lbfgs(starts[s:s + 1], lo, hi, max_iter=30)
            inner = h.inner()
            fits.append((inner["likelihood"], inner["theta"].copy(), ne))
    with egx.GpHandle(x, y, corr=0, n_workspaces=3) as h:
        ne = h.fit_lbfgs(starts, lo, hi, max_iter=30)
        best = int(np.argmax([f[0] for f in fits]))
        assert ne == sum(f[2] for f in fits)
        inner = h.inner()
        assert inner["likelihood"] == fits[best][0]
        assert np.array_equal(inner["theta"], fits[best][1])


def test_left_looking_handles_candidates_do_not_depend_on_their_companions(egx):
    """Round 4: a handle with a padded n >= 14336 and a lock-step width >= 8 factors LEFT-looking over its panel groups
    (kernels_chol.hip launch_potrf).  The schedule belongs to the handle, not to a launch: a candidate gets the same bits
    alone (a group of one), in a full group of eight and in a ragged group, next to a NaN theta and a candidate that is not
    positive definite; and the left-looking likelihoods are the right-looking ones to rounding (the same sums in another
    order)."""
    n, d = 14400, 8
    x, y = _data(n, d, 3)
    rng = np.random.default_rng(8)
    thetas = egx.workload.default_theta(d) * 3.0 * 10.0 ** rng.uniform(-0.1, 0.1, (11, d))
    thetas[2, 1] = np.nan
    thetas[6] = 1e-4  # R ~ all ones: not positive definite (or at rounding level)
    with egx.GpHandle(x, y, corr=0, n_workspaces=16) as h:
        assert h.set_lockstep(0) == 8
        lk, st = h.likelihood_batch(thetas)                       # 8 + 2 (the NaN takes no slot)
        alone = [h.likelihood_batch(thetas[c:c + 1]) for c in range(11)]
        lk3, st3 = h.likelihood_batch(thetas[[9, 0, 4]])          # other companions, other slots
        prev = egx.set_tuning("potrf_left", 0)
        try:
            # (round 5: a handle's schedule is decided when it is created or its lock-step width is set, schedule.h:
            #  setting the width again re-decides it under the changed knob)
            assert h.schedule()["left_looking"] == 1
            h.set_lockstep(0)
            assert h.schedule()["left_looking"] == 0
            lk_r, st_r = h.likelihood_batch(thetas)               # the same handle, right-looking
        finally:
            egx.set_tuning("potrf_left", prev)
            h.set_lockstep(0)
        assert h.schedule()["left_looking"] == 1
        # the theta-gradient on a left-looking handle (C^-T rides along the left-looking schedule) against the same
        # candidates on a right-looking one-workspace handle
        lkg, gg, stg = h.likelihood_grad_batch(thetas[[0, 1, 4, 5]])
    singles = []
    with egx.GpHandle(x, y, corr=0, n_workspaces=1) as h1:
        for q, c in enumerate((0, 1, 4, 5)):
            l1, g1, s1 = h1.likelihood_grad(thetas[c])
            singles.append((l1, g1))
            assert s1 == 0 and stg[q] == 0 and lkg[q] == lk[c]
            assert l1 == pytest.approx(lkg[q], rel=1e-9)
            np.testing.assert_allclose(gg[q], g1, rtol=1e-6, atol=1e-7 * np.abs(g1).max())
    # a lock-step width of four: right-looking factorisation, but the C^-T rider updates LEFT-looking (w_left_for): the same
    # products as the right-looking rider, in the same order where every group is 1024 columns wide (n = 16384: identical bits,
    # profiles/r04_run12_*); here the last group is 256 wide and its right-looking update is another kernel's -- equal to
    # rounding.  Round 6: the one-workspace handle hands its last columns to a flow launch (schedule.h flow_tail, slot 6 of
    # egx_gp_get_schedule = 2), another order of the same sums -- the likelihoods agree to rounding, no longer bit for bit; on one
    # handle a candidate still gets the same bits whatever its companions
    with egx.GpHandle(x, y, corr=0, n_workspaces=4) as h4:
        assert h4.set_lockstep(0) == 4
        lk4, g4, st4 = h4.likelihood_grad_batch(thetas[[0, 1, 4, 5]])
        lk4b, g4b, st4b = h4.likelihood_grad_batch(thetas[[5, 0]])
        assert lk4b[0] == lk4[3] and lk4b[1] == lk4[0]
        np.testing.assert_array_equal(g4b[0], g4[3])
        for q in range(4):
            assert st4[q] == 0 and lk4[q] == pytest.approx(singles[q][0], rel=1e-10)
            np.testing.assert_allclose(g4[q], singles[q][1], rtol=1e-6, atol=1e-7 * np.abs(singles[q][1]).max())
    assert st[2] == 4 and st[6] in (0, 1)
    for c in range(11):
        assert alone[c][1][0] == st[c]
        if st[c] == 0:
            assert alone[c][0][0] == lk[c]
    assert lk3[0] == lk[9] and lk3[1] == lk[0] and lk3[2] == lk[4]
    ok = (st == 0) & (st_r == 0) & (np.arange(11) != 6)
    assert ok.sum() == 9
    np.testing.assert_allclose(lk[ok], lk_r[ok], rtol=1e-10)
    assert np.any(lk[ok] != lk_r[ok])  # (it IS another order of operations: if this ever fails the knob does nothing)


def test_sweep_counter_slots_survive_any_mix_of_static_and_dynamic_calls(egx):
    """the node-wide candidate counter of call s lives in slot s mod 64 and is zeroed half a ring ahead.  The
    sequence number advances on EVERY call, so the slot must be recycled on every call too: 40 dynamic calls, 30 static
    ones, then dynamic again used to find a dirty counter (every rank pulled nothing -> a spurious EGX_ERR_PEER)."""
    n, d = 300, 3
    x, y = _data(n, d, 4)
    thetas = egx.theta_sweep_candidates(9, d, seed=2)
    with egx.Sweep(x, y, corr=0, rank=0, world=1, id_bytes="new", n_workspaces=3) as sw:
        want = sw.likelihood(thetas)
        for dynamic, calls in ((True, 40), (False, 30), (True, 70), (False, 5), (True, 70)):
            sw.set_assignment(dynamic)
            for _ in range(calls):
                lk, st = sw.likelihood(thetas)
                np.testing.assert_array_equal(st, want[1])
                np.testing.assert_array_equal(lk, want[0])


@pytest.mark.parametrize("corr", [0, 1])
def test_huge_theta_gives_the_identity_correlation_not_nan(egx, corr):
    """with theta = 1e8 (1e160: the exponent's sum overflows to +inf) every off-diagonal correlation underflows to
    0, R = (1 + nugget) I and the reference returns a perfectly good likelihood; the fast exp of the correlation kernels
    clamps its argument instead of turning -inf into NaN."""
    import warnings
    from oracle import gp_oracle as O
    x, y = _data(300, 3, seed=2)
    for th in (1e8, 1e160):
        theta = np.full(3, th)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = O.fit_fixed(x, y, theta, corr=["SquaredExponential", "AbsoluteExponential"][corr])
        with egx.GpHandle(x, y, corr=corr) as h:
            lk, st = h.likelihood(theta)
            assert st == 0 and lk == pytest.approx(ref.likelihood, rel=LK_RTOL)
            h.finalize(theta)
            xq = np.random.default_rng(1).random((20, 3))
            np.testing.assert_allclose(h.predict(xq), ref.predict(xq), rtol=PRED_RTOL, atol=1e-9)


def test_theta_gradient_batch_edge_cases(egx):
    """Small and degenerate calls of egx_gp_likelihood_grad_batch: no candidate, one point more than the trend needs, a
    one-dimensional input, a broadcast theta (theta_len = 1), more candidates than workspaces, every kernel."""
    from oracle import gp_oracle as O
    rng = np.random.default_rng(0)
    x = rng.random((37, 2))
    y = np.sin(3 * x[:, 0]) + x[:, 1]
    for corr in range(4):
        with egx.GpHandle(x, y, corr=corr, n_workspaces=3) as h:
            lk, g, st = h.likelihood_grad_batch(np.zeros((0, 2)))
            assert lk.shape == (0,) and g.shape == (0, 2) and st.shape == (0,)
            thetas = 0.5 + rng.random((7, 2))
            lk, g, st = h.likelihood_grad_batch(thetas)
            assert np.all(st == 0)
            for c in (0, 6):
                lr, gr = O.likelihood_grad(x, y, thetas[c], corr=["SquaredExponential", "AbsoluteExponential", "Matern32", "Matern52"][corr])
                assert lk[c] == pytest.approx(lr, rel=LK_RTOL)
                np.testing.assert_allclose(g[c], gr, rtol=1e-6, atol=1e-7 * np.abs(gr).max())
            # broadcast: theta_len = 1 stands for (t, t); the gradient has h = 2 entries and is the full gradient at (t, t)
            lb, gb, sb = h.likelihood_grad_batch(np.array([[0.8], [1.1]]))
            lf, gf, sf = h.likelihood_grad_batch(np.array([[0.8, 0.8], [1.1, 1.1]]))
            assert np.array_equal(lb, lf) and np.array_equal(gb, gf) and gb.shape == (2, 2)
    x1 = np.linspace(0.0, 1.0, 9).reshape(-1, 1)
    y1 = np.cos(4 * x1[:, 0])
    with egx.GpHandle(x1, y1, corr=0) as h:
        lk, g, st = h.likelihood_grad(np.array([2.0]))
        e = 1e-6
        fd = (h.likelihood([2.0 + e])[0] - h.likelihood([2.0 - e])[0]) / (2 * e)
        assert st == 0 and g[0] == pytest.approx(fd, rel=1e-5, abs=1e-7)
