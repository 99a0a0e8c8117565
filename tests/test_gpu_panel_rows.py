"""The row-owning panel solve of the factorisation (k_panel_trsm_rows, csrc/kernels_chol.hip) against the column-strip kernels
it replaces for tall panels (k_panel_trsm16<1> / <2>), as BITS: "trsm_rows_min" = 64 sends every panel below a diagonal block
to the new kernel, a value beyond any n none.  The knob is a launch-time one only because the two give the same bits -- which
is what every test here asserts (np.array_equal on the bit patterns), on the separate-launch path ("pipe" = 0: the chain
launches solve their panels by tasks of their own)."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS_ALL, ROWS_NONE = 64, 1 << 30


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@contextlib.contextmanager
def _separate_launches(egx, rows_min):
    saved = {}
    try:
        saved["pipe"] = egx.set_tuning("pipe", 0)
        saved["trsm_rows_min"] = egx.set_tuning("trsm_rows_min", rows_min)
        yield
    finally:
        for k, v in saved.items():
            egx.set_tuning(k, v)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _potrf_both(egx, a):
    out = []
    for rows_min in (ROWS_ALL, ROWS_NONE):
        with _separate_launches(egx, rows_min):
            out.append(egx.potrf(a))
    return out


@pytest.mark.parametrize("n", [320, 576, 1100])
def test_well_conditioned_factor_has_the_same_bits(egx, n):
    """n = 320: padded 384, a 128-wide last panel (8 strips) and 128 rows under the first block; 576: three panels with 384
    and 128 rows below; 1100: a multiple of nothing.  Tolerances against LAPACK: test_gpu_parity.py::test_potrf_vs_lapack."""
    rng = np.random.default_rng(n)
    g = rng.standard_normal((n, n))
    spd = g @ g.T + n * np.eye(n)
    (new, info_new), (old, info_old) = _potrf_both(egx, spd)
    assert info_new == 0 and info_old == 0
    assert np.array_equal(_bits(new), _bits(old))
    want = np.linalg.cholesky(spd)
    np.testing.assert_allclose(new, want, rtol=1e-11, atol=1e-11 * np.abs(want).max())
    assert np.all(np.triu(new, 1) == 0.0)


def test_ill_conditioned_kernel_matrix_takes_the_refinement_step(egx):
    """exp(-(t_i - t_j)^2 / 0.02) + 1e-10 I on 1024 uniform points of [0, 3] (seed 5): the recipe of tools/trsm_check.hip with
    numpy's generator, cond(L) ~ 5e5, whose 16x16 diagonal tiles are flagged for the refinement step X += (T - X L^T) Linv^T.  That the new
    kernel takes the branch here was confirmed with a scratch build in which k_panel_trsm_rows ignored the flag: this test
    then failed, with 489 337 entries of the factor differing from the column-strip kernels'."""
    n = 1024
    t = np.random.default_rng(5).uniform(0.0, 3.0, n)
    a = np.exp(-((t[:, None] - t[None, :]) ** 2) / 0.02) + 1e-10 * np.eye(n)
    (new, info_new), (old, info_old) = _potrf_both(egx, a)
    assert info_new == 0 and info_old == 0
    differ = int(np.count_nonzero(_bits(new) != _bits(old)))
    print("entries that differ:", differ)
    assert differ == 0
    # (backward error as in test_gpu_diag_block.py::test_partial_blocks_and_strips: eps * cond(L64) below a diagonal block)
    assert np.abs(new @ new.T - a).max() / np.abs(a).max() < 2e4 * np.finfo(float).eps


def test_lost_pivot_in_the_second_diagonal_block(egx):
    """The recipe of test_gpu_diag_block.py::test_info_is_lapacks_for_a_pivot_failing_anywhere, first bad pivot in column
    300 of 700: the panel solve under the first block has run, every kernel after the second block returns on entry."""
    n, bad = 700, 300
    rng = np.random.default_rng(n + bad)
    g = rng.standard_normal((n, n))
    a = g @ g.T / n + 0.1 * np.eye(n)
    a[bad, bad] = a[bad, :bad] @ np.linalg.solve(a[:bad, :bad], a[:bad, bad]) - 1e-3
    (new, info_new), (old, info_old) = _potrf_both(egx, a)
    assert info_new == bad + 1 and info_old == bad + 1
    # everything egx_potrf hands back -- the factored first block column, the rows nothing touched after the failure, NaNs
    # included -- bit for bit (one stream, so which kernels still ran does not depend on timing)
    assert np.array_equal(_bits(new), _bits(old))
    assert np.all(np.isfinite(new[:, :256]))


def _data(n, d, seed):  # (the generator of test_gpu_pipe.py)
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, d))
    y = np.sin(3 * x[:, 0]) + x[:, 1:].sum(axis=1) ** 2 + 0.1 * rng.standard_normal(n)
    return x, y


THETAS = np.array([[2.0, 2.4, 2.8, 2.2], [2.2, 2.0, 3.2, 2.6], [2.8, 1.8, 2.4, 3.0],
                   [2.4, 2.6, 2.0, 2.8], [3.0, 2.2, 2.6, 2.0], [2.6, 3.0, 2.2, 2.4]])


@pytest.fixture(scope="module")
def handle_runs(egx):
    """n = 600, d = 4 (padded 640: panels of 256, 256 and 128 columns, the fused right-hand-side rows below the square):
    three workspaces in lock-step 3 under both settings, and a one-workspace handle; every evaluation once."""
    x, y = _data(600, 4, 11)
    runs = {}
    for name, rows_min, nws in (("new", ROWS_ALL, 3), ("old", ROWS_NONE, 3), ("lone", ROWS_ALL, 1)):
        with _separate_launches(egx, rows_min):
            with egx.GpHandle(x, y, n_workspaces=nws) as h:
                if nws > 1:
                    assert h.set_lockstep(3) == 3
                s = h.schedule()
                assert s["pipelined_chain"] == 0 and s["lockstep"] == (3 if nws > 1 else 1), s
                lk, st = h.likelihood_batch(THETAS)  # two lock-step sequences of three
                lkg, g, stg = h.likelihood_grad(THETAS[0])
                runs[name] = {"lk": lk, "st": st, "lkg": lkg, "g": g, "stg": stg}
    return runs


def test_lockstep_likelihoods_have_the_same_bits(handle_runs):
    """blockIdx.z, the fused right-hand-side rows (m_tot > n_pad) and the companions of a lock-step sequence"""
    new, old, lone = (handle_runs[k] for k in ("new", "old", "lone"))
    assert not np.any(new["st"]) and np.all(np.isfinite(new["lk"]))
    for other in (old, lone):
        assert np.array_equal(new["st"], other["st"])
        assert np.array_equal(_bits(new["lk"]), _bits(other["lk"]))


def test_theta_gradient_rider_has_the_same_bits(handle_runs):
    """likelihood_grad: the C^-T rider's panels (W_TRSM) take the new kernel too"""
    new, old = handle_runs["new"], handle_runs["old"]
    assert new["stg"] == 0 and old["stg"] == 0
    assert np.array_equal(_bits(new["lkg"]), _bits(old["lkg"]))
    assert np.array_equal(_bits(new["g"]), _bits(old["g"]))
    assert np.all(np.isfinite(new["g"])) and np.any(new["g"] != 0.0)
