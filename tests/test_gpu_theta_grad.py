"""The likelihood's theta-gradient (kernels_corr.hip k_grad_accum / k_grad_reduce, gp_host.hip make_coef, gp_fit.hip
grad_chain_rule) against the closed form of tests/theta_grad_oracle.py on every row of tests/theta_grad_cases.py: each compiled
form of the trace kernel (MODE 0 / 1 / 2, DK 8 / 16 / 32), one and two output chunks from the slabs of pass 1, the restaged
chunks beyond 64 dimensions, partial 64-tiles, zeros in theta and in w_star, the collapsed coefficients' chain rule, and the
linear and quadratic trends.  Then the same values through the lock-step entry points: a batch of one handle on a MODE 0 shape,
a group with the raw form between prescaled neighbours, and the collapse beside its zero-row twin.

The bar is the project's gradient bar (tests/test_gpu_parity.py test_likelihood_gradient): 1e-6 relative with an absolute floor
of 1e-6 of the largest component, and LK_RTOL on the likelihood.  tests/test_theta_grad_oracle_cpu.py holds every row's oracle
pivot in [1e-2, 0.98]; the achieved deviations are printed per case (profiles/theta_grad_parity.txt)."""
import numpy as np
import pytest

import theta_grad_cases as TC
from test_gpu_parity import LK_RTOL

pytestmark = pytest.mark.gpu

OK = 0


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _check(label, lk, g, st, ref):
    lk_ref, g_ref, piv = ref
    scale = np.abs(g_ref).max()
    print(f"{label}: status {st} likelihood rel {abs(lk - lk_ref) / abs(lk_ref):.2e} gradient worst {np.max(np.abs(g - g_ref)) / scale:.2e} "
          f"of max |g| {scale:.3e} (oracle pivot {piv:.2e})")
    assert st == OK
    assert lk == pytest.approx(lk_ref, rel=LK_RTOL)
    np.testing.assert_allclose(g, g_ref, rtol=1e-6, atol=1e-6 * scale)


@pytest.mark.parametrize("case", TC.CASES, ids=[c.name for c in TC.CASES])
def test_row_against_closed_form(egx, case):
    m = TC.member(case)
    with egx.GpHandle(m.x, m.y, mean=m.mean, corr=m.corr, w_star=m.w) as h:
        assert h.h == m.theta.size
        lk, g, st = h.likelihood_grad(m.theta)
    _check(case.name, lk, g, st, TC.reference(case))
    if case.zero_component:
        # sq-exp and the Materns are flat in a coefficient at zero: the raw form gives an exact zero, not a small number
        assert (g[1] != 0.0) if case.corr == TC.ABSEXP else (g[1] == 0.0)


def test_mode0_batch_rows(egx):
    """likelihood_grad_batch of four thetas on KPLS + Matern-5/2 (12, 9), in lock-step on four workspaces: every row"""
    ms = TC.mode0_batch()
    with egx.GpHandle(ms[0].x, ms[0].y, mean=ms[0].mean, corr=ms[0].corr, w_star=ms[0].w, n_workspaces=4) as h:
        lk, g, st = h.likelihood_grad_batch(np.stack([m.theta for m in ms]))
    for j, m in enumerate(ms):
        _check(m.label, lk[j], g[j], st[j], TC.reference(m))


def test_mixed_form_group_rows(egx):
    """likelihood_grad_multi on a group of four whose member 2 has theta[1] = 0.0 (the raw form between prescaled
    neighbours: three launch sequences): all four rows, not only the statuses"""
    ms = TC.mixed_group()
    hs = egx.GpHandle.create_group(np.stack([m.x for m in ms]), np.stack([m.y for m in ms]), mean=ms[0].mean, corr=ms[0].corr)
    try:
        lk, g, st = egx.likelihood_grad_multi(hs, np.stack([m.theta for m in ms]))
    finally:
        for h in hs:
            h.close()
    for j, m in enumerate(ms):
        _check(m.label, lk[j], g[j], st[j], TC.reference(m))
    assert g[2, 1] == 0.0 and np.all(g[[0, 1, 3], 1] != 0.0)


def test_collapse_beside_its_zero_row_twin(egx):
    """The sq-exp collapse at (40, 33) as a batch of two thetas, and the same batch on the twin whose w_star has a zero row
    (coef_1 = 0: the raw form, the chain rule's guard), both handles open at once: every row"""
    ms = TC.companions()
    dense, twin = ms[:2], ms[2:]
    with egx.GpHandle(dense[0].x, dense[0].y, corr=dense[0].corr, w_star=dense[0].w, n_workspaces=2) as ha, \
            egx.GpHandle(twin[0].x, twin[0].y, corr=twin[0].corr, w_star=twin[0].w, n_workspaces=2) as hb:
        ra = ha.likelihood_grad_batch(np.stack([m.theta for m in dense]))
        rb = hb.likelihood_grad_batch(np.stack([m.theta for m in twin]))
        ra2 = ha.likelihood_grad_batch(np.stack([m.theta for m in dense]))
    for (lk, g, st), part in ((ra, dense), (rb, twin)):
        for j, m in enumerate(part):
            _check(m.label, lk[j], g[j], st[j], TC.reference(m))
    assert np.array_equal(ra[0], ra2[0]) and np.array_equal(ra[1], ra2[1])  # (the twin's run left the first handle alone)
