"""The conditioning of an infill handle on its pending points (egobox_amd/csrc/kernels_pending.hip, infill_pending.hip pending_tile) at
the shapes where its launch code branches -- the table of tests/pending_cases.py, which tests/test_pending_cases_cpu.py holds to
its gate and to the thresholds on the CPU:

  a  every row: the parts against the oracle's refit with frozen normalisation (tests/pending_oracle.py), tolerances of
     tests/test_gpu_infill_pending.py unchanged
  b  fused = composed to rounding where the fused kernel takes another instance, pass count or LDS path
  c  the hand-over at kPendingMaxD on ONE data set: its 65 inputs (composed) and its first 64 (fused)
  d  the values-only instance (<.., 1, false>) gives the sums of the gradient instance bit for bit at d > 16 and above 64 KiB
  e  companions and clear_pending at d = 17 with a quadratic trend, two tiles
  f  the batch call at d = 12 on models whose pending rows start a slab of Z"""
import numpy as np
import pytest

import pending_cases as PC
from pending_cases import (KEYS, _assert_conditioned, _assert_same_to_rounding, _check_batch, _check_clear_pending,
                           _check_companions, _check_composed_form, _check_parts_against_refit, _close, _objective, _push_all)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


def _row_case(egx, O, r, **kw):
    c = PC.row_case(egx, O, r, **kw)
    assert c.hs[0].h == (r.kpls or c.d)
    return c


# ---- a. parts against the frozen refit ---------------------------------------------------------------------------------------
# (the rows of PC.TWO_MODELS -- three-pass and d >= 41: lds-below, lds-above, fused-last, composed-first, finish-lds -- build the
# objective and one constraint model: the per-point Jacobians of the oracle are what a case costs there; every other row three)
@pytest.mark.parametrize("r", PC.ROWS, ids=[r.id for r in PC.ROWS])
def test_parts_are_the_frozen_refit(egx, O, r):
    c = _row_case(egx, O, r)
    try:
        _assert_conditioned(c, c.xq)
        with _objective(egx, c) as obj:
            _push_all(obj, c)
            px, py, s2 = obj.pending
            np.testing.assert_array_equal(px, c.xv)
            np.testing.assert_array_equal(py, c.yv)
            _check_parts_against_refit(c, obj.parts(c.xq), c.xq, s2)
    finally:
        _close(c)


# ---- b. fused equals composed to rounding ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", ["dk16-first", "two-pass", "three-pass", "lds-above", "fused-last", "kpls-d12"])
def test_fused_is_the_composed_form_to_rounding(egx, O, rid):
    """egx_set_tuning("pending_composed", 1): every per-model key within 1e-9 of its scale, the composed parts against the
    refit, the mean-only twin on the composed layouts bit for bit"""
    c = _row_case(egx, O, PC.BY_ID[rid])
    try:
        _assert_conditioned(c, c.xq)
        with _objective(egx, c) as obj:
            _push_all(obj, c)
            _check_composed_form(egx, c, obj)
    finally:
        _close(c)


# ---- c. the hand-over at kPendingMaxD ----------------------------------------------------------------------------------------
def _parts_under_the_knob(egx, obj, xq):
    assert egx.set_tuning("pending_composed", 1) == 0
    try:
        return obj.parts(xq)
    finally:
        assert egx.set_tuning("pending_composed", 0) == 1


def test_hand_over_at_the_last_fused_dimension(egx, O):
    """The data, pending points and queries of composed-first, once with their 65 inputs and once with the first 64: either
    side of d = kPendingMaxD against its own refit.  At 65 the knob changes nothing (composed either way: the same bits); at
    64 it changes the form, not the values (fused-last itself under the knob is a row of b)."""
    r = PC.BY_ID["composed-first"]
    for keep in (None, PC.K_PENDING_MAX_D):
        c = _row_case(egx, O, r, keep=keep)
        try:
            assert c.d == (65 if keep is None else 64) and c.x.shape == (r.n, c.d) and c.xv.shape == (r.q, c.d)
            _assert_conditioned(c, c.xq)
            with _objective(egx, c) as obj:
                _push_all(obj, c)
                p = obj.parts(c.xq)
                _check_parts_against_refit(c, p, c.xq, obj.pending[2])
                knob = _parts_under_the_knob(egx, obj, c.xq)
                if keep is None:
                    for k in KEYS:
                        np.testing.assert_array_equal(knob[k], p[k])
                else:
                    _assert_same_to_rounding(knob, p)
                    assert any(not np.array_equal(knob[k], p[k]) for k in KEYS[2:])  # (another order of summation did run)
        finally:
            _close(c)


# ---- d. the values-only instance ---------------------------------------------------------------------------------------------
# two-pass and lds-above, the other three kernels at d = 16 / 17 (q = 7: a ragged QV = 4 pass), and the DK = 8 instance at d = 3
VALUES_ONLY = ["two-pass", "lds-above", "two-pass-abs", "two-pass-m32", "dk16-full", (130, 3, 5, 1.5, 0, 3)]


@pytest.mark.parametrize("spec", VALUES_ONLY, ids=[s if isinstance(s, str) else "d3" for s in VALUES_ONLY])
def test_values_only_instance_gives_the_same_sums(egx, O, spec):
    """outg == nullptr launches k_pending_cross<.., 1, false>: a column's value sum is the one of the gradient instance"""
    c = _row_case(egx, O, PC.BY_ID[spec]) if isinstance(spec, str) else PC._case(egx, O, *spec)
    try:
        with _objective(egx, c) as obj:
            np.testing.assert_array_equal(obj.value(c.xq), obj.value_and_grad(c.xq)[0])  # (the fitted handle: no pending kernel)
            _push_all(obj, c)
            v, g = obj.value_and_grad(c.xq)
            np.testing.assert_array_equal(obj.value(c.xq), v)
            np.testing.assert_array_equal(v, obj.parts(c.xq)["value"])
            assert np.all(np.isfinite(v)) and np.all(np.isfinite(g))
            for strategy in ("mean", "utb"):
                obj.set_cstr_strategy(strategy, [1.3, 0.6][:len(c.hs) - 1])
                v0, cs0 = obj.constraints(c.xq, grad=False)
                v1, cs1, g1, gc1 = obj.constraints(c.xq, grad=True)
                np.testing.assert_array_equal(v0, v1)
                np.testing.assert_array_equal(cs0, cs1)
                assert np.all(np.isfinite(cs1)) and np.all(np.isfinite(gc1))
    finally:
        _close(c)


# ---- e. companions and clearing at d > 16 ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quad(egx, O):
    c = _row_case(egx, O, PC.BY_ID["two-pass-quad"], m=131)
    yield c
    _close(c)


def test_a_conditioned_point_does_not_depend_on_its_companions(egx, quad):
    c = quad
    big = _check_companions(egx, c)  # 131 points: two tiles, the second ragged
    with _objective(egx, c, criterion=egx.LOG_EI) as obj:  # ... nor on their order
        _push_all(obj, c)
        perm = np.random.default_rng(5).permutation(131)
        shuffled = obj.parts(c.xq[perm])
        for k in KEYS:
            np.testing.assert_array_equal(shuffled[k], np.take(big[k], perm, axis=0 if k in ("value", "grad") else 1))


def test_clear_pending_gives_back_the_fitted_handle_bit_for_bit(egx, quad):
    _check_clear_pending(egx, quad)


# ---- f. a batch at d = 12 ----------------------------------------------------------------------------------------------------
def test_batch_is_the_manual_loop_and_the_refit(egx, O):
    """the models of slab-q16 (n = 192: every pushed point's identity row starts the fourth slab), q = 3"""
    c = _row_case(egx, O, PC.BY_ID["slab-q16"])
    try:
        _check_batch(egx, c, 3, 8, "slsqp", "kb")
    finally:
        _close(c)
