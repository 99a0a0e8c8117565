"""What launch_potrf (csrc/kernels_chol.hip; its launch order is csrc/potrf_plan.h) computes, as BITS, against
tests/golden/potrf_bits.json: the reduced likelihood and its theta-gradient as float.hex(), and for one-workspace handles the
SHA-256 of the fitted factor, on every branch of the launch order -- separate launches with look-ahead, chain launches per
group of panels (waiting on the device and on the stream), the whole chain launch, left-looking updates, each with and without
the theta-gradient's C^-T rider and alone and in lock-step, forced at the smallest sizes that have one, two and three groups
of panels; and at n = 14336, the first size with the look-ahead columns' update on the side stream, the default left-looking
schedule and the flow tail; and, in the group refine/..., an ill-conditioned matrix whose strips take the refinement step of
the strip solve (csrc/panel_strip.h) through every kernel that solves a panel.  The other tests pin these forms to EACH OTHER and to LAPACK to rounding; a change of the order
that moved a form's bits, or all forms alike, would pass those.  The file was recorded at the commit its "recorded_at" names,
not by the code under test.

Regenerate (only when a change is MEANT to move the bits): `python tests/test_gpu_potrf_bits.py tests/golden/potrf_bits.json`."""
import contextlib
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "potrf_bits.json")


def _data(n, d, seed):  # (the generator of test_gpu_pipe.py)
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, d))
    y = np.sin(3 * x[:, 0]) + x[:, 1:].sum(axis=1) ** 2 + 0.1 * rng.standard_normal(n)
    return x, y


@contextlib.contextmanager
def _knobs(egx, settings):
    """egx_set_tuning settings of one case, restored afterwards (the `knobs` fixture of test_gpu_pipe.py)"""
    saved = {}
    try:
        for name, value in settings.items():
            saved.setdefault(name, egx.set_tuning(name, value))
        yield
    finally:
        for k, v in saved.items():
            egx.set_tuning(k, v)


def _hex(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


# "potrf_left", "pipe" and "potrf_group" enter a handle when it is created, "look_min" when it evaluates: the settings of a form
# stay in force from the handle's creation to its last evaluation.  (knobs, workspaces, lock-step width, what schedule() says)
FORMS = {
    "separate/look": ({"pipe": 0, "look_min": 256, "potrf_group": 1}, 1, 1,
                      {"pipelined_chain": 0, "left_looking": 0, "panels_per_group": 1}),
    "chain-per-group/1ws": ({"pipe": 2, "look_min": 256}, 1, 1,
                            {"pipelined_chain": 1, "whole_factorisation_launch": 0, "left_looking": 0}),
    "chain-per-group/3ws-width3": ({"pipe": 2, "look_min": 256}, 3, 3,
                                   {"pipelined_chain": 1, "whole_factorisation_launch": 0, "lockstep": 3}),
    # (three launch sequences of the handle in flight: the look-ahead chain launch waits on the STREAM, not on the device)
    "chain-per-group/3ws-width1": ({"pipe": 2, "look_min": 256}, 3, 1,
                                   {"pipelined_chain": 1, "whole_factorisation_launch": 0, "lockstep": 1}),
    "left/separate": ({"potrf_left": 2, "pipe": 0}, 1, 1, {"left_looking": 1, "pipelined_chain": 0}),
    "defaults": ({}, 1, 1, {"pipelined_chain": 1, "whole_factorisation_launch": 1, "left_looking": 0}),
}
SMALL_N = (300, 1000, 1500)  # padded 384, 1024, 1536: a last panel of 128 columns; two panels; three groups of two panels at most
# (squared exponential on 1500 points in three dimensions: smaller thetas lose a pivot at the default nugget)
THETAS3 = np.array([[2.0, 2.4, 2.8], [2.2, 2.0, 3.2], [2.8, 1.8, 2.4]])


def _evaluate(h, thetas, lone):
    """every evaluation entry point once: the factorisation alone, with the rider, and both through the batch path"""
    rec = {}
    lk, st = h.likelihood(thetas[0])
    rec["likelihood"] = [float(lk).hex(), int(st)]
    lk, g, st = h.likelihood_grad(thetas[0])
    rec["likelihood_grad"] = [float(lk).hex(), _hex(g), int(st)]
    lk, st = h.likelihood_batch(thetas)
    rec["likelihood_batch"] = [_hex(lk), [int(s) for s in st]]
    lk, g, st = h.likelihood_grad_batch(thetas)
    rec["likelihood_grad_batch"] = [_hex(lk), _hex(g), [int(s) for s in st]]
    if lone:
        h.finalize(thetas[0])
        rec["r_chol_sha256"] = hashlib.sha256(np.ascontiguousarray(h.inner(with_chol=True)["r_chol"]).tobytes()).hexdigest()
    return rec


def run_form(egx, form):
    settings, nws, width, want = FORMS[form]
    out = {}
    with _knobs(egx, settings):
        for n in SMALL_N:
            x, y = _data(n, 3, 7 + n)
            with egx.GpHandle(x, y, n_workspaces=nws) as h:
                if nws > 1:
                    assert h.set_lockstep(width) == width
                s = h.schedule()
                assert {k: s[k] for k in want} == want, (form, n, s)
                out[f"{form}/n={n}"] = _evaluate(h, THETAS3, nws == 1)
    return out


N_BIG, D_BIG = 14336, 8


def _big_thetas(egx, k):
    base = egx.workload.default_theta(D_BIG) * 3.0
    return np.stack([base * (1.0 + 0.01 * j) for j in range(k)])


def run_big(egx, which):
    """n = 14336 under the default knobs; the schedule each case relies on is checked on the handle"""
    x, y = _data(N_BIG, D_BIG, 3)
    out = {}
    if which == "lone":
        th = _big_thetas(egx, 1)[0]
        with egx.GpHandle(x, y) as h:
            s = h.schedule()
            assert (s["left_looking"], s["left_looking_rider"], s["pipelined_chain"], s["panels_per_group"], s["lockstep"],
                    s["flow"]) == (0, 0, 0, 4, 1, 2), s        # (flow = 2: the flow tail)
            lk, st = h.likelihood(th)                      # right-looking by separate launches, the last 6144 columns a flow launch
            lkg, g, stg = h.likelihood_grad(th)            # right-looking with the side stream, the rider right-looking
            rec = {"likelihood": [float(lk).hex(), int(st)], "likelihood_grad": [float(lkg).hex(), _hex(g), int(stg)]}
            h.finalize(th)
            rec["r_chol_sha256"] = hashlib.sha256(np.ascontiguousarray(h.inner(with_chol=True)["r_chol"]).tobytes()).hexdigest()
            out["n=14336/lone"] = rec
    elif which == "width4":
        with egx.GpHandle(x, y, n_workspaces=4) as h:
            assert h.set_lockstep(4) == 4
            s = h.schedule()
            assert (s["left_looking"], s["left_looking_rider"], s["panels_per_group"], s["lockstep"]) == (0, 1, 4, 4), s
            lk, g, st = h.likelihood_grad_batch(_big_thetas(egx, 4))   # the rider left-looking
            out["n=14336/width4"] = {"likelihood_grad_batch": [_hex(lk), _hex(g), [int(v) for v in st]]}
    else:
        with egx.GpHandle(x, y, n_workspaces=8) as h:
            assert h.set_lockstep(8) == 8
            s = h.schedule()
            assert (s["left_looking"], s["left_looking_rider"], s["panels_per_group"], s["lockstep"]) == (1, 1, 4, 8), s
            lk, st = h.likelihood_batch(_big_thetas(egx, 8))           # left-looking
            out["n=14336/width8"] = {"likelihood_batch": [_hex(lk), [int(v) for v in st]]}
    return out


BIG = ("lone", "width4", "width8")

# ---- refine/...: the refinement step X += (T - X L_kk^T) Linv_k^T of the strip solve, on every kernel that solves a panel.
# The matrix of test_gpu_panel_rows.py::test_ill_conditioned_kernel_matrix_takes_the_refinement_step (cond(L) ~ 1e6, padded
# 1024: four panels with 768 / 512 / 256 rows below the blocks) through egx.potrf by separate launches -- the row-owning
# kernel and the column-strip kernel under the diagonal-block kernel -- and by the two chain launches (the chain role's TRSM
# task under the chain's diagonal role).  That every case takes the branch was confirmed with ONE scratch build in which the
# refinement step of panel_strip.h did nothing: all six cases then failed.
# (knobs, what schedule() says of a one-workspace handle of this size: egx.potrf factors by that handle's schedule)
REFINE_POTRF = {
    "separate/rows": ({"pipe": 0, "trsm_rows_min": 64}, {"pipelined_chain": 0, "left_looking": 0}),
    "separate/strips": ({"pipe": 0, "trsm_rows_min": 1 << 30}, {"pipelined_chain": 0, "left_looking": 0}),
    "chain-per-group": ({"pipe": 2}, {"pipelined_chain": 1, "whole_factorisation_launch": 0, "left_looking": 0}),
    "whole-chain": ({"pipe": 1}, {"pipelined_chain": 1, "whole_factorisation_launch": 1, "left_looking": 0}),
}
# ... and on the solves after the factorisation: a one-dimensional training set of 300 points of [0, 3] at theta = 3.2 on the
# standardised inputs with the same nugget (cond(L) ~ 9e5 by numpy, as above), predict_var at 128 queries (k_panel_trsm16<1, true>)
# and at 4096, the first size launch_trsm_rows gives to k_panel_trsm16<2, true>
REFINE_QUERIES = (128, 4096)


def _ill_conditioned_matrix():
    n = 1024
    t = np.random.default_rng(5).uniform(0.0, 3.0, n)
    return np.exp(-((t[:, None] - t[None, :]) ** 2) / 0.02) + 1e-10 * np.eye(n)


def run_refine_potrf(egx, form):
    settings, want = REFINE_POTRF[form]
    with _knobs(egx, settings):
        with egx.GpHandle(np.linspace(0.0, 1.0, 1024)[:, None], np.linspace(0.0, 1.0, 1024)) as h:
            s = h.schedule()
            assert {k: s[k] for k in want} == want, (form, s)
        fac, info = egx.potrf(_ill_conditioned_matrix())
    return {f"refine/potrf/{form}": {"info": int(info), "sha256": hashlib.sha256(np.ascontiguousarray(fac).tobytes()).hexdigest()}}


def run_refine_predict(egx):
    x = np.random.default_rng(5).uniform(0.0, 3.0, 300)
    xq = np.random.default_rng(6).uniform(-0.3, 3.3, max(REFINE_QUERIES))
    with egx.GpHandle(x[:, None], np.sin(3.0 * x), nugget=1e-10) as h:
        h.finalize(np.array([3.2]))
        return {f"refine/predict_var/m={m}": {"predict_var": _hex(h.predict_var(xq[:m, None]))} for m in REFINE_QUERIES}


def run_cases(egx):
    out = {}
    for form in FORMS:
        out.update(run_form(egx, form))
    for which in BIG:
        out.update(run_big(egx, which))
    for form in REFINE_POTRF:
        out.update(run_refine_potrf(egx, form))
    out.update(run_refine_predict(egx))
    return out


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _compare(golden, got):
    assert got
    for name, rec in got.items():
        print(name, rec)
        assert rec == golden["cases"][name], name


def test_the_golden_file_names_the_cases(golden):
    names = [f"{form}/n={n}" for form in FORMS for n in SMALL_N] + [f"n=14336/{w}" for w in BIG]
    refine = [f"refine/potrf/{form}" for form in REFINE_POTRF] + [f"refine/predict_var/m={m}" for m in REFINE_QUERIES]
    assert sorted(golden["cases"]) == sorted(names + refine)
    assert len(golden["recorded_at"]) == 40 and golden["how"]
    for name, rec in golden["cases"].items():  # a recording of lost pivots would pin nothing
        if name.startswith("refine/potrf/"):
            assert rec["info"] == 0 and len(rec["sha256"]) == 64, name
            continue
        if name.startswith("refine/predict_var/"):
            var = np.array([float.fromhex(v) for v in rec["predict_var"]])
            assert var.size == int(name.split("=")[1]) and np.all(np.isfinite(var)) and np.unique(var).size > var.size // 2, name
            continue
        for key, val in rec.items():
            if key != "r_chol_sha256":
                assert not np.any(np.asarray(val[-1])), (name, key)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_forced_forms_give_the_recorded_bits(egx, golden, form):
    _compare(golden, run_form(egx, form))


@pytest.mark.parametrize("which", BIG)
def test_n_14336_gives_the_recorded_bits(egx, golden, which):
    _compare(golden, run_big(egx, which))


@pytest.mark.parametrize("form", sorted(REFINE_POTRF))
def test_refinement_step_in_the_factorisation_gives_the_recorded_bits(egx, golden, form):
    _compare(golden, run_refine_potrf(egx, form))


def test_refinement_step_moves_between_the_panel_kernels_without_a_bit(egx, golden):
    """ "trsm_rows_min" is a launch-time knob: the recorded factors of the two separate-launch forms are one factor"""
    assert golden["cases"]["refine/potrf/separate/rows"] == golden["cases"]["refine/potrf/separate/strips"]
    rows, strips = (list(run_refine_potrf(egx, form).values())[0] for form in ("separate/rows", "separate/strips"))
    assert rows["info"] == 0 and rows == strips


@pytest.mark.parametrize("m", REFINE_QUERIES)
def test_refinement_step_after_the_factorisation_gives_the_recorded_bits(egx, golden, m):
    name = f"refine/predict_var/m={m}"
    _compare(golden, {name: run_refine_predict(egx)[name]})


if __name__ == "__main__":  # record: see the module docstring
    sys.path.insert(0, ROOT)
    import egobox_amd

    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    doc = {"recorded_at": os.environ.get("EGX_POTRF_BITS_COMMIT", commit),
           "how": "On an MI355X, with the library built at the commit of recorded_at: `python tests/test_gpu_potrf_bits.py "
                  "tests/golden/potrf_bits.json` (EGX_POTRF_BITS_COMMIT names the commit where the tree is no git checkout).",
           "cases": run_cases(egobox_amd)}
    with open(sys.argv[1], "w") as f:  # one case per line
        f.write('{"recorded_at": %s,\n "how": %s,\n "cases": {\n' % (json.dumps(doc["recorded_at"]), json.dumps(doc["how"])))
        names = sorted(doc["cases"])
        for i, name in enumerate(names):
            f.write('  %s: %s%s\n' % (json.dumps(name), json.dumps(doc["cases"][name], sort_keys=True), "," if i + 1 < len(names) else ""))
        f.write(' }\n}\n')
    print(f"wrote {len(doc['cases'])} cases to {sys.argv[1]}")
