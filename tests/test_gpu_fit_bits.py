"""Every hyperparameter fit's result as BITS, against tests/golden/fit_bits.json: the fitted parameters and the likelihood as
float.hex() and the evaluation counts of each entry point -- egx_gp_fit, egx_gp_fit_partial, egx_gp_fit_lbfgs, egx_sweep_fit,
egx_gp_fit_multi, egx_sgp_fit, egx_sgp_fit_lbfgs, egx_sgp_fit_lbfgs_z -- at the smallest shapes at which each multistart
driver branches (starts of unequal length, one on the lower bound, a broadcast and a full-length box, a partial active set,
noise estimated and fixed).  The other fit tests pin these paths to EACH OTHER; a change that moved all of them alike would
pass those.  The file was recorded at the commit its "recorded_at" names, not by the code under test: a difference means the
arithmetic or the order of the evaluations moved.

Regenerate (only when a change is MEANT to move the bits): `python tests/test_gpu_fit_bits.py tests/golden/fit_bits.json`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fit_bits.json")


def _dense(n, d, seed):  # (the generator of test_gpu_pipe.py)
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, d))
    y = np.sin(3 * x[:, 0]) + x[:, 1:].sum(axis=1) ** 2 + 0.1 * rng.standard_normal(n)
    return x, y


def _sparse(n, nz, d, seed=0, noise=0.05):  # (the generator of test_gpu_sgp_grad.py)
    rng = np.random.default_rng(seed)
    x = rng.random((n, d)) * 2 - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + noise * rng.standard_normal(n)
    z = x[rng.permutation(n)[:nz]].copy()
    return x, y, z


def _hex(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def _dense_record(h, ne):
    inner = h.inner()
    return {"theta": _hex(inner["theta"]), "likelihood": float(inner["likelihood"]).hex(), "n_evals": int(ne)}


def _sparse_record(h, ne, with_z=False):
    st = h.state()
    out = {"theta": _hex(st["theta"]), "sigma2": float(st["sigma2"]).hex(), "noise": float(st["noise"]).hex(),
           "likelihood": float(st["likelihood"]).hex(), "n_evals": int(ne)}
    if with_z:
        out["z"] = _hex(h.inducings())
    return out


# three starts, the first ON the lower bound of the box: its machine ends rounds before the others do
LO1, HI1 = [0.05], [5.0]
LO3, HI3 = [0.05, 0.02, 0.1], [5.0, 8.0, 3.0]
STARTS3 = np.array([[0.05, 0.05, 0.05], [1.0, 0.5, 2.0], [0.3, 3.0, 0.8]])
STARTS3_BH = np.array([[0.05, 0.02, 0.1], [1.0, 0.5, 2.0], [0.3, 3.0, 0.8]])


def run_cases(egx):
    """name -> record, every entry point once."""
    out = {}
    x, y = _dense(200, 3, 11)
    for name, corr, nws, lo, hi, starts in (("fit/sqexp/bounds_len=1", 0, 1, LO1, HI1, STARTS3),
                                            ("fit/sqexp/bounds_len=h/2-workspaces", 0, 2, LO3, HI3, STARTS3_BH),
                                            ("fit/absexp/bounds_len=1", 1, 1, LO1, HI1, STARTS3)):
        with egx.GpHandle(x, y, corr=corr, n_workspaces=nws) as h:
            out[name] = _dense_record(h, h.fit(starts, lo, hi))
    for name, lo, hi in (("fit_partial/active=0,2/bounds_len=1", LO1, HI1),
                         ("fit_partial/active=0,2/bounds_len=h", [0.05, 0.1], [5.0, 3.0])):
        with egx.GpHandle(x, y) as h:
            ne = h.fit_partial([0.7, 0.4, 1.1], [0, 2], STARTS3[:, [0, 2]] if len(lo) == 1 else STARTS3_BH[:, [0, 2]], lo, hi)
            out[name] = _dense_record(h, ne)
    for name, nws, lo, hi, starts in (("fit_lbfgs/bounds_len=1", 1, LO1, HI1, STARTS3),
                                      ("fit_lbfgs/bounds_len=h/2-workspaces", 2, LO3, HI3, STARTS3_BH)):
        with egx.GpHandle(x, y, n_workspaces=nws) as h:
            out[name] = _dense_record(h, h.fit_lbfgs(starts, lo, hi))
    with egx.Sweep(x, y, device=0, rank=0, world=1, id_bytes="new", n_workspaces=2) as sw:
        ne = sw.fit(STARTS3, LO1, HI1)
        m = sw.model()
        out["sweep_fit/one-rank"] = _dense_record(m, ne)
        m.close()

    sets = [_dense(256, 2, 90 + j) for j in range(3)]
    starts2 = np.array([[0.05, 0.05], [1.0, 0.4]])
    hs = egx.GpHandle.create_group(np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]))
    try:
        nes = egx.fit_multi(hs, np.tile(starts2, (3, 1, 1)), LO1, HI1)
        for j, h in enumerate(hs):
            out[f"fit_multi/k=3/member-{j}"] = _dense_record(h, nes[j])
    finally:
        for h in hs:
            h.close()

    xs, ys, zs = _sparse(200, 10, 2, seed=200)
    s20 = float(np.var(ys, ddof=1))
    slo, shi = [1e-2, 1e-2, 1e-12, 1e-10], [1e2, 1e2, 9.0 * s20, 1.0]
    sstarts = np.array([[1.0, 1.0, s20, 1e-2], [5.0, 0.2, 0.5 * s20, 1e-3]])
    with egx.SgpHandle(xs, ys, zs, corr=3) as h:
        out["sgp_fit/noise-estimated"] = _sparse_record(h, h.fit(sstarts, slo, shi, True, 1e-2, 1000))
        out["sgp_fit/noise-fixed"] = _sparse_record(h, h.fit(sstarts[:, :3], slo[:3], shi[:3], False, 2.5e-3, 1000))
        out["sgp_fit_lbfgs/noise-estimated"] = _sparse_record(h, h.fit_lbfgs(sstarts, slo, shi, True, 1e-2))
        out["sgp_fit_lbfgs/noise-fixed"] = _sparse_record(h, h.fit_lbfgs(sstarts[:, :3], slo[:3], shi[:3], False, 2.5e-3))
    with egx.SgpHandle(xs, ys, zs, corr=3) as h:
        ne = h.fit_lbfgs_z(sstarts, slo, shi, True, 1e-2, max_iter_z=5)
        out["sgp_fit_lbfgs_z/max_iter_z=5"] = _sparse_record(h, ne, with_z=True)
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    import egobox_amd
    return run_cases(egobox_amd)


def test_the_golden_file_and_the_cases_name_the_same_fits(golden, got):
    assert sorted(golden["cases"]) == sorted(got)
    assert len(golden["recorded_at"]) == 40 and golden["how"]


@pytest.mark.parametrize("prefix", ["fit/", "fit_partial/", "fit_lbfgs/", "sweep_fit/", "fit_multi/", "sgp_fit/", "sgp_fit_lbfgs/",
                                    "sgp_fit_lbfgs_z/"])
def test_fit_ends_at_the_recorded_bits_after_the_recorded_evaluations(golden, got, prefix):
    names = [n for n in golden["cases"] if n.startswith(prefix)]
    assert names
    for name in names:
        print(name, got[name])
        assert got[name] == golden["cases"][name], name


if __name__ == "__main__":  # record: see the module docstring
    sys.path.insert(0, ROOT)
    import egobox_amd

    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    doc = {"recorded_at": os.environ.get("EGX_FIT_BITS_COMMIT", commit),
           "how": "On an MI355X, at the commit of recorded_at: build, then `python tests/test_gpu_fit_bits.py "
                  "tests/golden/fit_bits.json` (EGX_FIT_BITS_COMMIT names the commit where the tree is no git checkout).",
           "cases": run_cases(egobox_amd)}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(doc['cases'])} cases to {sys.argv[1]}")
