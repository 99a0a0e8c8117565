"""CPU checks of the mixture recombination behind the infill criterion: egobox_amd/csrc/infill_mix_math.h compiled with g++
(tests/c_host/infill_mix_math_test.cpp, no GPU) against the numpy fold of egobox_amd/moe.py (GpMixture.predict_valvar /
predict_valvar_gradients with duck-typed experts), and the C ABI of the feature.

The bound.  Every output is a sum over the k experts of at most 2 k products of at most 3 factors, one rounding per operation:
each term carries at most 3 roundings, the running sum k more, and the numpy fold is allowed the same.  With margin for a fused
against a separate multiply-add:  |got - want| <= 4 (k + 1) eps sum |terms|.  Hard mode copies: equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egobox_amd", "csrc")
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("infill_mix") / "infill_mix_math_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "c_host", "infill_mix_math_test.cpp"), "-o", str(out)], check=True)
    return str(out)


def _line(smooth, p, dp, mu, v, gmu, gv):
    k, d = dp.shape
    tok = [int(smooth), k, d]
    for a in (p, dp, mu, v, gmu, gv):
        tok += [repr(float(x)) for x in np.ravel(a)]
    return " ".join(str(t) for t in tok)


def _run(exe, lines, d):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [np.array([float(t) for t in ln.split()]) for ln in out.strip().splitlines()]
    assert len(rows) == len(lines)
    return [(r[0], r[1], r[2:2 + d], r[2 + d:2 + 2 * d]) for r in rows]


class _Expert:
    """a duck-typed expert that returns fixed parts for the one query point"""

    def __init__(self, mu, v, gmu, gv):
        self.mu, self.v, self.gmu, self.gv = mu, v, gmu, gv

    def predict(self, x):
        return np.full(x.shape[0], self.mu)

    def predict_var(self, x):
        return np.full(x.shape[0], self.v)

    def predict_valvar(self, x):
        return self.predict(x), self.predict_var(x)

    def predict_gradients(self, x):
        return np.tile(self.gmu, (x.shape[0], 1))

    def predict_var_gradients(self, x):
        return np.tile(self.gv, (x.shape[0], 1))


class _Gmx:
    """a duck-typed mixture with fixed responsibilities"""

    def __init__(self, p, dp):
        self.p, self.dp, self.n_clusters = p, dp, p.shape[0]

    def predict_probas(self, x):
        return np.tile(self.p, (x.shape[0], 1))

    def predict_probas_derivatives(self, x):
        return np.tile(self.dp, (x.shape[0], 1, 1))

    def predict(self, x):
        return np.full(x.shape[0], int(np.argmax(self.p)))


def _fold(smooth, p, dp, mu, v, gmu, gv):
    """egobox_amd/moe.py's numpy recombination at one point"""
    from egobox_amd.moe import GpMixture
    k, d = dp.shape
    moe = GpMixture([_Expert(mu[e], v[e], gmu[e], gv[e]) for e in range(k)], _Gmx(p, dp), "smooth" if smooth else "hard")
    moe.n_in_flight = 1
    x = np.zeros((1, d))
    val, var = moe.predict_valvar(x)
    gy, gvv = moe.predict_valvar_gradients(x)
    return val[0], var[0], gy[0], gvv[0]


def _bounds(p, dp, mu, v, gmu, gv):
    """4 (k + 1) eps sum |terms| per output"""
    k = p.shape[0]
    c = 4.0 * (k + 1) * EPS
    pc = p[:, None]
    return (c * np.sum(np.abs(p * mu)), c * np.sum(np.abs(p * p * v)),
            c * np.sum(np.abs(pc * gmu) + np.abs(dp * mu[:, None]), axis=0),
            c * np.sum(np.abs(pc * pc * gv) + np.abs(2.0 * pc * dp * v[:, None]), axis=0))


def _case(rng, k, d, tie=False):
    p = rng.random(k) + 0.05
    p /= p.sum()
    if tie and k > 1:
        p[1] = p[0]
        if k > 2:
            p[2:] = p[2:] * 0.1  # the two tied experts hold the maximum
    dp = rng.standard_normal((k, d))
    if k == 1:  # one cluster: the responsibilities are ones (gaussian_mixture.rs:115-116)
        p, dp = np.ones(1), np.zeros((1, d))
    mu, v = rng.standard_normal(k) * 3.0, np.exp(rng.uniform(np.log(1e-4), np.log(10.0), k))
    return p, dp, mu, v, rng.standard_normal((k, d)), rng.standard_normal((k, d)) * v[:, None]


@pytest.mark.parametrize("d", [1, 3, 4])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_recombination_matches_the_numpy_fold(exe, k, d):
    rng = np.random.default_rng(1000 * k + d)
    cases = [(smooth, _case(rng, k, d)) for smooth in (True, False) for _ in range(25)]
    rows = _run(exe, [_line(s, *c) for s, c in cases], d)
    worst = 0.0
    for (smooth, c), got in zip(cases, rows):
        want = _fold(smooth, *c)
        if smooth:
            for g, w, b in zip(got, want, _bounds(*c)):
                assert np.all(np.abs(g - w) <= b), (k, d, g, w, b)
                worst = max(worst, float(np.max(np.abs(g - w) / np.where(b > 0, b, 1.0))))
        else:  # hard: a copy of the winner's parts
            e = int(np.argmax(c[0]))
            for g, w, src in zip(got, want, (c[2][e], c[3][e], c[4][e], c[5][e])):
                np.testing.assert_array_equal(g, w)
                np.testing.assert_array_equal(g, src)
    print(f"k {k} d {d}: worst smooth error / bound {worst:.3f}")


@pytest.mark.parametrize("k", [2, 3, 5])
def test_a_tie_goes_to_the_first_expert(exe, k):
    rng = np.random.default_rng(77 + k)
    d = 3
    c = _case(rng, k, d, tie=True)
    assert c[0][0] == c[0][1] == c[0].max()
    mean, var, gm, gv = _run(exe, [_line(False, *c)], d)[0]
    assert (mean, var) == (c[2][0], c[3][0])
    np.testing.assert_array_equal(gm, c[4][0])
    np.testing.assert_array_equal(gv, c[5][0])
    assert mean != c[2][1]
    # and the smooth form of the same case stays inside its bound
    got = _run(exe, [_line(True, *c)], d)[0]
    for g, w, b in zip(got, _fold(True, *c), _bounds(*c)):
        assert np.all(np.abs(g - w) <= b)


def test_header_declares_and_library_exports_the_mixture_symbols():
    import egobox_amd as egx
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egx_gp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(egx_[a-z0-9_]+)\s*\(", txt))
    lib = C.CDLL(egx._lib.LIB_PATH)
    bound = {s[0] for s in egx._lib.SIGNATURES}
    for name in ("egx_infill_create_mix", "egx_infill_eval_experts"):
        assert name in declared and hasattr(lib, name) and name in bound, name
    assert "egx_infill_surrogate" in txt
    assert egx._lib.load().egx_abi_version() == 2
    # the ctypes mirror has the C layout: pointer, int32 (+ padding), three pointers, double, int32 (+ padding)
    S = egx._lib.InfillSurrogate
    assert (S.experts.offset, S.n_experts.offset, S.weights.offset, S.means.offset, S.precisions_chol.offset,
            S.heaviside_factor.offset, S.smooth.offset, C.sizeof(S)) == (0, 8, 16, 24, 32, 40, 48, 56)
    assert hasattr(egx.InfillObjective, "expert_parts")


def test_mix_driver_and_cpp_wrapper_compile(tmp_path):
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{inc}",
                    os.path.join(ROOT, "tests", "c_host", "infill_mix_driver.c")], check=True)
    cpp = tmp_path / "t.cpp"
    cpp.write_text('#include "egx_gp.hpp"\n'
                   'int use(egobox::GaussianProcess &gp) { egobox::InfillSurrogate s; s.experts = {&gp, &gp}; s.weights = {0.5, 0.5};\n'
                   '  s.smooth = false; egobox::InfillObjective o({s}, {}, EGX_INFILL_EI, 0.0); double x[1] = {0.0};\n'
                   '  return (int)o.value(x, 1).size() + (int)o.eval_experts(0, x, 1).probas.size(); }\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{inc}", str(cpp)], check=True)


def test_mixtures_are_refused_by_name_without_touching_the_device():
    """What Python checks before the library is asked: rank count, the mixture's type, the experts' type."""
    import egobox_amd as egx
    from egobox_amd.moe import GaussianMixture, GpMixture
    gmx = GaussianMixture([0.5, 0.5], [[0.0], [1.0]], [[[1.0]], [[1.0]]])
    experts = [_Expert(0.0, 1.0, np.zeros(1), np.zeros(1))] * 2
    with pytest.raises(egx.InvalidValueError, match="ranks"):
        egx.InfillObjective(GpMixture([None, None], gmx, "smooth", rank=0, world=2))
    with pytest.raises(egx.InvalidValueError, match="surrogate 0 expert 0"):
        egx.InfillObjective(GpMixture(experts, gmx, "smooth"))
    with pytest.raises(egx.InvalidValueError, match="GaussianMixture"):
        egx.InfillObjective(GpMixture(experts, _Gmx(np.array([0.5, 0.5]), np.zeros((2, 1))), "hard"))


def test_create_mix_refuses_bad_arguments_before_the_device_is_touched():
    import egobox_amd as egx
    L = egx._lib
    lib = L.load()
    h = C.c_void_p()
    assert lib.egx_infill_create_mix(None, None, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and not h
    assert lib.egx_infill_create_mix(None, (L.InfillSurrogate * 1)(), None, 0, None) == L.ERR_INVALID_VALUE
    s = (L.InfillSurrogate * 2)()  # zeroed: no experts
    assert lib.egx_infill_create_mix(None, s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and not h
    assert b"surrogate 0" in lib.egx_last_error()
    assert lib.egx_infill_create_mix(None, s, None, 1, C.byref(h)) == L.ERR_INVALID_VALUE  # a constraint without tolerances
    arr = (C.c_void_p * 2)(None, None)
    s[0].experts, s[0].n_experts, s[0].heaviside_factor = arr, 2, 1.0
    assert lib.egx_infill_create_mix(None, s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE and not h
    assert b"surrogate 0 expert 0 is NULL" in lib.egx_last_error()
    cfg = L.InfillConfig()
    lib.egx_infill_config_default(C.byref(cfg))
    cfg.criterion = 9
    assert lib.egx_infill_create_mix(C.byref(cfg), s, None, 0, C.byref(h)) == L.ERR_INVALID_VALUE
    assert lib.egx_infill_eval_experts(None, 0, None, 0, None, None, None, None, None, None) == L.ERR_INVALID_VALUE
