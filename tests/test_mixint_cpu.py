"""CPU checks of the mixed-integer helpers: the C ABI (egx_mixint_*, through egobox_amd.mixint) and egobox_amd/csrc/mixint.h
itself (tests/c_host/mixint_test.cpp, compiled with g++ -fsanitize=address,undefined and run as its own process) against
tests/mixint_oracle.py -- random rows of two specs, the tie and edge rows, the reference's known answers
(tests/golden/mixint_kat.json), every validation error, and the declarations of the feature."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mixint_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egobox_amd", "csrc")
SPECS = {"A": MO.SPEC_A, "B": MO.SPEC_B}


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(ROOT, "tests", "golden", "mixint_kat.json")) as f:
        return json.load(f)


def _spec(js):
    return [tuple(t) for t in js]


def _same(a, b):
    """bit equality up to the payload of a NaN: values, NaN positions and the sign of every zero"""
    a, b = np.asarray(a), np.asarray(b)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.signbit(a), np.signbit(b))


def _rows(name, seed=0, m=200):
    """random rows beyond the limits on both sides, the edge rows, and rows with non-finite coordinates"""
    spec = SPECS[name]
    rng = np.random.default_rng(seed)
    lim = MO.as_continuous_limits(spec)
    w = lim[:, 1] - lim[:, 0]
    x = np.vstack([lim[:, 0] - 0.2 * w + 1.4 * w * rng.random((m, lim.shape[0])), MO.edge_rows(spec, rng)])
    bad = x[:12].copy()
    for i, v in enumerate([np.nan, np.inf, -np.inf] * 4):
        bad[i, (7 * i + i // 3) % x.shape[1]] = v
    bad[3, :] = np.nan
    return np.vstack([x, bad])


# ---- the C ABI against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_cabi_matches_the_oracle(egx, name):
    spec, xt = SPECS[name], MO.xtypes(egx, SPECS[name])
    x = _rows(name)
    assert egx.mixint.unfolded_dim(xt) == MO.unfolded_dim(spec) == {"A": 6, "B": 70}[name]
    _same(egx.as_continuous_limits(xt), MO.as_continuous_limits(spec))
    cast = egx.cast_to_discrete_values(xt, x)
    _same(cast, MO.cast(spec, x))
    _same(egx.cast_to_discrete_values(xt, cast), cast)  # idempotent
    _same(egx.fold_with_enum_index(xt, x), MO.fold(spec, x))
    disc = egx.to_discrete_space(xt, x)
    _same(disc, MO.to_discrete(spec, x))
    ok = np.isfinite(disc).all(axis=1)
    assert ok.sum() >= 200
    unf = egx.unfold_with_enum_mask(xt, disc[ok])
    _same(unf, MO.unfold(spec, disc[ok]))
    _same(egx.to_continuous_space(xt, disc[ok]), unf)
    _same(unf, cast[ok])  # unfold(fold(cast x)) = cast x
    assert not np.array_equal(cast[ok], x[ok])  # (the cast does something on these rows)


def test_tie_and_edge_rows(egx):
    X = egx.XType
    ints = np.array([[0.5], [-0.5], [1.5], [-1.5], [2.5], [-0.3], [2.0 ** 53], [0.49999999999999994], [np.nan], [np.inf], [-np.inf]])
    got = egx.cast_to_discrete_values([X.Int(-10, 10)], ints)[:, 0]
    _same(got, [1.0, -1.0, 2.0, -2.0, 3.0, -0.0, 2.0 ** 53, 0.0, np.nan, np.inf, -np.inf])
    assert np.signbit(got[5]) and not np.signbit(got[7])
    _same(got, MO.cast([("int", -10, 10)], ints)[:, 0])
    assert np.round(2.5) == 2.0  # half-to-even: why the oracle does not use np.round
    ords = np.array([[2.0], [4.0], [6.5], [-40.0], [1e9], [np.nan], [np.inf], [-np.inf]])
    _same(egx.cast_to_discrete_values([X.Ord([1, 3, 5, 8])], ords)[:, 0], [1.0, 3.0, 5.0, 1.0, 8.0, np.nan, np.inf, -np.inf])
    _same(egx.cast_to_discrete_values([X.Ord([5, 1, 3])], [[2.0], [4.0]])[:, 0], [1.0, 5.0])  # first in LIST order
    en = np.array([[0.7, 0.2, 0.7], [0.4, 0.4, 0.4], [0.1, 0.9, 0.9], [0.1, np.nan, 0.3], [0.1, np.inf, 0.3], [-np.inf, 0.0, 0.0]])
    hot = egx.cast_to_discrete_values([X.Enum(3)], en)
    _same(hot[:3], [[1, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert np.isnan(hot[3:]).all()
    _same(egx.fold_with_enum_index([X.Enum(3)], en)[:, 0], [0, 0, 1, np.nan, np.nan, np.nan])
    _same(egx.cast_to_discrete_values([X.Enum(4)], [[0.9, 0.1, 0.9, 0.9]]), [[1, 0, 0, 0]])  # three equal maxima


def test_reference_known_answers(egx, kat):
    # test_mixint_ffact: the 4 x 4 grid linspace(-10, 10, 4)^2 under [Float, Int]
    spec = _spec(kat["ffact_spec"])
    g = np.linspace(-10.0, 10.0, 4)
    grid = np.array([[a, b] for a in g for b in g])
    got = egx.to_discrete_space(MO.xtypes(egx, spec), grid)
    np.testing.assert_allclose(got, np.array(kat["ffact_expected"]), rtol=0, atol=1e-6)
    _same(got, MO.to_discrete(spec, grid))
    # test_mixint_lhs' ten rows: discrete points survive the round trip through the continuous space
    spec = _spec(kat["spec_a"])
    assert spec == MO.SPEC_A
    xt, rows = MO.xtypes(egx, spec), np.array(kat["lhs_rows"])
    cont = egx.to_continuous_space(xt, rows)
    assert cont.shape == (10, 6)
    _same(egx.to_discrete_space(xt, cont), rows)
    _same(egx.to_continuous_space(xt, egx.to_discrete_space(xt, cont)), cont)
    _same(egx.as_continuous_limits(xt), np.array(kat["spec_a_limits"]))


def test_lhs_sampling_is_admissible(egx):
    xt = MO.xtypes(egx, MO.SPEC_A)
    ctx = egx.MixintContext(xt)
    assert ctx.get_unfolded_dim() == 6
    s = ctx.create_lhs_sampling(seed=0).sample(10)
    assert s.shape == (10, 4)
    assert np.all((s[:, 0] >= -10) & (s[:, 0] <= 10)) and set(s[:, 1]) <= {0.0, 1.0, 2.0}
    assert np.all(s[:, 2] == np.round(s[:, 2])) and set(s[:, 3]) <= {1.0, 3.0, 5.0, 8.0}
    _same(s, ctx.create_lhs_sampling(seed=0).sample(10))


# ---- validation: the code and a message that names the entry, with no device touched ----------------------------------------
def _raw(kind, n=0, lo=0.0, hi=0.0, values=None):
    from egobox_amd import _lib as L
    t = L.XTypeC()
    t.kind, t.n, t.lo, t.hi = kind, n, lo, hi
    keep = None
    if values is not None:
        keep = np.ascontiguousarray(values, dtype=np.float64)
        t.values = L.dptr(keep)
    return t, keep


@pytest.mark.parametrize("entry, word", [
    (dict(kind=7), "unknown kind"),
    (dict(kind=2, n=0, values=[1.0]), "Ord"),
    (dict(kind=2, n=2, values=[1.0, np.nan]), "not finite"),
    (dict(kind=2, n=2, values=[1.0, np.inf]), "not finite"),
    (dict(kind=3, n=0), "Enum"),
    (dict(kind=0, lo=1.0, hi=0.0), "lo > hi"),
    (dict(kind=1, lo=3.0, hi=-3.0), "lo > hi"),
])
def test_validation_errors_name_the_entry(egx, entry, word):
    from egobox_amd import _lib as L
    lib = L.load()
    good, _ = _raw(0, lo=0.0, hi=1.0)
    bad, keep = _raw(**entry)
    arr = (L.XTypeC * 2)(good, bad)
    d = C.c_int64(-1)
    x, out = np.zeros((1, 8)), np.zeros((1, 8))
    for call in (lambda: lib.egx_mixint_unfolded_dim(arr, 2, C.byref(d)),
                 lambda: lib.egx_mixint_continuous_limits(arr, 2, L.dptr(out)),
                 lambda: lib.egx_mixint_unfold(arr, 2, L.dptr(x), 1, L.dptr(out)),
                 lambda: lib.egx_mixint_fold(arr, 2, L.dptr(x), 1, L.dptr(out)),
                 lambda: lib.egx_mixint_cast(arr, 2, L.dptr(x), 1, L.dptr(out)),
                 lambda: lib.egx_mixint_to_discrete(arr, 2, L.dptr(x), 1, L.dptr(out))):
        assert call() == L.ERR_INVALID_VALUE
        msg = lib.egx_last_error().decode()
        assert "xtype 1" in msg and word in msg, msg
    assert d.value == -1
    # the typed mixture calls validate before they look for a device
    w, mu, pc = np.array([0.5, 0.5]), np.zeros((2, 2)), np.stack([np.eye(2)] * 2)
    rc = lib.egx_gmx_predict_probas_mixint(-1, L.dptr(w), L.dptr(mu), L.dptr(pc), 2, 2, 1.0, L.dptr(x), 1, L.dptr(out), arr, 2)
    assert rc == L.ERR_INVALID_VALUE and "xtype 1" in lib.egx_last_error().decode()


def test_dimension_and_cap_errors(egx):
    from egobox_amd import _lib as L
    lib = L.load()
    X = egx.XType
    with pytest.raises(L.InvalidValueError, match="row 2, xtype 1"):
        egx.unfold_with_enum_mask([X.Float(0, 1), X.Enum(3)], [[0.1, 0], [0.2, 2.9], [0.3, 3.0]])
    for v in (-1.0, np.nan, np.inf):
        with pytest.raises(L.InvalidValueError, match="xtype 0"):
            egx.unfold_with_enum_mask([X.Enum(2)], [[v]])
    with pytest.raises(L.InvalidValueError):
        egx.cast_to_discrete_values([X.Float(0, 1), X.Enum(3)], np.zeros((2, 3)))  # d = 4
    with pytest.raises(L.InvalidValueError, match="nx >= 1"):
        egx.mixint.unfolded_dim([])
    # the typed mixture call: the spec must unfold to d
    arr, nx, keep = egx.mixint._c_xtypes([X.Float(0, 1), X.Enum(3)])
    w, mu, pc, x, out = np.array([0.5, 0.5]), np.zeros((2, 2)), np.stack([np.eye(2)] * 2), np.zeros((1, 2)), np.zeros((1, 2))
    rc = lib.egx_gmx_predict_probas_derivatives_mixint(-1, L.dptr(w), L.dptr(mu), L.dptr(pc), 2, 2, 1.0, L.dptr(x), 1, L.dptr(out), arr, nx)
    assert rc == L.ERR_INVALID_VALUE and "unfold to 4 columns, expected 2" in lib.egx_last_error().decode()
    # the cap on Ord values
    txt = open(os.path.join(ROOT, "include", "egx_gp.h")).read()
    cap = int(re.search(r"#define EGX_MIXINT_MAX_ORD_VALUES (\d+)", txt).group(1))
    vals = np.arange(cap // 2 + 1, dtype=np.float64)
    assert egx.mixint.unfolded_dim([X.Ord(vals[:cap // 2]), X.Ord(vals[:cap // 2])]) == 2
    with pytest.raises(L.EgxError) as ei:
        egx.mixint.unfolded_dim([X.Ord(vals), X.Ord(vals)])
    assert ei.value.rc == L.ERR_UNSUPPORTED and "EGX_MIXINT_MAX_ORD_VALUES" in str(ei.value)


# ---- mixint.h itself, under the sanitizers, in a process of its own ---------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("mixint") / "mixint_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{CSRC}", os.path.join(ROOT, "tests", "c_host", "mixint_test.cpp"), "-o", str(out)], check=True)
    return str(out)


def _ask(exe, lines):
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rows = res.stdout.strip().splitlines()
    assert len(rows) == len(lines)
    return rows


def _fmt(row):
    return " ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in row)


@pytest.mark.parametrize("name", ["A", "B"])
def test_header_under_sanitizers_matches_the_oracle(exe, name):
    spec = SPECS[name]
    x = _rows(name, seed=5, m=40)
    for op, ref in (("cast", MO.cast(spec, x)), ("fold", MO.fold(spec, x)), ("disc", MO.to_discrete(spec, x))):
        rows = _ask(exe, [f"{name} {op} {_fmt(r)}" for r in x])
        _same(np.array([[float(t) for t in ln.split()] for ln in rows]), ref)
    disc = MO.to_discrete(spec, x)
    disc = disc[np.isfinite(disc).all(axis=1)]
    assert disc.shape[0] >= 40
    rows = _ask(exe, [f"{name} unfold {_fmt(r)}" for r in disc])
    _same(np.array([[float(t) for t in ln.split()] for ln in rows]), MO.unfold(spec, disc))


def test_header_under_sanitizers_refuses_bad_enum_indices(exe):
    assert _ask(exe, ["A unfold 0 3 0 1", "A unfold 0 nan 0 1", "A unfold 0 -1 0 1", "A unfold 0 2.9 0 1"])[:3] == ["bad 1"] * 3


# ---- the declarations of the feature ------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols(egx, tmp_path):
    from egobox_amd import _lib as L
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "egx_gp.h")).read(), flags=re.S)
    names = ["egx_mixint_unfolded_dim", "egx_mixint_continuous_limits", "egx_mixint_unfold", "egx_mixint_fold", "egx_mixint_cast",
             "egx_mixint_to_discrete", "egx_gp_set_xtypes", "egx_gp_get_xtypes", "egx_gmx_predict_probas_mixint",
             "egx_gmx_predict_probas_derivatives_mixint"]
    typed = {n for n, _, _ in L.SIGNATURES}
    lib = L.load()
    for n in names:
        assert re.search(rf"\bint32_t {n}\(", txt), n
        assert n in typed and hasattr(lib, n), n
    assert all(k in txt for k in ("EGX_XTYPE_FLOAT = 0", "EGX_XTYPE_INT = 1", "EGX_XTYPE_ORD = 2", "EGX_XTYPE_ENUM = 3"))
    for name in ("XType", "MixintContext", "MixintGpMixture", "MixintGpMixtureParams", "as_continuous_limits", "to_continuous_space",
                 "to_discrete_space", "cast_to_discrete_values", "fold_with_enum_index", "unfold_with_enum_mask"):
        assert hasattr(egx, name), name
    assert hasattr(egx.GpHandle, "set_xtypes") and hasattr(egx.GpHandle, "xtypes") and hasattr(egx.GaussianProcess, "set_xtypes")
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c", os.path.join(inc, "egx_gp.h")],
                   check=True)
    cpp = tmp_path / "t.cpp"
    cpp.write_text('#include "egx_gp.hpp"\n'
                   'int use(egobox::GaussianProcess &gp) { std::vector<egobox::XType> xt = {egobox::XType::Float(0, 1), egobox::XType::Enum(3),\n'
                   '  egobox::XType::Int(-3, 3), egobox::XType::Ord({1.0, 3.0})}; gp.set_xtypes(xt); double x[6] = {0}, f[4] = {0};\n'
                   '  return (int)(egobox::mixint::unfolded_dim(xt) + egobox::mixint::as_continuous_limits(xt).size() +\n'
                   '    egobox::mixint::cast_to_discrete_values(xt, x, 1).size() + egobox::mixint::to_discrete_space(xt, x, 1).size() +\n'
                   '    egobox::mixint::fold_with_enum_index(xt, x, 1).size() + egobox::mixint::to_continuous_space(xt, f, 1).size() +\n'
                   '    egobox::mixint::unfold_with_enum_mask(xt, f, 1).size()); }\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", f"-I{inc}", str(cpp)], check=True)
