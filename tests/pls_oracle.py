"""Oracles and cases of the PLS-rotation tests (tests/test_pls_cpu.py, tests/test_gpu_pls.py); a helper, not a test module.

Three statements of the x rotations W (P^T W)^-1 of a PLS1 regression on centred, unit-variance (ddof = 1) columns:
  nipals_longdouble   the NIPALS recursion of egobox_amd/kpls.py on the data in np.longdouble: the reference of the rule
  kpls.pls_rotations  the host path of the package (float64 NIPALS)
  gram_form           a float64 numpy restatement of what the device path computes: means, centred Gram matrix of [x | y], the
                      deflation in d-space
and the error measure of the rule  e_dev <= 8 max(e_host, e_gram, 16 eps).
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
FACTOR = 8.0
FLOOR = 16.0 * EPS


def _inv_longdouble(a):
    """Gauss-Jordan with row pivoting (np.linalg has no extended precision)."""
    k = a.shape[0]
    a = a.astype(np.longdouble).copy()
    inv = np.eye(k, dtype=np.longdouble)
    for c in range(k):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        if p != c:
            a[[c, p]], inv[[c, p]] = a[[p, c]], inv[[p, c]]
        pv = a[c, c]
        a[c], inv[c] = a[c] / pv, inv[c] / pv
        for r in range(k):
            if r != c and a[r, c] != 0:
                f = a[r, c]
                a[r], inv[r] = a[r] - f * a[c], inv[r] - f * inv[c]
    return inv


def nipals_longdouble(x, y, k):
    """(d, k) float64 from an np.longdouble NIPALS; zeros where the response is constant (kpls.py's contract)."""
    x = np.asarray(x, dtype=np.float64).astype(np.longdouble)
    y = np.asarray(y, dtype=np.float64).reshape(-1).astype(np.longdouble)
    n, d = x.shape
    xm, ym = x.sum(axis=0) / n, y.sum() / n
    xc, yc = x - xm, y - ym
    xs = np.sqrt((xc * xc).sum(axis=0) / (n - 1))
    xs[xs == 0] = 1
    ys = np.sqrt((yc * yc).sum() / (n - 1))
    if ys <= 1e-12 * max(1.0, abs(float(ym))):
        return np.zeros((d, k))
    xk, yk = xc / xs, yc / ys
    w = np.zeros((d, k), dtype=np.longdouble)
    p = np.zeros((d, k), dtype=np.longdouble)
    for a in range(k):
        if np.all(np.abs(yk) < 10 * EPS):
            return np.zeros((d, k))
        wa = xk.T @ yk
        nrm = np.sqrt((wa * wa).sum())
        if nrm < EPS:
            return np.zeros((d, k))
        wa = wa / nrm
        t = xk @ wa
        tt = t @ t
        pa = xk.T @ t / tt
        qa = yk @ t / tt
        xk = xk - np.outer(t, pa)
        yk = yk - qa * t
        w[:, a], p[:, a] = wa, pa
    return np.asarray(w @ _inv_longdouble(p.T @ w), dtype=np.float64)


def gram_inputs(x, y):
    """float64: the scaled Gram matrix G (d, d), s (d) and y^T y of the standardised columns -- the inputs of csrc/pls_host.h"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, d = x.shape
    a = np.concatenate([x - x.mean(axis=0), (y - y.mean())[:, None]], axis=1)
    c = a.T @ a
    sd = np.sqrt(np.diag(c) / (n - 1))
    sd[sd == 0.0] = 1.0
    g = c / np.outer(sd, sd)
    return g[:d, :d].copy(), g[:d, d].copy(), float(g[d, d])


def gram_recursion(g, s, k):
    """float64 deflation in d-space: w = s / |s|, tt = w^T G w, p = G w / tt, s <- (I - p w^T)(s - |s| p), G <- (I - p w^T) G (I - w p^T)"""
    d = g.shape[0]
    g, s = g.copy(), s.copy()
    w = np.zeros((d, k))
    p = np.zeros((d, k))
    eye = np.eye(d)
    for a in range(k):
        nrm = np.linalg.norm(s)
        if nrm < EPS:
            return np.zeros((d, k))
        wa = s / nrm
        gw = g @ wa
        tt = wa @ gw
        pa = gw / tt
        s = (eye - np.outer(pa, wa)) @ (s - nrm * pa)
        g = (eye - np.outer(pa, wa)) @ g @ (eye - np.outer(wa, pa))
        w[:, a], p[:, a] = wa, pa
    return w @ np.linalg.inv(p.T @ w)


def gram_form(x, y, k):
    g, s, _ = gram_inputs(x, y)
    return gram_recursion(g, s, k)


def col_err(w, ref):
    """max over the columns of |w_col -+ ref_col|_inf / |ref_col|_inf, the better sign per column: the kernels read |w| or w^2"""
    w, ref = np.asarray(w, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    worst = 0.0
    for j in range(ref.shape[1]):
        scale = np.max(np.abs(ref[:, j]))
        if scale == 0.0:
            e = float(np.max(np.abs(w[:, j])))
        else:
            e = float(min(np.max(np.abs(w[:, j] - ref[:, j])), np.max(np.abs(w[:, j] + ref[:, j]))) / scale)
        worst = max(worst, e)
    return worst


def bound(e_host, e_gram):
    return FACTOR * max(e_host, e_gram, FLOOR)


# (name, n or the name of a plan-derived n, d, k, kind).  one / two / three: one chunk, two chunks with a ragged last one, three
# chunks, from egx_pls_get_plan; the small n: the K tail and the padding.  d + 1 on and off a 16-wide tile, y first or last in its
# tile; d = 64, 65, 130: one, two and three 64-wide blocks per side.
CASES = [
    ("one-d1", "one", 1, 1, "plain"),
    ("two-d3", "two", 3, 3, "plain"),
    ("three-d15", "three", 15, 4, "plain"),
    ("one-d16-full", "one", 16, 16, "plain"),
    ("two-d17", "two", 17, 2, "plain"),
    ("three-d64", "three", 64, 4, "plain"),
    ("two-d65", "two", 65, 4, "plain"),
    ("one-d130", "one", 130, 4, "plain"),
    ("n2", 2, 3, 1, "plain"),
    ("n5", 5, 3, 3, "plain"),
    ("n17", 17, 15, 2, "plain"),
    ("n127", 127, 16, 4, "plain"),
    ("n129-full", 129, 16, 16, "plain"),
    ("n129-d64", 129, 64, 1, "plain"),
    ("big-mean", "two", 17, 4, "bigmean"),
    ("const-column", "two", 16, 2, "constcol"),
    ("scales", "three", 15, 4, "scales"),
]
CONST_COLUMN = 5


def plan_n(which, d, plan):
    """n for "one" / "two" / "three" from the plan function (n, d) -> dict of egx_pls_get_plan"""
    cr = plan(2, d)["chunk_rows"]
    n = {"one": cr - 56, "two": cr + 44, "three": 2 * cr + 88}[which]
    want = {"one": 1, "two": 2, "three": 3}[which]
    p = plan(n, d)
    assert p["chunk_rows"] == cr and p["n_chunks"] == want, (which, d, p)
    assert n % p["chunk_rows"] != 0
    return n


_ROWS = []


def rows(plan):
    """[(name, n, d, k, kind, x, y, the long-double rotations, e_host, e_gram)] for CASES: computed once per process and shared,
    never modified by a test"""
    if not _ROWS:
        from egobox_amd import kpls
        for name, n, d, k, kind in CASES:
            n = plan_n(n, d, plan) if isinstance(n, str) else n
            x, y = make_case(name, n, d, k, kind)
            ref = nipals_longdouble(x, y, k)
            _ROWS.append((name, n, d, k, kind, x, y, ref, col_err(kpls.pls_rotations(x, y, k), ref), col_err(gram_form(x, y, k), ref)))
    return _ROWS


def make_case(name, n, d, k, kind):
    rng = np.random.default_rng(1000 * n + 10 * d + k)
    x = rng.standard_normal((n, d))
    beta = rng.standard_normal(d)
    y = x @ beta + 0.3 * np.sin(3.0 * x[:, 0]) + 0.1 * rng.standard_normal(n)
    if kind == "bigmean":  # mean ~ 1e8 std: a one-pass sum of squares loses everything
        x = 1e-3 * x + 1e5
    elif kind == "constcol":
        x[:, CONST_COLUMN] = 2.5
    elif kind == "scales":  # scales spread over 1e4 across the columns
        x = x * np.logspace(-2, 2, d)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)
