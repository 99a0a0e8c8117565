"""Helper of the theta-gradient tests (not a test): the table of shapes at which the likelihood's theta-gradient branches
(egobox_amd/csrc/kernels_corr.hip k_grad_accum / launch_grad_accum, gp_host.hip make_coef, gp_fit.hip grad_chain_rule) and the
recipe of a case.  Imports without the library.

tests/test_theta_grad_oracle_cpu.py checks on the oracle alone that every row is well posed (the smallest pivot of the factor in
[1e-2, 0.98], max |g| >= 1e-3); tests/test_gpu_theta_grad.py runs the library on every row.

What a row reaches (MODE / DK: the compiled form of k_grad_accum; nout: d when one coefficient column, h for KPLS + Matern):
    A  w = I, d = 3, n = 5 .. 129     MODE 2, DK 8; a single tile, exact 64-tiles, one valid row in the last tile (i < n mask)
    B  w = I, n = 130, d = 1 .. 129   MODE 2; DK 8 (d <= 8), 16 (9 .. 16), 32 (>= 17); two output chunks read from the slabs of
                                      pass 1 (33 .. 64: o0 = 32, base = 0); a full 64-dimension stage (64); a second and a third
                                      stage of one dimension and a last output chunk of one (65, 97 = 3 * 32 + 1, 129 = 2 * 64 + 1)
    C  w = I, theta[1] = 0.0          MODE 1 (raw coefficients) at DK 8, at two chunks from the slabs, at d > 64
    D  w_star (d, h)                  Matern: MODE 0 at DK 8 / 16 / 32, two output chunks (h = 33), d > 64 restaged with h <= 8
                                      and h > 8, and with zeros in w_star the wa != 0 skip; sq-exp / abs-exp: the collapse to one
                                      coefficient per input and the host chain rule, and with a zero row of w_star MODE 1 and
                                      the chain rule's coef > 0 guard
    E  linear, quadratic trend        gamma and sigma2 through the generalised least squares"""
import collections

import numpy as np

from oracle import gp_oracle as GO

KINDS = [GO.SQEXP, GO.ABSEXP, GO.MATERN32, GO.MATERN52]
MEANS = [GO.CONSTANT, GO.LINEAR, GO.QUADRATIC]
SQEXP, ABSEXP, MATERN32, MATERN52 = range(4)

PIVOT_WINDOW = (1e-2, 0.98)  # of the oracle's factor: below it 1e-6 means nothing, above it R = I and the gradient underflows
MIN_GRAD = 1e-3              # max |g| of a row: the test must see something
N_DEFAULT = 130              # three 64-tiles, the last with two valid rows

#: h None: w = I.  zero_component: theta[1] = 0.0 exactly.  w_zero_row: w_star[1, :] = 0 and w_star[0, h - 1] = 0.
Case = collections.namedtuple("Case", "name n d h mean corr zero_component w_zero_row")

KPLS_SHAPES = [(6, 3), (12, 9), (20, 17), (40, 33), (70, 3), (70, 33)]
KPLS_ZERO_SHAPES = [(6, 3), (40, 33), (70, 3)]


def _table():
    rows = []
    for corr in range(4):
        k = ("sqexp", "absexp", "matern32", "matern52")[corr]
        for n in (5, 63, 64, 65, 128, 129):
            rows.append(Case(f"A-n{n}-{k}", n, 3, None, 0, corr, False, False))
        for d in (1, 8, 9, 16, 17, 32, 33, 64, 65, 97, 129):
            rows.append(Case(f"B-d{d}-{k}", N_DEFAULT, d, None, 0, corr, False, False))
        for d in (6, 40, 70):
            rows.append(Case(f"C-d{d}-{k}", N_DEFAULT, d, None, 0, corr, True, False))
        for d, h in KPLS_SHAPES:
            rows.append(Case(f"D-d{d}-h{h}-{k}", N_DEFAULT, d, h, 0, corr, False, False))
        for d, h in KPLS_ZERO_SHAPES:
            rows.append(Case(f"D-d{d}-h{h}-wzero-{k}", N_DEFAULT, d, h, 0, corr, False, True))
        for mean in (1, 2):
            rows.append(Case(f"E-{MEANS[mean].lower()}-{k}", N_DEFAULT, 3, None, mean, corr, False, False))
    return rows


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _ramp(k):
    return 1.0 + 0.3 * np.arange(k) / max(1, k - 1)


# sq-exp with weights: theta = c / sqrt(h) * ramp, c by shape (between 1 and 3; chosen on the oracle's pivots)
_SQEXP_KPLS_C = {(6, 3): 3.0, (12, 9): 1.5, (20, 17): 1.5, (40, 33): 1.0, (70, 3): 1.0, (70, 33): 1.0}


def case_theta(c):
    """The row's theta (h, or d when w = I): scales that keep the factor's pivots inside PIVOT_WINDOW at the row's shape
    (scanned on the oracle; with one scale for all d the smooth kernels are singular at d = 1 and every kernel's R is the
    identity to a per cent at d >= 32)."""
    d = c.d
    if c.h is None:
        base = default_theta(d)
        if d == 1:
            th = np.array([40.0])  # 130 points on a line: neighbours 0.03 apart after normalisation
        elif c.corr == SQEXP:
            th = base * (4.0 if d <= 17 else 2.0) * _ramp(d)
        elif c.corr == ABSEXP and d >= 16:
            th = _ramp(d) / d
        else:
            th = base * 2.0 * _ramp(d)
    else:
        h = c.h
        if c.corr == SQEXP:
            th = _SQEXP_KPLS_C[(d, h)] / np.sqrt(h) * _ramp(h)
        elif c.corr == ABSEXP:
            th = 2.0 / (h * np.sqrt(d)) * _ramp(h)
        else:
            th = 6.0 / (h * np.sqrt(d)) * _ramp(h)
    if c.zero_component:
        th[1] = 0.0
    return th


def case_weights(c):
    """w_star (d, h) with unit columns, seeded by the shape; None when w = I"""
    if c.h is None:
        return None
    w = np.random.default_rng(100 * c.d + c.h).standard_normal((c.d, c.h))
    if c.w_zero_row:
        w[1, :] = 0.0
        w[0, c.h - 1] = 0.0
    return w / np.linalg.norm(w, axis=0)


def case_data(c):
    """(x, y): the numbers of workload.make_training_set(n, d, seed = 1000 + d), drawn by the oracle's copy of the generator"""
    x = GO.lhs_classic(c.n, c.d, 1000 + c.d)
    return x, GO.griewank(x)


def default_theta(d):
    """workload.default_theta"""
    return np.full(d, 0.5 / np.sqrt(d))


#: one evaluation: a label, the training set, theta, the codes of trend and kernel, w_star or None
Member = collections.namedtuple("Member", "label x y theta mean corr w")
_REFS = {}


def member(c):
    x, y = case_data(c)
    return Member(c.name, x, y, case_theta(c), c.mean, c.corr, case_weights(c))


def reference(m):
    """(likelihood, gradient, smallest pivot) of a row of the table or of a Member on the oracle, computed once per label
    and read-only"""
    import theta_grad_oracle as TO
    if isinstance(m, Case):
        m = member(m)
    if m.label not in _REFS:
        lk, g, piv = TO.likelihood_grad(m.x, m.y, m.theta, MEANS[m.mean], KINDS[m.corr], w_star=m.w)
        g.setflags(write=False)
        _REFS[m.label] = (lk, g, piv)
    return _REFS[m.label]


# ---- the entry points that carry the values into the lock-step paths ---------------------------------------------------------
def mode0_batch():
    """Four thetas of ONE handle on a MODE 0 shape (KPLS + Matern-5/2, d = 12, h = 9: DK 16): likelihood_grad_batch"""
    c = BY_NAME["D-d12-h9-matern52"]
    x, y = case_data(c)
    return [Member(f"batch-{c.name}-x{s}", x, y, case_theta(c) * s, c.mean, c.corr, case_weights(c)) for s in (1.0, 1.1, 0.9, 1.2)]


def mixed_group():
    """A group of four (n = 130, d = 6, Matern-5/2, a training set each) whose member 2 has theta[1] = 0.0: the raw form
    between prescaled neighbours in one likelihood_grad_multi"""
    c = BY_NAME["C-d6-matern52"]
    out = []
    for j in range(4):
        x = GO.lhs_classic(c.n, c.d, 2000 + j)
        th = default_theta(c.d) * 2.0 * _ramp(c.d) * (1.0 + 0.1 * j)
        if j == 2:
            th[1] = 0.0
        out.append(Member(f"group-member{j}", x, GO.griewank(x), th, c.mean, c.corr, None))
    return out


def companions():
    """The sq-exp collapse at (40, 33) and its twin with a zero row of w_star, each a handle of its own with a batch of two
    thetas: [dense x 2, zero-row x 2]"""
    out = []
    for name in ("D-d40-h33-sqexp", "D-d40-h33-wzero-sqexp"):
        c = BY_NAME[name]
        x, y = case_data(c)
        out += [Member(f"companions-{name}-x{s}", x, y, case_theta(c) * s, c.mean, c.corr, case_weights(c)) for s in (1.0, 1.1)]
    return out
