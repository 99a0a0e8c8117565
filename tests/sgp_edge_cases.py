"""The edge table of the sparse GP's forward path (tests/test_sgp_edges_cpu.py, tests/test_gpu_sgp_edges.py): rows
(n, nz, d, theta, h), the data of tests/test_sgp_gpu.py's _problem with seed = n and noise = 0.05, sigma2 = 0.9, noise variance
0.02, every row under all four correlations and both methods.  With kTile = 128: n_pad = round_up(n, 128), z_pad = round_up(nz, 128),
zext = z_pad + 128 (the right-hand-side row block that rides through the second factorisation), the Gram product contracts over
n_pad in splits (launch_gram_lower).  What each row reaches is beside it; the CPU file checks, on the oracle alone, that every
row is one the oracle can vouch for, and that the two `gram-` rows still produce the splits they are here for."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sgp_kpls_cases as KC  # noqa: E402
from test_sgp_surrogate_cpu import KINDS, problem  # noqa: E402

SIGMA2, NOISE = 0.9, 0.02
NUGGET = 100.0 * np.finfo(float).eps
T3 = np.array([1.3, 0.8, 1.1])
T4 = 1.5 * np.array([1.3, 0.8, 1.1, 1.3])
KTILE = 128
# id: (n, nz, d, theta, h) -- h: columns of the KPLS weights, None without
CASES = {
    "n2-nz1": (2, 1, 1, np.array([1.0]), None),         # smallest legal handle: all but one row and one column is padding
    "nz1": (130, 1, 2, np.array([1.3, 0.8]), None),     # one inducing point, 127 padded columns, two row tiles
    "n128": (128, 40, 3, T3, None),                     # no padded training row
    "A": (130, 70, 3, T3, None),                        # shape A of tests/test_gpu_sgp_grad.py
    "nz128": (300, 128, 4, T4, None),                   # nz = z_pad: no padded inducing column, zext = 256
    "nz129": (300, 129, 4, T4, None),                   # one column into the second 128-block of both factorisations
    "nz-eq-n": (129, 129, 3, 3.0 * T3, None),           # nz = n: every training point is an inducing point
    "nz256": (600, 256, 5, np.full(5, 2.5), None),      # two full Cholesky blocks
    "nz257": (600, 257, 5, np.full(5, 2.5), None),      # ... and one column into a third (z_pad = 384, zext = 512)
    "gram-uneven": (1100, 40, 3, T3, None),             # n_pad = 1152: two K splits of 640 and 512
    "gram-fewer": (3100, 40, 3, T3, None),              # n_pad = 3200: gram_nsplit says 6, the launch runs 5
    "d64": (200, 20, 64, np.full(64, 0.25), None),      # last dimension of the first staging chunk (k_cross_corr / k_predict_mean)
    "d65": (200, 20, 65, np.full(65, 0.25), None),      # first dimension of the second
    # hcols > 1 (Matern) through the same forward path.  theta = [1.3, 0.8] puts 129 points projected onto two directions at
    # cond(R_zz) = 1.4e9 under the squared exponential, beyond what the oracle can vouch for; twice that: 4.0e5
    "kpls": (300, 129, 4, 2.0 * np.array([1.3, 0.8]), 2),
}
M_FORWARD = 131                                         # one full tile of queries plus three rows
M_COUNTS = (1, 16, 17, 127, 128, 129, 256, 257)         # on the nz129 model; 16 is the last size of the few-query route
CHUNK = 65536                                           # queries per chunk of sgp_query
M_CHUNK = (CHUNK, CHUNK + 1, CHUNK + 129)               # on the A model: one chunk, a second of one row, a second of two tiles
# a row's query seed: changed (never the 5 % cap) where too many queries of a set sit on the variance clamp
QUERY_SEED = {}


def round_up(v, m):
    return (v + m - 1) // m * m


def pads(cid):
    """(n_pad, z_pad, zext) of a row, as egx_sgp_create computes them."""
    n, nz = CASES[cid][:2]
    z_pad = round_up(nz, KTILE)
    return round_up(n, KTILE), z_pad, z_pad + KTILE


def gram_nsplit(rows, k):
    """kernels_chol.hip: the number of K splits the scratch of the Gram product is sized for."""
    nt = rows // 64
    tiles = nt * (nt + 1) // 2
    return max(1, min((2048 + tiles - 1) // tiles, max(k // 512, 1)))


def gram_splits(rows, k):
    """launch_gram_lower: the lengths of the K splits it launches (kc rounded up to 128, the count recomputed after that)."""
    nsplit = gram_nsplit(rows, k)
    kc = round_up((k + nsplit - 1) // nsplit, 128)
    nsplit = (k + kc - 1) // kc
    return tuple(min(kc, k - s * kc) for s in range(nsplit))


_data, _ref, _xq = {}, {}, {}


def data(cid):
    """(x, y, z, w) of a row, computed once; w is None without KPLS weights."""
    if cid not in _data:
        n, nz, d, _, h = CASES[cid]
        _data[cid] = problem(n, nz, d, seed=n) + (None if h is None else KC.weights(d, h),)
    return _data[cid]


def theta(cid):
    return CASES[cid][3]


def oracle(cid, corr, method):
    """The row's SparseGpOracle, built once and shared by every test that needs it."""
    from oracle import sgp_oracle as S
    key = (cid, corr, method)
    if key not in _ref:
        x, y, z, w = data(cid)
        _ref[key] = S.SparseGpOracle(x, y, z, theta(cid), SIGMA2, NOISE, corr=KINDS[corr], method=[S.FITC, S.VFE][method], w_star=w)
    return _ref[key]


def queries(cid, m):
    """The first m queries of the row's set, uniform in [-1, 1]^d like the training inputs."""
    key = (cid, m)
    if key not in _xq:
        _xq[key] = np.random.default_rng(QUERY_SEED.get(cid, 9)).random((m, CASES[cid][2])) * 2 - 1
    return _xq[key]


def raw_variance(ref, xq):
    """sigma2 - kx^T W kx before the clamp at 1e-15, as tests/test_sgp_surrogate_cpu.py::analytic_gradients forms it."""
    from oracle import sgp_oracle as S
    kx = S.compute_k(ref.corr, np.atleast_2d(xq), ref.z, ref.w_star, ref.theta, ref.sigma2)
    return ref.sigma2 - ((kx @ ref.w_inv) * kx).sum(axis=1)


def unsure(var_raw):
    """Queries whose clamp decision rounding may turn: the rule of test_few_queries_equal_rows_of_a_large_batch."""
    return np.abs(var_raw - 1e-15) < 1e-7 * SIGMA2
