"""The shapes of the sparse KPLS tests (tests/test_sgp_kpls_cpu.py, tests/test_gpu_sgp_kpls.py): rows (n, nz, d, h), the data
of tests/test_gpu_sgp_grad.py's _problem (seed = n), weights w = default_rng(2).standard_normal((d, h)) / sqrt(d), sigma2 = 0.9,
noise = 0.02 and, per correlation, theta = the first value of the ladder 1, 0.5, 0.25, 0.1, 0.05, 0.02, 0.01, ... (halving on)
at which the median entry of R_nz is at least 0.2 -- so that the weights matter: with a theta far too large every
correlation is 0 and every gradient with it."""
import numpy as np

import sgp_kpls_oracle as KO

SIGMA2, NOISE = 0.9, 0.02
NUGGET = 100.0 * np.finfo(float).eps
# id: (n, nz, d, h) -- what each reaches in the two gradient kernels
CASES = {
    "a": (130, 20, 12, 2),   # two row tiles (one partial), one partial column tile, h + 1 = 3 outputs in DK = 4
    "b": (270, 70, 70, 3),   # d > 64: a second staging chunk, restaged in pass 2; five row tiles in runs of 2, 2, 1; two column tiles
    "c": (130, 70, 9, 5),    # h + 1 = 6 outputs: an 8-wide output chunk
    "d": (200, 40, 20, 17),  # h + 1 = 18 outputs: two 16-wide output chunks
}
LADDER = [1.0, 0.5, 0.25, 0.1, 0.05, 0.02] + [0.01 / 2 ** i for i in range(12)]


def problem(n, nz, d, seed=0, noise=0.05):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d)) * 2 - 1
    y = np.sin(3 * x[:, 0]) + 0.5 * np.cos(2 * x[:, -1]) + noise * rng.standard_normal(n)
    z = x[rng.permutation(n)[:nz]].copy()
    return x, y, z


def weights(d, h):
    """The (d, h) KPLS weights of every case here (and of the `kpls` row of tests/sgp_edge_cases.py)."""
    return np.random.default_rng(2).standard_normal((d, h)) / np.sqrt(d)


_data, _theta = {}, {}


def data(cid):
    """(x, y, z, w) of a case, computed once."""
    if cid not in _data:
        n, nz, d, h = CASES[cid]
        _data[cid] = problem(n, nz, d, seed=n) + (weights(d, h),)
    return _data[cid]


def theta(cid, corr):
    """(h,) the case's theta for correlation `corr` (0 .. 3): one ladder value for every component."""
    if (cid, corr) not in _theta:
        x, _, z, w = data(cid)
        for t in LADDER:
            th = np.full(w.shape[1], t)
            if np.median(KO.corr(corr, x, z, w, th)) >= 0.2:
                break
        else:
            raise AssertionError(f"case {cid}, correlation {corr}: no theta of the ladder reaches a median of 0.2")
        _theta[cid, corr] = th
    return _theta[cid, corr]
