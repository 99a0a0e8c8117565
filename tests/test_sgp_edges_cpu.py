"""The edge table of the sparse GP's forward path (tests/sgp_edge_cases.py), the part that needs no GPU: for every row,
correlation and method the CPU oracle must be ALLOWED to judge the library at the bars of tests/test_gpu_sgp_edges.py
(likelihood 1e-8, predictions 1e-6) -- a failure there is then the kernels', not the test's:
  * cond(R_zz + nugget / sigma2 I) <= 1e8, the bound of tests/test_gpu_sgp_grad.py (beyond it the oracle does not resolve 1e-6:
    the table beside test_gpu_sgp_surrogate.py::test_gradients_on_an_ill_conditioned_kmm);
  * the oracle agrees with itself on the same problem with training rows and inducing rows permuted (another summation order
    and another pivot order through the same FP64 algebra): likelihood 1e-10, mean 1e-9 of max |mean|, variance 1e-8 of the
    largest variance -- margins of 100 under the GPU bars;
  * at most 5 % of each query set sits within 1e-7 sigma2 of the variance clamp (those are left out of variance comparisons);
  * the two `gram-` rows still produce the K splits they are in the table for (a restatement of the launch arithmetic: a
    retuned rule fails here instead of silently losing the edge).
Measured where this was written (worst over the table): cond 1.5e7 (A, squared exponential; 6.9e5 for gram-uneven, the next),
likelihood 2.7e-13 (nz-eq-n), mean 2.6e-13 and variance 1.0e-9 (A, squared exponential; 1.3e-10 for n128, the next); no query of
any set within 1e-7 sigma2 of the clamp.  The `kpls` row's theta is twice the [1.3, 0.8] first tried: at that value cond = 1.4e9
under the squared exponential, beyond the bound (tests/sgp_edge_cases.py)."""
import numpy as np
import pytest

import sgp_edge_cases as EC
import sgp_grad_oracle as GO
import sgp_kpls_oracle as KO

CASE_IDS = list(EC.CASES)


def _permuted_oracle(cid, corr, method):
    from oracle import sgp_oracle as S
    x, y, z, w = EC.data(cid)
    rng = np.random.default_rng(1000 + corr)
    pn, pz = rng.permutation(x.shape[0]), rng.permutation(z.shape[0])
    return S.SparseGpOracle(x[pn], y[pn], z[pz], EC.theta(cid), EC.SIGMA2, EC.NOISE, corr=EC.KINDS[corr],
                            method=[S.FITC, S.VFE][method], w_star=w)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("corr", range(4))
@pytest.mark.parametrize("cid", CASE_IDS)
def test_the_oracle_can_vouch_for_the_row(cid, corr, method):
    x, y, z, w = EC.data(cid)
    n, nz, d, th, h = EC.CASES[cid]
    assert x.shape == (n, d) and z.shape == (nz, d) and th.shape == ((d if h is None else h),)
    if w is None:
        cond = GO.zz_condition(corr, z, th, EC.SIGMA2, EC.NUGGET)
    else:
        cond = KO.zz_condition(corr, z, w, th, EC.SIGMA2, EC.NUGGET)
    assert cond <= 1e8, cond
    ref, per = EC.oracle(cid, corr, method), _permuted_oracle(cid, corr, method)
    xq = EC.queries(cid, 50)
    mean, var = ref.predict(xq), ref.predict_var(xq)
    e_lk = abs(per.likelihood - ref.likelihood) / abs(ref.likelihood)
    e_mean = np.abs(per.predict(xq) - mean).max() / np.abs(mean).max()
    e_var = np.abs(per.predict_var(xq) - var).max() / var.max()
    print(f"{cid} corr {corr} method {method}: cond {cond:.2e}, likelihood {e_lk:.1e}, mean {e_mean:.1e}, variance {e_var:.1e}")
    assert np.isfinite(ref.likelihood) and e_lk <= 1e-10
    assert e_mean <= 1e-9
    assert e_var <= 1e-8


def _query_sets():
    sets = [(cid, EC.M_FORWARD, range(4)) for cid in CASE_IDS]
    sets += [("nz129", m, (0, 3)) for m in EC.M_COUNTS]
    sets += [("nz257", 3, (0, 3))]
    sets += [("A", m, (3,)) for m in EC.M_CHUNK]
    return sets


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("cid,m,corrs", _query_sets(), ids=[f"{c}-m{m}" for c, m, _ in _query_sets()])
def test_few_queries_sit_on_the_variance_clamp(cid, m, corrs, method):
    """Every query set the GPU file uses: a row's 131 queries, the query counts on nz129, the three of nz257's few-query case and
    the chunk sets on A.  At most 5 % unsure; a set that breaks it gets another query seed (sgp_edge_cases.QUERY_SEED)."""
    for corr in corrs:
        var_raw = EC.raw_variance(EC.oracle(cid, corr, method), EC.queries(cid, m))
        share = EC.unsure(var_raw).mean()
        print(f"{cid} m {m} corr {corr} method {method}: unsure {EC.unsure(var_raw).sum()} of {m}, clamped {(var_raw < 1e-15).sum()}")
        assert share <= 0.05, (corr, share)


def test_gram_rows_reach_the_splits_they_are_here_for():
    """kernels_chol.hip, gram_nsplit and the kc / nsplit lines of launch_gram_lower, restated: rows = zext, K = n_pad."""
    n_pad, _, zext = EC.pads("gram-uneven")
    assert (n_pad, zext) == (1152, 256)
    assert EC.gram_splits(zext, n_pad) == (640, 512)  # kc rounded up from 576: a short last split
    n_pad, _, zext = EC.pads("gram-fewer")
    assert (n_pad, zext) == (3200, 256)
    assert EC.gram_nsplit(zext, n_pad) == 6 and len(EC.gram_splits(zext, n_pad)) == 5  # the scratch is sized for one more
    assert EC.gram_splits(zext, n_pad) == (640,) * 5
    # the two shapes pinned before this table divide evenly: one split of 768, ten of 512
    assert EC.gram_splits(256, 768) == (768,) and EC.gram_splits(512, 5120) == (512,) * 10
    for cid in EC.CASES:
        n_pad, z_pad, zext = EC.pads(cid)
        parts = EC.gram_splits(zext, n_pad)
        assert sum(parts) == n_pad and len(parts) <= EC.gram_nsplit(zext, n_pad) and all(p > 0 and p % 128 == 0 for p in parts)


def test_padding_of_the_rows():
    """What the ids promise about n_pad, z_pad and zext."""
    want = {"n2-nz1": (128, 128, 256), "nz1": (256, 128, 256), "n128": (128, 128, 256), "A": (256, 128, 256),
            "nz128": (384, 128, 256), "nz129": (384, 256, 384), "nz-eq-n": (256, 256, 384), "nz256": (640, 256, 384),
            "nz257": (640, 384, 512), "gram-uneven": (1152, 128, 256), "gram-fewer": (3200, 128, 256), "d64": (256, 128, 256),
            "d65": (256, 128, 256), "kpls": (384, 256, 384)}
    assert {cid: EC.pads(cid) for cid in EC.CASES} == want
