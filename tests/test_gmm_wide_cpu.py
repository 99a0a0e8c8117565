"""CPU side of the wide-row mixture training (egx_gmm_fit_wide): csrc/gmm_wide_plan.h compiled for the host, plainly and with
the address and undefined-behaviour sanitizers, and run as the stand-alone program it is (tests/c_host/gmm_wide_plan_test.cpp);
the validation that happens before a device is touched; and the routing of moe.train_mixture.  No device compute."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gmm_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_host", "gmm_wide_plan_test.cpp")
CHECKS = ["padding and LDS", "tile owners", "row cover", "a function of n and D", "workspace bound"]


@pytest.fixture(scope="module")
def egx():
    import egobox_amd
    return egobox_amd


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _check(out):
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-800:])
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "OK" and not [l for l in lines if l.startswith("FAIL")], lines
    for what in CHECKS:
        assert any(l.startswith(f"ok {what}") for l in lines), what


def test_plan(tmp_path):
    exe = tmp_path / "gmm_wide_plan_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", str(exe)], check=True)
    _check(subprocess.run([str(exe)], capture_output=True, text=True))


def test_plan_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "gmm_wide_plan_test_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert "runtime error" not in out.stderr, out.stderr[-800:]
    _check(out)


def test_the_library_uses_the_plan():
    """The kernels and the host size their launches by this header, and both entry points share one driver."""
    csrc = os.path.join(ROOT, "egobox_amd", "csrc")
    assert '#include "gmm_wide_plan.h"' in open(os.path.join(csrc, "kernels_gmm_wide.hip")).read()
    host = open(os.path.join(csrc, "gmm_host.hip")).read()
    assert '#include "gmm_wide_plan.h"' in host and host.count("return gmm_fit_driver(") == 2
    assert host.count("path.estep(") == 1 and host.count("path.mstep(") == 1
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "gmm_wide_plan.h" in mk and "kernels_gmm_wide.hip" in mk


def test_fit_wide_validates_before_the_device(egx):
    x = GO.blobs(60, 40, 2, seed=0)
    bad = x.copy()
    bad[7, 1] = np.nan
    with pytest.raises(egx.InvalidValueError, match="finite"):
        egx.GaussianMixture.fit_wide(bad, 2)
    with pytest.raises(egx.InvalidValueError):
        egx.GaussianMixture.fit_wide(x, 0)
    with pytest.raises(egx.InvalidValueError):
        egx.GaussianMixture.fit_wide(x[:3], 4)
    with pytest.raises(egx.InvalidValueError):
        egx.GaussianMixture.fit_wide(x, 2, n_runs=0)
    with pytest.raises(egx.InvalidValueError):
        egx.GaussianMixture.fit_wide(x, 2, n_runs=2, init_means=np.zeros((2, 2, 41)))
    with pytest.raises(egx.InvalidValueError, match="dim <= 128"):
        egx.GaussianMixture.fit_wide(np.random.default_rng(0).random((200, 129)), 2)
    with pytest.raises(egx.InvalidValueError, match="n_clusters <= 16"):
        egx.GaussianMixture.fit_wide(np.random.default_rng(0).random((50, 3)), 17)


def test_c_abi_validates_before_the_device(egx):
    """NULLs, n < k, n_runs = 0, NaN data, dim 129 and 17 clusters through ctypes: EGX_ERR_INVALID_VALUE with the entry point's
    name in the message, whatever the machine."""
    L = egx._lib
    lib = L.load()
    x = np.ascontiguousarray(GO.blobs(60, 40, 2, seed=0))
    st = np.ascontiguousarray(GO.starts(x, 2, 2, seed=1))
    w, m, c, lb = np.empty(2), np.empty((2, 40)), np.empty((2, 40, 40)), np.empty(2)
    it, stt, best = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), C.c_int32(-1)

    def call(cfg, data=x, n=60, dim=40, init=st, weights=w):
        return lib.egx_gmm_fit_wide(cfg, None if data is None else L.dptr(data), n, dim, None if init is None else L.dptr(init),
                                    None if weights is None else L.dptr(weights), L.dptr(m), L.dptr(c), L.dptr(lb),
                                    it.ctypes.data_as(L.c_int32_p), stt.ctypes.data_as(L.c_int32_p), C.byref(best), None, None, None)

    def config(**kw):
        cfg = L.GmmConfig()
        lib.egx_gmm_config_default(cfg)
        cfg.n_clusters, cfg.n_runs = 2, 2
        for name, v in kw.items():
            setattr(cfg, name, v)
        return cfg

    for kw in (dict(data=None), dict(init=None), dict(weights=None)):
        assert call(config(), **kw) == L.ERR_INVALID_VALUE and b"egx_gmm_fit_wide: NULL" in lib.egx_last_error()
    assert lib.egx_gmm_fit_wide(None, L.dptr(x), 60, 40, L.dptr(st), L.dptr(w), L.dptr(m), L.dptr(c), L.dptr(lb),
                                it.ctypes.data_as(L.c_int32_p), stt.ctypes.data_as(L.c_int32_p), C.byref(best), None, None,
                                None) == L.ERR_INVALID_VALUE
    assert call(config(), n=1) == L.ERR_INVALID_VALUE
    assert call(config(n_runs=0)) == L.ERR_INVALID_VALUE
    assert call(config(), dim=0) == L.ERR_INVALID_VALUE
    bad = x.copy()
    bad[3, 39] = np.nan
    assert call(config(), data=bad) == L.ERR_INVALID_VALUE and b"finite" in lib.egx_last_error()
    assert call(config(), dim=129) == L.ERR_INVALID_VALUE and b"dim <= 128" in lib.egx_last_error()  # before the data is read
    assert call(config(n_clusters=17)) == L.ERR_INVALID_VALUE and b"n_clusters <= 16" in lib.egx_last_error()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU behaviour")
def test_fit_wide_has_no_cpu_fallback(egx):
    x = GO.blobs(60, 40, 2, seed=0)
    with pytest.raises(egx.NoDeviceError):
        egx.GaussianMixture.fit_wide(x, 2)
    with pytest.raises(egx.NoDeviceError):
        egx.GpMixture.params().n_clusters(2).recombination("hard").fit(x[:, :39], x[:, 39])


def test_train_mixture_routes_by_width(egx, monkeypatch):
    """36 columns go to GaussianMixture.fit -- what every narrow training has always called -- and 37 to fit_wide, keywords
    passed on; GaussianMixture.fit itself still refuses 37 columns with its own message."""
    M = egx.moe
    calls = []
    monkeypatch.setattr(M.GaussianMixture, "fit", classmethod(lambda cls, data, k, **kw: calls.append(("fit", data.shape, k, kw))))
    monkeypatch.setattr(M.GaussianMixture, "fit_wide",
                        classmethod(lambda cls, data, k, **kw: calls.append(("fit_wide", data.shape, k, kw))))
    M.train_mixture(np.zeros((50, 36)), 2, n_runs=3, seed=5)
    M.train_mixture(np.zeros((50, 37)), 2, n_runs=3, seed=5)
    M.train_mixture(np.zeros((50, 128)), 3)
    assert calls == [("fit", (50, 36), 2, dict(n_runs=3, seed=5)), ("fit_wide", (50, 37), 2, dict(n_runs=3, seed=5)),
                     ("fit_wide", (50, 128), 3, {})]
    monkeypatch.undo()
    with pytest.raises(egx.InvalidValueError, match="dim <= 36"):
        egx.GaussianMixture.fit(np.random.default_rng(0).random((50, 37)), 2)
    assert M.GMM_NARROW_MAX_DIM == 36
    import inspect
    assert "train_mixture(" in inspect.getsource(M.GpMixtureParams.fit) + inspect.getsource(M.GpMixtureParams)
    assert "train_mixture(" in inspect.getsource(egx.sgp)
