"""The case table of tests/pending_cases.py on the CPU, without the library: every row is well posed on the oracle alone (the
gate of the GPU tests: min diag S >= 1e-2, min conditioned unit variance >= 1e-4), and the rows named after a threshold of the
launch code straddle it.  The launch arithmetic is restated in pending_cases.py from egobox_amd/csrc; a retune of kPcThreads,
kPendingQV, kPendingMaxD or an opt-in threshold fails here instead of emptying a GPU case."""
import os
import re
import time

import pytest

import pending_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egobox_amd", "csrc")


@pytest.mark.parametrize("r", PC.ROWS, ids=[r.id for r in PC.ROWS])
def test_row_meets_the_gate_on_the_oracle(r):
    t0 = time.perf_counter()
    g, xv, xq = PC.oracle_case(r)
    assert xv.shape == (r.q, r.d) and xq.shape == (r.m, r.d) and g.theta.shape == ((r.kpls or r.d),)
    min_diag, min_unit, ok = PC.gate(g, xv, xq)
    print(f"{r.id}: min diag S {min_diag:.3g}, min conditioned unit variance {min_unit:.3g} ({time.perf_counter() - t0:.2f} s)")
    assert ok


def test_the_hand_over_case_without_its_last_input_meets_the_gate():
    """the 65 inputs of composed-first with the 65th dropped: the d = 64 side of the hand-over test"""
    r = PC.BY_ID["composed-first"]
    g, xv, xq = PC.oracle_case(r, keep=PC.K_PENDING_MAX_D)
    assert xv.shape == (r.q, 64) and xq.shape == (r.m, 64) and g.xt_norm.shape == (r.n, 64)
    min_diag, min_unit, ok = PC.gate(g, xv, xq)
    print(f"composed-first[:, :64]: min diag S {min_diag:.3g}, min conditioned unit variance {min_unit:.3g}")
    assert ok


def _constant(name, path):
    src = open(os.path.join(CSRC, path)).read()
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\w+)\s*;", src)
    assert m, name
    return m.group(1)


def test_constants_are_the_sources():
    assert int(_constant("kTile", "egx_internal.h")) == PC.K_TILE
    assert int(_constant("kPendingQV", "egx_internal.h")) == PC.K_PENDING_QV
    assert int(_constant("kPendingMaxD", "egx_internal.h")) == PC.K_PENDING_MAX_D
    assert int(_constant("kPcThreads", "kernels_pending.hip")) == PC.K_PC_THREADS
    assert int(_constant("kMaxPending", "pending_math.h")) == PC.K_LD and _constant("kLd", "pending_math.h") == "kMaxPending"
    src = open(os.path.join(CSRC, "kernels_pending.hip")).read()
    assert f"if (lds > {PC.CROSS_OPT_IN})" in src and f"if (lds > {PC.FINISH_OPT_IN})" in src
    assert "(size_t)d * kPcThreads + (size_t)d * 64 + (size_t)d * hcols + 64 * kPendingQV" in src
    assert "sizeof(double) * (size_t)pending::kLd * (size_t)(f.d > 0 ? f.d : 1)" in src


def test_rows_straddle_the_edges_they_are_named_after():
    B = PC.BY_ID
    # the LDS of k_pending_cross: 8 ((128 + 64 + hcols) d + 256) bytes, the opt-in above 64 KiB
    assert PC.cross_lds_bytes(41) == 65352 and PC.cross_lds_bytes(42) == 66896
    assert PC.cross_lds_bytes(B["lds-below"].d) <= PC.CROSS_OPT_IN < PC.cross_lds_bytes(B["lds-above"].d)
    assert B["lds-above"].d == B["lds-below"].d + 1
    # ... of k_pending_finish: 16 d doubles, its opt-in above 60 000 bytes
    assert PC.finish_lds_bytes(468) == 59904 and PC.finish_lds_bytes(469) == 60032
    assert PC.finish_lds_bytes(B["finish-lds"].d - 1) <= PC.FINISH_OPT_IN < PC.finish_lds_bytes(B["finish-lds"].d)
    assert PC.K_PENDING_MAX_D < B["finish-lds"].d <= 1024
    # the hand-over
    assert B["fused-last"].d == PC.K_PENDING_MAX_D and B["composed-first"].d == PC.K_PENDING_MAX_D + 1
    # DK and the k0 passes
    assert PC.k0_passes(8) == (8, [8])
    assert PC.k0_passes(B["dk16-first"].d) == (16, [9])
    assert PC.k0_passes(B["dk16-full"].d) == (16, [16])
    assert PC.k0_passes(B["two-pass"].d) == (16, [16, 1])
    assert PC.k0_passes(B["three-pass"].d) == (16, [16, 16, 1])
    assert PC.k0_passes(B["fused-last"].d) == (16, [16] * 4)
    # the column passes
    assert PC.column_passes(B["dk16-first"].q) == [(0, 4), (4, 2)]
    assert PC.column_passes(B["dk16-full"].q) == [(0, 4), (4, 3)]
    assert PC.column_passes(B["two-pass"].q) == [(0, 4)]
    assert PC.column_passes(B["three-pass"].q) == [(0, 4), (4, 4)]
    assert PC.column_passes(B["kpls-d12"].q) == [(0, 4), (4, 1)]
    assert PC.column_passes(B["slab-q16"].q) == [(0, 4), (4, 4), (8, 4), (12, 4)]
    # the slabs of Z
    assert (B["slab-exact"].n + B["slab-exact"].q) % 64 == 0
    assert (B["slab-pending-only"].n + B["slab-pending-only"].q) % 64 == 1 and B["slab-pending-only"].n % 64 == 0
    assert B["slab-q16"].n % 64 == 0 and B["slab-q16"].q == PC.K_LD
    # the trend of two-pass-quad
    d = B["two-pass-quad"].d
    assert B["two-pass-quad"].mean == 2 and 1 + d + d * (d + 1) // 2 == 171
    assert B["kpls-d12"].kpls == 2 and PC.row_weights(B["kpls-d12"]).shape == (12, 2)
    assert PC.TWO_MODELS == {"three-pass", "lds-below", "lds-above", "fused-last", "composed-first", "finish-lds"}
