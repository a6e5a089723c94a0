"""GPU: the error-controlled probe sweeps (kt_slq_trace_auto):
kt_slq_trace's probes with each probe's depth chosen by the stopping rule of
the adaptive Lanczos depth, on resumable y-form sweeps.

Tolerances.  Forms against the oracle at a depth far past the stopping depth:
1e-9 relative, the tolerance test_fmv_auto_against_the_oracle holds the
adaptive forms to (the rule alone leaves <= 2.3e-13 on these graphs,
tests/test_slq_auto_host.py).  Forms of probes stopped by the cap against the
oracle at the SAME depth: 1e-8, the per-form GPU tolerance of DESIGN.md §2."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_graph
from oracle import slq_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


def grid_graph(a, b):
    pa = sp.diags([np.ones(a - 1), np.ones(a - 1)], [-1, 1])
    pb = sp.diags([np.ones(b - 1), np.ones(b - 1)], [-1, 1])
    return sp.csr_matrix(sp.kron(sp.identity(b), pa) + sp.kron(pb, sp.identity(a)))


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "cl20k":
        from krylov_robustness_amd import graphs
        return sp.csr_matrix(graphs.chung_lu(20_000, 200_000, seed=0))
    if name.startswith("grid40"):
        A = grid_graph(40, 40)
    else:
        A = load_graph(name.split("_x")[0])
    return sp.csr_matrix(A * float(name.split("_x")[1])) if "_x" in name else A


@functools.lru_cache(maxsize=None)
def oracle(name, nprobes, m, seed=0, offset=0):
    q = slq_ref.slq_trace(graph(name), nprobes, m, seed=seed, fun="exp", probe_offset=offset)[1]
    q.setflags(write=False)
    return q


def relerr(q, ref):
    return np.abs(q - ref) / np.abs(ref)


def _ctx_with(monkeypatch, kra, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return kra.Context(0)


@pytest.mark.parametrize("name", ["grid40_x40", "rome_x40"])
def test_auto_is_accurate_where_m30_drifts(kra, name):
    """Flat, wide spectra (weighted: the fp64 y_0 path): the auto forms agree
    with the oracle at depth 128 to 1e-9 on every probe, where the fixed
    m = 30 forms are off by more than 1e-7 on at least half of them."""
    ctx = kra.Context(0)  # stat 5 is a running maximum: a fresh context
    D = kra.DeviceMatrix(graph(name), ctx)
    ref = oracle(name, 32, 128)
    _, _, q, info = kra.slq_quadforms_auto(D, 32, seed=0, block=16, return_info=True, ctx=ctx)
    err = relerr(q, ref)
    q30 = kra.slq_quadforms(D, 32, 30, seed=0, block=16, ctx=ctx)[2]
    err30 = relerr(q30, ref)
    print(name, "auto max err", err.max(), "depths", info["depth"].min(), info["depth"].max(),
          "m=30 err min/median/max", err30.min(), np.median(err30), err30.max())
    assert np.all(err <= 1e-9), err.max()
    assert np.sum(err30 > 1e-7) >= 16, np.sort(err30)
    assert np.all((info["depth"] >= 8) & (info["depth"] <= 128)) and info["capped"] == 0
    assert ctx.stat(5) == info["depth"].max()


@pytest.mark.parametrize("name", ["anaheim", "oregon_A0", "cl20k"])
def test_auto_unit_weight_compact_path(kra, monkeypatch, name):
    """Unit weights: the sweeps carry y_0 as int16 row sums through their first
    two steps (stat 7 counts them); cl20k has long rows (the wave-per-row
    branch).  Depths stay well below 30 (CPU figures 12, 17, 22)."""
    ctx = _ctx_with(monkeypatch, kra, KT_SLQ_YFORM="1")
    D = kra.DeviceMatrix(graph(name), ctx)
    s7 = ctx.stat(7)
    _, _, q, info = kra.slq_quadforms_auto(D, 32, seed=0, block=16, return_info=True, ctx=ctx)
    err = relerr(q, oracle(name, 32, 60))
    print(name, "max err", err.max(), "depths", info["depth"].min(), info["depth"].max())
    assert np.all(err <= 1e-9), err.max()
    assert ctx.stat(7) - s7 == 2
    assert info["depth"].max() < 30 and info["depth"].min() >= 8 and info["capped"] == 0
    assert ctx.stat(0) == 0


def test_early_stop_is_real(kra, monkeypatch):
    """anaheim stops at depth 12: two sweeps queue far fewer than the 2 x 127
    step passes of the cap."""
    ctx = _ctx_with(monkeypatch, kra, KT_SLQ_YFORM="1")
    D = kra.DeviceMatrix(graph("anaheim"), ctx)
    s8 = ctx.stat(8)
    info = kra.slq_quadforms_auto(D, 32, m_max=128, seed=0, block=16, return_info=True, ctx=ctx)[3]
    queued = ctx.stat(8) - s8
    print("step passes queued", queued, "deepest column", info["depth"].max())
    assert info["depth"].max() - 1 <= queued < 127
    # at most 9 passes per sweep past the check that stopped its last column
    assert queued <= 2 * (info["depth"].max() - 1 + 9)


@pytest.mark.parametrize("block", [1, 4, 16, 64, 128])
def test_auto_widths_and_ragged_ranges(kra, monkeypatch, block):
    """Every sweep width with a ragged probe count and an offset: the oracle's
    forms, bit-identical repeats, and the same bits with 1 and 3 lanes."""
    ctx = _ctx_with(monkeypatch, kra, KT_SLQ_YFORM="1")
    D = kra.DeviceMatrix(graph("grid40_x16"), ctx)
    nprobes = 3 * block + 1 if block > 1 else 6
    ref = oracle("grid40_x16", nprobes, 128, 0, 5)

    def run():
        _, _, q, info = kra.slq_quadforms_auto(D, nprobes, seed=0, probe_offset=5, block=block, return_info=True,
                                               ctx=ctx)
        return q, info["depth"]

    qa, da = run()
    qb, db = run()
    err = relerr(qa, ref)
    print("block", block, "max err", err.max(), "depths", da.min(), da.max())
    assert np.all(err <= 1e-9), err.max()
    assert np.array_equal(qa, qb) and np.array_equal(da, db)
    monkeypatch.setenv("KT_SLQ_LANES", "1")
    q1, d1 = run()
    monkeypatch.setenv("KT_SLQ_LANES", "3")
    q3, d3 = run()
    assert np.array_equal(q1, qa) and np.array_equal(d1, da)
    assert np.array_equal(q3, qa) and np.array_equal(d3, da)
    assert ctx.stat(0) == 0


def test_auto_independent_of_company_and_call_size(kra, monkeypatch):
    """Probes 16..31 from a 16-probe call equal, bit for bit, the same probes
    in a 70-probe call."""
    ctx = _ctx_with(monkeypatch, kra, KT_SLQ_YFORM="1")
    D = kra.DeviceMatrix(graph("grid40_x16"), ctx)
    s0 = ctx.stat(0)
    _, _, qs, si = kra.slq_quadforms_auto(D, 16, seed=0, probe_offset=16, block=16, return_info=True, ctx=ctx)
    _, _, ql, li = kra.slq_quadforms_auto(D, 70, seed=0, block=16, return_info=True, ctx=ctx)
    assert np.array_equal(qs, ql[16:32]) and np.array_equal(si["depth"], li["depth"][16:32])
    assert ctx.stat(0) == s0


def test_auto_cap(kra, gpu_ctx):
    """A cap below the stopping depth (90..94 on grid40_x150): every probe runs
    the 60 rows, is counted as capped, and its form is the fixed-depth one."""
    D = kra.DeviceMatrix(graph("grid40_x150"), gpu_ctx)
    s6 = gpu_ctx.stat(6)
    _, _, q, info = kra.slq_quadforms_auto(D, 20, m_max=60, seed=0, block=16, return_info=True, ctx=gpu_ctx)
    assert np.all(info["depth"] == 60)
    assert info["capped"] == 20 == gpu_ctx.stat(6) - s6
    err = relerr(q, oracle("grid40_x150", 20, 60))
    print("max err at the cap", err.max())
    assert np.all(err <= 1e-8), err.max()


def test_auto_handover_past_the_horizon(kra, monkeypatch):
    """rtol = 1e-17 stops no probe (asserted on the host first), so the y-form
    sweep reaches its horizon with every column running and is handed whole to
    the explicit sweep, whose checks past 128 rows take the large-LDS form of
    the check kernel; all 16 probes are capped at 160 with the oracle's forms.
    The default call on the same graph (CPU depths 90..94) holds the oracle's
    forms whichever side of the horizon stops a probe."""
    import ctypes as C
    from krylov_robustness_amd import _lib
    from oracle import krylov_oracle as ko
    lib = _lib.load()
    A = graph("grid40_x150")
    Z = ko.rademacher(A.shape[0], np.arange(16), 0)
    for c in range(16):
        al, off, _, lucky = ko.lanczos_probe_tridiag(A, Z[:, c], 160)
        assert not lucky and len(al) == 160
        for j in range(8, 161):
            cv, qq = C.c_int(-1), C.c_double()
            a, o = np.ascontiguousarray(al[:j]), np.ascontiguousarray(off[:j - 1])
            assert lib.kt_host_quad_converged(j, a.ctypes.data_as(_lib._dp), o.ctypes.data_as(_lib._dp), 0, 0, 1e-17,
                                              C.byref(cv), C.byref(qq)) == 0
            assert cv.value == 0, (c, j)
    ctx = _ctx_with(monkeypatch, kra, KT_SLQ_YFORM="1")
    D = kra.DeviceMatrix(A, ctx)
    _, _, q, info = kra.slq_quadforms_auto(D, 16, m_max=160, rtol=1e-17, seed=0, block=16, return_info=True, ctx=ctx)
    err = relerr(q, oracle("grid40_x150", 16, 160))
    print("capped at 160: max err", err.max())
    assert np.all(info["depth"] == 160) and info["capped"] == 16
    assert np.all(err <= 1e-8), err.max()
    assert ctx.stat(0) == 0  # a handover at the horizon is not a guard redo
    _, _, q, info = kra.slq_quadforms_auto(D, 16, seed=0, block=16, return_info=True, ctx=ctx)
    err = relerr(q, oracle("grid40_x150", 16, 200))
    print("default call: max err", err.max(), "depths", info["depth"].min(), info["depth"].max())
    assert np.all(err <= 1e-9), err.max()
    assert info["capped"] == 0 and info["depth"].max() <= 128


def test_auto_guard_and_breakdown(kra, monkeypatch):
    """K_50 as in test_slq_yform_breakdown_falls_back: the Krylov space is
    exhausted after 2 steps, both sweeps trip the guard and are redone by the
    explicit sweep, which cuts every probe at the breakdown."""
    from oracle import krylov_oracle as ko
    A = sp.csr_matrix(np.ones((50, 50)) - np.eye(50))
    ctx = _ctx_with(monkeypatch, kra, KT_SLQ_YFORM="1")
    D = kra.DeviceMatrix(A, ctx)
    _, _, q, info = kra.slq_quadforms_auto(D, 20, seed=6, block=16, return_info=True, ctx=ctx)
    assert ctx.stat(0) == 2
    assert np.all(info["depth"] <= 2) and info["capped"] == 0
    Z = ko.rademacher(50, np.arange(20), 6)
    s = Z.sum(axis=0)
    exact = s ** 2 / 50 * np.exp(49.0) + (50 - s ** 2 / 50) * np.exp(-1.0)
    np.testing.assert_allclose(q, exact, rtol=1e-10)


def test_auto_explicit_path(kra, monkeypatch):
    """KT_SLQ_YFORM=0: every sweep takes the explicit auto path."""
    ctx = _ctx_with(monkeypatch, kra, KT_SLQ_YFORM="0")
    D = kra.DeviceMatrix(graph("grid40_x16"), ctx)
    s8 = ctx.stat(8)
    _, _, q, info = kra.slq_quadforms_auto(D, 20, seed=0, block=16, return_info=True, ctx=ctx)
    err = relerr(q, oracle("grid40_x16", 20, 128))
    print("explicit auto path: max err", err.max(), "depths", info["depth"].min(), info["depth"].max())
    assert np.all(err <= 1e-9), err.max()
    assert info["capped"] == 0 and info["depth"].max() < 45 and ctx.stat(8) == s8


def test_neighbours_keep_their_bits(kra, gpu_ctx):
    """The fixed-depth call and trace_exp return the same bits before and
    after an auto call on the same context (shared lane buffers)."""
    D = kra.DeviceMatrix(graph("grid40_x16"), gpu_ctx)
    q0 = kra.slq_quadforms(D, 64, 30, ctx=gpu_ctx)[2]
    t0 = kra.trace_exp(D, ctx=gpu_ctx)
    kra.slq_quadforms_auto(D, 40, ctx=gpu_ctx)
    q1 = kra.slq_quadforms(D, 64, 30, ctx=gpu_ctx)[2]
    t1 = kra.trace_exp(D, ctx=gpu_ctx)
    assert np.array_equal(q0, q1) and t0 == t1


def test_auto_arguments(kra, gpu_ctx):
    D = kra.DeviceMatrix(graph("anaheim"), gpu_ctx)
    with pytest.raises(kra.KrylovError, match="at most 256"):
        kra.slq_quadforms_auto(D, 4, m_max=257, ctx=gpu_ctx)
    s1, s2, q, info = kra.slq_quadforms_auto(D, 0, return_info=True, ctx=gpu_ctx)
    assert (s1, s2, q.size, info["depth"].size, info["capped"]) == (0.0, 0.0, 0, 0, 0)
    est, q = kra.slq_trace_auto(D, 8, seed=3, ctx=gpu_ctx)
    assert est == pytest.approx(q.mean(), rel=1e-14) and q.size == 8
    pending = kra.slq_submit(D, 8, 20, seed=3, ctx=gpu_ctx)
    with pytest.raises(kra.KrylovError, match="outstanding"):
        kra.slq_quadforms_auto(D, 8, ctx=gpu_ctx)
    got = kra.slq_collect(pending)[2]
    assert np.array_equal(got, kra.slq_quadforms(D, 8, 20, seed=3, ctx=gpu_ctx)[2])
