"""GPU: the adaptive Lanczos depth (KT_AFUN_LANCZOS_AUTO, kt_lanczos_fmv_auto).

Item-1 tolerance.  On the CPU, the oracle's mc_trace with the Lanczos-exp
Afun at m = 128 against its trace_exp (expmv Afun), same seed
(tests/golden/make_adaptive_fixture.py -> adaptive_values.json "gaps"):
  anaheim 1.1e-16, oregon_A0 7.8e-15, anaheim x16 2.4e-14, rome x16 2.2e-16,
  grid 40x40 x16 5.1e-15, rome x40 1.9e-14, grid x40 5.2e-15.
Every graph reaches 1e-10, so none is dropped.  The device gets ten times the
worst (2.4e-13), but not tighter than 1e-12: TOL = 1e-12.  A fixed m = 30
drifts by 6.9e-7 .. 1.9e-5 on the scaled graphs (the fixture's "gap30").
The x40 graphs run here too (each trace_exp pair well under 5 s)."""
import json
import os
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, load_graph
from oracle import krylov_oracle as ko

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "adaptive_values.json")) as _f:
    FIX = json.load(_f)
TOL = max(1e-12, 10.0 * max(g["gap128"] for g in FIX["gaps"].values()))
GRAPHS = ["anaheim", "oregon_A0", "anaheim_x16", "rome_x16", "grid40_x16", "rome_x40", "grid40_x40"]


def grid_graph(a, b):
    pa = sp.diags([np.ones(a - 1), np.ones(a - 1)], [-1, 1])
    pb = sp.diags([np.ones(b - 1), np.ones(b - 1)], [-1, 1])
    return sp.csr_matrix(sp.kron(sp.identity(b), pa) + sp.kron(pb, sp.identity(a)))


def graph(name):
    if name.startswith("grid40"):
        A = grid_graph(40, 40)
    else:
        A = load_graph(name.split("_x")[0])
    return sp.csr_matrix(A * float(name.split("_x")[1])) if "_x" in name else A


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


@pytest.fixture(scope="module")
def traces(kra, gpu_ctx):
    """Per graph (expmv, lanczos-auto, lanczos m = 30), seed 0, computed once."""
    assert all(FIX["gaps"][g]["gap128"] < 1e-10 for g in GRAPHS)
    out = {"_capped_before": gpu_ctx.stat(6)}
    for name in GRAPHS:
        D = kra.DeviceMatrix(graph(name), gpu_ctx)
        out[name] = (kra.trace_exp(D, "expmv", ctx=gpu_ctx), kra.trace_exp(D, "lanczos-auto", ctx=gpu_ctx),
                     kra.trace_exp(D, "lanczos", m=30, ctx=gpu_ctx))
    out["_capped"] = gpu_ctx.stat(6) - out["_capped_before"]
    out["_max_depth"] = gpu_ctx.stat(5)
    return out


@pytest.mark.parametrize("name", GRAPHS)
def test_auto_matches_the_expmv_composition(traces, gpu_ctx, name):
    ref, auto, _ = traces[name]
    print(name, "expmv", ref, "auto", auto, "rel", abs(auto / ref - 1), "tol", TOL,
          "max depth", gpu_ctx.stat(5), "capped", gpu_ctx.stat(6))
    assert abs(auto - ref) <= TOL * abs(ref), (name, abs(auto / ref - 1))


@pytest.mark.parametrize("name", ["grid40_x16", "rome_x16"])
def test_fixed_depth_drifts_where_auto_does_not(traces, name):
    ref, auto, fixed = traces[name]
    print(name, "m=30 rel", abs(fixed / ref - 1), "auto rel", abs(auto / ref - 1))
    assert abs(fixed / ref - 1) > 1e-7
    assert abs(auto - ref) <= TOL * abs(ref)


def test_no_column_was_capped_at_the_default_cap(traces):
    print("max depth", traces["_max_depth"])
    assert traces["_capped"] == 0
    assert 8 <= traces["_max_depth"] <= 128


@pytest.fixture(scope="module")
def grid16(kra):
    A = graph("grid40_x16")
    X = ko.rademacher(A.shape[0], np.arange(100, 116), 3)
    return A, X


def test_fmv_auto_against_the_oracle(kra, grid16):
    A, X16 = grid16
    X = X16[:, :10]
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    Y, info = kra.lanczos_fmv_auto(D, X, return_info=True, ctx=ctx)
    print("depths", info["depth"], "capped", info["capped"])
    assert info["capped"] == 0 and ctx.stat(6) == 0
    assert np.all(info["depth"] >= 8) and np.all(info["depth"] <= 128)
    assert ctx.stat(5) == int(info["depth"].max())
    Yo = ko.lanczos_fmv(A, X, 2 * int(info["depth"].max()))
    err = np.linalg.norm(Y - Yo, axis=0) / np.linalg.norm(Yo, axis=0)
    print("rel 2-norm error per column", err)
    assert np.all(err <= 1e-9)
    q = np.einsum("ij,ij->j", X, Yo)
    assert np.all(np.abs(info["quad"] - q) <= 1e-9 * np.abs(q))
    # a cap of 12 is reached: counted, not an error, and the fixed-depth result
    Yc, ic = kra.lanczos_fmv_auto(D, X, m_max=12, return_info=True, ctx=ctx)
    assert ic["capped"] > 0 and ctx.stat(6) == ic["capped"] and np.all(ic["depth"] == 12)
    Yf = kra.lanczos_fmv(D, X, m=12, ctx=ctx)
    errc = np.linalg.norm(Yc - Yf, axis=0) / np.linalg.norm(Yf, axis=0)
    print("capped vs fixed m=12", errc)
    assert np.all(errc <= 1e-10)


def test_a_column_does_not_depend_on_its_company(kra, gpu_ctx, grid16):
    A, X = grid16
    D = kra.DeviceMatrix(A, gpu_ctx)
    got = []
    for nc in (1, 10, 16):
        _, info = kra.lanczos_fmv_auto(D, X[:, :nc], return_info=True, want_y=False, ctx=gpu_ctx)
        got.append((info["quad"][0], int(info["depth"][0])))
    assert got[0] == got[1] == got[2], got
    # with Y too (the f(A) x test decides the depth)
    goty = []
    for nc in (1, 10, 16):
        Y, info = kra.lanczos_fmv_auto(D, X[:, :nc], return_info=True, ctx=gpu_ctx)
        goty.append((info["quad"][0], int(info["depth"][0]), Y[:, 0].tobytes()))
    assert goty[0] == goty[1] == goty[2]


def test_many_columns_run_on_every_sweep_lane(kra, gpu_ctx):
    """70 columns are five 16-wide sweeps (four lanes, then a second group):
    each column equals, bit for bit, the same column in a call of its own
    16-column sweep alone."""
    A = graph("grid40_x16")
    X = ko.rademacher(A.shape[0], np.arange(200, 270), 5)
    D = kra.DeviceMatrix(A, gpu_ctx)
    Y, info = kra.lanczos_fmv_auto(D, X, return_info=True, ctx=gpu_ctx)
    assert info["capped"] == 0 and np.all(info["depth"] >= 8)
    for c0 in range(0, 70, 16):
        Yk, ik = kra.lanczos_fmv_auto(D, X[:, c0:c0 + 16], return_info=True, ctx=gpu_ctx)
        assert np.array_equal(ik["depth"], info["depth"][c0:c0 + 16]), c0
        assert np.array_equal(ik["quad"], info["quad"][c0:c0 + 16]), c0
        assert Yk.tobytes() == np.asfortranarray(Y[:, c0:c0 + 16]).tobytes(), c0


def test_zero_and_parallel_columns(kra, gpu_ctx, grid16):
    """A zero column stops at once with quad 0 and depth 0; an eigenvector
    (lucky breakdown at step 1) stops at depth 1."""
    A, X = grid16
    n = A.shape[0]
    w, V = np.linalg.eigh(A.toarray())
    Z = np.column_stack([X[:, 0], np.zeros(n), V[:, -1], X[:, 1]])
    D = kra.DeviceMatrix(A, gpu_ctx)
    Y, info = kra.lanczos_fmv_auto(D, Z, return_info=True, ctx=gpu_ctx)
    assert info["depth"][1] == 0 and info["quad"][1] == 0.0 and not Y[:, 1].any()
    assert info["depth"][2] == 1 and info["quad"][2] == pytest.approx(np.exp(w[-1]), rel=1e-12)
    assert np.linalg.norm(Y[:, 2] - np.exp(w[-1]) * V[:, -1]) <= 1e-10 * np.exp(w[-1])
    assert info["capped"] == 0


class _ThreadReduce:
    def __init__(self, world):
        self.bar = threading.Barrier(world)
        self.bufs = [None] * world

    def fn(self, rank):
        from krylov_robustness_amd import _lib

        def cb(buf, count, user):
            arr = np.ctypeslib.as_array(buf, shape=(int(count),))
            self.bufs[rank] = arr.copy()
            self.bar.wait()
            tot = np.zeros(int(count))
            for b in self.bufs:
                tot = tot + b
            self.bar.wait()
            arr[:] = tot
            return 0
        return _lib.REDUCE_FN(cb)


def _run_world(kra, A, world, **kw):
    red = _ThreadReduce(world)
    out, errs = [None] * world, []

    def worker(r):
        try:
            ctx = kra.Context(0)
            D = kra.DeviceMatrix(A, ctx)
            out[r] = kra.mc_trace_sharded("lanczos-auto", None, A=D, rank=r, world=world, allreduce=red.fn(r),
                                          ctx=ctx, **kw)
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)
            red.bar.abort()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    return out


def test_sharded_worlds_are_bit_identical(kra):
    A = load_graph("oregon_A0")
    kw = dict(tol=1e-6, maxit=120, isAreal=1, seed=3, fun="exp")
    ref = _run_world(kra, A, 1, **kw)[0]
    for world in (2, 4):
        for r in _run_world(kra, A, world, **kw):
            assert r == ref, (world, r, ref)
    assert ref[2] >= 2


def test_fixed_depth_paths_keep_their_bits_around_an_adaptive_call(kra, grid16):
    """The adaptive path shares the context's workspaces with the fixed-depth
    one: trace_exp's default and lanczos_fmv(m = 30) return the same bits
    before and after an adaptive call."""
    A, X = grid16
    ctx = kra.Context(0)
    D = kra.DeviceMatrix(A, ctx)
    t0 = kra.trace_exp(D, ctx=ctx)
    y0 = kra.lanczos_fmv(D, X[:, :10], m=30, ctx=ctx)
    kra.trace_exp(D, "lanczos-auto", ctx=ctx)
    kra.lanczos_fmv_auto(D, X, ctx=ctx)
    assert kra.trace_exp(D, ctx=ctx) == t0
    assert kra.lanczos_fmv(D, X[:, :10], m=30, ctx=ctx).tobytes() == y0.tobytes()


def test_cap_above_256_is_refused(kra, gpu_ctx):
    D = kra.DeviceMatrix(load_graph("anaheim"), gpu_ctx)
    with pytest.raises(kra.KrylovError):
        kra.trace_exp(D, "lanczos-auto", m=257, ctx=gpu_ctx)
    with pytest.raises(kra.KrylovError):
        kra.lanczos_fmv_auto(D, np.ones((416, 1)), m_max=300, ctx=gpu_ctx)
