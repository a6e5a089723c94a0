"""kt_entries_fun_bracket on the device against dense eigh and
against the NumPy restatement (tests/entries_bracket_ref.py) evaluated at the
device's column depths, and find_top_edges_bracket over it.

Bounds.  lo <= exact <= hi up to SLACK (E_ii + E_jj) / 2, SLACK of
tests/test_entries_bracket_host.py (ten times the restatement's own largest
violation against dense eigh, 4.93e-14, in that unit).  Device values against
the restatement cut at the device's col_iter: 1e-7 of that unit, the convention
of tests/test_gpu_bracket.py.  Flags: the restatement's own run
(entries_bracket_ref.pair_run), or another one only where, at the earlier of the
two decisions, the restatement's gap lies within SLACK (E_ii + E_jj) / 2 of the
threshold it was compared with."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_graph

import entries_bracket_ref as er

GRAPHS = ("anaheim", "india", "rome", "oregon_A0")
SLACK = 10.0 * 4.93e-14
RTOL, FTOL = 1e-10, 1e-12
I64P, DP, IP = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def kra():
    import krylov_robustness_amd as kra
    return kra


def c_call(D, pairs, mu, rtol=RTOL, ftol=FTOL, it=0):
    """kt_entries_fun_bracket with col_iter: (lo, hi, iter, flag, col_iter (npairs, 2))."""
    from krylov_robustness_amd import _lib
    P = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    q = P.shape[0]
    ei, ej = np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(P[:, 1])
    lo, hi = np.zeros(q), np.zeros(q)
    itr, fl, ci = np.zeros(q, dtype=np.int32), np.zeros(q, dtype=np.int32), np.zeros(2 * q, dtype=np.int32)
    _lib.check(_lib.load().kt_entries_fun_bracket(
        D.handle, q, ei.ctypes.data_as(I64P), ej.ctypes.data_as(I64P), float(mu), float(rtol), float(ftol), int(it),
        lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), itr.ctypes.data_as(IP), fl.ctypes.data_as(IP),
        ci.ctypes.data_as(IP)))
    return lo, hi, itr, fl, ci.reshape(-1, 2)


@pytest.fixture(scope="module")
def cases(kra, gpu_ctx):
    """Per graph: entries_bracket_ref.graph_case (shared with the CPU tests: A,
    exp(A) by dense eigh, mu, the pair set and its Lanczos runs), the device
    copy and the pair set's call.  The device copies are closed here, while the
    context is alive."""
    out = {}
    for g in GRAPHS:
        c = dict(er.graph_case(g))
        c["D"] = kra.DeviceMatrix(c["A"], gpu_ctx)
        c["more runs"] = {}
        c["list"] = er.flat(c["pairs"])
        c["res"] = c_call(c["D"], c["list"], c["mu"])
        c["sweeps"] = gpu_ctx.stat(13)
        out[g] = c
    yield out
    for c in out.values():
        c.pop("D").close()


def runs_of(c, pair, depth=40):
    """The pair's restatement runs: the shared case's, which stays as it is, or this module's own."""
    key = (min(pair), max(pair))
    for k in (key, key[::-1]):
        if k in c["runs"]:
            return c["runs"][k]
    if key not in c["more runs"]:
        c["more runs"][key] = er.pair_runs(c["A"], key[0], key[1], depth)
    return c["more runs"][key]


def check_pairs(c, g, pairs, res, rtol=RTOL, ftol=FTOL, it_cap=100, flags=True):
    lo, hi, it, fl, ci = res
    E, mu = c["E"], c["mu"]
    worst = 0.0
    for h, (i, j) in enumerate(pairs):
        sc = er.scale_of(E, i, j)
        ex = E[i, j]
        runs = runs_of(c, (i, j))
        dp, dm = int(ci[h, 0]), int(ci[h, 1])
        print(g, "pair", (i, j), "lo", lo[h], "hi", hi[h], "iter", int(it[h]), "flag", int(fl[h]), "depths", (dp, dm),
              "exact", ex, "exact / scale %.3e" % (ex / sc), "gap / scale %.3e" % ((hi[h] - lo[h]) / sc))
        assert fl[h] in (0, 1, 3, 4), (g, i, j, int(fl[h]))
        assert 1 <= min(dp, dm) and max(dp, dm) == it[h] <= it_cap
        assert lo[h] - SLACK * sc <= ex <= hi[h] + SLACK * sc, (g, i, j, lo[h], ex, hi[h])
        worst = max(worst, (lo[h] - ex) / sc, (ex - hi[h]) / sc)
        if fl[h] == 0:
            assert lo[h] * hi[h] > 0 and 0 <= hi[h] - lo[h] <= rtol * min(abs(lo[h]), abs(hi[h]))
        if fl[h] == 1:
            assert hi[h] == lo[h]
        # the restatement cut at the device's depths
        assert max(dp, dm) <= 40, (g, i, j, dp, dm)  # the restatement's runs are 40 deep
        rlo, rhi, _ = er.pair_at(runs, dp, dm, mu, rtol, ftol)
        assert abs(lo[h] - rlo) <= 1e-7 * sc and abs(hi[h] - rhi) <= 1e-7 * sc, (g, i, j, lo[h], rlo, hi[h], rhi)
        if not flags:
            continue
        _, _, rit, rfl, rdep = er.pair_run(c["A"], i, j, mu, rtol=rtol, ftol=ftol, it=min(it_cap, 40), runs=runs)
        if (int(fl[h]), (dp, dm)) != (rfl, rdep):
            # only where the restatement's gap at the earlier decision sits at a threshold
            d = min(int(it[h]), rit)
            fz = [next((k for k in range(1, d + 1) if er.column(r, k, mu)[2] == 1), d) for r in runs]
            s = float(np.exp(mu))
            cp, cm = er.column(runs[0], fz[0], mu), er.column(runs[1], fz[1], mu)
            glo, ghi = 0.5 * (cp[0] - cm[1]) * s, 0.5 * (cp[1] - cm[0]) * s
            gap = ghi - glo
            near = min(abs(gap - rtol * min(abs(glo), abs(ghi))), abs(gap - ftol * 0.5 * (cp[1] + cm[1]) * s),
                       min(abs(glo), abs(ghi)))
            print(g, "pair", (i, j), "device", int(fl[h]), (dp, dm), "restatement", rfl, rdep, "gap / scale",
                  gap / sc, "distance to a threshold / scale", near / sc)
            assert near <= SLACK * sc, (g, i, j, int(fl[h]), (dp, dm), rfl, rdep, near / sc)
    print(g, len(pairs), "pairs: largest violation of the bracket in units of (E_ii + E_jj) / 2:", worst,
          "slack", SLACK)


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRAPHS)
def test_the_pair_set(kra, gpu_ctx, cases, g):
    """21-22 pairs: three sweeps on three lanes, the last partly filled."""
    c = cases[g]
    assert c["sweeps"] == 3 and len(c["list"]) in (21, 22)
    check_pairs(c, g, c["list"], c["res"])
    lo, hi, it, fl, ci = c["res"]
    kinds = [k for k in ("hub edges", "hubs", "leaf edges", "twins", "distant") for _ in c["pairs"][k]]
    for h, k in enumerate(kinds):
        if k in ("hub edges", "leaf edges"):
            assert fl[h] == 0 and 5 <= it[h] <= 14, (g, k, c["list"][h], int(fl[h]), int(it[h]))
        if k == "twins":  # e_i - e_j is an eigenvector to 0: the - column ends at depth 1
            assert ci[h, 1] == 1 and ci[h, 0] == it[h] > 1 and fl[h] == 0
            i, j = c["list"][h]
            sc = er.scale_of(c["E"], i, j)
            assert lo[h] - SLACK * sc <= c["E"][i, i] - 1.0 <= hi[h] + SLACK * sc
        if k == "distant":
            assert fl[h] in (4, 1), (g, c["list"][h], int(fl[h]))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, 8, 9, 33])
def test_call_sizes(kra, gpu_ctx, cases, size):
    """1 pair, one full sweep, one pair into a second sweep, and 33 pairs: five
    sweeps, the fifth on the first lane again."""
    import scipy.sparse as sp
    c = cases["rome"]
    I, J = sp.tril(c["A"], -1).nonzero()
    pool = c["list"] + [(int(i), int(j)) for i, j in zip(I[:40:3], J[:40:3])]
    pairs = pool[:size - 1] + [pool[0]] if size > 1 else pool[:1]  # the first pair a second time
    res = c_call(c["D"], pairs, c["mu"])
    assert gpu_ctx.stat(13) == (size + 7) // 8
    check_pairs(c, "rome", pairs, res)
    if size > 1:
        assert all(r[-1].tobytes() == r[0].tobytes() for r in res)


@pytest.mark.gpu
def test_every_edge_of_anaheim(kra, gpu_ctx, cases):
    import scipy.sparse as sp
    c = cases["anaheim"]
    I, J = sp.tril(c["A"], -1).nonzero()
    pairs = np.stack([I, J], axis=1)
    lo, hi, it, fl = kra.entries_fun_bracket(c["D"], pairs, lam_hi=c["mu"], ctx=gpu_ctx)
    sc = 0.5 * (np.diag(c["E"])[I] + np.diag(c["E"])[J])
    ex = c["E"][I, J]
    print("anaheim:", len(I), "edges, sweeps", gpu_ctx.stat(13), "steps", gpu_ctx.stat(14), "flags",
          np.bincount(fl, minlength=5).tolist(), "iter", int(it.min()), int(it.max()),
          "largest violation", float(np.max(np.maximum(lo - ex, ex - hi) / sc)))
    assert np.all(fl == 0)
    assert np.all(lo - SLACK * sc <= ex) and np.all(ex <= hi + SLACK * sc)
    assert np.all(hi - lo <= RTOL * np.minimum(abs(lo), abs(hi))) and np.all(lo > 0)


@pytest.mark.gpu
def test_values_do_not_depend_on_the_call(kra, gpu_ctx, cases):
    """A pair alone, the reversed list, a second call and the swapped
    orientation: the same bits.  Rows with i == j are diag_fun_bracket's."""
    c = cases["india"]
    pairs = c["list"]
    res = c["res"]

    def bits(r, h):
        return tuple(np.ascontiguousarray(a[h]).tobytes() for a in r)
    for h in (0, 7, 8, 14, 18, 19, 21):
        one = c_call(c["D"], [pairs[h]], c["mu"])
        assert bits(one, 0) == bits(res, h), (h, pairs[h])
    again = c_call(c["D"], pairs, c["mu"])
    rev = c_call(c["D"], pairs[::-1], c["mu"])
    swapped = c_call(c["D"], [(j, i) for i, j in pairs], c["mu"])
    for a, b, r, s in zip(res, again, rev, swapped):
        assert a.tobytes() == b.tobytes() == np.ascontiguousarray(r[::-1]).tobytes() == s.tobytes()
    # the wrapper: diagonal rows in place
    mixed = np.array([pairs[0], (pairs[0][0], pairs[0][0]), pairs[5], (pairs[5][1], pairs[5][1]), pairs[0][::-1]])
    lo, hi, it, fl = kra.entries_fun_bracket(c["D"], mixed, lam_hi=c["mu"], ctx=gpu_ctx)
    dlo, dhi, dit, dfl = kra.diag_fun_bracket(c["D"], [pairs[0][0] + 1, pairs[5][1] + 1], lam_hi=c["mu"], ctx=gpu_ctx)
    for got, want in ((lo, dlo), (hi, dhi), (it, dit), (fl, dfl)):
        assert got[[1, 3]].tobytes() == want.tobytes()
    for a, k in zip((lo, hi, it, fl), range(4)):
        assert a[0].tobytes() == a[4].tobytes() == res[k][0].tobytes()
        assert a[2].tobytes() == res[k][5].tobytes()


@pytest.mark.gpu
def test_corner_cases(kra, gpu_ctx, cases):
    c = cases["rome"]
    i, j = c["list"][0]
    ex, sc = c["E"][i, j], er.scale_of(c["E"], i, j)
    res = c_call(c["D"], [(i, j)], c["mu"], it=3)
    print("it = 3:", res, "exact", ex)
    assert (res[2][0], res[3][0], res[4].tolist()) == (3, 3, [[3, 3]])
    assert res[0][0] - SLACK * sc <= ex <= res[1][0] + SLACK * sc and res[1][0] - res[0][0] > 1e-3 * ex
    check_pairs(c, "rome", [(i, j)], res, it_cap=3, flags=False)
    lo, hi, it, fl, _ = c_call(c["D"], [(i, j)], 0.5 * float(c["w"][-1]))
    print("lam_hi = 0.5 lambda_max:", lo, hi, it, fl)
    assert fl[0] == 2 and np.isnan(lo[0]) and np.isnan(hi[0]) and it[0] <= 40
    # india's isolated node with a hub: the entry is 0
    c = cases["india"]
    deg = np.diff(c["A"].indptr)
    iso, hub = int(np.flatnonzero(deg == 0)[0]), int(np.argmax(deg))
    lo, hi, it, fl, ci = c_call(c["D"], [(iso, hub)], c["mu"])
    sc = er.scale_of(c["E"], iso, hub)
    print("isolated node with a hub:", lo, hi, it, fl, ci)
    assert fl[0] in (4, 1) and lo[0] - SLACK * sc <= 0.0 <= hi[0] + SLACK * sc and hi[0] - lo[0] <= FTOL * sc * 1.01


@pytest.mark.gpu
def test_dense_branch(kra, gpu_ctx):
    A = load_graph("denmark")
    assert A.shape[0] == 96
    E, _ = er.exp_dense(A)
    pairs = np.array([[85, 0], [0, 85], [42, 7], [85, 0], [3, 3]])
    lo, hi, it, fl = kra.entries_fun_bracket(A, pairs, ctx=gpu_ctx)
    assert np.all(it == 0) and np.all(fl == 0) and np.array_equal(lo, hi)
    assert lo == pytest.approx(E[pairs[:, 0], pairs[:, 1]], rel=1e-10, abs=1e-12)
    assert lo[0].tobytes() == lo[1].tobytes() == lo[3].tobytes()


@pytest.mark.gpu
def test_find_top_edges_bracket(kra, gpu_ctx, cases):
    import scipy.sparse as sp
    c = cases["anaheim"]
    A, E = c["A"], c["E"]
    I, J = kra.greedy._tril_edges(sp.csc_matrix(A))
    ex = E[I, J]
    # every edge a candidate: the stochastic ranking decides nothing
    edges, info = kra.find_top_edges_bracket(c["D"], 10, ncand=len(I), lam_hi=c["mu"], ctx=gpu_ctx)
    cand, lo, hi = info["candidates"], info["lo"], info["hi"]
    assert cand.shape == (len(I), 2) and np.all(cand[:, 0] > cand[:, 1]) and edges.tolist() == cand[:10].tolist()
    assert len({tuple(e) for e in cand.tolist()}) == len(I)
    assert np.all(lo[:-1] >= lo[1:]) and info["separated"] == bool(np.all(lo[:-1] > hi[1:]))
    cex = E[cand[:, 0] - 1, cand[:, 1] - 1]
    sc = 0.5 * (np.diag(E)[cand[:, 0] - 1] + np.diag(E)[cand[:, 1] - 1])
    assert np.all(lo - SLACK * sc <= cex) and np.all(cex <= hi + SLACK * sc)
    sep = lo[:-1] > hi[1:]  # wherever two neighbours are separated their exact order is proved
    above = lo[:-1] > np.maximum.accumulate(hi[::-1])[::-1][1:]  # and r lies above all that follow it
    print("find_top_edges_bracket: every edge,", int(sep.sum()), "of", len(sep), "neighbours separated; separated",
          info["separated"])
    assert np.all(cex[:-1][sep] > cex[1:][sep])
    want = np.lexsort((np.arange(len(I)), -ex))
    k = int(np.argmin(above)) if not above.all() else len(above)  # the proved prefix
    assert cand[:k].tolist() == np.stack([I[want] + 1, J[want] + 1], axis=1)[:k].tolist()
    # defaults: 4 num candidates, the returned ones their head by lower bound
    edges, info = kra.find_top_edges_bracket(c["D"], 5, ctx=gpu_ctx)
    cand, lo, hi = info["candidates"], info["lo"], info["hi"]
    assert cand.shape == (20, 2) and edges.tolist() == cand[:5].tolist() and np.all(lo[:-1] >= lo[1:])
    assert {tuple(e) for e in cand.tolist()} <= {(int(i) + 1, int(j) + 1) for i, j in zip(I, J)}
    cex = E[cand[:, 0] - 1, cand[:, 1] - 1]
    sc = 0.5 * (np.diag(E)[cand[:, 0] - 1] + np.diag(E)[cand[:, 1] - 1])
    assert np.all(lo - SLACK * sc <= cex) and np.all(cex <= hi + SLACK * sc)
    # usable as greedy_krylov's top: 1-based rows with i > j of existing edges
    assert np.all(edges[:, 0] > edges[:, 1]) and all(A[i - 1, j - 1] != 0 for i, j in edges)


@pytest.mark.gpu
def test_abi_rejects_an_index_equal_to_n(kra, gpu_ctx, cases):
    from krylov_robustness_amd import _lib
    c = cases["anaheim"]
    n = c["A"].shape[0]
    with pytest.raises(kra.KrylovError, match="pair index out of range") as e:
        c_call(c["D"], [(0, n)], c["mu"])
    assert e.value.code == _lib.KT_ERR_ARG
    lo, hi, it, fl, ci = c_call(c["D"], [(0, n - 1)], c["mu"], rtol=0.0, ftol=0.0)  # the defaults
    sc = er.scale_of(c["E"], 0, n - 1)
    assert lo[0] - SLACK * sc <= c["E"][0, n - 1] <= hi[0] + SLACK * sc and fl[0] in (0, 4)
