#!/usr/bin/env python3
"""Bit parity of the probe-Lanczos sweep engine between two builds.

The sweeps use no atomics, so a change to the host code that queues them
(kt_slq.cpp, kt_diag_fun.cpp) must leave every result the same bits.  This
tool runs a fixed set of small cases through the public Python API -- every
caller of the sweep engine, at the widths, depths, lane counts and start forms
at which the engine takes another path -- and writes every returned array and
the context counters (yform_redone, stat 5, 6, 7) to one .npz:

    python tools/sweep_parity.py run --root <checkout> --out <file.npz>

`--root` names the checkout whose package and library are loaded (default:
the one this file is in).  Run it twice on the build to compare against (what
differs between those two runs is not reproducible and can only be compared
at a tolerance) and once on the build under test, each in its own process:

    python tools/sweep_parity.py compare base1.npz base2.npz new.npz --out parity.json

exits non-zero unless every reproducible output is np.array_equal and every
other one within rtol 1e-8, atol 1e-10 max|base| (the tolerance the GPU tests
of these entry points use against their references).

Run on demand; not a test, and its outputs are not fixtures: kernel work
legitimately changes low bits.
"""
import argparse
import json
import os
import sys

import numpy as np

WIDTHS = [1, 8, 16, 32]
DEPTHS = [2, 3, 4, 30]  # 2, 3: the first / second step is the sweep's last pass
LANES = [1, 2, 3]


def star(n):
    """Node 0 joined to every other node, as tests/test_gpu_int_start.py builds
    it: the Krylov space is exhausted after three steps, so the guard trips and
    the sweeps are redone by the explicit sweep."""
    import scipy.sparse as sp
    leaves = np.arange(1, n)
    i, j = np.zeros(n - 1, dtype=np.int64), leaves
    A = sp.coo_matrix((np.ones(2 * i.size), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(n, n))
    return A.tocsr()


def setenv(**kw):
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)


def run(out_path):
    import krylov_robustness_amd as kra
    from krylov_robustness_amd import graphs

    unit = graphs.chung_lu(3_000, 30_000, seed=4)
    deg = np.diff(unit.indptr)
    assert np.all(unit.data == 1.0) and deg.max() > 64 and deg.min() <= 4
    mats = {"unit": unit, "weighted": graphs.symmetric_weights(unit), "star": star(200)}
    res = {}

    def put(key, *arrays):
        assert key not in res, key
        res[key] = np.concatenate([np.atleast_1d(np.asarray(a, dtype=np.float64)).ravel(order="F") for a in arrays])

    def counters(key, ctx):
        res[key + "/counters"] = np.array([ctx.yform_redone(), ctx.stat(5), ctx.stat(6), ctx.stat(7)], dtype=np.int64)

    setenv(KT_LC_YFORM=None, KT_LC_YBASIS=None)
    for yform in ("0", None):  # read when the context is created
        setenv(KT_SLQ_YFORM=yform, KT_SLQ_LANES=None, KT_SLQ_INT0=None)
        ctx = kra.Context(0)
        for gname, A in mats.items():
            tag = f"yform={yform or 'default'}/{gname}"
            D = kra.DeviceMatrix(A, ctx)
            n = A.shape[0]
            for P in WIDTHS:
                for m in DEPTHS:
                    for lanes in LANES:
                        for int0 in (0, 1):
                            setenv(KT_SLQ_LANES=lanes, KT_SLQ_INT0=int0)
                            s1, s2, q = kra.slq_quadforms(D, 2 * P + (P + 1) // 2, m, seed=12, block=P, ctx=ctx)
                            put(f"{tag}/slq/P={P}/m={m}/lanes={lanes}/int0={int0}", s1, s2, q)
            setenv(KT_SLQ_LANES=None, KT_SLQ_INT0=None)
            counters(f"{tag}/slq", ctx)
            # both tickets outstanding at once
            t1 = kra.slq_submit(D, 40, 30, seed=1, block=8, ctx=ctx)
            t2 = kra.slq_submit(D, 37, 20, seed=2, probe_offset=5, block=16, ctx=ctx)
            put(f"{tag}/submit/first", *kra.slq_collect(t1))
            put(f"{tag}/submit/second", *kra.slq_collect(t2))
            counters(f"{tag}/submit", ctx)
            for m_max in (40, 128):
                s1, s2, q, info = kra.slq_quadforms_auto(D, 20, m_max=m_max, seed=3, block=8, return_info=True,
                                                         ctx=ctx)
                put(f"{tag}/auto/m_max={m_max}", s1, s2, q, info["depth"], info["capped"])
            counters(f"{tag}/auto", ctx)
            # lanczos_columns_split: explicit sweeps with basis, basis-forming
            # y-form sweeps (KT_LC_YBASIS=1), forms-only y-form chunks (mc_trace)
            X = np.random.default_rng(5).standard_normal((n, 5))
            for lc in (None, "0"):
                setenv(KT_LC_YFORM=lc)
                put(f"{tag}/fmv/lc_yform={lc or 'default'}", kra.lanczos_fmv(D, X, m=10, ctx=ctx))
                setenv(KT_LC_YBASIS=1)
                put(f"{tag}/fmv_ybasis/lc_yform={lc or 'default'}", kra.lanczos_fmv(D, X, m=10, ctx=ctx))
                setenv(KT_LC_YBASIS=None)
                # on the star its forms-only columns trip the guard: the per-column redo
                put(f"{tag}/trace_exp/lc_yform={lc or 'default'}", kra.trace_exp(D, method="lanczos", ctx=ctx))
            setenv(KT_LC_YFORM=None)
            counters(f"{tag}/columns", ctx)
            # probe_sweeps; on the star the whole-sweep redo with basis
            Q = np.linalg.qr(np.random.default_rng(6).standard_normal((n, 3)))[0]
            pairs = np.random.default_rng(7).integers(0, n, size=(20, 2))
            for dname, defl in (("none", None), ("three", Q)):
                r = kra.diag_fun(D, 10, m=12, seed=8, block=4, deflate=defl, ctx=ctx)
                put(f"{tag}/diag_fun/deflate={dname}", r.d0, r.dsum, r.dsum2, r.sum_q, r.sum_q2)
                r = kra.entries_fun(D, pairs, 10, m=12, seed=8, block=4, deflate=defl, ctx=ctx)
                put(f"{tag}/entries_fun/deflate={dname}", r.e0, r.esum, r.esum2, r.sum_q, r.sum_q2)
            counters(f"{tag}/probe_sweeps", ctx)
            D.close()
        ctx.close()
    np.savez(out_path, **res)
    print(f"sweep_parity: {len(res)} outputs -> {out_path}")


def compare(base1, base2, new, out_path):
    a, b, c = (dict(np.load(p)) for p in (base1, base2, new))
    assert a.keys() == b.keys() == c.keys(), "the runs recorded different cases"
    cases, ok, at_tol = {}, True, []
    for k in sorted(a):
        repro = a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
        same_shape = a[k].shape == c[k].shape
        diff = float(np.max(np.abs(a[k].astype(np.float64) - c[k]))) if same_shape and a[k].size else 0.0
        if repro or k.endswith("/counters"):
            mode, passed = "bitwise", same_shape and np.array_equal(a[k], c[k])
        else:
            mode = "tolerance"
            passed = same_shape and np.allclose(c[k], a[k], rtol=1e-8, atol=1e-10 * np.abs(a[k]).max())
            at_tol.append(k)
        cases[k] = {"mode": mode, "reproducible_on_base": bool(repro), "max_abs_diff": diff, "pass": bool(passed)}
        ok &= bool(passed)
    report = {"outputs": len(cases), "bitwise": len(cases) - len(at_tol), "at_tolerance": at_tol,
              "failed": [k for k, v in cases.items() if not v["pass"]], "pass": ok, "cases": cases}
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(f"sweep_parity: {report['outputs']} outputs, {report['bitwise']} bitwise, "
          f"{len(at_tol)} at tolerance, {len(report['failed'])} failed -> {out_path}")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("base1")
    c.add_argument("base2")
    c.add_argument("new")
    c.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.cmd == "run":
        sys.path.insert(0, os.path.abspath(args.root))
        run(args.out)
        return 0
    return compare(args.base1, args.base2, args.new, args.out)


if __name__ == "__main__":
    sys.exit(main())
