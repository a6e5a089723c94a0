"""Measured numbers behind the adaptive Lanczos depth (KT_AFUN_LANCZOS_AUTO,
kt_lanczos_fmv_auto), on the CPU with the numpy oracle.  Build container
only; tests/test_adaptive_host.py and tests/test_gpu_adaptive.py read the JSON
this writes, DESIGN.md §4 quotes it.

  * graphs: anaheim, oregon_A0, and the scaled graphs on which a fixed depth
    of 30 drifts: 16 anaheim, 16 rome, 16 and 40 times the 40 x 40 grid, 40 rome.
  * rtol sweep: for the first 10 Rademacher probes (seed 0) of each graph, the
    oracle's tridiagonal (lanczos_probe_tridiag, 130 steps) and the depth at
    which the library's host rule (kt_host_quad_converged) first holds, for
    rtol = 1e-10 .. 1e-16, quadrature-only and f(A) x columns.  The default is
    ten times the smallest power of ten at which every column stops before
    depth 128.  Also written to profiles/adaptive/rtol_sweep.txt.
  * gaps: |trace_exp_lanczos(B, m = 128, seed 0) / trace_exp(B, seed 0) - 1| per
    graph (same probes, Lanczos-exp Afun at a depth that leaves no truncation
    against the reference's expmv Afun): ten times the worst is the device
    tolerance of test_gpu_adaptive.py item 1, not tighter than 1e-12.  The
    oracle's lanczos_fmv solves T with scipy's eigh_tridiagonal (stemr), which
    fails to converge at m = 128 on oregon_A0 (LAPACK info = 22: the record
    runs on past a near-breakdown); the composition here is the oracle's
    mc_trace and lanczos_probe_tridiag with numpy.linalg.eigh on the dense T,
    on every graph.
  * spread: the host QL quadrature (kt_host_tridiag_quad) against
    numpy.linalg.eigh on the sweep's tridiagonals at depths 3, 8, 31, 32, 128
    (relative, scaled by exp(-theta_max)): the tolerance unit of
    tests/test_gpu_quad_check.py.

  python tests/golden/make_adaptive_fixture.py [--skip-gaps]
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
from oracle import krylov_oracle as ko  # noqa: E402
from krylov_robustness_amd import _lib  # noqa: E402

RTOLS = [10.0 ** -k for k in range(10, 17)]
NPROBE = 10
MAXD = 128


def grid_graph(a, b):
    """Adjacency of the a x b grid (4-neighbour), unit weights."""
    pa = sp.diags([np.ones(a - 1), np.ones(a - 1)], [-1, 1])
    pb = sp.diags([np.ones(b - 1), np.ones(b - 1)], [-1, 1])
    return sp.csr_matrix(sp.kron(sp.identity(b), pa) + sp.kron(pb, sp.identity(a)))


def load_graph(name):
    z = np.load(os.path.join(HERE, "graphs.npz"))
    n = int(z[name + "__n"][0])
    return sp.csr_matrix((z[name + "__data"], z[name + "__indices"], z[name + "__indptr"]), shape=(n, n))


def graphs():
    g = grid_graph(40, 40)
    return {"anaheim": load_graph("anaheim"), "oregon_A0": load_graph("oregon_A0"),
            "anaheim_x16": load_graph("anaheim") * 16.0, "rome_x16": load_graph("rome") * 16.0,
            "grid40_x16": g * 16.0, "rome_x40": load_graph("rome") * 40.0, "grid40_x40": g * 40.0}


def lanczos_fmv_dense(A, X, m):
    """ko.lanczos_fmv (fun = exp) with numpy.linalg.eigh on the dense T."""
    Y = np.zeros_like(X)
    for c in range(X.shape[1]):
        x = X[:, c]
        nx = np.linalg.norm(x)
        if nx == 0:
            continue
        a, e, V, _ = ko.lanczos_probe_tridiag(A, x, m)
        theta, W = np.linalg.eigh(np.diag(a) + np.diag(e, 1) + np.diag(e, -1))
        coef = W @ (np.exp(theta) * W[0, :])
        s = np.sign(V[:, 0] @ x) or 1.0
        Y[:, c] = s * nx * (V @ coef)
    return Y


def trace_exp_lanczos(A, m):
    return ko.mc_trace(lambda X: lanczos_fmv_dense(A, X, m), A.shape[0], 1e-4, 1000, 1, seed=0)[0]


def host_rule(lib, al, off, j, want, rtol):
    cv, q = C.c_int(), C.c_double()
    a = np.ascontiguousarray(al[:j])
    o = np.ascontiguousarray(off[:j if want else max(j - 1, 1)])
    st = lib.kt_host_quad_converged(j, a.ctypes.data_as(_lib._dp), o.ctypes.data_as(_lib._dp), 0, want, rtol,
                                    C.byref(cv), C.byref(q))
    assert st == 0
    return bool(cv.value), q.value


def stop_depth(lib, al, off, want, rtol):
    for j in range(8, min(MAXD, len(al) - 1) + 1):
        if host_rule(lib, al, off, j, want, rtol)[0]:
            return j
    return None


def main():
    lib = _lib.load()
    rec = {"rtols": RTOLS, "nprobe": NPROBE, "max_depth": MAXD, "sweep": {}, "gaps": {}, "spread": {}}
    G = graphs()
    tri = {}
    for name, A in G.items():
        t0 = time.time()
        Z = ko.rademacher(A.shape[0], np.arange(NPROBE), 0)
        tri[name] = [ko.lanczos_probe_tridiag(A, Z[:, c], MAXD + 2)[:2] for c in range(NPROBE)]
        print(f"{name}: n={A.shape[0]} tridiagonals {time.time() - t0:.1f}s", flush=True)
    lines = ["# adaptive Lanczos depth: rtol against the largest stopping depth over the first 10",
             "# Rademacher probes (seed 0) of each graph, fun = exp; host rule on the oracle's tridiagonals.",
             "# '-' : a column had not stopped by depth 128.  columns: quadrature-only / f(A)x",
             "graph            " + "  ".join(f"{r:>9.0e}" for r in RTOLS)]
    spread = 0.0
    for name in G:
        rec["sweep"][name] = {"quad": [], "fmv": []}
        cells = []
        for rtol in RTOLS:
            dq = [stop_depth(lib, al, off, 0, rtol) for al, off in tri[name]]
            df = [stop_depth(lib, al, off, 1, rtol) for al, off in tri[name]]
            mq = None if None in dq else max(dq)
            mf = None if None in df else max(df)
            rec["sweep"][name]["quad"].append(mq)
            rec["sweep"][name]["fmv"].append(mf)
            cells.append(f"{mq if mq else '-':>4}/{mf if mf else '-':<4}")
        lines.append(f"{name:<16} " + "  ".join(cells))
        print(lines[-1], flush=True)
        # host QL against numpy.linalg.eigh on the same tridiagonals
        worst = 0.0
        for al, off in tri[name]:
            for j in (3, 8, 31, 32, MAXD):
                if j >= len(al):
                    continue
                q = host_rule(lib, al, off, j, 0, 1e-14)[1]
                T = np.diag(al[:j]) + np.diag(off[:j - 1], 1) + np.diag(off[:j - 1], -1)
                w, V = np.linalg.eigh(T)
                qn = float(np.sum(V[0] ** 2 * np.exp(w - w.max())))
                worst = max(worst, abs(q - qn) / abs(qn))
        rec["spread"][name] = worst
        spread = max(spread, worst)
    ok = [r for k, r in enumerate(RTOLS)
          if all(rec["sweep"][g]["quad"][k] is not None and rec["sweep"][g]["fmv"][k] is not None and
                 max(rec["sweep"][g]["quad"][k], rec["sweep"][g]["fmv"][k]) < MAXD for g in G)]
    rec["rtol_smallest_all_stop"] = min(ok)
    rec["rtol_default"] = 10.0 * min(ok)
    rec["spread_max"] = spread
    lines.append(f"# smallest rtol at which every column stops before depth 128: {min(ok):.0e}; "
                 f"default = 10 x that = {10 * min(ok):.0e}")
    lines.append(f"# host QL vs numpy.linalg.eigh quadrature, worst relative spread: {spread:.2e}")
    os.makedirs(os.path.join(ROOT, "profiles", "adaptive"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "adaptive", "rtol_sweep.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]), flush=True)
    out = os.path.join(HERE, "adaptive_values.json")
    if "--skip-gaps" in sys.argv and os.path.exists(out):
        with open(out) as f:
            rec["gaps"] = json.load(f).get("gaps", {})
    else:
        for name, A in G.items():
            t0 = time.time()
            ref = ko.trace_exp(A, seed=0)
            lz = trace_exp_lanczos(A, MAXD)
            f30 = trace_exp_lanczos(A, 30)
            rec["gaps"][name] = {"trace_exp": ref, "lanczos128": lz, "gap128": abs(lz / ref - 1.0),
                                 "gap30": abs(f30 / ref - 1.0)}
            print(f"{name}: gap128 {rec['gaps'][name]['gap128']:.2e} gap30 {rec['gaps'][name]['gap30']:.2e} "
                  f"{time.time() - t0:.1f}s", flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote adaptive_values.json", flush=True)


if __name__ == "__main__":
    main()
