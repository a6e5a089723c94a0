"""Row -> XCD schedules for run.py (each returns order, xoff), and physical
relabellings (relabel_*: each returns new2old over the hubs-first labels)."""
import numpy as np


def _pack(groups, A, key=None):
    deg = np.diff(A.indptr)
    lists = []
    for g in range(8):
        rows = np.where(groups == g)[0]
        if key is not None:
            rows = rows[np.argsort(key[rows], kind="stable")]
        lists.append(rows)
    order = np.concatenate(lists)
    xoff = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    return order, xoff


def contiguous(A):
    """Each XCD takes one contiguous eighth of the rows (by nnz)."""
    cum = A.indptr[1:]
    g = np.minimum((cum * 8) // (A.nnz + 1), 7)
    return _pack(g, A)


def _balanced_split(order, A, parts=8):
    nz = np.diff(A.indptr)[order]
    cum = np.cumsum(nz)
    g = np.minimum((cum * parts) // (cum[-1] + 1), parts - 1)
    xoff = np.concatenate([[0], np.searchsorted(g, np.arange(1, parts)), [len(order)]])
    return order, xoff


def _primary(A, t0):
    """Per row: its highest-degree neighbour that is not among the top t0
    (hubs-first labels: the smallest column index >= t0), n if none."""
    n = A.shape[0]
    col = A.indices.astype(np.int64)
    col[col < t0] = n
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    prim = np.full(n, n, dtype=np.int64)
    np.minimum.at(prim, rows, col)
    return prim


def sort_primary_4k(A):
    prim = _primary(A, 4096)
    order = np.argsort(prim, kind="stable")
    return _balanced_split(order, A)


def sort_primary_0(A):
    prim = _primary(A, 0)
    order = np.argsort(prim, kind="stable")
    return _balanced_split(order, A)


def _hgroup(A, t0, k, order_within=None):
    """Columns of degree rank [t0, t0 + 8k) get a home XCD ((c - t0) % 8);
    each row goes to the XCD holding most of its home-set neighbours, under
    a 1 % nnz balance cap (greedy, strongest preference first)."""
    n = A.shape[0]
    deg = np.diff(A.indptr)
    col = A.indices.astype(np.int64)
    rows = np.repeat(np.arange(n), deg)
    inh = (col >= t0) & (col < t0 + 8 * k)
    cnt = np.zeros((n, 8), dtype=np.int32)
    np.add.at(cnt, (rows[inh], (col[inh] - t0) % 8), 1)
    pref = np.argsort(-cnt, axis=1, kind="stable")
    best = cnt.max(axis=1)
    cap = A.nnz / 8 * 1.01
    load = np.zeros(8)
    g = np.full(n, -1, dtype=np.int64)
    for r in np.argsort(-best, kind="stable"):
        for q in pref[r]:
            if load[q] + deg[r] <= cap:
                g[r] = q
                load[q] += deg[r]
                break
        else:
            q = int(np.argmin(load))
            g[r] = q
            load[q] += deg[r]
    lists = []
    for q in range(8):
        rr = np.where(g == q)[0]
        if order_within is not None:
            rr = rr[np.argsort(order_within[rr], kind="stable")]
        lists.append(rr)
    order = np.concatenate(lists)
    xoff = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    return order, xoff


def hgroup_4k_16k(A):
    return _hgroup(A, 4096, 16384)


def hgroup_4k_32k(A):
    return _hgroup(A, 4096, 32768)


def hgroup_0_64k(A):
    return _hgroup(A, 0, 65536)


def hgroup_4k_16k_prim(A):
    return _hgroup(A, 4096, 16384, _primary(A, 4096))


def _relabel_primary(A, orig, exact, t0=4096, long_thresh=64):
    """The library's row order (csrc/kt_order.h hub_order) as a PHYSICAL
    relabelling of the hubs-first graph A -- rows and columns both move, where
    the schedules above only reorder processing: degree class descending
    (ceil(deg / 4) up to long_thresh and the exact degree above it, or the
    exact degree throughout), then the highest-degree neighbour of degree rank
    >= t0, then the original index orig[r] of hubs-first row r."""
    deg = np.diff(A.indptr)
    cls = deg if exact else np.where(deg > long_thresh, deg, (deg + 3) // 4)
    return np.lexsort((orig, _primary(A, t0), -cls))


def relabel_primary_quad(A, orig):
    return _relabel_primary(A, orig, exact=False)


def relabel_primary_exact(A, orig):
    return _relabel_primary(A, orig, exact=True)


def _relabel_chain(A, orig, cap=0, long_thresh=64):
    """csrc/kt_order.h chain_order on top of relabel_primary_quad: the base
    order is walked and from each row not yet placed a run starts -- the row,
    then its not yet placed same-class neighbour of smallest degree rank (in
    the hubs-first labels of A the rank IS the label, and sorted indices list
    a row's neighbours by rank), and so on from that one until none is left
    (or the run holds `cap` rows, 0 = no cap).  Rows above long_thresh are not
    chained."""
    n = A.shape[0]
    indptr, indices = A.indptr, A.indices
    deg = np.diff(indptr)
    cls = np.where(deg > long_thresh, -1, (deg + 3) // 4)  # -1: never eligible
    # per row: its same-class neighbours, ascending label, self loops dropped
    rows = np.repeat(np.arange(n), deg)
    keep = (cls[rows] == cls[indices]) & (cls[rows] >= 0) & (rows != indices)
    cptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).tolist()
    cand = indices[keep].tolist()
    placed = bytearray(n)
    out = []
    for start in relabel_primary_quad(A, orig).tolist():
        if placed[start]:
            continue
        cur, length = start, 0
        while cur >= 0:
            placed[cur] = 1
            out.append(cur)
            length += 1
            nxt = -1
            if not cap or length < cap:
                for k in range(cptr[cur], cptr[cur + 1]):
                    if not placed[cand[k]]:
                        nxt = cand[k]
                        break
            cur = nxt
    return np.asarray(out, dtype=np.int64)


def relabel_chain(A, orig):
    return _relabel_chain(A, orig)


def relabel_chain_pairs(A, orig):
    return _relabel_chain(A, orig, cap=2)


def relabel_chain_cap8(A, orig):
    return _relabel_chain(A, orig, cap=8)


def contiguous_chunks(A, P=16, long_thresh=64, chunk=64):
    """Schedule for the relabelled graphs above: each XCD walks one contiguous
    slice of the short rows, cut at 64-row chunk boundaries into eight slices
    of equal weight (a row weighs its nonzeros plus 3, the model's lines per
    row); the long rows lead the order and are dealt as in run.py's baseline."""
    n = A.shape[0]
    deg = np.diff(A.indptr)
    n_long = int((deg > long_thresh).sum())
    assert np.all(deg[:n_long] > long_thresh)
    lists = [list(range(x, n_long, 8)) for x in range(8)]
    w = np.cumsum(deg[n_long:] + 3)
    nchunks = -(-(n - n_long) // chunk)
    cw = w[np.minimum(np.arange(1, nchunks + 1) * chunk, n - n_long) - 1] if nchunks else np.zeros(0)
    cuts = [0] + [int(np.searchsorted(cw, cw[-1] * x / 8)) for x in range(1, 8)] + [nchunks]
    for x in range(8):
        lists[x] = np.concatenate([np.asarray(lists[x], dtype=np.int64),
                                   np.arange(n_long + cuts[x] * chunk, min(n_long + cuts[x + 1] * chunk, n))])
    order = np.concatenate(lists)
    xoff = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    return order, xoff
