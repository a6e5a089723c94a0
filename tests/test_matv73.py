"""MAT v7.3 (HDF5) reader and dataset preparation.

Pinning: the reader's output for the three HDF5 datasets of
datasets_paper/Misc is checked against digests recorded in
tests/golden/v73_values.json (make_golden.py --v73), and independently
against the file's own redundancy -- CollegeMsg stores its 59,835 temporal
edges beside Problem.A, and accumulating them must reproduce A entry for
entry (multiplicities included); Drugs/as_735 store the same matrix twice
(Problem.A and W).  The MAT-files are fixtures under tests/golden/datasets_paper
(make_golden.py --mat: the three v7.3 files as the reference ships them, and
Transport/Hawaii.mat's Problem.A in a compressed MAT v5 file), so every test
here runs wherever the repository is checked out."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg

from conftest import GOLDEN, load_v73_graph

REF = os.path.join(GOLDEN, "datasets_paper")
NAMES = ["Drugs", "as_735", "CollegeMsg"]


@pytest.fixture(scope="module")
def vals():
    with open(os.path.join(GOLDEN, "v73_values.json")) as f:
        return json.load(f)


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name", NAMES)
def test_reader_digests(name, vals):
    from krylov_robustness_amd import datasets as ds
    path = os.path.join(REF, "Misc", name + ".mat")
    assert ds.is_v73(path)
    P = ds.load_variable(path, "Problem")
    R = sp.csc_matrix(P["A"])
    rec = vals[name.lower()]
    assert list(R.shape) == rec["raw_shape"] and R.nnz == rec["raw_nnz"]
    assert R.sum() == rec["raw_sum"]
    assert _sha(R.indptr.astype(np.int64)) == rec["raw_sha_indptr"]
    assert _sha(R.indices.astype(np.int64)) == rec["raw_sha_indices"]
    assert _sha(R.data.astype(np.float64)) == rec["raw_sha_data"]
    assert isinstance(P["name"], str) and P["name"] == rec["name"]


def test_collegemsg_temporal_edges_rebuild_A():
    from krylov_robustness_amd import matv73
    P = matv73.loadmat(os.path.join(REF, "Misc", "CollegeMsg.mat"))["Problem"]
    A, te = P["A"], P["aux"]["temporal_edges"]
    assert te.shape == (59835, 3)
    assert np.all(np.diff(te[:, 2]) >= 0)  # time-ordered
    B = sp.csc_matrix((np.ones(len(te)), (te[:, 0].astype(int) - 1, te[:, 1].astype(int) - 1)),
                      shape=A.shape)
    assert abs(B - A).max() == 0
    assert P["kind"] == "directed temporal multigraph"


@pytest.mark.parametrize("name", ["Drugs", "as_735"])
def test_struct_fields_and_duplicate_matrix(name):
    from krylov_robustness_amd import matv73
    d = matv73.loadmat(os.path.join(REF, "Misc", name + ".mat"))
    A, W = d["Problem"]["A"], d["W"]
    assert abs(A - W).max() == 0
    n = A.shape[0]
    assert d["C_NL"].shape == (n, 1) and d["numModules_NL"].shape == (1, 1)
    assert 0.0 < float(d["modularity_NL"][0, 0]) < 1.0


@pytest.mark.parametrize("name", NAMES)
def test_prepared_graph_matches_fixture(name):
    from krylov_robustness_amd import datasets as ds
    A = ds.load_unweighted(os.path.join(REF, "Misc", name + ".mat"))
    G = load_v73_graph(name.lower())
    assert A.shape == G.shape and abs(A - G).max() == 0


def test_load_variable_v5_struct():
    """MAT v5 files go through scipy with the same dict shape."""
    from krylov_robustness_amd import datasets as ds
    path = os.path.join(REF, "Transport", "Hawaii.mat")
    assert not ds.is_v73(path)
    A = ds.load_unweighted(path)
    assert A.shape == (21774, 21774) and A.nnz == 52014


@pytest.mark.parametrize("name", [n.lower() for n in NAMES])
def test_prepared_fixture_properties(name, vals):
    """test_unweighted_make.m:45-52: symmetric 0/1, no loops, connected."""
    A = load_v73_graph(name)
    rec = vals[name]
    assert A.shape == (rec["n"], rec["n"]) and A.nnz == rec["nnz"]
    assert abs(A - A.T).max() == 0 and np.all(A.data == 1.0)
    assert A.diagonal().sum() == 0
    assert csg.connected_components(A, directed=False)[0] == 1


def test_prepare_unweighted_small():
    from krylov_robustness_amd import datasets as ds
    # directed multigraph with a loop and two components (sizes 3 and 2)
    i = np.array([0, 1, 1, 2, 2, 3])
    j = np.array([1, 0, 2, 2, 0, 4])
    A = sp.csr_matrix((np.array([2.0, 1, 5, 1, 1, 1]), (i, j)), shape=(5, 5))
    P = ds.prepare_unweighted(A)
    E = np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=float)
    assert np.array_equal(P.toarray(), E)
    W = ds.prepare_weighted(A)
    assert W.max() == 1.0 and W[1, 2] == 1.0
