"""CPU-only: tests/tsne_nn_ref.py -- the float64 restatement the sparse-affinity t-SNE kernels are held to
(tests/test_gpu_tsne_nn.py) -- against scikit-learn's private _joint_probabilities_nn where it is installed, against the dense
restatement tests/tsne_ref.py where the neighbour list is the whole row, and against its own invariants."""
import numpy as np
import pytest

import tsne_nn_ref as nn
import tsne_ref as ref


@pytest.fixture(scope="module")
def case300():
    X, labels = nn.blobs(300, 40, 3, 0)
    return dict(X=X, labels=labels, perp=30.0, **nn.affinities(X, 30.0))


def test_neighbour_count_and_pattern(case300):
    c = case300
    assert c["k"] == 91 and c["idx"].shape == (300, 91)
    rp, col, val = nn.joint_csr(c["idx"], c["cond"])
    assert len(col) == 29470 and rp[-1] == len(col) and len(col) <= 2 * 300 * 91
    assert nn.n_neighbours(61, 20.0) == 60 and nn.n_neighbours(33000, 10.0) == 31 and nn.n_neighbours(1000, 85.0) == 256


def test_joint_matches_scikit_learn(case300):
    """scikit-learn stops its search at an entropy error of 1e-5; measured agreement 5.1e-6 of max(P) against 1.7.2"""
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    sparse = pytest.importorskip("scipy.sparse")
    c = case300
    n, k = c["idx"].shape
    G = sparse.csr_matrix((c["d2"].ravel(), c["idx"].ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    Ps = np.asarray(tsne._joint_probabilities_nn(G, c["perp"], 0).todense())
    err = np.abs(Ps - c["P"]).max() / c["P"].max()
    print("sparse joint P vs scikit-learn: %.3g of max(P)" % err)
    assert err <= 2e-5


def test_whole_row_of_neighbours_is_the_dense_joint():
    """N = 61, perplexity 20: k = 60 = N - 1, every other point is a neighbour, and the sparse joint is the dense one (the dense
    restatement keeps its distances in float64, this one rounds them to float32 first, hence not bit for bit)"""
    X, _ = nn.blobs(61, 40, 3, 1)
    a = nn.affinities(X, 20.0)
    assert a["k"] == 60
    P = ref.affinities(X, 20.0)[0]
    err = np.abs(a["P"] - P).max() / P.max()
    print("k = N - 1: sparse vs dense restatement %.3g of max(P)" % err)
    assert err <= 1e-7
    rp, col, val = nn.joint_csr(a["idx"], a["cond"])
    assert len(col) == 61 * 60


def test_neighbours_order_ties_and_self():
    """eight identical rows: the seven duplicates of a point are its nearest neighbours at distance 0 in index order, the point
    itself is not among them; against a brute-force sort of (value, index) pairs"""
    X, _ = nn.blobs(97, 40, 4, 3)
    X[5] += 40.0
    X[20:28] = X[20]
    idx, d2 = nn.neighbours(X, 16)
    assert list(idx[22, :7]) == [20, 21, 23, 24, 25, 26, 27] and np.all(d2[22, :7] == 0) and d2[22, 7] > 0
    D = nn.distances(X)
    for i in (0, 5, 22, 96):
        want = sorted((D[i, j], j) for j in range(97) if j != i)[:16]
        assert [j for _, j in want] == list(idx[i]) and [v for v, _ in want] == list(d2[i])
    assert np.all(idx != np.arange(97)[:, None]) and np.all(np.diff(d2, axis=1) >= 0)


def test_invariants_in_both_precisions(case300):
    c = case300
    for dtype in (np.float64, np.float32):
        a = nn.affinities(c["X"], c["perp"], dtype)
        P = a["P"]
        assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0) and np.all(np.isfinite(P)) and np.all(P >= 0)
        assert abs(P.astype(np.float64).sum() - 1.0) <= (1e-13 if dtype is np.float64 else 1e-5)
        assert np.abs(a["cond"].astype(np.float64).sum(axis=1) - 1.0).max() <= (1e-13 if dtype is np.float64 else 1e-5)
        perp = nn.row_perplexity(a["d2"], a["beta"])
        assert np.abs(perp - c["perp"]).max() <= (1e-9 if dtype is np.float64 else 1e-2) * c["perp"]
        rp, col, val = nn.joint_csr(a["idx"], a["cond"], dtype)
        assert np.array_equal(nn.densify(rp, col, val, dtype), P)
        assert np.all(np.diff(rp) >= a["k"])                       # every row keeps at least its own neighbours
        for i in (0, 150, 299):
            assert np.all(np.diff(col[rp[i]:rp[i + 1]]) > 0) and i not in col[rp[i]:rp[i + 1]]


def test_duplicates_cannot_reach_the_target():
    """a duplicate row has seven neighbours at distance zero and cannot go below perplexity 7: the search doubles to its end"""
    X, _ = nn.blobs(97, 40, 4, 3)
    X[5] += 40.0
    X[20:28] = X[20]
    for dtype in (np.float64, np.float32):
        a = nn.affinities(X, 5.0, dtype)
        assert a["k"] == 16 and np.all(np.isfinite(a["P"])) and np.all(a["beta"][20:28] == 2.0 ** nn.SEARCH_STEPS)
        assert np.allclose(nn.row_perplexity(a["d2"], a["beta"])[20:28], 7.0)
        assert np.allclose(a["cond"][20, :7], 1.0 / 7.0) and np.all(a["cond"][20, 7:] == 0)


def test_whole_run_on_the_sparse_joint_separates_the_blobs(case300):
    c = case300
    Y0 = np.random.RandomState(0).randn(300, 2) * 1e-4
    kl0 = nn.forces(c["P"], Y0)[2]
    Y, kl = nn.run(c["P"], Y0, 500, 125)
    print("sparse-P run: KL %.4f from %.4f" % (kl, kl0))           # 0.79 here; the descent is chaotic, the digits vary by machine
    assert np.all(np.isfinite(Y)) and kl < 0.5 * kl0
    assert nn.neighbour_purity(Y, c["labels"], 10) == 1.0
