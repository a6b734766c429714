"""CPU-only: tests/tsne_ref.py -- the float64 restatement the t-SNE kernels are held to (tests/test_gpu_tsne.py) -- against
scikit-learn's private routines where it is installed, against its own invariants and a hand-worked update step everywhere."""
import numpy as np
import pytest

import tsne_ref as ref

SHAPES = [(97, 40, 5.0), (200, 40, 30.0), (257, 3, 30.0)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "N%d_zd%d_perp%g" % s)
def case(request):
    n, zd, perp = request.param
    X, _ = ref.blobs(n, zd, 4, seed=1000 + n)
    P, beta, D = ref.affinities(X, perp)
    return dict(n=n, zd=zd, perp=perp, X=X, P=P, beta=beta, D=D)


def test_joint_probabilities_match_scikit_learn(case):
    """scikit-learn stops its search at an entropy error of 1e-5; measured agreement 3.1e-6 .. 7.0e-6 of max(P)"""
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    Ps = squareform(tsne._joint_probabilities(case["D"].astype(np.float32), case["perp"], 0))
    err = np.abs(Ps - case["P"]).max() / case["P"].max()
    print("joint P vs scikit-learn: %.3g of max(P)" % err)
    assert err <= 2e-5


@pytest.mark.parametrize("scale", [1e-4, 1.0, 30.0])
def test_kl_and_gradient_match_scikit_learn(case, scale):
    tsne = pytest.importorskip("sklearn.manifold._t_sne")
    from scipy.spatial.distance import squareform
    n = case["n"]
    Y = np.random.RandomState(7).randn(n, 2) * scale
    for exag in (1.0, 12.0):
        grad, Z, _, _, _ = ref.forces(case["P"], Y, exag)
        kl = ref.forces(case["P"] * exag, Y, 1.0)[2]                      # scikit-learn's KL takes the exaggerated P
        Pc = squareform(case["P"] * exag, checks=False)
        kl_s, grad_s = tsne._kl_divergence(Y.ravel().copy(), Pc, 1.0, n, 2)
        gerr = np.abs(grad_s.reshape(n, 2) - grad).max() / np.abs(grad).max()
        print("scale %g exag %g: KL %.12g vs %.12g, gradient %.3g of its largest entry" % (scale, exag, kl, kl_s, gerr))
        assert abs(kl - kl_s) <= 1e-12
        assert gerr <= 1e-12


def test_joint_probabilities_invariants(case):
    P, n = case["P"], case["n"]
    assert np.array_equal(P, P.T) and np.all(np.diag(P) == 0) and np.all(np.isfinite(P)) and np.all(P >= 0)
    assert abs(P.sum() - 1.0) <= 1e-13
    C = ref.conditional_rows(case["D"], case["beta"])
    assert np.abs(C.sum(axis=1) - 1.0).max() <= 1e-13 and np.all(np.diag(C) == 0)
    assert np.abs(P.sum(axis=1) - (1.0 + C.sum(axis=0)) / (2 * n)).max() <= 1e-15
    assert np.abs(ref.row_perplexity(case["D"], case["beta"]) - case["perp"]).max() <= 1e-9 * case["perp"]


def test_outlier_and_duplicate_rows_stay_finite():
    """a far row (its distances differ only in their low digits) and eight identical rows (d = 0; seven duplicates cannot be
    spread over a perplexity of 5: the search doubles to its end, 2^steps, and the row is uniform over its duplicates)"""
    X, _ = ref.blobs(97, 40, 4, seed=3)
    X[5] += 40.0
    X[20:28] = X[20]
    reach = None
    for dtype in (np.float64, np.float32):
        P, beta, D = ref.affinities(X, 5.0, dtype)
        assert np.all(np.isfinite(P)) and np.all(np.isfinite(beta)) and np.array_equal(P, P.T)
        assert np.all(beta[20:28] == 2.0 ** ref.SEARCH_STEPS)
        C = ref.conditional_rows(D, beta, dtype)
        assert np.allclose(C[20, 21:28], 1.0 / 7.0) and C[20, :20].max() == 0
        perp = ref.row_perplexity(D.astype(np.float64), beta)
        assert np.allclose(perp[20:28], 7.0)
        if reach is None:
            # a row whose NEAREST neighbours are the eight identical rows cannot go below perplexity 8 either; every other row
            # reaches the target
            reach = np.abs(perp - 5.0) <= 1e-9
            assert reach[5] and reach.sum() >= 80 and np.all(perp[~reach] >= 7.0 - 1e-9)
        assert np.abs(perp[reach] - 5.0).max() <= (1e-9 if dtype is np.float64 else 1e-2)


def test_update_step_hand_worked():
    """three points, momentum 0.5, lr 10; by hand:
    point 0: grad ( 0.01,  0.02) vel ( 0.1, -0.1) gains (1, 1):      x agrees -> 0.8, vel 0.05 - 0.08 = -0.03; y disagrees -> 1.2, vel -0.05 - 0.24 = -0.29
    point 1: grad (-0.01,  0   ) vel ( 0,    0.2) gains (0.012, 1):  x product 0 -> x0.8 = 0.0096 -> floor 0.01, vel 0.001; y -> 0.8, vel 0.1
    point 2: grad ( 0.03, -0.02) vel (-0.3,  0  ) gains (1, 0.0124): x disagrees -> 1.2, vel -0.15 - 0.36 = -0.51; y -> 0.00992 -> 0.01, vel 0.002"""
    Y = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0]])
    grad = np.array([[0.01, 0.02], [-0.01, 0.0], [0.03, -0.02]])
    vel = np.array([[0.1, -0.1], [0.0, 0.2], [-0.3, 0.0]])
    gains = np.array([[1.0, 1.0], [0.012, 1.0], [1.0, 0.0124]])
    Y1, v1, g1 = ref.update(Y, vel, gains, grad, 0.5, 10.0)
    assert np.allclose(g1, [[0.8, 1.2], [0.01, 0.8], [1.2, 0.01]], rtol=0, atol=1e-15)
    assert np.allclose(v1, [[-0.03, -0.29], [0.001, 0.1], [-0.51, 0.002]], rtol=0, atol=1e-15)
    moved = np.array([[-0.03, -0.29], [1.001, 0.1], [-0.51, 2.002]])
    assert np.allclose(Y1, moved - [0.461 / 3, 1.812 / 3], rtol=0, atol=1e-15)
    assert np.abs(Y1.mean(axis=0)).max() <= 1e-16


def test_whole_run_separates_blobs_and_lowers_kl():
    X, labels = ref.blobs(120, 10, 3, seed=5, shift=8.0)
    P = ref.affinities(X, 15.0)[0]
    Y0 = np.random.RandomState(0).randn(120, 2) * 1e-4
    kl0 = ref.forces(P, Y0)[2]
    Y, kl = ref.run(P, Y0, 200, 50)
    assert np.all(np.isfinite(Y)) and kl < 0.5 * kl0
    assert ref.neighbour_purity(Y, labels, 10) >= 0.9
