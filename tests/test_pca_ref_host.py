"""CPU-only: tests/pca_ref.py -- the float64 restatement the PCA kernels are held to (tests/test_gpu_pca.py) -- against
sklearn.decomposition.PCA(svd_solver='full') where scikit-learn is installed, and the two conditions of its input generator that
the GPU tests lean on everywhere.  scikit-learn's own t-SNE takes its PCA with svd_solver='randomized'; this project holds to
'full', the exact decomposition the randomized one approximates."""
import numpy as np
import pytest

import pca_ref as ref


@pytest.fixture(scope="module", params=ref.PLANTED, ids=lambda s: "n%d_d%d_r%g" % s[:3])
def case(request):
    n, d, ratio, seed = request.param
    X = ref.planted(n, d, ratio, seed)
    mean, evals, comps = ref.fit(X)
    return dict(n=n, d=d, ratio=ratio, X=X, mean=mean, evals=evals, comps=comps)


def test_generator_keeps_its_gaps_and_sign_margins(case):
    """what the GPU tests assume of planted(): neighbouring eigenvalues apart by the planted ratio (so every component is
    determined) and no component whose two largest entries nearly tie (so the sign rule is determined).  Measured: the smallest
    ratio equals `ratio` to four digits, the smallest margin is 2.1e-5 (n = 513, d = 256)."""
    got = ref.min_neighbour_ratio(case["evals"])
    margin = ref.sign_margins(case["comps"]).min()
    print("n=%d d=%d: min ratio %.6f (planted %g), min sign margin %.3g" % (case["n"], case["d"], got, case["ratio"], margin))
    assert got >= 0.999 * case["ratio"]
    assert margin >= 1e-6
    j = np.arange(case["d"])
    assert np.allclose(case["evals"], case["ratio"] ** -j.astype(np.float64), rtol=1e-4)


def test_fit_matches_scikit_learn_full(case):
    decomposition = pytest.importorskip("sklearn.decomposition")
    pca = decomposition.PCA(svd_solver='full').fit(case["X"].astype(np.float64))
    k = len(pca.explained_variance_)
    e_val = np.abs(pca.explained_variance_ - case["evals"][:k]).max() / case["evals"][0]
    e_mean = np.abs(pca.mean_ - case["mean"]).max()
    e_comp = np.abs(pca.components_ - case["comps"][:k]).max()
    print("n=%d d=%d vs PCA(full): eigenvalues %.3g of the largest, mean %.3g, components %.3g"
          % (case["n"], case["d"], e_val, e_mean, e_comp))
    assert e_val <= 1e-12 and e_mean <= 1e-12 and e_comp <= 1e-12
    total = case["evals"].sum()
    assert np.abs(pca.explained_variance_ratio_ - case["evals"][:k] / total).max() <= 1e-12
    assert np.abs(pca.singular_values_ - np.sqrt(case["evals"][:k] * (case["n"] - 1))).max() <= 1e-12 * pca.singular_values_[0]
    Y = pca.transform(case["X"].astype(np.float64))
    assert np.abs(Y - ref.project(case["X"], case["mean"], case["comps"][:k])).max() <= 1e-12 * np.abs(Y).max()


def test_covariance_route_agrees_within_its_own_allowance(case):
    """eigh(moments(X)) -- what the eigen-solver tests on the GPU compare with -- against fit(X): eigenvalues to
    32 d eps lambda_max, component i to that over gap_i (Davis-Kahan), the bound those tests use."""
    d = case["d"]
    evals, comps = ref.eigh(ref.moments(case["X"])[1])
    tol = 32 * d * ref.EPS * case["evals"][0]
    e_val = np.abs(evals - case["evals"]).max()
    e_comp = (np.abs(comps - case["comps"]).max(axis=1) * ref.gaps(case["evals"])).max()
    print("n=%d d=%d eigh(cov) vs svd: eigenvalues %.3g, components x gap %.3g, allowance %.3g" % (case["n"], d, e_val, e_comp, tol))
    assert e_val <= tol and e_comp <= tol


def test_tsne_initial_state_is_scikit_learns_formula(case):
    """TSNE._fit with init='pca': PCA(2) scores, rounded to float32, / np.std(first column) * 1e-4 -- with 'full' in the place of
    its 'randomized'.  Without the rounding the two agree to float64; with it to one float32 rounding."""
    decomposition = pytest.importorskip("sklearn.decomposition")
    if case["d"] < 2:
        pytest.skip("two components need two features")
    X = case["X"].astype(np.float64)
    scores = decomposition.PCA(n_components=2, svd_solver='full').fit_transform(X)
    mine = ref.tsne_initial(case["X"])
    exact = scores / np.std(scores[:, 0]) * 1e-4
    assert np.abs(exact - mine).max() <= 1e-12 * 1e-4
    rounded = scores.astype(np.float32, copy=False)
    rounded = rounded / np.std(rounded[:, 0]) * 1e-4
    assert np.abs(rounded - mine).max() <= 2.0 ** -22 * np.abs(mine).max()
    assert abs(np.std(mine[:, 0]) - 1e-4) <= 1e-12 * 1e-4


def test_sign_rule_and_order_by_hand():
    comps = np.array([[0.5, -0.5, 0.1], [-0.2, 0.1, -0.9], [0.3, 0.3, -0.3]])
    got = ref.sign_rule(comps)
    assert np.array_equal(got[0], comps[0]) and np.array_equal(got[1], -comps[1]) and np.array_equal(got[2], comps[2])
    evals, vecs = ref.eigh(np.diag([1.0, 3.0, 2.0, 3.0]))
    assert np.array_equal(evals, [3.0, 3.0, 2.0, 1.0])
    assert np.array_equal(np.abs(vecs[2]), [0, 0, 1, 0]) and np.array_equal(np.abs(vecs[3]), [1, 0, 0, 0])
    assert np.array_equal(ref.gaps([4.0, 3.0, 1.0]), [1.0, 1.0, 2.0])
