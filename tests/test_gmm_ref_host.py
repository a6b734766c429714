"""CPU-only: tests/gmm_ref.py -- the float64 restatement the mixture kernels are held to (tests/test_gpu_gmm.py) -- against
scikit-learn where it is installed, the preconditions of the shared case table that the GPU tests lean on, and the refusals of
evae.mixture.GaussianMixture that are known from arguments and shapes alone.

The preconditions are conditions, not measurements: a GPU test may compare n_iter_, converged_ and labels EXACTLY only because
the reference itself stays clear of the stop's threshold (| |change| - tol | >= 1e-8, where fp64 rounding of a mean of at most
2 049 log-densities is about 1e-13) and of arg-max ties (margin >= 1e-9)."""
import warnings

import numpy as np
import pytest

import gmm_ref as ref

ROWS = pytest.mark.parametrize("row", ref.CASES, ids=ref.case_id)


@ROWS
def test_case_table_stays_clear_of_thresholds(row):
    f = ref.solved(*row)["fit"]
    print("%s: %d iterations, stop margin %.3g, arg-max margin %.3g, smallest n_k %.3g, factor condition %.3g"
          % (ref.case_id(row), f["n_iter"], f["tol_margin"], f["argmax_margin"], f["min_nk"], f["cond"]))
    assert f["tol_margin"] >= 1e-8
    assert f["argmax_margin"] >= 1e-9
    assert f["min_nk"] >= 1.0
    assert f["converged"] and f["n_iter"] < ref.MAX_ITER
    assert f["cond"] <= ref.MAX_COND                         # the Cholesky-and-inverse bound of the GPU test carries it


def test_table_covers_the_edges():
    ns, ds, ks = {r[0] for r in ref.CASES}, {r[1] for r in ref.CASES if r[3] == 'full'}, {r[2] for r in ref.CASES}
    assert {ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1, 2 * ref.CHUNK + 1} <= ns and min(ns) < ref.STRIP
    assert {1, 2, 15, 16, 17, 40, 96} <= ds
    assert 256 in {r[1] for r in ref.CASES if r[3] == 'diag'}
    assert {1, 2, 10, 33, 256} <= ks
    assert {r[3] for r in ref.CASES} == {'full', 'diag', 'spherical'}
    assert max(r[0] * r[1] * r[2] for r in ref.CASES) <= 2100 * 40 * 33
    assert sum(ref.solved(*r)["fit"]["n_iter"] >= 8 for r in ref.CASES) >= 3


def test_the_library_uses_the_table_s_chunk_and_strip():
    from evae import ops
    assert (ops.gmm_chunk_rows(), ops.gmm_strip_rows()) == (ref.CHUNK, ref.STRIP)
    assert (ops.gmm_max_components(), ops.gmm_max_points(), ops.gmm_max_bytes()) == (256, 2 ** 20, 2 ** 30)
    assert (ops.gmm_max_features('full'), ops.gmm_max_features('diag'), ops.gmm_max_features('spherical')) == (96, 256, 256)


# ---------------------------------------------------------------------------------------------- against scikit-learn
@ROWS
def test_fit_matches_scikit_learn(row):
    """Same means_init / weights_init / precisions_init, same tol: n_iter_ and converged_ equal, parameters and lower_bound_
    within 10 x the largest difference observed over the table (ref.SPREAD), each relative to the largest magnitude of the
    quantity.  The two are float64 implementations that differ in summation order (BLAS against numpy) and, for 'diag', in the
    covariance formula (scikit-learn's E[x^2] - 2 mu E[x] + mu^2 against the two-pass form).  Largest observed, scikit-learn
    1.7.2: weights 9.7e-15, means 8.3e-15, covariances 3.2e-14 (all three at n2049_d40_K33_diag), precisions_cholesky 2.9e-14
    (n2049_d40_K10_full), lower_bound 3.5e-16 (n40_d1_K2_full)."""
    mixture = pytest.importorskip("sklearn.mixture")
    n, d, K, ctype, seed = row
    s = ref.solved(*row)
    f = s["fit"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = mixture.GaussianMixture(K, covariance_type=ctype, tol=ref.TOL, reg_covar=ref.REG, max_iter=ref.MAX_ITER,
                                    weights_init=s["w"], means_init=s["mu"], precisions_init=s["prec"])
        g.fit(np.asarray(s["X"], np.float64))
    assert g.n_iter_ == f["n_iter"] and bool(g.converged_) == f["converged"]
    got = dict(weights=g.weights_, means=g.means_, covariances=g.covariances_, P=g.precisions_cholesky_,
               lower_bound=g.lower_bound_)
    errs = {key: ref.rel_err(got[key], f[key]) for key in got}
    print(ref.case_id(row), " ".join("%s %.3g" % kv for kv in sorted(errs.items())))
    for key, e in errs.items():
        assert e <= 10.0 * ref.SPREAD[key], key


@pytest.mark.parametrize("row", ref.RANDOM_ROWS, ids=ref.case_id)
def test_fit_from_random_responsibilities_matches_scikit_learn(row):
    """The fits from uniform responsibilities that the GPU test makes, against scikit-learn started from the reference's own
    initial M-step.  Largest observed (all at n1024_d16_K10_full, 38 iterations): weights 9.9e-13, means 1.6e-12, covariances
    1.5e-12, precisions_cholesky 5.7e-12, lower_bound 8.9e-16; asserted at 10 x (ref.SPREAD_RANDOM)."""
    mixture = pytest.importorskip("sklearn.mixture")
    n, d, K, ctype, seed = row
    X = np.asarray(ref.solved(*row)["X"], np.float64)
    resp, f = ref.solved_from_random(*row)
    nk, mu, cov = ref.mstep(X, resp, ref.REG, ctype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = mixture.GaussianMixture(K, covariance_type=ctype, tol=ref.TOL, reg_covar=ref.REG, max_iter=300, weights_init=nk / nk.sum(),
                                    means_init=mu, precisions_init=np.linalg.inv(cov) if ctype == 'full' else 1.0 / cov).fit(X)
    assert g.n_iter_ == f["n_iter"] and bool(g.converged_) == f["converged"] and f["converged"]
    assert f["tol_margin"] >= 1e-8 and f["argmax_margin"] >= 1e-9 and f["min_nk"] >= 1.0
    got = dict(weights=g.weights_, means=g.means_, covariances=g.covariances_, P=g.precisions_cholesky_, lower_bound=g.lower_bound_)
    errs = {key: ref.rel_err(got[key], f[key]) for key in got}
    print(ref.case_id(row), " ".join("%s %.3g" % kv for kv in sorted(errs.items())))
    for key, e in errs.items():
        assert e <= 10.0 * ref.SPREAD_RANDOM[key], key


def test_init_from_responsibilities_matches_scikit_learn():
    """fit_from_resp against scikit-learn's own initial M-step (init_params='random' with its responsibilities reproduced)"""
    mixture = pytest.importorskip("sklearn.mixture")
    row = ref.CASES[0]
    n, d, K, ctype, seed = row
    X = np.asarray(ref.solved(*row)["X"], np.float64)
    resp = np.random.RandomState(3).uniform(size=(n, K))     # what check_random_state(3) draws first in _initialize_parameters
    resp /= resp.sum(axis=1)[:, np.newaxis]
    f = ref.fit_from_resp(X, resp, ctype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g = mixture.GaussianMixture(K, covariance_type=ctype, tol=ref.TOL, reg_covar=ref.REG, max_iter=ref.MAX_ITER,
                                    init_params='random', random_state=3).fit(X)
    assert g.n_iter_ == f["n_iter"]
    assert ref.rel_err(g.means_, f["means"]) <= 10.0 * ref.SPREAD["means"]
    assert ref.rel_err(g.lower_bound_, f["lower_bound"]) <= 10.0 * ref.SPREAD["lower_bound"]


def test_densities_and_sampling_match_scikit_learn():
    mixture = pytest.importorskip("sklearn.mixture")
    row = ref.CASES[1]
    n, d, K, ctype, seed = row
    s = ref.solved(*row)
    f = s["fit"]
    g = mixture.GaussianMixture(K, covariance_type=ctype)
    g.weights_, g.means_, g.covariances_, g.precisions_cholesky_ = f["weights"], f["means"], f["covariances"], f["P"]
    X = np.asarray(s["X"], np.float64)
    assert np.abs(g.score_samples(X) - f["logp"]).max() <= 1e-11
    assert np.abs(g.predict_proba(X) - np.exp(f["log_resp"])).max() <= 1e-12
    assert np.array_equal(g.predict(X), f["labels"])
    lb = float(f["logp"].mean())
    assert abs(g.bic(X) - (-2.0 * lb * n + ref.n_parameters(K, d, ctype) * np.log(n))) <= 1e-8
    # z = mu + L eps with L the lower Cholesky factor of the covariance equals the reference's forward substitution
    rs = np.random.RandomState(0)
    comp, eps = rs.randint(0, K, 50), rs.standard_normal((50, d))
    want = f["means"][comp] + np.einsum('nij,nj->ni', np.linalg.cholesky(f["covariances"])[comp], eps)
    assert np.abs(ref.sample(f["means"], f["P"], ctype, comp, eps) - want).max() <= 1e-11


@pytest.mark.parametrize("ctype,K,d,want", [('full', 3, 4, 3 * 10 + 12 + 2), ('diag', 3, 4, 12 + 12 + 2), ('spherical', 3, 4, 3 + 12 + 2),
                                            ('full', 1, 1, 2), ('diag', 10, 40, 809), ('full', 10, 40, 8200 + 400 + 9)])
def test_parameter_counts(ctype, K, d, want):
    from evae.mixture import n_parameters
    assert n_parameters(K, d, ctype) == want == ref.n_parameters(K, d, ctype)
    mixture = pytest.importorskip("sklearn.mixture")
    g = mixture.GaussianMixture(K, covariance_type=ctype)
    g.means_ = np.zeros((K, d))
    assert g._n_parameters() == want


# ---------------------------------------------------------------------------------------------- refusals known without a GPU
def test_gaussian_mixture_refuses_from_arguments_and_shapes_alone():
    from evae import _lib, ops
    from evae.mixture import GaussianMixture
    with _lib.count_calls("evae_gmm_step") as steps, _lib.count_calls("evae_gmm_mstep") as msteps:
        with pytest.raises(ValueError, match="tied"):
            GaussianMixture(2, covariance_type='tied')
        for bad in (dict(n_components=0), dict(n_components=257), dict(covariance_type='banded'), dict(init_params='k-means++'),
                    dict(max_iter=0), dict(n_init=0), dict(check_every=0), dict(tol=-1.0), dict(reg_covar=-1e-6),
                    dict(n_components=2, weights_init=np.ones(3) / 3), dict(n_components=2, weights_init=np.array([0.9, 0.9])),
                    dict(n_components=2, means_init=np.zeros((3, 2))), dict(n_components=2, precisions_init=np.ones((2, 2))),
                    dict(n_components=2, covariance_type='diag', precisions_init=np.ones(2)),
                    dict(n_components=2, covariance_type='spherical', precisions_init=np.ones((2, 2)))):
            with pytest.raises(ValueError):
                GaussianMixture(**bad)
        with pytest.raises(ValueError):
            GaussianMixture(3).fit(np.zeros((2, 2), np.float32))                               # K > N
        with pytest.raises(ValueError):
            GaussianMixture(1).fit(np.zeros((1, 2), np.float32))                               # N < 2
        with pytest.raises(ValueError):
            GaussianMixture(2).fit(np.zeros(8, np.float32))                                    # not [N x d]
        with pytest.raises(ValueError, match="pca"):
            GaussianMixture(2).fit(np.zeros((300, 97), np.float32))                            # 'full' above 96 features
        with pytest.raises(ValueError):
            GaussianMixture(2, covariance_type='diag').fit(np.zeros((300, 257), np.float32))
        with pytest.raises(ValueError):
            GaussianMixture(2, means_init=np.zeros((2, 3))).fit(np.zeros((8, 2), np.float32))  # init of another width
        with pytest.raises(ValueError):
            GaussianMixture(2, precisions_init=np.ones((2, 3, 3))).fit(np.zeros((8, 2), np.float32))
        with pytest.raises(ValueError, match="bytes"):                                         # responsibilities + workspace > 1 GiB
            GaussianMixture(256).fit(torch_empty_rows(2 ** 20, 2))
    assert not steps and not msteps
    with pytest.raises(_lib.EvaeError, match="bytes"):
        ops.gmm_check_sizes(2 ** 20, 96, 256, 'full', "test")
    with pytest.raises(_lib.EvaeError):
        GaussianMixture(2).predict(np.zeros((4, 2), np.float32))                               # not fitted


def torch_empty_rows(n, d):
    import torch
    return torch.empty((n, d), dtype=torch.float32)
