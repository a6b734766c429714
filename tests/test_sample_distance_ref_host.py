"""CPU-only: the longdouble restatement tests/sample_distance_ref.py (the yardstick of tests/test_gpu_sample_distance.py) held
to independent evaluations -- plain float64 numpy always, scikit-learn's pairwise kernels and scipy.linalg.sqrtm where they
import -- within the bounds the device is held to and on the inputs used there; to closed forms; and the bounds to their caps:
no bound of a row sum or a total may exceed 1e-9 of the value at any parity shape, where a pair left out or counted twice moves
a total by at least 1 / (B N) >= 1e-6 of it (the terms lie in (0.19, 1.81) for KID's kernel, in (e^-3.24, 1] for the RBF one)."""
import numpy as np
import pytest

import sample_distance_ref as ref

KINDS = [dict(kind='poly', gamma=None, coef0=1.0, degree=3), dict(kind='rbf', gamma=None)]
IDS = ['poly', 'rbf']


def shapes(skip_self):
    """(B, N, d) of the parity tests; the within-set form takes the queries as its columns"""
    return [(B, B if skip_self else N, d) for B, N, d in ref.parity_shapes()]


def f64_rows(q, c, kind, gamma=None, coef0=1.0, degree=3, skip_self=False):
    """the second evaluation: float64 numpy, BLAS for the dot products, numpy's pairwise sum"""
    q, c = q.astype(np.float64), c.astype(np.float64)
    g = 1.0 / q.shape[1] if gamma is None else gamma
    if kind == 'poly':
        K = (g * (q @ c.T) + coef0) ** degree
    else:
        K = np.exp(-g * ((q[:, None, :] - c[None, :, :]) ** 2).sum(axis=-1))
    if skip_self:
        np.fill_diagonal(K, 0.0)
    return K.sum(axis=1)


@pytest.mark.parametrize("skip_self", [False, True], ids=['all', 'skip_self'])
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_bounds_are_capped_and_admit_float64(kw, skip_self):
    for B, N, d in shapes(skip_self):
        q, c = ref.rows_case(B, N, d)
        c = q if skip_self else c
        rs, tot = ref.row_sums(q, c, skip_self=skip_self, **kw), ref.total(q, c, skip_self=skip_self, **kw)
        rb, tb = ref.error_bounds_rows(q, c, skip_self=skip_self, **kw)
        if N == 1 and skip_self:
            assert rs[0] == 0.0 and rb[0] == 0.0 and tot == 0.0                 # nothing is left of a single row
            continue
        assert (rs > 0).all() and (rb <= 1e-9 * rs).all() and tb <= 1e-9 * tot, (B, N, d)
        assert (rb >= 2.0 ** -53 * rs).all()                                    # and it is a bound, not zero
        got = f64_rows(q, c, skip_self=skip_self, **kw)
        assert (np.abs(got - rs) <= rb).all() and abs(got.sum() - tot) <= tb, (B, N, d)


@pytest.mark.parametrize("skip_self", [False, True], ids=['all', 'skip_self'])
def test_restatement_against_scikit_learn(skip_self):
    pairwise = pytest.importorskip("sklearn.metrics.pairwise")
    for B, N, d in shapes(skip_self):
        q, c = ref.rows_case(B, N, d)
        c = q if skip_self else c
        q64, c64 = q.astype(np.float64), c.astype(np.float64)
        for kw, K in ((KINDS[0], pairwise.polynomial_kernel(q64, c64, degree=3, gamma=None, coef0=1)),
                      (KINDS[1], pairwise.rbf_kernel(q64, c64, gamma=None))):
            if skip_self:
                np.fill_diagonal(K, 0.0)
            rb, tb = ref.error_bounds_rows(q, c, skip_self=skip_self, **kw)
            assert (np.abs(K.sum(axis=1) - ref.row_sums(q, c, skip_self=skip_self, **kw)) <= rb).all(), (B, N, d, kw['kind'])
            assert abs(K.sum() - ref.total(q, c, skip_self=skip_self, **kw)) <= tb


def test_skip_self_goes_by_index_in_the_restatement():
    q = np.array([[1.0, 2.0], [1.0, 2.0], [0.5, -1.0]], np.float32)             # rows 0 and 1 are equal
    full, skip = ref.row_sums(q, q, **KINDS[0]), ref.row_sums(q, q, skip_self=True, **KINDS[0])
    diag = [(1.0 / 2 * float(r @ r) + 1.0) ** 3 for r in q.astype(np.float64)]
    assert np.allclose(full - skip, diag, rtol=1e-15)
    assert skip[0] == skip[1] and skip[0] > diag[0]                             # the duplicate at j != i is still counted


@pytest.mark.parametrize("name", sorted(ref.SETS))
def test_frechet_restatement_against_float64_and_sqrtm(name):
    c = ref.distance_case(name)
    fr, fb = c['frechet'], c['fb']
    r64, f64 = c['real'].astype(np.float64), c['fake'].astype(np.float64)
    mu_r, mu_f = r64.mean(axis=0), f64.mean(axis=0)
    cov_r, cov_f = np.cov(r64, rowvar=False), np.cov(f64, rowvar=False)
    mean_term = float(((mu_r - mu_f) ** 2).sum())
    assert abs(mean_term - fr['mean_term']) <= fb['mean_term']
    lam, V = np.linalg.eigh(cov_r)
    A = np.sqrt(np.maximum(lam, 0.0))[:, None] * V.T
    tr_sqrt = float(np.sqrt(np.maximum(np.linalg.eigvalsh(A @ cov_f @ A.T), 0.0)).sum())
    trace_term = float(np.trace(cov_r) + np.trace(cov_f) - 2.0 * tr_sqrt)
    print("%s: float64 numpy used %.3g of tr_sqrt's bound %.3g (E = %.3g, nu_min = %.3g, %d small)"
          % (name, abs(tr_sqrt - fr['tr_sqrt']) / fb['tr_sqrt'], fb['tr_sqrt'], fb['e_total'], fb['nu_min'], fb['small']))
    assert abs(tr_sqrt - fr['tr_sqrt']) <= fb['tr_sqrt']
    assert abs(trace_term - fr['trace_term']) <= fb['trace_term']
    assert abs(mean_term + trace_term - fr['frechet_distance']) <= fb['frechet_distance']
    if name != 'rank':                                     # a full-rank pair: every eigenvalue stands clear of the perturbation
        assert fb['small'] == 0 and fb['frechet_distance'] <= 1e-6 * (fr['tr_r'] + fr['tr_f'])
    linalg = pytest.importorskip("scipy.linalg")
    if name == 'rank':
        return                                                                   # sqrtm of a singular product: not a yardstick
    root = linalg.sqrtm(cov_r @ cov_f)
    assert abs(float(np.trace(root).real) - fr['tr_sqrt']) <= max(fb['tr_sqrt'], 1e-11 * fr['tr_sqrt'])    # (sqrtm's own: Schur)


def test_frechet_closed_form_for_diagonal_covariances():
    rs = np.random.RandomState(5)
    a, b = rs.uniform(0.5, 2.0, 9), rs.uniform(0.5, 2.0, 9)
    mu_r, mu_f = rs.randn(9), rs.randn(9)
    fr = ref.frechet_of_moments(mu_r, np.diag(a), mu_f, np.diag(b))
    want = ((mu_r - mu_f) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(fr['frechet_distance'] - want) <= 1e-14 * (a.sum() + b.sum())
    assert abs(fr['tr_sqrt'] - np.sqrt(a * b).sum()) <= 1e-14 * a.sum()
    assert np.allclose(np.sort(fr['nu']), np.sort(a * b), rtol=1e-13)


def test_identical_sets():
    real, _ = ref.gaussian_sets(N=60, M=60, d=6, seed=3)
    fr = ref.frechet(real, real)
    assert fr['frechet_distance'] == 0.0 and fr['mean_term'] == 0.0 and fr['trace_term'] == 0.0
    for kw in KINDS:
        assert ref.kernel_mmd(real, real, biased=True, **kw)['mmd2'] == 0.0
    # the unbiased estimate is not a square: its within-set means lack the diagonal, the largest terms of the rbf kernel
    unbiased = ref.kernel_mmd(real, real, **KINDS[1])
    assert unbiased['mmd2'] < 0.0 and unbiased['k_rr'] < unbiased['k_rf']


def test_biased_and_unbiased_differ_by_the_diagonal():
    c = ref.distance_case('small')
    b, u = ref.mmd_case('small', biased=True), ref.mmd_case('small')
    for s, x in (('s_rr', c['real']), ('s_ff', c['fake'])):
        diag = ref.diagonal_sum(x)
        assert abs((b[s] - u[s]) - diag) <= 1e-15 * b[s]
    assert b['s_rf'] == u['s_rf']


def test_mmd_bounds_are_capped():
    for name in sorted(ref.SETS):
        for kw in KINDS:
            m = ref.mmd_case(name, kw['kind'])
            for s, tb in zip(('s_rr', 's_ff', 's_rf'), m['bounds']):
                assert 0 < tb <= 1e-9 * abs(m[s]), (name, kw['kind'], s)


def test_median_gamma_is_the_lower_median_of_the_other_rows():
    x = np.array([[0.0], [1.0], [3.0]], np.float32)                              # squared distances 1, 4, 9, each twice
    assert ref.median_gamma(x) == 1.0 / 4.0
    x = np.array([[0.0], [1.0]], np.float32)
    assert ref.median_gamma(x) == 1.0
