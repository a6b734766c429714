"""GPU: the fp64 Gaussian-mixture kernels (csrc/evae_gmm.hip), evae.ops.gmm_*, evae.mixture.GaussianMixture and the latent-space
report, against the numpy float64 restatement tests/gmm_ref.py (held to scikit-learn, and its case table to its margins, by
tests/test_gmm_ref_host.py).

The yardstick is always the restatement, never the code under test.  Decisions -- n_iter_, converged_, labels -- are compared
EXACTLY: the restatement's own margins (>= 1e-8 for the stop, >= 1e-9 for an arg-max; asserted on the host for the table, here
for inputs made here) are far above fp64 rounding.  Fitted parameters and lower_bound_ are held to 10 x the spread recorded
between the restatement and scikit-learn (ref.SPREAD), relative to the largest magnitude of the quantity.  Single steps from
given inputs are held to bounds from the arithmetic, eps = 2^-52, both sides' rounding allowed (hence the leading 2):

* E-step.  a_j = sum_i |x_i| |P[i,j]| + sum_i |mu_i| |P[i,j]| bounds every partial sum of y_j; y_j takes j + 1 fused steps and a
  subtraction (b_j itself j + 1 steps): |dy_j| <= (d + 2) eps a_j.  With A = sum_j a_j^2, m = sum y_j^2 carries
  sum 2 |y_j| |dy_j| + (d + 1) eps sum y_j^2 <= (3 d + 5) eps A.  log N + log pi adds four roundings of terms of size d log(2 pi)
  / 2, A / 2, Ld = sum_j |log P[j,j]| (d additions and logarithms: (d + 4) eps Ld) and |log pi|.  Per side
  E_ik = (1.5 d + 4.5) eps A_ik + 4 eps (d log(2 pi) / 2 + |log pi_k|) + (d + 4) eps Ld_k.
  log p(x_i): the maximum is exact, every exponent moves by <= E, K additions, one exp and one log each:
  2 max_k E_ik + 2 (K + 4) eps (1 + |log p(x_i)|).  log_resp adds E_ik's two sides and two roundings of itself.
  The lower bound is a mean: the mean of the rows' allowances plus 2 (STRIP + strips) eps mean |log p|.
* M-step.  r = exp(log_resp) is 2 eps relative between two libraries.  n_k: N additions of non-negative terms, (N + 4) eps n_k.
  mu_kc = sum r x / n_k: (N + 4) eps sum r |x_c| / n_k + (N + 6) eps |mu_kc| =: dmu.  With df = x - mu (|d df| <= dmu + eps |df|),
  T_ab = sum r |df_a| |df_b| / n_k and M_a = sum r |df_a| / n_k: |dcov_ab| <= (N + 6) eps (T_ab + |cov_ab|) + M_a dmu_b + M_b dmu_a.
  'spherical' is a mean of d such entries: their mean plus (d + 2) eps |var|.
* Factor.  'diag' / 'spherical': P = var^-1/2, |dP| / P <= |dvar| / (2 var) + 3 eps.  'full': a relative perturbation rho of
  Sigma (Frobenius) moves its Cholesky factor L by <= kappa(Sigma) rho / sqrt 2 = kappa(L)^2 rho / sqrt 2 and the inverse of L by
  kappa(L) times that; the factorisation and the substitution add 4 (d + 2) eps kappa(L) each.  Allowed, Frobenius and relative:
  kappa(L)^3 (rho + 8 (d + 2) eps).  The table keeps kappa(L) <= ref.MAX_COND (asserted on the host, printed there and here).
  log_det = sum_j log P[j,j]: sqrt(d) |dP|_F / min_j P[j,j] + 4 d eps (1 + max_j |log P[j,j]|).
* sample: the substitution in fp64 is good to about d eps kappa; the one rounding to fp32 dominates: 2^-24 |z| (1 + 2^-20) + 1e-12.

Every test prints the figures it asserts on; DESIGN 3.7e records the largest."""
import json
import os

import numpy as np
import pytest
import torch

import gmm_ref as ref

pytestmark = pytest.mark.gpu

EPS = ref.EPS
ROWS = pytest.mark.parametrize("row", ref.CASES, ids=ref.case_id)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view({torch.float64: np.uint64, torch.float32: np.uint32, torch.int32: np.uint32}[t.dtype])


def load_params(w, mu, P, ctype):
    """reference parameters -> (a device parameter buffer with b and log_det prepared on the device, its views)"""
    from evae import ops
    K, d = mu.shape
    params = ops.gmm_params(d, K, ctype, 'cuda')
    params.zero_()
    v = ops.gmm_views(params, d, K, ctype)
    v['weights'].copy_(dev(np.asarray(w, np.float64)))
    v['means'].copy_(dev(np.asarray(mu, np.float64)))
    v['precisions_cholesky'].copy_(dev(np.asarray(P, np.float64)))
    ops.gmm_prepare(params, d, K, ctype)
    return params, v


def model_with(f, ctype, d):
    """a GaussianMixture carrying the reference fit f's parameters"""
    from evae import ops
    from evae.mixture import GaussianMixture
    K = len(f["weights"])
    gm = GaussianMixture(K, covariance_type=ctype, random_state=0)
    gm._params, v = load_params(f["weights"], f["means"], f["P"], ctype)
    gm.weights_, gm.means_, gm.precisions_cholesky_, gm.covariances_ = v['weights'], v['means'], v['precisions_cholesky'], v['covariances']
    gm.n_features_in_ = d
    return gm


def full_P(P, ctype, d):
    """[K x d x d] whatever the type"""
    if ctype == 'full':
        return P
    if ctype == 'diag':
        return np.stack([np.diag(p) for p in P])
    return np.stack([p * np.eye(d) for p in P])


def estep_allowance(X, w, mu, P, ctype, logp):
    """-> (E [N x K] per side, allowance of log p [N])"""
    X64 = np.abs(np.asarray(X, np.float64))
    n, d = X64.shape
    K = len(w)
    Pf = np.abs(full_P(P, ctype, d))
    E = np.empty((n, K))
    for k in range(K):
        a = X64 @ Pf[k] + (np.abs(mu[k]) @ Pf[k])[None, :]
        A = (a * a).sum(axis=1)
        Ld = np.abs(np.log(np.diagonal(Pf[k]))).sum()
        E[:, k] = (1.5 * d + 4.5) * EPS * A + 4 * EPS * (d * ref.LOG_2PI / 2 + abs(np.log(w[k]))) + (d + 4) * EPS * Ld
    return E, 2 * E.max(axis=1) + 2 * (K + 4) * EPS * (1 + np.abs(logp))


def check_estep(name, X, w, mu, P, ctype):
    from evae import ops
    n, d = X.shape
    K = len(w)
    params, _ = load_params(w, mu, P, ctype)
    log_resp, logp, mean = ops.gmm_estep(dev(X), params, K, ctype)
    assert log_resp.dtype == logp.dtype == mean.dtype == torch.float64 and tuple(log_resp.shape) == (n, K)
    rl, rp, rm = ref.estep(X, w, mu, P, ctype)
    E, allow_p = estep_allowance(X, w, mu, P, ctype, rp)
    allow_r = 2 * E + allow_p[:, None] + 2 * EPS * np.abs(rl)
    allow_m = allow_p.mean() + 2 * (ref.STRIP + (n + ref.STRIP - 1) // ref.STRIP) * EPS * np.abs(rp).mean()
    e_p, e_r, e_m = np.abs(host(logp) - rp), np.abs(host(log_resp) - rl), abs(float(mean.item()) - rm)
    print("estep %s: log p at %.3g of its allowance (largest error %.3g), log_resp at %.3g (%.3g), bound apart by %.3g (allowed %.3g)"
          % (name, (e_p / allow_p).max(), e_p.max(), (e_r / allow_r).max(), e_r.max(), e_m, allow_m))
    assert (e_p <= allow_p).all() and (e_r <= allow_r).all() and e_m <= allow_m
    return log_resp


@ROWS
def test_estep_on_the_table(row):
    s = ref.solved(*row)
    f = s["fit"]
    check_estep(ref.case_id(row), s["X"], f["weights"], f["means"], f["P"], row[3])


@pytest.mark.parametrize("d,ctype", [(1, 'full'), (2, 'full'), (15, 'full'), (16, 'full'), (17, 'full'), (63, 'full'), (64, 'full'),
                                     (65, 'full'), (95, 'full'), (96, 'full'), (255, 'diag'), (256, 'diag'), (256, 'spherical')])
def test_estep_over_the_width_edges(d, ctype):
    """widths around 16, around the 64 lanes of the sampling wave and at the caps; K = 5 leaves the last tile of components
    ragged, whether it holds 4 or (at d = 96) 3; a well-conditioned random factor per component"""
    rs = np.random.RandomState(d)
    n, K = 130, 5
    X = rs.standard_normal((n, d)).astype(np.float32)
    mu = 0.5 * rs.standard_normal((K, d))
    w = 1.0 + rs.random_sample(K)
    w /= w.sum()
    if ctype == 'full':
        P = np.triu(np.eye(d)[None] * (0.8 + 0.4 * rs.random_sample((K, d, 1))) + 0.2 * rs.standard_normal((K, d, d)) / np.sqrt(d))
    else:
        P = 0.8 + 0.4 * rs.random_sample((K, d) if ctype == 'diag' else K)
    check_estep("d%d %s" % (d, ctype), X, w, mu, P, ctype)


def mstep_allowances(X, resp, nk, mu, cov, ctype):
    X64 = np.asarray(X, np.float64)
    n, d = X64.shape
    K = len(nk)
    a_nk = (n + 4) * EPS * nk
    a_mu = (n + 4) * EPS * (resp.T @ np.abs(X64)) / nk[:, None] + (n + 6) * EPS * np.abs(mu)
    a_cov = np.empty((K, d, d)) if ctype == 'full' else np.empty((K, d))
    for k in range(K):
        df = np.abs(X64 - mu[k])
        r = resp[:, k][:, None]
        M = (r * df).sum(axis=0) / nk[k]
        if ctype == 'full':
            T = (r * df).T @ df / nk[k]
            a_cov[k] = (n + 6) * EPS * (T + np.abs(cov[k])) + M[:, None] * a_mu[k][None, :] + M[None, :] * a_mu[k][:, None]
        else:
            T = (r * df * df).sum(axis=0) / nk[k]
            c = cov[k] if ctype == 'diag' else np.full(d, cov[k])
            a_cov[k] = (n + 6) * EPS * (T + np.abs(c)) + 2 * M * a_mu[k]
    if ctype == 'spherical':
        a_cov = a_cov.mean(axis=1) + (d + 2) * EPS * np.abs(cov)
    return a_nk, a_mu, a_cov


def check_mstep(name, X, ctype, K, resp=None, labels=None):
    from evae import ops
    n, d = X.shape
    x = dev(X)
    params = ops.gmm_params(d, K, ctype, 'cuda')
    params.fill_(float('nan'))
    state = ops.gmm_state('cuda')
    if resp is not None:
        log_resp = np.log(resp)
        ops.gmm_mstep(x, params, K, ctype, ref.REG, state, log_resp=dev(log_resp))
        resp = np.exp(log_resp)
    else:
        ops.gmm_mstep(x, params, K, ctype, ref.REG, state, labels=dev(labels.astype(np.int32)))
        resp = ref.one_hot(labels, K)
    record = host(state)
    assert record[5] == -1.0 and record[1] == 0.0 and record[0] == 0.0
    v = {key: host(t) for key, t in ops.gmm_views(params, d, K, ctype).items()}
    nk, mu, cov = ref.mstep(X, resp, ref.REG, ctype)
    P, cond = ref.factor_of_covariances(cov, ctype)
    a_nk, a_mu, a_cov = mstep_allowances(X, resp, nk, mu, cov, ctype)
    e_nk, e_mu, e_cov = np.abs(v['nk'] - nk), np.abs(v['means'] - mu), np.abs(v['covariances'] - cov)
    e_w = np.abs(v['weights'] - nk / nk.sum())
    a_w = (a_nk + (K + 4) * EPS * nk) / nk.sum() + (nk / nk.sum()) * (a_nk.sum() / nk.sum())
    with np.errstate(invalid='ignore', divide='ignore'):     # an empty component of a labelling: 0 of an allowance of 0
        rep = "mstep %s: n_k at %.3g of its allowance, means %.3g, covariances %.3g, weights %.3g" % (
            name, np.nanmax(e_nk / a_nk), np.nanmax(e_mu / a_mu), np.nanmax(e_cov / a_cov), np.nanmax(e_w / a_w))
    assert (e_nk <= a_nk).all() and (e_mu <= a_mu).all() and (e_cov <= a_cov).all() and (e_w <= a_w).all(), rep
    ld = ref.log_det(P, ctype, d)
    worst_p = worst_l = 0.0
    for k in range(K):
        if ctype == 'full':
            L = np.linalg.cholesky(cov[k])
            kappa = float(np.linalg.cond(L))
            rho = np.linalg.norm(a_cov[k]) / np.linalg.norm(cov[k])
            a_p = kappa ** 3 * (rho + 8 * (d + 2) * EPS) * np.linalg.norm(P[k])
            e_p = np.linalg.norm(v['precisions_cholesky'][k] - P[k])
            diag = np.diagonal(P[k])
            assert np.array_equal(np.tril(v['precisions_cholesky'][k], -1), np.zeros((d, d)))
        else:
            pk, ck, ak = np.atleast_1d(P[k]), np.atleast_1d(cov[k]), np.atleast_1d(a_cov[k])
            a_vec = pk * (ak / (2 * ck) + 3 * EPS)
            a_p = np.linalg.norm(a_vec) if ctype == 'diag' else float(a_vec[0])
            e_p = np.linalg.norm(np.atleast_1d(v['precisions_cholesky'][k]) - pk)
            diag = pk if ctype == 'diag' else np.full(d, pk[0])
        a_l = np.sqrt(d) * (a_p if ctype != 'spherical' else a_p * np.sqrt(d)) / diag.min() + 4 * d * EPS * (1 + np.abs(np.log(diag)).max())
        e_l = abs(v['log_det'][k] - ld[k])
        worst_p, worst_l = max(worst_p, e_p / a_p), max(worst_l, e_l / a_l)
        assert e_p <= a_p and e_l <= a_l, (rep, k, e_p, a_p, e_l, a_l)
        b = (mu[k] @ P[k]) if ctype == 'full' else mu[k] * P[k]
        a_b = (d + 2) * EPS * (np.abs(mu[k]) @ np.abs(full_P(P, ctype, d)[k])) + np.abs(mu[k]).max() * a_p + np.abs(full_P(P, ctype, d)[k]).sum(axis=0) * a_mu[k].max()
        assert (np.abs(v['b'][k] - b) <= a_b).all(), (rep, k)
    print(rep + ", factor %.3g, log_det %.3g; factor condition %.3g" % (worst_p, worst_l, cond))


@ROWS
def test_mstep_from_responsibilities(row):
    s = ref.solved(*row)
    check_mstep(ref.case_id(row), s["X"], row[3], row[2], resp=np.exp(s["fit"]["log_resp"]))


@ROWS
def test_mstep_from_labels(row):
    s = ref.solved(*row)
    check_mstep(ref.case_id(row), s["X"], row[3], row[2], labels=s["fit"]["labels"])


# ---------------------------------------------------------------------------------------------- fits
def compare_fit(name, gm, labels, f, X, spread=ref.SPREAD):
    got = dict(weights=gm.weights_, means=gm.means_, covariances=gm.covariances_, P=gm.precisions_cholesky_)
    errs = {key: ref.rel_err(host(t), f[key]) for key, t in got.items()}
    errs["lower_bound"] = ref.rel_err(gm.lower_bound_, f["lower_bound"])
    print("fit %s: %d iterations (%d), converged %s, " % (name, gm.n_iter_, f["n_iter"], gm.converged_)
          + " ".join("%s %.3g" % kv for kv in sorted(errs.items())) + " | allowed "
          + " ".join("%s %.3g" % (k, 10 * v) for k, v in sorted(spread.items())))
    assert gm.n_iter_ == f["n_iter"] and gm.converged_ == f["converged"]
    assert np.array_equal(host(labels), f["labels"])
    assert np.array_equal(host(gm.predict(X)), f["labels"])
    for key, e in errs.items():
        assert e <= 10.0 * spread[key], (name, key, e)


def assert_margins(name, f):
    print("%s: stop margin %.3g, arg-max margin %.3g, smallest n_k %.3g, %d iterations" % (name, f["tol_margin"], f["argmax_margin"],
                                                                                          f["min_nk"], f["n_iter"]))
    assert f["tol_margin"] >= 1e-8 and f["argmax_margin"] >= 1e-9 and f["min_nk"] >= 1.0      # the preconditions of exactness


@ROWS
def test_fit_from_a_given_init(row):
    from evae.mixture import GaussianMixture
    n, d, K, ctype, seed = row
    s = ref.solved(*row)
    gm = GaussianMixture(K, covariance_type=ctype, tol=ref.TOL, reg_covar=ref.REG, max_iter=ref.MAX_ITER, weights_init=s["w"],
                         means_init=s["mu"], precisions_init=s["prec"])
    labels = gm.fit_predict(s["X"])
    assert labels.dtype == torch.int32 and labels.is_cuda and gm.means_.dtype == torch.float64
    compare_fit(ref.case_id(row), gm, labels, s["fit"], s["X"])


INIT_ROWS = [ref.CASES[0], ref.CASES[1], ref.CASES[12], ref.CASES[13]]


@pytest.mark.parametrize("row", INIT_ROWS, ids=ref.case_id)
def test_fit_from_kmeans(row):
    from evae.cluster import KMeans
    from evae.mixture import GaussianMixture
    n, d, K, ctype, seed = row
    X = ref.solved(*row)["X"]
    km_labels = host(KMeans(K, n_init=1, random_state=seed).fit(X).labels_)
    f = ref.fit_from_resp(X, ref.one_hot(km_labels, K), ctype)
    assert_margins("kmeans init " + ref.case_id(row), f)
    gm = GaussianMixture(K, covariance_type=ctype, init_params='kmeans', random_state=seed)
    compare_fit("kmeans init " + ref.case_id(row), gm, gm.fit_predict(X), f, X)


@pytest.mark.parametrize("row", ref.RANDOM_ROWS, ids=ref.case_id)
def test_fit_from_random_responsibilities(row):
    """held to the spread the host test records for these very fits (ref.SPREAD_RANDOM): a near-uniform start amplifies rounding"""
    from evae.mixture import GaussianMixture
    n, d, K, ctype, seed = row
    X = ref.solved(*row)["X"]
    _, f = ref.solved_from_random(*row)
    assert_margins("random init " + ref.case_id(row), f)
    assert f["converged"]
    gm = GaussianMixture(K, covariance_type=ctype, init_params='random', random_state=seed, max_iter=300)
    compare_fit("random init " + ref.case_id(row), gm, gm.fit_predict(X), f, X, ref.SPREAD_RANDOM)


def given(row, **kw):
    from evae.mixture import GaussianMixture
    s = ref.solved(*row)
    return GaussianMixture(row[2], covariance_type=row[3], tol=ref.TOL, reg_covar=ref.REG, weights_init=s["w"], means_init=s["mu"],
                           precisions_init=s["prec"], **kw)


def test_check_every_does_not_change_the_fit():
    row = ref.CASES[0]
    s = ref.solved(*row)
    runs = []
    for every in (1, 4, 7):
        gm = given(row, check_every=every)
        labels = gm.fit_predict(s["X"])
        compare_fit("check_every=%d" % every, gm, labels, s["fit"], s["X"])
        runs.append((bits(gm._params), bits(labels), gm.lower_bound_, gm.n_iter_))
    for other in runs[1:]:
        assert np.array_equal(other[0], runs[0][0]) and np.array_equal(other[1], runs[0][1]) and other[2:] == runs[0][2:]


def test_max_iter_is_not_an_error():
    row = ref.CASES[1]
    s = ref.solved(*row)
    f = ref.fit(s["X"], s["w"], s["mu"], ref.factor_of_precisions(s["prec"], row[3]), row[3], max_iter=5)
    assert not f["converged"] and f["n_iter"] == 5
    assert_margins("max_iter=5", f)
    gm = given(row, max_iter=5, check_every=4)
    labels = gm.fit_predict(s["X"])
    assert gm.converged_ is False and gm.n_iter_ == 5
    compare_fit("max_iter=5", gm, labels, f, s["X"])


def test_n_init_keeps_the_highest_bound():
    from evae.mixture import GaussianMixture
    row = ref.CASES[0]
    n, d, K, ctype, seed = row
    X = ref.solved(*row)["X"]
    g = torch.Generator().manual_seed(11)
    fits = [ref.fit_from_resp(X, ref.random_resp(n, K, g), ctype, max_iter=300) for _ in range(3)]
    bounds = [f["lower_bound"] for f in fits]
    best = int(np.argmax(bounds))
    gaps = sorted(bounds)
    print("n_init: bounds %s, the best is run %d" % (bounds, best))
    assert gaps[-1] - gaps[-2] >= 1e-9                       # the reference itself is clear about the winner
    for f in fits:
        assert_margins("n_init run", f)
    gm = GaussianMixture(K, covariance_type=ctype, init_params='random', random_state=11, n_init=3, max_iter=300)
    compare_fit("n_init=3", gm, gm.fit_predict(X), fits[best], X, ref.SPREAD_RANDOM)


def test_two_identical_fits_are_bit_equal():
    row = ref.CASES[1]
    X = ref.solved(*row)["X"]
    from evae.mixture import GaussianMixture
    runs = []
    for _ in range(2):
        gm = GaussianMixture(row[2], covariance_type=row[3], init_params='kmeans', random_state=4, n_init=2)
        labels = gm.fit_predict(X)
        runs.append([bits(gm._params), bits(gm.weights_), bits(gm.means_), bits(gm.covariances_), bits(gm.precisions_cholesky_),
                     bits(labels), np.array([gm.lower_bound_]).view(np.uint64), np.array([gm.n_iter_, int(gm.converged_)])])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def run_steps(row, fill, steps, extra=0):
    """gmm_step from the row's given init with every other buffer filled with `fill` -> (record, params, log_resp) bits"""
    from evae import ops
    n, d, K, ctype, seed = row
    s = ref.solved(*row)
    x = dev(s["X"])
    params, _ = load_params(s["w"], s["mu"], ref.factor_of_precisions(s["prec"], ctype), ctype)
    log_resp = torch.full((n, K), fill, dtype=torch.float64, device='cuda')
    logp = torch.full((n,), fill, dtype=torch.float64, device='cuda')
    ws = ops.gmm_workspace(n, d, K, ctype, 'cuda')
    ws.view(torch.float64)[:] = fill if ws.numel() % 8 == 0 else 0.0
    state = ops.gmm_state('cuda')
    for _ in range(steps):
        ops.gmm_step(x, params, K, ctype, log_resp, logp, ref.REG, ref.TOL, state, ws)
    before = (bits(state), bits(params), bits(log_resp), bits(logp))
    for _ in range(extra):
        ops.gmm_step(x, params, K, ctype, log_resp, logp, ref.REG, ref.TOL, state, ws)
    return before, (bits(state), bits(params), bits(log_resp), bits(logp)), host(state)


@pytest.mark.parametrize("row", [ref.CASES[0], ref.CASES[12], ref.CASES[13]], ids=ref.case_id)
def test_first_step_does_not_depend_on_what_the_buffers_held(row):
    clean, _, record = run_steps(row, 0.0, 1)
    dirty, _, _ = run_steps(row, float('nan'), 1)
    assert record[0] == 1.0 and record[1] == 0.0 and record[4] == -np.inf and record[5] == -1.0
    s = ref.solved(*row)
    _, _, lb = ref.estep(s["X"], s["w"], s["mu"], ref.factor_of_precisions(s["prec"], row[3]), row[3])
    assert abs(record[3] - lb) <= 1e-12 * abs(lb)
    for a, b in zip(clean, dirty):
        assert np.array_equal(a, b)


def test_steps_after_the_done_flag_change_nothing():
    row = ref.CASES[0]
    f = ref.solved(*row)["fit"]
    before, after, record = run_steps(row, 0.0, f["n_iter"], extra=3)
    assert record[0] == f["n_iter"] and record[1] == 1.0 and record[2] == 1.0
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("ctype", ['full', 'diag', 'spherical'])
def test_a_collapsed_component_raises_and_the_process_stays_usable(ctype):
    """reg_covar = 0 and a component made of 60 copies of one point: its covariance is exactly zero (the other blob is 200 units
    away, its responsibilities underflow to 0), the first pivot is not positive: a flag in the record, not a device fault"""
    from evae.mixture import GaussianMixture
    rs = np.random.RandomState(0)
    X = np.concatenate([rs.standard_normal((100, 3)), np.tile(np.array([[200.0, 0.0, 0.0]]), (60, 1))]).astype(np.float32)
    prec = {'full': np.tile(np.eye(3), (2, 1, 1)), 'diag': np.ones((2, 3)), 'spherical': np.ones(2)}[ctype]
    gm = GaussianMixture(2, covariance_type=ctype, reg_covar=0.0, weights_init=np.array([0.5, 0.5]),
                         means_init=np.array([[0.0, 0.0, 0.0], [200.0, 0.0, 0.0]]), precisions_init=prec)
    with pytest.raises(ValueError, match=r"ill-defined empirical covariance.*component is 1\."):
        gm.fit(X)
    assert torch.isfinite(torch.ones(1, device='cuda') * 2).all()
    row = ref.CASES[4]
    s = ref.solved(*row)
    ok = given(row)
    compare_fit("after the refusal", ok, ok.fit_predict(s["X"]), s["fit"], s["X"])


# ---------------------------------------------------------------------------------------------- densities, memberships
@pytest.mark.parametrize("row", [ref.CASES[0], ref.CASES[1], ref.CASES[12], ref.CASES[13]], ids=ref.case_id)
def test_densities_and_memberships(row):
    n, d, K, ctype, seed = row
    s = ref.solved(*row)
    f = s["fit"]
    X = ref.blobs(300, d, K, seed + 100)[0]                  # held-out rows
    gm = model_with(f, ctype, d)
    rl, rp, rm = ref.estep(X, f["weights"], f["means"], f["P"], ctype)
    _, allow_p = estep_allowance(X, f["weights"], f["means"], f["P"], ctype, rp)
    got = gm.score_samples(X)
    assert got.dtype == torch.float64 and got.is_cuda and (np.abs(host(got) - rp) <= allow_p).all()
    allow_m = allow_p.mean() + 2 * (ref.STRIP + 5) * EPS * np.abs(rp).mean()
    assert abs(gm.score(X) - rm) <= allow_m
    proba = host(gm.predict_proba(X))
    sums = np.abs(proba.sum(axis=1) - 1.0).max()
    apart = np.abs(proba - np.exp(rl)).max()
    print("%s: predict_proba rows sum to 1 within %.3g (allowed K eps = %.3g), apart from the reference by %.3g"
          % (ref.case_id(row), sums, K * EPS, apart))
    assert sums <= K * EPS
    E, _ = estep_allowance(X, f["weights"], f["means"], f["P"], ctype, rp)
    allow_r = 2 * E + allow_p[:, None] + 2 * EPS * np.abs(rl)           # of log_resp; a probability moves by itself times that,
    assert (np.abs(proba - np.exp(rl)) <= np.exp(rl) * allow_r + (K + 6) * EPS).all()   # plus exp, the row sum and the division
    margin = np.sort(rl, axis=1)
    if K > 1:
        assert (margin[:, -1] - margin[:, -2]).min() >= 1e-9
    assert np.array_equal(host(gm.predict(X)), np.argmax(rl, axis=1))
    p = ref.n_parameters(K, d, ctype)
    bic, aic = -2 * rm * len(X) + p * np.log(len(X)), -2 * rm * len(X) + 2 * p
    assert abs(gm.bic(X) - bic) <= 2 * len(X) * allow_m + 4 * EPS * abs(bic)
    assert abs(gm.aic(X) - aic) <= 2 * len(X) * allow_m + 4 * EPS * abs(aic)


@pytest.mark.parametrize("ctype", ['full', 'diag', 'spherical'])
def test_predict_breaks_ties_to_the_lowest_component(ctype):
    rs = np.random.RandomState(1)
    d = 5
    X = np.concatenate([rs.standard_normal((80, d)), 4.0 + rs.standard_normal((80, d))]).astype(np.float32)
    mu = np.array([np.zeros(d), np.full(d, 4.0), np.full(d, 4.0)])       # components 1 and 2 are one and the same
    P = {'full': np.tile(np.triu(np.eye(d) + 0.1), (3, 1, 1)), 'diag': np.full((3, d), 0.9), 'spherical': np.full(3, 0.9)}[ctype]
    f = dict(weights=np.array([0.4, 0.3, 0.3]), means=mu, P=P)
    labels = host(model_with(f, ctype, d).predict(X))
    assert set(labels.tolist()) == {0, 1} and (labels[80:] == 1).sum() >= 70


# ---------------------------------------------------------------------------------------------- sampling
@pytest.mark.parametrize("row", [ref.CASES[1], ref.CASES[9], ref.CASES[12], ref.CASES[13]], ids=ref.case_id)
def test_sample_against_the_reference(row):
    from evae import ops
    n, d, K, ctype, seed = row
    f = ref.solved(*row)["fit"]
    rs = np.random.RandomState(seed)
    m = 70
    comp, eps = rs.randint(0, K, m).astype(np.int32), rs.standard_normal((m, d))
    params, _ = load_params(f["weights"], f["means"], f["P"], ctype)
    z = ops.gmm_sample(params, d, K, ctype, dev(comp), dev(eps))
    assert z.dtype == torch.float32 and tuple(z.shape) == (m, d)
    want = ref.sample(f["means"], f["P"], ctype, comp, eps)
    err = np.abs(host(z).astype(np.float64) - want)
    allow = 2.0 ** -24 * np.abs(want) * (1 + 2.0 ** -20) + 1e-12
    print("sample %s: %.3g of one rounding to float32, %d of %d entries equal the rounded reference" % (
        ref.case_id(row), (err / allow).max(), int((host(z) == want.astype(np.float32)).sum()), want.size))
    assert (err <= allow).all()


def test_sample_of_a_model():
    from evae import ops
    row = ref.CASES[1]
    n, d, K, ctype, seed = row
    gm = model_with(ref.solved(*row)["fit"], ctype, d)
    z, comp = gm.sample(500)
    assert z.dtype == torch.float32 and z.is_cuda and tuple(z.shape) == (500, d) and comp.dtype == torch.int32
    c = host(comp)
    counts = np.bincount(c, minlength=K)
    assert counts.sum() == 500 and len(counts) == K and (np.diff(c) >= 0).all()
    draws_c, draws_e = gm.sample_draws(500)
    assert np.array_equal(host(draws_c), c)
    f = ref.solved(*row)["fit"]
    want = ref.sample(f["means"], f["P"], ctype, c, draws_e.numpy())
    assert (np.abs(host(z) - want) <= 2.0 ** -24 * np.abs(want) * (1 + 2.0 ** -20) + 1e-12).all()
    z2, comp2 = gm.sample(500)
    assert np.array_equal(bits(z), bits(z2)) and np.array_equal(c, host(comp2))
    assert np.abs(counts / 500.0 - f["weights"]).max() <= 0.1


# ---------------------------------------------------------------------------------------------- inputs, refusals, report
def test_host_tensors_and_arrays_are_taken_as_device_tensors_are():
    row = ref.CASES[4]
    X = ref.solved(*row)["X"]
    runs = []
    for data in (X, torch.from_numpy(X), torch.from_numpy(X).cuda(), X.astype(np.float64)):
        gm = given(row)
        labels = gm.fit_predict(data)
        runs.append((bits(gm._params), bits(labels), bits(gm.score_samples(data))))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)


def test_ops_refuse_host_tensors_wrong_dtypes_and_sizes_beyond_the_caps():
    from evae import _lib, ops
    x = torch.zeros((100, 4), device='cuda')
    params = ops.gmm_params(4, 3, 'full', 'cuda')
    state = ops.gmm_state('cuda')
    ws = ops.gmm_workspace(100, 4, 3, 'full', 'cuda')
    lr, lp = torch.zeros((100, 3), dtype=torch.float64, device='cuda'), torch.zeros(100, dtype=torch.float64, device='cuda')
    with _lib.count_calls("evae_gmm_step") as a, _lib.count_calls("evae_gmm_estep") as b, _lib.count_calls("evae_gmm_mstep") as c, \
            _lib.count_calls("evae_gmm_sample") as e:
        for bad in (lambda: ops.gmm_estep(x.cpu(), params, 3, 'full'), lambda: ops.gmm_estep(x, params.cpu(), 3, 'full'),
                    lambda: ops.gmm_estep(x.double(), params, 3, 'full'), lambda: ops.gmm_estep(x, params.float(), 3, 'full'),
                    lambda: ops.gmm_estep(x, params[:-1], 3, 'full'), lambda: ops.gmm_estep(x, params, 3, 'tied'),
                    lambda: ops.gmm_estep(x.t(), params, 3, 'full'),
                    lambda: ops.gmm_mstep(x, params, 3, 'full', 1e-6, state), lambda: ops.gmm_mstep(x, params, 3, 'full', 1e-6, state, lr.cpu()),
                    lambda: ops.gmm_mstep(x, params, 3, 'full', 1e-6, state, labels=torch.zeros(100, dtype=torch.int64, device='cuda')),
                    lambda: ops.gmm_mstep(x, params, 3, 'full', -1.0, state, lr),
                    lambda: ops.gmm_step(x, params, 3, 'full', lr.float(), lp, 1e-6, 1e-3, state, ws),
                    lambda: ops.gmm_step(x, params, 3, 'full', lr, lp, 1e-6, 1e-3, state.cpu(), ws),
                    lambda: ops.gmm_step(x, params, 3, 'full', lr, lp, 1e-6, -1.0, state, ws),
                    lambda: ops.gmm_estep(torch.zeros((10, 97), device='cuda'), params, 3, 'full'),
                    lambda: ops.gmm_params(4, 257, 'full', 'cuda'), lambda: ops.gmm_params(257, 2, 'diag', 'cuda'),
                    lambda: ops.gmm_sample(params, 4, 3, 'full', torch.zeros(5, dtype=torch.int32), torch.zeros((5, 4), dtype=torch.float64)),
                    lambda: ops.gmm_sample(params, 4, 3, 'full', torch.zeros(5, dtype=torch.int32, device='cuda'),
                                           torch.zeros((5, 4), dtype=torch.float32, device='cuda')),
                    lambda: ops.gmm_argmax(lr.cpu()), lambda: ops.gmm_argmax(lr.float())):
            with pytest.raises(_lib.EvaeError):
                bad()
    assert not a and not b and not c and not e
    lib = _lib.load()
    assert lib.evae_gmm_step(_lib.vp(x), 100, 4, 3, 0, _lib.vp(params), _lib.vp(lr), _lib.vp(lp), 1e-6, 1e-3, _lib.vp(state), _lib.vp(ws),
                             8, None) != 0                   # a workspace too small is refused by the library itself
    assert b"workspace" in lib.evae_last_error()


def test_report_on_a_stub_model(tmp_path, capsys):
    import evae_oracle as orc
    import smoke_case
    import golden_inputs as gi
    from utils.gmm_on_latent import report_gmm_on_latent
    B = 32
    args = smoke_case.vae_args(number_components=20, training_set_size=100, batch_size=B)
    args.seed, args.gmm_components, args.gmm_covariance_type, args.gmm_max_iter = 3, 3, 'diag', 20
    model, _ = smoke_case.build_model(torch, np, orc, args)
    model.eval()

    def loader(seed, n):
        data = torch.from_numpy(gi.binary_images(seed, n))
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, torch.arange(n) % 10), batch_size=B, shuffle=False)

    out = str(tmp_path / "gmm")
    gm = report_gmm_on_latent(loader(91, 130), loader(92, 75), model, out, args)
    assert "mixture of 3 diag Gaussians" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == ["gmm_covariances.npy", "gmm_means.npy", "gmm_quality.json", "gmm_test_labels.npy", "gmm_weights.npy"]
    zd = gm.n_features_in_
    assert np.load(os.path.join(out, "gmm_weights.npy")).shape == (3,) and np.load(os.path.join(out, "gmm_means.npy")).shape == (3, zd)
    assert np.load(os.path.join(out, "gmm_covariances.npy")).shape == (3, zd)
    saved = np.load(os.path.join(out, "gmm_test_labels.npy"))
    assert saved.dtype == np.int32 and saved.shape == (64,)
    quality = json.load(open(os.path.join(out, "gmm_quality.json")))
    assert sorted(quality) == sorted(["lower_bound", "n_iter", "converged", "bic", "aic", "train_mean_log_density", "test_mean_log_density",
                                      "nmi", "ari", "purity", "n_components", "n_train", "n_test"])
    assert quality["n_train"] == 128 and quality["n_test"] == 64 and quality["n_iter"] == gm.n_iter_
    assert quality["train_mean_log_density"] == gm.score(_train_latents(model, loader(91, 130), args, B))
    args.gmm_decode = 5
    report_gmm_on_latent(loader(91, 130), loader(92, 75), model, out, args)
    samples = np.load(os.path.join(out, "gmm_samples.npy"))
    with torch.no_grad():
        want = model.generate_x_from_z(torch.zeros((5, zd), device=args.device), with_reparameterize=False)
    assert samples.shape == tuple(want.shape) and np.isfinite(samples).all()


def _train_latents(model, loader, args, B):
    from utils.knn_on_latent import _posterior_means, extract_full_data
    x, _, _ = extract_full_data(loader)
    with torch.no_grad():
        return _posterior_means(model, x.to(args.device), B)
