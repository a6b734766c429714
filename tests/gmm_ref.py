"""numpy float64 restatement of what csrc/evae_gmm.hip computes: the yardstick of tests/test_gpu_gmm.py, held to
scikit-learn by tests/test_gmm_ref_host.py.  Not product code.  The E-step goes through the upper-triangular precision factors
P_k (P_k P_k^T = Sigma_k^-1), the M-step takes covariances about the new means (two passes), and the loop is scikit-learn's:
E-step, M-step, then |bound - previous| < tol.  A fit also returns how far the reference itself was from deciding otherwise --
the stop's margin, the arg-max margin of the final responsibilities, the smallest n_k -- so a GPU test may compare n_iter,
converged and labels exactly only where those are far above fp64 rounding."""
import functools

import numpy as np

EPS = 2.0 ** -52
CHUNK = 512           # ops.gmm_chunk_rows(): rows whose weighted sums are formed together (test_gmm_ref_host.py asserts it)
STRIP = 64            # ops.gmm_strip_rows(): rows of an E-step block
TOL, REG, MAX_ITER = 1e-3, 1e-6, 100
LOG_2PI = float(np.log(2.0 * np.pi))

# (n, d, K, type, seed).  n straddles CHUNK (and one row lies below STRIP), d straddles 16 and reaches the caps, K reaches 256.
CASES = [(1023, 2, 3, 'full', 0), (1024, 16, 10, 'full', 1), (2049, 40, 10, 'full', 32), (600, 2, 33, 'full', 3),
         (511, 2, 2, 'full', 4), (512, 16, 2, 'full', 5), (513, 17, 1, 'full', 6), (1025, 15, 10, 'full', 7),
         (40, 1, 2, 'full', 8), (1200, 96, 2, 'full', 9), (2049, 2, 256, 'diag', 10), (1025, 256, 3, 'diag', 11),
         (513, 17, 10, 'diag', 12), (1024, 16, 10, 'spherical', 13), (1025, 40, 33, 'spherical', 14), (2049, 1, 2, 'full', 15),
         (2049, 40, 33, 'diag', 16)]


MAX_COND = 100.0      # the largest condition number of a covariance's Cholesky factor that a row of the table may reach

# The largest difference between this reference and scikit-learn 1.7.2 over the table, each relative to the largest magnitude of
# the quantity (tests/test_gmm_ref_host.py measures and asserts 10 x these; tests/test_gpu_gmm.py holds the kernels' fits to the
# same 10 x): two float64 implementations that differ in summation order and, for 'diag', in the covariance formula.
SPREAD = dict(weights=9.7e-15, means=8.3e-15, covariances=3.2e-14, P=2.9e-14, lower_bound=3.5e-16)


# The same for fits from random responsibilities (RANDOM_ROWS): a near-uniform start leaves EM to break a symmetry, which amplifies
# rounding -- n1024_d16_K10_full takes 38 iterations and its two float64 implementations end 1e-12 apart.
SPREAD_RANDOM = dict(weights=9.9e-13, means=1.6e-12, covariances=1.5e-12, P=5.7e-12, lower_bound=8.9e-16)


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def case_id(row):
    return "n%d_d%d_K%d_%s" % row[:4]


def blobs(n, d, K, seed, centre_scale=0.8):
    """-> (X float32 [n x d], component of every row): K Gaussian blobs, each a random linear map (identity + 0.3 x normal / sqrt d,
    so the covariances stay well conditioned) of standard normals, centres drawn at centre_scale of the within-cluster scale:
    the blobs overlap and EM takes tens of iterations"""
    rs = np.random.RandomState(seed)
    centres = centre_scale * rs.standard_normal((K, d))
    maps = np.eye(d)[None] + 0.3 * rs.standard_normal((K, d, d)) / np.sqrt(d)
    y = np.arange(n) % K
    rs.shuffle(y)
    X = centres[y] + np.einsum('ni,nij->nj', rs.standard_normal((n, d)), maps[y])
    return X.astype(np.float32), y


def given_init(X, K, ctype, seed):
    """-> (weights [K], means [K x d], precisions): K distinct rows as means, unequal weights, every precision the inverse of
    the data's mean variance"""
    rs = np.random.RandomState(5000 + seed)
    X64 = np.asarray(X, np.float64)
    n, d = X64.shape
    means = X64[rs.choice(n, K, replace=False)].copy()
    w = 1.0 + rs.random_sample(K)
    w /= w.sum()
    p = 1.0 / float(X64.var(axis=0).mean())
    prec = {'full': np.tile(p * np.eye(d), (K, 1, 1)), 'diag': np.full((K, d), p), 'spherical': np.full(K, p)}[ctype]
    return w, means, prec


def factor_of_precisions(prec, ctype):
    """scikit-learn's precisions_cholesky_ of given precisions"""
    if ctype != 'full':
        return np.sqrt(prec)
    return np.array([np.linalg.cholesky(p[::-1, ::-1])[::-1, ::-1] for p in prec])


def factor_of_covariances(cov, ctype):
    """-> (P, the largest condition number of a Cholesky factor): P_k upper triangular with P_k P_k^T = Sigma_k^-1, i.e. the
    transposed inverse of the lower Cholesky factor; 1 / sqrt(var) for 'diag' and 'spherical'"""
    if ctype != 'full':
        if np.any(~(cov > 0)):
            raise ValueError("ill-defined empirical covariance: component %d" % int(np.argmax(~(cov.reshape(len(cov), -1) > 0).all(1))))
        return 1.0 / np.sqrt(cov), float(np.sqrt(cov.max() / cov.min()))
    P, cond = np.empty_like(cov), 1.0
    for k, c in enumerate(cov):
        try:
            L = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            raise ValueError("ill-defined empirical covariance: component %d" % k)
        P[k] = np.triu(np.linalg.solve(L, np.eye(len(c))).T)
        cond = max(cond, float(np.linalg.cond(L)))
    return P, cond


def log_det(P, ctype, d):
    if ctype == 'full':
        return np.log(np.diagonal(P, axis1=1, axis2=2)).sum(axis=1)
    return np.log(P).sum(axis=1) if ctype == 'diag' else d * np.log(P)


def mean_in_strips(v):
    """the mean as the kernels form it: strips of STRIP rows added in row order, then the strips in order"""
    strips = [np.cumsum(v[s:s + STRIP])[-1] for s in range(0, len(v), STRIP)]
    return float(np.cumsum(strips)[-1] / len(v))


def estep(X, w, mu, P, ctype):
    """-> (log_resp [N x K], log p(x_i) [N], their mean)"""
    X64 = np.asarray(X, np.float64)
    n, d = X64.shape
    K = len(w)
    ld = log_det(P, ctype, d)
    lp = np.empty((n, K))
    for k in range(K):
        if ctype == 'full':
            y = X64 @ P[k] - mu[k] @ P[k]
        elif ctype == 'diag':
            y = X64 * P[k] - mu[k] * P[k]
        else:
            y = X64 * P[k] - mu[k] * P[k]
        lp[:, k] = -0.5 * (d * LOG_2PI + (y * y).sum(axis=1)) + ld[k]
    with np.errstate(divide='ignore'):
        lp += np.log(w)[None, :]
    mx = lp.max(axis=1)
    logp = mx + np.log(np.exp(lp - mx[:, None]).sum(axis=1))
    return lp - logp[:, None], logp, mean_in_strips(logp)


def mstep(X, resp, reg, ctype):
    """-> (n_k [K], means [K x d], covariances): n_k = sum r + 10 eps; covariances about the NEW means (two passes), + reg on the
    diagonal; 'spherical' is the mean of the diagonal"""
    X64 = np.asarray(X, np.float64)
    n, d = X64.shape
    nk = resp.sum(axis=0) + 10.0 * EPS
    mu = (resp.T @ X64) / nk[:, None]
    K = len(nk)
    cov = np.empty((K, d, d)) if ctype == 'full' else np.empty((K, d))
    for k in range(K):
        df = X64 - mu[k]
        if ctype == 'full':
            cov[k] = (resp[:, k][:, None] * df).T @ df / nk[k]
            cov[k].flat[::d + 1] += reg
        else:
            cov[k] = (resp[:, k][:, None] * df * df).sum(axis=0) / nk[k] + reg
    if ctype == 'spherical':
        cov = cov.mean(axis=1)
    return nk, mu, cov


def one_hot(labels, K):
    r = np.zeros((len(labels), K))
    r[np.arange(len(labels)), labels] = 1.0
    return r


def fit(X, w, mu, P, ctype, tol=TOL, reg=REG, max_iter=MAX_ITER):
    """scikit-learn's loop from given weights, means and factors -> dict(weights, means, covariances, P, n_iter, converged,
    lower_bound (of the last E-step of the loop: the parameters before the last M-step), bounds, tol_margin = the smallest
    | |change| - tol | over the iterations, min_nk, cond, and from one closing E-step labels, argmax_margin, log_resp, logp)"""
    w, mu, P = np.array(w, np.float64), np.array(mu, np.float64), np.array(P, np.float64)
    lb, bounds, converged, tol_margin, min_nk, cond, cov, n_iter = -np.inf, [], False, np.inf, np.inf, 1.0, None, 0
    for n_iter in range(1, max_iter + 1):
        prev = lb
        log_resp, _, lb = estep(X, w, mu, P, ctype)
        nk, mu, cov = mstep(X, np.exp(log_resp), reg, ctype)
        w = nk / nk.sum()
        P, c = factor_of_covariances(cov, ctype)
        cond, min_nk = max(cond, c), min(min_nk, float(nk.min()))
        bounds.append(lb)
        tol_margin = min(tol_margin, abs(abs(lb - prev) - tol))
        if abs(lb - prev) < tol:
            converged = True
            break
    log_resp, logp, _ = estep(X, w, mu, P, ctype)
    labels = np.argmax(log_resp, axis=1)
    margin = np.inf
    if log_resp.shape[1] > 1:
        two = -np.partition(-log_resp, 1, axis=1)[:, :2]
        margin = float((two[:, 0] - two[:, 1]).min())
    return dict(weights=w, means=mu, covariances=cov, P=P, n_iter=n_iter, converged=converged, lower_bound=lb, bounds=bounds,
                tol_margin=float(tol_margin), min_nk=min_nk, cond=cond, labels=labels, argmax_margin=margin, log_resp=log_resp,
                logp=logp)


def fit_from_resp(X, resp, ctype, tol=TOL, reg=REG, max_iter=MAX_ITER):
    """the initial M-step scikit-learn makes from responsibilities (weights = n_k / sum n here), then fit"""
    nk, mu, cov = mstep(X, resp, reg, ctype)
    P, _ = factor_of_covariances(cov, ctype)
    return fit(X, nk / nk.sum(), mu, P, ctype, tol, reg, max_iter)


def sample(mu, P, ctype, comp, eps):
    """float64 [n x d]: mu_c + (P_c^T)^-1 eps by forward substitution, every column's running value in ascending row order"""
    eps = np.asarray(eps, np.float64)
    n, d = eps.shape
    out = np.empty((n, d))
    for i in range(n):
        c = int(comp[i])
        if ctype != 'full':
            out[i] = mu[c] + eps[i] / P[c]
            continue
        acc = eps[i].copy()
        for j in range(d):
            acc[j] = acc[j] / P[c][j, j]
            acc[j + 1:] -= P[c][j, j + 1:] * acc[j]
        out[i] = mu[c] + acc
    return out


def n_parameters(K, d, ctype):
    return {'full': K * d * (d + 1) // 2, 'diag': K * d, 'spherical': K}[ctype] + K * d + K - 1


@functools.lru_cache(maxsize=None)
def solved(n, d, K, ctype, seed):
    """a row of CASES fitted from its given initialisation: computed once, shared, never written to"""
    X, y = blobs(n, d, K, seed)
    w, mu, prec = given_init(X, K, ctype, seed)
    return dict(X=X, y=y, w=w, mu=mu, prec=prec, fit=fit(X, w, mu, factor_of_precisions(prec, ctype), ctype))


RANDOM_ROWS = [CASES[0], CASES[1], CASES[12], CASES[13]]


def random_resp(n, K, generator):
    """what GaussianMixture(init_params='random') draws from its CPU generator: uniforms in float64, normalised per row; the
    kernel takes exp of the logarithm it is given"""
    import torch
    resp = torch.rand((n, K), dtype=torch.float64, generator=generator)
    resp /= resp.sum(dim=1, keepdim=True)
    return np.exp(np.log(resp.numpy()))


@functools.lru_cache(maxsize=None)
def solved_from_random(n, d, K, ctype, seed):
    import torch
    X = solved(n, d, K, ctype, seed)["X"]
    resp = random_resp(n, K, torch.Generator().manual_seed(seed))
    return resp, fit_from_resp(X, resp, ctype, max_iter=300)
