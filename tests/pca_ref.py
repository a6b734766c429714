"""numpy float64 restatement of what csrc/evae_pca.hip and evae/pca.py compute: the covariance of the centred rows,
np.linalg.eigh, descending order, the sign rule of scikit-learn's svd_flip(u_based_decision=False), the projection and the
initial state of TSNE(init='pca').  tests/test_pca_ref_host.py holds this file to sklearn.decomposition.PCA(svd_solver='full');
tests/test_gpu_pca.py holds the kernels to this file."""
import numpy as np

EPS = 2.0 ** -52

# (n, d, ratio, seed) of the planted inputs the GPU tests use: below, at and above the 64-lane width of a column (63 / 64 / 65
# sit in the moments tests), both homes of the solver's matrices (d <= 96: LDS; above: the workspace), odd d (a bye in the
# round-robin), one to five chunks of rows
PLANTED = ((97, 3, 1.5, 11), (300, 40, 1.5, 12), (1025, 40, 1.5, 13), (4099, 40, 1.5, 14), (257, 64, 1.3, 15), (300, 65, 1.3, 16),
           (2049, 128, 1.1, 17), (513, 256, 1.05, 18))


def planted(n, d, ratio, seed):
    """X float32 [n x d] (n > d) whose sample covariance has the eigenvalues ratio^-j, j = 0 .. d - 1, up to the float32 rounding
    of X: orthonormal centred scores times sqrt(n - 1) s_j, s_j = ratio^(-j / 2), in a random orthonormal basis, plus a mean."""
    rs = np.random.RandomState(seed)
    G = rs.randn(n, d)
    G -= G.mean(axis=0)
    Qg = np.linalg.qr(G)[0]
    Q = np.linalg.qr(rs.randn(d, d))[0]
    s = float(ratio) ** (-np.arange(d) / 2.0)
    X = np.sqrt(n - 1.0) * (Qg * s) @ Q.T + 3.0 * rs.randn(d)
    return X.astype(np.float32)


def moments(X):
    """-> (mean [d], cov [d x d]) of the rows, ddof 1, from the centred rows"""
    X = np.asarray(X, np.float64)
    mean = X.mean(axis=0)
    Xc = X - mean
    return mean, Xc.T @ Xc / (len(X) - 1.0)


def sign_rule(comps):
    """every row's entry of largest magnitude made positive, the lowest index on a tie"""
    comps = np.array(comps, np.float64)
    at = np.argmax(np.abs(comps), axis=1)                 # the first of equal maxima
    signs = np.where(comps[np.arange(len(comps)), at] < 0, -1.0, 1.0)
    return comps * signs[:, None]


def eigh(cov):
    """-> (evals [d] descending, ties by original index, clamped at 0; comps [d x d], row i = component i, sign rule applied)"""
    w, v = np.linalg.eigh(np.asarray(cov, np.float64))
    order = np.argsort(-w, kind="stable")
    return np.maximum(w[order], 0.0), sign_rule(v[:, order].T)


def fit(X):
    """-> (mean, evals, comps): the decomposition eigh(moments(X)[1]) stands for, taken from the singular values of the centred
    rows.  eigh of the covariance leaves an error of eps lambda_max / gap_i in component i -- 1.4e-10 at (300, 40, ratio 1.5),
    where the smallest eigenvalue is 1.4e-7 of the largest -- which is the solver tests' own allowance (test_gpu_pca.py) but
    not what a reference of the whole fit should carry; the singular vectors are good to eps sigma_max / (sigma gap), and
    agree with scikit-learn's 'full' solver to 1e-14.  test_pca_ref_host.py holds the two routes together at that allowance."""
    X = np.asarray(X, np.float64)
    mean = X.mean(axis=0)
    assert len(X) >= X.shape[1], "fit: at least as many rows as columns (d singular values)"
    s, vt = np.linalg.svd(X - mean, full_matrices=False)[1:]
    return mean, s * s / (len(X) - 1.0), sign_rule(vt)


def project(X, mean, comps, scale=1.0):
    return scale * ((np.asarray(X, np.float64) - mean) @ np.asarray(comps, np.float64).T)


def reconstruct(Y, mean, comps):
    return mean + np.asarray(Y, np.float64) @ np.asarray(comps, np.float64)


def tsne_initial(X):
    """scikit-learn's TSNE(init='pca'): the first two principal components' scores, divided by np.std of the first column,
    times 1e-4 (float64 throughout; scikit-learn rounds the scores to float32 before the division)"""
    mean, _, comps = fit(X)
    Y = project(X, mean, comps[:2])
    return Y / np.std(Y[:, 0]) * 1e-4


def min_neighbour_ratio(evals):
    """the smallest ratio of neighbouring eigenvalues, descending order"""
    evals = np.asarray(evals, np.float64)
    return float(np.min(evals[:-1] / evals[1:])) if len(evals) > 1 else np.inf


def sign_margins(comps):
    """per row: the largest |entry| minus the second largest (inf for a single column)"""
    a = np.sort(np.abs(np.asarray(comps, np.float64)), axis=1)
    return a[:, -1] - a[:, -2] if a.shape[1] > 1 else np.full(len(a), np.inf)


def gaps(evals):
    """per eigenvalue: the distance to the nearest other one (inf for a single one)"""
    evals = np.asarray(evals, np.float64)
    if len(evals) == 1:
        return np.full(1, np.inf)
    diff = np.abs(np.diff(evals))
    return np.minimum(np.concatenate(([np.inf], diff)), np.concatenate((diff, [np.inf])))
