"""numpy restatement of the exact t-SNE the kernels of csrc/evae_tsne.hip compute.  Every function takes a
`dtype`: float64 is the reference the kernels are held to; the same formulas in float32 give the yardstick of what float32
arithmetic costs at a case (tests/test_gpu_tsne.py: a kernel may miss float64 by 8 x that error, never by its own).
tests/test_tsne_ref_host.py holds this file to scikit-learn's private routines."""
import numpy as np

SEARCH_STEPS = 100


def blobs(n, zd, n_blobs, seed, shift=4.0):
    """shifted class means plus unit noise -> (X float32 [n x zd], labels [n])"""
    rs = np.random.RandomState(seed)
    means = rs.randn(n_blobs, zd) * shift / np.sqrt(zd) * np.sqrt(2.0)
    labels = np.arange(n) % n_blobs
    return (means[labels] + rs.randn(n, zd)).astype(np.float32), labels


def sq_distances(X, dtype=np.float64):
    """[N x N] squared distances by direct differences, all arithmetic in dtype"""
    X = np.asarray(X).astype(dtype)
    out = np.zeros((len(X), len(X)), dtype)
    for k in range(X.shape[1]):
        d = X[:, k][:, None] - X[:, k][None, :]
        out += d * d
    return out


def _shifted(D, dtype):
    D = np.asarray(D).astype(dtype)
    n = len(D)
    off = ~np.eye(n, dtype=bool)
    dmin = np.where(off, D, np.inf).min(axis=1).astype(dtype)
    dd = np.where(off, D - dmin[:, None], 0).astype(dtype)
    return dd, off.astype(dtype)


def _row_sums(dd, off, beta):
    E = np.exp(-beta[:, None] * dd) * off
    return E, E.sum(axis=1), (dd * E).sum(axis=1)


def search_beta(D, perplexity, dtype=np.float64, steps=SEARCH_STEPS):
    """precision of every row: `steps` steps of the bracketing bisection from beta = 1 (doubled / halved while one side is
    unbounded), on the row's distances less their minimum over j != i.  No early exit."""
    dd, off = _shifted(D, dtype)
    n = len(dd)
    target = dtype(np.log(perplexity))
    beta = np.ones(n, dtype)
    lo = np.full(n, -np.inf, dtype)
    hi = np.full(n, np.inf, dtype)
    two = dtype(2)
    for _ in range(steps):
        _, S, SD = _row_sums(dd, off, beta)
        H = np.log(S) + beta * SD / S
        up = H > target
        lo = np.where(up, beta, lo)
        hi = np.where(up, hi, beta)
        beta = np.where(up, np.where(np.isinf(hi), beta * two, (beta + hi) / two),
                        np.where(np.isinf(lo), beta / two, (beta + lo) / two)).astype(dtype)
    return beta


def conditional_rows(D, beta, dtype=np.float64):
    """p(j|i) [N x N], zero diagonal, rows sum to 1"""
    dd, off = _shifted(D, dtype)
    E, S, _ = _row_sums(dd, off, np.asarray(beta).astype(dtype))
    return (E / S[:, None]).astype(dtype)


def row_perplexity(D, beta):
    """achieved perplexity of every row at the given precisions, in float64"""
    dd, off = _shifted(D, np.float64)
    beta = np.asarray(beta).astype(np.float64)
    _, S, SD = _row_sums(dd, off, beta)
    return np.exp(np.log(S) + beta * SD / S)


def joint(C, dtype=np.float64):
    C = np.asarray(C).astype(dtype)
    return ((C + C.T) / dtype(2 * len(C))).astype(dtype)


def affinities(X, perplexity, dtype=np.float64, steps=SEARCH_STEPS):
    """X -> (P, beta, D)"""
    D = sq_distances(X, dtype)
    beta = search_beta(D, perplexity, dtype, steps)
    return joint(conditional_rows(D, beta, dtype), dtype), beta, D


def forces(P, Y, exaggeration=1.0, dtype=np.float64, want_kl=True):
    """-> (grad [N x 2], Z, KL or None, A, R): w_ij = 1 / (1 + |y_i - y_j|^2), A = exag sum_j p w (y_i - y_j),
    R = sum_j w^2 (y_i - y_j), Z = sum_{k != l} w_kl, grad = 4 (A - R / Z), KL = sum_{p > 0} p log(p Z / w) (P as given)."""
    P = np.asarray(P).astype(dtype)
    Y = np.asarray(Y).astype(dtype)
    dx = Y[:, 0][:, None] - Y[:, 0][None, :]
    dy = Y[:, 1][:, None] - Y[:, 1][None, :]
    q = dtype(1) + (dx * dx + dy * dy)
    w = dtype(1) / q
    pw = P * w
    w2 = w * w
    A = dtype(exaggeration) * np.stack(((pw * dx).sum(axis=1), (pw * dy).sum(axis=1)), axis=1)
    R = np.stack(((w2 * dx).sum(axis=1), (w2 * dy).sum(axis=1)), axis=1)
    wz = w.copy()
    np.fill_diagonal(wz, 0)
    Z = wz.sum()
    grad = (dtype(4) * (A - R / Z)).astype(dtype)
    kl = None
    if want_kl:
        pos = P > 0
        kl = (P[pos] * np.log(P[pos] * q[pos])).sum() + np.log(Z) * P.sum()
    return grad, Z, kl, A, R


def update(Y, velocity, gains, grad, momentum, lr, dtype=np.float64):
    """scikit-learn's step plus the re-centring -> (Y, velocity, gains)"""
    Y, velocity, gains, grad = (np.asarray(a).astype(dtype) for a in (Y, velocity, gains, grad))
    inc = velocity * grad < 0
    gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01)).astype(dtype)
    velocity = (dtype(momentum) * velocity - dtype(lr) * gains * grad).astype(dtype)
    Y = Y + velocity
    Y = (Y - Y.mean(axis=0)).astype(dtype)
    return Y, velocity, gains


def learning_rate(n, early_exaggeration=12.0):
    return max(n / early_exaggeration / 4.0, 50.0)


def run(P, Y0, n_iter, exaggerated_iters, early_exaggeration=12.0, lr=None, dtype=np.float64):
    """the whole descent from the init Y0 -> (Y, KL at Y with the un-exaggerated P)"""
    P = np.asarray(P).astype(dtype)
    Y = np.asarray(Y0).astype(dtype)
    lr = learning_rate(len(Y), early_exaggeration) if lr is None else lr
    velocity = np.zeros_like(Y)
    gains = np.ones_like(Y)
    for it in range(n_iter):
        early = it < exaggerated_iters
        grad = forces(P, Y, early_exaggeration if early else 1.0, dtype, want_kl=False)[0]
        Y, velocity, gains = update(Y, velocity, gains, grad, 0.5 if early else 0.8, lr, dtype)
    return Y, float(forces(P, Y, 1.0, dtype)[2])


def neighbour_purity(Y, labels, k=10):
    """fraction of points whose k nearest neighbours in the embedding all carry the point's own label"""
    Y = np.asarray(Y, np.float64)
    D = sq_distances(Y)
    np.fill_diagonal(D, np.inf)
    nn = np.argsort(D, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).all(axis=1).mean())
