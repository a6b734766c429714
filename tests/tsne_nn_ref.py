"""numpy restatement of the t-SNE on sparse affinities that csrc/evae_tsne_nn.hip computes: P only on each point's
k = min(N - 1, floor(3 perplexity) + 1) nearest neighbours, symmetrised; everything after P -- forces, update, the whole run -- is
tests/tsne_ref.py on the densified matrix.  Every function takes a `dtype`, as there: float64 is the reference, the same
formulas in float32 the yardstick of what float32 costs at a case.  tests/test_tsne_nn_ref_host.py holds this file to
scikit-learn's private _joint_probabilities_nn."""
import numpy as np

import tsne_ref as ref
from tsne_ref import SEARCH_STEPS, blobs, forces, neighbour_purity, run, update  # noqa: F401  (reused as they are)


def n_neighbours(n, perplexity):
    """scikit-learn's n_neighbors"""
    return min(n - 1, int(3.0 * perplexity + 1))


def distances(X):
    """[N x N] squared distances by direct differences, accumulated in float64 and rounded once to float32 (the project's)"""
    return ref.sq_distances(X, np.float64).astype(np.float32)


def neighbours(X, k, D=None):
    """-> (idx int64 [N x k], d2 float32 [N x k]): the k nearest other points, nearest first, ordered by (value, index); the
    point itself is removed by index, so its exact duplicates stay.  D: the float32 distances to use (default distances(X))."""
    D = np.array(distances(X) if D is None else D, dtype=np.float32)
    n = len(D)
    D[np.arange(n), np.arange(n)] = np.inf
    cols = np.broadcast_to(np.arange(n), D.shape)
    order = np.lexsort((cols, D), axis=1)[:, :k]
    return order.astype(np.int64), np.take_along_axis(D, order, axis=1)


def _sums(dd, beta):
    E = np.exp(-beta[:, None] * dd)
    return E, E.sum(axis=1), (dd * E).sum(axis=1)


def _shifted(d2, dtype):
    d2 = np.asarray(d2).astype(dtype)
    return (d2 - d2.min(axis=1)[:, None]).astype(dtype)


def search_beta(d2, perplexity, dtype=np.float64, steps=SEARCH_STEPS):
    """tsne_ref.search_beta over the k columns of d2 [N x k]: fixed length, doubling / halving while one side is unbounded"""
    dd = _shifted(d2, dtype)
    n = len(dd)
    target = dtype(np.log(perplexity))
    beta = np.ones(n, dtype)
    lo = np.full(n, -np.inf, dtype)
    hi = np.full(n, np.inf, dtype)
    two = dtype(2)
    for _ in range(steps):
        _, S, SD = _sums(dd, beta)
        H = np.log(S) + beta * SD / S
        up = H > target
        lo = np.where(up, beta, lo)
        hi = np.where(up, hi, beta)
        beta = np.where(up, np.where(np.isinf(hi), beta * two, (beta + hi) / two),
                        np.where(np.isinf(lo), beta / two, (beta + lo) / two)).astype(dtype)
    return beta


def conditional_rows(d2, beta, dtype=np.float64):
    """p(j|i) on the k neighbours [N x k], rows sum to 1"""
    E, S, _ = _sums(_shifted(d2, dtype), np.asarray(beta).astype(dtype))
    return (E / S[:, None]).astype(dtype)


def row_perplexity(d2, beta):
    """achieved perplexity of every row over its k neighbours, in float64"""
    dd = _shifted(d2, np.float64)
    beta = np.asarray(beta).astype(np.float64)
    _, S, SD = _sums(dd, beta)
    return np.exp(np.log(S) + beta * SD / S)


def joint_dense(idx, cond, dtype=np.float64):
    """(p(j|i) + p(i|j)) / 2N as a dense [N x N] matrix, a conditional outside its row's neighbours being 0"""
    n, k = idx.shape
    C = np.zeros((n, n), dtype)
    C[np.repeat(np.arange(n), k), idx.ravel()] = np.asarray(cond).astype(dtype).ravel()
    return ((C + C.T) / dtype(2 * n)).astype(dtype)


def pattern(idx):
    """bool [N x N]: the non-zero pattern of the joint (an edge or its reverse), whatever the values underflow to"""
    n, k = idx.shape
    M = np.zeros((n, n), bool)
    M[np.repeat(np.arange(n), k), idx.ravel()] = True
    return M | M.T


def joint_csr(idx, cond, dtype=np.float64):
    """-> (row_ptr [N + 1], col [nnz], val [nnz]), columns ascending within a row"""
    P, M = joint_dense(idx, cond, dtype), pattern(idx)
    rows, cols = np.nonzero(M)
    row_ptr = np.concatenate(([0], np.cumsum(M.sum(axis=1))))
    return row_ptr.astype(np.int64), cols.astype(np.int64), P[rows, cols]


def densify(row_ptr, col, val, dtype=np.float64):
    n = len(row_ptr) - 1
    P = np.zeros((n, n), dtype)
    P[np.repeat(np.arange(n), np.diff(row_ptr)), col] = val
    return P


def affinities(X, perplexity, dtype=np.float64, steps=SEARCH_STEPS, D=None):
    """X -> dict(k, idx, d2, beta, cond, P): P the densified joint"""
    k = n_neighbours(len(X), perplexity)
    idx, d2 = neighbours(X, k, D)
    beta = search_beta(d2, perplexity, dtype, steps)
    cond = conditional_rows(d2, beta, dtype)
    return dict(k=k, idx=idx, d2=d2, beta=beta, cond=cond, P=joint_dense(idx, cond, dtype))
