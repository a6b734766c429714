"""numpy restatement of what csrc/evae_nn_rank.hip and evae.tsne.trustworthiness / continuity / embedding_quality compute
(DESIGN 3.7b): the rank of chosen columns within a row of distances, the order being (value ascending, index ascending), and the
three scores that are sums of those ranks.  Integers throughout; the scores are the integers through scikit-learn's expression in
float64.  tests/test_nn_rank_ref_host.py holds this file to sklearn.manifold.trustworthiness."""
import numpy as np


def ranks(D, nbr):
    """D [N x N] distances (any dtype that orders), nbr [N x k] columns -> rank int64 [N x k]:
    rank[i][m] = 1 + #{ l != i : (D[i][l], l) < (D[i][j], j) }, j = nbr[i][m]; the point itself is left out by index, so its exact
    duplicates count; an entry j == i or outside [0, N) gets rank 0."""
    D, nbr = np.asarray(D), np.asarray(nbr, dtype=np.int64)
    n = len(D)
    cols = np.arange(n)
    out = np.zeros(nbr.shape, np.int64)
    for i in range(n):
        others = cols[cols != i]
        order = others[np.lexsort((others, D[i, others]))]     # by value, then by index
        place = np.zeros(n, np.int64)                          # 1-based place of every other point; 0 for the point itself
        place[order] = np.arange(1, n)
        ok = (nbr[i] >= 0) & (nbr[i] < n)
        out[i, ok] = place[nbr[i, ok]]
    return out


def row_sums(rank, k=None):
    """-> int64 [N x 2]: (sum of max(0, rank - k) over the entries with rank > 0, the number of entries with 1 <= rank <= k)"""
    rank = np.asarray(rank, dtype=np.int64)
    k = rank.shape[1] if k is None else k
    penalty = np.where(rank > 0, np.maximum(rank - k, 0), 0).sum(axis=1)
    hits = ((rank >= 1) & (rank <= k)).sum(axis=1)
    return np.stack((penalty, hits), axis=1)


def neighbours(D, k):
    """the k nearest other points of every row, nearest first, by (value, index): int64 [N x k]"""
    D = np.array(D)
    n = len(D)
    D[np.arange(n), np.arange(n)] = np.inf
    cols = np.broadcast_to(np.arange(n), D.shape)
    return np.lexsort((cols, D), axis=1)[:, :k].astype(np.int64)


def score(penalty, n, k):
    """scikit-learn's expression, in its order"""
    return 1.0 - int(penalty) * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def trustworthiness(DX, DY, k):
    """DX, DY: the distance matrices of the input space and of the embedding"""
    return score(row_sums(ranks(DX, neighbours(DY, k)))[:, 0].sum(), len(DX), k)


def continuity(DX, DY, k):
    return trustworthiness(DY, DX, k)


def neighbourhood_preservation(DX, DY, k):
    return int(row_sums(ranks(DX, neighbours(DY, k)))[:, 1].sum()) / (len(DX) * k)


def label_accuracy(nbr, labels):
    """leave-one-out majority vote of the neighbours' labels, ties to the lowest class"""
    labels = np.asarray(labels)
    classes = np.unique(labels)
    right = 0
    for i in range(len(nbr)):
        votes = [(labels[nbr[i]] == c).sum() for c in classes]
        right += classes[int(np.argmax(votes))] == labels[i]    # np.argmax: the first of equal counts = the lowest class
    return int(right) / len(nbr)


def embedding_quality(DX, DY, k, labels=None):
    out = dict(trustworthiness=trustworthiness(DX, DY, k), continuity=continuity(DX, DY, k),
               neighbourhood_preservation=neighbourhood_preservation(DX, DY, k), n_neighbors=k, n_samples=len(DX))
    if labels is not None:
        out['label_accuracy'] = label_accuracy(neighbours(DY, k), labels)
    return out
