"""numpy restatement of what csrc/evae_ball_count.hip and evae.sample_quality compute: k-th neighbour radii, ball
counts, nearest columns, and precision / recall / density / coverage / authenticity as sums of them.  Everything starts from
distance matrices and is an integer until one float64 expression, written in the order the `prdc` package writes it.  Every
inequality is strict.  tests/test_sample_quality_ref_host.py holds this file to an independent formulation on scikit-learn's
distances."""
import numpy as np


def radii(DXX, k):
    """DXX [N x N] distances within one set -> [N]: the distance from row i to its k-th nearest OTHER row.  The row itself is
    left out by index, so its exact duplicates stay eligible and a radius can be 0."""
    D = np.array(DXX)
    n = len(D)
    assert D.shape == (n, n) and 1 <= k <= n - 1
    out = np.empty(n, D.dtype)
    for i in range(n):
        out[i] = np.sort(np.delete(D[i], i))[k - 1]
    return out


def ball_counts(D, col_radius=None, row_radius=None):
    """D [B x N] -> (col_hits int64 [B] or None, row_hits int64 [B] or None):
    col_hits[i] = #{ j : D[i][j] < col_radius[j] }, row_hits[i] = #{ j : D[i][j] < row_radius[i] }"""
    D = np.asarray(D)
    col = None if col_radius is None else (D < np.asarray(col_radius)[None, :]).sum(axis=1).astype(np.int64)
    row = None if row_radius is None else (D < np.asarray(row_radius)[:, None]).sum(axis=1).astype(np.int64)
    return col, row


def nearest(D):
    """D [B x N] -> (idx int64 [B], d2 [B]): the column minimising (D[i][j], j) lexicographically"""
    D = np.asarray(D)
    idx = np.empty(len(D), np.int64)
    for i in range(len(D)):
        idx[i] = min(range(D.shape[1]), key=lambda j: (D[i, j], j))
    return idx, D[np.arange(len(D)), idx]


def prdc(DRR, DFF, DRF, k):
    """DRR [N x N] real to real, DFF [M x M] generated to generated, DRF [N x M] real to generated -> the dict of
    evae.sample_quality.compute_prdc"""
    DRF = np.asarray(DRF)
    n, m = DRF.shape
    rho_r, rho_f = radii(DRR, k), radii(DFF, k)
    in_real = ball_counts(DRF.T, col_radius=rho_r)[0]                   # per generated row: the real balls it lies in
    in_fake, own = ball_counts(DRF, col_radius=rho_f, row_radius=rho_r)  # per real row: generated balls it lies in; its own ball's content
    return dict(precision=int((in_real > 0).sum()) / m, recall=int((in_fake > 0).sum()) / n,
                density=(1.0 / k) * (int(in_real.sum()) / m), coverage=int((own > 0).sum()) / n, nearest_k=k, n_real=n, n_fake=m)


def authentic_count(DTT, DTF):
    """DTT [N x N] within the training set, DTF [N x M] training to generated -> #{ j : D(T_i*, F_j) >= rho_1(T)[i*] }"""
    idx, d2 = nearest(np.asarray(DTF).T)
    return int((d2 >= radii(DTT, 1)[idx]).sum())


def authenticity(DTT, DTF):
    return authentic_count(DTT, DTF) / np.asarray(DTF).shape[1]


def nearest_distance_median(DTF):
    """the (lower) median of the float32 square roots of every generated row's squared distance to its nearest training row"""
    d = np.sort(np.sqrt(nearest(np.asarray(DTF, np.float32).T)[1]))
    return float(d[(len(d) - 1) // 2])


def sample_quality(DRR, DFF, DRF, k, DTT=None, DTF=None):
    """-> the dict of evae.sample_quality.sample_quality; authenticity against the training set when its matrices are given"""
    out = prdc(DRR, DFF, DRF, k)
    DTT, DTF = (DRR, DRF) if DTT is None else (DTT, DTF)
    out['authenticity'] = authenticity(DTT, DTF)
    out['nearest_distance_median'] = nearest_distance_median(DTF)
    return out
