"""numpy float64 restatement of what csrc/evae_kmeans.hip computes: the yardstick of tests/test_gpu_kmeans.py, held
to scikit-learn by tests/test_kmeans_ref_host.py.  Not product code.  Every function that takes a decision -- an argmin, a
seeding pick, a stop on the shift -- also returns its margin: how far the reference itself was from deciding otherwise.  A GPU
test may compare labels, picks and iteration counts exactly only where those margins are far above fp64 rounding."""
import functools
import math

import numpy as np

from tsne_ref import blobs

EPS = 2.0 ** -52
CHUNK = 512           # ops.kmeans_chunk_rows(): the running sums of the seeding go chunk by chunk (test_gpu_kmeans.py asserts it)
TILE = 32             # ops.kmeans_centre_tile()

# (n, d, K, seed): inputs are blobs(n, d, min(K, 10), seed), uniforms RandomState(1000 + seed).  The last rows straddle CHUNK
# and TILE in N and K.
CASES = [(2, 1, 2, 0), (65, 3, 4, 1), (1025, 40, 10, 2), (2049, 40, 37, 3), (513, 256, 7, 4), (3000, 40, 257, 5), (1500, 2, 64, 6),
         (1100, 3, 1024, 7), (1023, 40, 31, 8), (1024, 40, 32, 9), (2049, 65, 33, 10), (1025, 1, 5, 11), (1025, 255, 10, 12),
         (3, 2, 1, 13), (1025, 63, 64, 14), (511, 40, 31, 0), (512, 40, 32, 1), (513, 40, 33, 2)]


def case_input(n, d, K, seed):
    """-> (X float32 [n x d], blob labels [n], uniforms float64 [K])"""
    X, y = blobs(n, d, min(K, 10), seed)
    return X, y, np.random.RandomState(1000 + seed).random_sample(K)


def sq_distances(X, C):
    """[N x K] by direct differences in float64, features ascending"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    out = np.zeros((len(X), len(C)))
    for k in range(X.shape[1]):
        df = X[:, k][:, None] - C[:, k][None, :]
        out += df * df
    return out


def assign(X, C):
    """-> (labels [N] -- the lowest index among equal minima --, d2 [N], margin): margin = the smallest (second - best) / second
    over the rows (inf for one centre, 0 where two centres tie)"""
    D = sq_distances(X, C)
    labels = np.argmin(D, axis=1)
    d2 = D[np.arange(len(D)), labels]
    if D.shape[1] < 2:
        return labels, d2, np.inf
    two = np.partition(D, 1, axis=1)[:, :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
    return labels, d2, float(gap.min())


def cluster_sums(X, labels, K):
    """-> (sums [K x d], counts [K]); every column by numpy's pairwise summation (the reduction runs along the contiguous axis),
    so the yardstick's own rounding grows with log n, not n"""
    X = np.asarray(X, np.float64)
    sums = np.zeros((K, X.shape[1]))
    for c in np.unique(labels):
        if 0 <= c < K:
            sums[c] = np.ascontiguousarray(X[labels == c].T).sum(axis=1)
    return sums, np.bincount(labels[(labels >= 0) & (labels < K)], minlength=K)


def lloyd(X, C0, tol_abs=0.0, max_iter=300):
    """scikit-learn's Lloyd iteration without weights -> dict(centres, labels, inertia, n_iter, relocations, argmin_margin,
    shift_margin).  An empty cluster, in ascending index, takes the point of largest d2 of the iteration (lowest index on a
    tie) that no earlier one took and whose cluster keeps a member; the point leaves its donor's sum.  Stops when no label
    changed against the previous iteration (never in the first) or sum |c_new - c_old|^2 <= tol_abs.  labels and inertia come
    from one closing assignment to the final centres."""
    X64 = np.asarray(X, np.float64)
    C = np.array(C0, np.float64)
    K = len(C)
    prev, argmin_margin, shift_margin, relocations, n_iter = None, np.inf, np.inf, 0, 0
    for n_iter in range(1, max_iter + 1):
        labels, d2, m = assign(X64, C)
        argmin_margin = min(argmin_margin, m)
        sums, counts = cluster_sums(X64, labels, K)
        taken = []
        for e in range(K):
            if counts[e] != 0:
                continue
            cand = np.where(counts[labels] >= 2, d2, -1.0)
            cand[taken] = -1.0
            if cand.max() < 0:
                continue
            i = int(np.argmax(cand))
            sums[labels[i]] -= X64[i]
            counts[labels[i]] -= 1
            sums[e], counts[e] = X64[i], 1
            taken.append(i)
        relocations += len(taken)
        new = C.copy()
        full = counts > 0
        new[full] = sums[full] / counts[full][:, None]
        shift = float(((new - C) ** 2).sum())
        C = new
        if tol_abs > 0:
            shift_margin = min(shift_margin, abs(shift - tol_abs) / tol_abs)
        done = (prev is not None and np.array_equal(labels, prev)) or shift <= tol_abs
        prev = labels
        if done:
            break
    labels, d2, m = assign(X64, C)
    return dict(centres=C, labels=labels, inertia=float(d2.sum()), n_iter=n_iter, relocations=relocations,
                argmin_margin=min(argmin_margin, m), shift_margin=shift_margin)


def seed(X, K, u, chunk=CHUNK):
    """k-means++ by D^2 sampling from the uniforms u [K] -> (idx [K], centres [K x d], margin).  The first index is
    min(floor(u_0 N), N - 1); then d2min = min(d2min, distance to the last pick), and the pick is the first i whose inclusive
    running sum -- the chunks before i's in order plus the rows of its chunk in order -- exceeds u_t x total (N - 1 if none
    does); total == 0 picks the lowest index not chosen yet.  margin = the smallest |u_t total - nearest running sum| / total."""
    X64 = np.asarray(X, np.float64)
    N = len(X64)
    idx = [min(int(np.floor(u[0] * N)), N - 1)]
    d2min, margin = None, np.inf
    for t in range(1, K):
        d = sq_distances(X64, X64[idx[-1]][None, :])[:, 0]
        d2min = d if d2min is None else np.minimum(d2min, d)
        running, base = np.empty(N), 0.0
        for c0 in range(0, N, chunk):
            part = np.cumsum(d2min[c0:c0 + chunk])
            running[c0:c0 + chunk] = base + part
            base = base + part[-1]
        total = base
        if total > 0:
            target = u[t] * total
            above = np.nonzero(running > target)[0]
            idx.append(int(above[0]) if len(above) else N - 1)
            margin = min(margin, float(np.abs(np.concatenate(([0.0], running)) - target).min() / total))
        else:
            idx.append(min(set(range(t + 1)) - set(idx)))
    idx = np.array(idx)
    return idx, X64[idx].copy(), margin


def contingency(a, Ka, b, Kb):
    table = np.zeros((Ka, Kb), np.int64)
    np.add.at(table, (np.asarray(a), np.asarray(b)), 1)
    return table


def scores(table):
    """-> dict(entropy_a, entropy_b, mutual_info, nmi, ari, purity): natural logarithms; NMI with the arithmetic mean; the ARI
    from exact integer pair counts (Python integers, one division); one non-empty row and column give nmi = ari = 1"""
    T = np.asarray(table, np.int64)
    n = int(T.sum())
    a, b = T.sum(axis=1), T.sum(axis=0)
    ha = math.fsum((int(v) / n) * math.log(n / int(v)) for v in a if v > 0)             # fsum: the terms' sum without rounding
    hb = math.fsum((int(v) / n) * math.log(n / int(v)) for v in b if v > 0)
    ii, jj = np.nonzero(T)
    mi = math.fsum((int(T[i, j]) / n) * math.log((int(T[i, j]) * n) / (int(a[i]) * int(b[j]))) for i, j in zip(ii, jj))
    mi = max(mi, 0.0)
    if (a > 0).sum() == 1 and (b > 0).sum() == 1:
        nmi = 1.0
    elif mi == 0.0:
        nmi = 0.0
    else:
        nmi = mi / (0.5 * (ha + hb))
    ss = int(sum(int(v) ** 2 for v in T.ravel()))
    tp, fp, fn = ss - n, int(sum(int(v) ** 2 for v in b)) - ss, int(sum(int(v) ** 2 for v in a)) - ss
    tn = n * n - fp - fn - ss
    ari = 1.0 if fn == 0 and fp == 0 else 2 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    return dict(entropy_a=ha, entropy_b=hb, mutual_info=mi, nmi=nmi, ari=float(ari), purity=int(T.max(axis=0).sum()) / n,
                nonzero=len(ii))


def silhouette_samples(X, labels):
    """[N] float64 by direct float64 differences: a = mean distance to the rest of the own cluster, b = the smallest mean
    distance to another cluster, (b - a) / max(a, b); 0 for a singleton and for max(a, b) = 0"""
    X64 = np.asarray(X, np.float64)
    labels = np.asarray(labels)
    D = np.sqrt(sq_distances(X64, X64))
    classes = np.unique(labels)
    means = np.stack([D[:, labels == c].sum(axis=1) for c in classes], axis=1)          # sums first
    counts = np.array([(labels == c).sum() for c in classes])
    own = np.searchsorted(classes, labels)
    rows = np.arange(len(X64))
    a_sum, n_own = means[rows, own], counts[own]
    other = means / counts[None, :]
    other[rows, own] = np.inf
    b = other.min(axis=1)
    out = np.zeros(len(X64))
    ok = n_own > 1
    a = np.where(ok, a_sum / np.maximum(n_own - 1, 1), 0.0)
    m = np.maximum(a, b)
    good = ok & (m > 0) & np.isfinite(b)
    out[good] = (b[good] - a[good]) / m[good]
    return out


@functools.lru_cache(maxsize=None)
def solved(n, d, K, seed_):
    """a row of CASES, seeded from its uniforms and run to convergence at tol = 0: computed once, shared, never written to"""
    X, y, u = case_input(n, d, K, seed_)
    idx, C0, seed_margin = seed(X, K, u)
    return dict(X=X, y=y, u=u, idx=idx, C0=C0, seed_margin=seed_margin, fit=lloyd(X, C0))


TOL_CASE, TOL = CASES[3], 0.1       # a run that the shift stops at iteration 9; its labels settle at 18


def tol_abs(X, tol):
    """scikit-learn's _tolerance: tol x the mean population variance of the features"""
    return tol * float(np.asarray(X, np.float64).var(axis=0).mean())


@functools.lru_cache(maxsize=None)
def solved_with_tol():
    s = solved(*TOL_CASE)
    return lloyd(s["X"], s["C0"], tol_abs=tol_abs(s["X"], TOL))


RELOCATION_CASE = CASES[2]


@functools.lru_cache(maxsize=None)
def solved_with_relocations(how_many):
    s = solved(*RELOCATION_CASE)
    C0 = far_centres(s["X"], s["C0"], how_many)
    return C0, lloyd(s["X"], C0)


def far_centres(X, C, how_many):
    """C with its last `how_many` rows moved far from every point: they start empty and are relocated"""
    C = np.array(C, np.float64)
    for r in range(how_many):
        C[len(C) - 1 - r] = np.abs(np.asarray(X, np.float64)).max() * (100.0 + 10.0 * r)
    return C
