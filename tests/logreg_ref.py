"""numpy restatement of what csrc/evae_logreg.hip and evae/linear.py compute: the yardstick of
tests/test_gpu_logreg.py, held to scikit-learn by tests/test_logreg_ref_host.py.  Not product code.

Multinomial (softmax) regression with an L2 penalty, always K >= 2 rows of coefficients.  With a_n = (x_n, 1), p = d + 1
(p = d without an intercept) and lambda = 1 / C:

    f(W) = sum_n [ lse_k(a_n . w_k) - a_n . w_{y_n} ] + (lambda / 2) sum_k sum_{c<d} W_kc^2

L-BFGS from W = 0 with `history` pairs, scaling s.y / y.y of the newest pair (1 / max|G| before any), a pair with s.y <= 0
skipped; Armijo (c1 = 1e-4) over t = 2^-j, j < line_steps, the first j that passes; trial logits Z + t Z_D with Z_D = A D^T, the
penalty at W + t D the exact quadratic; after the pick W += t D and Z += t Z_D (the same axpy the kernels do: Z is never
recomputed from W).  Stop: max|G| / N <= tol.

A fit also returns how far the restatement itself was from deciding otherwise -- per iteration the smallest Armijo margin over
the trials looked at and the stop's margin -- so a GPU test may compare n_iter, converged and the chosen steps exactly only
where those are far above fp64 rounding.  fit(..., dt=numpy.longdouble, replay=...) takes the decisions of an earlier run and
redoes its arithmetic in a wider format: the difference of the two is the rounding spread of the float64 run.  Where the platform
has no wider format (numpy.longdouble is float64), fit(..., replay=..., exact=True) redoes it with every sum, dot and matrix
product EXACT -- the products split without error (Dekker), the terms added as rationals by math.fsum, one rounding of the
result -- which is what a wider format buys for them; exp, log and the divisions stay float64's, they have no rational value."""
import functools
import math

import numpy as np

EPS = 2.0 ** -52
CHUNK = 1024          # ops.logreg_chunk_rows(): rows whose losses and gradient sums are formed together
C1 = 1e-4
TOL, MAX_ITER, HISTORY, LINE_STEPS = 1e-4, 100, 10, 12

# (n, d, K, seed, separation, fit_intercept, C).  n straddles CHUNK, d and K are odd and even, one case has no intercept, one is
# binary (two rows of coefficients), one has more classes than features, and two classes of n700_d3_K17 overlap enough that
# the search halves its step (tests/test_logreg_ref_host.py asserts the coverage and the margins).
CASES = [(300, 5, 3, 0, 1.5, True, 1.0), (1025, 40, 10, 1, 0.6, True, 1.0), (700, 3, 17, 2, 1.0, True, 1.0),
         (2049, 16, 2, 3, 0.5, True, 1.0), (1023, 8, 5, 4, 1.0, False, 0.5), (1500, 24, 33, 5, 0.4, True, 10.0)]

# 10 x the largest figures tests/test_logreg_ref_host.py measures over the table (it prints them and asserts that what it
# measures stays within these): `sklearn_excess` is (f(restatement at tol 1e-8) - f(scikit-learn 1.7.2 at tol 1e-10)) / |f|; the
# others are the relative differences (largest difference over largest magnitude) between the float64 run at the default tol
# and its replay in numpy.longdouble.
SPREAD = dict(sklearn_excess=1.8e-11, coef=2.1e-13, loss=1.2e-15, direction=8.3e-11)


def case_id(row):
    return "n%d_d%d_K%d%s" % (row[0], row[1], row[2], "" if row[5] else "_nointercept")


def rel_err(got, want):
    got, want = np.asarray(got, np.longdouble), np.asarray(want, np.longdouble)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def blobs(n, d, K, seed, sep):
    """-> (X float32 [n x d], y int32 [n]): class-conditional unit Gaussians, centres drawn at `sep` of the within-class scale"""
    rs = np.random.RandomState(seed)
    centres = sep * rs.standard_normal((K, d))
    y = np.arange(n) % K
    rs.shuffle(y)
    X = centres[y] + rs.standard_normal((n, d))
    return X.astype(np.float32), y.astype(np.int32)


def design(X, fit_intercept, dt=np.float64):
    """-> A [n x p]: the rows, with a column of ones last when there is an intercept"""
    X = np.asarray(X, dt)
    return np.concatenate([X, np.ones((X.shape[0], 1), dt)], axis=1) if fit_intercept else X


_EXACT = False       # set by fit(exact=True) for its duration: total and mm below round once


def _two_prod(a, b):
    """float64 a, b -> (p, e) with p + e == a b exactly (Veltkamp's split, Dekker's product; no overflow at these magnitudes)"""
    p = a * b
    ca, cb = a * 134217729.0, b * 134217729.0
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def total(v, axis=None):
    """v.sum(axis); exact and rounded once under fit(exact=True)"""
    if not _EXACT:
        return v.sum(axis=axis)
    if axis is None:
        return np.float64(math.fsum(v.reshape(-1).tolist()))
    w = np.moveaxis(v, axis, -1)
    return np.array([math.fsum(r) for r in w.reshape(-1, w.shape[-1]).tolist()]).reshape(w.shape[:-1])


def dot(a, b):
    """(a * b).sum(); exact and rounded once under fit(exact=True)"""
    if not _EXACT:
        return (a * b).sum()
    p, e = _two_prod(a.reshape(-1), b.reshape(-1))
    return np.float64(math.fsum(p.tolist() + e.tolist()))


def mm(A, B):
    """A @ B; every entry exact and rounded once under fit(exact=True)"""
    if not _EXACT:
        return A @ B
    p, e = _two_prod(A[:, None, :], B.T[None, :, :])               # [n x K x c] each
    terms = np.concatenate([p, e], axis=2)
    return np.array([math.fsum(r) for r in terms.reshape(-1, terms.shape[2]).tolist()]).reshape(A.shape[0], B.shape[1])


def row_losses(Z, y):
    """lse_k z_nk - z_{n y_n}: the row maximum subtracted, the exponentials added in class order"""
    m = Z.max(axis=1)
    return (m + np.log(total(np.exp(Z - m[:, None]), 1))) - Z[np.arange(Z.shape[0]), y]


def in_chunks(v):
    """the sum of v [n] (or of every column of v [n x T]): per chunk of CHUNK rows, then the chunks in chunk order"""
    acc = np.zeros(v.shape[1:], v.dtype)
    for c0 in range(0, v.shape[0], CHUNK):
        acc = acc + total(v[c0:c0 + CHUNK], 0)
    return acc


def penalty(W, d, lam):
    return 0.5 * lam * dot(W[:, :d], W[:, :d])


def residual(Z, y):
    """softmax(Z) - onehot(y)"""
    E = np.exp(Z - Z.max(axis=1)[:, None])
    R = E / total(E, 1)[:, None]
    R[np.arange(Z.shape[0]), y] -= 1
    return R


def gradient(A, Z, y, W, d, lam):
    """[K x p]: sum_n R_nk a_nc per chunk, the chunks in chunk order, + lam W on the penalised columns"""
    R = residual(Z, y)
    G = np.zeros(W.shape, Z.dtype)
    for c0 in range(0, A.shape[0], CHUNK):
        G = G + mm(R[c0:c0 + CHUNK].T, A[c0:c0 + CHUNK])
    G[:, :d] += lam * W[:, :d]
    return G


def objective(X, y, W, C, fit_intercept=True, dt=np.float64):
    """f(W) from scratch"""
    A, W = design(X, fit_intercept, dt), np.asarray(W, dt)
    return in_chunks(row_losses(A @ W.T, y)) + penalty(W, X.shape[1], dt(1) / dt(C))


def gradient_at(X, y, W, C, fit_intercept=True, dt=np.float64):
    """G(W) from scratch"""
    A, W = design(X, fit_intercept, dt), np.asarray(W, dt)
    return gradient(A, A @ W.T, y, W, X.shape[1], dt(1) / dt(C))


def direction(G, pairs):
    """-H G by the two-loop recursion; pairs: (s, y, s.y, y.y), oldest first"""
    q = G.copy()
    alphas = []
    for s, yv, sy, yy in reversed(pairs):
        a = dot(s, q) / sy
        alphas.append(a)
        q = q - a * yv
    if pairs:
        q = q * (pairs[-1][2] / pairs[-1][3])
    else:
        q = q * (1 / np.abs(G).max())
    for (s, yv, sy, yy), a in zip(pairs, reversed(alphas)):
        b = dot(yv, q) / sy
        q = q + (a - b) * s
    return -q


def line_trials(Z, ZD, y, W, D, d, lam, line_steps):
    """-> f(W + t_j D), j < line_steps, t_j = 2^-j: the trial logits Z + t Z_D, the penalty the exact quadratic"""
    dt = Z.dtype.type
    ww, wd, dd = dot(W[:, :d], W[:, :d]), dot(W[:, :d], D[:, :d]), dot(D[:, :d], D[:, :d])
    out = []
    for j in range(line_steps):
        t = dt(2.0) ** -j
        out.append(in_chunks(row_losses(Z + t * ZD, y)) + 0.5 * lam * ((ww + (2 * t) * wd) + (t * t) * dd))
    return np.array(out, Z.dtype)


def fit(X, y, K, C=1.0, tol=TOL, max_iter=MAX_ITER, fit_intercept=True, history=HISTORY, line_steps=LINE_STEPS, dt=np.float64,
        replay=None, exact=False):
    """-> dict(W [K x p], n_iter, converged, line_failed, loss, js, accepted, armijo_margin, stop_margin, directions, Z).
    replay = the dict of an earlier run: its js, accepted and n_iter are taken as decisions, no test is made.
    exact (float64, with a replay): every sum, dot and matrix product exact and rounded once."""
    global _EXACT
    if exact:
        assert replay is not None and dt is np.float64 and not _EXACT
        _EXACT = True
        try:
            return fit(X, y, K, C, tol, max_iter, fit_intercept, history, line_steps, dt, replay)
        finally:
            _EXACT = False
    n, d = X.shape
    A = design(X, fit_intercept, dt)
    lam = dt(1) / dt(C)
    W = np.zeros((K, A.shape[1]), dt)
    Z = mm(A, W.T)
    G = gradient(A, Z, y, W, d, lam)
    f = in_chunks(row_losses(Z, y)) + penalty(W, d, lam)
    pairs, js, accepted, armijo, stops, dirs = [], [], [], [], [], []
    converged = line_failed = False
    it = 0

    def stop():
        gn = np.abs(G).max() / n
        stops.append(float(abs(gn - tol) / tol))
        return bool(gn <= tol)

    converged = stop() if replay is None else replay['n_iter'] == 0
    limit = max_iter if replay is None else replay['n_iter']
    while not converged and it < limit:
        D = direction(G, pairs)
        dirs.append(D)
        gd = dot(G, D)
        ZD = mm(A, D.T)
        if replay is None:
            trials = line_trials(Z, ZD, y, W, D, d, lam, line_steps)
            ts = dt(2.0) ** -np.arange(line_steps)
            bound = f + (C1 * ts) * gd
            ok = np.nonzero(trials <= bound)[0]
            looked = line_steps if ok.size == 0 else int(ok[0]) + 1
            armijo.append(float((np.abs(trials[:looked] - bound[:looked]) / max(abs(f), 1.0)).min()))
            if ok.size == 0:
                line_failed = True
                break
            j = int(ok[0])
        else:
            j = replay['js'][it]
        t = dt(2.0) ** -j
        js.append(j)
        W = W + t * D
        Z = Z + t * ZD
        Gn = gradient(A, Z, y, W, d, lam)
        f = in_chunks(row_losses(Z, y)) + penalty(W, d, lam)
        s, yv = t * D, Gn - G
        sy, yy = dot(s, yv), dot(yv, yv)
        keep = bool(sy > 0) if replay is None else replay['accepted'][it]
        accepted.append(keep)
        if keep:
            pairs = (pairs + [(s, yv, sy, yy)])[-history:]
        G = Gn
        it += 1
        if replay is None:
            converged = stop()
    if replay is not None:
        converged = replay['converged']
    return dict(W=W, n_iter=it, converged=converged, line_failed=line_failed, loss=f, js=js, accepted=accepted,
                armijo_margin=armijo, stop_margin=stops, directions=dirs, Z=Z, G=G)


@functools.lru_cache(maxsize=None)
def solved(row, tol=TOL):
    """-> (X, y, the float64 fit of a row of the table): computed once, shared, not to be changed"""
    n, d, K, seed, sep, fit_intercept, C = row
    X, y = blobs(n, d, K, seed, sep)
    return X, y, fit(X, y, K, C=C, tol=tol, fit_intercept=fit_intercept)


def top_two_gap(Z):
    s = np.sort(np.asarray(Z, np.float64), axis=1)
    return s[:, -1] - s[:, -2]
