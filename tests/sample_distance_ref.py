"""numpy restatement of what csrc/evae_kernel_sum.hip and evae/sample_quality.py's distances compute, in
np.longdouble (a 64-bit mantissa on x86) with direct differences, returned as float64: its own error is 2^-11 of float64's.
Inputs are float32 arrays.

    POLY: k(x, y) = (gamma <x, y> + coef0)^degree        RBF: k(x, y) = exp(-gamma |x - y|^2)
    row_sum[i] = sum_j k(q_i, c_j)   (skip_self: without j == i)        total = sum_i row_sum[i]
    mmd2 (unbiased) = S_rr / (N (N - 1)) + S_ff / (M (M - 1)) - 2 S_rf / (N M), the within-set sums without their diagonal
    mmd2 (biased)   = S_rr / N^2 + S_ff / M^2 - 2 S_rf / (N M), the diagonals kept
    frechet = |mu_r - mu_f|^2 + tr S_r + tr S_f - 2 tr (S_r S_f)^(1/2), covariances with ddof 1

The moments are longdouble; the square root's trace is numpy.linalg.eigvalsh in float64 on matrices built in longdouble:
S_r = V diag(lambda) V^T, A = diag(sqrt lambda) V^T, C = A S_f A^T (longdouble products), tr = sum sqrt max(nu(C), 0).  Two equal
covariance matrices take the closed form (S S)^(1/2) = S, so that identical sets give exactly 0.

error_bounds_* are the tolerances the device is held to (and the second evaluations of tests/test_sample_distance_ref_host.py);
the derivations stand at the functions.  u = 2^-53."""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TILE = 32                  # evae_kernel_sum_tile(): the tests assert it
MAX_SWEEPS = 64            # evae_pca_max_sweeps(): the tests assert it
MEDIAN_ROWS = 2048

KID = dict(kind='poly', gamma=None, coef0=1.0, degree=3)


def parity_shapes(T=TILE):
    """(B, N, d) of the row-sum parity tests; with skip_self the columns are the B rows themselves"""
    return [(1, 1, 1), (3, T - 1, 2), (65, T, 7), (64, T + 1, 40), (257, 2 * T + 3, 40), (5, 3 * T, 256)]


_CASES = {}


def rows_case(B, N, d):
    """-> (q [B x d], c [N x d]) float32, uniform in (-0.9, 0.9): with KID's kernel every term lies in (0.19, 1.81), so a row
    sum is a sum of positive terms and 'relative to the value' means what it says.  Made once per shape, read-only."""
    key = (B, N, d)
    if key not in _CASES:
        rs = np.random.RandomState(B * 1000003 + N * 1009 + d)
        q = rs.uniform(-0.9, 0.9, size=(B, d)).astype(np.float32)
        c = rs.uniform(-0.9, 0.9, size=(N, d)).astype(np.float32)
        q.setflags(write=False)
        c.setflags(write=False)
        _CASES[key] = (q, c)
    return _CASES[key]


def gaussian_sets(N, M, d, seed=0, shift=0.3, scale=0.8, rank=None):
    """-> (real [N x d], fake [M x d]) float32: real ~ N(0, L L^T) with a random mixing L, fake a shifted and shrunk draw of the
    same; rank < d: the real set lies in a rank-dimensional subspace (its covariance is rank-deficient), the fake set is full"""
    key = ('g', N, M, d, seed, shift, scale, rank)
    if key not in _CASES:
        rs = np.random.RandomState(7919 * seed + 31 * N + 17 * M + d)
        L = 0.3 * rs.randn(d, d) / math.sqrt(d) + np.eye(d)        # well conditioned: the spectrum of C stands clear of 0
        real = rs.randn(N, d) @ L.T
        if rank is not None:
            basis = np.linalg.qr(rs.randn(d, rank))[0]
            real = rs.randn(N, rank) @ (basis * np.linspace(1.0, 2.0, rank)).T
        fake = scale * (rs.randn(M, d) @ L.T) + shift
        real, fake = real.astype(np.float32), fake.astype(np.float32)
        real.setflags(write=False)
        fake.setflags(write=False)
        _CASES[key] = (real, fake)
    return _CASES[key]


# the sets of the Frechet / MMD tests: name -> gaussian_sets arguments
SETS = {'small': dict(N=300, M=300, d=5), 'mid': dict(N=1024, M=700, d=40), 'wide': dict(N=400, M=400, d=97),
        'rank': dict(N=300, M=300, d=8, rank=3)}


def distance_case(name):
    """-> dict(real, fake: float32; frechet: frechet(); fb: error_bounds_frechet()), made once and never written to"""
    key = ('case', name)
    if key not in _CASES:
        real, fake = gaussian_sets(**SETS[name])
        fr = frechet(real, fake)
        _CASES[key] = dict(real=real, fake=fake, frechet=fr, fb=error_bounds_frechet(real, fake, fr))
    return _CASES[key]


def mmd_case(name, kind='poly', gamma=None, coef0=1.0, degree=3, biased=False):
    """kernel_mmd() of a named set, made once"""
    key = ('mmd', name, kind, gamma, coef0, degree, biased)
    if key not in _CASES:
        c = distance_case(name)
        _CASES[key] = kernel_mmd(c['real'], c['fake'], kind, gamma, coef0, degree, biased)
    return _CASES[key]


def _ld(a):
    return np.asarray(a, dtype=np.float32).astype(LD)


def _osum(a, axis=-1):
    """sum along an axis in ascending index, in longdouble"""
    return np.take(np.cumsum(a, axis=axis, dtype=LD), -1, axis=axis)


def _gamma(gamma, d):
    return 1.0 / d if gamma is None else float(gamma)


# ---------------------------------------------------------------------------------------------- kernel sums
def _dots(q, c):
    """[B x N] longdouble <q_i, c_j>, one feature after the other in ascending order (no [B x N x d] array)"""
    out = np.zeros((len(q), len(c)), LD)
    for k in range(q.shape[1]):
        out += q[:, k, None] * c[None, :, k]
    return out


def _sqdist(q, c):
    """[B x N] longdouble |q_i - c_j|^2 from direct differences, features ascending"""
    out = np.zeros((len(q), len(c)), LD)
    for k in range(q.shape[1]):
        df = q[:, k, None] - c[None, :, k]
        out += df * df
    return out


def kernel_matrix(q, c, kind='poly', gamma=None, coef0=1.0, degree=3):
    """[B x N] longdouble: every k(q_i, c_j); the features summed in ascending order, the RBF distance from direct differences"""
    q, c = _ld(q), _ld(c)
    g = LD(_gamma(gamma, q.shape[1]))
    if kind == 'poly':
        b = g * _dots(q, c) + LD(coef0)
        v = b.copy()
        for _ in range(int(degree) - 1):
            v = v * b
        return v
    if kind == 'rbf':
        return np.exp(-g * _sqdist(q, c))
    raise ValueError(kind)


def row_sums(q, c, kind='poly', gamma=None, coef0=1.0, degree=3, skip_self=False, as_ld=False):
    K = kernel_matrix(q, c, kind, gamma, coef0, degree)
    if skip_self:
        assert K.shape[0] == K.shape[1]
        K[np.arange(len(K)), np.arange(len(K))] = LD(0)
    s = _osum(K)
    return s if as_ld else s.astype(np.float64)


def total(q, c, kind='poly', gamma=None, coef0=1.0, degree=3, skip_self=False, as_ld=False):
    s = _osum(row_sums(q, c, kind, gamma, coef0, degree, skip_self, as_ld=True))
    return s if as_ld else float(s)


def diagonal_sum(x, kind='poly', gamma=None, coef0=1.0, degree=3):
    """sum_i k(x_i, x_i): what the biased within-set total has over the unbiased one"""
    x = _ld(x)
    g = LD(_gamma(gamma, x.shape[1]))
    if kind == 'poly':
        b = g * _osum(x * x) + LD(coef0)
        v = b.copy()
        for _ in range(int(degree) - 1):
            v = v * b
        return float(_osum(v))
    return float(len(x))


def error_bounds_rows(q, c, kind='poly', gamma=None, coef0=1.0, degree=3, skip_self=False, T=TILE):
    """-> (row bound [B], total bound): absolute, for any correct float64 evaluation whose sums add each term through at most
    N - 1 + ceil(N / T) additions.  q, c are fp32 values, exact in fp64, and so is every product q_k c_k (48 bits).

    * Dot product over d: (d + 1) u P, P = sum_k |q_k| |c_k| (d - 1 additions; the two spare roundings admit an evaluation that
      rounds its products).  b = gamma dot + coef0: the product and the addition, 2 u Bm with Bm = |gamma| P + |coef0| >= |b|,
      on top of |gamma| times the dot product's: db <= (d + 3) u Bm.
    * Power: v = b^p by p - 1 multiplications: p |b|^(p-1) db from the argument (|b| taken as |b| + db) and 2 p u |v| for the
      multiplications (2 u each, so that pow() is admitted too).
    * RBF: a difference u, its square 3 u relative, d - 1 additions: (d + 3) u d2; the product with gamma u: da <= (d + 4) u a.
      exp at 2 ulp = 4 u relative, the argument's error propagated: dv <= v (da + 4 u).
    * Row sum: the terms' own errors, and (N - 1 + ceil(N / T)) u sum_j |v_j| for the ordered additions of a tile and the tile
      merges (a term passes through at most T - 1 + ceil(N / T) of them; a plain left-to-right or pairwise sum through N - 1).
    * Total: the rows' bounds, and (B - 1) u sum_i |row_i| for the ordered additions."""
    ql, cl = _ld(q), _ld(c)
    (B, d), N = ql.shape, cl.shape[0]
    g = abs(_gamma(gamma, d))
    if kind == 'poly':
        P = _dots(np.abs(ql), np.abs(cl))
        Bm = g * P + abs(coef0)
        db = (d + 3) * U * Bm
        b = np.abs(LD(_gamma(gamma, d)) * _dots(ql, cl) + LD(coef0)) + db
        p = int(degree)
        dv = p * b ** (p - 1) * db + 2 * p * U * b ** p
        av = b ** p
    else:
        a = g * _sqdist(ql, cl)
        av = np.exp(-a)
        dv = av * ((d + 4) * U * a + 4 * U)
    if skip_self:
        idx = np.arange(B)
        dv[idx, idx] = 0
        av[idx, idx] = 0
    adds = N - 1 + -(-N // T)
    rb = (dv.sum(axis=1) + adds * U * av.sum(axis=1)).astype(np.float64)
    tb = float(rb.sum() + (B - 1) * U * av.sum())
    return rb, tb


# ---------------------------------------------------------------------------------------------- kernel MMD
def median_gamma(real):
    """1 / the lower median of the fp32 squared distances (direct differences, rounded once) between the first MEDIAN_ROWS real
    rows and their other members: what torch.median of the strips of ops.pairwise_distance gives"""
    x = _ld(real[:MEDIAN_ROWS])
    n = len(x)
    d2 = _sqdist(x, x).astype(np.float32)
    other = np.sort(d2[~np.eye(n, dtype=bool)])
    return 1.0 / float(other[(len(other) - 1) // 2])


def kernel_mmd(real, fake, kind='poly', gamma=None, coef0=1.0, degree=3, biased=False):
    """-> dict(mmd2, k_rr, k_ff, k_rf, s_rr, s_ff, s_rf: floats, and bound: the absolute bound of mmd2, bounds: of the three
    totals).  mmd2's bound: the three totals' bounds over their divisors (the division exact in the bound: its rounding is in
    the 4 u below), and 4 u (|k_rr| + |k_ff| + 2 |k_rf|) for the three divisions, the doubling (exact) and the two additions."""
    N, M = len(real), len(fake)
    kw = dict(kind=kind, gamma=gamma, coef0=coef0, degree=degree)
    skip = not biased
    pairs = ((real, real, skip), (fake, fake, skip), (real, fake, False))
    s = [total(a, b, skip_self=k, as_ld=True, **kw) for a, b, k in pairs]
    tb = [error_bounds_rows(a, b, skip_self=k, **kw)[1] for a, b, k in pairs]
    div = [LD(N * (N - 1) if skip else N * N), LD(M * (M - 1) if skip else M * M), LD(N * M)]
    k = [s[i] / div[i] for i in range(3)]
    mmd2 = k[0] + k[1] - 2 * k[2]
    bound = float(tb[0] / div[0] + tb[1] / div[1] + 2 * tb[2] / div[2] + 4 * U * (abs(k[0]) + abs(k[1]) + 2 * abs(k[2])))
    return dict(mmd2=float(mmd2), k_rr=float(k[0]), k_ff=float(k[1]), k_rf=float(k[2]), s_rr=float(s[0]), s_ff=float(s[1]),
                s_rf=float(s[2]), bound=bound, bounds=tb)


# ---------------------------------------------------------------------------------------------- Frechet distance
def moments(x):
    """-> (mean [d], cov [d x d], ddof 1) in longdouble, the rows centred before the products"""
    x = _ld(x)
    n = len(x)
    mu = _osum(x, axis=0) / LD(n)
    y = x - mu
    return mu, (y.T @ y) / LD(n - 1)


def sqrt_trace(cov_r, cov_f):
    """-> (tr (cov_r cov_f)^(1/2), nu): through the symmetric congruence, eigvalsh in float64 on longdouble-built matrices; nu
    are the eigenvalues of C, clamped at 0, descending.  Equal matrices: (S S)^(1/2) = S, the trace itself."""
    lam, V = np.linalg.eigh(np.asarray(cov_r, np.float64))
    lam = np.maximum(lam, 0.0)
    A = np.sqrt(lam.astype(LD))[:, None] * V.T.astype(LD)
    C = A @ np.asarray(cov_f, LD) @ A.T
    C = ((C + C.T) / 2).astype(np.float64)
    nu = np.maximum(np.linalg.eigvalsh(C), 0.0)[::-1]
    if np.array_equal(np.asarray(cov_r), np.asarray(cov_f)):
        return np.trace(np.asarray(cov_r, LD)), nu
    return np.sqrt(nu.astype(LD)).sum(), nu


def frechet(real, fake):
    """-> dict(frechet_distance, mean_term, trace_term, tr_r, tr_f, tr_sqrt: floats; nu: the spectrum of the congruence)"""
    return frechet_of_moments(*moments(real), *moments(fake))


def frechet_of_moments(mu_r, cov_r, mu_f, cov_f):
    """the same from given means and covariances (longdouble or float64)"""
    mu_r, cov_r, mu_f, cov_f = (np.asarray(a, LD) for a in (mu_r, cov_r, mu_f, cov_f))
    dm = mu_r - mu_f
    mean_term = _osum(dm * dm)
    tr_r, tr_f = np.trace(cov_r), np.trace(cov_f)
    tr_sqrt, nu = sqrt_trace(cov_r, cov_f)
    trace_term = tr_r + tr_f - 2 * tr_sqrt
    return dict(frechet_distance=float(mean_term + trace_term), mean_term=float(mean_term), trace_term=float(trace_term),
                tr_r=float(tr_r), tr_f=float(tr_f), tr_sqrt=float(tr_sqrt), nu=nu)


def error_bounds_congruence(A, S):
    """elementwise bound of A S A^T in float64, both products in ascending index: 2 d u (|A| |S| |A|^T) (d roundings per
    product, by fma or not; the second product carries the first's)"""
    A, S = np.abs(np.asarray(A, LD)), np.abs(np.asarray(S, LD))
    return (2 * A.shape[0] * U * (A @ S @ A.T)).astype(np.float64)


def error_bounds_frechet(real, fake, ref=None):
    """-> dict(mean_term, trace_term, frechet_distance, tr_sqrt: absolute bounds; e_total, nu_min).  For the device's
    pipeline -- pca_moments, pca_eigh, sym_congruence, pca_eigh, ordered sums -- against the restatement.

    * Moments.  The mean is an ordered sum of N fp32 values and a division: dmu_i <= (N + 1) u mean|x_i|.  The covariance is a
      sum of N products of centred values; with m2_i the RAW second moment (>= the variance, and what the mean's error and the
      centring's rounding scale with): |dS_ij| <= (2 N + 8) u N / (N - 1) sqrt(m2_i m2_j).  (The sum's own part is (N + 2) u
      sqrt(S_ii S_jj); the rest pays for centring with a rounded mean.)  Its Frobenius norm: e_S = (2 N + 8) u N / (N - 1)
      sum_i m2_i.  The trace: sum_i |dS_ii| and (d - 1) u tr S for the ordered sum.
    * mean_term.  dm_i = mu_r,i - mu_f,i has D_i = dmu_r,i + dmu_f,i + u |dm_i|; the squares 2 |dm_i| D_i + D_i^2 + u dm_i^2,
      the ordered sum (d - 1) u: sum_i (2 |dm_i| D_i + D_i^2) + (d + 1) u sum_i dm_i^2.
    * The square root's trace, tr_sqrt = sum_i sqrt nu_i with nu the spectrum of C = A S_f A^T, A^T A = S_r.
      - The device's A is diag(sqrt lambda') V' from its eigen-solver.  Whatever V' is, A' S_f A'^T has the non-zero spectrum
        of (A'^T A') S_f: the pipeline is exact for S_r' = A'^T A', and what matters is |S_r' - S_r|.  The one-sided Jacobi
        solver stops when every pair has |g_p . g_q| <= 2^-52 |g_p| |g_q|, which leaves an off-diagonal of at most
        2^-52 sqrt(lambda_p lambda_q) / 2 in V' S V'^T (Frobenius norm <= u tr S), and each of at most MAX_SWEEPS = 64 sweeps
        rotates every column d - 1 times at 4 u per rotation: e_eig(S) = (4 d MAX_SWEEPS + 1) u tr S.  Forming A' (a square
        root and a product) adds 4 u tr S.  So e_r = e_S(real) + e_eig(S_r) + 4 u tr S_r, and e_f = e_S(fake).
      - A symmetric matrix with the spectrum nu is S_f^(1/2) S_r S_f^(1/2) (or the same with r and f exchanged): e_r moves it
        by at most |S_f| e_r, e_f by |S_r| e_f (Frobenius norms, >= the spectral ones).
      - The congruence in float64: 2 d u |A|^2_F |S_f|_F = 2 d u tr S_r |S_f|_F.  The second eigen-solve, on C:
        e_eig(C), tr C = tr(S_r S_f) <= |S_r|_F |S_f|_F; taken twice, for the restatement's own float64 eigvalsh.
      - E = the sum of these.  Weyl and Hoffman-Wielandt: sum_i |nu_i' - nu_i| <= sqrt(d) E and each |nu_i' - nu_i| <= E.  Then
        |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= min(|a - b| / sqrt nu_i, sqrt |a - b|): for the eigenvalues that
        are known to be >= nu_min > E the first form, sqrt(d) E / sqrt(nu_min) in all; for the k eigenvalues below that
        (a rank-deficient set: they are 0 up to E, and the solver clamps at 0) the second, k sqrt(E).  nu_min is a property of
        the test matrices, taken from the restatement's spectrum (`ref`), never from the device.
      - sqrt and the ordered sum: (d + 1) u tr_sqrt.
    * trace_term = tr_r + tr_f - 2 tr_sqrt: the three bounds (the last doubled) + 3 u (tr_r + tr_f + 2 tr_sqrt)."""
    ref = ref or frechet(real, fake)
    out = {}
    stats = []
    for x in (real, fake):
        xl = _ld(x)
        n, d = xl.shape
        m2 = (xl * xl).mean(axis=0)
        c = (2 * n + 8) * U * n / (n - 1)
        stats.append(dict(dmu=(n + 1) * U * np.abs(xl).mean(axis=0), e_S=float(c * m2.sum()), n=n))
    d = np.asarray(real).shape[1]
    (mu_r, cov_r), (mu_f, cov_f) = moments(real), moments(fake)
    dm = np.abs(mu_r - mu_f)
    D = stats[0]['dmu'] + stats[1]['dmu'] + U * dm
    out['mean_term'] = float((2 * dm * D + D * D).sum() + (d + 1) * U * (dm * dm).sum())
    tr_r, tr_f = float(np.trace(cov_r)), float(np.trace(cov_f))
    fro_r, fro_f = float(np.sqrt((cov_r * cov_r).sum())), float(np.sqrt((cov_f * cov_f).sum()))
    e_eig = lambda tr: (4 * d * MAX_SWEEPS + 1) * U * tr
    e_r = stats[0]['e_S'] + e_eig(tr_r) + 4 * U * tr_r
    e_f = stats[1]['e_S']
    E = fro_f * e_r + fro_r * e_f + 2 * d * U * tr_r * fro_f + 2 * e_eig(fro_r * fro_f)
    nu = np.asarray(ref['nu'], np.float64)
    big = nu[nu > 16 * E]                                    # bounded away from 0 by more than the perturbation
    k = len(nu) - len(big)
    b_sqrt = (math.sqrt(d) * E / math.sqrt(big.min() - E) if len(big) else 0.0) + k * math.sqrt(E + (nu[nu <= 16 * E].max() if k else 0.0))
    b_sqrt += (d + 1) * U * ref['tr_sqrt']
    b_tr = [s['e_S'] + (d - 1) * U * t for s, t in zip(stats, (tr_r, tr_f))]
    out['tr_sqrt'] = float(b_sqrt)
    out['trace_term'] = float(b_tr[0] + b_tr[1] + 2 * b_sqrt + 3 * U * (tr_r + tr_f + 2 * ref['tr_sqrt']))
    out['frechet_distance'] = out['mean_term'] + out['trace_term'] + U * (abs(ref['mean_term']) + abs(ref['trace_term']))
    out['e_total'], out['nu_min'], out['small'] = float(E), float(big.min()) if len(big) else 0.0, int(k)
    return out
