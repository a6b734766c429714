"""Quality of generated samples against real ones, as exact integers from the device (csrc/evae_ball_count.hip):
improved precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020; the definitions and argument
names of their `prdc` package, on squared distances) and authenticity (Alaa et al. 2021).

With R [N x d] the real rows, F [M x d] the generated ones, D the fp32 squared distance of ops.pairwise_distance and rho_k(X)[i]
the distance from X[i] to its k-th nearest OTHER row of X (ops.kth_neighbour_radius; self left out by index, so a radius can be
0), every inequality strict:

    precision    = #{ j : some i has D(R_i, F_j) < rho_k(R)[i] } / M
    recall       = #{ i : some j has D(R_i, F_j) < rho_k(F)[j] } / N
    density      = sum_j #{ i : D(R_i, F_j) < rho_k(R)[i] } / (k M)
    coverage     = #{ i : min_j D(R_i, F_j) < rho_k(R)[i] } / N
    authenticity = #{ j : D(R_i*, F_j) >= rho_1(R)[i*] } / M,  i* the nearest real of F_j, the lower index on a tie

Each is integers through one float64 expression on the host, in the order `prdc` writes it (density: (1 / k) * (sum / M)).
Neither an [N x M] matrix nor a sorted row exists at any point.

Beside the ball counts, two distribution-level distances in fp64 (csrc/evae_kernel_sum.hip), which move under a
uniform shift or shrink of the sample cloud where the counts do not: frechet_distance, FID's formula on whatever features are
given, and kernel_mmd / kernel_inception_distance, the unbiased kernel MMD^2 (KID's cubic kernel by default).  Every sum in
them has a fixed order: equal inputs give bit-equal results.
Inputs are tensors on the device; there is no CPU path."""
import warnings

import torch

from . import _lib, ops


def _rows(t, name, who):
    if not torch.is_tensor(t):
        raise ValueError("%s: %s must be a tensor on the device, got %s" % (who, name, type(t).__name__))
    if not t.is_cuda:
        raise _lib.EvaeError("%s: %s is a %s tensor; there is no CPU fallback" % (who, name, t.device))
    if t.dim() != 2 or not t.is_floating_point():
        raise ValueError("%s: %s must be a floating-point [rows x d] tensor, got %s %s" % (who, name, t.dtype, tuple(t.shape)))
    return ops._f32(t.detach())


def _pair(real_features, fake_features, who):
    R, F = _rows(real_features, "real_features", who), _rows(fake_features, "fake_features", who)
    if R.shape[1] != F.shape[1] or R.shape[1] < 1:
        raise ValueError("%s: %d features in real_features, %d in fake_features" % (who, R.shape[1], F.shape[1]))
    if R.shape[0] < 1 or F.shape[0] < 1:
        raise ValueError("%s: %d real rows and %d generated rows" % (who, R.shape[0], F.shape[0]))
    return R, F


def _nearest_k(nearest_k, N, M, who):
    k, top, cap = int(nearest_k), min(N, M) - 1, ops.tsne_nn_max_neighbours()
    if not 1 <= k <= top:
        raise ValueError("%s: nearest_k=%d outside [1, min(N=%d, M=%d) - 1 = %d]" % (who, k, N, M, top))
    if k > cap:
        raise ValueError("%s: nearest_k=%d above the neighbour search's %d" % (who, k, cap))
    return k


def compute_prdc(real_features, fake_features, nearest_k=5, strip_rows=0):
    """-> dict(precision, recall, density, coverage: floats; nearest_k, n_real, n_fake: ints).  Two neighbour searches for the
    radii and two ball-count passes: the generated rows against the real ones (precision, density), the real rows against the
    generated ones (recall, coverage)."""
    R, F = _pair(real_features, fake_features, "compute_prdc")
    N, M = R.shape[0], F.shape[0]
    k = _nearest_k(nearest_k, N, M, "compute_prdc")
    with torch.no_grad():
        rho_r, rho_f = ops.kth_neighbour_radius(R, k), ops.kth_neighbour_radius(F, k)
        in_real = ops.ball_count(F, R, col_radius=rho_r, want_nearest=False, strip_rows=strip_rows).col_hits
        of_real = ops.ball_count(R, F, col_radius=rho_f, row_radius=rho_r, want_nearest=False, strip_rows=strip_rows)
        sums = torch.stack(((in_real > 0).sum(), in_real.sum(dtype=torch.int64), (of_real.col_hits > 0).sum(),
                            (of_real.row_hits > 0).sum())).tolist()      # read once: four Python integers
    return dict(precision=sums[0] / M, recall=sums[2] / N, density=(1.0 / k) * (sums[1] / M), coverage=sums[3] / N, nearest_k=k, n_real=N,
                n_fake=M)


def nearest_real(real_features, fake_features, strip_rows=0):
    """-> (idx int32 [M], d2 float32 [M]): every generated row's nearest real row, the lower index on a tie"""
    R, F = _pair(real_features, fake_features, "nearest_real")
    with torch.no_grad():
        out = ops.ball_count(F, R, strip_rows=strip_rows)
    return out.nn_idx, out.nn_d2


def _authentic(R, F, strip_rows=0):
    """(the number of authentic rows of F, nn_idx, nn_d2): not closer to a real row than that row's nearest other real row is"""
    if R.shape[0] < 2:
        raise ValueError("authenticity: %d real rows, at least 2 expected" % R.shape[0])
    with torch.no_grad():
        rho_1 = ops.kth_neighbour_radius(R, 1)
        out = ops.ball_count(F, R, strip_rows=strip_rows)
        count = int((out.nn_d2 >= rho_1[out.nn_idx.long()]).sum().item())
    return count, out.nn_idx, out.nn_d2


def authenticity(real_features, fake_features, strip_rows=0):
    """the share of generated rows that are not copies: 0 for exact copies of real rows"""
    R, F = _pair(real_features, fake_features, "authenticity")
    return _authentic(R, F, strip_rows)[0] / F.shape[0]


def frechet_distance(real_features, fake_features):
    """-> dict(frechet_distance, mean_term, trace_term: floats; n_real, n_fake: ints; eigh_converged: bool).  The Frechet
    distance |mu_r - mu_f|^2 + tr(S_r + S_f - 2 (S_r S_f)^(1/2)) between the Gaussians fitted to the two sets, covariances with
    ddof 1, in fp64 on the device.  This is the distance of the features GIVEN: it is "FID" only when they are Inception features.

    The square root's trace without a non-symmetric product: ops.pca_eigh(S_r) = (lambda, V), A = diag(sqrt lambda) V so that
    A^T A = S_r; C = A S_f A^T (ops.sym_congruence) is symmetric positive semi-definite and has the non-zero spectrum of
    S_r S_f, so tr (S_r S_f)^(1/2) = sum sqrt nu over the eigenvalues nu of C (ops.pca_eigh again, which clamps at 0).  Every
    sum is ordered (ops.ordered_sum); one device-to-host read.  An eigen-solve that did not converge sets eigh_converged False
    and warns (RuntimeWarning); the value is returned all the same."""
    who = "frechet_distance"
    R, F = _pair(real_features, fake_features, who)
    (N, d), M = R.shape, F.shape[0]
    if d > ops.pca_max_features():
        raise ValueError("%s: %d features in real_features, above the %d of the device eigen-solver; reduce them first with "
                         "evae.pca.PCA" % (who, d, ops.pca_max_features()))
    if N < 2 or M < 2:
        raise ValueError("%s: %d rows in real_features and %d in fake_features, at least 2 each expected" % (who, N, M))
    with torch.no_grad():
        (mu_r, cov_r), (mu_f, cov_f) = ops.pca_moments(R), ops.pca_moments(F)
        dm = mu_r - mu_f
        lam, V, info_r = ops.pca_eigh(cov_r)
        A = (torch.sqrt(lam).unsqueeze(1) * V).contiguous()
        nu, _, info_c = ops.pca_eigh(ops.sym_congruence(A, cov_f))
        got = torch.stack((ops.ordered_sum(dm * dm), ops.ordered_sum(torch.diagonal(cov_r).contiguous()),
                           ops.ordered_sum(torch.diagonal(cov_f).contiguous()), ops.ordered_sum(torch.sqrt(nu)), info_r[1],
                           info_c[1])).tolist()                         # read once
    mean_term, tr_r, tr_f, tr_sqrt = got[:4]
    converged = bool(got[4] != 0.0 and got[5] != 0.0)
    if not converged:
        warnings.warn("%s: the Jacobi eigen-solver did not converge within %d sweeps (real covariance: %s, congruence: %s); the "
                      "value is returned as it stands" % (who, ops.pca_max_sweeps(), got[4] != 0.0, got[5] != 0.0), RuntimeWarning)
    trace_term = tr_r + tr_f - 2.0 * tr_sqrt
    return dict(frechet_distance=mean_term + trace_term, mean_term=mean_term, trace_term=trace_term, n_real=N, n_fake=M,
                eigh_converged=converged)


MEDIAN_ROWS = 2048      # gamma='median': the real rows the heuristic looks at
_MEDIAN_STRIP = 256


def median_gamma(real_features):
    """1 / median of the squared distances (ops.pairwise_distance: fp32) between every real row and the OTHER rows, the usual
    bandwidth heuristic -- over the first MEDIAN_ROWS = 2 048 rows only: a subsample of a larger set.  torch.median: the lower
    of the two middle values.  -> (gamma, rows used)"""
    R = _rows(real_features, "real_features", "median_gamma")
    n = min(R.shape[0], MEDIAN_ROWS)
    if n < 2:
        raise ValueError("median_gamma: %d rows in real_features, at least 2 expected" % R.shape[0])
    R = R[:n]
    with torch.no_grad():
        other = torch.empty((n, n - 1), device=R.device)
        for r0 in range(0, n, _MEDIAN_STRIP):                           # strips: no [N x N] buffer beside the one collected
            strip = ops.pairwise_distance(R[r0:r0 + _MEDIAN_STRIP], R)
            rows = strip.shape[0]
            keep = torch.ones_like(strip, dtype=torch.bool)
            keep[torch.arange(rows, device=R.device), torch.arange(r0, r0 + rows, device=R.device)] = False
            other[r0:r0 + rows] = strip[keep].view(rows, n - 1)
        med = float(other.view(-1).median().item())
    if not med > 0.0:
        raise ValueError("median_gamma: the median squared distance between real rows is %r; no bandwidth follows from it" % med)
    return 1.0 / med, n


def kernel_mmd(real_features, fake_features, kernel='poly', gamma=None, coef0=1.0, degree=3, biased=False):
    """-> dict(mmd2, k_rr, k_ff, k_rf: floats; kernel, gamma, n_real, n_fake).  The squared maximum mean discrepancy of the two
    sets under the kernel (ops.kernel_row_sums: 'poly' (gamma <x, y> + coef0)^degree or 'rbf' exp(-gamma |x - y|^2)), in fp64
    on the device: three row-sum passes, each followed by ops.ordered_sum, one device-to-host read of the three totals.

        unbiased: mmd2 = S_rr / (N (N - 1)) + S_ff / (M (M - 1)) - 2 S_rf / (N M), the within-set sums without their diagonal
                  (left out by index); it can be negative.  Needs N, M >= 2.
        biased:   the V-statistic: the diagonals stay, the divisors are N^2 and M^2; never negative beyond rounding.

    k_rr, k_ff, k_rf are the three means as they enter mmd2.  gamma=None is 1 / d for both kernels (KID's and scikit-learn's
    default).  kernel='rbf', gamma='median': 1 / median of the squared distances between real rows, from the first 2 048 real
    rows only -- a subsample (median_gamma)."""
    who = "kernel_mmd"
    R, F = _pair(real_features, fake_features, who)
    (N, d), M = R.shape, F.shape[0]
    ops.kernel_sum_check(kernel, degree, coef0, who, name="kernel")      # every argument before the first launch
    if not biased and (N < 2 or M < 2):
        raise ValueError("%s: %d rows in real_features and %d in fake_features, the unbiased form needs 2 each" % (who, N, M))
    if not 1 <= d <= ops.kernel_sum_max_features():
        raise ValueError("%s: %d features in real_features, outside [1, %d]" % (who, d, ops.kernel_sum_max_features()))
    if isinstance(gamma, str):
        if gamma != 'median' or kernel != 'rbf':
            raise ValueError("%s: gamma=%r with kernel=%r; only kernel='rbf' takes gamma='median'" % (who, gamma, kernel))
        gamma = median_gamma(R)[0]
    elif gamma is not None and (isinstance(gamma, bool) or not isinstance(gamma, (int, float))):
        raise ValueError("%s: gamma=%r, a number, None (1 / d) or 'median' expected" % (who, gamma))
    gamma = 1.0 / d if gamma is None else float(gamma)
    skip = not biased
    with torch.no_grad():
        sums = torch.stack([ops.ordered_sum(ops.kernel_row_sums(q, c, kernel, gamma, coef0, degree, skip_self=s))
                            for q, c, s in ((R, R, skip), (F, F, skip), (R, F, False))]).tolist()      # read once
    k_rr = sums[0] / (N * (N - 1) if skip else N * N)
    k_ff = sums[1] / (M * (M - 1) if skip else M * M)
    k_rf = sums[2] / (N * M)
    return dict(mmd2=k_rr + k_ff - 2.0 * k_rf, k_rr=k_rr, k_ff=k_ff, k_rf=k_rf, kernel=kernel, gamma=gamma, n_real=N, n_fake=M)


def kernel_inception_distance(real_features, fake_features):
    """The unbiased MMD^2 under KID's kernel (<x, y> / d + 1)^3, over the FULL sets: one number.  The subset protocol of the KID
    paper (the mean over subsets of 1 000 rows, with its variance estimate) is not carried over; like frechet_distance this is
    the distance of the features given, "KID" only for Inception features."""
    return kernel_mmd(real_features, fake_features, 'poly', None, 1.0, 3)['mmd2']


def sample_quality(real, fake, nearest_k=5, train=None, distances=False):
    """compute_prdc(real, fake, nearest_k) plus authenticity -- against `train` when given, else against `real` -- and, for
    information, nearest_distance_median: the median distance (not squared) from a generated row to its nearest row of that set.
    distances=True adds the distribution-level distances of fake to real: frechet_distance and kid, and with `train` kid_train,
    the kernel distance to the training set: copies of training rows give a kid_train far below kid.  A distance whose kernels
    do not take the width (ops.pca_max_features(), ops.kernel_sum_max_features()) is left out, not approximated.  The default
    issues no launch beyond the ones above."""
    out = compute_prdc(real, fake, nearest_k)
    T, F = _pair(real if train is None else train, fake, "sample_quality")
    count, _, d2 = _authentic(T, F)
    out['authenticity'] = count / F.shape[0]
    out['nearest_distance_median'] = float(torch.sqrt(d2).median().item())
    if distances:
        if F.shape[1] <= ops.pca_max_features():
            out['frechet_distance'] = frechet_distance(real, fake)['frechet_distance']
        if F.shape[1] <= ops.kernel_sum_max_features():
            out['kid'] = kernel_inception_distance(real, fake)
            if train is not None:
                out['kid_train'] = kernel_inception_distance(train, fake)
    return out
