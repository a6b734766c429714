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
Inputs are tensors on the device; there is no CPU path."""
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


def sample_quality(real, fake, nearest_k=5, train=None):
    """compute_prdc(real, fake, nearest_k) plus authenticity -- against `train` when given, else against `real` -- and, for
    information, nearest_distance_median: the median distance (not squared) from a generated row to its nearest row of that set."""
    out = compute_prdc(real, fake, nearest_k)
    T, F = _pair(real if train is None else train, fake, "sample_quality")
    count, _, d2 = _authentic(T, F)
    out['authenticity'] = count / F.shape[0]
    out['nearest_distance_median'] = float(torch.sqrt(d2).median().item())
    return out
