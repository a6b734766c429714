"""How much the latent code says about the data, from the aggregate posterior in fp64 (csrc/evae_agg_lse.hip).

With mu_j, lv_j the posterior mean and log-variance of data point j (N of them), q(z|x_j) = N(z; mu_j, diag exp(lv_j)), the
aggregate posterior q(z) = 1/N sum_j q(z|x_j), its marginals q_d(z_d) = 1/N sum_j N(z_d; mu_jd, exp(lv_jd)), and z_i a draw of
q(z|x_{rows[i]}), i < B:

    mutual_information   I_q(x; z)               = mean_i [ sum_d log q(z_id | x_rows[i]) - log q(z_i) ]         (<= log N)
    total_correlation    KL(q(z) || prod_d q_d)  = mean_i [ log q(z_i) - sum_d log q_d(z_id) ]                   (Chen et al. 2018)
    dimension_wise_kl    sum_d KL(q_d || N(0,1)) = mean_i sum_d [ log q_d(z_id) - log N(z_id; 0, 1) ]
    mutual_information_per_dimension [d]         = mean_i [ log q(z_id | x_rows[i]) - log q_d(z_id) ]
    kl_per_dimension [d]                         = mean_i [ log q_d(z_id) - log N(z_id; 0, 1) ]
    entropy_aggregate                            = - mean_i log q(z_i)

over ALL N components, not a minibatch estimate.  With log p(z_i) of a prior (log_prior) also kl = mean_i [ sum_d log q(z_id |
x_rows[i]) - log p(z_i) ] and marginal_kl = mean_i [ log q(z_i) - log p(z_i) ]: the average KL term of the ELBO and its split
kl = mutual_information + marginal_kl (Hoffman & Johnson 2016).

The three [B] and [B x d] arrays come from the device in float64 (ops.agg_posterior_lse).  Every mean is then taken on the
host from those float64 entries themselves, never from per-row differences: the sum of all entries a mean is made of (signs
applied, which is exact) is math.fsum's -- the exactly rounded sum, so its order is immaterial and stated once: any -- and is
divided by B once.  A mean therefore carries two roundings whatever B is, and kl = mutual_information + marginal_kl, exact
for the three sums, holds for the three means up to their roundings (a running sum over 60 000 rows would not give that).
log N(z; 0, 1) is -log(2 pi)/2 - z^2/2, the term of a component with mu = 0, lv = 0.
Inputs are tensors on the device; there is no CPU path."""
import itertools
import math

import numpy as np
import torch

from . import _lib, ops

_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _components(mean, log_var, who):
    for name, t in (("mean", mean), ("log_var", log_var)):
        if not torch.is_tensor(t):
            raise ValueError("%s: %s must be a tensor on the device, got %s" % (who, name, type(t).__name__))
        if not t.is_cuda:
            raise _lib.EvaeError("%s: %s is a %s tensor; there is no CPU fallback" % (who, name, t.device))
        if t.dim() != 2 or not t.is_floating_point():
            raise ValueError("%s: %s must be a floating-point [N x d] tensor, got %s %s" % (who, name, t.dtype, tuple(t.shape)))
    if mean.shape != log_var.shape or mean.shape[0] < 1 or mean.shape[1] < 1:
        raise ValueError("%s: mean is %s, log_var %s" % (who, tuple(mean.shape), tuple(log_var.shape)))
    return ops._f32(mean.detach()), ops._f32(log_var.detach())


def _queries(z, d, who):
    if not torch.is_tensor(z):
        raise ValueError("%s: z must be a tensor on the device, got %s" % (who, type(z).__name__))
    if not z.is_cuda:
        raise _lib.EvaeError("%s: z is a %s tensor; there is no CPU fallback" % (who, z.device))
    if z.dim() != 2 or not z.is_floating_point() or z.shape[1] != d or z.shape[0] < 1:
        raise ValueError("%s: z must be a floating-point [B x %d] tensor, got %s %s" % (who, d, z.dtype, tuple(z.shape)))
    return ops._f32(z.detach())


def _generator(random_state):
    g = torch.Generator(device="cpu")
    if random_state is None:
        g.seed()
    else:
        g.manual_seed(int(random_state))
    return g


def _mean(B, plus, minus):
    """(sum of every entry of `plus` - sum of every entry of `minus`) / B: ONE exactly rounded sum of all the float64 entries
    (math.fsum), then one division"""
    return math.fsum(itertools.chain(plus.ravel().tolist(), (-minus).ravel().tolist())) / B


def _column_means(B, plus, minus):
    """_mean of every column of two [B x d] arrays -> float64 [d]"""
    return np.array([_mean(B, plus[:, k], minus[:, k]) for k in range(plus.shape[1])], dtype=np.float64)


def aggregate_posterior_log_density(z, mean, log_var, per_dimension=False):
    """z [B x d], mean and log_var [N x d] -> log q(z_i), float64 [B] on the device; per_dimension=True: (log_q, log_qd) with
    log_qd [B x d] the log-density of every marginal q_d at z_id."""
    mean, log_var = _components(mean, log_var, "aggregate_posterior_log_density")
    z = _queries(z, mean.shape[1], "aggregate_posterior_log_density")
    with torch.no_grad():
        out = ops.agg_posterior_lse(z, mean, log_var, joint=True, per_dimension=bool(per_dimension))
    return (out.log_q, out.log_qd) if per_dimension else out.log_q


def draw_posterior_samples(mean, log_var, rows=None, n_samples=None, random_state=None):
    """-> (z float32 [B x d], rows int32 [B]) on the device: z_i = mu + exp(lv / 2) eps of data point rows[i].  rows: given, or
    every row once in index order, or (n_samples) that many distinct rows, the head of a permutation of a CPU torch.Generator
    seeded with random_state (None draws a seed).  eps is float64 standard normals [B x d] of the same generator, taken after
    the permutation; the expression is float64 on the host and z is rounded to float32 once."""
    mean, log_var = _components(mean, log_var, "draw_posterior_samples")
    N = mean.shape[0]
    g = _generator(random_state)
    if rows is not None:
        if n_samples is not None:
            raise ValueError("draw_posterior_samples: rows and n_samples given; one of them expected")
        rows = _rows_of(rows, None, N, "draw_posterior_samples").cpu().long()
    elif n_samples is not None:
        n = int(n_samples)
        if not 1 <= n <= N:
            raise ValueError("draw_posterior_samples: n_samples=%d outside [1, N=%d]" % (n, N))
        rows = torch.randperm(N, generator=g)[:n]
    else:
        rows = torch.arange(N)
    eps = torch.randn((len(rows), mean.shape[1]), dtype=torch.float64, generator=g)
    mu, lv = mean.cpu()[rows].double(), log_var.cpu()[rows].double()
    z = (mu + torch.exp(0.5 * lv) * eps).float()
    return z.to(mean.device), rows.to(torch.int32).to(mean.device)


def _rows_of(rows, B, N, who):
    """rows -> contiguous int32 [B] on the device it is on, inside [0, N)"""
    if not torch.is_tensor(rows) or rows.is_floating_point() or rows.dim() != 1 or (B is not None and rows.shape[0] != B) \
            or rows.shape[0] < 1:
        raise ValueError("%s: rows must be an integer tensor of %s entries" % (who, "B=%d" % B if B is not None else ">= 1"))
    lo, hi = int(rows.min()), int(rows.max())
    if lo < 0 or hi >= N:
        raise ValueError("%s: rows span [%d, %d], outside [0, %d)" % (who, lo, hi, N))
    return rows.to(torch.int32).contiguous()


def latent_information(mean, log_var, z=None, rows=None, n_samples=None, random_state=None, log_prior=None,
                       information_threshold=0.01):
    """mean, log_var [N x d] on the device -> dict (Python floats; the [d] vectors float64 on the device; z and rows as used).
    z=None: draw_posterior_samples(mean, log_var, rows, n_samples, random_state).  z given: rows[i] names the data point z_i was
    drawn for (default: row i, which needs B = N).  log_prior [B], any float dtype: log p(z_i) of a prior, adds kl and
    marginal_kl.  Keys: mutual_information, total_correlation, dimension_wise_kl, mutual_information_per_dimension,
    kl_per_dimension, entropy_aggregate, log_n (the ceiling of any estimate of the mutual information), active_units (the
    reference's rule: population variance of the means > 0.01, two-pass float64 moments on the device),
    active_units_by_information (dimensions whose I(x; z_d) exceeds information_threshold nats), n, z_size."""
    who = "latent_information"
    mean, log_var = _components(mean, log_var, who)
    N, d = mean.shape
    if z is None:
        z, rows = draw_posterior_samples(mean, log_var, rows, n_samples, random_state)
    else:
        if n_samples is not None:
            raise ValueError("%s: n_samples given with z" % who)
        z = _queries(z, d, who)
        if rows is None:
            if z.shape[0] != N:
                raise ValueError("%s: z has %d rows for N=%d components and no rows were given" % (who, z.shape[0], N))
            rows = torch.arange(N, dtype=torch.int32, device=z.device)
        else:
            rows = _rows_of(rows, z.shape[0], N, who).to(z.device)
    B = z.shape[0]
    if log_prior is not None:
        if not torch.is_tensor(log_prior) or not log_prior.is_floating_point() or tuple(log_prior.shape) != (B,):
            raise ValueError("%s: log_prior must be a floating-point [%d] tensor" % (who, B))
    with torch.no_grad():
        out = ops.agg_posterior_lse(z, mean, log_var, rows=rows)
        m64 = mean.double()
        centre = m64.mean(dim=0)
        variance = ((m64 - centre) ** 2).mean(dim=0)
        active = int((variance > 0.01).sum().item())
        log_q, log_qd, log_cond = (t.cpu().numpy() for t in out)
        zz = z.double().cpu().numpy()
    log_std = -_HALF_LOG_2PI - 0.5 * (zz * zz)
    mi_d = _column_means(B, log_cond, log_qd)
    kl_d = _column_means(B, log_qd, log_std)
    res = {
        'mutual_information': _mean(B, log_cond, log_q),
        'total_correlation': _mean(B, log_q, log_qd),
        'dimension_wise_kl': _mean(B, log_qd, log_std),
        'mutual_information_per_dimension': torch.from_numpy(mi_d).to(z.device),
        'kl_per_dimension': torch.from_numpy(kl_d).to(z.device),
        'entropy_aggregate': _mean(B, -log_q, np.zeros(0)),
        'log_n': math.log(N),
        'active_units': active,
        'active_units_by_information': int((mi_d > float(information_threshold)).sum()),
        'n': int(B), 'z_size': int(d), 'z': z, 'rows': rows,
    }
    if log_prior is not None:
        lp = log_prior.detach().double().cpu().numpy()
        res['kl'] = _mean(B, log_cond, lp)
        res['marginal_kl'] = _mean(B, log_q, lp)
    return res
