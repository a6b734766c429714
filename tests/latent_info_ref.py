"""numpy restatement of what csrc/evae_agg_lse.hip and evae/latent_info.py compute, in np.longdouble (a 64-bit
mantissa on x86) and returned as float64: its own error is far below the bounds it is used with.  Inputs are float32 arrays.

    w_jd = exp(-lv_jd), c_jd = -(lv_jd + log 2 pi) / 2, t_ijd = c_jd - (z_id - mu_jd)^2 w_jd / 2
    log_q[i] = LSE_j sum_d t_ijd - log N, log_qd[i][d] = LSE_j t_ijd - log N, log_cond[i][d] = t_{rows[i], d}

Every log-sum-exp subtracts the maximum; the count is taken inside the logarithm (m + log(S / N)), so N equal components give
the single term back exactly.  error_bounds is the tolerance the device (and float64 torch on the host) are held to."""
import math

import numpy as np

LD = np.longdouble
LOG_2PI = LD("1.8378770664093454835606594728112352797")
U = 2.0 ** -53
G_TERM = 24.0          # roundings of one term, in u, scaled by A = |lv|/2 + log(2 pi)/2 + (z - mu)^2 w / 2 (see error_bounds)
TILE = 32


# the parity shapes (B, N, d) of tests/test_gpu_latent_info.py and tests/test_latent_info_ref_host.py
SHAPES = [(1, 1, 1), (3, 1, 40), (5, 2, 1), (17, 63, 40), (64, 64, 64), (65, 257, 65), (33, TILE - 1, 40), (33, TILE, 40),
          (33, TILE + 1, 40), (33, 2 * TILE + 1, 40), (100, 1000, 256), (300, 7, 3)]
_CASES = {}


def case(B, N, d):
    """-> dict(z, mean, log_var: float32; rows: int32; log_q, log_qd, log_cond: the restatement; bq, bqd, bc: error_bounds),
    made once per shape and never written to.  means ~ 0.5 N(0, 1), lv ~ U(-3, 1), query i drawn from component rows[i] =
    a shuffle of i mod N: every component carries weight in some row as soon as B >= N."""
    key = (B, N, d)
    if key not in _CASES:
        rs = np.random.RandomState(B * 1000003 + N * 1009 + d)
        mean = (0.5 * rs.randn(N, d)).astype(np.float32)
        log_var = rs.uniform(-3.0, 1.0, size=(N, d)).astype(np.float32)
        rows = rs.permutation(np.arange(B) % N).astype(np.int32)
        z = (mean[rows] + np.exp(0.5 * log_var[rows]) * rs.randn(B, d)).astype(np.float32)
        c = dict(z=z, mean=mean, log_var=log_var, rows=rows)
        c['log_q'], c['log_qd'], c['log_cond'] = agg_lse(z, mean, log_var, rows)
        c['bq'], c['bqd'], c['bc'] = error_bounds(z, mean, log_var, rows, values=(c['log_q'], c['log_qd']))
        for a in c.values():
            a.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


def _ld(a):
    return np.asarray(a, dtype=np.float32).astype(LD)


def _row_sum(a):
    """sum over the last axis in ascending index"""
    return np.cumsum(a, axis=-1, dtype=LD)[..., -1]


def _lse(t, n):
    """LSE over axis 0 of t [N x ...] minus log n"""
    m = t.max(axis=0)
    return m + np.log(np.exp(t - m).sum(axis=0, dtype=LD) / LD(n))


def _parts(z, mean, log_var, rows=None):
    """(log_q [B], log_qd [B x d], log_cond [B x d] or None) in longdouble, a query row at a time"""
    z, mu, lv = _ld(z), _ld(mean), _ld(log_var)
    B, d = z.shape
    N = mu.shape[0]
    w, c = np.exp(-lv), LD(-0.5) * (lv + LOG_2PI)
    log_q, log_qd = np.empty(B, dtype=LD), np.empty((B, d), dtype=LD)
    log_cond = None if rows is None else np.empty((B, d), dtype=LD)
    for i in range(B):
        df = z[i][None, :] - mu
        t = c - LD(0.5) * (df * df) * w                     # [N x d]
        log_q[i] = _lse(_row_sum(t), N)
        log_qd[i] = _lse(t, N)
        if rows is not None:
            log_cond[i] = t[int(rows[i])]
    return log_q, log_qd, log_cond


def agg_lse(z, mean, log_var, rows=None):
    """-> (log_q, log_qd, log_cond or None), float64"""
    return tuple(None if a is None else a.astype(np.float64) for a in _parts(z, mean, log_var, rows))


def error_bounds(z, mean, log_var, rows=None, tile=TILE, values=None):
    """-> (bound_q [B], bound_qd [B x d], bound_cond [B x d] or None): what a float64 evaluation of agg_lse may differ from the
    exact value by, from u = 2^-53 (tests/test_gpu_latent_info.py has the derivation):

        term:   |dt_ijd| <= G u A_ijd,  A_ijd = |lv_jd| / 2 + log(2 pi) / 2 + (z_id - mu_jd)^2 w_jd / 2,  G = 24
        joint:  |d sum_d t_ijd| <= (G + d - 1) u sum_d A_ijd
        LSE:    the largest input error over j, + L u with L = (N - 1) + 6 log N + 8 (1 + ceil(N / tile)),
                + 3 u (|result| + log N)"""
    z, mu, lv = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (z, mean, log_var))
    B, d = z.shape
    N = mu.shape[0]
    w = np.exp(-lv)
    base = 0.5 * np.abs(lv) + 0.5 * float(LOG_2PI)
    L = (N - 1) + 6.0 * math.log(N) + 8.0 * (1 + -(-N // tile))
    if values is None:
        values = agg_lse(z, mean, log_var)
    log_q, log_qd = values[0], values[1]
    bq, bqd = np.empty(B), np.empty((B, d))
    bc = None if rows is None else np.empty((B, d))
    for i in range(B):
        A = base + 0.5 * (z[i][None, :] - mu) ** 2 * w       # [N x d]
        bq[i] = (G_TERM + d - 1) * U * A.sum(axis=1).max()
        bqd[i] = G_TERM * U * A.max(axis=0)
        if rows is not None:
            bc[i] = G_TERM * U * A[int(rows[i])]
    bq += L * U + 3.0 * U * (np.abs(log_q) + math.log(N))
    bqd += L * U + 3.0 * U * (np.abs(log_qd) + math.log(N))
    return bq, bqd, bc


def draws(mean, log_var, rows=None, n_samples=None, random_state=0):
    """-> (z float32 [B x d], rows int64 [B]): evae.latent_info.draw_posterior_samples restated.  The permutation and the
    normals are torch's (a CPU generator seeded with random_state: numpy has no copy of that stream); the expression
    mu + exp(lv / 2) eps is longdouble, rounded to float32 once."""
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(int(random_state))
    N, d = np.asarray(mean).shape
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
    elif n_samples is not None:
        rows = torch.randperm(N, generator=g)[:int(n_samples)].numpy()
    else:
        rows = np.arange(N, dtype=np.int64)
    eps = torch.randn((len(rows), d), dtype=torch.float64, generator=g).numpy().astype(LD)
    z = _ld(mean)[rows] + np.exp(LD(0.5) * _ld(log_var)[rows]) * eps
    return z.astype(np.float32), rows


def _mean(a):
    """mean over axis 0, a running sum in index order"""
    return np.cumsum(a, axis=0, dtype=LD)[-1] / LD(a.shape[0])


def latent_information(mean, log_var, z, rows, log_prior=None, information_threshold=0.01):
    """evae.latent_info.latent_information restated for given z and rows; nothing is rounded to float64 before the end"""
    log_q, log_qd, log_cond = _parts(z, mean, log_var, rows)
    zz = _ld(z)
    log_std = LD(-0.5) * LOG_2PI - LD(0.5) * (zz * zz)
    cond = _row_sum(log_cond)
    mi_d, kl_d = _mean(log_cond - log_qd), _mean(log_qd - log_std)
    N, d = np.asarray(mean).shape
    res = {
        'mutual_information': float(_mean(cond - log_q)),
        'total_correlation': float(_mean(log_q - _row_sum(log_qd))),
        'dimension_wise_kl': float(_mean(_row_sum(log_qd - log_std))),
        'mutual_information_per_dimension': mi_d.astype(np.float64),
        'kl_per_dimension': kl_d.astype(np.float64),
        'entropy_aggregate': float(-_mean(log_q)),
        'log_n': math.log(N),
        'active_units': int((np.var(np.asarray(mean, dtype=np.float64), axis=0) > 0.01).sum()),
        'active_units_by_information': int((mi_d > information_threshold).sum()),
        'n': int(len(zz)), 'z_size': int(d),
    }
    if log_prior is not None:
        lp = np.asarray(log_prior).astype(LD)
        res['kl'] = float(_mean(cond - lp))
        res['marginal_kl'] = float(_mean(log_q - lp))
    return res
