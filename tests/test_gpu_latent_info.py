"""GPU: the aggregate-posterior kernels (csrc/evae_agg_lse.hip), evae.ops.agg_posterior_lse, evae.latent_info and the
latent-information report, against the longdouble restatement tests/latent_info_ref.py (held to float64 torch and scipy, within
the bound used here and on the inputs used here, by tests/test_latent_info_ref_host.py).

The yardstick is always the restatement, never the code under test.  Its own error (a 64-bit mantissa) is 2^-11 of float64's.
The tolerance is a bound from the arithmetic, u = 2^-53 (ref.error_bounds computes it per element):

* Term.  t = c - (z - mu)^2 w / 2 with c = -(lv + log 2 pi) / 2 and w = exp(-lv).  z, mu, lv are fp32 values, exact in fp64.
  c: one addition, 2 u (|lv| / 2 + log(2 pi) / 2), the halving exact.  w: the library exp, taken at 2 ulp = 4 u.  The
  difference u, its square 3 u, times w 8 u, the halving exact, the last subtraction u |t|.  With
  A = |lv| / 2 + log(2 pi) / 2 + (z - mu)^2 w / 2 >= |c| + (z - mu)^2 w / 2 >= |t| that is 11 u A; float64 torch, the other
  correct evaluation the bound must admit, forms sigma = exp(lv / 2), (z - mu)^2 / (2 sigma^2) and log sigma: 20 u A.  G = 24:
  |dt| <= G u A.  log_cond is one term.
* Joint exponent.  sum_d t in ascending d: (d - 1) u sum_d |t| on top of the terms' own: (G + d - 1) u sum_d A.
* Log-sum-exp.  m + log sum_j exp(e_j - m) is a convex combination's logarithm: moving every e_j by at most D moves it by at
  most D = max_j of the above.  Then, relative to S = sum exp(e_j - m) >= 1: the subtractions e_j - m add
  u sum_j p_j |e_j - m| <= u log N (p_j = exp(e_j - m) / S: the sum is H(p) - log S <= log N); every exp 4 u; N - 1 ordered
  additions of positive terms (N - 1) u; every tile merge one exp and three roundings, 8 u, ceil(N / T) of them.  The
  logarithm turns S's relative error into an absolute one and adds 4 u |log S| <= 4 u log N.  Rounded up:
  L = (N - 1) + 6 log N + 8 (1 + ceil(N / T)), in u.  The last additions (+ m, - log N, log N itself) 3 u (|result| + log N).
* Means (latent_information).  A mean is the exactly rounded sum of all its entries over B: the sum of the entries' bounds over
  B, + 2 u s for the rounding of the sum and of the division, s = sum |entries| / B >= |mean|; the restatement's own running
  sum in longdouble adds B 2^-64 s <= u s / 2 at the B <= 1024 used here.  Together: the mean bound + 3 u s.

Two conditions keep the bound honest: it may not exceed 1e-10 at any parity shape (asserted here and on the host), where a
component left out or counted twice moves a value by about 1 / N >= 1e-3; and the restatement itself satisfies it against float64
torch (the host file).  Every test prints the fraction of the bound it used; DESIGN 3.7g records the largest."""
import json
import math
import os

import numpy as np
import pytest
import torch

import latent_info_ref as ref

pytestmark = pytest.mark.gpu

U = ref.U
T = ref.TILE
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared cases are read-only)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.uint64)


@pytest.fixture(scope="module")
def ops():
    from evae import ops
    assert ops.agg_lse_tile() == T                        # the restatement's bound and the shapes below are built on it
    return ops


def call(ops, c, rows=True, **kw):
    return ops.agg_posterior_lse(dev(c['z']), dev(c['mean']), dev(c['log_var']), rows=dev(c['rows']) if rows else None, **kw)


def fraction(got, want, bound):
    got = host(got)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.max(np.abs(got - want) / bound))


def made(z, mean, log_var, rows):
    """a case from given arrays, in ref.case's layout"""
    c = dict(z=np.asarray(z, np.float32), mean=np.asarray(mean, np.float32), log_var=np.asarray(log_var, np.float32),
             rows=np.asarray(rows, np.int32))
    c['log_q'], c['log_qd'], c['log_cond'] = ref.agg_lse(c['z'], c['mean'], c['log_var'], c['rows'])
    c['bq'], c['bqd'], c['bc'] = ref.error_bounds(c['z'], c['mean'], c['log_var'], c['rows'], values=(c['log_q'], c['log_qd']))
    return c


def within(ops, c, what):
    out = call(ops, c)
    fr = [fraction(g, c[k], c[b]) for g, k, b in zip(out, ('log_q', 'log_qd', 'log_cond'), ('bq', 'bqd', 'bc'))]
    print("%s: bound <= %.3g, used %.3f / %.3f / %.3f (log_q / log_qd / log_cond)" % (what, max(c['bq'].max(), c['bqd'].max()), *fr))
    assert max(fr) <= 1.0
    return out


# ---------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("B,N,d", ref.SHAPES, ids=lambda v: str(v))
def test_parity_with_the_restatement(ops, B, N, d):
    c = ref.case(B, N, d)
    assert max(c['bq'].max(), c['bqd'].max(), c['bc'].max()) <= 1e-10
    out = within(ops, c, "B=%d N=%d d=%d" % (B, N, d))
    assert out.log_q.dtype == out.log_qd.dtype == out.log_cond.dtype == torch.float64
    assert out.log_q.shape == (B,) and out.log_qd.shape == out.log_cond.shape == (B, d)


# ---------------------------------------------------------------------------------------------- 2. every component once
def test_one_hot_every_component_is_seen(ops):
    """means 100 apart on a line, lv = 0, query j on mean j: log_q[j] = sum_d c_jd - log N; a skipped component reads ~ -5000"""
    N, d = 2 * T + 3, 3
    mean = np.zeros((N, d), np.float32)
    mean[:, 0] = 100.0 * np.arange(N)
    c = made(mean, mean, np.zeros((N, d), np.float32), np.arange(N))
    out = within(ops, c, "one-hot N=%d" % N)
    want = -d * HALF_LOG_2PI - math.log(N)
    assert np.abs(host(out.log_q) - want).max() <= c['bq'].max()
    assert np.abs(host(out.log_qd)[:, 1:] - (-HALF_LOG_2PI)).max() <= 2 * U * math.log(N) + 4 * U    # N equal terms off the line


@pytest.mark.parametrize("N", [T - 1, T, T + 1, 3 * T])
def test_equal_components_are_counted_exactly(ops, N):
    """N identical components: the sum is N exactly and log N cancels within 2 u log N; one component more or less shifts the
    value by log((N +- 1) / N) >= 1 / (3 T + 1)"""
    d, B = 5, 9
    rs = np.random.RandomState(N)
    mean = np.repeat((0.5 * rs.randn(1, d)).astype(np.float32), N, axis=0)
    log_var = np.repeat(rs.uniform(-3, 1, size=(1, d)).astype(np.float32), N, axis=0)
    z = (mean[:B] + rs.randn(B, d)).astype(np.float32)
    out = call(ops, dict(z=z, mean=mean, log_var=log_var, rows=np.zeros(B, np.int32)))
    term = host(out.log_cond)                                          # the single term, from the device itself
    # the cancellation, + the roundings of (m + log S) and of (. - log N)
    slack = 2 * U * math.log(N) + U * (2 * np.abs(term) + math.log(N))
    assert (np.abs(host(out.log_qd) - term) <= slack).all()
    # log_q against the device's own terms added in ascending d: the same additions, then the same cancellation
    joint, size = np.cumsum(term, axis=1)[:, -1], np.abs(term).sum(axis=1)
    assert (np.abs(host(out.log_q) - joint) <= 2 * U * math.log(N) + U * (2 * size + math.log(N)) + (d - 1) * U * size).all()
    assert fraction(out.log_cond, ref.agg_lse(z, mean, log_var, np.zeros(B, np.int32))[2],
                    ref.error_bounds(z, mean, log_var, np.zeros(B, np.int32))[2]) <= 1.0


# ---------------------------------------------------------------------------------------------- 3. range
def test_log_variances_from_minus_14_to_6(ops):
    rs = np.random.RandomState(5)
    N, d, B = 70, 40, 70
    mean = (0.5 * rs.randn(N, d)).astype(np.float32)
    log_var = rs.uniform(-14.0, 6.0, size=(N, d)).astype(np.float32)
    log_var[0, 0], log_var[1, 0] = -14.0, 6.0
    rows = np.arange(B) % N
    z = (mean[rows] + np.exp(0.5 * log_var[rows]) * rs.randn(B, d)).astype(np.float32)
    within(ops, made(z, mean, log_var, rows), "lv in [-14, 6]")


def test_one_component_ahead_by_more_than_745_nats(ops):
    """every other component underflows: the result is the winner's term minus log N"""
    N, d = 2 * T + 5, 2
    mean = np.zeros((N, d), np.float32)
    mean[:, 0] = 60.0 * (1 + np.arange(N))                             # >= 60 sigma from the query: 1800 nats behind
    mean[T + 3] = 0.0
    z = np.zeros((4, d), np.float32)
    c = made(z, mean, np.zeros((N, d), np.float32), np.full(4, T + 3))
    out = within(ops, c, "one component ahead")
    assert np.abs(host(out.log_q) - (-d * HALF_LOG_2PI - math.log(N))).max() <= c['bq'].max()
    assert np.abs(host(out.log_qd)[:, 0] - (-HALF_LOG_2PI - math.log(N))).max() <= c['bqd'].max()


def test_queries_ten_thousand_sigma_away(ops):
    rs = np.random.RandomState(6)
    N, d = T + 9, 7
    mean, log_var = (0.5 * rs.randn(N, d)).astype(np.float32), rs.uniform(-3, 1, size=(N, d)).astype(np.float32)
    z = (1.0e4 * np.exp(0.5 * 1.0) * np.sign(rs.randn(6, d)) + rs.randn(6, d)).astype(np.float32)
    c = made(z, mean, log_var, np.arange(6))
    out = within(ops, c, "10^4 sigma away")
    assert np.isfinite(host(out.log_q)).all() and (host(out.log_q) < -1e7).all()


# ---------------------------------------------------------------------------------------------- 4. bits
def test_bits(ops):
    c = ref.case(65, 257, 65)
    z, mean, log_var, rows = (dev(c[k]) for k in ('z', 'mean', 'log_var', 'rows'))
    first = ops.agg_posterior_lse(z, mean, log_var, rows=rows)
    again = ops.agg_posterior_lse(z, mean, log_var, rows=rows)
    for a, b in zip(first, again):
        assert np.array_equal(bits(a), bits(b))
    # a row alone is the row in the batch
    for i in (0, 31, 63, 64):
        one = ops.agg_posterior_lse(z[i:i + 1].contiguous(), mean, log_var, rows=rows[i:i + 1].contiguous())
        for a, b in zip(first, one):
            assert np.array_equal(bits(a)[i:i + 1], bits(b))
    # a permuted batch gives the permuted outputs
    perm = torch.from_numpy(np.random.RandomState(2).permutation(65)).cuda()
    moved = ops.agg_posterior_lse(z[perm].contiguous(), mean, log_var, rows=rows[perm].contiguous())
    for a, b in zip(first, moved):
        assert np.array_equal(bits(a[perm]), bits(b))
    # outputs switched off one by one leave the others as they were
    for kw in (dict(rows=None), dict(rows=rows, joint=False), dict(rows=rows, per_dimension=False), dict(rows=None, joint=False),
               dict(rows=None, per_dimension=False), dict(rows=rows, joint=False, per_dimension=False)):
        part = ops.agg_posterior_lse(z, mean, log_var, **kw)
        on = (kw.get('joint', True), kw.get('per_dimension', True), kw['rows'] is not None)
        for a, b, wanted in zip(first, part, on):
            assert (b is not None) == wanted
            if wanted:
                assert np.array_equal(bits(a), bits(b))


def test_a_nan_query_stays_in_its_row(ops):
    c = ref.case(17, 63, 40)
    z = np.array(c['z'])
    z[5, 7] = np.nan
    out = ops.agg_posterior_lse(dev(z), dev(c['mean']), dev(c['log_var']), rows=dev(c['rows']))
    clean = call(ops, c)
    assert np.isnan(host(out.log_q)[5]) and np.isnan(host(out.log_qd)[5, 7]) and np.isnan(host(out.log_cond)[5, 7])
    keep = np.ones((17, 40), bool)
    keep[5, 7] = False
    assert np.array_equal(bits(out.log_qd)[keep], bits(clean.log_qd)[keep])
    assert np.array_equal(bits(out.log_cond)[keep], bits(clean.log_cond)[keep])
    assert np.array_equal(np.delete(bits(out.log_q), 5), np.delete(bits(clean.log_q), 5))


# ---------------------------------------------------------------------------------------------- 5. latent_information
SCALARS = ('mutual_information', 'total_correlation', 'dimension_wise_kl', 'entropy_aggregate')


def info_bounds(c, log_prior=None):
    """the bound of every key of latent_information at case c, propagated through the means (module docstring)"""
    B, d = c['z'].shape
    z = c['z'].astype(np.float64)
    std = HALF_LOG_2PI + 0.5 * z * z
    b_std = 4 * U * std                                    # the square, the halving (exact), the subtraction, on both sides
    cond, qd, q = np.abs(c['log_cond']), np.abs(c['log_qd']), np.abs(c['log_q'])
    assert B <= 1024

    def mean_of(err, size):
        return float(err.mean() + 3 * U * size.mean())

    extra = {}
    if log_prior is not None:                              # given exactly: only the means round
        lp = np.abs(log_prior)
        extra = {'kl': mean_of(c['bc'].sum(1), cond.sum(1) + lp), 'marginal_kl': mean_of(c['bq'], q + lp)}
    return {
        **extra,
        'mutual_information': mean_of(c['bc'].sum(1) + c['bq'], cond.sum(1) + q),
        'total_correlation': mean_of(c['bq'] + c['bqd'].sum(1), q + qd.sum(1)),
        'dimension_wise_kl': mean_of((c['bqd'] + b_std).sum(1), (qd + std).sum(1)),
        'entropy_aggregate': mean_of(c['bq'], q),
        'mutual_information_per_dimension': (c['bc'] + c['bqd']).mean(0) + 3 * U * (cond + qd).mean(0),
        'kl_per_dimension': (c['bqd'] + b_std).mean(0) + 3 * U * (qd + std).mean(0),
    }


@pytest.mark.parametrize("B,N,d", [(17, 63, 40), (300, 7, 3), (65, 257, 65)], ids=lambda v: str(v))
def test_latent_information_of_given_draws(B, N, d):
    from evae.latent_info import latent_information
    c = ref.case(B, N, d)
    want = ref.latent_information(c['mean'], c['log_var'], c['z'], c['rows'])
    got = latent_information(dev(c['mean']), dev(c['log_var']), z=dev(c['z']), rows=dev(c['rows']))
    bound = info_bounds(c)
    for k in SCALARS:
        assert isinstance(got[k], float)
        print("%s: %.12g, off by %.3g of a bound of %.3g" % (k, got[k], abs(got[k] - want[k]), bound[k]))
        assert abs(got[k] - want[k]) <= bound[k]
    for k in ('mutual_information_per_dimension', 'kl_per_dimension'):
        assert got[k].is_cuda and got[k].dtype == torch.float64 and got[k].shape == (d,)
        assert (np.abs(host(got[k]) - want[k]) <= bound[k]).all()
    assert got['log_n'] == math.log(N) and got['n'] == B and got['z_size'] == d
    assert got['active_units'] == want['active_units'] == int((np.var(c['mean'], axis=0) > 0.01).sum())
    margin = np.abs(want['mutual_information_per_dimension'] - 0.01).min()
    assert margin > bound['mutual_information_per_dimension'].max()    # no dimension sits on the threshold
    assert got['active_units_by_information'] == want['active_units_by_information']
    assert 0.0 <= got['mutual_information'] <= math.log(N) + bound['mutual_information']


def test_latent_information_draws_its_own_z():
    from evae.latent_info import aggregate_posterior_log_density, draw_posterior_samples, latent_information
    c = ref.case(17, 63, 40)
    mean, log_var = dev(c['mean']), dev(c['log_var'])
    for kw in (dict(), dict(n_samples=30), dict(rows=np.array([5, 5, 0, 62]))):
        want_z, want_rows = ref.draws(c['mean'], c['log_var'], random_state=11, **kw)
        if 'rows' in kw:
            kw = dict(rows=dev(kw['rows']))
        z, rows = draw_posterior_samples(mean, log_var, random_state=11, **kw)
        assert z.dtype == torch.float32 and rows.dtype == torch.int32 and z.is_cuda and rows.is_cuda
        assert np.array_equal(host(rows), want_rows) and np.array_equal(host(z).view(np.uint32), want_z.view(np.uint32))
        got = latent_information(mean, log_var, random_state=11, **kw)
        assert np.array_equal(host(got['z']), want_z) and np.array_equal(host(got['rows']), want_rows)
        want = ref.latent_information(c['mean'], c['log_var'], want_z, want_rows)
        bound = info_bounds(made(want_z, c['mean'], c['log_var'], want_rows))
        for k in SCALARS:
            assert abs(got[k] - want[k]) <= bound[k]
    assert len(set(host(draw_posterior_samples(mean, log_var, n_samples=30, random_state=11)[1]).tolist())) == 30
    # the density alone
    log_q, log_qd = aggregate_posterior_log_density(dev(c['z']), mean, log_var, per_dimension=True)
    assert fraction(log_q, c['log_q'], c['bq']) <= 1.0 and fraction(log_qd, c['log_qd'], c['bqd']) <= 1.0
    assert np.array_equal(bits(aggregate_posterior_log_density(dev(c['z']), mean, log_var)), bits(log_q))


def test_a_single_component_carries_nothing():
    from evae.latent_info import latent_information
    c = ref.case(3, 1, 40)
    got = latent_information(dev(c['mean']), dev(c['log_var']), z=dev(c['z']), rows=dev(c['rows']))
    bound = info_bounds(c)
    assert abs(got['mutual_information']) <= bound['mutual_information'] and got['log_n'] == 0.0
    assert abs(got['total_correlation']) <= bound['total_correlation']
    assert got['active_units'] == 0 and got['active_units_by_information'] == 0


def test_kl_splits_into_information_and_marginal_kl():
    from evae.latent_info import latent_information
    c = ref.case(65, 257, 65)
    log_prior = -HALF_LOG_2PI * 65 - 0.5 * (c['z'].astype(np.float64) ** 2).sum(axis=1)          # a standard-normal prior
    want = ref.latent_information(c['mean'], c['log_var'], c['z'], c['rows'], log_prior=log_prior)
    bound = info_bounds(c, log_prior)
    for lp in (dev(log_prior), dev(log_prior.astype(np.float32))):
        got = latent_information(dev(c['mean']), dev(c['log_var']), z=dev(c['z']), rows=dev(c['rows']), log_prior=lp)
        gap = got['kl'] - (got['mutual_information'] + got['marginal_kl'])
        print("kl %.12g = %.12g + %.12g, gap %.3g" % (got['kl'], got['mutual_information'], got['marginal_kl'], gap))
        assert abs(gap) <= 4 * U * max(abs(got['kl']), 1.0)
    # the float32 prior last: its own rounding (2^-24 of each value) and nothing more
    assert abs(got['kl'] - want['kl']) <= 2.0 ** -24 * np.abs(log_prior).mean() + bound['kl']
    got = latent_information(dev(c['mean']), dev(c['log_var']), z=dev(c['z']), rows=dev(c['rows']), log_prior=dev(log_prior))
    for k in ('kl', 'marginal_kl'):
        assert abs(got[k] - want[k]) <= bound[k]


# ---------------------------------------------------------------------------------------------- 6. interface
def test_refusals(ops):
    from evae import _lib
    from evae._lib import EvaeError
    from evae.latent_info import latent_information
    refused = (ValueError, EvaeError)
    c = ref.case(17, 63, 40)
    z, mean, log_var, rows = (dev(c[k]) for k in ('z', 'mean', 'log_var', 'rows'))
    wide = torch.zeros((4, 257), device="cuda")
    bad_rows = rows.clone()
    bad_rows[3] = 63
    neg_rows = rows.clone()
    neg_rows[0] = -1
    for bad in (lambda: ops.agg_posterior_lse(wide, wide, wide),                                   # d = 257
                lambda: ops.agg_posterior_lse(z, mean[:0], log_var[:0]),                           # N = 0
                lambda: ops.agg_posterior_lse(z[:0], mean, log_var),                               # B = 0
                lambda: ops.agg_posterior_lse(z[:, ::2], mean[:, ::2], log_var[:, ::2]),           # strided
                lambda: ops.agg_posterior_lse(z.double(), mean, log_var), lambda: ops.agg_posterior_lse(z, mean.double(), log_var),
                lambda: ops.agg_posterior_lse(z, mean, log_var.double()),
                lambda: ops.agg_posterior_lse(z, mean, log_var[:-1]), lambda: ops.agg_posterior_lse(z[:, :39].contiguous(), mean, log_var),
                lambda: ops.agg_posterior_lse(z[0], mean, log_var),
                lambda: ops.agg_posterior_lse(z, mean, log_var, rows=bad_rows), lambda: ops.agg_posterior_lse(z, mean, log_var, rows=neg_rows),
                lambda: ops.agg_posterior_lse(z, mean, log_var, rows=rows.long()), lambda: ops.agg_posterior_lse(z, mean, log_var, rows=rows[:-1]),
                lambda: ops.agg_posterior_lse(z, mean, log_var, joint=False, per_dimension=False),  # nothing asked for
                lambda: ops.agg_posterior_lse(z.cpu(), mean, log_var), lambda: ops.agg_posterior_lse(z, mean, log_var, rows=rows.cpu()),
                lambda: latent_information(mean, log_var, z=z[:5]),                                 # whose draws?
                lambda: latent_information(mean, log_var, z=z, rows=bad_rows), lambda: latent_information(mean, log_var, n_samples=64),
                lambda: latent_information(mean, log_var, n_samples=0), lambda: latent_information(mean.cpu(), log_var.cpu()),
                lambda: latent_information(mean, log_var, z=z, rows=rows, log_prior=torch.zeros(16, device="cuda"))):
        with pytest.raises(refused):
            bad()
    # the entry point's own checks, under the operator's: every pointer is a live buffer of the right size, nothing is launched
    lib, vp = _lib.load(), _lib.vp
    B, N, d = 17, 63, 40
    log_q = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    log_qd, log_cond = (torch.full((B, d), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    ws = torch.empty(lib.evae_agg_lse_workspace_bytes(B, N, d), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= 3 * 8 * N * d and lib.evae_agg_lse_workspace_bytes(B, N, 257) == 0
    assert lib.evae_agg_lse_max_features() == 256 and lib.evae_agg_lse_max_points() == 1 << 20

    def raw(B=B, N=N, d=d, z=z, rows=rows, log_q=log_q, log_qd=log_qd, log_cond=log_cond, ws_bytes=None):
        return lib.evae_agg_lse(vp(z), B, vp(mean), vp(log_var), N, d, vp(rows), vp(log_q), vp(log_qd), vp(log_cond), vp(ws),
                                ws.numel() if ws_bytes is None else ws_bytes, None)

    for attempt, word in ((lambda: raw(d=257), b"257 features"), (lambda: raw(d=0), b"0 features"), (lambda: raw(N=0), b"N=0"),
                          (lambda: raw(B=0), b"B=0"), (lambda: raw(N=(1 << 20) + 1), b"N=1048577"), (lambda: raw(rows=None), b"without rows"),
                          (lambda: raw(log_q=None, log_qd=None, log_cond=None), b"no output"), (lambda: raw(z=None), b"null pointer"),
                          (lambda: raw(ws_bytes=ws.numel() - 1), b"workspace")):
        assert attempt() != 0
        assert word in lib.evae_last_error(), word
    torch.cuda.synchronize()
    assert bool((log_q == -7.0).all()) and bool((log_qd == -7.0).all()) and bool((log_cond == -7.0).all())   # a refused call wrote nothing
    assert raw() == 0
    assert fraction(log_q, c['log_q'], c['bq']) <= 1.0 and fraction(log_cond, c['log_cond'], c['bc']) <= 1.0
    # the kernel's own guard under the operator's check: a row outside [0, N) reads nothing and gives NaN, there and only there
    assert raw(rows=bad_rows, log_q=None, log_qd=None) == 0
    got = host(log_cond)
    assert np.isnan(got[3]).all() and np.isfinite(np.delete(got, 3, axis=0)).all()


# ---------------------------------------------------------------------------------------------- 7. the report
def test_report_on_a_stub_model(tmp_path, capsys):
    import evae_oracle as orc
    import smoke_case
    import golden_inputs as gi
    from utils.latent_info_on_latent import report_latent_information
    B = 32
    args = smoke_case.vae_args(number_components=20, training_set_size=200, batch_size=B)
    args.seed = 14
    model, _ = smoke_case.build_model(torch, np, orc, args)
    model.eval()

    def loader(seed, n):
        data = torch.from_numpy(gi.binary_images(seed, n))
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, torch.arange(n) % 10), batch_size=B, shuffle=False)

    train, test = loader(91, 200), loader(92, 100)                    # 96 test rows in full batches
    first, second = str(tmp_path / "a"), str(tmp_path / "b")
    report = report_latent_information(train, test, model, first, args)
    assert "latent information of 96 test posteriors, z = 40" in capsys.readouterr().out
    names = ["latent_information.json", "latent_information_per_dimension.npy"]
    assert sorted(os.listdir(first)) == names
    with open(os.path.join(first, names[0])) as f:
        saved = json.load(f)
    assert saved == report
    assert sorted(saved) == sorted(['mutual_information', 'total_correlation', 'dimension_wise_kl', 'entropy_aggregate', 'log_n',
                                    'active_units', 'active_units_by_information', 'kl', 'marginal_kl', 'n', 'z_size', 'split'])
    assert saved['n'] == 96 and saved['z_size'] == 40 and saved['split'] == 'test' and saved['log_n'] == math.log(96)
    per_dimension = np.load(os.path.join(first, names[1]))
    assert per_dimension.shape == (2, 40) and per_dimension.dtype == np.float64 and np.isfinite(per_dimension).all()
    assert abs(saved['kl'] - (saved['mutual_information'] + saved['marginal_kl'])) <= 4 * U * max(abs(saved['kl']), 1.0)
    assert all(math.isfinite(saved[k]) for k in SCALARS) and saved['mutual_information'] <= saved['log_n'] + 1e-9
    # the same seed again: the same files, byte for byte
    report_latent_information(train, test, model, second, args)
    for name in names:
        with open(os.path.join(first, name), 'rb') as f, open(os.path.join(second, name), 'rb') as g:
            assert f.read() == g.read()
    # the training split on request
    args.latent_info_split = 'train'
    assert report_latent_information(train, test, model, str(tmp_path / "c"), args)['n'] == 192
    args.latent_info_split = 'validation'
    with pytest.raises(ValueError):
        report_latent_information(train, test, model, str(tmp_path / "d"), args)
