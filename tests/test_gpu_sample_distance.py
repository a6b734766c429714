"""GPU: the kernel-sum entry points (csrc/evae_kernel_sum.hip), evae.ops.kernel_row_sums / ordered_sum / sym_congruence,
evae.sample_quality's frechet_distance, kernel_mmd and kernel_inception_distance, and the report's new keys, against the
longdouble restatement tests/sample_distance_ref.py (held to float64 numpy, scikit-learn and scipy, within the bounds used here
and on the inputs used here, by tests/test_sample_distance_ref_host.py).

The yardstick is always the restatement, never the code under test.  Its own error (a 64-bit mantissa) is 2^-11 of float64's.
The tolerances are bounds from the arithmetic, u = 2^-53; ref.error_bounds_rows, ref.error_bounds_congruence and
ref.error_bounds_frechet compute them per quantity and carry the derivations.  In short:

* A kernel term.  fp32 entries and their products are exact in fp64.  The dot product over d: (d + 1) u sum |q| |c|; gamma, coef0
  and the power: 2 u and 2 degree u relative, the argument's error propagated; the RBF exponent (d + 4) u relative, exp at
  2 ulp.  A row sum adds (N - 1 + ceil(N / T)) u sum |terms| for the ordered additions and the tile merges, a total (B - 1) u.
* The congruence A S A^T: 2 d u (|A| |S| |A|^T) elementwise.
* The square root's trace sum_i sqrt nu_i, nu the spectrum of C = A S_f A^T with A^T A = S_r.  No figure is fixed in advance.
  Whatever eigenvectors V' the device's solver returns, A' S_f A'^T has the non-zero spectrum of (A'^T A') S_f, so the pipeline
  is exact for a perturbed S_r' = A'^T A'.  The perturbations add up to E (Frobenius norm of the equivalent symmetric
  perturbation of a matrix with the spectrum nu): the moments' (2 N + 8) u, pca_eigh's documented stop at 2^-52 |g_p| |g_q|
  (off-diagonal mass <= u tr S) with at most evae_pca_max_sweeps() = 64 sweeps of d - 1 rotations per column at 4 u each, the
  congruence's 2 d u, and the second eigen-solve likewise (twice: the restatement's eigvalsh).  By Weyl and Hoffman-Wielandt
  sum_i |nu_i' - nu_i| <= sqrt(d) E, and |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b): the eigenvalues known to be
  >= nu_min > 16 E move sum sqrt nu by at most sqrt(d) E / sqrt(nu_min - E); an eigenvalue below that (the rank-deficient set:
  0 up to E, where the solver clamps) by at most sqrt(E + nu).  nu_min is a property of the test matrices -- the sets are
  built well conditioned so that it is ~ 0.05 -- and is taken from the restatement's spectrum, never from the device.  The
  sweep count is the solver's compile-time cap, not what a run took, so the bound is loose by the factor the solver stops early:
  the fractions printed below say by how much.

Two conditions keep the bounds honest: no bound of a row sum or a total may exceed 1e-9 of the value at any parity shape
(asserted here and on the host), where a pair left out or counted twice moves a total by at least 1 / (B N) >= 1e-6 of it; and
the restatement itself satisfies the bounds against second evaluations (the host file).  Every test prints the fraction of the
bound it used; DESIGN 3.7h records the largest."""
import functools
import json
import operator
import os
import warnings

import numpy as np
import pytest
import torch

import sample_distance_ref as ref

pytestmark = pytest.mark.gpu

U = ref.U
T = ref.TILE
POLY = dict(kind='poly', gamma=None, coef0=1.0, degree=3)
RBF = dict(kind='rbf', gamma=None)
KINDS = [POLY, RBF]
IDS = ['poly', 'rbf']
QUERIES = ("_max_features", "_max_points", "_max_degree", "_max_sweeps", "_max_neighbours", "_tile", "_workspace_bytes", "_chunk_rows",
           "evae_last_error", "evae_version")


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared cases are read-only)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.uint64)


@pytest.fixture(scope="module")
def ops():
    from evae import ops
    assert ops.kernel_sum_tile() == T and ops.pca_max_sweeps() == ref.MAX_SWEEPS      # the bounds and the shapes are built on them
    assert ops.kernel_sum_max_features() == 256 and ops.kernel_sum_max_points() == 1 << 20
    return ops


@pytest.fixture(scope="module")
def sq(ops):
    from evae import sample_quality
    return sample_quality


def launches(counts):
    """the entry points of a count_calls record that launch something"""
    return sorted(n for n in counts if not n.endswith(QUERIES))


# ---------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("skip_self", [False, True], ids=['all', 'skip_self'])
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
@pytest.mark.parametrize("B,N,d", ref.parity_shapes(), ids=lambda v: str(v))
def test_row_sums_and_totals_against_the_restatement(ops, B, N, d, kw, skip_self):
    q, c = ref.rows_case(B, B if skip_self else N, d)
    c = q if skip_self else c
    want, tot = ref.row_sums(q, c, skip_self=skip_self, **kw), ref.total(q, c, skip_self=skip_self, **kw)
    rb, tb = ref.error_bounds_rows(q, c, skip_self=skip_self, **kw)
    got = ops.kernel_row_sums(dev(q), dev(c), skip_self=skip_self, **kw)
    assert got.dtype == torch.float64 and got.shape == (B,)
    g, gt = host(got), float(ops.ordered_sum(got))
    if B == 1 and skip_self:
        assert g[0] == 0.0 and gt == 0.0                               # nothing is left of a single row
        return
    assert (rb <= 1e-9 * want).all() and tb <= 1e-9 * tot
    fr, ft = float(np.max(np.abs(g - want) / rb)), abs(gt - tot) / tb
    print("B=%d N=%d d=%d %s%s: bound <= %.3g of the value, used %.3f (rows) / %.3f (total)"
          % (B, len(c), d, kw['kind'], " skip_self" if skip_self else "", float(np.max(rb / want)), fr, ft))
    assert np.isfinite(g).all() and fr <= 1.0 and ft <= 1.0


@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_unaligned_rows_of_odd_width(ops, kw):
    """a slice from row 1 of a [. x 7] tensor: the row pointers are 4-byte aligned and no more"""
    q, c = ref.rows_case(70, T + 6, 7)
    dq, dc = dev(q)[1:], dev(c)[1:]
    assert dq.is_contiguous() and dq.data_ptr() % 8 == 4 and dc.data_ptr() % 8 == 4
    want = ref.row_sums(q[1:], c[1:], **kw)
    rb = ref.error_bounds_rows(q[1:], c[1:], **kw)[0]
    fr = float(np.max(np.abs(host(ops.kernel_row_sums(dq, dc, **kw)) - want) / rb))
    print("unaligned d=7 %s: used %.3f" % (kw['kind'], fr))
    assert fr <= 1.0


# ---------------------------------------------------------------------------------------------- 2. every pair once
def test_one_hot_every_pair_is_counted_once(ops):
    """q_i = e_i, c_j = (j + 1) e_j, the linear kernel: row_sum[i] = i + 1 exactly; a skipped column reads 0, a doubled one twice"""
    N = 2 * T + 3
    assert N <= ops.kernel_sum_max_features()
    q = np.eye(N, dtype=np.float32)
    c = (np.eye(N) * np.arange(1, N + 1)).astype(np.float32)
    lin = dict(kind='poly', gamma=1.0, coef0=0.0, degree=1)
    assert np.array_equal(host(ops.kernel_row_sums(dev(q), dev(c), **lin)), np.arange(1, N + 1, dtype=np.float64))
    assert np.array_equal(host(ops.kernel_row_sums(dev(c), dev(q), **lin)), np.arange(1, N + 1, dtype=np.float64))
    assert np.array_equal(host(ops.kernel_row_sums(dev(c), dev(c), skip_self=True, **lin)), np.zeros(N))
    # all ones against integer rows, B != N: every column of every tile, a partial last tile included
    ones, cols = np.ones((5, N), np.float32), np.tile(np.arange(1, 3 * T + 8, dtype=np.float32)[:, None], (1, N))
    assert np.array_equal(host(ops.kernel_row_sums(dev(ones), dev(cols), **lin)), np.full(5, N * cols[:, 0].sum(), np.float64))


def test_skip_self_goes_by_index(ops):
    rs = np.random.RandomState(3)
    x = rs.uniform(-0.9, 0.9, size=(T + 9, 6)).astype(np.float32)
    x[7] = x[2]                                                        # a duplicate at i != j is still counted
    x[T + 1] = x[2]
    for kw in KINDS:
        full, skip = host(ops.kernel_row_sums(dev(x), dev(x), **kw)), host(ops.kernel_row_sums(dev(x), dev(x), skip_self=True, **kw))
        want = ref.row_sums(x, x, skip_self=True, **kw)
        rb = ref.error_bounds_rows(x, x, skip_self=True, **kw)[0]
        assert (np.abs(skip - want) <= rb).all()
        diag = ref.row_sums(x, x, **kw) - want                         # k(x_i, x_i): for rbf 1, the value the duplicates share
        assert (np.abs((full - skip) - diag) <= rb + ref.error_bounds_rows(x, x, **kw)[0]).all()
    # The diagonal's value is shared by other columns: under the rbf kernel k(x_2, x_2) = k(x_2, x_7) = k(x_2, x_{T+1}) = 1.
    # Rows 2, 7 and T + 1 each lose ONE of the three ones -- their own, whichever tile it sits in -- and keep the other two.
    sk = host(ops.kernel_row_sums(dev(x), dev(x), skip_self=True, **RBF))
    rb = ref.error_bounds_rows(x, x, skip_self=True, **RBF)[0]
    others = np.delete(np.arange(len(x)), [2, 7, T + 1])
    k_rest = float(ref.kernel_matrix(x[[2]], x[others], **RBF).sum())
    for i in (2, 7, T + 1):
        assert abs(sk[i] - (k_rest + 2.0)) <= rb[i]


# ---------------------------------------------------------------------------------------------- 3. bits
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
def test_a_rows_bits_do_not_depend_on_the_batch(ops, kw):
    q, c = ref.rows_case(257, 2 * T + 3, 40)
    dq, dc = dev(q), dev(c)
    whole = bits(ops.kernel_row_sums(dq, dc, **kw))
    assert np.array_equal(whole, bits(ops.kernel_row_sums(dq, dc, **kw)))                       # a second run
    assert np.array_equal(whole[100:103], bits(ops.kernel_row_sums(dq[100:103].clone(), dc, **kw)))   # alone
    moved = torch.cat((dq[100:103], dq[:70]), dim=0)                                             # another place, another grid
    assert np.array_equal(np.concatenate((whole[100:103], whole[:70])), bits(ops.kernel_row_sums(moved, dc, **kw)))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 256 + 1])
def test_ordered_sum_is_the_left_to_right_sum(ops, n):
    x = np.random.RandomState(n).randn(n) * 10.0 ** np.random.RandomState(n + 1).randint(-6, 6, n)
    want = functools.reduce(operator.add, x.tolist())                  # Python floats: float64, left to right
    got = ops.ordered_sum(dev(x))
    assert got.dim() == 0 and got.dtype == torch.float64
    assert np.float64(want).view(np.uint64) == bits(got.reshape(1))[0]


# ---------------------------------------------------------------------------------------------- 4. the congruence
@pytest.mark.parametrize("d", [1, 2, 17, 96, 97, 256])
def test_sym_congruence(ops, d):
    rs = np.random.RandomState(d)
    A = rs.randn(d, d)
    S = rs.randn(d, d)
    S = S @ S.T / d
    S = (S + S.T) / 2
    got = ops.sym_congruence(dev(A), dev(S))
    want = (A.astype(ref.LD) @ S.astype(ref.LD) @ A.T.astype(ref.LD)).astype(np.float64)
    fr = float(np.max(np.abs(host(got) - want) / ref.error_bounds_congruence(A, S)))
    print("sym_congruence d=%d: used %.3f" % (d, fr))
    assert fr <= 1.0
    assert np.array_equal(bits(got), bits(got.t().contiguous()))       # symmetric bit for bit
    assert np.array_equal(bits(ops.sym_congruence(dev(np.eye(d)), dev(S))), S.view(np.uint64))


# ---------------------------------------------------------------------------------------------- 5. non-finite inputs
def test_non_finite_inputs_stay_where_they_are(ops):
    q, c = ref.rows_case(65, T, 7)
    for kw in KINDS:
        clean = bits(ops.kernel_row_sums(dev(q), dev(c), **kw))
        bad = np.array(q)
        bad[13, 3] = np.nan
        got = ops.kernel_row_sums(dev(bad), dev(c), **kw)
        torch.cuda.synchronize()
        g = host(got)
        assert np.isnan(g[13]) and np.isfinite(np.delete(g, 13)).all()
        assert np.array_equal(np.delete(bits(got), 13), np.delete(clean, 13))
        bad[13, 3] = np.inf
        g = host(ops.kernel_row_sums(dev(bad), dev(c), **kw))
        torch.cuda.synchronize()
        assert not np.isfinite(g[13]) if kw['kind'] == 'poly' else g[13] == 0.0
        assert np.array_equal(np.delete(g, 13).view(np.uint64), np.delete(clean, 13))
        cols = np.array(c)
        cols[5, 0] = np.inf                                            # a column is every row's: no fault, nothing else asked
        ops.kernel_row_sums(dev(q), dev(cols), **kw)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 6. the Frechet distance
def check_frechet(got, fr, fb, what):
    used = {k: abs(got[k] - fr[k]) / fb[k] for k in ("mean_term", "trace_term", "frechet_distance")}
    print("%s: bounds %.3g / %.3g / %.3g, used %.3g / %.3g / %.3g (mean / trace / distance); E = %.3g, nu_min = %.3g, %d small"
          % (what, fb['mean_term'], fb['trace_term'], fb['frechet_distance'], used['mean_term'], used['trace_term'],
             used['frechet_distance'], fb['e_total'], fb['nu_min'], fb['small']))
    assert max(used.values()) <= 1.0
    assert got['eigh_converged'] is True


@pytest.mark.parametrize("name", ["small", "mid", "wide", "rank"])
def test_frechet_distance_against_the_restatement(sq, name):
    c = ref.distance_case(name)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = sq.frechet_distance(dev(c['real']), dev(c['fake']))
    assert sorted(got) == sorted(["frechet_distance", "mean_term", "trace_term", "n_real", "n_fake", "eigh_converged"])
    assert (got['n_real'], got['n_fake']) == (len(c['real']), len(c['fake']))
    assert got['frechet_distance'] == got['mean_term'] + got['trace_term']
    check_frechet(got, c['frechet'], c['fb'], name)
    assert (c['fb']['small'] > 0) == (name == "rank")


def test_frechet_distance_of_identical_and_translated_sets(sq):
    real = ref.distance_case('small')['real']
    same = sq.frechet_distance(dev(real), dev(real))
    fb = ref.error_bounds_frechet(real, real)
    print("identical: |FD| = %.3g, bound %.3g" % (abs(same['frechet_distance']), fb['frechet_distance']))
    assert same['mean_term'] == 0.0 and abs(same['frechet_distance']) <= fb['frechet_distance'] and same['eigh_converged'] is True
    # a translation that fp32 carries exactly: values on a 2^-10 grid
    grid = (np.round(real * 1024.0) / 1024.0).astype(np.float32)
    t = np.array([0.5, -1.25, 2.0, 0.0, 3.0 / 1024.0], np.float32)
    moved = grid + t
    assert np.array_equal(moved.astype(np.float64), grid.astype(np.float64) + t.astype(np.float64))
    got = sq.frechet_distance(dev(grid), dev(moved))
    fb = ref.error_bounds_frechet(grid, moved)
    want = float((t.astype(np.float64) ** 2).sum())
    print("translated: mean_term off by %.3g of its bound, trace_term %.3g of its bound"
          % (abs(got['mean_term'] - want) / fb['mean_term'], abs(got['trace_term']) / fb['trace_term']))
    assert abs(got['mean_term'] - want) <= fb['mean_term'] and abs(got['trace_term']) <= fb['trace_term']
    assert got['eigh_converged'] is True


# ---------------------------------------------------------------------------------------------- 7. kernel MMD
@pytest.mark.parametrize("kw", KINDS, ids=IDS)
@pytest.mark.parametrize("name,biased", [("small", False), ("mid", False), ("wide", False), ("rank", False), ("small", True)])
def test_kernel_mmd_against_the_restatement(sq, name, kw, biased):
    c, m = ref.distance_case(name), ref.mmd_case(name, kw['kind'], biased=biased)
    got = sq.kernel_mmd(dev(c['real']), dev(c['fake']), kernel=kw['kind'], biased=biased)
    assert sorted(got) == sorted(["mmd2", "k_rr", "k_ff", "k_rf", "kernel", "gamma", "n_real", "n_fake"])
    N, M = len(c['real']), len(c['fake'])
    assert (got['kernel'], got['gamma'], got['n_real'], got['n_fake']) == (kw['kind'], 1.0 / c['real'].shape[1], N, M)
    div = (N * N if biased else N * (N - 1), M * M if biased else M * (M - 1), N * M)
    used = [abs(got[k] - m[k]) / (tb / dv + U * abs(m[k])) for k, tb, dv in zip(("k_rr", "k_ff", "k_rf"), m['bounds'], div)]
    used.append(abs(got['mmd2'] - m['mmd2']) / m['bound'])
    print("%s %s %s: mmd2 = %.6g, bound %.3g, used %.3f / %.3f / %.3f / %.3f (rr / ff / rf / mmd2)"
          % (name, kw['kind'], "biased" if biased else "unbiased", m['mmd2'], m['bound'], *used))
    assert max(used) <= 1.0
    if kw == POLY and not biased:
        assert sq.kernel_inception_distance(dev(c['real']), dev(c['fake'])) == got['mmd2']


def test_biased_and_unbiased_differ_by_the_diagonal(sq):
    c = ref.distance_case('small')
    N, M = len(c['real']), len(c['fake'])
    b, u = (sq.kernel_mmd(dev(c['real']), dev(c['fake']), biased=f) for f in (True, False))
    rb, ru = ref.mmd_case('small', biased=True), ref.mmd_case('small')
    for k, s, x, n, i in (("k_rr", "s_rr", c['real'], N, 0), ("k_ff", "s_ff", c['fake'], M, 1)):
        diff = b[k] * (n * n) - u[k] * (n * (n - 1))
        tol = rb['bounds'][i] + ru['bounds'][i] + 4 * U * rb[s]
        assert abs(diff - ref.diagonal_sum(x)) <= tol
    assert b['k_rf'] == u['k_rf']


def test_median_gamma(sq):
    for name in ("small", "mid"):
        real, fake = (ref.distance_case(name)[k] for k in ('real', 'fake'))
        want = ref.median_gamma(real)
        gamma, rows = sq.median_gamma(dev(real))
        assert rows == len(real) and gamma == want
    got = sq.kernel_mmd(dev(real), dev(fake), kernel='rbf', gamma='median')
    assert got['gamma'] == want
    m = ref.kernel_mmd(real, fake, 'rbf', want)
    assert abs(got['mmd2'] - m['mmd2']) <= m['bound']
    assert sq.MEDIAN_ROWS == ref.MEDIAN_ROWS == 2048
    assert "subsample" in sq.kernel_mmd.__doc__


# ---------------------------------------------------------------------------------------------- 8. sample_quality and the report
def test_sample_quality_with_distances(ops, sq, monkeypatch):
    from evae import _lib
    c = ref.distance_case('small')
    real, fake = dev(c['real']), dev(c['fake'])
    train = dev(ref.gaussian_sets(N=200, M=8, d=5, seed=9)[0])
    called = []
    for name in ("kernel_row_sums", "ordered_sum", "sym_congruence", "pca_moments", "pca_eigh"):
        def wrapper(*a, _fn=getattr(ops, name), _name=name, **kw):
            called.append(_name)
            return _fn(*a, **kw)
        monkeypatch.setattr(ops, name, wrapper)
    with _lib.count_calls("evae_") as counts:
        plain = sq.sample_quality(real, fake, nearest_k=3, train=train)
    assert called == [] and not [n for n in counts if n.startswith(("evae_kernel_", "evae_ordered_", "evae_sym_", "evae_pca_"))]
    full = sq.sample_quality(real, fake, nearest_k=3, train=train, distances=True)
    assert {k: full[k] for k in plain} == plain
    assert sorted(set(full) - set(plain)) == ["frechet_distance", "kid", "kid_train"]
    assert called.count("kernel_row_sums") == 6 and called.count("ordered_sum") == 6 + 4 and called.count("sym_congruence") == 1
    assert full['frechet_distance'] == sq.frechet_distance(real, fake)['frechet_distance']
    assert full['kid'] == sq.kernel_inception_distance(real, fake) and full['kid_train'] == sq.kernel_inception_distance(train, fake)
    assert abs(full['kid'] - ref.mmd_case('small')['mmd2']) <= ref.mmd_case('small')['bound']
    assert sorted(set(sq.sample_quality(real, fake, nearest_k=3, distances=True)) - set(plain)) == ["frechet_distance", "kid"]
    # copies of training rows: far nearer to the training set than to the real one
    copies = sq.sample_quality(real, train[:150], nearest_k=3, train=train, distances=True)
    assert copies['kid_train'] < copies['kid']


def test_report_writes_the_distances_when_asked(tmp_path):
    import evae_oracle as orc
    import smoke_case
    import golden_inputs as gi
    from utils.sample_quality_on_latent import report_sample_quality
    B = 32
    args = smoke_case.vae_args(number_components=20, training_set_size=200, batch_size=B)
    args.sample_quality_space, args.sample_quality_k, args.sample_quality_save = "both", 3, 0
    model, _ = smoke_case.build_model(torch, np, orc, args)
    model.eval()

    def loader(seed, n):
        data = torch.from_numpy(gi.binary_images(seed, n))
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, torch.arange(n) % 10), batch_size=B, shuffle=False)

    train, test = loader(91, 200), loader(92, 100)
    new = ["frechet_distance", "kid", "kid_train"]
    torch.manual_seed(5)
    plain = report_sample_quality(train, test, model, str(tmp_path / "plain"), args)
    assert not any(k in plain[s] for k in new for s in plain)
    args.sample_quality_distances = True
    torch.manual_seed(5)
    report = report_sample_quality(train, test, model, str(tmp_path / "distances"), args)
    with open(os.path.join(str(tmp_path / "distances"), "sample_quality.json")) as f:
        saved = json.load(f)
    assert saved == report
    assert sorted(set(saved["latent"]) - set(plain["latent"])) == new and all(np.isfinite(saved["latent"][k]) for k in new)
    assert {k: saved["latent"][k] for k in plain["latent"]} == plain["latent"]
    assert saved["pixel"] == plain["pixel"]                            # 784 pixels: wider than the kernels take, nothing added


# ---------------------------------------------------------------------------------------------- 9. argument errors
def test_argument_errors_launch_nothing(ops, sq, monkeypatch):
    from evae import _lib
    EvaeError = _lib.EvaeError
    q, c = dev(ref.rows_case(65, T, 7)[0]), dev(ref.rows_case(65, T, 7)[1])
    f64 = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
    with _lib.count_calls("evae_") as counts:
        for call, exc, word in (
                (lambda: ops.kernel_row_sums(q.cpu(), c), EvaeError, "no CPU fallback"),
                (lambda: ops.kernel_row_sums(q, c.cpu()), EvaeError, "no CPU fallback"),
                (lambda: ops.kernel_row_sums(q, c[:, :5]), ValueError, "q has 7 features, c 5"),
                (lambda: ops.kernel_row_sums(q, c, skip_self=True), ValueError, "skip_self"),
                (lambda: ops.kernel_row_sums(q, c, kind='linear'), ValueError, "kind="),
                (lambda: ops.kernel_row_sums(q, c, degree=0), ValueError, "degree=0"),
                (lambda: ops.kernel_row_sums(q, c, degree=9), ValueError, "degree=9"),
                (lambda: ops.kernel_row_sums(q, c, degree=2.5), ValueError, "degree=2.5"),
                (lambda: ops.kernel_row_sums(torch.zeros((3, 257), device="cuda"), torch.zeros((3, 257), device="cuda")), ValueError,
                 "257 features"),
                (lambda: ops.kernel_row_sums(q[0], c), ValueError, "q must be"),
                (lambda: ops.ordered_sum(torch.zeros(3, dtype=torch.float64)), EvaeError, "no CPU fallback"),
                (lambda: ops.ordered_sum(torch.zeros(3, device="cuda")), ValueError, "x must be"),
                (lambda: ops.ordered_sum(torch.zeros(0, dtype=torch.float64, device="cuda")), ValueError, "0 entries"),
                (lambda: ops.sym_congruence(f64.cpu(), f64.cpu()), EvaeError, "no CPU fallback"),
                (lambda: ops.sym_congruence(f64, f64[:3, :3].contiguous()), ValueError, "S must be"),
                (lambda: ops.sym_congruence(f64.float(), f64), ValueError, "A must be"),
                (lambda: ops.sym_congruence(torch.zeros((257, 257), dtype=torch.float64, device="cuda"),
                                            torch.zeros((257, 257), dtype=torch.float64, device="cuda")), ValueError, "d outside"),
                (lambda: sq.frechet_distance(q.cpu(), c), EvaeError, "no CPU fallback"),
                (lambda: sq.frechet_distance(q, c[:, :5]), ValueError, "features"),
                (lambda: sq.frechet_distance(q[:1], c), ValueError, "at least 2"),
                (lambda: sq.frechet_distance(torch.zeros((3, 300), device="cuda"), torch.zeros((3, 300), device="cuda")), ValueError,
                 "evae.pca.PCA"),
                (lambda: sq.kernel_mmd(q.cpu(), c), EvaeError, "no CPU fallback"),
                (lambda: sq.kernel_mmd(q[:1], c), ValueError, "unbiased form needs 2"),
                (lambda: sq.kernel_mmd(q, c, kernel='cosine'), ValueError, "kernel="),
                (lambda: sq.kernel_mmd(q, c, gamma='median'), ValueError, "gamma='median'"),
                (lambda: sq.kernel_mmd(q, c, degree=0), ValueError, "degree=0"),
                (lambda: sq.kernel_mmd(q, c, degree="3"), ValueError, "degree='3'"),
                (lambda: sq.kernel_mmd(q, c, coef0=None), ValueError, "coef0=None"),
                (lambda: sq.kernel_mmd(q, c, gamma=[0.5]), ValueError, "gamma="),
                (lambda: sq.kernel_mmd(q, c, kernel='rbf', gamma='mean'), ValueError, "gamma='mean'"),
                (lambda: sq.kernel_mmd(torch.zeros((3, 257), device="cuda"), torch.zeros((3, 257), device="cuda"), kernel='rbf',
                                       gamma='median'), ValueError, "257 features"),
                (lambda: ops.kernel_row_sums(q, c, degree=None), ValueError, "degree=None"),
                (lambda: ops.kernel_row_sums(q, c, gamma="0.5"), ValueError, "gamma='0.5'")):
            with pytest.raises(exc, match=word):
                call()
        with monkeypatch.context() as m:                               # the caps on points, made small: no 2^20-row allocation
            m.setattr(ops, "kernel_sum_max_points", lambda: 40)
            with pytest.raises(ValueError, match="q has 65 rows"):
                ops.kernel_row_sums(q, c)
            with pytest.raises(ValueError, match="c has 65 rows"):
                ops.kernel_row_sums(q[:3], q)
    assert launches(counts) == [], counts
    # the entry points' own checks, under the operators': live buffers, nothing launched, nothing written
    lib, vp = _lib.load(), _lib.vp
    out = torch.full((65,), -7.0, dtype=torch.float64, device="cuda")

    def raw(B=65, d=7, kind=0, degree=3, skip_self=0):
        return lib.evae_kernel_row_sums(vp(q), B, vp(c), T, d, kind, 1.0, 1.0, degree, skip_self, vp(out), None)

    for call, word in ((lambda: raw(kind=2), b"kind=2"), (lambda: raw(degree=9), b"degree=9"), (lambda: raw(skip_self=1), b"skip_self"),
                       (lambda: raw(d=257), b"257 features"), (lambda: raw(B=0), b"B=0"),
                       (lambda: lib.evae_ordered_sum(vp(out), 0, vp(out), None), b"n=0"),
                       (lambda: lib.evae_sym_congruence(vp(f64), vp(f64), vp(out), 4, vp(out), 64, None), b"workspace"),
                       (lambda: lib.evae_sym_congruence(vp(f64), vp(f64), vp(out), 4, vp(out), 512, None), b"overlaps A, S or out"),
                       (lambda: lib.evae_sym_congruence(vp(f64), vp(f64), vp(f64), 4, vp(out), 512, None), b"out overlaps")):
        assert call() != 0
        assert word in lib.evae_last_error(), word
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
