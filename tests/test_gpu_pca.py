"""GPU: the fp64 PCA kernels (csrc/evae_pca.hip), evae.ops.pca_*, evae.pca.PCA, TSNE(init='pca') and the two latent-space
reports, against the numpy float64 restatement tests/pca_ref.py (held to scikit-learn by tests/test_pca_ref_host.py).

The yardstick is always the restatement, never the code under test.  Every bound comes from the arithmetic, with eps = 2^-52:

* moments: both sides add N float64 terms; 4 N eps covers the two sums, the centring and the reference's own rounding.
* eigen-solver: Jacobi and LAPACK are both backward stable at p(d) eps |A|; tol = 32 d eps lambda_max, 32 being the margin over
  d eps.  A component is then good to tol / gap_i (Davis-Kahan), a subspace of tied eigenvalues to tol / (its distance to the
  rest of the spectrum).
* projections: accumulated in fp64 and rounded once to fp32; 2^-22 of the largest entry of a column is four such roundings.

Every test prints the figures it asserts on; DESIGN 3.7c records the largest."""
import os

import numpy as np
import pytest
import torch

import pca_ref as ref
from tsne_ref import blobs

pytestmark = pytest.mark.gpu

EPS = ref.EPS


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view(np.uint64 if t.dtype == torch.float64 else np.uint32)


# ---------------------------------------------------------------------------------------------- 1. moments
def moment_shapes():
    from evae import ops
    C = ops.pca_chunk_rows()
    ns, ds = (2, 3, C - 1, C, C + 1, 2 * C + 1), (1, 2, 3, 40, 63, 64, 65, 255, 256)
    return [(n, 40) for n in ns] + [(C + 1, d) for d in ds if d != 40] + [(2, 1), (3, 256), (2 * C + 1, 65), (2 * C + 1, 256)]


def moment_input(n, d):
    rs = np.random.RandomState(100 * d + n % 97)
    return (rs.randn(n, d) * np.exp(rs.randn(d)) + 2.0 * rs.randn(d)).astype(np.float32)


def check_moments(X):
    from evae import ops
    n, d = X.shape
    x = dev(X)
    mean, cov = ops.pca_moments(x)
    assert mean.dtype == cov.dtype == torch.float64 and tuple(mean.shape) == (d,) and tuple(cov.shape) == (d, d)
    rmean, rcov = ref.moments(X)
    sd = np.sqrt(np.diag(rcov))
    scale = np.outer(sd, sd)
    e_mean = np.abs(host(mean) - rmean).max() / np.abs(X).max()
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(scale > 0, np.abs(host(cov) - rcov) / scale, np.where(host(cov) == rcov, 0.0, np.inf))
    e_cov = ratio.max()
    print("moments n=%d d=%d: mean %.3g of max|x|, cov %.3g of sqrt(c_ii c_jj); allowed %.3g" % (n, d, e_mean, e_cov, 4 * n * EPS))
    assert e_mean <= 4 * n * EPS
    assert e_cov <= 4 * n * EPS
    assert np.array_equal(bits(cov), bits(cov.t().contiguous()))
    mean2, cov2 = ops.pca_moments(x)
    assert np.array_equal(bits(mean), bits(mean2)) and np.array_equal(bits(cov), bits(cov2))


def test_moments_over_the_shapes():
    """every N at d = 40, every d at N = chunk + 1, and the corners: bounds, exact symmetry, bit-equal repeats"""
    for n, d in moment_shapes():
        check_moments(moment_input(n, d))


def test_moments_of_a_far_off_mean():
    """column means of 4096 against a standard deviation of 1e-2: E[x^2] - E[x]^2 in one pass would miss by about 1e7 x"""
    from evae import ops
    rs = np.random.RandomState(5)
    X = (4096.0 + 1e-2 * rs.randn(ops.pca_chunk_rows() + 1, 40)).astype(np.float32)
    check_moments(X)
    X64 = X.astype(np.float64)
    one_pass = (X64 * X64).mean(axis=0) - X64.mean(axis=0) ** 2
    print("one-pass variance misses by %.3g of the variance" % (np.abs(one_pass * len(X) / (len(X) - 1.0) - X64.var(axis=0, ddof=1))
                                                               / X64.var(axis=0, ddof=1)).max())


def test_moments_refuse_what_they_cannot_take():
    from evae import ops, _lib
    with pytest.raises(_lib.EvaeError):
        ops.pca_moments(torch.zeros(8, 4))                                   # a CPU tensor
    with pytest.raises(_lib.EvaeError):
        ops.pca_moments(torch.zeros(8, ops.pca_max_features() + 1, device="cuda"))
    with pytest.raises(_lib.EvaeError):
        ops.pca_moments(torch.zeros(1, 4, device="cuda"))
    with pytest.raises(_lib.EvaeError):
        ops.pca_eigh(torch.zeros(4, 4, device="cuda"))                       # float32
    assert ops.pca_max_features() == 256 and ops.pca_max_points() == 2 ** 20


# ---------------------------------------------------------------------------------------------- 2. the eigen-solver
def hand_made():
    rs = np.random.RandomState(5)
    A = rs.randn(40, 3)
    Q24 = np.linalg.qr(rs.randn(24, 24))[0]
    Q12 = np.linalg.qr(rs.randn(12, 12))[0]
    tied = (Q12 * np.concatenate(([1.0, 1.0], 1.5 ** -np.arange(1.0, 11.0)))) @ Q12.T
    return [("1x1", np.array([[2.5]])),
            ("2x2 negative off-diagonal", np.array([[2.0, -1.5], [-1.5, 3.0]])),
            ("diagonal, ascending", np.diag(np.arange(1.0, 8.0))),
            ("5 I_40", 5.0 * np.eye(40)),
            ("rank 3 in d = 40", A @ A.T),
            ("spectrum 1 .. 1e-12", (Q24 * 10.0 ** -np.linspace(0.0, 12.0, 24)) @ Q24.T),
            ("tied leading pair", (tied + tied.T) / 2.0)]


def planted_covariances():
    return [("planted n=%d d=%d r=%g" % (n, d, r), ref.moments(ref.planted(n, d, r, seed))[1]) for n, d, r, seed in ref.PLANTED]


def check_eigh(name, C, every_row):
    """every_row: compare every component element-wise (the planted cases).  Otherwise only TIED eigenvalues -- neighbours no
    further apart than tol, the eigenvalues' own allowance: the identity multiple, the null space of the rank-3 matrix, the equal
    pair -- form a group whose projector is compared; every other row is compared element-wise at tol / gap_i, however small
    its gap (the 24 distinct eigenvalues of the 1 .. 1e-12 spectrum among them)."""
    from evae import ops
    d = len(C)
    evals, evecs, info = ops.pca_eigh(dev(C))
    assert evals.dtype == evecs.dtype == info.dtype == torch.float64
    assert tuple(evals.shape) == (d,) and tuple(evecs.shape) == (d, d) and tuple(info.shape) == (4,)
    ev, V, info = host(evals), host(evecs), host(info)
    rv, rV = ref.eigh(C)
    lmax = rv[0]
    tol = 32 * d * EPS * lmax
    e_val = np.abs(ev - rv).max()
    e_res = np.abs(C @ V.T - V.T * ev).max()
    e_orth = np.abs(V @ V.T - np.eye(d)).max()
    print("%s: sweeps %d, converged %d, last off-diagonal %.3g; eigenvalues %.3g, residual %.3g (allowed %.3g), "
          "orthogonality %.3g (allowed %.3g)" % (name, info[0], info[1], info[2], e_val, e_res, tol, e_orth, 32 * d * EPS))
    assert info[1] == 1.0 and 1 <= info[0] <= ops.pca_max_sweeps() and info[2] <= EPS
    assert abs(info[3] - np.trace(C)) <= d * EPS * np.abs(np.diag(C)).sum()
    assert e_val <= tol and e_res <= tol and e_orth <= 32 * d * EPS
    assert np.all(ev[:-1] >= ev[1:]) and np.all(ev >= 0)
    # the sign rule, as the solver states it: in every row the entry of largest magnitude is positive ...
    assert np.all(V[np.arange(d), np.argmax(np.abs(V), axis=1)] > 0)
    # ... and, below, where a row is the reference's row and the reference's own choice is safe, it is the same entry
    safe = ref.sign_margins(rV) >= 1e-6
    gaps = ref.gaps(rv)
    if every_row:
        groups = [[i] for i in range(d)]
    else:
        groups = [[0]]
        for i in range(1, d):
            if rv[i - 1] - rv[i] > tol:
                groups.append([i])
            else:
                groups[-1].append(i)
    worst = 0.0
    for g in groups:
        if len(g) == 1:
            i = g[0]
            if d == 1:
                assert V[0, 0] == 1.0
                continue
            err, allowed = np.abs(V[i] - rV[i]).max(), tol / gaps[i]
            assert not safe[i] or V[i, np.argmax(np.abs(rV[i]))] > 0, (name, i)
        else:
            outside = np.delete(rv, g)
            gap = np.abs(outside[:, None] - rv[g][None, :]).min() if len(outside) else np.inf
            err, allowed = np.abs(V[g].T @ V[g] - rV[g].T @ rV[g]).max(), tol / gap
        worst = max(worst, err / allowed if allowed > 0 else (0.0 if err == 0 else np.inf))
        assert err <= allowed, (name, g[:4], err, allowed)
    print("%s: components at %.3g of their allowance (%d groups for %d rows)" % (name, worst, len(groups), d))


def test_eigh_on_planted_covariances():
    for name, C in planted_covariances():
        check_eigh(name, C, every_row=True)


def test_eigh_on_hand_made_matrices():
    for name, C in hand_made():
        check_eigh(name, C, every_row=False)


def test_eigh_repeats_bit_for_bit():
    from evae import ops
    C = dev(planted_covariances()[4][1])
    a, b = ops.pca_eigh(C), ops.pca_eigh(C)
    assert all(np.array_equal(bits(s), bits(t)) for s, t in zip(a, b))


# ---------------------------------------------------------------------------------------------- 3. the class
@pytest.fixture(scope="module", params=[ref.PLANTED[1], ref.PLANTED[2], ref.PLANTED[7]], ids=lambda s: "n%d_d%d" % s[:2])
def fitted(request):
    n, d, ratio, seed = request.param
    X = ref.planted(n, d, ratio, seed)
    return dict(n=n, d=d, X=X, x=dev(X), ref=ref.fit(X))


def test_planted_sizes_cover_the_chunk_boundary():
    from evae import ops
    assert ref.PLANTED[2][0] == ops.pca_chunk_rows() + 1


@pytest.mark.parametrize("k", [1, 2, None])
def test_fit_transform_against_the_reference(fitted, k):
    from evae import ops
    from evae.pca import PCA
    n, d = fitted["n"], fitted["d"]
    mean, evals, comps = fitted["ref"]
    kk = d if k is None else k
    pca = PCA(n_components=k)
    Y = pca.fit_transform(fitted["x"])
    assert Y.dtype == torch.float32 and tuple(Y.shape) == (n, kk)
    want = ref.project(fitted["X"], mean, comps[:kk])
    err = np.abs(host(Y) - want).max(axis=0) / np.abs(want).max(axis=0)
    print("fit_transform n=%d d=%d k=%d: worst column at %.3g of its largest entry (allowed %.3g)" % (n, d, kk, err.max(), 2.0 ** -22))
    assert np.all(err <= 2.0 ** -22)
    # attributes: shapes, dtypes, values
    for name, shape in (("mean_", (d,)), ("components_", (kk, d)), ("explained_variance_", (kk,)),
                        ("explained_variance_ratio_", (kk,)), ("singular_values_", (kk,))):
        t = getattr(pca, name)
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape, name
    assert (pca.n_samples_, pca.n_features_in_, pca.n_components_) == (n, d, kk) and 1 <= pca.n_sweeps_ <= ops.pca_max_sweeps()
    tol = 32 * d * EPS * evals[0]
    assert np.abs(host(pca.explained_variance_) - evals[:kk]).max() <= tol + 4 * n * EPS * evals[0]
    assert np.abs(host(pca.explained_variance_ratio_) - evals[:kk] / evals.sum()).max() <= (tol + 8 * n * EPS * evals[0]) / evals.sum()
    assert np.abs(host(pca.singular_values_) ** 2 / (n - 1) - evals[:kk]).max() <= tol + 4 * n * EPS * evals[0]
    assert np.abs(host(pca.mean_) - mean).max() <= 4 * n * EPS * np.abs(fitted["X"]).max()
    assert np.array_equal(host(pca.transform(fitted["x"])), host(Y))


def test_inverse_transform_gives_the_input_back(fitted):
    from evae.pca import PCA
    pca = PCA().fit(fitted["x"])
    back = pca.inverse_transform(pca.transform(fitted["x"]))
    assert back.dtype == torch.float32 and tuple(back.shape) == fitted["X"].shape
    err = np.abs(host(back).astype(np.float64) - fitted["X"]).max() / np.abs(fitted["X"]).max()
    print("inverse_transform(transform(X)) n=%d d=%d: %.3g of max|X| (allowed %.3g)" % (fitted["n"], fitted["d"], err, 2.0 ** -22))
    assert err <= 2.0 ** -22


def test_reconstruct_from_fewer_components(fitted):
    """k < d: the reverse map against the reference's, from the same float32 scores"""
    from evae import ops
    mean, _, comps = fitted["ref"]
    Y = ref.project(fitted["X"], mean, comps[:2]).astype(np.float32)
    got = host(ops.pca_reconstruct(dev(Y), dev(mean), dev(comps[:2])))
    want = ref.reconstruct(Y, mean, comps[:2])
    assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max()      # one rounding of the result


def test_pca_refuses_what_it_cannot_take():
    from evae import _lib
    from evae.pca import PCA
    with pytest.raises(_lib.EvaeError):
        PCA(2).fit(torch.zeros(16, 4))                                       # a CPU tensor
    with pytest.raises(_lib.EvaeError):
        PCA(2).fit(torch.randn(300, 257, device="cuda"))
    with _lib.count_calls("evae_pca") as calls:
        with pytest.raises(ValueError):
            PCA(5).fit(torch.randn(30, 4, device="cuda"))
    assert not calls                                                         # known from the shape: before any launch
    with pytest.raises(ValueError):
        PCA(0)
    with pytest.raises(_lib.EvaeError):
        PCA(2).transform(torch.randn(30, 4, device="cuda"))                  # not fitted


def test_pca_of_equal_rows_has_zero_ratios_not_nan():
    from evae.pca import PCA
    pca = PCA().fit(torch.full((30, 4), 2.5, device="cuda"))
    assert pca.n_sweeps_ == 1
    for name in ("explained_variance_", "explained_variance_ratio_", "singular_values_"):
        assert np.array_equal(host(getattr(pca, name)), np.zeros(4)), name
    assert np.array_equal(host(pca.mean_), np.full(4, 2.5))
    assert np.array_equal(host(pca.transform(torch.full((3, 4), 2.5, device="cuda"))), np.zeros((3, 4), np.float32))


# ---------------------------------------------------------------------------------------------- 4. TSNE(init='pca')
@pytest.mark.parametrize("which", ["blobs", "planted"])
def test_tsne_initial_state(which):
    from evae.tsne import TSNE
    X = blobs(300, 40, 4, seed=21)[0] if which == "blobs" else ref.planted(*ref.PLANTED[2])
    Y0 = host(TSNE(init='pca')._initial(len(X), torch.device("cuda"), dev(X))).astype(np.float64)
    want = ref.tsne_initial(X)
    err = np.abs(Y0 - want).max()
    std = np.std(Y0[:, 0])
    print("init='pca' on %s: %.3g from the reference (allowed %.3g); std of the first column %.9g" % (which, err, 2.0 ** -22 * 1e-4, std))
    assert Y0.shape == (len(X), 2)
    assert err <= 2.0 ** -22 * 1e-4
    assert abs(std - 1e-4) <= 1e-6 * 1e-4


@pytest.mark.parametrize("method", ["exact", "neighbours"])
def test_tsne_from_pca_does_not_depend_on_the_seed(method):
    from evae.tsne import TSNE
    x = dev(blobs(300, 40, 4, seed=22)[0])

    def run(seed):
        return TSNE(init='pca', n_iter=60, exaggerated_iters=15, random_state=seed, method=method).fit_transform(x)
    a, b, c = run(0), run(0), run(1)
    assert tuple(a.shape) == (300, 2) and torch.isfinite(a).all()
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(a), bits(c))
    r = TSNE(n_iter=60, exaggerated_iters=15, random_state=0, method=method).fit_transform(x)       # the default is still 'random'
    assert not np.array_equal(bits(a), bits(r))


def test_tsne_from_pca_refuses_what_has_no_second_component():
    from evae import _lib
    from evae.tsne import TSNE
    tsne = TSNE(init='pca', perplexity=5.0, n_iter=2)                       # the constructor takes 'pca'; the refusals are the fit's
    for method in ("exact", "neighbours"):
        tsne.method = method
        with _lib.count_calls("evae_") as calls:
            with pytest.raises(ValueError):
                tsne.fit_transform(torch.randn(50, 1, device="cuda"))         # zd = 1
        assert not calls                                                      # refused before any launch
        with _lib.count_calls("evae_") as calls:
            with pytest.raises(ValueError):
                tsne.fit_transform(torch.ones(50, 4, device="cuda"))          # all points equal
        assert calls.get("evae_pca_eigh") == 1                                # refused by the PCA, before the affinity stage:
        assert not {"evae_pairwise_distance", "evae_tsne_affinities", "evae_tsne_knn"} & set(calls)
    with pytest.raises(ValueError):
        tsne._initial(50, torch.device("cuda"), torch.ones(50, 4, device="cuda"))
    with pytest.raises(ValueError):
        TSNE(init='svd')


# ---------------------------------------------------------------------------------------------- 5. the reports
def test_reports_on_a_stub_model(tmp_path):
    import evae_oracle as orc
    import smoke_case
    import golden_inputs as gi
    from evae.pca import PCA
    from utils.knn_on_latent import _posterior_means
    from utils.pca_on_latent import report_pca_on_latent
    from utils.tsne_on_latent import report_tsne_on_latent
    n, B = 75, 32
    args = smoke_case.vae_args(number_components=20, training_set_size=100, batch_size=B)
    args.tsne_n_iter, args.tsne_perplexity, args.seed, args.tsne_init = 30, 5.0, 3, 'pca'
    model, _ = smoke_case.build_model(torch, np, orc, args)
    model.eval()
    data = torch.from_numpy(gi.binary_images(91, n))
    labels = torch.arange(n) % 10
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, labels), batch_size=B, shuffle=False)
    with torch.no_grad():
        z = _posterior_means(model, data.to(args.device), B)
    N, zd = z.shape
    assert N == 64

    out = str(tmp_path / "tsne")
    Y = report_tsne_on_latent(loader, model, out, args)
    saved = np.load(os.path.join(out, "tsne.npy"))
    assert saved.shape == (N, 2) and np.isfinite(saved).all() and np.array_equal(saved, host(Y))
    args.seed = 4                                                            # init='pca': another seed, the same picture
    again = report_tsne_on_latent(loader, model, str(tmp_path / "tsne_again"), args)
    assert np.array_equal(bits(Y), bits(again))

    out = str(tmp_path / "pca")
    P = report_pca_on_latent(loader, model, out, args)
    assert sorted(os.listdir(out)) == ["pca.npy", "pca_explained_variance_ratio.npy", "pca_labels.npy"]
    saved = np.load(os.path.join(out, "pca.npy"))
    ratio = np.load(os.path.join(out, "pca_explained_variance_ratio.npy"))
    assert saved.shape == (N, 2) and saved.dtype == np.float32 and np.array_equal(saved, host(P))
    assert np.array_equal(np.load(os.path.join(out, "pca_labels.npy")), labels[:N].numpy())
    assert ratio.shape == (zd,) and ratio.dtype == np.float64 and np.all(ratio[:-1] >= ratio[1:]) and abs(ratio.sum() - 1.0) <= 1e-12
    assert np.array_equal(saved, host(PCA(2).fit_transform(z)))
    assert np.abs(ratio - host(PCA().fit(z).explained_variance_ratio_)).max() == 0
