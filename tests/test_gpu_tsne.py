"""GPU: the exact t-SNE kernels (csrc/evae_tsne.hip), evae.ops.tsne_*, evae.tsne.TSNE and utils.tsne_on_latent against the
float64 restatement tests/tsne_ref.py (held to scikit-learn by tests/test_tsne_ref_host.py).

THE TOLERANCE RULE of every comparison with float64: the restatement runs a second time in float32 at the same case; a kernel
may miss float64 by max(8 x the float32 restatement's error, 4 x eps32 x scale) -- 8 for another summation order, the floor for
a float32 run that happens to land exact.  The yardstick is the reference, never the kernel.  Where a quantity is per row
(beta, achieved perplexity) the rule is applied row by row, so that one loose row cannot excuse the others.  Seven duplicates
of a row (and a row whose nearest neighbours are those eight identical rows) cannot be spread over a perplexity of 5: there
the float64 search itself ends at perplexity 7 (8), the float32 one too, and the rule holds the kernel to the same place."""
import os

import numpy as np
import pytest
import torch

import tsne_ref as ref

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
CASES = [(97, 40, 5.0), (200, 40, 30.0), (257, 3, 30.0), (1025, 40, 30.0)]


def allowed(err32, scale):
    return np.maximum(8.0 * err32, 4.0 * EPS32 * scale)


def held(name, got, want64, want32, scale=None):
    """max |got - float64| against the rule, the float32 restatement's error as yardstick; prints the figures"""
    got, want64, want32 = (np.asarray(a, np.float64) for a in (got, want64, want32))
    scale = float(np.abs(want64).max()) if scale is None else scale
    err, err32 = float(np.abs(got - want64).max()), float(np.abs(want32 - want64).max())
    tol = float(allowed(err32, scale))
    print("%-28s kernel %.3g  float32 restatement %.3g  allowed %.3g  (scale %.3g)" % (name, err, err32, tol, scale))
    assert np.all(np.isfinite(got)), name
    assert err <= tol, (name, err, tol)


_cases = {}


def case(n, zd, perp):
    """inputs and both restatements of a case, computed once and shared"""
    key = (n, zd, perp)
    if key not in _cases:
        X, labels = ref.blobs(n, zd, 4, seed=2000 + n)
        if n == 97:
            X[5] += 40.0                    # one far outlier row
            X[20:28] = X[20]                # eight identical rows
        P64, b64, D64 = ref.affinities(X, perp, np.float64)
        P32, b32, _ = ref.affinities(X, perp, np.float32)
        _cases[key] = dict(X=X, labels=labels, P64=P64, b64=b64, D64=D64, P32=P32, b32=b32)
    return _cases[key]


@pytest.fixture(scope="module")
def ops():
    from evae import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


# ---------------------------------------------------------------------------------------------- 1. affinities
@pytest.mark.parametrize("n,zd,perp", CASES)
def test_affinities(ops, n, zd, perp):
    c = case(n, zd, perp)
    P, beta = ops.tsne_affinities(dev(c["X"]), perp)
    assert P.shape == (n, n) and beta.shape == (n,) and P.dtype == torch.float32
    assert torch.equal(P, P.t().contiguous())                       # bit-symmetric
    P, beta = P.cpu().numpy(), beta.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(beta)) and np.all(np.diag(P) == 0) and np.all(P >= 0)
    held("P", P, c["P64"], c["P32"])
    held("sum(P)", P.astype(np.float64).sum(), 1.0, c["P32"].astype(np.float64).sum(), scale=1.0)
    # beta and the achieved perplexity, row by row
    b64, b32 = c["b64"], c["b32"].astype(np.float64)
    tol_b = allowed(np.abs(b32 - b64), np.abs(b64))
    err_b = np.abs(beta - b64)
    print("beta: worst row kernel %.3g of its allowance (float32 restatement: %.3g relative at worst)"
          % ((err_b / tol_b).max(), (np.abs(b32 - b64) / b64).max()))
    assert np.all(err_b <= tol_b), np.nonzero(err_b > tol_b)
    pk, p32, p64 = (ref.row_perplexity(c["D64"], b) for b in (beta, c["b32"], c["b64"]))
    tol_p = allowed(np.abs(p32 - perp), perp)
    err_p = np.abs(pk - perp)
    print("perplexity: worst row kernel %.3g of its allowance; rows the float64 search cannot bring to the target: %d"
          % ((err_p / tol_p).max(), int((np.abs(p64 - perp) > 1e-9 * perp).sum())))
    assert np.all(err_p <= tol_p), np.nonzero(err_p > tol_p)
    held("achieved perplexity", pk, p64, p32, scale=perp)          # and the same place as float64 where the target is out of reach
    if n == 97:
        assert np.all(beta[20:28] == 2.0 ** ref.SEARCH_STEPS) and np.allclose(pk[20:28], 7.0)
        assert np.all(P[20, 21:28] == P[20, 21]) and P[5].sum() > 0


def test_affinities_in_both_row_kernels_agree(ops):
    """N = 1024 is the last size of the wave-per-row search, 1025 the first of the workgroup-per-row one: the first 1024 points
    of the larger case through both must give the float64 answer (the rule), i.e. the switch is not a numerical seam"""
    c = case(1025, 40, 30.0)
    X = c["X"][:1024]
    P64, b64, _ = ref.affinities(X, 30.0, np.float64)
    P32, b32, _ = ref.affinities(X, 30.0, np.float32)
    P, beta = ops.tsne_affinities(dev(X), 30.0)
    assert torch.equal(P, P.t().contiguous())
    held("P at N = 1024", P.cpu().numpy(), P64, P32)
    err, tol = np.abs(beta.cpu().numpy() - b64), allowed(np.abs(b32 - b64), np.abs(b64))
    assert np.all(err <= tol)


# ---------------------------------------------------------------------------------------------- 2. forces, gradient, KL
def embedding(n, scale, seed=11):
    Y = (np.random.RandomState(seed).randn(n, 2) * scale).astype(np.float32)
    Y[3] = Y[17]                             # two coincident points
    return Y


@pytest.mark.parametrize("scale", [1e-4, 1.0, 30.0])
@pytest.mark.parametrize("n,zd,perp", CASES)
def test_forces_gradient_and_kl(ops, n, zd, perp, scale):
    c = case(n, zd, perp)
    P = c["P64"].astype(np.float32)          # the kernel and both restatements see the same float32 matrix
    Y = embedding(n, scale)
    Pd, Yd = dev(P), dev(Y)
    for exag in (12.0, 1.0):
        g64, Z64, kl64, A64, R64 = ref.forces(P, Y, exag, np.float64)
        g32, Z32, kl32, A32, R32 = ref.forces(P, Y, exag, np.float32)
        part = ops.tsne_forces(Pd, Yd, exag, True)
        stats = ops.tsne_stats(part, True).cpu().numpy()
        pn = part.cpu().numpy()
        tag = "scale %g exag %g: " % (scale, exag)
        held(tag + "A", pn[:, 0:2], A64, A32)
        held(tag + "R", pn[:, 2:4], R64, R32)
        held(tag + "Z", stats[0], Z64, Z32)
        held(tag + "KL", stats[1], kl64, kl32, scale=max(abs(kl64), 1.0))
        assert stats[0] == pn[:, 4].sum() or abs(stats[0] - pn[:, 4].sum()) <= 1e-12 * Z64
        # the gradient as the update launch forms it (lr 0: nothing moves but the re-centring)
        Yc, v, ga = Yd.clone(), torch.zeros_like(Yd), torch.ones_like(Yd)
        grad, st2 = ops.tsne_update(ops.tsne_forces(Pd, Yd, exag, False), Yc, v, ga, 0.5, 0.0, want_grad=True)
        held(tag + "gradient", grad.cpu().numpy(), g64, g32)
        held(tag + "Z (update launch)", float(st2[0]), Z64, Z32)       # the pass without KL is other code: equal under the rule, not bit for bit
        assert float(st2[1]) == 0.0
        assert np.all(pn[:, 5:7] != 0) and torch.all(ops.tsne_forces(Pd, Yd, exag, False)[:, 5:7] == 0)


# ---------------------------------------------------------------------------------------------- 3. update
@pytest.mark.parametrize("momentum", [0.5, 0.8])
@pytest.mark.parametrize("n,zd,perp", [CASES[0], CASES[3]])
def test_update_step(ops, n, zd, perp, momentum):
    c = case(n, zd, perp)
    P = c["P64"].astype(np.float32)
    Y = embedding(n, 1.0, seed=12)
    rs = np.random.RandomState(13)
    g64 = ref.forces(P, Y, 1.0, np.float64, want_kl=False)[0]
    g32 = ref.forces(P, Y, 1.0, np.float32, want_kl=False)[0]
    # velocities of both signs against the gradient, well away from zero; gains at 1, above the floor and where x0.8 goes under it
    vel = (np.where(rs.rand(n, 2) < 0.5, 1.0, -1.0) * np.sign(g64) * (0.5 + rs.rand(n, 2)) * np.abs(g64).max()).astype(np.float32)
    vel[np.sign(g64) == 0] = 0.0
    gains = rs.choice([1.0, 0.05, 0.011, 0.0124, 2.5], size=(n, 2)).astype(np.float32)
    lr = ref.learning_rate(n)
    Y64, v64, ga64 = ref.update(Y, vel, gains, g64, momentum, lr, np.float64)
    Y32, v32, ga32 = ref.update(Y, vel, gains, g32, momentum, lr, np.float32)
    inc = vel.astype(np.float64) * g64 < 0
    assert inc.any() and (~inc).any() and (ga64 == 0.01).any() and (ga64[~inc] > 0.01).any()        # every branch of the gain rule
    Yd, vd, gd = dev(Y), dev(vel), dev(gains)
    ops.tsne_update(ops.tsne_forces(dev(P), Yd, 1.0, False), Yd, vd, gd, momentum, lr)
    held("gains", gd.cpu().numpy(), ga64, ga32)
    held("velocity", vd.cpu().numpy(), v64, v32)
    held("Y", Yd.cpu().numpy(), Y64, Y32)
    mean = Yd.double().mean(dim=0).abs().max().item()
    assert mean <= 4.0 * EPS32 * np.abs(Y64).max(), mean                                    # zero mean after the step


# ---------------------------------------------------------------------------------------------- 4. determinism
def test_fit_transform_is_deterministic():
    from evae.tsne import TSNE
    X = dev(case(200, 40, 30.0)["X"])
    runs = [TSNE(random_state=5, n_iter=60, exaggerated_iters=15) for _ in range(2)]
    Ya, Yb = (t.fit_transform(X).clone() for t in runs)
    assert torch.equal(Ya, Yb) and runs[0].kl_divergence_ == runs[1].kl_divergence_ and runs[0].n_iter_ == 60
    assert torch.all(torch.isfinite(Ya)) and Ya.is_cuda and Ya.shape == (200, 2)
    Yc = TSNE(random_state=6, n_iter=60, exaggerated_iters=15).fit_transform(X)
    assert not torch.equal(Ya, Yc)


# ---------------------------------------------------------------------------------------------- 5. end to end
def test_end_to_end_against_the_reference_spread():
    """(300, 40, 30), three blobs, 500 iterations of which 125 exaggerated.  Trajectories of a chaotic descent do not match
    pointwise; the yardstick is the float64 restatement's own spread over five inits: the device's final KL -- evaluated in
    float64 from the float64 P -- from the same five inits must lie within [min - spread, max + spread], and the share of
    points whose 10 nearest neighbours in the embedding carry their own blob's label must reach the lowest reference run's
    less 0.02 (six points of 300)."""
    from evae.tsne import TSNE
    n, n_iter, n_exag = 300, 500, 125
    X, labels = ref.blobs(n, 40, 3, seed=77)
    P64 = ref.affinities(X, 30.0)[0]
    inits = [(np.random.RandomState(100 + s).randn(n, 2) * 1e-4).astype(np.float32) for s in range(5)]
    ref_runs = [ref.run(P64, Y0, n_iter, n_exag) for Y0 in inits]
    ref_kl = np.array([kl for _, kl in ref_runs])
    ref_purity = np.array([ref.neighbour_purity(Y, labels) for Y, _ in ref_runs])
    spread = ref_kl.max() - ref_kl.min()
    Xd = dev(X)
    dev_kl, dev_purity, own_kl = [], [], []
    for Y0 in inits:
        t = TSNE(perplexity=30.0, n_iter=n_iter, exaggerated_iters=n_exag, init=torch.from_numpy(Y0))
        Y = t.fit_transform(Xd).cpu().numpy()
        assert np.all(np.isfinite(Y)) and t.n_iter_ == n_iter
        dev_kl.append(float(ref.forces(P64, Y, 1.0)[2]))
        dev_purity.append(ref.neighbour_purity(Y, labels))
        own_kl.append(t.kl_divergence_)
    print("reference KL %s (spread %.4g), purity %s" % (np.round(ref_kl, 5), spread, ref_purity))
    print("device    KL %s, purity %s; kl_divergence_ %s" % (np.round(dev_kl, 5), dev_purity, np.round(own_kl, 5)))
    assert min(dev_kl) >= ref_kl.min() - spread and max(dev_kl) <= ref_kl.max() + spread
    assert min(dev_purity) >= ref_purity.min() - 0.02
    # kl_divergence_ is the device's own float32-P evaluation of the same number
    assert np.abs(np.array(own_kl) - np.array(dev_kl)).max() <= 1e-4 * max(dev_kl)


# ---------------------------------------------------------------------------------------------- 6. interface
def test_interface_errors(ops):
    from evae.tsne import TSNE
    from evae._lib import EvaeError
    X = dev(case(97, 40, 5.0)["X"])
    with pytest.raises(ValueError):
        TSNE(perplexity=97.0).fit_transform(X)
    with pytest.raises(ValueError):
        TSNE(perplexity=200.0).fit_transform(X)
    with pytest.raises(ValueError):
        TSNE(n_components=3)
    with pytest.raises(ValueError):
        TSNE().fit_transform(torch.zeros(ops.tsne_max_points() + 1, 2))
    assert ops.tsne_max_points() >= 10000
    with pytest.raises(EvaeError):
        ops.tsne_affinities(torch.zeros(8, 4), 2.0)
    with pytest.raises(EvaeError):
        ops.tsne_forces(torch.zeros(8, 8), torch.zeros(8, 2), 1.0, False)
    with pytest.raises(EvaeError):
        ops.tsne_update(torch.zeros(8, 8, dtype=torch.float64), torch.zeros(8, 2), torch.zeros(8, 2), torch.ones(8, 2), 0.5, 50.0)
    with pytest.raises(EvaeError):
        ops.tsne_stats(torch.zeros(8, 8, dtype=torch.float64))
    with pytest.raises(EvaeError):
        ops.tsne_affinities(X, 97.0)                     # the entry point's own check, under the class's


def test_report_tsne_on_latent(tmp_path):
    import evae_oracle as orc
    import smoke_case
    from utils.knn_on_latent import _posterior_means
    from utils.tsne_on_latent import report_tsne_on_latent
    import golden_inputs as gi
    n, B = 75, 32                                        # two full batches; the ragged last one (11 rows) is dropped, as in the kNN report
    args = smoke_case.vae_args(number_components=20, training_set_size=100, batch_size=B)
    args.tsne_n_iter, args.tsne_perplexity, args.seed = 30, 5.0, 3
    model, _ = smoke_case.build_model(torch, np, orc, args)
    model.eval()
    data = torch.from_numpy(gi.binary_images(91, n))
    labels = torch.arange(n) % 10
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, labels), batch_size=B, shuffle=False)
    out = str(tmp_path / "report")
    Y = report_tsne_on_latent(loader, model, out, args)
    assert Y.is_cuda and Y.shape == (64, 2)
    saved, saved_labels = np.load(os.path.join(out, "tsne.npy")), np.load(os.path.join(out, "tsne_labels.npy"))
    assert saved.shape == (64, 2) and saved_labels.shape == (64,) and np.array_equal(saved, Y.cpu().numpy())
    assert np.array_equal(saved_labels, labels[:64].numpy())
    with torch.no_grad():
        assert len(_posterior_means(model, data.cuda(), B)) == 64
