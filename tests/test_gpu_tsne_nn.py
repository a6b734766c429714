"""GPU: t-SNE on sparse affinities with exact repulsion (csrc/evae_tsne_nn.hip), evae.ops.tsne_knn / tsne_nn_*,
evae.tsne.TSNE(method='neighbours') and utils.tsne_on_latent, against the float64 restatement tests/tsne_nn_ref.py (held to
scikit-learn by tests/test_tsne_nn_ref_host.py) and, after P, tests/tsne_ref.py on the densified matrix.

Neighbours are held bit for bit to the oracle.  Every comparison with float64 follows THE TOLERANCE RULE of
tests/test_gpu_tsne.py: the restatement runs a second time in float32 at the same case; a kernel may miss float64 by
max(8 x the float32 restatement's error, 4 x eps32 x scale), per row where the quantity is per row (beta, achieved perplexity).
The yardstick is the reference, never the kernel."""
import os

import numpy as np
import pytest
import torch

import tsne_nn_ref as nn
import tsne_ref as ref

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
ROW_BLOCK = 256      # rows of a repulsion workgroup = columns of its Y tile (csrc/evae_tsne_nn.hip: kRepRows, kRepTile)
CASES = [(97, 40, 5.0), (1025, 40, 30.0)]
FORCE_CASES = [(97, 40, 5.0), (ROW_BLOCK - 1, 40, 30.0), (ROW_BLOCK, 40, 30.0), (ROW_BLOCK + 1, 3, 30.0), (1025, 40, 30.0)]


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


def held_rows(name, got, want64, want32, scale):
    """the rule row by row: one loose row cannot excuse the others"""
    got, want64, want32 = (np.asarray(a, np.float64) for a in (got, want64, want32))
    err, tol = np.abs(got - want64), allowed(np.abs(want32 - want64), scale)
    print("%-28s worst row: kernel at %.3g of its allowance" % (name, (err / tol).max()))
    assert np.all(np.isfinite(got)), name
    assert np.all(err <= tol), (name, np.nonzero(err > tol))


def points(n, zd):
    X, labels = nn.blobs(n, zd, 4, seed=3000 + n)
    if n == 97:
        X[5] += 40.0                        # one far outlier row
        X[20:28] = X[20]                    # eight identical rows
    return X, labels


def oracle_distances(X, rows=None):
    import evae_oracle as orc
    return orc.pairdist_direct_f64(X if rows is None else X[rows], X)


def oracle_neighbours(X, k):
    import evae_oracle as orc
    D = oracle_distances(X)
    D[np.arange(len(X)), np.arange(len(X))] = np.inf
    val, idx = orc.topk_smallest(D, k)
    return idx, val


_cases = {}


def case(n, zd, perp):
    """inputs and both restatements of a case, computed once and shared"""
    key = (n, zd, perp)
    if key not in _cases:
        X, labels = points(n, zd)
        D = oracle_distances(X)
        a64, a32 = nn.affinities(X, perp, np.float64, D=D), nn.affinities(X, perp, np.float32, D=D)
        P = a64["P"].astype(np.float32)      # the matrix the force kernels and both force restatements see
        M = nn.pattern(a64["idx"])
        rows, cols = np.nonzero(M)
        row_ptr = np.concatenate(([0], np.cumsum(M.sum(axis=1))))
        _cases[key] = dict(X=X, labels=labels, a64=a64, a32=a32, P=P, row_ptr=row_ptr, col=cols, val=P[rows, cols])
    return _cases[key]


@pytest.fixture(scope="module")
def ops():
    from evae import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def csr_dev(c):
    return dev(c["row_ptr"], torch.int32), dev(c["col"], torch.int32), dev(c["val"])


def densify(row_ptr, col, val):
    return nn.densify(row_ptr.cpu().numpy(), col.cpu().numpy().astype(np.int64), val.cpu().numpy(), np.float32)


# ---------------------------------------------------------------------------------------------- 1. neighbours
@pytest.mark.parametrize("n,zd,k,strip", [(97, 40, 16, 0), (300, 3, 91, 0), (1025, 40, 91, 0), (600, 8, 256, 0), (200, 40, 31, 64),
                                          (300, 3, 91, 77)])       # 77 rows x 3 floats: strips that start off a 16-byte boundary
def test_neighbours_bit_equal_to_the_oracle(ops, n, zd, k, strip):
    X, _ = points(n, zd)
    want_idx, want_val = oracle_neighbours(X, k)
    idx, d2 = ops.tsne_knn(dev(X), k, strip_rows=strip)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == (n, k) and d2.shape == (n, k)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), want_val.view(np.uint32))
    if n == 97:
        # ties at 0 (a duplicate row's seven twins, itself not among them) and at the k-th place (a row for which the eight
        # identical rows straddle the cut: only the lowest-indexed of them are taken)
        assert np.all(want_val[22, :7] == 0) and 22 not in want_idx[22]
        full = oracle_neighbours(X, k + 1)[1]
        assert np.any(full[:, k] == full[:, k - 1])
    if strip:
        # 200 rows in strips of 64: three full strips and a ragged one of 8; equal to the automatic strip bit for bit
        idx0, d20 = ops.tsne_knn(dev(X), k)
        assert torch.equal(idx, idx0) and torch.equal(d2, d20)
    if strip and k <= 64:
        # tie-free and k <= 64: also what the older top-k kernel gives once the point's own index is dropped
        ti, tv = ops.pairdist_topk(dev(X), dev(X), k + 1)
        own = ti == torch.arange(n, device="cuda")[:, None]
        assert bool((own.sum(dim=1) == 1).all())
        assert torch.equal(ti[~own].reshape(n, k), idx.long()) and torch.equal(tv[~own].reshape(n, k), d2)


def test_neighbours_beyond_256_fail(ops):
    from evae import launch
    from evae._lib import EvaeError
    X = dev(points(600, 8)[0])
    assert ops.tsne_nn_max_neighbours() == 256
    with pytest.raises(EvaeError):
        ops.tsne_knn(X, 257)
    idx, d2 = torch.empty((600, 257), dtype=torch.int32, device="cuda"), torch.empty((600, 257), device="cuda")
    ws = torch.empty(600 * 600 * 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(EvaeError, match="k=257"):             # the entry point's own check, under the operator's
        launch.Launcher(X.device).tsne_knn(X, 600, 8, 257, 0, idx, d2, ws)
    with pytest.raises(EvaeError):
        ops.tsne_knn(X[:20], 20)                              # a point has N - 1 neighbours
    with pytest.raises(EvaeError):
        ops.tsne_knn(torch.zeros(8, 4), 3)


# ---------------------------------------------------------------------------------------------- 2. conditionals
@pytest.mark.parametrize("n,zd,perp", CASES)
def test_conditionals(ops, n, zd, perp):
    c = case(n, zd, perp)
    a64, a32 = c["a64"], c["a32"]
    beta, cond = ops.tsne_nn_conditionals(dev(a64["d2"]), perp)
    assert beta.shape == (n,) and cond.shape == (n, a64["k"])
    beta, cond = beta.cpu().numpy().astype(np.float64), cond.cpu().numpy()
    b64, b32 = a64["beta"], a32["beta"].astype(np.float64)
    held_rows("beta", beta, b64, b32, np.abs(b64))
    pk, p32, p64 = (nn.row_perplexity(a64["d2"], b) for b in (beta, b32, b64))
    held_rows("achieved perplexity", pk, p64, p32, perp)       # the same place as float64 where the target is out of reach
    err_p, tol_p = np.abs(pk - perp), allowed(np.abs(p32 - perp), perp)
    assert np.all(err_p <= tol_p), np.nonzero(err_p > tol_p)
    held("conditionals", cond, a64["cond"], a32["cond"])
    assert np.abs(cond.astype(np.float64).sum(axis=1) - 1.0).max() <= 4 * EPS32
    if n == 97:
        assert np.all(beta[20:28] == 2.0 ** nn.SEARCH_STEPS) and np.allclose(pk[20:28], 7.0)
        assert np.all(cond[20, :7] == cond[20, 0]) and np.all(cond[20, 7:] == 0)


# ---------------------------------------------------------------------------------------------- 3. joint
def check_structure(row_ptr, col, val, n, k):
    assert row_ptr.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float32
    nnz = col.numel()
    assert row_ptr.shape == (n + 1,) and val.shape == (nnz,) and nnz <= 2 * n * k
    rp = row_ptr.long()
    assert int(rp[0]) == 0 and int(rp[-1]) == nnz and bool((rp[1:] >= rp[:-1]).all())
    rows = torch.repeat_interleave(torch.arange(n, device="cuda"), rp[1:] - rp[:-1])
    keys = rows * n + col.long()
    assert bool((keys[1:] > keys[:-1]).all())                                   # columns strictly ascending within a row
    assert bool((rows != col.long()).all())                                     # no diagonal
    tkeys, order = torch.sort(col.long() * n + rows)                            # the transposed entries, in key order
    assert torch.equal(tkeys, keys)                                             # (i, j) present <=> (j, i) present
    assert torch.equal(val[order].view(torch.int32), val.view(torch.int32))     # and bit-equal
    assert bool(torch.isfinite(val).all()) and bool((val >= 0).all())
    assert abs(float(val.double().sum()) - 1.0) <= 1e-6


@pytest.mark.parametrize("n,zd,perp", CASES)
def test_joint(ops, n, zd, perp):
    c = case(n, zd, perp)
    a64, a32 = c["a64"], c["a32"]
    row_ptr, col, val, beta = ops.tsne_nn_affinities(dev(c["X"]), perp)
    check_structure(row_ptr, col, val, n, a64["k"])
    assert np.array_equal(row_ptr.cpu().numpy(), c["row_ptr"]) and np.array_equal(col.cpu().numpy(), c["col"])
    held("P", densify(row_ptr, col, val), a64["P"], a32["P"])
    held_rows("beta", beta.cpu().numpy(), a64["beta"], a32["beta"], np.abs(a64["beta"]))


def test_joint_with_every_point_a_neighbour_is_the_dense_kernels(ops):
    """N = 61, perplexity 20: k = 60 = N - 1; the CSR joint and the dense kernel's P both against float64 by the rule, and
    against each other within the same allowance"""
    X, _ = points(61, 40)
    D = oracle_distances(X)
    a64, a32 = nn.affinities(X, 20.0, np.float64, D=D), nn.affinities(X, 20.0, np.float32, D=D)
    row_ptr, col, val, _ = ops.tsne_nn_affinities(dev(X), 20.0)
    check_structure(row_ptr, col, val, 61, 60)
    assert col.numel() == 61 * 60
    Pn = densify(row_ptr, col, val)
    Pd = ops.tsne_affinities(dev(X), 20.0)[0].cpu().numpy()
    held("sparse P", Pn, a64["P"], a32["P"])
    held("dense kernel P", Pd, a64["P"], a32["P"])
    held("sparse P vs dense kernel", Pn, Pd.astype(np.float64), Pd.astype(np.float64) + (a32["P"] - a64["P"]), scale=float(a64["P"].max()))


# ---------------------------------------------------------------------------------------------- 4. forces
def embedding(n, scale, seed=11):
    Y = (np.random.RandomState(seed).randn(n, 2) * scale).astype(np.float32)
    Y[3] = Y[17]                             # two coincident points
    return Y


def check_forces(ops, part, P, Y, exag, tag):
    g64, Z64, kl64, A64, R64 = ref.forces(P, Y, exag, np.float64)
    g32, Z32, kl32, A32, R32 = ref.forces(P, Y, exag, np.float32)
    stats = ops.tsne_stats(part, True).cpu().numpy()
    pn = part.cpu().numpy()
    held(tag + "A", pn[:, 0:2], A64, A32)
    held(tag + "R", pn[:, 2:4], R64, R32)
    held(tag + "Z", stats[0], Z64, Z32)
    held(tag + "KL", stats[1], kl64, kl32, scale=max(abs(kl64), 1.0))
    return (g64, g32, Z64, Z32)


@pytest.mark.parametrize("scale", [1e-4, 1.0, 30.0])
@pytest.mark.parametrize("n,zd,perp", FORCE_CASES)
def test_forces_gradient_and_kl(ops, n, zd, perp, scale):
    c = case(n, zd, perp)
    Y = embedding(n, scale)
    csr, Yd = csr_dev(c), dev(Y)
    for exag in (12.0, 1.0):
        tag = "scale %g exag %g: " % (scale, exag)
        part = ops.tsne_nn_forces(*csr, Yd, exag, True)
        assert part.shape == (n, 8) and part.dtype == torch.float64
        g64, g32, Z64, Z32 = check_forces(ops, part, c["P"], Y, exag, tag)
        # the gradient as the unchanged update launch forms it (lr 0: nothing moves but the re-centring)
        Yc, v, ga = Yd.clone(), torch.zeros_like(Yd), torch.ones_like(Yd)
        plain = ops.tsne_nn_forces(*csr, Yd, exag, False)
        grad, st2 = ops.tsne_update(plain, Yc, v, ga, 0.5, 0.0, want_grad=True)
        held(tag + "gradient", grad.cpu().numpy(), g64, g32)
        held(tag + "Z (update launch)", float(st2[0]), Z64, Z32)
        assert float(st2[1]) == 0.0 and bool((plain[:, 5:7] == 0).all()) and bool((part[:, 5:7] != 0).all())
        assert torch.equal(plain[:, :5], part[:, :5])            # want_kl adds K and S and changes nothing else
        assert torch.equal(part, ops.tsne_nn_forces(*csr, Yd, exag, True))     # fixed summation order


def test_forces_with_every_point_a_neighbour_are_the_dense_kernels(ops):
    X, _ = points(61, 40)
    a64 = nn.affinities(X, 20.0, np.float64, D=oracle_distances(X))
    P = a64["P"].astype(np.float32)
    rows, cols = np.nonzero(nn.pattern(a64["idx"]))
    csr = (dev(np.arange(62) * 60, torch.int32), dev(cols, torch.int32), dev(P[rows, cols]))
    for scale in (1e-4, 1.0, 30.0):
        Y = embedding(61, scale)
        sparse = ops.tsne_nn_forces(*csr, dev(Y), 12.0, True)
        dense = ops.tsne_forces(dev(P), dev(Y), 12.0, True)
        check_forces(ops, sparse, P, Y, 12.0, "sparse, scale %g: " % scale)
        check_forces(ops, dense, P, Y, 12.0, "dense,  scale %g: " % scale)


# ---------------------------------------------------------------------------------------------- 5. one descent step
@pytest.mark.parametrize("momentum", [0.5, 0.8])
@pytest.mark.parametrize("n,zd,perp", CASES)
def test_update_step(ops, n, zd, perp, momentum):
    c = case(n, zd, perp)
    P = c["P"]
    Y = embedding(n, 1.0, seed=12)
    rs = np.random.RandomState(13)
    g64 = ref.forces(P, Y, 1.0, np.float64, want_kl=False)[0]
    g32 = ref.forces(P, Y, 1.0, np.float32, want_kl=False)[0]
    vel = (np.where(rs.rand(n, 2) < 0.5, 1.0, -1.0) * np.sign(g64) * (0.5 + rs.rand(n, 2)) * np.abs(g64).max()).astype(np.float32)
    vel[np.sign(g64) == 0] = 0.0
    gains = rs.choice([1.0, 0.05, 0.011, 0.0124, 2.5], size=(n, 2)).astype(np.float32)
    lr = ref.learning_rate(n)
    Y64, v64, ga64 = ref.update(Y, vel, gains, g64, momentum, lr, np.float64)
    Y32, v32, ga32 = ref.update(Y, vel, gains, g32, momentum, lr, np.float32)
    Yd, vd, gd = dev(Y), dev(vel), dev(gains)
    ops.tsne_update(ops.tsne_nn_forces(*csr_dev(c), Yd, 1.0, False), Yd, vd, gd, momentum, lr)
    held("gains", gd.cpu().numpy(), ga64, ga32)
    held("velocity", vd.cpu().numpy(), v64, v32)
    held("Y", Yd.cpu().numpy(), Y64, Y32)
    mean = Yd.double().mean(dim=0).abs().max().item()
    assert mean <= 4.0 * EPS32 * np.abs(Y64).max(), mean


# ---------------------------------------------------------------------------------------------- 6. end to end
def test_end_to_end_against_the_reference_spread():
    """300 points, three blobs, perplexity 30 (k = 91), 500 iterations of which 125 exaggerated, five inits.  The yardstick is the
    float64 restatement's own spread over the five: the device's final KL -- evaluated in float64 from the float64 sparse P --
    must lie within [min - spread, max + spread], and every point's 10 nearest neighbours in the embedding carry its own
    blob's label, as in all five reference runs.  (The descent is chaotic, so the restatement's digits vary with the host: five
    runs gave KL 0.7838 .. 0.7940 on one CPU and 0.7872 .. 0.7932 on another, the device 0.7864 .. 0.7975 beside the latter.)"""
    from evae.tsne import TSNE
    n, n_iter, n_exag = 300, 500, 125
    X, labels = nn.blobs(n, 40, 3, 0)
    P64 = nn.affinities(X, 30.0)["P"]
    inits = [(np.random.RandomState(s).randn(n, 2) * 1e-4).astype(np.float32) for s in range(5)]
    ref_runs = [nn.run(P64, Y0, n_iter, n_exag) for Y0 in inits]
    ref_kl = np.array([kl for _, kl in ref_runs])
    assert all(nn.neighbour_purity(Y, labels) == 1.0 for Y, _ in ref_runs)
    spread = ref_kl.max() - ref_kl.min()
    Xd = dev(X)
    dev_kl, dev_purity, own_kl = [], [], []
    for Y0 in inits:
        t = TSNE(perplexity=30.0, n_iter=n_iter, exaggerated_iters=n_exag, init=torch.from_numpy(Y0), method='neighbours')
        Y = t.fit_transform(Xd).cpu().numpy()
        assert np.all(np.isfinite(Y)) and t.n_iter_ == n_iter
        dev_kl.append(float(ref.forces(P64, Y, 1.0)[2]))
        dev_purity.append(nn.neighbour_purity(Y, labels))
        own_kl.append(t.kl_divergence_)
    print("reference KL %s (spread %.4g)" % (np.round(ref_kl, 5), spread))
    print("device    KL %s, purity %s; kl_divergence_ %s" % (np.round(dev_kl, 5), dev_purity, np.round(own_kl, 5)))
    assert min(dev_kl) >= ref_kl.min() - spread and max(dev_kl) <= ref_kl.max() + spread
    assert min(dev_purity) == 1.0
    assert np.abs(np.array(own_kl) - np.array(dev_kl)).max() <= 1e-4 * max(dev_kl)     # the device's own float32-P evaluation


def test_fit_transform_is_deterministic():
    from evae.tsne import TSNE
    X = dev(points(200, 40)[0])
    runs = [TSNE(random_state=5, n_iter=60, exaggerated_iters=15, method='neighbours') for _ in range(2)]
    Ya, Yb = (t.fit_transform(X).clone() for t in runs)
    assert torch.equal(Ya, Yb) and runs[0].kl_divergence_ == runs[1].kl_divergence_ and runs[0].n_iter_ == 60
    assert torch.all(torch.isfinite(Ya)) and Ya.is_cuda and Ya.shape == (200, 2)
    Yc = TSNE(random_state=6, n_iter=60, exaggerated_iters=15, method='neighbours').fit_transform(X)
    assert not torch.equal(Ya, Yc)


# ---------------------------------------------------------------------------------------------- 7. above the old cap
def test_above_the_dense_cap(ops):
    """N = 33 000 (the dense path stops at 32 768; its P would be 4.06 GiB), zd 8, ten blobs, perplexity 10 (k = 31), 3 iterations;
    48 sampled rows against float64"""
    from evae.tsne import TSNE
    n, zd, perp, k = 33000, 8, 10.0, 31
    assert ops.tsne_max_points() < n <= ops.tsne_nn_max_points() and ops.tsne_nn_max_points() >= 131072
    X, _ = nn.blobs(n, zd, 10, seed=33)
    Xd = dev(X)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t = TSNE(perplexity=perp, n_iter=3, exaggerated_iters=2, random_state=0, method='neighbours')
    Y = t.fit_transform(Xd)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("N = %d: device memory allocated by the fit peaks at %.1f MiB" % (n, peak / 2.0 ** 20))
    assert peak < 2 ** 30
    assert Y.shape == (n, 2) and bool(torch.isfinite(Y).all()) and np.isfinite(t.kl_divergence_) and t.n_iter_ == 3
    with pytest.raises(ValueError):
        TSNE().fit_transform(torch.zeros(n, 2))                 # method='exact' still refuses

    rows = np.sort(np.random.RandomState(1).choice(n, 48, replace=False))
    rows[0], rows[-1] = 0, n - 1
    # neighbours, on those rows only
    import evae_oracle as orc
    D = oracle_distances(X, rows)
    D[np.arange(48), rows] = np.inf
    want_val, want_idx = orc.topk_smallest(D, k)
    idx, d2 = ops.tsne_knn(Xd, k)
    assert np.array_equal(idx.cpu().numpy()[rows], want_idx)
    assert np.array_equal(d2.cpu().numpy()[rows].view(np.uint32), want_val.view(np.uint32))
    # beta
    row_ptr, col, val, beta = ops.tsne_nn_affinities(Xd, perp)
    b64, b32 = nn.search_beta(want_val, perp, np.float64), nn.search_beta(want_val, perp, np.float32)
    held_rows("beta", beta.cpu().numpy()[rows], b64, b32, np.abs(b64))
    check_rp = row_ptr.long()
    assert int(check_rp[-1]) == col.numel() <= 2 * n * k and bool((check_rp[1:] - check_rp[:-1] >= k).all())
    # forces at a spread-out embedding: R_i and Z_i over all 33 000 columns, A_i over the kernel's own CSR row
    Yh = (np.random.RandomState(2).randn(n, 2) * 5.0).astype(np.float32)
    Yh[rows[3]] = Yh[rows[7]]                                    # two coincident points among the sampled rows
    part = ops.tsne_nn_forces(row_ptr, col, val, dev(Yh), 12.0, False).cpu().numpy()[rows]
    rp, cl, vl = row_ptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()
    sums = {}
    for dtype in (np.float64, np.float32):
        Yt = Yh.astype(dtype)
        dx = Yt[rows, 0][:, None] - Yt[None, :, 0]
        dy = Yt[rows, 1][:, None] - Yt[None, :, 1]
        w = dtype(1) / (dtype(1) + (dx * dx + dy * dy))
        R = np.stack(((w * w * dx).sum(axis=1), (w * w * dy).sum(axis=1)), axis=1)
        w[np.arange(48), rows] = 0
        A = np.zeros((48, 2), dtype)
        for m, i in enumerate(rows):
            js, p = cl[rp[i]:rp[i + 1]], vl[rp[i]:rp[i + 1]].astype(dtype)
            ex, ey = Yt[i, 0] - Yt[js, 0], Yt[i, 1] - Yt[js, 1]
            pw = p * (dtype(1) / (dtype(1) + (ex * ex + ey * ey)))
            A[m] = dtype(12) * np.array([(pw * ex).sum(), (pw * ey).sum()], dtype)
        sums[dtype] = (A, R, w.sum(axis=1))
    (A64, R64, Z64), (A32, R32, Z32) = sums[np.float64], sums[np.float32]
    held("A (48 rows)", part[:, 0:2], A64, A32)
    held("R (48 rows)", part[:, 2:4], R64, R32)
    held_rows("Z_i (48 rows)", part[:, 4], Z64, Z32, np.abs(Z64))


# ---------------------------------------------------------------------------------------------- 8. routing and interface
def test_interface_errors(ops):
    from evae.tsne import TSNE
    from evae._lib import EvaeError
    X = dev(points(97, 40)[0])
    with pytest.raises(ValueError, match="'exact' and 'neighbours'"):
        TSNE(method='barnes_hut')
    with pytest.raises(ValueError, match="'exact' and 'neighbours'"):
        TSNE(method='nearest')
    with pytest.raises(ValueError, match="85"):
        TSNE(method='neighbours', perplexity=86.0)
    assert TSNE(method='neighbours', perplexity=85.0).method == 'neighbours' and TSNE().method == 'exact'
    assert TSNE(perplexity=86.0).perplexity == 86.0              # the dense path has no such bound
    with pytest.raises(ValueError):
        TSNE(method='neighbours', perplexity=97.0).fit_transform(X)
    with pytest.raises(ValueError):
        TSNE(method='neighbours').fit_transform(torch.zeros(ops.tsne_nn_max_points() + 1, 2))
    c = case(97, 40, 5.0)
    rp, col, val = csr_dev(c)
    Y = dev(embedding(97, 1.0))
    with pytest.raises(EvaeError):
        ops.tsne_nn_forces(rp.long(), col, val, Y)
    with pytest.raises(EvaeError):
        ops.tsne_nn_forces(rp, col.long(), val, Y)
    with pytest.raises(EvaeError):
        ops.tsne_nn_forces(rp, col, val.double(), Y)
    with pytest.raises(EvaeError):
        ops.tsne_nn_forces(rp[:-1], col, val, Y)
    with pytest.raises(EvaeError):
        ops.tsne_nn_forces(rp, col, val, Y.double())
    with pytest.raises(EvaeError):
        ops.tsne_nn_forces(rp.cpu(), col.cpu(), val.cpu(), Y.cpu())
    with pytest.raises(EvaeError):
        ops.tsne_nn_affinities(X, 97.0)
    with pytest.raises(EvaeError):
        ops.tsne_nn_affinities(torch.zeros(8, 4), 2.0)
    with pytest.raises(EvaeError):
        ops.tsne_nn_conditionals(dev(c["a64"]["d2"]).double(), 5.0)


def test_report_tsne_on_latent_routes_the_method(tmp_path):
    import evae_oracle as orc
    import smoke_case
    from evae import _lib
    from utils.tsne_on_latent import report_tsne_on_latent
    import golden_inputs as gi
    n, B = 75, 32
    args = smoke_case.vae_args(number_components=20, training_set_size=100, batch_size=B)
    args.tsne_n_iter, args.tsne_perplexity, args.seed, args.tsne_method = 30, 5.0, 3, 'neighbours'
    model, _ = smoke_case.build_model(torch, np, orc, args)
    model.eval()
    data = torch.from_numpy(gi.binary_images(91, n))
    labels = torch.arange(n) % 10
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, labels), batch_size=B, shuffle=False)
    out = str(tmp_path / "report")
    with _lib.count_calls("evae_tsne_") as calls:
        Y = report_tsne_on_latent(loader, model, out, args)
    assert calls.get("evae_tsne_nn_forces") == 31 and calls.get("evae_tsne_knn") == 1 and "evae_tsne_forces" not in calls
    assert Y.is_cuda and Y.shape == (64, 2) and bool(torch.isfinite(Y).all())
    saved, saved_labels = np.load(os.path.join(out, "tsne.npy")), np.load(os.path.join(out, "tsne_labels.npy"))
    assert saved.shape == (64, 2) and saved_labels.shape == (64,) and np.array_equal(saved, Y.cpu().numpy())
    assert np.array_equal(saved_labels, labels[:64].numpy())
    args.tsne_method = 'barnes_hut'
    with pytest.raises(ValueError):
        report_tsne_on_latent(loader, model, out, args)
