"""GPU: ball counts and nearest columns (csrc/evae_ball_count.hip), evae.ops.ball_count / kth_neighbour_radius,
evae.sample_quality and the report of utils.sample_quality_on_latent, against the numpy restatement tests/sample_quality_ref.py
(held to scikit-learn and the `prdc` expressions by tests/test_sample_quality_ref_host.py) on the oracle's distances.

Everything here is an integer, or integers through one float64 expression, so every comparison is for equality.  The yardstick is
the restatement, never the kernel."""
import json
import os

import numpy as np
import pytest
import torch

import sample_quality_ref as rr
from tsne_ref import blobs

pytestmark = pytest.mark.gpu

ROW_TILE = 1024      # distances one pass of a counting workgroup takes: 256 threads x one 16-byte load (csrc/evae_ball_count.hip)
# (B, N, d): queries, columns, width.  The ROW_TILE cases have 5 query rows: a row starts at i * N floats, so with N = 1023 and
# 1025 the five rows start on every phase of a 16-byte boundary (head of 0, 1, 2, 3 scalars) and end in tails of 0 .. 3.
CASES = [(61, 97, 40), (257, 300, 3), (5, ROW_TILE - 1, 8), (5, ROW_TILE, 8), (5, ROW_TILE + 1, 8), (300, 7, 2), (1, 1, 1)]


def oracle_distances(A, B):
    import evae_oracle as orc
    return orc.pairdist_direct_f64(np.asarray(A, np.float32), np.asarray(B, np.float32))


def two_sets(b, n, d, seed=None):
    """two samples of one mixture of blobs -> (q [b x d], c [n x d]), with the outlier and the identical rows of
    test_gpu_nn_rank.py's points in each set that is large enough, and tied nearest columns where there are at least 64 columns"""
    X = blobs(b + n, d, 4, seed=5000 + 7 * b + n if seed is None else seed)[0]
    q, c = X[:b].copy(), X[b:].copy()
    for S in (q, c):
        if len(S) >= 61:
            S[5] += 40.0                    # one far outlier row
            S[20:28] = S[20]                # eight identical rows: radius 0 up to k = 7
    if n >= 64 and b >= 5:
        # ties for the minimum.  The lower column wins, whichever thread saw it: copies of one column in the head of a row (or,
        # for a row that starts on a boundary, its first 16-byte load), in the first full load behind every head, and in the
        # tail (the last load where there is no tail) -- and the queries that sit on them, at distance 0 from every copy.
        c[6] = c[n - 1] = c[1]
        c[n - 2] = c[4]
        c[n - 3] = c[n - 4]                 # a tie whose winner sits at the end of the row too: both copies in the last columns
        q[0], q[1], q[2] = c[1], c[4], c[n - 4]
        q[3] = 0.5 * (c[1] + c[4])          # not on a column: equally far from each copy within a group, bit for bit
    return q, c


_cases = {}


def case(b, n, d):
    """inputs, the oracle's distances and the radii of a case, computed once, shared and left alone"""
    key = (b, n, d)
    if key not in _cases:
        q, c = two_sets(b, n, d)
        D = oracle_distances(q, c)
        col, row = {}, {}
        for k in (1, 5):
            if n > k:
                col["k%d" % k] = rr.radii(oracle_distances(c, c), k)
            if b > k:
                row["k%d" % k] = rr.radii(oracle_distances(q, q), k)
        col["zero"], row["zero"] = np.zeros(n, np.float32), np.zeros(b, np.float32)
        col["inf"], row["inf"] = np.full(n, np.inf, np.float32), np.full(b, np.inf, np.float32)
        col["median"], row["median"] = np.full(n, np.median(D), np.float32), np.full(b, np.median(D), np.float32)
        _cases[key] = dict(q=q, c=c, D=D, col=col, row=row, nearest=rr.nearest(D))
    return _cases[key]


@pytest.fixture(scope="module")
def ops():
    from evae import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def same(got, D, col_radius, row_radius, nearest):
    """every output of a ball_count call against the restatement on D; what was switched off is None"""
    want_col, want_row = rr.ball_counts(D, col_radius, row_radius)
    for name, have, want in (("col_hits", got.col_hits, want_col), ("row_hits", got.row_hits, want_row)):
        if want is None:
            assert have is None, name
        else:
            assert have.dtype == torch.int32 and have.shape == (len(D),), name
            assert np.array_equal(have.cpu().numpy(), want), name
    if nearest is None:
        assert got.nn_idx is None and got.nn_d2 is None
    else:
        assert got.nn_idx.dtype == torch.int32 and got.nn_d2.dtype == torch.float32
        assert got.nn_idx.shape == got.nn_d2.shape == (len(D),)
        assert np.array_equal(got.nn_idx.cpu().numpy(), nearest[0])
        assert np.array_equal(got.nn_d2.cpu().numpy().view(np.uint32), np.asarray(nearest[1], np.float32).view(np.uint32))


# ---------------------------------------------------------------------------------------------- 1. counts and nearest columns
@pytest.mark.parametrize("b,n,d", CASES)
def test_ball_counts_and_nearest_columns(ops, b, n, d):
    c = case(b, n, d)
    q, cols, D = dev(c["q"]), dev(c["c"]), c["D"]
    assert "zero" in c["col"] and "inf" in c["col"] and (n == 1 or "k1" in c["col"]) and (b <= 5 or "k5" in c["row"])
    for name in c["col"]:                                             # both radii, and the nearest column with them
        for rname in ([name] if name in c["row"] else ["median"]):
            cr, rrad = c["col"][name], c["row"][rname]
            same(ops.ball_count(q, cols, col_radius=dev(cr), row_radius=dev(rrad)), D, cr, rrad, c["nearest"])
    for name, cr in c["col"].items():                                 # each alone, nothing else asked for
        same(ops.ball_count(q, cols, col_radius=dev(cr), want_nearest=False), D, cr, None, None)
    for name, rrad in c["row"].items():
        same(ops.ball_count(q, cols, row_radius=dev(rrad), want_nearest=False), D, None, rrad, None)
    same(ops.ball_count(q, cols), D, None, None, c["nearest"])        # the nearest column only
    zero = ops.ball_count(q, cols, col_radius=dev(c["col"]["zero"]), row_radius=dev(c["row"]["zero"]), want_nearest=False)
    assert not zero.col_hits.any() and not zero.row_hits.any()        # strict: nothing is below 0, not even a distance of 0
    full = ops.ball_count(q, cols, col_radius=dev(c["col"]["inf"]), row_radius=dev(c["row"]["inf"]), want_nearest=False)
    assert bool((full.col_hits == n).all()) and bool((full.row_hits == n).all())
    if n >= 64 and b >= 5:
        idx, d2 = c["nearest"]
        assert idx[:3].tolist() == [1, 4, n - 4] and d2[:3].tolist() == [0.0, 0.0, 0.0]       # the lowest copy, from any part of a row
        assert D[0, 1] == D[0, 6] == D[0, n - 1] and D[1, 4] == D[1, n - 2] and D[2, n - 4] == D[2, n - 3]
        assert D[3, 1] == D[3, 6] == D[3, n - 1] and D[3, 4] == D[3, n - 2]
    if (b, n) == (61, 97):
        assert c["col"]["k5"][20:28].max() == 0.0 and c["col"]["k1"][5] > 1000.0              # the identical rows, the outlier
        hits = rr.ball_counts(D, c["col"]["k5"], c["row"]["k5"])
        assert 0 < np.count_nonzero(hits[0]) < b and 0 < np.count_nonzero(hits[1]) < b        # the counts count


# ---------------------------------------------------------------------------------------------- 2. strips, repeated calls
def test_the_result_does_not_depend_on_the_strip(ops):
    c = case(257, 300, 3)
    q, cols, cr, rrad = dev(c["q"]), dev(c["c"]), dev(c["col"]["k5"]), dev(c["row"]["k5"])
    first = ops.ball_count(q, cols, col_radius=cr, row_radius=rrad)
    same(first, c["D"], c["col"]["k5"], c["row"]["k5"], c["nearest"])
    for strip in (0, 64, 77):            # 257 rows: full strips and a ragged last one; 77 x 300 floats: strips of every phase
        again = ops.ball_count(q, cols, col_radius=cr, row_radius=rrad, strip_rows=strip)
        for a, b in zip(first, again):
            assert torch.equal(a, b), strip


# ---------------------------------------------------------------------------------------------- 3. pixel width
@pytest.mark.parametrize("b,n,d", [(70, 130, 784), (70, 130, 100)])
def test_rows_as_wide_as_images(ops, b, n, d):
    """the distance kernel walks d in chunks of 64: 784 = 12 chunks and a part of one, 100 = one and a part"""
    c = case(b, n, d)
    got = ops.ball_count(dev(c["q"]), dev(c["c"]), col_radius=dev(c["col"]["k5"]), row_radius=dev(c["row"]["k5"]))
    same(got, c["D"], c["col"]["k5"], c["row"]["k5"], c["nearest"])
    assert np.array_equal(ops.pairwise_distance(dev(c["q"]), dev(c["c"])).cpu().numpy().view(np.uint32), c["D"].view(np.uint32))


# ---------------------------------------------------------------------------------------------- 4. radii
@pytest.mark.parametrize("n,d,k", [(97, 40, 1), (97, 40, 5), (300, 3, 1), (300, 3, 5), (300, 3, 256)])
def test_kth_neighbour_radius(ops, n, d, k):
    X = two_sets(61, n, d)[1]
    want = rr.radii(oracle_distances(X, X), k)
    got = ops.kth_neighbour_radius(dev(X), k)
    assert got.dtype == torch.float32 and got.shape == (n,) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert want[20:28].max() == 0.0 if k <= 7 else want.min() > 0.0


# ---------------------------------------------------------------------------------------------- 5. the scores
SIZES = [(97, 61, 40, 5), (300, 257, 3, 1), (300, 300, 8, 12)]
N_TRAIN = 120


def score_sets(n, m, d, variant):
    """real [n x d], generated [m x d], training [N_TRAIN x d]: three samples of one mixture, then the variant's generated rows"""
    X = blobs(n + m + N_TRAIN, d, 4, seed=8000 + n + m)[0]
    real, fake, train = X[:n].copy(), X[n:n + m].copy(), X[n + m:].copy()
    real[5] += 40.0
    real[20:28] = real[20]
    if variant == "same":                   # the generated rows are the real ones (m of them)
        fake = real[:m].copy()
    elif variant == "copies":               # every other generated row is a copy of a training row
        fake[::2] = train[(np.arange(len(fake[::2])) * 7) % N_TRAIN]
    elif variant == "translated":           # the training rows, moved far away
        fake = (train[np.arange(m) % N_TRAIN] - 30.0).astype(np.float32)       # away from the real outlier, whose ball is wide
        fake += 1e-3 * np.arange(m, dtype=np.float32)[:, None]       # no two of them equal
    return real, fake, train


@pytest.mark.parametrize("variant", ["plain", "same", "copies", "translated"])
@pytest.mark.parametrize("n,m,d,k", SIZES)
def test_scores_are_the_restatements_floats(n, m, d, k, variant):
    from evae import sample_quality as sq
    real, fake, train = score_sets(n, m, d, variant)
    DRR, DFF, DRF = oracle_distances(real, real), oracle_distances(fake, fake), oracle_distances(real, fake)
    DTT, DTF = oracle_distances(train, train), oracle_distances(train, fake)
    R, F, T = dev(real), dev(fake), dev(train)

    want = rr.prdc(DRR, DFF, DRF, k)
    got = sq.compute_prdc(R, F, nearest_k=k)
    print("device %s\nreference %s" % (got, want))
    assert got == want and list(got) == ["precision", "recall", "density", "coverage", "nearest_k", "n_real", "n_fake"]
    assert all(type(got[key]) is float for key in ("precision", "recall", "density", "coverage"))
    assert all(type(got[key]) is int for key in ("nearest_k", "n_real", "n_fake"))
    assert sq.compute_prdc(R.double(), F.double(), k, strip_rows=77) == want       # any float dtype (these are exact in fp32), any strip

    idx, d2 = sq.nearest_real(T, F)
    want_idx, want_d2 = rr.nearest(DTF.T)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (m,)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(d2.cpu().numpy().view(np.uint32), want_d2.view(np.uint32))

    a, a_real = sq.authenticity(T, F), sq.authenticity(R, F)
    assert type(a) is float and a == rr.authenticity(DTT, DTF) and a_real == rr.authenticity(DRR, DRF)

    whole, want_whole = sq.sample_quality(R, F, nearest_k=k, train=T), rr.sample_quality(DRR, DFF, DRF, k, DTT, DTF)
    print("device %s\nreference %s" % (whole, want_whole))
    assert whole == want_whole and type(whole["authenticity"]) is float and type(whole["nearest_distance_median"]) is float
    assert sq.sample_quality(R, F, nearest_k=k) == rr.sample_quality(DRR, DFF, DRF, k)

    if variant == "plain":
        assert 0.0 < want["precision"] < 1.0 and 0.0 < want["recall"] < 1.0 and 0.0 < want["coverage"] <= 1.0
    elif variant == "same":                 # every row with a ball of its own is inside it; the eight identical rows have none at k <= 7
        assert want["precision"] >= (m - 8) / m and a_real == 8 / m       # 0 >= 0: only the identical rows pass for authentic
        if k > 7 and m == n:
            assert want["precision"] == want["recall"] == want["coverage"] == 1.0
    elif variant == "copies":               # the copies are inauthentic, and found where they were taken from
        assert a <= (m // 2) / m
        assert np.array_equal(want_idx[::2], (np.arange(len(want_idx[::2])) * 7) % N_TRAIN) and not want_d2[::2].any()
    elif variant == "translated":           # nowhere near anything: in no ball, covering nothing, all authentic
        assert want["precision"] == want["recall"] == want["coverage"] == want["density"] == 0.0 and a == 1.0


# ---------------------------------------------------------------------------------------------- 6. guards
def test_interface_errors(ops, monkeypatch):
    from evae import _lib, sample_quality as sq
    from evae._lib import EvaeError
    c = case(61, 97, 40)
    q, cols, cr, rrad = dev(c["q"]), dev(c["c"]), dev(c["col"]["k5"]), dev(c["row"]["k5"])
    for bad in (lambda: ops.ball_count(q.cpu(), cols.cpu()), lambda: ops.ball_count(q, cols.cpu()),
                lambda: ops.ball_count(q, cols, col_radius=cr.cpu()),
                lambda: ops.ball_count(q, cols[:, :39]),                              # unequal d
                lambda: ops.ball_count(q[0], cols), lambda: ops.ball_count(q, cols[0]),      # 1-D
                lambda: ops.ball_count(q, cols, col_radius=cr[:-1]), lambda: ops.ball_count(q, cols, col_radius=rrad),
                lambda: ops.ball_count(q, cols, row_radius=cr), lambda: ops.ball_count(q, cols, row_radius=rrad.double()),
                lambda: ops.ball_count(q, cols, col_radius=cr.reshape(-1, 1)),
                lambda: ops.ball_count(q, cols, want_nearest=False),                  # nothing asked for
                lambda: ops.ball_count(q, cols, strip_rows=-1),
                lambda: sq.compute_prdc(cols.cpu(), q.cpu()), lambda: sq.nearest_real(cols.cpu(), q),
                lambda: sq.authenticity(cols, q.cpu()), lambda: sq.sample_quality(cols.cpu(), q.cpu())):
        with pytest.raises(EvaeError):
            bad()
    for bad in (lambda: sq.compute_prdc(cols, q[:, :39]), lambda: sq.compute_prdc(cols[0], q), lambda: sq.nearest_real(cols, q[0]),
                lambda: sq.authenticity(cols[:, :3], q), lambda: sq.sample_quality(cols, q, train=cols[:, :5]),
                lambda: sq.compute_prdc(cols, q, nearest_k=0), lambda: sq.compute_prdc(cols, q, nearest_k=61),      # = min(N, M)
                lambda: sq.sample_quality(cols, q, nearest_k=97)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match=r"nearest_k=61 .*N=97, M=61.* 60\]"):
        sq.compute_prdc(cols, q, nearest_k=61)
    assert sq.compute_prdc(cols, q, nearest_k=60)["nearest_k"] == 60
    wide = torch.zeros((300, 3), device="cuda")
    cap = ops.tsne_nn_max_neighbours()
    with pytest.raises(ValueError, match="nearest_k=%d above" % (cap + 1)):
        sq.compute_prdc(wide, wide, nearest_k=cap + 1)
    # above the cap on points: the operator's own check, against a cap made small (no 131 073-row allocation)
    assert ops.ball_count_max_points() == ops.tsne_nn_max_points()
    with monkeypatch.context() as m:
        m.setattr(ops, "ball_count_max_points", lambda: 96)
        with pytest.raises(EvaeError, match="N=97 outside"):
            ops.ball_count(q, cols)
        with pytest.raises(EvaeError, match="B=97"):
            ops.ball_count(cols, q)
        assert ops.ball_count(q, cols[:96]).nn_idx.shape == (61,)
    # the entry point's own checks, under the operator's: every pointer is a live buffer of the right size, nothing is launched
    lib, vp = _lib.load(), _lib.vp
    hits, idx, d2 = torch.full((61,), -7, dtype=torch.int32, device="cuda"), torch.empty(61, dtype=torch.int32, device="cuda"), torch.empty(61, device="cuda")
    ws = torch.empty(lib.evae_ball_count_workspace_bytes(61, 97, 0), dtype=torch.uint8, device="cuda")
    assert ws.numel() == 61 * 97 * 4 and lib.evae_ball_count_workspace_bytes(61, 97, 16) == 16 * 97 * 4

    def raw(B=61, N=97, d=40, col_radius=None, row_radius=None, strip=0, col_hits=None, row_hits=None, nn_idx=idx, nn_d2=d2, ws_bytes=None):
        return lib.evae_ball_count(vp(q), B, vp(cols), N, d, vp(col_radius), vp(row_radius), strip, vp(col_hits), vp(row_hits), vp(nn_idx),
                                   vp(nn_d2), vp(ws), ws.numel() if ws_bytes is None else ws_bytes, None)

    for call, word in ((lambda: raw(col_hits=hits), b"col_hits"), (lambda: raw(row_hits=hits), b"row_hits"),
                       (lambda: raw(col_radius=cr), b"col_radius"), (lambda: raw(row_radius=rrad), b"row_radius"),
                       (lambda: raw(nn_idx=None, nn_d2=None), b"no output"), (lambda: raw(B=0), b"B=0"),
                       (lambda: raw(N=ops.tsne_nn_max_points() + 1), b"N=%d" % (ops.tsne_nn_max_points() + 1)), (lambda: raw(d=0), b"d=0"),
                       (lambda: raw(strip=-1), b"strip_rows"), (lambda: raw(ws_bytes=ws.numel() - 4), b"workspace")):
        assert call() != 0
        assert word in lib.evae_last_error(), word
    torch.cuda.synchronize()
    assert bool((hits == -7).all())                                   # a refused call wrote nothing
    assert raw() == 0
    assert np.array_equal(idx.cpu().numpy(), c["nearest"][0])


# ---------------------------------------------------------------------------------------------- 7. the report
@pytest.mark.parametrize("space", ["latent", "pixel", "both"])
def test_report_on_a_stub_model(tmp_path, capsys, space):
    import evae_oracle as orc
    import smoke_case
    import golden_inputs as gi
    from evae import sample_quality as sq
    from utils.knn_on_latent import _posterior_means, extract_full_data
    from utils.sample_quality_on_latent import report_sample_quality
    B, k = 32, 3
    args = smoke_case.vae_args(number_components=20, training_set_size=200, batch_size=B)
    args.sample_quality_space, args.sample_quality_k, args.sample_quality_save = space, k, 1
    model, _ = smoke_case.build_model(torch, np, orc, args)
    model.eval()

    def loader(seed, n):
        data = torch.from_numpy(gi.binary_images(seed, n))
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, torch.arange(n) % 10), batch_size=B, shuffle=False)

    train, test = loader(91, 200), loader(92, 100)                    # 192 and 96 rows in full batches
    out = str(tmp_path / "quality")
    torch.manual_seed(5)
    report = report_sample_quality(train, test, model, out, args)
    assert "sample quality of 96 draws, k = 3" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == ["sample_quality.json", "sample_quality_nearest.npy"]
    with open(os.path.join(out, "sample_quality.json")) as f:
        saved = json.load(f)
    spaces = ["latent", "pixel"] if space == "both" else [space]
    assert saved == report and sorted(saved) == spaces

    # the same draws again, scored directly (a DataLoader's iterator takes a seed from the host generator: the report's order)
    torch.manual_seed(5)
    with torch.no_grad():
        train_x, test_x = [extract_full_data(ld)[0].to(args.device) for ld in (train, test)]
        fake_x = torch.cat([model.generate_x(N=B, dataset=train.dataset).reshape(B, -1) for _ in range(3)], dim=0)
        sets = dict(latent=[_posterior_means(model, x, B) for x in (train_x, test_x, fake_x)],
                    pixel=[x[:(len(x) // B) * B].reshape(-1, 784).float() for x in (train_x, test_x, fake_x)])
    for s in spaces:
        tr, te, fk = sets[s]
        assert tr.shape == (192, 40 if s == "latent" else 784) and te.shape[0] == fk.shape[0] == 96
        assert sorted(saved[s]) == sorted(["precision", "recall", "density", "coverage", "authenticity", "nearest_distance_median",
                                           "nearest_k", "n_real", "n_fake", "n_train"])
        want = dict(sq.sample_quality(te, fk, nearest_k=k, train=tr), n_train=192)
        assert saved[s] == want and (saved[s]["n_real"], saved[s]["n_fake"], saved[s]["nearest_k"]) == (96, 96, k)
    nearest = np.load(os.path.join(out, "sample_quality_nearest.npy"))
    assert nearest.dtype == np.int32 and nearest.shape == (96,) and nearest.min() >= 0 and nearest.max() < 192
    assert np.array_equal(nearest, sq.nearest_real(sets[spaces[0]][0], sets[spaces[0]][2])[0].cpu().numpy())

    # fewer draws, nothing saved
    args.sample_quality_samples, args.sample_quality_save = 70, 0
    small = report_sample_quality(train, test, model, str(tmp_path / "small"), args)
    assert all(v["n_fake"] == 64 for v in small.values()) and os.listdir(str(tmp_path / "small")) == ["sample_quality.json"]
