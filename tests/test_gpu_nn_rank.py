"""GPU: ranks of chosen neighbours (csrc/evae_nn_rank.hip), evae.ops.nn_rank, evae.tsne.trustworthiness / continuity /
embedding_quality and the quality report of utils.tsne_on_latent, against the numpy restatement tests/nn_rank_ref.py (held to
scikit-learn by tests/test_nn_rank_ref_host.py) on the oracle's distances.

Everything here is an integer, or integers through one float64 expression, so every comparison is for equality.  The yardstick is
the restatement, never the kernel."""
import json
import os

import numpy as np
import pytest
import torch

import nn_rank_ref as rr
from tsne_ref import blobs

pytestmark = pytest.mark.gpu

ROW_TILE = 1024      # distances one pass of a counting workgroup takes: 256 threads x one 16-byte load (csrc/evae_nn_rank.hip)
CASES = [(97, 40, 5), (97, 40, 16), (300, 3, 91), (1025, 40, 12), (600, 8, 256), (300, 2, 12), (ROW_TILE - 1, 8, 12), (ROW_TILE, 8, 12),
         (ROW_TILE + 1, 3, 12)]


def points(n, zd):
    X, labels = blobs(n, zd, 4, seed=3000 + n)
    if n == 97:
        X[5] += 40.0                        # one far outlier row
        X[20:28] = X[20]                    # eight identical rows
    return X, labels


def other_space(n):
    """a second space that knows nothing of the first: its neighbours have ranks far above k there"""
    Y = np.random.RandomState(7000 + n).randn(n, 2).astype(np.float32)
    Y[11] = Y[40]                           # two coincident points
    return Y


def oracle_distances(X):
    import evae_oracle as orc
    return orc.pairdist_direct_f64(X, X)


def oracle_neighbours(X, k):
    import evae_oracle as orc
    D = oracle_distances(X)
    D[np.arange(len(X)), np.arange(len(X))] = np.inf
    return orc.topk_smallest(D, k)[1]


_cases = {}


def case(n, zd, k):
    """inputs and the restatement of a case, computed once, shared and left alone"""
    key = (n, zd, k)
    if key not in _cases:
        X, labels = points(n, zd)
        D = oracle_distances(X)
        nbr = oracle_neighbours(other_space(n), k)
        _cases[key] = dict(X=X, labels=labels, D=D, nbr=nbr, rank=rr.ranks(D, nbr))
    return _cases[key]


@pytest.fixture(scope="module")
def ops():
    from evae import ops
    return ops


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def same(got_rank, got_sums, want_rank, k):
    assert got_rank.dtype == torch.int32 and got_sums.dtype == torch.int64
    assert got_rank.shape == want_rank.shape and got_sums.shape == (len(want_rank), 2)
    assert np.array_equal(got_rank.cpu().numpy(), want_rank)
    assert np.array_equal(got_sums.cpu().numpy(), rr.row_sums(want_rank, k))


# ---------------------------------------------------------------------------------------------- 1. ranks and row sums
@pytest.mark.parametrize("n,zd,k", CASES)
def test_ranks_of_another_spaces_neighbours(ops, n, zd, k):
    c = case(n, zd, k)
    rank, sums = ops.nn_rank(dev(c["X"]), dev(c["nbr"], torch.int32))
    same(rank, sums, c["rank"], k)
    assert c["rank"].min() >= 1 and c["rank"].max() > n // 2 and np.median(c["rank"]) > k       # far above k: both sums are exercised
    if n == 97 and k == 16:
        # ties at 0 inside the eight identical rows: from row 22 its seven twins hold ranks 1 .. 7 in index order
        twins = [j for j in range(20, 28) if j != 22]
        r22 = ops.nn_rank(dev(c["X"]), dev(np.tile(np.array(twins + [5] * (k - 7))[None, :], (n, 1)), torch.int32))[0][22].cpu().numpy()
        assert r22[:7].tolist() == [1, 2, 3, 4, 5, 6, 7] and np.all(r22[7:] == n - 1)     # the outlier is the farthest; named k - 7 times


@pytest.mark.parametrize("n,zd,k", CASES)
def test_ranks_of_the_own_neighbours_count_up(ops, n, zd, k):
    """the neighbour search's own m-th neighbour has rank m + 1, ties included: from the oracle's neighbours and from the kernel's"""
    X = points(n, zd)[0]
    want = np.tile(np.arange(1, k + 1), (n, 1))
    rank, sums = ops.nn_rank(dev(X), dev(oracle_neighbours(X, k), torch.int32))
    same(rank, sums, want, k)
    assert bool((sums[:, 0] == 0).all()) and bool((sums[:, 1] == k).all())
    rank2, sums2 = ops.nn_rank(dev(X), ops.tsne_knn(dev(X), k)[0])
    assert torch.equal(rank, rank2) and torch.equal(sums, sums2)


# ---------------------------------------------------------------------------------------------- 2. strips
@pytest.mark.parametrize("strip", [64, 77])      # 77 rows x 3 floats: strips whose queries start off a 16-byte boundary
def test_the_result_does_not_depend_on_the_strip(ops, strip):
    c = case(300, 3, 91)
    X, nbr = dev(c["X"]), dev(c["nbr"], torch.int32)
    rank0, sums0 = ops.nn_rank(X, nbr)
    rank, sums = ops.nn_rank(X, nbr, strip_rows=strip)              # 300 rows: full strips and a ragged last one
    assert torch.equal(rank, rank0) and torch.equal(sums, sums0)
    same(rank, sums, c["rank"], 91)


# ---------------------------------------------------------------------------------------------- 3. guards
def test_entries_that_name_the_point_itself_or_no_point(ops):
    """such an entry gets rank 0 and is never dereferenced; its row's other entries and sums are those of the row without it"""
    n, k = 97, 16
    c = case(n, 40, k)
    nbr = c["nbr"].copy()
    nbr[3, 0], nbr[96, 2] = 3, 96                                   # the point itself
    nbr[10, 5], nbr[50, 15], nbr[51, 0] = -1, n, n + 1000           # no point
    nbr[60, 7], nbr[61, 8] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    nbr[70, :] = -1                                                 # a row with nothing to rank
    nbr[22, 1] = 22                                                 # one of the identical rows: its twins stay, itself goes
    touched = np.zeros(nbr.shape, bool)
    touched[[3, 96, 10, 50, 51, 60, 61, 22], [0, 2, 5, 15, 0, 7, 8, 1]] = True
    touched[70] = True
    want = rr.ranks(c["D"], nbr)
    assert np.all(want[touched] == 0) and np.array_equal(want[~touched], c["rank"][~touched])
    rank, sums = ops.nn_rank(dev(c["X"]), dev(nbr, torch.int32))
    same(rank, sums, want, k)
    assert sums[70].tolist() == [0, 0]
    kept = rr.row_sums(np.where(touched, 0, c["rank"]), k)
    assert np.array_equal(sums.cpu().numpy(), kept)


def test_interface_errors(ops):
    from evae import launch
    from evae._lib import EvaeError
    c = case(600, 8, 256)
    X, nbr = dev(c["X"]), dev(c["nbr"], torch.int32)
    with pytest.raises(EvaeError):
        ops.nn_rank(X, nbr.long())
    with pytest.raises(EvaeError):
        ops.nn_rank(X, nbr[:, ::2])                                 # not contiguous
    with pytest.raises(EvaeError):
        ops.nn_rank(X, nbr[:-1])
    with pytest.raises(EvaeError):
        ops.nn_rank(X, torch.cat((nbr, nbr[:, :1]), dim=1))         # k = 257
    with pytest.raises(EvaeError):
        ops.nn_rank(X[:200], nbr[:200, :200].contiguous())          # a point has N - 1 neighbours
    with pytest.raises(EvaeError):
        ops.nn_rank(X, nbr, strip_rows=-1)
    with pytest.raises(EvaeError):
        ops.nn_rank(X.cpu(), nbr.cpu())
    wide = torch.zeros((600, 257), dtype=torch.int32, device="cuda")
    rank, sums = torch.empty_like(wide), torch.empty((600, 2), dtype=torch.int64, device="cuda")
    ws = torch.empty(600 * 600 * 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(EvaeError, match="k=257"):                   # the entry point's own check, under the operator's
        launch.Launcher(X.device).nn_rank(X, 600, 8, wide, 257, 0, rank, sums, ws)
    with pytest.raises(EvaeError, match="workspace"):
        launch.Launcher(X.device).nn_rank(X, 600, 8, nbr, 256, 0, rank[:, :256].contiguous(), sums, ws[:-4])


# ---------------------------------------------------------------------------------------------- 4. scores
def reference_quality(X, Y, k, labels):
    return rr.embedding_quality(oracle_distances(np.asarray(X, np.float32)), oracle_distances(np.asarray(Y, np.float32)), k, labels)


@pytest.mark.parametrize("n,zd,k", [(97, 40, 5), (1025, 40, 12)])
def test_scores_are_the_restatements_floats(n, zd, k):
    from evae import tsne
    X, labels = points(n, zd)
    Y = (X[:, :2] + 0.5 * other_space(n)).astype(np.float32)        # an embedding that keeps something of X
    want = reference_quality(X, Y, k, labels)
    Xd, Yd = dev(X), dev(Y)
    got = tsne.embedding_quality(Xd, Yd, n_neighbors=k, labels=torch.from_numpy(labels))
    print("device %s\nreference %s" % (got, want))
    assert got == want and all(type(got[key]) is float for key in ("trustworthiness", "continuity", "neighbourhood_preservation",
                                                                   "label_accuracy"))
    assert type(got["n_neighbors"]) is int and type(got["n_samples"]) is int
    assert 0.5 < want["trustworthiness"] < 1.0 and 0.5 < want["continuity"] < 1.0      # neither perfect nor noise: the sums count
    t, c = tsne.trustworthiness(Xd, Yd, n_neighbors=k), tsne.continuity(Xd, Yd, n_neighbors=k)
    assert type(t) is float and t == want["trustworthiness"] and type(c) is float and c == want["continuity"]
    assert tsne.trustworthiness(X, Y, k) == t and tsne.continuity(X, Yd, k) == c      # arrays go to the device as fit_transform's do
    plain = tsne.embedding_quality(Xd, Yd, k)
    assert "label_accuracy" not in plain and plain == {key: v for key, v in want.items() if key != "label_accuracy"}


def test_scores_refuse_half_the_points_as_neighbours():
    from evae import tsne
    X, Y = dev(points(97, 40)[0]), dev(other_space(97))
    for fn in (tsne.trustworthiness, tsne.continuity, tsne.embedding_quality):
        with pytest.raises(ValueError, match="n_samples / 2"):
            fn(X, Y, n_neighbors=49)                                # 49 >= 97 / 2, as scikit-learn refuses
        with pytest.raises(ValueError):
            fn(X, Y[:-1], n_neighbors=5)
    assert 0.0 < tsne.trustworthiness(X, Y, n_neighbors=48) < 1.0
    with pytest.raises(ValueError):
        tsne.embedding_quality(X, Y, 5, labels=np.zeros(96, np.int64))


# ---------------------------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("method", ["exact", "neighbours"])
def test_end_to_end(method):
    """300 points in 4 blobs: the scores of a real embedding are the restatement's on the downloaded embedding, and a real
    embedding is more trustworthy than the same points handed to the wrong rows"""
    from evae import tsne
    n, k = 300, 5
    X, labels = blobs(n, 40, 4, seed=21)
    Xd = dev(X)
    Y = tsne.TSNE(n_iter=250, exaggerated_iters=60, random_state=0, method=method).fit_transform(Xd)
    got = tsne.embedding_quality(Xd, Y, k, labels=labels)
    want = reference_quality(X, Y.cpu().numpy(), k, labels)
    print("%s: %s" % (method, got))
    assert got == want
    shuffled = Y[torch.from_numpy(np.random.RandomState(4).permutation(n)).cuda()].contiguous()
    t_shuffled = tsne.trustworthiness(Xd, shuffled, k)
    print("rows permuted: trustworthiness %.4f" % t_shuffled)
    assert got["trustworthiness"] > t_shuffled
    assert t_shuffled == rr.trustworthiness(oracle_distances(X), oracle_distances(shuffled.cpu().numpy()), k)


# ---------------------------------------------------------------------------------------------- 6. the report
def test_report_tsne_on_latent_writes_the_quality(tmp_path):
    import evae_oracle as orc
    import smoke_case
    from evae import _lib, tsne
    from utils.knn_on_latent import _posterior_means
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

    # without the attribute, and with it at 0: the files of before, and no ranking launch
    plain, zero = str(tmp_path / "plain"), str(tmp_path / "zero")
    with _lib.count_calls("evae_nn_rank") as calls:
        report_tsne_on_latent(loader, model, plain, args)
        args.tsne_quality_neighbours = 0
        report_tsne_on_latent(loader, model, zero, args)
    assert not calls
    assert sorted(os.listdir(plain)) == sorted(os.listdir(zero)) == ["tsne.npy", "tsne_labels.npy"]
    with torch.no_grad():
        z = _posterior_means(model, data.to(args.device), B)
    direct = tsne.TSNE(perplexity=5.0, n_iter=30, random_state=3, method='neighbours').fit_transform(z)      # no report at all
    saved = np.load(os.path.join(plain, "tsne.npy"))
    assert np.array_equal(saved.view(np.uint32), direct.cpu().numpy().view(np.uint32))
    assert np.array_equal(saved.view(np.uint32), np.load(os.path.join(zero, "tsne.npy")).view(np.uint32))

    # with it: one more file, the others bit-equal
    out = str(tmp_path / "quality")
    args.tsne_quality_neighbours = 5
    with _lib.count_calls("evae_nn_rank") as calls:
        Y = report_tsne_on_latent(loader, model, out, args)
    assert calls.get("evae_nn_rank") == 2                           # one pass per direction
    assert sorted(os.listdir(out)) == ["tsne.npy", "tsne_labels.npy", "tsne_quality.json"]
    assert np.array_equal(np.load(os.path.join(out, "tsne.npy")).view(np.uint32), saved.view(np.uint32))
    assert np.array_equal(Y.cpu().numpy(), saved)
    saved_labels = np.load(os.path.join(out, "tsne_labels.npy"))
    with open(os.path.join(out, "tsne_quality.json")) as f:
        quality = json.load(f)
    want = tsne.embedding_quality(z, saved, n_neighbors=5, labels=saved_labels)
    assert quality.pop("method") == 'neighbours' and np.isfinite(quality.pop("kl_divergence"))
    assert quality == want and quality["n_samples"] == 64 and "label_accuracy" in quality
    assert want == reference_quality(z.cpu().numpy(), saved, 5, saved_labels)
