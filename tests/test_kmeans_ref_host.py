"""CPU-only: tests/kmeans_ref.py -- the float64 restatement the k-means kernels are held to (tests/test_gpu_kmeans.py) -- against
scikit-learn where it is installed, the preconditions of the shared case table that the GPU tests lean on, and the refusals of
evae.cluster.KMeans that are known from shapes alone.

The preconditions are conditions, not measurements: a GPU test may compare labels, picks and iteration counts EXACTLY only because
the reference itself stays clear of ties.  fp64 rounding over at most 3 000 terms is about 1e-12 relative; the floors -- 1e-9 for
an argmin and for a seeding pick, 1e-6 for a stop on the shift -- leave a thousandfold."""
import numpy as np
import pytest

import kmeans_ref as ref

ROWS = pytest.mark.parametrize("row", ref.CASES, ids=lambda r: "n%d_d%d_K%d" % r[:3])


@ROWS
def test_case_table_stays_clear_of_ties(row):
    n, d, K, _ = row
    s = ref.solved(*row)
    fit = s["fit"]
    counts = np.bincount(fit["labels"], minlength=K)
    print("n=%d d=%d K=%d: %d iterations, argmin margin %.3g, seed margin %.3g, smallest cluster %d"
          % (n, d, K, fit["n_iter"], fit["argmin_margin"], s["seed_margin"], counts.min()))
    assert len(set(s["idx"].tolist())) == K                  # K distinct seeds
    assert counts.min() >= 1 and fit["relocations"] == 0     # no empty cluster on the way or at the end
    assert fit["argmin_margin"] >= 1e-9
    assert s["seed_margin"] >= 1e-9
    assert 1 <= fit["n_iter"] < 300


def test_tol_and_relocation_cases_stay_clear_of_ties():
    full, stopped = ref.solved(*ref.TOL_CASE)["fit"], ref.solved_with_tol()
    print("tol case: stops at %d of %d iterations, shift margin %.3g, argmin margin %.3g"
          % (stopped["n_iter"], full["n_iter"], stopped["shift_margin"], stopped["argmin_margin"]))
    assert stopped["n_iter"] < full["n_iter"]                # the shift stops it, not the labels
    assert stopped["shift_margin"] >= 1e-6 and stopped["argmin_margin"] >= 1e-9
    for how_many in (1, 2, 3):
        _, fit = ref.solved_with_relocations(how_many)
        print("%d far centres: %d relocations, %d iterations, argmin margin %.3g"
              % (how_many, fit["relocations"], fit["n_iter"], fit["argmin_margin"]))
        assert fit["relocations"] == how_many and fit["argmin_margin"] >= 1e-9


def test_table_straddles_the_chunk_and_the_tile():
    ns, ks = {r[0] for r in ref.CASES}, {r[2] for r in ref.CASES}
    assert {ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1, 2 * ref.CHUNK + 1} <= ns
    assert {1, ref.TILE - 1, ref.TILE, ref.TILE + 1, 1024} <= ks


# ---------------------------------------------------------------------------------------------- against scikit-learn
def sklearn_lloyd(X, C0):
    cluster = pytest.importorskip("sklearn.cluster")
    km = cluster.KMeans(n_clusters=len(C0), init=np.array(C0), n_init=1, tol=0, algorithm='lloyd', max_iter=300)
    return km.fit(np.asarray(X, np.float64))


@pytest.mark.parametrize("row", ref.CASES[:7], ids=lambda r: "n%d_d%d_K%d" % r[:3])
def test_lloyd_matches_scikit_learn(row):
    s = ref.solved(*row)
    km, fit = sklearn_lloyd(s["X"], s["C0"]), s["fit"]
    e_inertia = abs(km.inertia_ - fit["inertia"]) / max(fit["inertia"], 1e-300)
    print("n=%d d=%d K=%d: n_iter %d / %d, inertia apart by %.3g" % (row[:3] + (fit["n_iter"], km.n_iter_, e_inertia)))
    assert np.array_equal(km.labels_, fit["labels"])
    assert km.n_iter_ == fit["n_iter"]
    assert e_inertia <= 1e-12


@pytest.mark.parametrize("how_many", [1, 2, 3])
def test_relocations_match_scikit_learn(how_many):
    X = ref.solved(*ref.RELOCATION_CASE)["X"]
    C0, fit = ref.solved_with_relocations(how_many)
    km = sklearn_lloyd(X, C0)
    assert np.array_equal(km.labels_, fit["labels"]) and km.n_iter_ == fit["n_iter"]
    assert abs(km.inertia_ - fit["inertia"]) <= 1e-12 * fit["inertia"]


def label_pairs():
    rs = np.random.RandomState(7)
    y = np.arange(600) % 10
    noisy = np.where(rs.random_sample(600) < 0.3, rs.randint(0, 7, 600), y % 7)
    return [("noisy", y, noisy), ("equal", y, y), ("permuted", y, (y + 3) % 10), ("one cluster", y, np.zeros(600, int)),
            ("one and one", np.zeros(50, int), np.zeros(50, int)), ("independent", y, rs.randint(0, 4, 600)),
            ("fit", ref.solved(*ref.CASES[2])["y"], ref.solved(*ref.CASES[2])["fit"]["labels"])]


@pytest.mark.parametrize("name,a,b", label_pairs(), ids=[p[0] for p in label_pairs()])
def test_scores_match_scikit_learn(name, a, b):
    metrics = pytest.importorskip("sklearn.metrics")
    table = ref.contingency(a, a.max() + 1, b, b.max() + 1)
    got = ref.scores(table)
    assert np.array_equal(table, metrics.cluster.contingency_matrix(a, b))
    want = dict(nmi=metrics.normalized_mutual_info_score(a, b), ari=metrics.adjusted_rand_score(a, b),
                mutual_info=metrics.mutual_info_score(a, b),
                purity=metrics.cluster.contingency_matrix(a, b).max(axis=0).sum() / len(a))
    for key, value in want.items():
        print("%s %s: %.17g against %.17g" % (name, key, got[key], value))
        assert abs(got[key] - value) <= 1e-12, key


@pytest.mark.parametrize("row", [ref.CASES[1], ref.CASES[2], ref.CASES[6]], ids=lambda r: "n%d_d%d_K%d" % r[:3])
def test_silhouette_matches_scikit_learn(row):
    metrics = pytest.importorskip("sklearn.metrics")
    s = ref.solved(*row)
    labels = s["fit"]["labels"].copy()
    labels[0] = row[2]                                        # a singleton cluster
    got = ref.silhouette_samples(s["X"], labels)
    want = metrics.silhouette_samples(np.asarray(s["X"], np.float64), labels)
    print("n=%d d=%d K=%d: silhouette apart by %.3g" % (row[:3] + (np.abs(got - want).max(),)))
    assert np.abs(got - want).max() <= 1e-10 and got[0] == 0.0


def test_seed_by_hand():
    X = np.array([[0.0], [1.0], [3.0], [3.0]], np.float32)
    idx, C, margin = ref.seed(X, 3, np.array([0.3, 0.5, 0.99]))
    # first floor(0.3 * 4) = 1; d2min = (1, 0, 4, 4), target 4.5 -> running (1, 1, 5, 9): row 2; then d2min = (1, 0, 0, 0): row 0
    assert idx.tolist() == [1, 2, 0] and np.array_equal(C[:, 0], [1.0, 3.0, 0.0])
    idx, _, _ = ref.seed(np.ones((5, 2), np.float32), 4, np.array([0.5, 0.1, 0.9, 0.5]))
    assert idx.tolist() == [2, 0, 1, 3]                      # total == 0: the lowest index not chosen yet


# ---------------------------------------------------------------------------------------------- refusals known from shapes
def test_kmeans_refuses_from_the_shape_alone():
    from evae import _lib, ops
    from evae.cluster import KMeans
    with _lib.count_calls("evae_kmeans_assign") as calls, _lib.count_calls("evae_kmeans_step") as steps:
        with pytest.raises(ValueError):
            KMeans(3).fit(np.zeros((2, 2), np.float32))                              # K > N
        with pytest.raises(ValueError):
            KMeans(1).fit(np.zeros((1, 2), np.float32))                              # N < 2
        with pytest.raises(ValueError):
            KMeans(2).fit(np.zeros((8, ops.kmeans_max_features() + 1), np.float32))
        with pytest.raises(ValueError):
            KMeans(ops.kmeans_max_clusters() + 1).fit(np.zeros((2000, 2), np.float32))
        with pytest.raises(ValueError):
            KMeans(2, init=np.zeros((2, 3))).fit(np.zeros((8, 2), np.float32))       # init of another width
        with pytest.raises(ValueError):
            KMeans(2).fit(np.zeros(8, np.float32))                                   # not [N x d]
    assert not calls and not steps
    for bad in (dict(n_clusters=0), dict(init='kmeans'), dict(init=np.zeros((3, 2)), n_clusters=2), dict(n_init=0),
                dict(n_init='many'), dict(max_iter=0), dict(check_every=0), dict(tol=-1.0), dict(init=np.zeros(4))):
        with pytest.raises(ValueError):
            KMeans(**bad)
    assert (ops.kmeans_max_clusters(), ops.kmeans_max_features(), ops.kmeans_max_points()) == (1024, 256, 2 ** 20)
    assert (ops.kmeans_chunk_rows(), ops.kmeans_centre_tile()) == (ref.CHUNK, ref.TILE)
