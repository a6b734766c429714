"""GPU: the fp64 k-means kernels (csrc/evae_kmeans.hip), evae.ops.kmeans_* / cluster_* / silhouette_*, evae.cluster and the
latent-space report, against the numpy float64 restatement tests/kmeans_ref.py (held to scikit-learn, and its case table to its
margins, by tests/test_kmeans_ref_host.py).

The yardstick is always the restatement, never the code under test.  Decisions -- labels, seeding picks, iteration counts -- are
compared EXACTLY: the restatement's own margins (>= 1e-9 for an argmin or a pick, >= 1e-6 for a stop on the shift; asserted on the
host for the table, here for inputs made here) are a thousandfold above fp64 rounding over the 3 000 terms at most that any sum
here has.  Every bound on a value comes from the arithmetic, with eps = 2^-52:

* d2: d differences, squares and additions in fp64 on both sides (one fused, one not): 4 d eps relative.
* cluster sums and centres: n_c fp64 additions per column on the device; 4 n_c eps max|x| (the restatement sums pairwise, so the
  allowance is the device's).  A centre is its sum over n_c: the same bound.
* inertia: N additions of values each good to 4 d eps; 4 N eps relative (N >= d in every case here, d eps <= N eps otherwise).
* entropies and MI: a term (v / N) log r carries three roundings, one of r and the logarithm's: <= 4 eps (1 + log N) summed over
  the table on each side; the device adds ceil(Ka Kb / 1024) terms per thread and ten levels of a tree, each at eps x the sum of
  |terms| <= log N; the restatement adds exactly (fsum).  Allowed: (ceil(Ka Kb / 1024) + 18) eps (1 + log N).  NMI = MI / mean H
  inherits (allowance of MI + allowance of H) / mean H, plus 4 eps for the closing operations.
* ARI: exact integers until 2 (tp tn - fn fp) / ((tp + fn)(fn + tn) + (tp + fp)(fp + tn)) in fp64; the denominator is at least
  tp tn + 2 fn fp, so the rounded products cost <= 9 eps absolute: 16 eps.  Purity is an integer over N: bit for bit.
* silhouette: the device takes sqrt of an fp32-rounded d2 (2^-25 relative on every distance, so on a and on b); |s| <= 1 and
  ds <= da / max + db / max: 2^-22 absolute is the issue's bound, four such roundings.

Every test prints the figures it asserts on; DESIGN 3.7d records the largest."""
import json
import math
import os

import numpy as np
import pytest
import torch

import kmeans_ref as ref
from tsne_ref import blobs

pytestmark = pytest.mark.gpu

EPS = ref.EPS
ROW_IDS = ["n%d_d%d_K%d" % r[:3] for r in ref.CASES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view({torch.float64: np.uint64, torch.float32: np.uint32, torch.int32: np.uint32, torch.int64: np.uint64}[t.dtype])


def test_constants_are_the_reference_s():
    from evae import ops
    assert (ops.kmeans_chunk_rows(), ops.kmeans_centre_tile()) == (ref.CHUNK, ref.TILE)
    assert (ops.kmeans_max_clusters(), ops.kmeans_max_features(), ops.kmeans_max_points()) == (1024, 256, 2 ** 20)


# ---------------------------------------------------------------------------------------------- 1. assign
def check_assign(name, X, C, need_margin=True):
    from evae import ops
    labels, d2 = ops.kmeans_assign(dev(X), dev(C))
    assert labels.dtype == torch.int32 and d2.dtype == torch.float64 and tuple(labels.shape) == tuple(d2.shape) == (len(X),)
    rl, rd, margin = ref.assign(X, C)
    if need_margin:
        assert margin >= 1e-9, (name, margin)               # the precondition of the exact comparison
    scale = np.where(rd > 0, rd, 1.0)
    err = (np.abs(host(d2) - rd) / scale).max()
    print("assign %s: margin %.3g, d2 at %.3g relative (allowed %.3g)" % (name, margin, err, 4 * X.shape[1] * EPS))
    assert np.array_equal(host(labels), rl)
    assert err <= 4 * X.shape[1] * EPS
    again = ops.kmeans_assign(dev(X), dev(C))
    assert np.array_equal(bits(labels), bits(again[0])) and np.array_equal(bits(d2), bits(again[1]))
    return err


@pytest.mark.parametrize("row", ref.CASES, ids=ROW_IDS)
def test_assign_on_the_table(row):
    s = ref.solved(*row)
    check_assign("seeds", s["X"], s["C0"])
    check_assign("final centres", s["X"], s["fit"]["centres"])


def test_assign_over_widths_and_tile_edges():
    """d in (1, 2, 3, 63, 64, 65, 255, 256) x K in (1, tile - 1, tile, tile + 1) at N = 130: three blocks of rows, the last partial"""
    worst = 0.0
    for d in (1, 2, 3, 63, 64, 65, 255, 256):
        X = blobs(130, d, 4, seed=300 + d)[0]
        rs = np.random.RandomState(d)
        for K in (1, ref.TILE - 1, ref.TILE, ref.TILE + 1):
            C = X[rs.permutation(130)[:K]].astype(np.float64) + 0.25 * rs.randn(K, d)
            worst = max(worst, check_assign("d=%d K=%d" % (d, K), X, C) / (4 * d * EPS))
    print("assign: worst d2 at %.3g of its allowance" % worst)


def test_assign_ties_go_to_the_lowest_centre():
    from evae import ops
    X = blobs(200, 5, 3, seed=9)[0]
    C = X[[3, 50, 3, 120, 50]].astype(np.float64)           # centres 0 == 2 and 1 == 4, bit for bit
    labels = host(ops.kmeans_assign(dev(X), dev(C))[0])
    rl = ref.assign(X, C)[0]
    assert np.array_equal(labels, rl) and not np.isin(labels, (2, 4)).any()
    far = np.tile(C[:1], (ref.TILE + 3, 1))                  # every centre the same, across a tile boundary
    assert not host(ops.kmeans_assign(dev(X), dev(far))[0]).any()


def test_transform_is_the_square_root_of_the_same_sums():
    from evae import ops
    s = ref.solved(*ref.CASES[2])
    got = host(ops.kmeans_transform(dev(s["X"]), dev(s["C0"])))
    want = np.sqrt(ref.sq_distances(s["X"], s["C0"]))
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 2.0 ** -23 * want.max()


# ---------------------------------------------------------------------------------------------- 2. update
def check_update(name, X, labels, K):
    from evae import ops
    order, start, sums = ops.kmeans_update(dev(X), dev(labels.astype(np.int32)), K)
    assert order.dtype == start.dtype == torch.int32 and sums.dtype == torch.float64
    assert np.array_equal(host(order), np.argsort(labels, kind="stable"))
    assert np.array_equal(host(start), np.concatenate(([0], np.cumsum(np.bincount(labels, minlength=K)))))
    rsums, counts = ref.cluster_sums(X, labels, K)
    allowed = 4 * np.maximum(counts, 1)[:, None] * EPS * np.abs(X).max()
    ratio = (np.abs(host(sums) - rsums) / allowed).max()
    print("update %s: N=%d d=%d K=%d, %d empty, sums at %.3g of 4 n_c eps max|x|" % (name, len(X), X.shape[1], K, (counts == 0).sum(), ratio))
    assert ratio <= 1.0
    assert np.array_equal(host(sums)[counts == 0], np.zeros(((counts == 0).sum(), X.shape[1])))
    again = ops.kmeans_update(dev(X), dev(labels.astype(np.int32)), K)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((order, start, sums), again))
    return ratio


@pytest.mark.parametrize("row", [ref.CASES[i] for i in (0, 1, 3, 4, 5, 7, 11, 13, 15, 16, 17)],
                         ids=[ROW_IDS[i] for i in (0, 1, 3, 4, 5, 7, 11, 13, 15, 16, 17)])
def test_update_on_the_table(row):
    s = ref.solved(*row)
    check_update("final labels", s["X"], s["fit"]["labels"], row[2])


def test_update_with_empty_clusters_and_with_one_cluster():
    X = ref.solved(*ref.CASES[2])["X"]
    rs = np.random.RandomState(3)
    labels = rs.choice([1, 4, 5, 40, 63], size=len(X))      # 59 of 64 clusters empty, the first and the last among them
    check_update("empty clusters", X, labels, 64)
    check_update("one cluster of ten", X, np.full(len(X), 7), 10)
    check_update("K = 1", X, np.zeros(len(X), int), 1)
    check_update("sorted already", X, np.sort(rs.randint(0, 1024, len(X))), 1024)


# ---------------------------------------------------------------------------------------------- 3. seed
@pytest.mark.parametrize("row", ref.CASES, ids=ROW_IDS)
def test_seed_on_the_table(row):
    from evae import ops
    s = ref.solved(*row)
    idx, centres = ops.kmeans_seed(dev(s["X"]), row[2], dev(s["u"]))
    assert idx.dtype == torch.int32 and centres.dtype == torch.float64
    print("seed n=%d d=%d K=%d: the reference's margin %.3g" % (row[:3] + (s["seed_margin"],)))
    assert np.array_equal(host(idx), s["idx"])
    assert np.array_equal(host(centres), s["X"][s["idx"]].astype(np.float64))
    again = ops.kmeans_seed(dev(s["X"]), row[2], dev(s["u"]))
    assert np.array_equal(bits(idx), bits(again[0]))


def test_seed_without_distinct_points():
    """all rows equal: the total is 0 from the second pick on, which is then the lowest index not chosen yet; and three distinct
    values for five centres: D^2 sampling while it can, the rule after"""
    from evae import ops
    u = np.array([0.5, 0.1, 0.9, 0.5, 0.7])
    X = np.full((ref.CHUNK + 88, 3), 1.5, np.float32)
    idx = host(ops.kmeans_seed(dev(X), 5, dev(u))[0])
    assert idx.tolist() == [300, 0, 1, 2, 3] == ref.seed(X, 5, u)[0].tolist()
    X = np.repeat(np.array([[0.0], [1.0], [4.0]], np.float32), 200, axis=0)
    u = np.array([0.5, 0.3713, 0.9327, 0.5, 0.7])           # the running sums are integers here: targets between them
    want, _, margin = ref.seed(X, 5, u)
    assert margin >= 1e-9
    assert host(ops.kmeans_seed(dev(X), 5, dev(u))[0]).tolist() == want.tolist()


# ---------------------------------------------------------------------------------------------- 4. fit
def check_fit(name, km, X, want):
    n_c = np.maximum(np.bincount(want["labels"], minlength=km.n_clusters), 1)
    e_centres = (np.abs(host(km.cluster_centers_) - want["centres"]) / (4 * n_c[:, None] * EPS * np.abs(X).max())).max()
    e_inertia = abs(km.inertia_ - want["inertia"]) / max(want["inertia"], 1e-300)
    print("fit %s: n_iter %d (reference %d), relocations %d, centres at %.3g of 4 n_c eps max|x|, inertia %.3g relative (allowed %.3g)"
          % (name, km.n_iter_, want["n_iter"], km.n_relocations_, e_centres, e_inertia, 4 * len(X) * EPS))
    assert km.labels_.dtype == torch.int32 and km.cluster_centers_.dtype == torch.float64 and km.labels_.is_cuda
    assert np.array_equal(host(km.labels_), want["labels"])
    assert km.n_iter_ == want["n_iter"] and km.n_relocations_ == want["relocations"]
    assert e_centres <= 1.0
    assert e_inertia <= 4 * len(X) * EPS
    return e_centres, e_inertia / (4 * len(X) * EPS)


@pytest.mark.parametrize("check_every", [1, 8])
@pytest.mark.parametrize("row", ref.CASES, ids=ROW_IDS)
def test_fit_from_a_given_init(row, check_every):
    from evae.cluster import KMeans
    s = ref.solved(*row)
    km = KMeans(row[2], init=s["C0"], tol=0, check_every=check_every).fit(dev(s["X"]))
    check_fit("n=%d d=%d K=%d" % row[:3], km, s["X"], s["fit"])
    assert np.array_equal(host(km.predict(dev(s["X"]))), host(km.labels_))


def uniforms(random_state, K, runs=1):
    g = torch.Generator()
    g.manual_seed(random_state)
    return [torch.rand(K, dtype=torch.float64, generator=g).numpy() for _ in range(runs)]


def test_fit_from_the_seeds():
    """init='k-means++': the class draws its uniforms from a CPU torch.Generator, so the restatement can be given the same"""
    from evae.cluster import KMeans
    n, d, K, seed_ = ref.CASES[8]
    X = ref.solved(n, d, K, seed_)["X"]
    idx, C0, seed_margin = ref.seed(X, K, uniforms(11, K)[0])
    want = ref.lloyd(X, C0)
    assert seed_margin >= 1e-9 and want["argmin_margin"] >= 1e-9          # this input's own preconditions
    km = KMeans(K, tol=0, random_state=11).fit(dev(X))
    check_fit("k-means++", km, X, want)
    again = KMeans(K, tol=0, random_state=11).fit(dev(X))
    assert np.array_equal(bits(km.cluster_centers_), bits(again.cluster_centers_)) and np.array_equal(bits(km.labels_), bits(again.labels_))
    assert km.inertia_ == again.inertia_
    other = KMeans(K, tol=0, random_state=12).fit(dev(X))
    assert not np.array_equal(bits(km.cluster_centers_), bits(other.cluster_centers_))


@pytest.mark.parametrize("check_every", [1, 8])
def test_fit_stops_on_the_shift(check_every):
    from evae.cluster import KMeans
    s, want = ref.solved(*ref.TOL_CASE), ref.solved_with_tol()
    km = KMeans(ref.TOL_CASE[2], init=s["C0"], tol=ref.TOL, check_every=check_every).fit(dev(s["X"]))
    print("tol = %g: the reference's shift margin %.3g, stops at %d of %d" % (ref.TOL, want["shift_margin"], want["n_iter"], s["fit"]["n_iter"]))
    assert want["n_iter"] < s["fit"]["n_iter"]
    check_fit("tol > 0", km, s["X"], want)


@pytest.mark.parametrize("how_many", [1, 3])
def test_fit_relocates_into_empty_clusters(how_many):
    from evae.cluster import KMeans
    X = ref.solved(*ref.RELOCATION_CASE)["X"]
    C0, want = ref.solved_with_relocations(how_many)
    assert want["relocations"] == how_many
    km = KMeans(len(C0), init=C0, tol=0).fit(dev(X))
    check_fit("%d far centres" % how_many, km, X, want)


def test_fit_stops_at_max_iter():
    from evae.cluster import KMeans
    s = ref.solved(*ref.CASES[3])
    want = ref.lloyd(s["X"], s["C0"], max_iter=2)
    for check_every in (1, 8):
        km = KMeans(ref.CASES[3][2], init=s["C0"], tol=0, max_iter=2, check_every=check_every).fit(dev(s["X"]))
        check_fit("max_iter = 2", km, s["X"], want)
        assert km.n_iter_ == 2


def test_n_init_returns_the_run_of_lowest_inertia():
    from evae.cluster import KMeans
    n, d, K, seed_ = ref.CASES[2]
    X = ref.solved(n, d, K, seed_)["X"]
    g = torch.Generator()
    g.manual_seed(5)
    runs = []
    for _ in range(3):
        idx = torch.randperm(n, generator=g)[:K].numpy()
        runs.append(ref.lloyd(X, X[idx].astype(np.float64)))
        assert runs[-1]["argmin_margin"] >= 1e-9
    inertias = [r["inertia"] for r in runs]
    print("n_init = 3: the reference's inertias", inertias)
    assert min(abs(a - b) for i, a in enumerate(inertias) for b in inertias[i + 1:]) > 1e-9 * max(inertias)
    km = KMeans(K, init='random', n_init=3, tol=0, random_state=5).fit(dev(X))
    check_fit("best of three", km, X, runs[int(np.argmin(inertias))])


# ---------------------------------------------------------------------------------------------- 5. the done flag
def test_steps_after_convergence_change_nothing():
    from evae import ops
    s = ref.solved(*ref.CASES[2])
    x, K = dev(s["X"]), ref.CASES[2][2]
    N, d = x.shape
    centres = dev(s["C0"])
    labels = torch.empty(N, dtype=torch.int32, device="cuda")
    d2 = torch.empty(N, dtype=torch.float64, device="cuda")
    order = torch.empty(N, dtype=torch.int32, device="cuda")
    start = torch.empty(K + 1, dtype=torch.int32, device="cuda")
    state, ws = ops.kmeans_state(x.device), ops.kmeans_workspace(N, d, K, x.device)
    for _ in range(s["fit"]["n_iter"]):
        ops.kmeans_step(x, centres, labels, d2, order, start, 0.0, state, ws)
    record = host(state)
    print("record after %d steps:" % s["fit"]["n_iter"], record)
    assert record[0] == s["fit"]["n_iter"] and record[1] == 1.0 and record[2] == 0.0 and record[3] == 0.0
    assert abs(record[4] - s["fit"]["inertia"]) <= 4 * N * EPS * s["fit"]["inertia"]
    kept = [bits(t).copy() for t in (centres, labels, d2, order, start, state)]
    for _ in range(5):
        ops.kmeans_step(x, centres, labels, d2, order, start, 0.0, state, ws)
    assert all(np.array_equal(a, bits(t)) for a, t in zip(kept, (centres, labels, d2, order, start, state)))
    assert np.array_equal(host(labels), s["fit"]["labels"])


def test_first_step_s_record_does_not_depend_on_what_the_label_buffer_held():
    """the first iteration has no previous labels: it counts every row as changed, whatever the caller's buffer holds"""
    from evae import ops
    s = ref.solved(*ref.CASES[2])
    x, K = dev(s["X"]), ref.CASES[2][2]
    N, d = x.shape
    records = []
    for fill in (0, 7, -1):
        centres = dev(s["C0"])
        labels = torch.full((N,), fill, dtype=torch.int32, device="cuda")
        d2 = torch.empty(N, dtype=torch.float64, device="cuda")
        order = torch.empty(N, dtype=torch.int32, device="cuda")
        start = torch.empty(K + 1, dtype=torch.int32, device="cuda")
        state, ws = ops.kmeans_state(x.device), ops.kmeans_workspace(N, d, K, x.device)
        ops.kmeans_step(x, centres, labels, d2, order, start, 0.0, state, ws)
        records.append(bits(state).copy())
        assert host(state)[0] == 1.0 and host(state)[2] == N
        ops.kmeans_step(x, centres, labels, d2, order, start, 0.0, state, ws)
        records.append(bits(state).copy())
    assert all(np.array_equal(records[0], r) for r in records[2::2]) and all(np.array_equal(records[1], r) for r in records[3::2])
    first = ref.assign(s["X"], s["C0"])[0]
    second = ref.assign(s["X"], ref.lloyd(s["X"], s["C0"], max_iter=1)["centres"])[0]
    assert records[1].view(np.float64)[2] == (first != second).sum()           # the second step counts against the first's labels


def test_host_tensors_are_taken_as_arrays_are():
    from evae.cluster import KMeans
    s = ref.solved(*ref.CASES[1])
    a = KMeans(ref.CASES[1][2], init=s["C0"], tol=0).fit(s["X"])
    b = KMeans(ref.CASES[1][2], init=torch.from_numpy(s["C0"]), tol=0).fit(torch.from_numpy(s["X"]))
    assert b.labels_.is_cuda and np.array_equal(bits(a.cluster_centers_), bits(b.cluster_centers_))
    assert np.array_equal(host(a.labels_), host(b.labels_)) and np.array_equal(host(b.predict(torch.from_numpy(s["X"]))), s["fit"]["labels"])


def test_transform_is_float32_whatever_the_default_dtype():
    from evae import ops
    s = ref.solved(*ref.CASES[1])
    want = ops.kmeans_transform(dev(s["X"]), dev(s["C0"]))
    torch.set_default_dtype(torch.float64)
    try:
        got = ops.kmeans_transform(dev(s["X"]), dev(s["C0"]))
    finally:
        torch.set_default_dtype(torch.float32)
    assert got.dtype == torch.float32 and np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------------------------- 6. scores
SCORE_PAIRS = ("noisy", "equal", "one cluster", "one and one", "independent", "fit of 257", "1024 x 1000")


def score_pair(name):
    rs = np.random.RandomState(7)
    y = np.arange(3000) % 10
    if name == "fit of 257":
        s = ref.solved(*ref.CASES[5])
        return s["y"], s["fit"]["labels"]
    return {"noisy": (y, np.where(rs.random_sample(3000) < 0.3, rs.randint(0, 7, 3000), y % 7)),
            "equal": (y, y), "one cluster": (y, np.zeros(3000, int)), "one and one": (np.zeros(700, int), np.zeros(700, int)),
            "independent": (y, rs.randint(0, 4, 3000)),
            "1024 x 1000": (rs.randint(0, 1024, 50000), rs.randint(0, 1000, 50000))}[name]


@pytest.mark.parametrize("name", SCORE_PAIRS)
def test_scores_against_the_reference(name):
    from evae import ops
    a, b = score_pair(name)
    Ka, Kb, n = int(a.max()) + 1, int(b.max()) + 1, len(a)
    table = ops.cluster_contingency(dev(a.astype(np.int32)), Ka, dev(b.astype(np.int32)), Kb)
    want_table = ref.contingency(a, Ka, b, Kb)
    assert table.dtype == torch.int64 and np.array_equal(host(table), want_table)
    got, want = host(ops.cluster_scores(table)), ref.scores(want_table)
    log_n = 1.0 + math.log(n)
    b_mi, b_h = (math.ceil(Ka * Kb / 1024) + 18) * EPS * log_n, 19 * EPS * log_n
    mean_h = 0.5 * (want["entropy_a"] + want["entropy_b"])
    b_nmi = (b_mi + b_h) / mean_h + 4 * EPS if mean_h > 0 else 0.0
    errs = dict(entropy_a=abs(got[0] - want["entropy_a"]), entropy_b=abs(got[1] - want["entropy_b"]),
                mutual_info=abs(got[2] - want["mutual_info"]), nmi=abs(got[3] - want["nmi"]), ari=abs(got[4] - want["ari"]))
    print("scores %s: nmi %.6f ari %.6f purity %.6f; errors H %.3g %.3g (allowed %.3g), MI %.3g (%.3g), NMI %.3g (%.3g), ARI %.3g (%.3g)"
          % (name, got[3], got[4], got[5], errs["entropy_a"], errs["entropy_b"], b_h, errs["mutual_info"], b_mi, errs["nmi"], b_nmi,
             errs["ari"], 16 * EPS))
    assert errs["entropy_a"] <= b_h and errs["entropy_b"] <= b_h and errs["mutual_info"] <= b_mi
    assert errs["nmi"] <= b_nmi and errs["ari"] <= 16 * EPS
    assert got[5] == want["purity"] and got[6] == n
    if name == "one and one":
        assert got[3] == 1.0 and got[4] == 1.0
    if name == "one cluster":
        assert got[3] == 0.0 and got[4] == 0.0
    assert np.array_equal(bits(ops.cluster_scores(table)), bits(ops.cluster_scores(table)))


def test_score_functions_take_arbitrary_labels():
    from evae import cluster
    rs = np.random.RandomState(2)
    a = rs.randint(0, 5, 400)
    b = np.where(rs.random_sample(400) < 0.2, rs.randint(0, 5, 400), a)
    want = ref.scores(ref.contingency(a, 5, b, 5))
    names = np.array([-7, 3, 40, 41, 1000])                 # not 0 .. K - 1, int64, one side on the host
    assert np.array_equal(host(cluster.contingency_matrix(names[a], dev(names[b] * 2))), ref.contingency(a, 5, b, 5))
    assert abs(cluster.normalized_mutual_info_score(names[a], dev(b)) - want["nmi"]) <= 1e-13
    assert abs(cluster.adjusted_rand_score(dev(a), names[b]) - want["ari"]) <= 16 * EPS
    assert cluster.purity_score(a, b) == want["purity"]


# ---------------------------------------------------------------------------------------------- 7. silhouette
@pytest.fixture(scope="module")
def silhouette_case():
    s = ref.solved(*ref.CASES[2])
    labels = s["fit"]["labels"].copy()
    labels[[0, 700]] = [10, 11]                             # two singleton clusters
    return s["X"], labels, ref.silhouette_samples(s["X"], labels)


def test_silhouette_against_the_reference(silhouette_case):
    from evae import cluster
    X, labels, want = silhouette_case
    got = cluster.silhouette_samples(dev(X), labels)
    assert got.dtype == torch.float64 and got.is_cuda
    err = np.abs(host(got) - want).max()
    print("silhouette N=%d: %.3g from the reference (allowed %.3g); mean %.6f" % (len(X), err, 2.0 ** -22, want.mean()))
    assert err <= 2.0 ** -22
    assert host(got)[0] == 0.0 and host(got)[700] == 0.0    # singletons
    for strip_rows in (1000, 64, 333):
        assert np.array_equal(bits(got), bits(cluster.silhouette_samples(dev(X), labels, strip_rows=strip_rows)))
    score = cluster.silhouette_score(dev(X), labels)
    assert abs(score - want.mean()) <= 2.0 ** -22
    quality = cluster.clustering_quality(dev(X), labels, labels_true=np.arange(len(X)) % 10)
    assert quality["silhouette"] == score and quality["n_clusters"] == 12 and quality["n_samples"] == len(X)
    assert set(quality) == {"n_samples", "n_clusters", "n_classes", "nmi", "ari", "purity", "silhouette"}
    assert set(cluster.clustering_quality(dev(X), labels, silhouette=False)) == {"n_samples", "n_clusters"}


def test_silhouette_of_small_and_odd_inputs():
    from evae import cluster
    for n, d, K, seed_ in (ref.CASES[1], ref.CASES[6], ref.CASES[11]):
        s = ref.solved(n, d, K, seed_)
        got = host(cluster.silhouette_samples(dev(s["X"]), s["fit"]["labels"]))
        err = np.abs(got - ref.silhouette_samples(s["X"], s["fit"]["labels"])).max()
        print("silhouette n=%d d=%d K=%d: %.3g (allowed %.3g)" % (n, d, K, err, 2.0 ** -22))
        assert err <= 2.0 ** -22
    X = np.repeat(np.array([[0.0, 0.0], [1.0, 1.0]], np.float32), 3, axis=0)       # max(a, b) = 0 never; a = 0 always: s = 1
    assert np.array_equal(host(cluster.silhouette_samples(dev(X), [0, 0, 0, 1, 1, 1])), np.ones(6))
    same = np.zeros((6, 2), np.float32)                                            # max(a, b) = 0: s = 0
    assert np.array_equal(host(cluster.silhouette_samples(dev(same), [0, 0, 0, 1, 1, 1])), np.zeros(6))


def test_silhouette_refuses_one_cluster_and_n_clusters():
    from evae import cluster
    X = dev(blobs(40, 3, 2, seed=1)[0])
    for labels in (np.zeros(40, int), np.arange(40)):
        with pytest.raises(ValueError):
            cluster.silhouette_score(X, labels)
        with pytest.raises(ValueError):
            cluster.silhouette_samples(X, labels)
    with pytest.raises(ValueError):
        cluster.silhouette_samples(X, np.arange(39) % 3)


# ---------------------------------------------------------------------------------------------- 8. refusals
def test_ops_refuse_what_they_cannot_take():
    from evae import ops, _lib
    x, c = torch.randn(64, 8, device="cuda"), torch.randn(4, 8, device="cuda", dtype=torch.float64)
    labels = torch.zeros(64, dtype=torch.int32, device="cuda")
    refused = [
        lambda: ops.kmeans_assign(x.cpu(), c.cpu()),                                 # CPU tensors
        lambda: ops.kmeans_assign(x, c.cpu()),
        lambda: ops.kmeans_assign(x.double(), c),                                    # wrong dtypes
        lambda: ops.kmeans_assign(x, c.float()),
        lambda: ops.kmeans_assign(x.t().contiguous().t(), c),                        # non-contiguous
        lambda: ops.kmeans_assign(x, c.t().contiguous().t()),
        lambda: ops.kmeans_assign(x, c[:, :7].contiguous()),                         # another width
        lambda: ops.kmeans_assign(torch.zeros(8, 257, device="cuda"), torch.zeros(2, 257, device="cuda", dtype=torch.float64)),
        lambda: ops.kmeans_assign(x, torch.zeros(1025, 8, device="cuda", dtype=torch.float64)),
        lambda: ops.kmeans_assign(torch.zeros(2 ** 20 + 1, 1, device="cuda"), torch.zeros(2, 1, device="cuda", dtype=torch.float64)),
        lambda: ops.kmeans_transform(x, c.float()),
        lambda: ops.kmeans_update(x, labels.long(), 4),
        lambda: ops.kmeans_update(x, labels[:63].contiguous(), 4),
        lambda: ops.kmeans_update(x, labels, 1025),
        lambda: ops.kmeans_update(x.cpu(), labels.cpu(), 4),
        lambda: ops.kmeans_seed(x, 65, torch.zeros(65, dtype=torch.float64, device="cuda")),      # more centres than points
        lambda: ops.kmeans_seed(x, 4, torch.zeros(4, device="cuda")),                             # float32 uniforms
        lambda: ops.kmeans_seed(x, 4, torch.zeros(5, dtype=torch.float64, device="cuda")),
        lambda: ops.kmeans_inertia(torch.zeros(8, device="cuda")),
        lambda: ops.cluster_contingency(labels, 4, labels.long(), 4),
        lambda: ops.cluster_contingency(labels, 4, labels, 1025),
        lambda: ops.cluster_contingency(labels.cpu(), 4, labels.cpu(), 4),
        lambda: ops.cluster_scores(torch.zeros(4, 4, dtype=torch.int32, device="cuda")),
        lambda: ops.cluster_scores(torch.zeros(4, 1025, dtype=torch.int64, device="cuda")),
        lambda: ops.silhouette_samples(x, labels.long(), torch.tensor([0, 64], dtype=torch.int32, device="cuda")),
        lambda: ops.silhouette_samples(x.cpu(), labels.cpu(), torch.tensor([0, 64], dtype=torch.int32)),
        lambda: ops.silhouette_samples(x, labels, torch.tensor([0, 64], dtype=torch.int32, device="cuda"), strip_rows=-1),
        lambda: ops.silhouette_samples(torch.zeros(ops.tsne_nn_max_points() + 1, 1, device="cuda"),
                                       torch.zeros(ops.tsne_nn_max_points() + 1, dtype=torch.int32, device="cuda"),
                                       torch.tensor([0, 1], dtype=torch.int32, device="cuda")),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(_lib.EvaeError):
            call()
            pytest.fail("refusal %d did not raise" % i)
    state, ws = ops.kmeans_state(x.device), ops.kmeans_workspace(64, 8, 4, x.device)
    d2, order, start = torch.empty(64, dtype=torch.float64, device="cuda"), labels.clone(), torch.empty(5, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.EvaeError):
        ops.kmeans_step(x, c, labels, d2.float(), order, start, 0.0, state, ws)
    with pytest.raises(_lib.EvaeError):
        ops.kmeans_step(x, c, labels, d2, order, start, -1.0, state, ws)
    with pytest.raises(_lib.EvaeError):
        ops.kmeans_step(x, c, labels, d2, order, start, 0.0, state, ws[:64])      # a workspace too small: refused by the library
    from evae.cluster import KMeans
    with pytest.raises(_lib.EvaeError):
        KMeans(2).predict(x)                                                      # not fitted


# ---------------------------------------------------------------------------------------------- 9. the report
def test_report_on_a_stub_model(tmp_path, capsys):
    import evae_oracle as orc
    import smoke_case
    import golden_inputs as gi
    from evae import cluster
    from utils.cluster_on_latent import report_kmeans_on_latent
    from utils.knn_on_latent import _posterior_means
    n, B = 75, 32
    args = smoke_case.vae_args(number_components=20, training_set_size=100, batch_size=B)
    args.seed, args.kmeans_n_init, args.kmeans_max_iter = 3, 2, 50
    model, _ = smoke_case.build_model(torch, np, orc, args)
    model.eval()
    data = torch.from_numpy(gi.binary_images(91, n))
    labels = torch.arange(n) % 10
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, labels), batch_size=B, shuffle=False)
    with torch.no_grad():
        z = _posterior_means(model, data.to(args.device), B)
    N, zd = z.shape
    assert N == 64

    out = str(tmp_path / "kmeans")
    got = report_kmeans_on_latent(loader, model, out, args)
    assert "k-means of" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == ["kmeans_centres.npy", "kmeans_labels.npy", "kmeans_quality.json"]
    km = cluster.KMeans(10, n_init=2, max_iter=50, random_state=3).fit(z)      # 10 distinct labels: the default of kmeans_clusters
    saved = np.load(os.path.join(out, "kmeans_labels.npy"))
    assert got.is_cuda and saved.dtype == np.int32 and np.array_equal(saved, host(got)) and np.array_equal(saved, host(km.labels_))
    centres = np.load(os.path.join(out, "kmeans_centres.npy"))
    assert centres.dtype == np.float64 and centres.shape == (10, zd) and np.array_equal(centres, host(km.cluster_centers_))
    quality = json.load(open(os.path.join(out, "kmeans_quality.json")))
    direct = cluster.clustering_quality(z, km.labels_, labels_true=labels[:N])
    assert quality == dict(inertia=km.inertia_, n_iter=km.n_iter_, n_clusters=10, n_samples=N, nmi=direct["nmi"], ari=direct["ari"],
                           purity=direct["purity"], silhouette=direct["silhouette"])
    args.kmeans_clusters, args.kmeans_silhouette = 4, False
    report_kmeans_on_latent(loader, model, out, args)
    quality = json.load(open(os.path.join(out, "kmeans_quality.json")))
    assert quality["n_clusters"] == 4 and quality["silhouette"] is None and np.load(os.path.join(out, "kmeans_centres.npy")).shape == (4, zd)
