"""CPU-only: tests/nn_rank_ref.py, the yardstick of tests/test_gpu_nn_rank.py, held to scikit-learn's trustworthiness and to cases
small enough to check by hand."""
import numpy as np
import pytest

import nn_rank_ref as rr


def sq_distances(X):
    X = np.asarray(X, np.float64)
    return ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)


@pytest.mark.parametrize("n,zd,k", [(97, 40, 5), (300, 8, 12), (257, 3, 30)])
def test_trustworthiness_and_continuity_are_scikit_learns(n, zd, k):
    """tie-free float64 Gaussian data: the same integers through the same expression.  Squared distances order as distances do."""
    manifold = pytest.importorskip("sklearn.manifold")
    rs = np.random.RandomState(100 + n)
    X, Y = rs.randn(n, zd), rs.randn(n, 2)
    DX, DY = sq_distances(X), sq_distances(Y)
    t, c = rr.trustworthiness(DX, DY, k), rr.continuity(DX, DY, k)
    want_t, want_c = manifold.trustworthiness(X, Y, n_neighbors=k), manifold.trustworthiness(Y, X, n_neighbors=k)
    print("trustworthiness %.17g (scikit-learn %.17g), continuity %.17g (scikit-learn %.17g)" % (t, want_t, c, want_c))
    assert abs(t - want_t) <= 1e-12 and abs(c - want_c) <= 1e-12
    assert 0.0 < t < 1.0 and 0.0 < c < 1.0 and t != c
    q = rr.embedding_quality(DX, DY, k)
    assert q["trustworthiness"] == t and q["continuity"] == c and q["n_neighbors"] == k and q["n_samples"] == n
    assert 0.0 <= q["neighbourhood_preservation"] <= 1.0 and "label_accuracy" not in q


def test_a_line_of_six_points():
    x = np.array([0.0, 1.0, 3.0, 6.0, 10.0, 15.0])
    D = (x[:, None] - x[None, :]) ** 2
    # from point 2 (x = 3): 1 at distance 2, 0 and 3 both at distance 3 (index decides: 0 first), 4 at 7, 5 at 12
    assert rr.ranks(D, np.tile(np.arange(6), (6, 1)))[2].tolist() == [2, 1, 0, 3, 4, 5]
    # from point 0: in order of x; from point 5: in reverse
    nbr = np.array([[1, 5], [0, 2], [1, 3], [2, 5], [3, 0], [4, 0]])
    rank = rr.ranks(D, nbr)
    assert rank.tolist() == [[1, 5], [1, 2], [1, 3], [1, 5], [1, 5], [1, 5]]
    # k = 2: penalties max(0, rank - 2), hits rank <= 2
    assert rr.row_sums(rank).tolist() == [[3, 1], [0, 2], [1, 1], [3, 1], [3, 1], [3, 1]]
    assert rr.neighbours(D, 2).tolist() == [[1, 2], [0, 2], [1, 0], [2, 4], [3, 5], [4, 3]]
    # an embedding that is the line itself: nothing to penalise, everything preserved
    assert rr.trustworthiness(D, D, 2) == 1.0 and rr.continuity(D, D, 2) == 1.0 and rr.neighbourhood_preservation(D, D, 2) == 1.0
    # 6 points, k = 2: 1 - 2 / (6 * 2 * (12 - 6 - 1)) * penalty
    assert rr.score(10, 6, 2) == 1.0 - 10 * (2.0 / 60.0)


def test_identical_rows_are_ordered_by_index():
    X = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0], [5.0, 0.0], [0.0, 0.0]])
    D = sq_distances(X)
    every = np.tile(np.arange(5), (5, 1))
    rank = rr.ranks(D, every)
    assert rank[0].tolist() == [0, 2, 3, 4, 1]       # its duplicate 4 counts, and comes first at distance 0; then 1 before 2
    assert rank[1].tolist() == [2, 0, 1, 4, 3]       # from 1: its twin 2 at 0; 0 and 4 tie at 1: 0 first
    assert rank[2].tolist() == [2, 1, 0, 4, 3]       # from 2: the twin 1 at 0
    assert rank[4].tolist() == [1, 2, 3, 4, 0]
    assert rr.neighbours(D, 2).tolist() == [[4, 1], [2, 0], [1, 0], [1, 2], [0, 1]]


def test_entries_that_name_the_point_itself_or_no_point():
    x = np.array([0.0, 1.0, 3.0, 6.0])
    D = (x[:, None] - x[None, :]) ** 2
    nbr = np.array([[0, 3], [4, 0], [-1, 3], [2, 3]])      # j == i in rows 0 and 3, j == N in row 1, j == -1 in row 2
    rank = rr.ranks(D, nbr)
    assert rank.tolist() == [[0, 3], [0, 1], [0, 3], [1, 0]]
    assert rr.row_sums(rank).tolist() == [[1, 0], [0, 1], [1, 0], [0, 1]]      # k = 2; the guarded entries add nothing


def test_the_vote():
    nbr = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 5], [0, 2, 4]])
    labels = np.array([7, 7, 3, 3, 3, 5])
    # row 0: votes 7, 3, 3 -> 3 (wrong); row 1: 7, 3, 3 -> 3 (wrong); row 2: 7, 7, 3 -> 7 (wrong); row 3: 7, 7, 3 -> 7 (wrong)
    # row 4: labels 7, 7, 5 -> 7 (wrong); row 5: 7, 3, 3 -> 3 (wrong)
    assert rr.label_accuracy(nbr, labels) == 0.0
    # a three-way tie goes to the lowest class
    assert rr.label_accuracy(np.array([[1, 2, 3]] * 4), np.array([3, 7, 5, 3])) == 0.5      # 7, 5, 3 once each -> 3: right for rows 0 and 3
