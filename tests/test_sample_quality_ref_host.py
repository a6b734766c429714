"""CPU-only: tests/sample_quality_ref.py, the yardstick of tests/test_gpu_sample_quality.py, held to an independent formulation on
scikit-learn's distances with the `prdc` package's four expressions in their original form, and to cases small enough to check by
hand.

The two formulations round distances differently -- the restatement is fed fp32-rounded squared direct differences, as the
device computes them; the other takes scikit-learn's float64 expansion and a square root -- so a distance within rounding of a
radius could flip an indicator.  The seeds below were picked (on the CPU, by running this file) so that none does:
test_prdc_is_the_packages checks the margin itself before it compares, and the comparison is for equality."""
import numpy as np
import pytest

import sample_quality_ref as rr


def sq_distances_f32(A, B):
    """squared direct differences accumulated in float64, rounded once to float32: what the device's distance kernel gives"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return ((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2).astype(np.float32)


def gaussian_blobs(n, d, seed, shift=0.0):
    """four blobs whose means depend on d alone, so that two draws are two samples of one distribution"""
    means = np.random.RandomState(1000 + d).randn(4, d) * 4.0 / np.sqrt(d) * np.sqrt(2.0)
    rs = np.random.RandomState(seed)
    return (means[np.arange(n) % 4] + rs.randn(n, d) + shift).astype(np.float32)


def prdc_as_published(real, fake, nearest_k):
    """Naeem et al.'s compute_prdc, expression for expression, on sklearn.metrics.pairwise_distances"""
    from sklearn.metrics import pairwise_distances

    def kth(x):                                              # the row itself is included, at distance 0: the (k + 1)-th value
        return np.partition(pairwise_distances(x, x, metric='euclidean'), nearest_k, axis=-1)[..., nearest_k]

    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    real_radii, fake_radii = kth(real), kth(fake)
    distance_real_fake = pairwise_distances(real, fake, metric='euclidean')
    precision = (distance_real_fake < np.expand_dims(real_radii, axis=1)).any(axis=0).mean()
    recall = (distance_real_fake < np.expand_dims(fake_radii, axis=0)).any(axis=1).mean()
    density = (1. / float(nearest_k)) * (distance_real_fake < np.expand_dims(real_radii, axis=1)).sum(axis=0).mean()
    coverage = (distance_real_fake.min(axis=1) < real_radii).mean()
    return dict(precision=precision, recall=recall, density=density, coverage=coverage), distance_real_fake, real_radii, fake_radii


@pytest.mark.parametrize("n,m,d,seed", [(300, 257, 8, 11), (97, 61, 40, 12)])
@pytest.mark.parametrize("k", [1, 5])
def test_prdc_is_the_packages(n, m, d, k, seed):
    R, F = gaussian_blobs(n, d, seed), gaussian_blobs(m, d, seed + 100, shift=0.3)
    want, dist, real_radii, fake_radii = prdc_as_published(R, F, k)
    # the margin the seeds were picked for: no distance within 1e-5 (relative) of a radius it is compared with; the two
    # formulations differ by some 1e-7 (fp32 rounding of the squares), the float64 expansion by far less at this scale
    for radius in (real_radii[:, None], fake_radii[None, :]):
        assert np.abs(dist / radius - 1.0).min() > 1e-5
    got = rr.prdc(sq_distances_f32(R, R), sq_distances_f32(F, F), sq_distances_f32(R, F), k)
    print("restatement %s\nas published %s" % (got, want))
    for key in ("precision", "recall", "density", "coverage"):
        assert type(got[key]) is float and got[key] == want[key], key
    assert (got["nearest_k"], got["n_real"], got["n_fake"]) == (k, n, m)
    assert 0.0 < got["precision"] < 1.0 and 0.0 < got["recall"] < 1.0 and 0.0 < got["coverage"] < 1.0      # the counts count
    # the radii themselves: the same rows' k-th other neighbour, up to the two roundings
    assert np.allclose(np.sqrt(rr.radii(sq_distances_f32(R, R), k).astype(np.float64)), real_radii, rtol=1e-6, atol=0.0)


def line(xs):
    return np.asarray(xs, np.float64)[:, None]


def test_points_on_a_line():
    R, F = line([0.0, 1.0, 3.0, 6.0]), line([0.5, 2.9, 20.0])
    DRR, DFF, DRF = sq_distances_f32(R, R), sq_distances_f32(F, F), sq_distances_f32(R, F)
    assert rr.radii(DRR, 1).tolist() == [1.0, 1.0, 4.0, 9.0] and rr.radii(DRR, 2).tolist() == [9.0, 4.0, 9.0, 25.0]
    assert np.allclose(rr.radii(DFF, 1), [5.76, 5.76, 292.41])
    #   D(R, F)   0.5     2.9    20
    #   0         0.25    8.41   400
    #   1         0.25    3.61   361
    #   3         6.25    0.01   289
    #   6        30.25    9.61   196
    # generated rows in real balls (radii 1, 1, 4, 9): 0.5 in those of 0 and 1; 2.9 in that of 3 only (9.61 is outside 9); 20 in none
    in_real = rr.ball_counts(DRF.T, col_radius=rr.radii(DRR, 1))[0]
    assert in_real.tolist() == [2, 1, 0]
    # real rows in generated balls (radii 5.76, 5.76, 292.41): the far sample's ball is wide enough to hold 3 and 6
    in_fake, own = rr.ball_counts(DRF, col_radius=rr.radii(DFF, 1), row_radius=rr.radii(DRR, 1))
    assert in_fake.tolist() == [1, 2, 2, 1] and own.tolist() == [1, 1, 1, 0]
    q = rr.prdc(DRR, DFF, DRF, 1)
    assert q == dict(precision=2 / 3, recall=1.0, density=1.0, coverage=0.75, nearest_k=1, n_real=4, n_fake=3)
    # nearest real: 0.5 is as far from 0 as from 1, the lower index wins
    idx, d2 = rr.nearest(DRF.T)
    assert idx.tolist() == [0, 2, 3] and d2.tolist() == [0.25, np.float32(0.01), 196.0]
    # authentic: only the far one (196 >= 9); 0.25 < 1 and 0.01 < 4 are closer than the real rows' own neighbours
    assert rr.authentic_count(DRR, DRF) == 1 and rr.authenticity(DRR, DRF) == 1 / 3
    assert rr.nearest_distance_median(DRF) == 0.5
    # strictness: a distance equal to the radius is outside the ball
    col, row = rr.ball_counts(np.array([[1.0, 4.0]]), col_radius=[1.0, 4.0], row_radius=[4.0])
    assert col.tolist() == [0] and row.tolist() == [1]


def test_the_generated_rows_are_the_real_ones():
    R = gaussian_blobs(60, 5, 3)
    D = sq_distances_f32(R, R)
    for k in (1, 5):
        assert rr.radii(D, k).min() > 0.0
        q = rr.prdc(D, D, D, k)
        assert q["precision"] == 1.0 and q["recall"] == 1.0 and q["coverage"] == 1.0 and q["density"] >= 1.0
    assert rr.authenticity(D, D) == 0.0                      # every row is a copy of a real row


def test_a_block_of_identical_rows_has_radius_zero():
    """four copies of one row, k = 2: their radius is 0, nothing is strictly inside it -- they hold nobody and cover nothing"""
    R = line([0.0, 0.0, 0.0, 0.0, 10.0, 11.0, 12.5, 14.0])
    D = sq_distances_f32(R, R)
    assert rr.radii(D, 2).tolist()[:4] == [0.0] * 4 and rr.radii(D, 2).min() == 0.0 and rr.radii(D, 4)[0] == 100.0
    q = rr.prdc(D, D, D, 2)
    assert q["precision"] == 0.5 and q["recall"] == 0.5 and q["coverage"] == 0.5
    col, row = rr.ball_counts(D, col_radius=rr.radii(D, 2), row_radius=rr.radii(D, 2))
    assert col[:4].tolist() == [0] * 4 and row[:4].tolist() == [0] * 4 and col[4:].min() >= 1
    # a copy of a duplicated row is at distance 0 from a row whose nearest other row is at 0 too: 0 >= 0 counts as authentic
    assert rr.authentic_count(D, D) == 4


def test_a_far_outlier_among_the_generated_rows():
    R = gaussian_blobs(50, 3, 5)
    F = gaussian_blobs(40, 3, 6)
    DRR = sq_distances_f32(R, R)
    base = rr.prdc(DRR, sq_distances_f32(F, F), sq_distances_f32(R, F), 1)
    assert 0.0 < base["recall"] < 1.0
    # alone out there, its nearest neighbour is in the crowd: its ball reaches that far and holds every real row that is nearer
    # to it than that neighbour is, so recall rises although nothing was generated near those rows
    lone = np.vstack((F, np.full((1, 3), 1000.0, np.float32)))
    q = rr.prdc(DRR, sq_distances_f32(lone, lone), sq_distances_f32(R, lone), 1)
    held_before = rr.ball_counts(sq_distances_f32(R, F), col_radius=rr.radii(sq_distances_f32(F, F), 1))[0] > 0
    held_by_it = sq_distances_f32(R, lone)[:, -1] < sq_distances_f32(lone, lone)[-1, :-1].min()
    assert 0 < held_by_it.sum() < 50 and (held_by_it & ~held_before).any()
    assert q["recall"] == int((held_before | held_by_it).sum()) / 50 > base["recall"]
    assert q["precision"] == round(base["precision"] * 40) / 41 and q["coverage"] == base["coverage"]
    # with a companion next to it, its radius excludes the real rows: recall and coverage stay, precision loses two samples
    pair = np.vstack((F, np.full((1, 3), 1000.0, np.float32), np.full((1, 3), 1000.5, np.float32)))
    q = rr.prdc(DRR, sq_distances_f32(pair, pair), sq_distances_f32(R, pair), 1)
    in_real = rr.ball_counts(sq_distances_f32(pair, R), col_radius=rr.radii(DRR, 1))[0]
    assert in_real[-2:].tolist() == [0, 0]
    assert q["recall"] == base["recall"] and q["coverage"] == base["coverage"]
    assert q["precision"] == int((in_real > 0).sum()) / 42 and int((in_real > 0).sum()) == round(base["precision"] * 40)


def test_copies_are_not_authentic_and_translates_are():
    T = gaussian_blobs(80, 6, 9)
    DTT = sq_distances_f32(T, T)
    assert rr.radii(DTT, 1).min() > 0.0
    copies = T[[3, 3, 17, 79, 0]]
    assert rr.authenticity(DTT, sq_distances_f32(T, copies)) == 0.0
    assert rr.nearest(sq_distances_f32(copies, T))[0].tolist() == [3, 3, 17, 79, 0]
    away = T + np.float32(1000.0)
    assert rr.authenticity(DTT, sq_distances_f32(T, away)) == 1.0
    mixed = np.vstack((copies, away[:15]))
    assert rr.authenticity(DTT, sq_distances_f32(T, mixed)) == 15 / 20
    q = rr.sample_quality(DTT, sq_distances_f32(mixed, mixed), sq_distances_f32(T, mixed), 2)
    assert q["authenticity"] == 0.75 and sorted(q) == sorted(["precision", "recall", "density", "coverage", "nearest_k", "n_real",
                                                               "n_fake", "authenticity", "nearest_distance_median"])
