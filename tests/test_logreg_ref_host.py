"""CPU-only: the numpy restatement tests/logreg_ref.py (the yardstick of tests/test_gpu_logreg.py) is held to its own margins, to
scikit-learn, and to a replay of itself in a wider format.

* Margins.  At the default tol every row of the table keeps its Armijo margins >= 1e-9 and its stop margins >= 1e-6: the GPU
  test compares n_iter_, converged_ and line_steps_ exactly, which means something only where the restatement was that far from
  deciding otherwise.  (At tol = 1e-7 the Armijo margins fall to 1e-13 -- the objective no longer changes in its leading digits
  -- which is why decisions are compared at the default tol only.)
* Coverage.  A row picks j > 0; a row runs more than `history` iterations, so the ring of pairs wraps.
* scikit-learn (1.7.2 here).  For K >= 3 the restatement at tol 1e-8 reaches the objective of LogisticRegression(tol=1e-10) on
  float64 input within SPREAD['sklearn_excess'] (relative), and its training predictions equal scikit-learn's wherever the
  restatement's top-two logit gap exceeds 1e-6.
* Rounding spread.  The float64 run's decisions replayed in numpy.longdouble (64-bit significand): the relative differences of
  coefficients, loss and directions stay within SPREAD, which holds 10 x the largest measured.  Where numpy.longdouble is no
  wider than float64 the replay is the one with exact (rational) sums, dots and products instead; that replay itself is checked
  against fractions.Fraction on every platform.
Every test prints the figures it asserts on."""
import numpy as np
import pytest

import logreg_ref as ref

ROWS = pytest.mark.parametrize("row", ref.CASES, ids=ref.case_id)


@ROWS
def test_margins(row):
    _, _, r = ref.solved(row)
    armijo, stop = min(r['armijo_margin']), min(r['stop_margin'])
    print("%s: %d iterations, converged %s, steps %s, smallest Armijo margin %.3g, smallest stop margin %.3g"
          % (ref.case_id(row), r['n_iter'], r['converged'], r['js'], armijo, stop))
    assert r['converged'] and not r['line_failed'] and 0 < r['n_iter'] < ref.MAX_ITER
    assert len(r['stop_margin']) == r['n_iter'] + 1 and len(r['armijo_margin']) == r['n_iter']
    assert armijo >= 1e-9
    assert stop >= 1e-6


def test_coverage():
    fits = [ref.solved(row)[2] for row in ref.CASES]
    halved = [ref.case_id(row) for row, r in zip(ref.CASES, fits) if max(r['js']) > 0]
    wrapped = [ref.case_id(row) for row, r in zip(ref.CASES, fits) if sum(r['accepted']) > ref.HISTORY]
    print("rows that pick j > 0:", halved, "| rows whose ring wraps:", wrapped)
    assert halved and wrapped
    assert any(not row[5] for row in ref.CASES) and any(row[2] == 2 for row in ref.CASES)
    assert any(row[0] % ref.CHUNK == 1 for row in ref.CASES) and any(row[0] % ref.CHUNK == ref.CHUNK - 1 for row in ref.CASES)


def test_objective_and_gradient_agree():
    """the restatement's gradient is the derivative of its objective (central differences in longdouble)"""
    row = ref.CASES[0]
    X, y, r = ref.solved(row)
    C, fi = row[6], row[5]
    W = np.asarray(r['W'], np.longdouble)
    G = ref.gradient_at(X, y, W, C, fi, np.longdouble)
    rs = np.random.RandomState(0)
    V = rs.standard_normal(W.shape).astype(np.longdouble)
    h = np.longdouble(1e-6)
    num = (ref.objective(X, y, W + h * V, C, fi, np.longdouble) - ref.objective(X, y, W - h * V, C, fi, np.longdouble)) / (2 * h)
    err = float(abs(num - (G * V).sum()) / max(1.0, float(abs(num))))
    print("directional derivative: central difference against G.V, relative error %.3g" % err)
    assert err <= 1e-8


@pytest.mark.parametrize("row", [r for r in ref.CASES if r[2] >= 3], ids=ref.case_id)
def test_agrees_with_sklearn(row):
    pytest.importorskip('sklearn')
    from sklearn.linear_model import LogisticRegression
    n, d, K, seed, sep, fi, C = row
    X, y = ref.blobs(n, d, K, seed, sep)
    r = ref.fit(X, y, K, C=C, tol=1e-8, fit_intercept=fi, max_iter=1000)
    assert r['converged']
    X64 = X.astype(np.float64)
    sk = LogisticRegression(C=C, tol=1e-10, max_iter=100000, fit_intercept=fi).fit(X64, y)
    Wsk = np.concatenate([sk.coef_, sk.intercept_[:, None]], axis=1) if fi else sk.coef_
    f_ref, f_sk = float(ref.objective(X, y, r['W'], C, fi)), float(ref.objective(X, y, Wsk, C, fi))
    excess = (f_ref - f_sk) / abs(f_sk)
    gap = ref.top_two_gap(r['Z'])
    differ = int(((r['Z'].argmax(axis=1) != sk.predict(X64)) & (gap > 1e-6)).sum())
    print("%s: %d iterations at tol 1e-8, f %.17g, scikit-learn's %.17g, excess %.3g (allowed %.3g); %d rows with a top-two gap "
          "<= 1e-6, %d predictions differ above it" % (ref.case_id(row), r['n_iter'], f_ref, f_sk, excess, ref.SPREAD['sklearn_excess'],
                                                       int((gap <= 1e-6).sum()), differ))
    assert excess <= ref.SPREAD['sklearn_excess']
    assert differ == 0


WIDER = np.finfo(np.longdouble).eps < 2.0 ** -60                  # numpy.longdouble has a significand of 64 bits or more


def _replay_spread(row, exact):
    n, d, K, seed, sep, fi, C = row
    X, y, r = ref.solved(row)
    if exact:
        wide = ref.fit(X, y, K, C=C, fit_intercept=fi, replay=r, exact=True)
    else:
        wide = ref.fit(X, y, K, C=C, fit_intercept=fi, dt=np.longdouble, replay=r)
    assert wide['n_iter'] == r['n_iter'] and wide['js'] == r['js']
    return dict(coef=ref.rel_err(r['W'], wide['W']), loss=ref.rel_err(r['loss'], wide['loss']),
                direction=max(ref.rel_err(a, b) for a, b in zip(r['directions'], wide['directions'])))


def test_rounding_spread():
    """the float64 run against its replay in numpy.longdouble -- or, where that is no wider than float64, against its replay
    with exact (rational) sums, dots and products, which then stands for the wider format: exp and log have no rational value
    and stay float64's there, so that replay can only show LESS than SPREAD holds, and only the upper side is asserted"""
    worst = dict(coef=0.0, loss=0.0, direction=0.0)
    for row in ref.CASES:
        sp = _replay_spread(row, exact=not WIDER)
        print(ref.case_id(row), {k: "%.3g" % v for k, v in sp.items()})
        worst = {k: max(worst[k], sp[k]) for k in worst}
    print("replay in %s; largest over the table:" % ("numpy.longdouble" if WIDER else "exact sums"), {k: "%.3g" % v for k, v in worst.items()},
          "| SPREAD (10 x what numpy.longdouble shows):", {k: ref.SPREAD[k] for k in worst})
    for k in worst:
        assert worst[k] <= ref.SPREAD[k]                       # SPREAD holds 10 x the figures measured when it was written
        if WIDER:
            assert ref.SPREAD[k] <= 100 * worst[k] + 1e-300, "SPREAD[%r] is no longer 10 x what is measured" % k


def test_exact_replay_is_exact_and_stays_within_the_spread():
    """the replay for platforms without a wider format, run here on the smallest row whatever the platform: its sums, dots and
    products equal the rationals' (fractions.Fraction) rounded once, and it differs from the float64 run by no more than SPREAD"""
    from fractions import Fraction
    rs = np.random.RandomState(3)
    a, b = rs.standard_normal(301) * 10.0 ** rs.randint(-8, 8, 301), rs.standard_normal(301)
    A, B = rs.standard_normal((7, 40)), rs.standard_normal((40, 3))
    ref._EXACT = True
    try:
        got = float(ref.dot(a, b)), float(ref.total(a)), ref.total(A, 0), ref.total(A, 1), ref.mm(A, B)
    finally:
        ref._EXACT = False
    fr = lambda v: [Fraction(float(x)) for x in v]
    assert got[0] == float(sum(x * z for x, z in zip(fr(a), fr(b)))) and got[1] == float(sum(fr(a)))
    assert got[2].tolist() == [float(sum(fr(A[:, j]))) for j in range(40)] and got[3].tolist() == [float(sum(fr(A[i]))) for i in range(7)]
    assert got[4].tolist() == [[float(sum(x * z for x, z in zip(fr(A[i]), fr(B[:, j])))) for j in range(3)] for i in range(7)]
    assert float(ref.dot(a, b)) == float((a * b).sum())            # and outside such a fit they are numpy's own
    sp = _replay_spread(ref.CASES[0], exact=True)
    print(ref.case_id(ref.CASES[0]), "float64 run against its replay with exact sums:", {k: "%.3g" % v for k, v in sp.items()})
    for k, v in sp.items():
        assert v <= ref.SPREAD[k]


def test_constants_match_the_library():
    from evae import ops
    assert ops.logreg_chunk_rows() == ref.CHUNK
    assert ops.logreg_max_classes() == 256 and ops.logreg_max_features() == 256 and ops.logreg_max_points() == 1 << 20
    assert ops.logreg_max_bytes() == 1 << 30


def test_driver_refuses_what_is_out_of_scope():
    from evae.linear import LogisticRegression
    for bad in (dict(C=0.0), dict(C=-1.0), dict(C=float('inf')), dict(C=float('nan')), dict(penalty='l1'), dict(class_weight='balanced'),
                dict(warm_start=True), dict(max_iter=0), dict(history=0), dict(line_steps=0), dict(line_steps=33), dict(tol=-1.0),
                dict(check_every=0)):
        with pytest.raises(ValueError):
            LogisticRegression(**bad)
    with pytest.raises(ValueError):                               # K < 2, refused before anything touches a device
        LogisticRegression().fit(np.zeros((5, 2), np.float32), np.zeros(5, np.int64))
    with pytest.raises(ValueError):
        LogisticRegression().fit(np.zeros((5, 300), np.float32), np.arange(5))
