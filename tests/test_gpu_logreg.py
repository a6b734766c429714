"""GPU: the fp64 softmax-regression kernels (csrc/evae_logreg.hip), evae.ops.logreg_*, evae.linear.LogisticRegression and the
latent-space report, against the numpy restatement tests/logreg_ref.py (held to scikit-learn, and its case table to its margins,
by tests/test_logreg_ref_host.py).

The yardstick is always the restatement, never the code under test.  Decisions -- n_iter_, converged_, line_steps_ -- are compared
EXACTLY: the restatement's own margins (>= 1e-9 for an Armijo test, >= 1e-6 for the stop; asserted on the host for the table,
here for inputs made here) are far above fp64 rounding.  Fitted coefficients and loss_ are held to ref.SPREAD, 10 x the rounding
spread of the restatement itself (its float64 run against its replay in longdouble), relative to the largest magnitude of the
quantity.  Single launches from given inputs are held to bounds from the arithmetic, eps = 2^-52.  Both sides' rounding is allowed in
the logits alone (the leading 2 there); every other allowance is taken once:

* Logits.  z_nk takes p fused steps (d products and the intercept) on terms bounded by s_nk = sum_c |a_nc| |w_kc|:
  |dz_nk| <= 2 (p + 1) eps s_nk.
* Row loss lse(z) - z_y.  The maximum is exact; K additions of positive terms, one exp each and one log:
  (K + 4) eps (1 + |lse|).  Where the logits themselves carry an error e_n = max_k |dz_nk| (the begin launch, which computes
  Z), lse moves by at most e_n (it is 1-Lipschitz in the largest norm) and z_y by e_n: 2 e_n more.  Where Z and Z_D are GIVEN
  (the line launch), the trial logit fma(t, zd, z) equals z + t zd (t a power of two) and e_n = 0.  The rounding of the last
  subtraction, eps |loss_n|, is within the totals' term below.
* Totals of losses.  A chunk adds 1024 rows, the chunks are added in order: the rows' allowances plus
  (1024 + chunks) eps sum_n |loss_n|.  The penalty (lambda / 2)(ww + 2 t wd + t^2 dd): three dots of L terms and four
  operations: (L + 8) eps (lambda / 2)(ww + 2 t |w|.|d| + t^2 dd).
* Gradient.  r_nk = p_nk - [y_n = k]; p_nk = exp(z_nk - m) / sum moves by p_nk (2 e_n + (K + 8) eps) =: |dr_nk|, and
  |dG_kc| <= (N + 4) eps sum_n |r_nk| |a_nc| + sum_n |dr_nk| |a_nc| + 4 eps lambda |W_kc|.  The last term is the penalty's
  rounding: on either side at most one rounding of the product lambda W_kc and the share eps lambda |W_kc| of the rounding of
  the addition that the (N + 4) eps term, which bounds the sum alone, does not hold.
* Direction.  The two-loop recursion from a GIVEN history differs from the restatement's by the order of its dots only;
  it is held to ref.SPREAD['direction'], which allows for a whole fit's drift.

Every test prints the figures it asserts on; DESIGN 3.7i records the largest."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import logreg_ref as ref

pytestmark = pytest.mark.gpu

EPS = ref.EPS
ROWS = pytest.mark.parametrize("row", ref.CASES, ids=ref.case_id)
EDGES = (1, 63, 1023, 1025, 2049)                              # N at the edges of a strip and of a chunk


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return host(t).view({torch.float64: np.uint64, torch.float32: np.uint32, torch.int32: np.uint32}[t.dtype])


def logit_allowance(A, W):
    """2 (p + 1) eps sum_c |a_nc| |w_kc|, [n x K]"""
    return 2.0 * (A.shape[1] + 1) * EPS * (np.abs(A) @ np.abs(W).T)


def row_allowance(Z, y, e_n):
    """the logit error's share 2 e_n plus (K + 4) eps (1 + |lse|), [n]"""
    K = Z.shape[1]
    m = Z.max(axis=1)
    lse = m + np.log(np.exp(Z - m[:, None]).sum(axis=1))
    return 2.0 * e_n + (K + 4) * EPS * (1.0 + np.abs(lse))


# ---------------------------------------------------------------------------------------------------------------- logits
@pytest.mark.parametrize("K", [2, 3, 33, 256])
@pytest.mark.parametrize("d", [1, 40, 96, 97, 256])
def test_logits(d, K):
    from evae import ops
    rs = np.random.RandomState(1000 * d + K)
    X = rs.standard_normal((EDGES[-1], d)).astype(np.float32)
    worst = 0.0
    for fi in (True, False):
        W = rs.standard_normal((K, d + (1 if fi else 0)))
        A = ref.design(X, fi)
        want, allow = A @ W.T, logit_allowance(A, W)
        x, w = dev(X), dev(W)
        full = ops.logreg_logits(x, w, fi)
        got = host(full)
        ratio = float((np.abs(got - want) / allow).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0
        for n in EDGES[:-1]:                                    # a row's bits depend neither on N ...
            assert np.array_equal(bits(ops.logreg_logits(x[:n].contiguous(), w, fi)), bits(full[:n]))
        for o, n in ((37, 63), (1000, 100), (2048, 1)):         # ... nor on its place in the batch ...
            assert np.array_equal(bits(ops.logreg_logits(x[o:o + n].contiguous(), w, fi)), bits(full[o:o + n]))
        for i in (0, 64, 1024):                                 # ... nor on company
            assert np.array_equal(bits(ops.logreg_logits(x[i:i + 1].contiguous(), w, fi)), bits(full[i:i + 1]))
    print("logits d=%d K=%d: largest |dz| / allowance %.3g" % (d, K, worst))


# ---------------------------------------------------------------------------------------------------------------- line launch
def _line_setup(n, d, K, seed, fi, lam, scale, ascent=False):
    """a point W, its gradient, D = -scale G (or +G), and the given Z, Z_D on both sides"""
    X, y = ref.blobs(n, d, K, seed, 1.0)
    rs = np.random.RandomState(seed + 77)
    A = ref.design(X, fi)
    W = 0.3 * rs.standard_normal((K, A.shape[1]))
    Z = A @ W.T
    G = ref.gradient(A, Z, y, W, d, lam)
    D = G.copy() if ascent else -scale * G / np.abs(G).max()
    ZD = A @ D.T
    f = float(ref.in_chunks(ref.row_losses(Z, y)) + ref.penalty(W, d, lam))
    return X, y, A, W, Z, G, D, ZD, f, float((G * D).sum())


def _run_line(n, d, K, fi, lam, y, W, Z, D, ZD, f, gd, T=ref.LINE_STEPS, it=3):
    from evae import ops
    m = 4
    solver = ops.logreg_solver(d, K, fi, m, 'cuda')
    ops.logreg_views(solver, d, K, fi, m)['D'].copy_(dev(D))
    state = ops.logreg_state('cuda')
    state[0], state[3], state[7] = float(it), f, gd
    ws = ops.logreg_workspace(n, d, K, fi, T, 'cuda')
    ring = torch.full((8,), -7, dtype=torch.int32, device='cuda')
    w = dev(W)
    ops.logreg_line(dev(Z), dev(ZD), dev(y), w, d, fi, solver, m, lam, T, state, ring, ws)
    return host(w), host(state), host(ring), host(ops.logreg_workspace_views(ws, n, d, K, fi, T)['line'])


@pytest.mark.parametrize("n,d,K,fi,scale", [(63, 5, 3, True, 1.0), (1025, 8, 33, True, 40.0), (2049, 3, 2, False, 25.0),
                                            (1023, 6, 5, True, 300.0)])
def test_line_launch(n, d, K, fi, scale):
    lam, T = 0.7, ref.LINE_STEPS
    X, y, A, W, Z, G, D, ZD, f, gd = _line_setup(n, d, K, n + K, fi, lam, scale)
    trials = ref.line_trials(Z, ZD, y, W, D, d, lam, T)
    ts = 2.0 ** -np.arange(T)
    bound = f + (ref.C1 * ts) * gd
    ok = np.nonzero(trials <= bound)[0]
    assert ok.size, "the case was made to have a passing step"
    j = int(ok[0])
    margin = float((np.abs(trials[:j + 1] - bound[:j + 1]) / max(abs(f), 1.0)).min())
    assert margin >= 1e-9, "the case was made to decide clearly"
    w, state, ring, line = _run_line(n, d, K, fi, lam, y, W, Z, D, ZD, f, gd)
    chunks = (n + ref.CHUNK - 1) // ref.CHUNK
    worst = 0.0
    for jj in range(T):
        Zt = Z + ts[jj] * ZD
        rows, allow = ref.row_losses(Zt, y), row_allowance(Zt, y, 0.0)
        for c in range(chunks):
            sl = slice(c * ref.CHUNK, (c + 1) * ref.CHUNK)
            a = allow[sl].sum() + (ref.CHUNK + chunks) * EPS * np.abs(rows[sl]).sum()
            worst = max(worst, abs(line[c, jj] - rows[sl].sum()) / a)
    print("line n=%d d=%d K=%d: restatement picks j=%d (margin %.3g), device j=%d t=%g; largest chunk-sum error / allowance %.3g"
          % (n, d, K, j, margin, int(state[5]), state[4], worst))
    assert worst <= 1.0
    assert int(state[5]) == j and state[4] == ts[j] and state[1] == 0.0 and state[6] == 0.0
    assert ring[3] == j and (np.delete(ring, 3) == -7).all()
    assert np.array_equal(w.view(np.uint64), (W + ts[j] * D).view(np.uint64))     # t D is exact: one rounding on both sides
    if scale > 1.0:
        assert j > 0


def test_line_launch_ascent_direction_is_a_status():
    n, d, K, fi, lam = 1025, 8, 5, True, 0.7
    X, y, A, W, Z, G, D, ZD, f, gd = _line_setup(n, d, K, 5, fi, lam, 1.0, ascent=True)
    assert gd > 0 and not (ref.line_trials(Z, ZD, y, W, D, d, lam, ref.LINE_STEPS) <= f).any()
    w, state, ring, _ = _run_line(n, d, K, fi, lam, y, W, Z, D, ZD, f, gd)
    print("ascent direction: record", state.tolist())
    assert state[6] == 1.0 and state[1] == 1.0 and state[2] == 0.0 and state[5] == -1.0 and state[0] == 3.0
    assert np.array_equal(w.view(np.uint64), W.view(np.uint64)) and (ring == -7).all()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- gradient + finish
@pytest.mark.parametrize("n,d,K,fi", [(n, 7, 5, True) for n in EDGES] + [(1025, 40, 33, True), (2049, 96, 3, False), (700, 256, 9, True)])
def test_gradient_and_finish(n, d, K, fi):
    from evae import ops
    lam, m, T = 0.5, 4, ref.LINE_STEPS
    X, y = ref.blobs(n, d, K, 3 * n + d, 1.0)
    y = np.where(y == 1, 0, y).astype(np.int32)                  # class 1: no row carries it
    rs = np.random.RandomState(n)
    A = ref.design(X, fi)
    W = 0.3 * rs.standard_normal((K, A.shape[1]))
    Z = A @ W.T
    x, yd, w = dev(X), dev(y), dev(W)
    Zd, ZDd = torch.empty((n, K), dtype=torch.float64, device='cuda'), torch.empty((n, K), dtype=torch.float64, device='cuda')
    solver, state = ops.logreg_solver(d, K, fi, m, 'cuda'), ops.logreg_state('cuda')
    ws = ops.logreg_workspace(n, d, K, fi, T, 'cuda')
    ops.logreg_begin(x, yd, w, Zd, ZDd, fi, solver, m, lam, 0.0, T, state, ws)
    v = {k: host(t) for k, t in ops.logreg_views(solver, d, K, fi, m).items()}
    st = host(state)
    # the gradient
    e_n = logit_allowance(A, W).max(axis=1)
    R = ref.residual(Z, y)
    P = R.copy()
    P[np.arange(n), y] += 1.0
    dR = P * (2.0 * e_n[:, None] + (K + 8) * EPS)
    allow = (n + 4) * EPS * (np.abs(R).T @ np.abs(A)) + dR.T @ np.abs(A)
    allow[:, :d] += 4.0 * EPS * lam * np.abs(W[:, :d])
    G = ref.gradient(A, Z, y, W, d, lam)
    g_ratio = float((np.abs(v['G'] - G) / allow).max())
    # the loss
    rows = ref.row_losses(Z, y)
    chunks = (n + ref.CHUNK - 1) // ref.CHUNK
    f = float(ref.in_chunks(rows) + ref.penalty(W, d, lam))
    ww = float((W[:, :d] ** 2).sum())
    f_allow = row_allowance(Z, y, e_n).sum() + (ref.CHUNK + chunks) * EPS * np.abs(rows).sum() + (K * A.shape[1] + 8) * EPS * 0.5 * lam * ww
    f_ratio = abs(st[3] - f) / f_allow
    # the first direction and G.D
    D = -G / np.abs(G).max()
    d_err = ref.rel_err(v['D'], D)
    gd_allow = (G.size + 4) * EPS * np.abs(G * D).sum() + np.abs(allow * D).sum() + np.abs(G).sum() * d_err
    gd_ratio = abs(st[7] - (G * D).sum()) / gd_allow
    print("gradient n=%d d=%d K=%d: |dG| / allowance %.3g, |df| / allowance %.3g, direction relative error %.3g, |dG.D| / allowance "
          "%.3g; max|G| / N %.6g" % (n, d, K, g_ratio, f_ratio, d_err, gd_ratio, v['scal'][2]))
    assert g_ratio <= 1.0 and f_ratio <= 1.0 and gd_ratio <= 1.0 and d_err <= ref.SPREAD['direction']
    assert st[0] == 0.0 and st[1] == 0.0 and st[2] == 0.0 and st[4] == 0.0 and v['scal'][0] == 0.0
    assert np.isfinite(v['G']).all() and not (y == 1).any()
    assert np.array_equal(bits(w), W.view(np.uint64))           # begin leaves the coefficients alone


def test_labels_outside_the_classes_are_refused():
    from evae import ops, _lib
    n, d, K, fi, m, T = 100, 4, 3, True, 4, 12
    x = torch.zeros((n, d), device='cuda')
    w = torch.zeros((K, d + 1), dtype=torch.float64, device='cuda')
    Z, ZD = torch.zeros((n, K), dtype=torch.float64, device='cuda'), torch.zeros((n, K), dtype=torch.float64, device='cuda')
    solver, state = ops.logreg_solver(d, K, fi, m, 'cuda'), ops.logreg_state('cuda')
    ws = ops.logreg_workspace(n, d, K, fi, T, 'cuda')
    with _lib.count_calls("evae_logreg_") as calls:
        for bad in (K, -1):
            y = torch.zeros(n, dtype=torch.int32, device='cuda')
            y[17] = bad
            with pytest.raises(_lib.EvaeError):
                ops.logreg_begin(x, y, w, Z, ZD, fi, solver, m, 1.0, 1e-4, T, state, ws)
            with pytest.raises(_lib.EvaeError):
                ops.logreg_step(x, y, w, Z, ZD, fi, solver, m, 1.0, 1e-4, T, state, None, ws)
            with pytest.raises(_lib.EvaeError):
                ops.logreg_grad(x, y, Z, ZD, fi, T, state, ws)
            with pytest.raises(_lib.EvaeError):
                ops.logreg_line(Z, ZD, y, w, d, fi, solver, m, 1.0, T, state, None, ws)
    launched = {k: c for k, c in calls.items() if k.split("evae_logreg_")[1] in ("begin", "step", "grad", "line")}
    assert not launched, launched


def test_ops_refuse_host_tensors_and_wrong_shapes():
    from evae import ops, _lib
    x = torch.zeros((10, 4), device='cuda')
    w = torch.zeros((3, 5), dtype=torch.float64, device='cuda')
    for bad in (lambda: ops.logreg_logits(x.cpu(), w), lambda: ops.logreg_logits(x, w.cpu()), lambda: ops.logreg_logits(x, w.float()),
                lambda: ops.logreg_logits(x, w, fit_intercept=False), lambda: ops.logreg_logits(x.double(), w),
                lambda: ops.logreg_logits(x, torch.zeros((1, 5), dtype=torch.float64, device='cuda')),
                lambda: ops.logreg_logits(torch.zeros((10, 257), device='cuda'), torch.zeros((3, 258), dtype=torch.float64, device='cuda')),
                lambda: ops.logreg_softmax(torch.zeros((10, 3), dtype=torch.float64)),
                lambda: ops.logreg_softmax(torch.zeros((10, 3), device='cuda')),
                lambda: ops.logreg_solver(4, 257, True, 4, 'cuda'), lambda: ops.logreg_solver(4, 3, True, 65, 'cuda')):
        with pytest.raises(_lib.EvaeError):
            bad()
    lib = _lib.load()
    ws = ops.logreg_workspace(10, 4, 3, True, 12, 'cuda')
    Z = torch.zeros((10, 3), dtype=torch.float64, device='cuda')
    y = torch.zeros(10, dtype=torch.int32, device='cuda')
    state = ops.logreg_state('cuda')
    assert lib.evae_logreg_grad(_lib.vp(x), _lib.vp(y), 10, 4, 3, 1, 12, _lib.vp(Z), _lib.vp(Z), _lib.vp(state), _lib.vp(ws), 8, None) != 0
    assert b"workspace" in lib.evae_last_error()                 # a workspace too small is refused by the library itself
    with pytest.raises(_lib.EvaeError, match="exceed"):          # and a shape over the byte cap before any allocation, with a message
        ops.logreg_check_sizes(1 << 20, 256, 256, True, 10, 12, "LogisticRegression")


# ---------------------------------------------------------------------------------------------------------------- direction
def _history(L, count, seed):
    rs = np.random.RandomState(seed)
    pairs = []
    for _ in range(count):
        s = rs.standard_normal(L)
        yv = (0.5 + rs.random_sample(L)) * s + 0.05 * rs.standard_normal(L)
        pairs.append((s, yv, float((s * yv).sum()), float((yv * yv).sum())))
        assert pairs[-1][2] > 0
    return pairs


def _load_history(v, pairs, head, K, p):
    """pairs oldest first into the ring so that the newest sits in slot head - 1"""
    m = v['sy'].shape[0]
    for i, (s, yv, sy, yy) in enumerate(reversed(pairs)):
        slot = (head - 1 - i) % m
        v['S'][slot].copy_(dev(s.reshape(K, p)))
        v['Y'][slot].copy_(dev(yv.reshape(K, p)))
        v['sy'][slot], v['yy'][slot] = sy, yy
    v['scal'][0], v['scal'][1] = float(len(pairs)), float(head)


@pytest.mark.parametrize("name,count,head", [("empty", 0, 0), ("partly_full", 2, 2), ("full", 4, 0), ("wrapped", 4, 3), ("wrapped_once", 4, 1)])
@pytest.mark.parametrize("d,K", [(5, 3), (256, 33)])
def test_direction_from_a_given_history(name, count, head, d, K):
    from evae import ops
    m, fi = 4, True
    p = d + 1
    rs = np.random.RandomState(count + 10 * head + d)
    G = rs.standard_normal((K, p))
    pairs = _history(K * p, count, 5 + head)
    solver, state = ops.logreg_solver(d, K, fi, m, 'cuda'), ops.logreg_state('cuda')
    v = ops.logreg_views(solver, d, K, fi, m)
    v['G'].copy_(dev(G))
    _load_history(v, pairs, head, K, p)
    ops.logreg_direction(solver, d, K, fi, m, state)
    want = ref.direction(G.reshape(-1), pairs).reshape(K, p)
    err = ref.rel_err(host(v['D']), want)
    gd = float(host(state)[7])
    gd_err = abs(gd - (G * want).sum()) / np.abs(G * want).sum()
    print("direction %s d=%d K=%d: relative error %.3g (allowed %.3g), G.D %.6g relative error %.3g"
          % (name, d, K, err, ref.SPREAD['direction'], gd, gd_err))
    assert err <= ref.SPREAD['direction'] and gd_err <= ref.SPREAD['direction'] and gd < 0


@pytest.mark.parametrize("curvature", [-1.0, 1.0], ids=["s.y<=0_is_skipped", "s.y>0_is_kept"])
def test_finish_takes_or_skips_the_pair(curvature):
    """the finish launch from a given state: G_old, D, t in the solver and the record, the new gradient as the one chunk's sums"""
    from evae import ops
    n, d, K, fi, m, T, lam, t = 600, 5, 3, True, 4, ref.LINE_STEPS, 0.0, 0.5
    p = d + 1
    rs = np.random.RandomState(11)
    pairs = _history(K * p, 4, 21)
    G_old, D = rs.standard_normal((K, p)), rs.standard_normal((K, p))
    G_new = G_old + curvature * (0.7 * t * D) + 0.01 * rs.standard_normal((K, p))
    s, yv = (t * D).reshape(-1), (G_new - G_old).reshape(-1)
    sy = float((s * yv).sum())
    assert sy * curvature > 0
    solver, state = ops.logreg_solver(d, K, fi, m, 'cuda'), ops.logreg_state('cuda')
    v = ops.logreg_views(solver, d, K, fi, m)
    v['G'].copy_(dev(G_old))
    v['D'].copy_(dev(D))
    _load_history(v, pairs, 2, K, p)
    state[0], state[4] = 6.0, t
    ws = ops.logreg_workspace(n, d, K, fi, T, 'cuda')
    wv = ops.logreg_workspace_views(ws, n, d, K, fi, T)
    wv['partial'][0].copy_(dev(G_new))
    wv['loss'][0] = 123.25
    W = dev(rs.standard_normal((K, p)))
    ops.logreg_finish(n, d, W, fi, solver, m, lam, 1e-9, T, state, ws)
    kept = pairs[1:] + [(s, yv, sy, float((yv * yv).sum()))] if curvature > 0 else pairs
    want = ref.direction(G_new.reshape(-1), kept).reshape(K, p)
    err = ref.rel_err(host(v['D']), want)
    st, scal = host(state), host(v['scal'])
    print("finish, s.y = %.3g: pairs held %d, next slot %d, direction relative error %.3g, record %s" % (sy, scal[0], scal[1], err, st.tolist()))
    assert err <= ref.SPREAD['direction']
    assert scal[0] == 4.0 and scal[1] == (3.0 if curvature > 0 else 2.0)
    assert st[0] == 7.0 and st[1] == 0.0 and st[3] == 123.25 and np.array_equal(host(v['G']), G_new)
    assert abs(scal[2] - np.abs(G_new).max() / n) <= 2 * EPS * scal[2]


# ---------------------------------------------------------------------------------------------------------------- fits
def _fit(row, **kw):
    from evae.linear import LogisticRegression
    n, d, K, seed, sep, fi, C = row
    X, y, r = ref.solved(row)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return LogisticRegression(C=C, fit_intercept=fi, **kw).fit(X, y), r


@ROWS
def test_fit_matches_the_restatement(row):
    n, d, K, seed, sep, fi, C = row
    clf, r = _fit(row)
    coef, icpt = host(clf.coef_), host(clf.intercept_)
    errs = dict(coef=ref.rel_err(coef, r['W'][:, :d]), loss=ref.rel_err(clf.loss_, r['loss']))
    if fi:
        errs['intercept'] = ref.rel_err(icpt, r['W'][:, d])
    print("%s: n_iter_ %d (restatement %d), converged_ %s, line_steps_ %s | relative errors %s (allowed coef %.3g, loss %.3g)"
          % (ref.case_id(row), clf.n_iter_, r['n_iter'], clf.converged_, host(clf.line_steps_).tolist(),
             {k: "%.3g" % e for k, e in errs.items()}, ref.SPREAD['coef'], ref.SPREAD['loss']))
    assert clf.n_iter_ == r['n_iter'] and clf.converged_ is True and r['converged']
    assert clf.line_steps_.dtype == torch.int32 and host(clf.line_steps_).tolist() == r['js']
    assert errs['coef'] <= ref.SPREAD['coef'] and errs['loss'] <= ref.SPREAD['loss'] and errs.get('intercept', 0.0) <= ref.SPREAD['coef']
    assert coef.shape == (K, d) and icpt.shape == (K,) and clf.n_features_in_ == d and list(clf.classes_) == list(range(K))
    if not fi:
        assert (icpt == 0.0).all()
    again, _ = _fit(row)                                         # equal inputs: equal bits
    each, _ = _fit(row, check_every=1)                           # and however often the record is read
    for other in (again, each):
        assert np.array_equal(bits(other._W), bits(clf._W)) and other.loss_ == clf.loss_ and other.n_iter_ == clf.n_iter_
        assert np.array_equal(host(other.line_steps_), host(clf.line_steps_))


def test_fit_at_a_tight_tolerance_is_certified():
    from evae.linear import LogisticRegression
    row, tol = ref.CASES[0], 1e-7
    n, d, K, seed, sep, fi, C = row
    X, y = ref.blobs(n, d, K, seed, sep)
    r = ref.fit(X, y, K, C=C, tol=tol, fit_intercept=fi, max_iter=500)
    clf = LogisticRegression(C=C, tol=tol, max_iter=500, fit_intercept=fi).fit(X, y)
    G = ref.gradient_at(X, y, host(clf._W), C, fi)
    gn = float(np.abs(G).max() / n)
    gap = ref.top_two_gap(r['Z'])
    pred = clf.predict(X)
    differ = int(((pred != r['Z'].argmax(axis=1)) & (gap > 1e-6)).sum())
    print("tol %g: device n_iter_ %d (restatement %d), the restatement's max|G| / N at the device's coefficients %.6g; %d rows with a "
          "top-two gap <= 1e-6, %d predictions differ above it" % (tol, clf.n_iter_, r['n_iter'], gn, int((gap <= 1e-6).sum()), differ))
    assert clf.converged_ and r['converged']
    assert gn <= tol * (1.0 + 1e-3)
    assert differ == 0


# ---------------------------------------------------------------------------------------------------------------- decisions
def test_probabilities_and_ties():
    from evae import ops
    from evae.linear import LogisticRegression
    row = ref.CASES[2]
    n, d, K, seed, sep, fi, C = row
    X, y, r = ref.solved(row)
    labels = np.array([10 * k - 30 for k in range(K)])           # classes_ are the sorted labels, not 0 .. K-1
    clf = LogisticRegression(C=C, fit_intercept=fi).fit(X, labels[y])
    assert list(clf.classes_) == sorted(labels) and np.array_equal(bits(clf._W), bits(_fit(row)[0]._W))
    proba, logp, dec = host(clf.predict_proba(X)), host(clf.predict_log_proba(X)), host(clf.decision_function(X))
    off = float(np.abs(proba.sum(axis=1) - 1.0).max())
    want = dec - dec.max(axis=1, keepdims=True)
    want = want - np.log(np.exp(want).sum(axis=1, keepdims=True))
    lp_err = float((np.abs(logp - want) / (1.0 + np.abs(want))).max())
    print("predict_proba: largest |row sum - 1| %.3g (allowed %.3g); predict_log_proba against numpy on the device's logits %.3g; "
          "accuracy %.4f" % (off, (K + 4) * EPS, lp_err, clf.score(X, labels[y])))
    assert off <= (K + 4) * EPS and (proba >= 0).all() and lp_err <= 2 * (K + 4) * EPS
    assert np.array_equal(clf.predict(X), labels[dec.argmax(axis=1)]) and clf.score(X, labels[y]) == float((clf.predict(X) == labels[y]).mean())
    Z = np.zeros((6, 4))
    Z[1] = [1, 3, 3, 2]
    Z[2] = [5, 5, 5, 5]
    Z[3] = [-1, -2, -1, -3]
    Z[4] = [0, 1, 2, 2]
    Z[5] = [7, 0, 0, 7]
    _, lab = ops.logreg_softmax(dev(Z))
    assert host(lab).tolist() == [0, 1, 0, 0, 2, 0]             # ties go to the lowest class


def test_max_iter_reached_warns():
    from evae.linear import LogisticRegression
    row = ref.CASES[0]
    n, d, K, seed, sep, fi, C = row
    X, y, r = ref.solved(row)
    with pytest.warns(RuntimeWarning, match="max_iter=3"):
        clf = LogisticRegression(C=C, fit_intercept=fi, max_iter=3, check_every=2).fit(X, y)
    assert clf.converged_ is False and clf.n_iter_ == 3 and host(clf.line_steps_).tolist() == r['js'][:3]
    short = ref.fit(X, y, K, C=C, fit_intercept=fi, max_iter=3)
    err = ref.rel_err(host(clf._W), short['W'])
    print("three iterations: relative error of the coefficients %.3g" % err)
    assert err <= ref.SPREAD['coef']


def test_a_gradient_that_is_not_finite_is_a_status_of_its_own():
    from evae.linear import LogisticRegression
    row = ref.CASES[0]
    n, d, K, seed, sep, fi, C = row
    X, y, r = ref.solved(row)
    X = X.copy()
    X[7, 2] = np.nan
    with pytest.warns(RuntimeWarning, match="not finite") as caught:
        clf = LogisticRegression(C=C, fit_intercept=fi).fit(X, y)
    print("an entry of X not a number: n_iter_ %d, converged_ %s, loss_ %s; %s" % (clf.n_iter_, clf.converged_, clf.loss_, caught[0].message))
    assert clf.converged_ is False and clf.n_iter_ == 0 and len(caught) == 1 and "max_iter" not in str(caught[0].message)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the report
def test_report_on_a_stub_model(tmp_path, capsys):
    import evae_oracle as orc
    import smoke_case
    import golden_inputs as gi
    from utils.linear_probe_on_latent import report_linear_probe_on_latent
    B = 32
    args = smoke_case.vae_args(number_components=20, training_set_size=100, batch_size=B)
    args.probe_C, args.probe_max_iter, args.probe_tol = 0.5, 200, 1e-4
    model, _ = smoke_case.build_model(torch, np, orc, args)
    model.eval()

    def loader(seed, n):
        data = torch.from_numpy(gi.binary_images(seed, n))
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, (torch.arange(n) * 7) % 10), batch_size=B, shuffle=False)

    out = str(tmp_path / "probe")
    for val, n_train, n_test in ((True, 128, 64), (False, 192, 96)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            clf = report_linear_probe_on_latent(loader(91, 130), loader(92, 75), loader(93, 100), model, out, args, val=val)
        assert "linear probe on" in capsys.readouterr().out
        assert sorted(os.listdir(out)) == ["linear_probe.json", "linear_probe_coef.npy", "linear_probe_test_predictions.npy"]
        result = json.load(open(os.path.join(out, "linear_probe.json")))
        assert sorted(result) == sorted(["train_accuracy", "test_accuracy", "test_log_loss", "n_iter", "converged", "loss", "C", "classes",
                                         "n_train", "n_test", "confusion"])
        coef = np.load(os.path.join(out, "linear_probe_coef.npy"))
        saved = np.load(os.path.join(out, "linear_probe_test_predictions.npy"))
        truth = ((np.arange(75 if val else 100) * 7) % 10)[:n_test]
        confusion = np.array(result["confusion"])
        print("report val=%s: %s" % (val, {k: result[k] for k in ("train_accuracy", "test_accuracy", "test_log_loss", "n_iter", "converged")}))
        assert result["n_train"] == n_train and result["n_test"] == n_test and result["n_iter"] == clf.n_iter_ and result["C"] == 0.5
        assert coef.shape == (10, clf.n_features_in_ + 1) and coef.dtype == np.float64 and saved.shape == (n_test,)
        assert confusion.shape == (10, 10) and confusion.sum() == n_test
        assert result["test_accuracy"] == float((saved == truth).mean()) and np.trace(confusion) == int((saved == truth).sum())
        assert np.isfinite(result["test_log_loss"]) and result["test_log_loss"] > 0
