"""Times evae.linear on the device and writes profiles/linear_probe.json (the protocol of tools/gmm_bench.py):

    python tools/linear_probe_bench.py [--runs 3 --reps 30 --out profiles/linear_probe.json] [--no-sklearn]

* THE ONE BAR: one L-BFGS iteration -- ops.logreg_step: the logits of the direction, the line launch with its 12 trial losses,
  the gradient, the finish; four launches -- under device events against the same arithmetic from torch operators in float64 on
  the same GPU (a matmul for Z_D, logsumexp over the 12 trial logits, the axpy on Z, a softmax, a matmul for the gradient),
  at (N, d, K) = (60 000, 40, 10) and (10 000, 40, 10) on tsne_bench's latents, from the state after three iterations.  The
  baseline's trial losses and gradient are checked against the kernels' first (relative differences recorded, <= 1e-10).  The
  two-loop recursion is NOT in the baseline: it does less.  Both are alternated in one session: --runs rounds, in each the mean
  over --reps iterations (an event pair around every iteration; W, Z, the solver and the record are put back outside the pair,
  so every iteration does the same work and none meets the done flag); median of the rounds with max - min.  The bar is met
  where the kernels are faster by more than the larger spread; recorded either way.  The baseline is the torch formulation,
  never an earlier build of this code.
* for information: whole LogisticRegression().fit calls at both sizes (host clock around a synchronised call, median of --runs
  with max - min) with the iterations each ran; ONE scikit-learn LogisticRegression fit on the host if scikit-learn imports
  (threads limited to 16).
Nothing here runs under a profiler."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tsne_bench import latents      # noqa: E402

SHAPES = ((60000, 40, 10), (10000, 40, 10))
C, TOL, HISTORY, LINE_STEPS, WARM_ITERATIONS = 1.0, 1e-4, 10, 12, 3


def spread(runs, clock):
    return {"runs": runs, "median": statistics.median(runs), "max_minus_min": max(runs) - min(runs), "clock": clock}


def time_sklearn(X, y):
    try:
        import sklearn
        from sklearn.linear_model import LogisticRegression as SkLogisticRegression
    except Exception as e:                                   # noqa: BLE001
        return {"timed": False, "reason": "scikit-learn does not import here: %r" % (e,)}
    limit = None
    try:
        from threadpoolctl import threadpool_limits
        limit = threadpool_limits(limits=16)
    except Exception:                                        # noqa: BLE001
        pass
    try:
        t0 = time.perf_counter()
        clf = SkLogisticRegression(C=C, tol=TOL, max_iter=1000).fit(X.astype("float64"), y)
        return {"timed": True, "fit_seconds": time.perf_counter() - t0, "n_iter": int(clf.n_iter_[0]),
                "train_accuracy": float(clf.score(X.astype("float64"), y)), "runs": 1, "threads": 16 if limit is not None else None,
                "version": sklearn.__version__, "note": "its L-BFGS has another line search and another stop: another iteration count"}
    finally:
        if limit is not None:
            limit.restore_original_limits()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_probe.json"))
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    from evae import ops
    from evae.linear import LogisticRegression

    if not torch.cuda.is_available():
        raise SystemExit("linear_probe_bench: no GPU; nothing is measured without one")

    def timed(prepare, fn, reps):
        """mean seconds of fn over reps, an event pair around each call; prepare() runs outside the pair"""
        total = 0.0
        for _ in range(reps):
            prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            total += e0.elapsed_time(e1) * 1e-3
        return total / reps

    res = {"device": torch.cuda.get_device_name(0), "one_iteration": {}, "fit": {}}
    clock = "device events around each of %d iterations, their mean; one value per round" % a.reps
    lam, fi, m, T = 1.0 / C, True, HISTORY, LINE_STEPS
    for n, d, K in SHAPES:
        X = latents(n, d)
        yh = (np.arange(n) % K).astype(np.int32)
        x, y = torch.from_numpy(X).cuda(), torch.from_numpy(yh).cuda()
        f64 = dict(dtype=torch.float64, device="cuda")
        W, Z, ZD = torch.zeros((K, d + 1), **f64), torch.empty((n, K), **f64), torch.empty((n, K), **f64)
        solver, state = ops.logreg_solver(d, K, fi, m, "cuda"), ops.logreg_state("cuda")
        ws = ops.logreg_workspace(n, d, K, fi, T, "cuda")
        ops.logreg_begin(x, y, W, Z, ZD, fi, solver, m, lam, TOL, T, state, ws)
        for _ in range(WARM_ITERATIONS):
            ops.logreg_step(x, y, W, Z, ZD, fi, solver, m, lam, TOL, T, state, None, ws, labels_checked=True)
        assert state.cpu()[1] == 0.0 and state.cpu()[0] == WARM_ITERATIONS
        W0, Z0, solver0, state0 = W.clone(), Z.clone(), solver.clone(), state.clone()
        views = ops.logreg_views(solver0, d, K, fi, m)
        D0 = views["D"].clone()
        a64 = torch.cat((x.double(), torch.ones((n, 1), **f64)), dim=1)
        onehot = torch.zeros((n, K), **f64)
        onehot[torch.arange(n, device="cuda"), y.long()] = 1.0
        ts = torch.tensor([2.0 ** -j for j in range(T)], **f64)
        yl = y.long()
        step = [1.0]

        def put_back():
            W.copy_(W0)
            Z.copy_(Z0)
            solver.copy_(solver0)
            state.copy_(state0)

        def candidate():
            ops.logreg_step(x, y, W, Z, ZD, fi, solver, m, lam, TOL, T, state, None, ws, labels_checked=True)

        def baseline():
            zd = a64 @ D0.t()                                                       # [n x K]
            trial = Z0.unsqueeze(0) + ts[:, None, None] * zd.unsqueeze(0)           # [T x n x K]
            losses = (torch.logsumexp(trial, dim=2) - trial.gather(2, yl.expand(T, n).unsqueeze(2)).squeeze(2)).sum(dim=1)
            z1 = Z0 + step[0] * zd                                                  # the step the kernels take from this state
            r = torch.softmax(z1, dim=1) - onehot
            g = r.t() @ a64
            g[:, :d] += lam * (W0 + step[0] * D0)[:, :d]
            return losses, g

        for fn in (candidate, baseline):                          # warm-up: code objects, allocator pools
            put_back()
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        put_back()
        candidate()
        rec = state.cpu()
        assert rec[1] == 0.0 and rec[5] >= 0.0, "the search from the benchmark's state must pass (record %r)" % (rec.tolist(),)
        step[0] = float(rec[4])
        got_lines = ops.logreg_workspace_views(ws, n, d, K, fi, T)["line"].sum(dim=0)
        got_g = ops.logreg_views(solver, d, K, fi, m)["G"]
        losses, g = baseline()
        apart = {"trial_losses": float(((losses - got_lines).abs() / losses.abs()).max()),
                 "gradient": float((g - got_g).abs().max() / g.abs().max())}
        assert max(apart.values()) <= 1e-10, apart
        variants = {"candidate": (put_back, candidate), "torch_float64": (lambda: None, baseline)}
        runs = {name: [] for name in variants}
        for _ in range(a.runs):                                   # alternated
            for name, (prep, fn) in variants.items():
                runs[name].append(timed(prep, fn, a.reps))
        cand, base = spread(runs["candidate"], clock), spread(runs["torch_float64"], clock)
        larger = max(cand["max_minus_min"], base["max_minus_min"])
        res["one_iteration"]["N=%d d=%d K=%d" % (n, d, K)] = {
            "candidate_seconds": cand, "torch_float64_seconds": base, "torch_float64_apart_from_candidate": apart,
            "bar": "candidate.median + max(candidate.max_minus_min, torch_float64.max_minus_min) < torch_float64.median",
            "bar_met": bool(cand["median"] + larger < base["median"]), "ratio_of_medians": cand["median"] / base["median"],
        }
        del a64, onehot, Z0, W0, solver0
        torch.cuda.empty_cache()

        host_clock = "host perf_counter around a synchronised call"
        LogisticRegression(C=C).fit(x, yh)                        # warm-up
        torch.cuda.synchronize()
        fits, iters = [], []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            clf = LogisticRegression(C=C).fit(x, yh)
            torch.cuda.synchronize()
            fits.append(time.perf_counter() - t0)
            iters.append(clf.n_iter_)
        res["fit"]["N=%d d=%d K=%d" % (n, d, K)] = {
            "fit_seconds": spread(fits, host_clock + " (labels from the host, tol 1e-4, check_every 10)"), "n_iter": iters,
            "converged": bool(clf.converged_), "train_accuracy": clf.score(x, yh), "loss": clf.loss_,
            "scikit_learn": {"timed": False, "reason": "--no-sklearn"} if a.no_sklearn or n != SHAPES[0][0] else time_sklearn(X, yh),
        }
    res["not_measured"] = ["kernel times under a profiler", "hardware counters", "the four launches of an iteration one by one",
                           "N other than 60 000 and 10 000", "d other than 40", "K other than 10", "history other than 10",
                           "decision_function, predict_proba and predict alone", "more than one scikit-learn run (no spread for it)",
                           "the two-loop recursion in the torch baseline (the kernels' side includes it)"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
