"""Times evae.mixture on the device and writes profiles/gmm.json (the protocol of tools/kmeans_bench.py):

    python tools/gmm_bench.py [--runs 3 --reps 30 --out profiles/gmm.json] [--no-sklearn]

* THE ONE BAR: one EM iteration -- ops.gmm_step: E-step, the two passes of the M-step, the finish, the record; six launches --
  under device events against the same arithmetic from torch operators in float64 on the same GPU (a batched product with the
  triangular factors, logsumexp, a matrix product for the means, an einsum for the weighted scatter about the new means,
  linalg.cholesky and solve_triangular), at (N, d, K) = (60 000, 40, 10), 'full', on tsne_bench's latents from a k-means start.
  The baseline's outputs are checked against the kernel's first (log_resp, means, covariances, factors; the differences are
  recorded and must stay below 1e-9).  Both are alternated in one session: --runs rounds, in each the mean over --reps iterations
  (an event pair around every iteration; the parameters are put back and the record is zeroed outside the pair, so no iteration
  meets the done flag; a variant that takes longer than --budget seconds per round gets fewer iterations, 3 at the least);
  median of the rounds with max - min.  Expected: the kernel ahead by more than the baseline's spread; recorded either way.
  The baseline is the torch formulation, never an earlier build of this code.
* for information: 'diag' at the same size and 'full' at (60 000, 40, 100) in the same way; whole GaussianMixture(10).fit calls
  (k-means start, tol 1e-3; host clock around a synchronised call, median of --runs with max - min) with the iterations each
  ran; ONE scikit-learn GaussianMixture(10).fit on the host if scikit-learn imports (threads limited to 16).
Nothing here runs under a profiler."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tsne_bench import latents      # noqa: E402

SHAPES = ((60000, 40, 10, 'full', True), (60000, 40, 10, 'diag', False), (60000, 40, 100, 'full', False))
REG, TOL = 1e-6, 1e-3


def spread(runs, clock):
    return {"runs": runs, "median": statistics.median(runs), "max_minus_min": max(runs) - min(runs), "clock": clock}


def time_sklearn(X, K):
    try:
        import sklearn
        from sklearn.mixture import GaussianMixture as SkGaussianMixture
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
        gm = SkGaussianMixture(K, random_state=0).fit(X.astype("float64"))
        return {"timed": True, "fit_seconds": time.perf_counter() - t0, "n_iter": int(gm.n_iter_), "lower_bound": float(gm.lower_bound_),
                "converged": bool(gm.converged_), "runs": 1, "threads": 16 if limit is not None else None,
                "version": sklearn.__version__,
                "note": "its k-means start has its own random stream: another local maximum, another iteration count"}
    finally:
        if limit is not None:
            limit.restore_original_limits()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--budget", type=float, default=4.0, help="seconds of device time a variant may take per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm.json"))
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()

    import torch
    from evae import ops
    from evae.cluster import KMeans
    from evae.mixture import GaussianMixture

    if not torch.cuda.is_available():
        raise SystemExit("gmm_bench: no GPU; nothing is measured without one")

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

    res = {"device": torch.cuda.get_device_name(0), "one_em_iteration": {}, "fit": {}}
    clock = "device events around each of %d iterations, their mean; one value per round"
    for n, d, K, ctype, is_bar in SHAPES:
        x = torch.from_numpy(latents(n, d)).cuda()
        x64 = x.double()
        labels = KMeans(K, n_init=1, random_state=0).fit(x).labels_
        p0 = ops.gmm_params(d, K, ctype, x.device)
        state, ws = ops.gmm_state(x.device), ops.gmm_workspace(n, d, K, ctype, x.device)
        ops.gmm_mstep(x, p0, K, ctype, REG, state, labels=labels, ws=ws)
        assert state.cpu()[5] == -1.0
        params = p0.clone()
        log_resp = torch.empty((n, K), dtype=torch.float64, device="cuda")
        logp = torch.empty(n, dtype=torch.float64, device="cuda")
        v0 = {k: t.clone() for k, t in ops.gmm_views(p0, d, K, ctype).items()}
        eye = torch.eye(d, dtype=torch.float64, device="cuda")
        half_d_log_2pi = 0.5 * d * math.log(2.0 * math.pi)

        def put_back():
            params.copy_(p0)
            state.zero_()

        def candidate():
            ops.gmm_step(x, params, K, ctype, log_resp, logp, REG, TOL, state, ws)

        def baseline():
            w, mu, P, ld = v0["weights"], v0["means"], v0["precisions_cholesky"], v0["log_det"]
            if ctype == 'full':
                y = torch.matmul(x64.unsqueeze(0), P) - torch.matmul(mu.unsqueeze(1), P)          # [K x N x d]
            else:
                y = x64.unsqueeze(0) * P.unsqueeze(1) - (mu * P).unsqueeze(1)
            lp = (-0.5 * (y * y).sum(dim=2) - half_d_log_2pi).t() + ld + torch.log(w)
            lse = torch.logsumexp(lp, dim=1)
            lr = lp - lse[:, None]
            bound = lse.mean()
            r = lr.exp()
            nk = r.sum(dim=0) + 10.0 * 2.0 ** -52
            mu2 = (r.t() @ x64) / nk[:, None]
            df = x64.unsqueeze(0) - mu2.unsqueeze(1)                                              # [K x N x d]
            if ctype == 'full':
                cov = torch.einsum('nk,knd,kne->kde', r, df, df) / nk[:, None, None] + REG * eye
                P2 = torch.linalg.solve_triangular(torch.linalg.cholesky(cov), eye.expand(K, d, d), upper=False).transpose(1, 2)
            else:
                cov = torch.einsum('nk,knd->kd', r, df * df) / nk[:, None] + REG
                P2 = cov.rsqrt()
            return lr, mu2, cov, P2, nk / nk.sum(), bound

        for fn in (candidate, baseline):                          # warm-up: code objects, allocator pools
            put_back()
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        put_back()
        candidate()
        got = ops.gmm_views(params, d, K, ctype)
        lr, mu2, cov, P2, w2, bound = baseline()
        apart = {"log_resp": float((lr - log_resp).abs().max()), "means": float((mu2 - got["means"]).abs().max()),
                 "covariances": float((cov - got["covariances"]).abs().max()),
                 "precisions_cholesky": float((P2 - got["precisions_cholesky"]).abs().max()),
                 "weights": float((w2 - got["weights"]).abs().max()), "lower_bound": abs(float(bound) - float(state.cpu()[3]))}
        assert max(apart.values()) <= 1e-9, apart
        del lr, mu2, cov, P2, w2
        variants = {"candidate": (put_back, candidate), "torch_float64": (lambda: None, baseline)}
        reps = {name: max(3, min(a.reps, int(a.budget / max(timed(prep, fn, 1), 1e-9)))) for name, (prep, fn) in variants.items()}
        runs = {name: [] for name in variants}
        for _ in range(a.runs):                                   # alternated
            for name, (prep, fn) in variants.items():
                runs[name].append(timed(prep, fn, reps[name]))
        cand, base = spread(runs["candidate"], clock % reps["candidate"]), spread(runs["torch_float64"], clock % reps["torch_float64"])
        res["one_em_iteration"]["N=%d d=%d K=%d %s" % (n, d, K, ctype)] = {
            "is_the_bar": is_bar, "candidate_seconds": cand, "torch_float64_seconds": base, "torch_float64_apart_from_candidate": apart,
            "bar": "candidate.median + torch_float64.max_minus_min < torch_float64.median",
            "bar_met": bool(cand["median"] + base["max_minus_min"] < base["median"]),
            "ratio_of_medians": cand["median"] / base["median"],
        }
        del x64, params, p0, log_resp, logp, ws, v0
        torch.cuda.empty_cache()

    host_clock = "host perf_counter around a synchronised call"
    n, d, K = 60000, 40, 10
    X = latents(n, d)
    x = torch.from_numpy(X).cuda()
    GaussianMixture(K, random_state=0).fit(x)                     # warm-up
    torch.cuda.synchronize()
    fits, iters, bounds = [], [], []
    for r in range(a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gm = GaussianMixture(K, random_state=r).fit(x)
        torch.cuda.synchronize()
        fits.append(time.perf_counter() - t0)
        iters.append(gm.n_iter_)
        bounds.append(gm.lower_bound_)
    res["fit"]["N=%d d=%d K=%d full" % (n, d, K)] = {
        "fit_seconds": spread(fits, host_clock + " (k-means start included, one run, tol 1e-3, check_every 4)"), "n_iter": iters,
        "lower_bound": bounds,
        "scikit_learn": {"timed": False, "reason": "--no-sklearn"} if a.no_sklearn else time_sklearn(X, K),
    }
    res["not_measured"] = ["kernel times under a profiler", "hardware counters", "the launches of an iteration one by one",
                           "N other than 60 000", "d other than 40", "'spherical'", "K other than 10 and 100",
                           "score_samples, predict and sample alone", "more than one scikit-learn run (no spread for it)"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
