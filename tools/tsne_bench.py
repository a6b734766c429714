"""Times evae.tsne.TSNE on the device and writes profiles/tsne.json:

    python tools/tsne_bench.py [--n 10000 --zd 40 --iters 1000 --runs 3 --out profiles/tsne.json] [--no-sklearn]

* whole fit_transform calls (host clock around a synchronised call): median of --runs, with max - min;
* the affinity stage (distances + row search + symmetrising) and one iteration (forces + update, mean of 50 in stream order),
  each between device events after a warm-up;
* the bytes and operations of both, computed from the shapes, and the rates they imply;
* scikit-learn's TSNE(n_components=2) ONCE on the same array if it imports (its default method, Barnes-Hut, an approximation;
  threads limited to 16) -- or the reason it was not timed.
Nothing here runs under a profiler."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))

PAIR_OPS = 22      # forces, per ordered pair: 2 sub, 3 for q, 1 reciprocal, 2 mul, 4 products, 5 conversions + 5 fp64 adds


def latents(n, zd, seed=0, classes=10):
    rs = np.random.RandomState(seed)
    means = rs.randn(classes, zd) * 1.5
    return (means[np.arange(n) % classes] + rs.randn(n, zd)).astype(np.float32)


def shape_counts(n, zd, search_steps):
    pairs = n * (n - 1)
    return {
        "affinities": {
            "bytes": 4 * n * n * 5 + 2 * 4 * n * zd,          # distances written; read + conditionals written; both read + P written
            "exponentials_fp64": pairs * (search_steps + 2),
            "distance_flops_fp64": 3 * n * n * zd,
        },
        "iteration": {
            "bytes": 4 * n * n + 64 * n + 8 * n + 3 * 2 * 8 * n,   # P once; per-point sums; Y; Y / velocity / gains read + written
            "pair_ops": PAIR_OPS * n * n,
            "reciprocals": n * n,
            "launches": 2,
        },
    }


def time_sklearn(X, iters):
    try:
        import sklearn
        from sklearn.manifold import TSNE as SkTSNE
    except Exception as e:                                   # noqa: BLE001
        return {"timed": False, "reason": "scikit-learn does not import here: %r" % (e,)}
    import inspect
    kw = {"n_components": 2, "random_state": 0}
    kw["max_iter" if "max_iter" in inspect.signature(SkTSNE.__init__).parameters else "n_iter"] = iters
    limit = None
    try:
        from threadpoolctl import threadpool_limits
        limit = threadpool_limits(limits=16)
    except Exception:                                        # noqa: BLE001
        pass
    try:
        est = SkTSNE(n_jobs=16, **kw)
        t0 = time.perf_counter()
        est.fit_transform(X)
        dt = time.perf_counter() - t0
    finally:
        if limit is not None:
            limit.restore_original_limits()
    return {"timed": True, "seconds": dt, "runs": 1, "method": est.method, "approximation": est.method != "exact",
            "angle": est.angle, "n_iter_run": int(est.n_iter_), "kl_divergence": float(est.kl_divergence_),
            "threads": 16, "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS"), "version": sklearn.__version__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--zd", type=int, default=40)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne.json"))
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()

    import torch
    from evae import ops
    from evae.tsne import TSNE
    X = latents(a.n, a.zd)
    Xd = torch.from_numpy(X).cuda()
    TSNE(perplexity=a.perplexity, n_iter=20, random_state=0).fit_transform(Xd)       # warm-up: code objects, allocator pools
    torch.cuda.synchronize()

    whole, kls = [], []
    for r in range(a.runs):
        t = TSNE(perplexity=a.perplexity, n_iter=a.iters, random_state=r)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Y = t.fit_transform(Xd)
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
        kls.append(t.kl_divergence_)
        assert bool(torch.isfinite(Y).all())

    def events(fn, reps):
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3)
        return out

    aff = events(lambda: ops.tsne_affinities(Xd, a.perplexity), 3)
    P, _ = ops.tsne_affinities(Xd, a.perplexity)
    Yd = torch.randn(a.n, 2, device="cuda") * 1e-4
    vel, gains = torch.zeros_like(Yd), torch.ones_like(Yd)
    lr = max(a.n / 12.0 / 4.0, 50.0)
    STEPS = 50

    def iterate():
        for _ in range(STEPS):
            ops.tsne_update(ops.tsne_forces(P, Yd, 1.0, False), Yd, vel, gains, 0.8, lr)
    iterate()
    its = [t / STEPS for t in events(iterate, 3)]

    counts = shape_counts(a.n, a.zd, ops.TSNE_SEARCH_STEPS)
    aff_med, it_med = statistics.median(aff), statistics.median(its)
    res = {
        "what": "exact t-SNE, evae.tsne.TSNE.fit_transform, N=%d zd=%d perplexity=%g n_iter=%d" % (a.n, a.zd, a.perplexity, a.iters),
        "device": torch.cuda.get_device_name(0),
        "fit_transform_seconds": {"runs": whole, "median": statistics.median(whole), "max_minus_min": max(whole) - min(whole),
                                  "clock": "host perf_counter around a synchronised call"},
        "kl_divergence": kls,
        "affinity_stage_seconds": {"runs": aff, "median": aff_med, "max_minus_min": max(aff) - min(aff), "clock": "device events"},
        "iteration_seconds": {"runs": its, "median": it_med, "max_minus_min": max(its) - min(its),
                              "clock": "device events around %d iterations in stream order, divided by %d" % (STEPS, STEPS)},
        "shape_derived": counts,
        "implied_rates": {
            "affinities_fp64_exponentials_per_s": counts["affinities"]["exponentials_fp64"] / aff_med,
            "iteration_bytes_per_s": counts["iteration"]["bytes"] / it_med,
            "iteration_pair_ops_per_s": counts["iteration"]["pair_ops"] / it_med,
        },
        "scikit_learn": ({"timed": False, "reason": "--no-sklearn"} if a.no_sklearn else time_sklearn(X, a.iters)),
        "not_measured": ["kernel times under a profiler", "hardware counters (bytes actually moved, occupancy)",
                         "N other than %d" % a.n, "scikit-learn's method='exact' (O(N^2) on the host; not attempted at this N)",
                         "more than one scikit-learn run (no spread for it)"],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("fit_transform_seconds", "affinity_stage_seconds", "iteration_seconds", "scikit_learn")}))


if __name__ == "__main__":
    main()
