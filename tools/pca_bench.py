"""Times evae.pca.PCA and TSNE(init='pca') on the device and writes profiles/pca.json (the protocol of tools/tsne_bench.py):

    python tools/pca_bench.py [--runs 3 --iters 1000 --out profiles/pca.json] [--no-sklearn]

* PCA().fit at (N, d) = (10 000, 40), (60 000, 40), (10 000, 256) on tsne_bench's latents: whole calls (host clock around a
  synchronised call), median of --runs with max - min; the stages -- moments, eigen-solver, projection on 2 and on d components --
  each between device events after a warm-up, with the sweeps the solver ran;
* TSNE.fit_transform at N = 10 000, d = 40 with init='random' and init='pca' alternated in one session, under both methods, and the
  affinity stage of each method by device events in that session.  THE ONE BAR: median(init='pca') - median(init='random') stays
  below the median of the affinity stage of the same method.  The file says whether it held;
* scikit-learn's PCA(svd_solver='full') once per shape on the host if it imports (threads limited to 16).
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tsne_bench import latents      # noqa: E402

SHAPES = ((10000, 40), (60000, 40), (10000, 256))


def spread(runs, clock):
    return {"runs": runs, "median": statistics.median(runs), "max_minus_min": max(runs) - min(runs), "clock": clock}


def time_sklearn(X):
    try:
        import sklearn
        from sklearn.decomposition import PCA as SkPCA
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
        SkPCA(svd_solver='full').fit(X)
        dt = time.perf_counter() - t0
    finally:
        if limit is not None:
            limit.restore_original_limits()
    return {"timed": True, "seconds": dt, "runs": 1, "svd_solver": "full", "threads": 16, "version": sklearn.__version__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca.json"))
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()

    import torch
    from evae import ops
    from evae.pca import PCA
    from evae.tsne import TSNE

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

    res = {"device": torch.cuda.get_device_name(0), "pca_fit": {}}
    for n, d in SHAPES:
        X = latents(n, d)
        Xd = torch.from_numpy(X).cuda()
        pca = PCA().fit(Xd)                                      # warm-up: code objects, allocator pools
        torch.cuda.synchronize()
        whole = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            PCA().fit(Xd)
            torch.cuda.synchronize()
            whole.append(time.perf_counter() - t0)
        mean, cov = ops.pca_moments(Xd)
        two = pca.components_[:2].contiguous()
        res["pca_fit"]["N=%d d=%d" % (n, d)] = {
            "fit_seconds": spread(whole, "host perf_counter around a synchronised call (moments, eigen-solver, one read of d + 4 doubles)"),
            "moments_seconds": spread(events(lambda: ops.pca_moments(Xd), a.runs), "device events"),
            "eigen_solver_seconds": spread(events(lambda: ops.pca_eigh(cov), a.runs), "device events"),
            "project_2_seconds": spread(events(lambda: ops.pca_project(Xd, mean, two), a.runs), "device events"),
            "project_d_seconds": spread(events(lambda: ops.pca_project(Xd, mean, pca.components_), a.runs), "device events"),
            "sweeps": pca.n_sweeps_, "sweep_bound": ops.pca_max_sweeps(),
            "matrices_in": "LDS" if d <= 96 else "workspace (global memory)",
            "explained_variance_ratio_first_two": [float(v) for v in pca.explained_variance_ratio_[:2].cpu()],
            "scikit_learn": {"timed": False, "reason": "--no-sklearn"} if a.no_sklearn else time_sklearn(X),
        }
        del Xd, pca, mean, cov, two

    n, d = SHAPES[0]
    Xd = torch.from_numpy(latents(n, d)).cuda()
    methods, inits = ("exact", "neighbours"), ("random", "pca")
    for m in methods:
        for i in inits:
            TSNE(perplexity=a.perplexity, n_iter=20, random_state=0, method=m, init=i).fit_transform(Xd)
    torch.cuda.synchronize()
    whole = {(m, i): [] for m in methods for i in inits}
    for r in range(a.runs):
        for m in methods:
            for i in inits:                                      # alternated: random, pca, random, ...
                t = TSNE(perplexity=a.perplexity, n_iter=a.iters, random_state=r, method=m, init=i)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                Y = t.fit_transform(Xd)
                torch.cuda.synchronize()
                whole[(m, i)].append(time.perf_counter() - t0)
                assert bool(torch.isfinite(Y).all())
                del Y, t
    clock = "host perf_counter around a synchronised call"
    res["tsne_init"] = {"what": "TSNE.fit_transform, N=%d zd=%d perplexity=%g n_iter=%d; random and pca alternated, %d rounds"
                                % (n, d, a.perplexity, a.iters, a.runs)}
    for m in methods:
        stage = (lambda: ops.tsne_nn_affinities(Xd, a.perplexity)) if m == "neighbours" else (lambda: ops.tsne_affinities(Xd, a.perplexity))
        stage()
        aff = spread(events(stage, a.runs), "device events")
        init_alone = spread(events(lambda: TSNE(init='pca')._initial(n, Xd.device, Xd), a.runs),
                            "device events around PCA(2).fit + projection, the read of the record included")
        added = statistics.median(whole[(m, "pca")]) - statistics.median(whole[(m, "random")])
        res["tsne_init"][m] = {
            "fit_transform_seconds": {i: spread(whole[(m, i)], clock) for i in inits},
            "affinity_stage_seconds": aff,
            "initial_state_alone_seconds": init_alone,
            "added_by_init_pca_seconds": added,
            "bar": "added_by_init_pca_seconds < affinity_stage_seconds.median",
            "bar_met": bool(added < aff["median"]),
        }
    res["not_measured"] = ["kernel times under a profiler", "hardware counters", "N above 60 000", "d between 40 and 256",
                           "more than one scikit-learn run (no spread for it)"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
