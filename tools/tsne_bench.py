"""Times evae.tsne.TSNE on the device and writes profiles/tsne.json:

    python tools/tsne_bench.py [--n 10000 --zd 40 --iters 1000 --runs 3 --out profiles/tsne.json] [--no-sklearn]
    python tools/tsne_bench.py --method both --no-sklearn          # 'exact' and 'neighbours' alternated -> profiles/tsne_nn.json
    python tools/tsne_bench.py --method neighbours --n 60000 --no-sklearn --out profiles/tsne_nn_60000.json

* whole fit_transform calls (host clock around a synchronised call): median of --runs, with max - min;
* the affinity stage (distances + row search + symmetrising) and one iteration (forces + update, mean of 50 in stream order),
  each between device events after a warm-up;
* the bytes and operations of both, computed from the shapes, and the rates they imply;
* scikit-learn's TSNE(n_components=2) ONCE on the same array if it imports (its default method, Barnes-Hut, an approximation;
  threads limited to 16) -- or the reason it was not timed.
--method exact (default) writes what it always wrote.  --method neighbours times TSNE(method='neighbours') (sparse P, exact
repulsion) the same way; --method both alternates whole calls of the two in one session (exact, neighbours, exact,
...) and reports each under its name.
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
PAIR_OPS_NN = 16   # repulsion alone: 2 sub, 3 for q, 1 reciprocal, 1 mul, 2 products, 1 select, 3 conversions + 3 fp64 adds
EDGE_OPS_NN = 13   # attraction, per non-zero: 2 sub, 3 for q, 1 reciprocal, 1 mul, 2 products, 2 conversions + 2 fp64 adds
ROW_PASSES = 5     # the neighbour selection reads a row of distances four times for the radix histograms and once to gather


def latents(n, zd, seed=0, classes=10):
    rs = np.random.RandomState(seed)
    means = rs.randn(classes, zd) * 1.5
    return (means[np.arange(n) % classes] + rs.randn(n, zd)).astype(np.float32)


def shape_counts(n, zd, search_steps, method="exact", k=None, nnz=None, splits=1):
    """bytes and operations from the shapes alone.  method='neighbours' needs k, the non-zeros of the joint and the number of
    column ranges the repulsion is split into (evae_tsne_nn_forces_workspace_bytes(n) / 24 n)."""
    pairs = n * (n - 1)
    if method == "neighbours":
        return {
            "affinities": {
                # strips of distances written once and read ROW_PASSES times; idx + d2 written; d2 read, conditionals written;
                # the int64 keys of the 2 n k edges written, sorted (read + written, keys and permutation), read; ia, ib, col, val
                "bytes": 4 * n * n * (1 + ROW_PASSES) + 2 * 4 * n * zd + 8 * n * k + 8 * n * k + 2 * n * k * (8 + 32 + 8) + 16 * nnz,
                "exponentials_fp64": n * k * (search_steps + 1),
                "distance_flops_fp64": 3 * n * n * zd,
                "neighbours": k, "non_zeros": nnz,
            },
            "iteration": {
                # compulsory traffic: Y once per launch; col, val and the gathered y_j per non-zero; row_ptr; the column ranges'
                # partial sums written and read; the per-point record written and read; Y / velocity / gains read + written
                "bytes": 2 * 8 * n + 16 * nnz + 4 * n + 2 * 24 * n * splits + 2 * 64 * n + 3 * 2 * 8 * n,
                "y_tile_bytes_from_cache": 8 * n * ((n + 255) // 256),       # every block of 256 rows stages all of Y through LDS
                "pair_ops": PAIR_OPS_NN * n * n + EDGE_OPS_NN * nnz,
                "reciprocals": n * n + nnz,
                "launches": 3,
                "column_ranges": splits,
            },
        }
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
    ap.add_argument("--method", choices=("exact", "neighbours", "both"), default="exact")
    ap.add_argument("--out", default=None, help="default profiles/tsne.json (exact) or profiles/tsne_nn.json")
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    methods = ["exact", "neighbours"] if a.method == "both" else [a.method]
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "tsne.json" if a.method == "exact" else "tsne_nn.json")

    import torch
    from evae import _lib, ops
    from evae.tsne import TSNE
    X = latents(a.n, a.zd)
    Xd = torch.from_numpy(X).cuda()
    for m in methods:                                          # warm-up: code objects, allocator pools
        TSNE(perplexity=a.perplexity, n_iter=20, random_state=0, method=m).fit_transform(Xd)
    torch.cuda.synchronize()

    whole, kls = {m: [] for m in methods}, {m: [] for m in methods}
    for r in range(a.runs):
        for m in methods:                                      # alternated: exact, neighbours, exact, ...
            t = TSNE(perplexity=a.perplexity, n_iter=a.iters, random_state=r, method=m)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            Y = t.fit_transform(Xd)
            torch.cuda.synchronize()
            whole[m].append(time.perf_counter() - t0)
            kls[m].append(t.kl_divergence_)
            assert bool(torch.isfinite(Y).all())
            del Y, t

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

    lr = max(a.n / 12.0 / 4.0, 50.0)
    STEPS = 50

    def stages(m):
        if m == "neighbours":
            affinities = lambda: ops.tsne_nn_affinities(Xd, a.perplexity)       # noqa: E731
            csr = affinities()[:3]
            forces = lambda Y: ops.tsne_nn_forces(*csr, Y, 1.0, False)          # noqa: E731
            k = ops.tsne_nn_neighbours(a.n, a.perplexity)
            splits = _lib.load().evae_tsne_nn_forces_workspace_bytes(a.n) // (24 * a.n)
            counts = shape_counts(a.n, a.zd, ops.TSNE_SEARCH_STEPS, m, k, csr[1].numel(), splits)
        else:
            affinities = lambda: ops.tsne_affinities(Xd, a.perplexity)          # noqa: E731
            P = affinities()[0]
            forces = lambda Y: ops.tsne_forces(P, Y, 1.0, False)                # noqa: E731
            counts = shape_counts(a.n, a.zd, ops.TSNE_SEARCH_STEPS)
        aff = events(affinities, 3)
        Yd = torch.randn(a.n, 2, device="cuda") * 1e-4
        vel, gains = torch.zeros_like(Yd), torch.ones_like(Yd)

        def iterate():
            for _ in range(STEPS):
                ops.tsne_update(forces(Yd), Yd, vel, gains, 0.8, lr)
        iterate()
        its = [t / STEPS for t in events(iterate, 3)]
        return aff, its, counts

    def report(m):
        aff, its, counts = stages(m)
        aff_med, it_med = statistics.median(aff), statistics.median(its)
        return {
            "what": "%s t-SNE, evae.tsne.TSNE.fit_transform, N=%d zd=%d perplexity=%g n_iter=%d"
                    % ("exact" if m == "exact" else "sparse-affinity (method='neighbours'), exact-repulsion", a.n, a.zd,
                       a.perplexity, a.iters),
            "device": torch.cuda.get_device_name(0),
            "fit_transform_seconds": {"runs": whole[m], "median": statistics.median(whole[m]),
                                      "max_minus_min": max(whole[m]) - min(whole[m]),
                                      "clock": "host perf_counter around a synchronised call"},
            "kl_divergence": kls[m],
            "affinity_stage_seconds": {"runs": aff, "median": aff_med, "max_minus_min": max(aff) - min(aff), "clock": "device events"},
            "iteration_seconds": {"runs": its, "median": it_med, "max_minus_min": max(its) - min(its),
                                  "clock": "device events around %d iterations in stream order, divided by %d" % (STEPS, STEPS)},
            "shape_derived": counts,
            "implied_rates": {
                "affinities_fp64_exponentials_per_s": counts["affinities"]["exponentials_fp64"] / aff_med,
                "iteration_bytes_per_s": counts["iteration"]["bytes"] / it_med,
                "iteration_pair_ops_per_s": counts["iteration"]["pair_ops"] / it_med,
            },
        }

    res = {m: report(m) for m in methods}
    res = dict(res[methods[0]]) if len(methods) == 1 else {"alternated": "whole calls in the order %s, %d rounds" % (methods, a.runs), **res}
    res["scikit_learn"] = {"timed": False, "reason": "--no-sklearn"} if a.no_sklearn else time_sklearn(X, a.iters)
    res["not_measured"] = ["kernel times under a profiler", "hardware counters (bytes actually moved, occupancy)",
                           "N other than %d" % a.n, "scikit-learn's method='exact' (O(N^2) on the host; not attempted at this N)",
                           "more than one scikit-learn run (no spread for it)"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    keys = ("fit_transform_seconds", "affinity_stage_seconds", "iteration_seconds", "kl_divergence")
    line = {m: {k: res[m][k] for k in keys} for m in methods} if len(methods) > 1 else {k: res[k] for k in keys}
    line["scikit_learn"] = res["scikit_learn"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
