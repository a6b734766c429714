"""Scores and times evae.tsne.embedding_quality on the device and writes profiles/tsne_quality.json:

    python tools/tsne_quality_bench.py [--n 10000 --zd 40 --iters 1000 --runs 3 --ks 5 12 --large-n 60000] [--no-sklearn]

At --n points (the latents of tools/tsne_bench.py), for TSNE(method='exact') and TSNE(method='neighbours') with the same seed:
* whole fit_transform calls and whole embedding_quality calls (host clock around a synchronised call): median of --runs, with
  max - min, and whether the score costs less than the fit it judges -- the only bar there is: the fit is --iters passes over
  the N^2 pairs, the score is two;
* one ops.nn_rank call between device events, the strip distances alone (ops.pairwise_distance on the same strips) between
  device events, and the counting kernel as the difference of the two -- it has no entry point of its own; the same with the
  chosen columns drawn at random, the case in which most of a row goes through the binary search;
* the scores of both embeddings at every k of --ks;
* sklearn.manifold.trustworthiness ONCE per k on the host on the exact embedding, its time, and the difference to the device's
  value (scikit-learn takes float64 distances from an expansion: ranks at float32 near-ties may differ), which must stay
  within 1e-6.
At --large-n points (0: skip): the neighbours embedding alone, its time and scores; no host version there.
Nothing here runs under a profiler."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))

from tsne_bench import latents  # noqa: E402


def spread(runs):
    return {"runs": runs, "median": statistics.median(runs), "max_minus_min": max(runs) - min(runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--zd", type=int, default=40)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--ks", type=int, nargs="+", default=[5, 12])
    ap.add_argument("--large-n", type=int, default=60000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_quality.json"))
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    from evae import _lib, ops
    from evae.tsne import TSNE, embedding_quality

    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def events(fn, reps=3):
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3)
        return out

    def fit(Xd, method, runs):
        """-> (seconds of `runs` whole calls with random_state 0, the embedding, its KL)"""
        TSNE(perplexity=a.perplexity, n_iter=20, random_state=0, method=method).fit_transform(Xd)      # warm-up
        secs = []
        for _ in range(runs):
            t = TSNE(perplexity=a.perplexity, n_iter=a.iters, random_state=0, method=method)
            dt, Y = clocked(lambda: t.fit_transform(Xd))
            secs.append(dt)
        return secs, Y, t.kl_divergence_

    def quality(Xd, Y, k, labels, runs):
        embedding_quality(Xd, Y, k, labels=labels)                                                     # warm-up
        secs = []
        for _ in range(runs):
            dt, q = clocked(lambda: embedding_quality(Xd, Y, k, labels=labels))
            secs.append(dt)
        return secs, q

    def stages(Xd, Y, k):
        """one ranking pass (the embedding's neighbours ranked in X), its strip distances alone, and the rest"""
        n = Xd.shape[0]
        nbr = ops.tsne_knn(Y, k)[0]
        rows = _lib.load().evae_nn_rank_workspace_bytes(n, 0) // (4 * n)

        def distances():
            for r0 in range(0, n, rows):
                ops.pairwise_distance(Xd[r0:r0 + rows], Xd)
        ops.nn_rank(Xd, nbr), distances()                                                              # warm-up
        total, dist = events(lambda: ops.nn_rank(Xd, nbr)), events(distances)
        # columns drawn at random instead: ranks anywhere up to N, so about (k - 1) / k of a row's elements walk the binary search
        anywhere = torch.randint(0, n, (n, k), device=Xd.device, generator=torch.Generator(device=Xd.device).manual_seed(k)).int()
        ops.nn_rank(Xd, anywhere)
        far = events(lambda: ops.nn_rank(Xd, anywhere))
        return {"clock": "device events", "strip_rows": int(rows), "strips": -(-n // int(rows)),
                "nn_rank_seconds": spread(total), "strip_distances_seconds": spread(dist),
                "counting_kernel_seconds_by_difference": statistics.median(total) - statistics.median(dist),
                "nn_rank_seconds_random_columns": spread(far),
                "counting_kernel_seconds_by_difference_random_columns": statistics.median(far) - statistics.median(dist),
                "strip_bytes_written_and_read": 8 * n * n, "distance_flops_fp64": 3 * n * n * Xd.shape[1]}

    def host(X, Y, k, device_value):
        if a.no_sklearn:
            return {"timed": False, "reason": "--no-sklearn"}
        try:
            import sklearn
            from sklearn.manifold import trustworthiness as sk_trustworthiness
        except Exception as e:                                   # noqa: BLE001
            return {"timed": False, "reason": "scikit-learn does not import here: %r" % (e,)}
        t0 = time.perf_counter()
        value = float(sk_trustworthiness(X, Y, n_neighbors=k))
        return {"timed": True, "seconds": time.perf_counter() - t0, "runs": 1, "trustworthiness": value,
                "device_minus_host": device_value - value, "agree_to_1e-6": abs(device_value - value) <= 1e-6,
                "version": sklearn.__version__, "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS")}

    X = latents(a.n, a.zd)
    labels = np.arange(a.n) % 10                                 # the classes latents() draws its means for
    Xd = torch.from_numpy(X).cuda()
    res = {"what": "evae.tsne.embedding_quality of TSNE embeddings, N=%d zd=%d perplexity=%g n_iter=%d random_state=0"
                   % (a.n, a.zd, a.perplexity, a.iters),
           "device": torch.cuda.get_device_name(0), "clock": "host perf_counter around a synchronised call unless stated"}
    fits = {m: fit(Xd, m, a.runs) for m in ("exact", "neighbours")}
    res["fit_transform_seconds"] = {m: spread(fits[m][0]) for m in fits}
    res["kl_divergence"] = {m: fits[m][2] for m in fits}
    res["by_k"] = {}
    for k in a.ks:
        entry = {}
        for m in fits:
            secs, q = quality(Xd, fits[m][1], k, labels, a.runs)
            entry[m] = {"scores": q, "embedding_quality_seconds": spread(secs),
                        "costs_less_than_its_fit": statistics.median(secs) < statistics.median(fits[m][0])}
        entry["stages_of_one_ranking_pass"] = stages(Xd, fits["exact"][1], k)
        entry["scikit_learn_on_the_exact_embedding"] = host(X, fits["exact"][1].cpu().numpy(), k, entry["exact"]["scores"]["trustworthiness"])
        res["by_k"][str(k)] = entry
    del fits

    if a.large_n:
        XL = latents(a.large_n, a.zd)
        XLd = torch.from_numpy(XL).cuda()
        secs, Y, kl = fit(XLd, "neighbours", 1)
        large = {"n": a.large_n, "method": "neighbours", "fit_transform_seconds": secs[0], "kl_divergence": kl, "by_k": {}}
        for k in a.ks:
            qs, q = quality(XLd, Y, k, np.arange(a.large_n) % 10, a.runs)
            large["by_k"][str(k)] = {"scores": q, "embedding_quality_seconds": spread(qs),
                                     "costs_less_than_its_fit": statistics.median(qs) < secs[0],
                                     "stages_of_one_ranking_pass": stages(XLd, Y, k)}
        res["large"] = large
    res["not_measured"] = ["kernel times under a profiler", "hardware counters (bytes actually moved, bank conflicts of the bins)",
                           "N other than %s" % ([a.n] + ([a.large_n] if a.large_n else [])), "k above %d" % max(a.ks),
                           "the counting kernel on its own (it is a difference of two event times)",
                           "scikit-learn's trustworthiness at the large N, or more than once (no spread for it)",
                           "chosen columns that are ALL far away (ranks near N in every entry; random columns are timed)"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"fit_transform_seconds": {m: v["median"] for m, v in res["fit_transform_seconds"].items()},
                      "by_k": {k: {m: {"seconds": e[m]["embedding_quality_seconds"]["median"], **e[m]["scores"]}
                                   for m in ("exact", "neighbours")} for k, e in res["by_k"].items()},
                      "scikit_learn": {k: e["scikit_learn_on_the_exact_embedding"] for k, e in res["by_k"].items()},
                      "large": res.get("large")}))
    bad = [k for k, e in res["by_k"].items() if e["scikit_learn_on_the_exact_embedding"].get("agree_to_1e-6") is False]
    if bad:
        sys.exit("device and scikit-learn trustworthiness differ by more than 1e-6 at k = %s" % bad)


if __name__ == "__main__":
    main()
