"""Times evae.cluster on the device and writes profiles/kmeans.json (the protocol of tools/pca_bench.py):

    python tools/kmeans_bench.py [--runs 3 --reps 50 --out profiles/kmeans.json] [--no-sklearn]

* THE ONE BAR: one Lloyd iteration -- ops.kmeans_step: assign + update + finish -- under device events against the same
  arithmetic from torch operators in float64 on the same GPU (cdist with compute_mode='donot_use_mm_for_euclid_dist', argmin,
  index_add_, bincount, a division), at (N, d, K) = (60 000, 40, 10) and (60 000, 40, 1 000) on tsne_bench's latents.  Both are
  alternated in one session: --runs rounds, in each the mean over --reps iterations (an event pair around every iteration; the
  centres are put back and the record is zeroed outside the pair, so no iteration meets the done flag; a variant that takes
  longer than --budget seconds per round gets fewer iterations, 3 at the least, and says how many); median of the rounds with
  max - min.  How many labels of each torch formulation differ from the candidate's is recorded beside the times.  Met: the
  candidate is no slower by more than the sum of the two spreads.  The baseline is the torch formulation, never an earlier build
  of this code.  Recorded either way.
* for information: the float32 torch formulation in the same rounds; whole KMeans(K).fit calls (k-means++, one run, tol 1e-4) and
  silhouette_score of their labels at N = 10 000 and 60 000 (host clock around a synchronised call, median of --runs with
  max - min), with the iterations each fit ran; ONE scikit-learn KMeans(algorithm='lloyd', n_init=1) at both N and ONE
  silhouette_score at N = 10 000 on the host if scikit-learn imports (threads limited to 16).
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

BAR_SHAPES = ((60000, 40, 10), (60000, 40, 1000))
FIT_SHAPES = ((10000, 40, 10), (60000, 40, 10))


def spread(runs, clock):
    return {"runs": runs, "median": statistics.median(runs), "max_minus_min": max(runs) - min(runs), "clock": clock}


def time_sklearn(X, K, labels, with_silhouette):
    try:
        import sklearn
        from sklearn.cluster import KMeans as SkKMeans
        from sklearn.metrics import silhouette_score as sk_silhouette
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
        km = SkKMeans(n_clusters=K, n_init=1, algorithm='lloyd', random_state=0).fit(X)
        out = {"timed": True, "fit_seconds": time.perf_counter() - t0, "n_iter": int(km.n_iter_), "inertia": float(km.inertia_),
               "runs": 1, "threads": 16 if limit is not None else None,      # None: threadpoolctl did not import, no limit in force
               "version": sklearn.__version__,
               "note": "its k-means++ has greedy local trials and its own random stream: another local minimum, another iteration count"}
        if with_silhouette:
            t0 = time.perf_counter()
            out["silhouette"] = float(sk_silhouette(X, labels))
            out["silhouette_seconds"] = time.perf_counter() - t0
    finally:
        if limit is not None:
            limit.restore_original_limits()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--budget", type=float, default=5.0, help="seconds of device time a variant may take per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans.json"))
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()

    import torch
    from evae import ops
    from evae.cluster import KMeans, silhouette_score

    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench: no GPU; nothing is measured without one")

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

    res = {"device": torch.cuda.get_device_name(0), "one_lloyd_iteration": {}, "fit": {}}
    clock = "device events around each of %d iterations, their mean; one value per round"
    for n, d, K in BAR_SHAPES:
        x = torch.from_numpy(latents(n, d)).cuda()
        c0 = x[torch.randperm(n, generator=torch.Generator().manual_seed(0))[:K].cuda()].double().contiguous()
        centres = c0.clone()
        labels = torch.empty(n, dtype=torch.int32, device="cuda")
        d2 = torch.empty(n, dtype=torch.float64, device="cuda")
        order = torch.empty(n, dtype=torch.int32, device="cuda")
        start = torch.empty(K + 1, dtype=torch.int32, device="cuda")
        state, ws = ops.kmeans_state(x.device), ops.kmeans_workspace(n, d, K, x.device)
        x64, x32c = x.double(), c0.float()

        def put_back():
            centres.copy_(c0)
            state.zero_()

        def candidate():
            ops.kmeans_step(x, centres, labels, d2, order, start, 0.0, state, ws)

        def torch_iteration(xx, cc):
            def run():
                lab = torch.cdist(xx, cc, compute_mode='donot_use_mm_for_euclid_dist').argmin(dim=1)
                sums = torch.zeros_like(cc).index_add_(0, lab, xx)
                return sums / torch.bincount(lab, minlength=K).clamp_(min=1).to(cc.dtype)[:, None], lab
            return run

        baseline, baseline32 = torch_iteration(x64, c0), torch_iteration(x, x32c)
        for fn in (candidate, baseline, baseline32):             # warm-up: code objects, allocator pools
            put_back()
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        put_back()
        candidate()
        def against_candidate(fn):                                # do the two compute the same assignment?
            differ = (fn()[1].int() != labels).nonzero().flatten()
            return {"labels_differing": int(differ.numel()), "first_differing_row": int(differ[0]) if differ.numel() else None}

        differing, differing32 = against_candidate(baseline), against_candidate(baseline32)
        variants = {"candidate": (put_back, candidate), "torch_float64": (lambda: None, baseline),
                    "torch_float32": (lambda: None, baseline32)}
        reps = {name: max(3, min(a.reps, int(a.budget / max(timed(prep, fn, 1), 1e-9)))) for name, (prep, fn) in variants.items()}
        runs = {name: [] for name in variants}
        for _ in range(a.runs):                                   # alternated
            for name, (prep, fn) in variants.items():
                runs[name].append(timed(prep, fn, reps[name]))
        cand, base = spread(runs["candidate"], clock % reps["candidate"]), spread(runs["torch_float64"], clock % reps["torch_float64"])
        res["one_lloyd_iteration"]["N=%d d=%d K=%d" % (n, d, K)] = {
            "candidate_seconds": cand, "torch_float64_seconds": base,
            "torch_float32_seconds": spread(runs["torch_float32"], clock % reps["torch_float32"]),
            "torch_float64_against_candidate": differing,
            "torch_float32_against_candidate": differing32,       # (float32 rounding may move a near tie: a few, not thousands)
            "bar": "candidate.median <= torch_float64.median + candidate.max_minus_min + torch_float64.max_minus_min",
            "bar_met": bool(cand["median"] <= base["median"] + cand["max_minus_min"] + base["max_minus_min"]),
            "ratio_of_medians": cand["median"] / base["median"],
        }
        del x, x64, centres, labels, d2, order, start, ws

    host_clock = "host perf_counter around a synchronised call"
    for n, d, K in FIT_SHAPES:
        X = latents(n, d)
        x = torch.from_numpy(X).cuda()
        km = KMeans(K, random_state=0).fit(x)                     # warm-up
        silhouette_score(x, km.labels_)
        torch.cuda.synchronize()
        fits, sils, iters = [], [], []
        for r in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            km = KMeans(K, random_state=r).fit(x)
            torch.cuda.synchronize()
            fits.append(time.perf_counter() - t0)
            iters.append(km.n_iter_)
            t0 = time.perf_counter()
            s = silhouette_score(x, km.labels_)
            torch.cuda.synchronize()
            sils.append(time.perf_counter() - t0)
        res["fit"]["N=%d d=%d K=%d" % (n, d, K)] = {
            "fit_seconds": spread(fits, host_clock + " (k-means++, one run, tol 1e-4, check_every 8)"), "n_iter": iters,
            "inertia": km.inertia_, "silhouette_seconds": spread(sils, host_clock), "silhouette": s,
            "scikit_learn": {"timed": False, "reason": "--no-sklearn"} if a.no_sklearn
            else time_sklearn(X, K, km.labels_.cpu().numpy(), with_silhouette=n <= 10000),
        }
        del x, km

    res["not_measured"] = ["kernel times under a profiler", "hardware counters", "the stages of an iteration one by one",
                           "N above 60 000", "d other than 40", "K between 10 and 1 000", "the seeding alone",
                           "scikit-learn's silhouette_score at N = 60 000", "more than one scikit-learn run (no spread for it)"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
