"""Times evae.sample_quality on the device and writes profiles/sample_quality.json:

    python tools/sample_quality_bench.py [--sizes 10000,10000,40,5 60000,60000,40,5 10000,10000,784,5 --runs 3]
                                         [--host-n 10000] [--no-torch] [--cdist] [--out profiles/sample_quality.json]

For every (N, M, d, k) -- N real and M generated rows, two draws of the mixture of tools/tsne_bench.py's latents:
* whole compute_prdc and sample_quality calls (host clock around a synchronised call): median of --runs, with max - min;
* the two ball-count passes of compute_prdc, each between device events: the whole ops.ball_count call, the strip distances
  alone (ops.pairwise_distance on the same strips), and the ball-count launches as the difference of the two -- the reader has
  no entry point of its own.  THE ONE BAR: at every size the ball-count launches of a pass take no longer than that pass's
  distance launches (the reader reads a strip once; the distance kernel computes it and writes it once);
* for information, the same four scores from torch float64 operators on the same GPU (squared direct differences accumulated
  feature by feature into chunks of rows, topk, comparisons, any / sum), alternated with ours run for run, and the differences
  of the scores (float64 distances there: an indicator at a float32 near-tie may differ).  --cdist takes the chunks from
  torch.cdist(compute_mode='donot_use_mm_for_euclid_dist') instead: shorter, but on the ROCm build this was written on it
  returned scores far from the host's at these sizes (density in the hundreds), so it is not the default;
* for information, ONE host run of the numpy restatement tests/sample_quality_ref.py at N = M = --host-n (0: skip) on the
  oracle's distances, and whether its four scores equal the device's.
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

SCORES = ("precision", "recall", "density", "coverage")


def spread(runs):
    return {"runs": runs, "median": statistics.median(runs), "max_minus_min": max(runs) - min(runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["10000,10000,40,5", "60000,60000,40,5", "10000,10000,784,5"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=10000)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--cdist", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_quality.json"))
    a = ap.parse_args()

    import torch
    from evae import _lib, ops
    from evae.sample_quality import compute_prdc, sample_quality

    def clocked(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def one_pass(Q, C, col_radius, row_radius):
        """a ball-count pass of compute_prdc: the whole call, its strip distances alone, the reader by difference"""
        B, N = Q.shape[0], C.shape[0]
        rows = _lib.load().evae_ball_count_workspace_bytes(B, N, 0) // (4 * N)

        def whole():
            ops.ball_count(Q, C, col_radius=col_radius, row_radius=row_radius, want_nearest=False)

        def distances():
            for r0 in range(0, B, rows):
                ops.pairwise_distance(Q[r0:r0 + rows], C)
        whole(), distances()                                                                           # warm-up
        total, dist = [], []
        for _ in range(a.runs):                                                                        # alternated
            total.append(events(whole))
            dist.append(events(distances))
        reader = statistics.median(total) - statistics.median(dist)
        return {"clock": "device events", "queries": B, "columns": N, "strip_rows": int(rows), "strips": -(-B // int(rows)),
                "ball_count_seconds": spread(total), "strip_distances_seconds": spread(dist),
                "ball_count_launches_seconds_by_difference": reader,
                "ball_count_launches_over_distance_launches": reader / statistics.median(dist),
                "bar_met": reader <= statistics.median(dist),
                "strip_bytes_written_and_read": 8 * B * N, "distance_flops_fp64": 3 * B * N * Q.shape[1]}

    def torch_prdc(R, F, k, chunk=2048):
        """prdc's four expressions from torch float64 operators on squared distances; the distances by direct differences, one
        feature at a time into a chunk of rows (elementwise operators only: see --cdist in the doc string)"""
        def dists(A, B):
            Bt = B.t().contiguous()
            for r0 in range(0, A.shape[0], chunk):
                if a.cdist:
                    yield r0, torch.cdist(A[r0:r0 + chunk], B, compute_mode='donot_use_mm_for_euclid_dist') ** 2
                    continue
                D = torch.zeros((min(chunk, A.shape[0] - r0), B.shape[0]), dtype=A.dtype, device=A.device)
                for t in range(A.shape[1]):
                    diff = A[r0:r0 + chunk, t, None] - Bt[t][None, :]
                    D.addcmul_(diff, diff)
                yield r0, D

        def kth(A):                                              # the row itself included, at distance 0: the (k + 1)-th value
            return torch.cat([D.topk(k + 1, dim=1, largest=False).values[:, k] for _, D in dists(A, A)])
        R, F = R.double(), F.double()
        rho_r, rho_f = kth(R), kth(F)
        in_real = torch.zeros(F.shape[0], dtype=torch.int64, device=R.device)
        held, covered = [], []
        for r0, D in dists(R, F):
            inside = D < rho_r[r0:r0 + chunk, None]
            in_real += inside.sum(dim=0)
            held.append((D < rho_f[None, :]).any(dim=1))
            covered.append(D.min(dim=1).values < rho_r[r0:r0 + chunk])
        N, M = R.shape[0], F.shape[0]
        sums = torch.stack(((in_real > 0).sum(), in_real.sum(), torch.cat(held).sum(), torch.cat(covered).sum())).tolist()
        return dict(precision=sums[0] / M, recall=sums[2] / N, density=(1.0 / k) * (sums[1] / M), coverage=sums[3] / N)

    def host(X, n, d, k, device_scores):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import evae_oracle as orc
        import sample_quality_ref as rr
        R, F = X[:n], X[n:]
        t0 = time.perf_counter()
        got = rr.prdc(orc.pairdist_direct_f64(R, R), orc.pairdist_direct_f64(F, F), orc.pairdist_direct_f64(R, F), k)
        return {"seconds": time.perf_counter() - t0, "runs": 1, "n": n, "m": n, "d": d, "k": k, "scores": {s: got[s] for s in SCORES},
                "equal_to_the_device": all(got[s] == device_scores[s] for s in SCORES),
                "what": "numpy float64 direct differences row by row, rounded to float32, then tests/sample_quality_ref.py",
                "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS")}

    def save(res):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res = {"what": "evae.sample_quality on two draws of the latents of tools/tsne_bench.py, by (N, M, d, k)",
           "device": torch.cuda.get_device_name(0), "clock": "host perf_counter around a synchronised call unless stated",
           "by_size": {}}
    for size in a.sizes:
        N, M, d, k = (int(v) for v in size.split(","))
        X = latents(N + M, d)
        R, F = torch.from_numpy(X[:N]).cuda(), torch.from_numpy(X[N:]).cuda()
        compute_prdc(R, F, k), sample_quality(R, F, k)                                                 # warm-up
        ours, whole, theirs, scores, their_scores = [], [], [], None, None
        for _ in range(a.runs):                                                                        # alternated with torch's
            dt, scores = clocked(lambda: compute_prdc(R, F, k))
            ours.append(dt)
            whole.append(clocked(lambda: sample_quality(R, F, k))[0])
            if not a.no_torch:
                dt, their_scores = clocked(lambda: torch_prdc(R, F, k))
                theirs.append(dt)
        rho_r, rho_f = ops.kth_neighbour_radius(R, k), ops.kth_neighbour_radius(F, k)
        knn = [events(lambda: ops.kth_neighbour_radius(R, k)) for _ in range(a.runs)]
        entry = {"n_real": N, "n_fake": M, "d": d, "nearest_k": k, "scores": scores,
                 "compute_prdc_seconds": spread(ours), "sample_quality_seconds": spread(whole),
                 "kth_neighbour_radius_seconds_device_events": spread(knn),
                 "pass_generated_against_real": one_pass(F, R, rho_r, None),
                 "pass_real_against_generated": one_pass(R, F, rho_f, rho_r)}
        entry["bar_met"] = entry["pass_generated_against_real"]["bar_met"] and entry["pass_real_against_generated"]["bar_met"]
        if theirs:
            entry["torch_float64_operators"] = {"seconds": spread(theirs), "scores": their_scores, "chunk_rows": 2048, "distances": "torch.cdist, no matrix product" if a.cdist else "elementwise, feature by feature",
                                                "ours_minus_theirs": {s: scores[s] - their_scores[s] for s in SCORES}}
        if a.host_n and (N, M) == (a.host_n, a.host_n) and d <= 64:
            entry["numpy_restatement_on_the_host"] = host(X, N, d, k, scores)
        res["by_size"][size] = entry
        save(res)                                                                                      # what is measured so far
        del R, F
        print(json.dumps({size: {"compute_prdc_seconds": entry["compute_prdc_seconds"]["median"], "scores": scores,
                                 "ratios": [entry[p]["ball_count_launches_over_distance_launches"]
                                            for p in ("pass_generated_against_real", "pass_real_against_generated")],
                                 "torch_seconds": statistics.median(theirs) if theirs else None,
                                 "host": entry.get("numpy_restatement_on_the_host")}}), flush=True)
    res["bar"] = {"what": "by device events, the ball-count launches of a pass take no longer than the pass's distance launches",
                  "met": {size: e["bar_met"] for size, e in res["by_size"].items()}}
    res["not_measured"] = ["kernel times under a profiler", "hardware counters (bytes actually moved, cache hits of the radii)",
                           "the ball-count launches on their own (they are a difference of two event times)",
                           "sizes other than %s" % a.sizes, "the numpy restatement more than once, or at the large N (no spread for it)",
                           "the `prdc` package itself (not installed); torch's operators stand in for a float64 formulation on the GPU",
                           "samples of a trained model: the rows are synthetic latents"]
    save(res)
    print(json.dumps(res["bar"]))


if __name__ == "__main__":
    main()
