"""Times the three row-sum passes of evae.sample_quality.kernel_mmd('poly') on the device against the same arithmetic from torch
float64 operators on the same GPU and writes profiles/kernel_mmd.json:

    python tools/kernel_mmd_bench.py [--sizes 10000,10000,40 60000,60000,40 --runs 3] [--torch-rows 6000] [--chunk 2048]
                                     [--out profiles/kernel_mmd.json]

For every (N, M, d) -- N real rows (the latents of tools/tsne_bench.py) and M generated ones (another seed, shrunk and shifted):
* the three launches of ops.kernel_row_sums that kernel_mmd issues -- real x real and fake x fake with skip_self, real x fake --
  with KID's kernel (<x, y> / d + 1)^3, between device events (the ordered totals are not in it: they are not the hot path);
* the torch form, between device events: the rows as float64, then per chunk of --chunk query rows times ALL columns a float64
  matmul, the affine map, the cube by two multiplications and a sum over the columns; for the within-set passes the diagonal's
  terms are taken off row by row.  torch.cdist is not used anywhere.  Where a pass has more than 2 x --torch-rows query rows the
  torch form runs on the first --torch-rows of them only, and its time for all rows is that times rows / --torch-rows (it is
  linear in the query rows: every chunk does the same work);
* the two alternated run for run in one session after a warm-up of each: median of --runs with max - min.
THE ONE BAR: at every size the kernel's median is below torch's by more than the larger of the two spreads.
Also recorded: the largest relative difference between the two implementations' row sums on the rows both computed, the rbf
kernel's three passes, whole frechet_distance and kernel_mmd calls under a host clock, and what was not measured.  Nothing here
runs under a profiler."""
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
    ap.add_argument("--sizes", nargs="+", default=["10000,10000,40", "60000,60000,40"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--torch-rows", type=int, default=6000)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_mmd.json"))
    a = ap.parse_args()

    import torch
    from evae import ops
    from evae.sample_quality import frechet_distance, kernel_mmd

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    def passes(R, F):
        return ((R, R, True), (F, F, True), (R, F, False))

    def kernel_form(R, F, kind):
        return [ops.kernel_row_sums(q, c, kind, skip_self=s) for q, c, s in passes(R, F)]

    def torch_pass(q, c, skip, rows, gamma):
        q64, c64 = q[:rows].double(), c.double()
        out = []
        for s in range(0, rows, a.chunk):
            b = (q64[s:s + a.chunk] @ c64.t()) * gamma + 1.0
            out.append((b * b * b).sum(dim=1))
        out = torch.cat(out)
        if skip:
            b = (q64 * q64).sum(dim=1) * gamma + 1.0
            out = out - b * b * b
        return out

    def torch_form(R, F, rows):
        gamma = 1.0 / R.shape[1]
        return [torch_pass(q, c, s, min(rows, q.shape[0]), gamma) for q, c, s in passes(R, F)]

    def save(res):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res = {"what": "the three ops.kernel_row_sums passes of kernel_mmd('poly') against torch float64 operators, by (N, M, d)",
           "device": torch.cuda.get_device_name(0), "clock": "device events around the three launches", "by_size": {}}
    for size in a.sizes:
        N, M, d = (int(v) for v in size.split(","))
        R = torch.from_numpy(latents(N, d)).cuda()
        F = torch.from_numpy(0.9 * latents(M, d, seed=1) + 0.1).cuda()
        rows = max(N, M) if max(N, M) <= 2 * a.torch_rows else a.torch_rows
        got = kernel_form(R, F, 'poly')                                                            # warm-up of both
        kernel_form(R, F, 'rbf')
        want = torch_form(R, F, rows)
        torch.cuda.synchronize()
        ours, theirs, rbf = [], [], []
        for _ in range(a.runs):                                                                    # alternated
            ours.append(events(lambda: kernel_form(R, F, 'poly'))[0])
            theirs.append(events(lambda: torch_form(R, F, rows))[0])
            rbf.append(events(lambda: kernel_form(R, F, 'rbf'))[0])
        scale = max(N, M) / rows if N == M else None
        assert scale is not None, "the scaled torch time needs N == M (every pass then has the same query rows)"
        k, t = spread(ours), spread(theirs)
        margin = max(k["max_minus_min"], t["max_minus_min"] * scale)
        pairs = N * (N - 1) + M * (M - 1) + N * M
        entry = {"real_rows": N, "fake_rows": M, "d": d, "pairs": pairs,
                 "kernel_seconds": k, "torch_float64_seconds": t, "torch_query_rows": rows, "torch_chunk_rows": a.chunk,
                 "torch_seconds_for_all_rows": t["median"] * scale,
                 "torch_time_is": "measured on all rows" if scale == 1 else
                 "measured on the first %d query rows of every pass, times %g for all of them" % (rows, scale),
                 "torch_over_kernel": t["median"] * scale / k["median"],
                 "larger_spread_seconds": margin, "bar_met": k["median"] + margin < t["median"] * scale,
                 "pairs_per_second_kernel": pairs / k["median"],
                 "fp64_fma_per_second_kernel": pairs * d / k["median"],
                 "largest_relative_difference_of_row_sums": max(float(((g[:len(w)] - w).abs() / w.abs()).max()) for g, w in zip(got, want)),
                 "rbf_kernel_seconds": spread(rbf)}
        del got, want
        whole = {"kernel_mmd_poly": [], "kernel_mmd_rbf": [], "frechet_distance": []}
        for _ in range(a.runs):
            for name, fn in (("kernel_mmd_poly", lambda: kernel_mmd(R, F)), ("kernel_mmd_rbf", lambda: kernel_mmd(R, F, kernel='rbf')),
                             ("frechet_distance", lambda: frechet_distance(R, F))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                whole[name].append(time.perf_counter() - t0)
                entry.setdefault("values", {})[name] = out
        entry["call_seconds_host_clock"] = {name: spread(v) for name, v in whole.items()}
        res["by_size"][size] = entry
        save(res)                                                                                  # what is measured so far
        print(json.dumps({size: {"kernel": k["median"], "torch_all_rows": t["median"] * scale, "bar_met": entry["bar_met"],
                                 "rbf": entry["rbf_kernel_seconds"]["median"],
                                 "difference": entry["largest_relative_difference_of_row_sums"]}}), flush=True)
        del R, F
    res["bar"] = {"what": "by device events, the kernel's median is below torch's by more than the larger of the two spreads",
                  "met": {size: e["bar_met"] for size, e in res["by_size"].items()}}
    res["not_measured"] = ["kernel times under a profiler, and hardware counters: fp64 VALU utilisation, LDS reads, L2 hits of the staged columns",
                           "the torch form on all 60 000 query rows (a 6 000-row slice of every pass, scaled: see torch_time_is)",
                           "torch chunk sizes other than %d rows, torch.compile, and a torch form of the rbf kernel" % a.chunk,
                           "sizes other than %s; d > 40 in particular (the query rows then take up to 64 KiB of LDS per wave)" % a.sizes,
                           "tiles other than 32 columns, blocks of more than one wave, more than one query row per thread",
                           "the ordered totals and the congruence product on their own (in the whole calls only)",
                           "gamma='median' (a 2 048-row subsample: not a hot path)",
                           "features of a trained model: the rows are synthetic latents"]
    save(res)
    print(json.dumps(res["bar"]))


if __name__ == "__main__":
    main()
