"""Times ops.agg_posterior_lse on the device against the same arithmetic from torch float64 operators on the same GPU and writes
profiles/latent_info.json:

    python tools/latent_info_bench.py [--sizes 10000,10000,40 60000,60000,40 --runs 3] [--torch-rows 6000] [--chunk 64]
                                      [--out profiles/latent_info.json]

For every (B, N, d) -- N posteriors whose means are the latents of tools/tsne_bench.py and whose log-variances are seeded
uniforms in [-6, -2], B queries drawn one per posterior (evae.latent_info.draw_posterior_samples):
* the launches of ONE agg_posterior_lse call with both outputs (log_q and log_qd; the prepare launch included), between device
  events;
* the torch form, between device events: w = exp(-lv), c = -(lv + log 2 pi) / 2, then per chunk of --chunk query rows the
  broadcast [chunk x N x d] terms c - (z - mu)^2 w / 2 by direct differences (never torch.cdist), torch.logsumexp over the
  components for log_qd, and over the components of their sums over d for log_q.  Where B exceeds 2 x --torch-rows the torch
  form runs on the first --torch-rows queries only, and its time for all B rows is that times B / rows (it is linear in the
  query rows: every chunk does the same work);
* the two alternated run for run in one session after a warm-up of each: median of --runs with max - min.
THE ONE BAR: at every size the kernel's median is below torch's by more than the larger of the two spreads.
Also recorded: the largest difference between the two implementations' outputs on the rows both computed, whole
evae.latent_info.latent_information calls under a host clock, and what was not measured.  Nothing here runs under a profiler."""
import argparse
import json
import math
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
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_info.json"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from evae import ops
    from evae.latent_info import draw_posterior_samples, latent_information

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    def torch_form(z, mean, log_var):
        z, mu, lv = z.double(), mean.double(), log_var.double()
        w, c = torch.exp(-lv), -0.5 * (lv + math.log(2.0 * math.pi))
        log_n = math.log(mu.shape[0])
        log_q, log_qd = [], []
        for s in range(0, z.shape[0], a.chunk):
            t = c[None] - 0.5 * (z[s:s + a.chunk, None, :] - mu[None]) ** 2 * w[None]
            log_qd.append(torch.logsumexp(t, dim=1) - log_n)
            log_q.append(torch.logsumexp(t.sum(dim=2), dim=1) - log_n)
        return torch.cat(log_q), torch.cat(log_qd)

    def save(res):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res = {"what": "ops.agg_posterior_lse (log_q and log_qd) against torch float64 operators, by (B, N, d)",
           "device": torch.cuda.get_device_name(0), "clock": "device events around the launches of one call", "by_size": {}}
    for size in a.sizes:
        B, N, d = (int(v) for v in size.split(","))
        mean = torch.from_numpy(latents(N, d)).cuda()
        log_var = torch.from_numpy(np.random.RandomState(1).uniform(-6.0, -2.0, size=(N, d)).astype(np.float32)).cuda()
        z = draw_posterior_samples(mean, log_var, n_samples=B, random_state=0)[0]
        rows = B if B <= 2 * a.torch_rows else a.torch_rows
        zt = z[:rows].contiguous()
        ours, theirs = [], []
        got = ops.agg_posterior_lse(z, mean, log_var)                                              # warm-up of both
        want = torch_form(zt, mean, log_var)
        torch.cuda.synchronize()
        for _ in range(a.runs):                                                                    # alternated
            ours.append(events(lambda: ops.agg_posterior_lse(z, mean, log_var))[0])
            theirs.append(events(lambda: torch_form(zt, mean, log_var))[0])
        scale = B / rows
        k, t = spread(ours), spread(theirs)
        margin = max(k["max_minus_min"], t["max_minus_min"] * scale)
        entry = {"queries": B, "components": N, "d": d, "terms": B * N * d,
                 "kernel_seconds": k, "torch_float64_seconds": t, "torch_query_rows": rows, "torch_chunk_rows": a.chunk,
                 "torch_seconds_for_all_queries": t["median"] * scale,
                 "torch_time_is": "measured on all queries" if rows == B else
                 "measured on the first %d queries, times %g for all of them" % (rows, scale),
                 "torch_over_kernel": t["median"] * scale / k["median"],
                 "larger_spread_seconds": margin, "bar_met": k["median"] + margin < t["median"] * scale,
                 "kernel_on_all_queries_below_torch_on_its_rows": k["median"] < t["median"],
                 "terms_per_second_kernel": B * N * d / k["median"],
                 "largest_difference": {"log_q": float((got.log_q[:rows] - want[0]).abs().max()),
                                        "log_qd": float((got.log_qd[:rows] - want[1]).abs().max()),
                                        "largest_magnitude_log_q": float(want[0].abs().max())}}
        del got, want
        whole = []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = latent_information(mean, log_var, random_state=0)
            torch.cuda.synchronize()
            whole.append(time.perf_counter() - t0)
        entry["latent_information_call_seconds_host_clock"] = spread(whole)
        entry["latent_information_call_rows"] = N
        entry["scores"] = {key: info[key] for key in ("mutual_information", "total_correlation", "dimension_wise_kl", "log_n",
                                                      "active_units", "active_units_by_information")}
        res["by_size"][size] = entry
        save(res)                                                                                  # what is measured so far
        print(json.dumps({size: {"kernel": k["median"], "torch_all_queries": t["median"] * scale, "bar_met": entry["bar_met"],
                                 "difference": entry["largest_difference"]}}), flush=True)
        del mean, log_var, z, zt
    res["bar"] = {"what": "by device events, the kernel's median is below torch's by more than the larger of the two spreads",
                  "met": {size: e["bar_met"] for size, e in res["by_size"].items()}}
    res["not_measured"] = ["kernel times under a profiler, and the share of each of the three launches (prepare, joint, per dimension)",
                           "hardware counters: fp64 VALU utilisation, LDS reads, cache hits of the staged components",
                           "the torch form on all 60 000 queries (a 6 000-row slice, scaled: see torch_time_is)",
                           "torch chunk sizes other than %d rows, and torch.compile" % a.chunk,
                           "sizes other than %s, d > 40 in particular (the joint kernel's rows then take up to 64 KiB of LDS)" % a.sizes,
                           "log_cond (one term per query and dimension: not a hot path)",
                           "posteriors of a trained model: the rows are synthetic latents"]
    save(res)
    print(json.dumps(res["bar"]))


if __name__ == "__main__":
    main()
