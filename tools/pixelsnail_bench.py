#!/usr/bin/env python3
"""First measurements of the PixelSNAIL decoder (model_name 'pixelcnn') on the GPU -> profiles/pixelsnail.json.

  1. the fused causal-attention kernels (csrc/evae_attn.hip, forward + backward, dropout 0.1) against the same formula composed from
     torch ops on the same GPU (matmul, masked_fill(-1e4), softmax, start mask, dropout, matmul: reference utils/nn.py:351-359), at
     B = 100 and B = 10, H = 8, L = 784, dh = 4: time per forward+backward and peak memory of each variant;
  2. one eager training step of `pixelcnn` at B = 100 (exemplar prior, AdamNormGrad, dropout on).

  --step (a leg of its own -> profiles/pixelsnail_step.json): ms per training step of `pixelcnn` through train_one_epoch, replayed from
     the captured graph (utils/training.py::pixelcnn_step_eligible) against use_hip_graph = False in one process, at B = 100 and
     B = 10 with the configuration of 2. (2 000 rows, 500 exemplars): a warm-up epoch per path (workspaces, the capture), then
     --rounds epochs per path, alternated between the two; host clock around an epoch that ends in the read-back of its sums, every
     epoch's figure kept (p50, min, max and max - min, the spread, per path); the node count of the captured graph.

Times are device-event intervals around work that ends in a synchronise; every shape is warmed up first; each figure is the median of
--reps windows with the minimum and maximum next to it (the spread).  The two attention variants alternate window by window.  Needs
a GPU: there is no fallback, and nothing here is an estimate."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))

import numpy as np
import torch


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "windows": len(ms)}


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def torch_attention(q, k, v, B, L, H, p_drop):
    """the reference's composition on [B*L, H*dh] rows"""
    heads = lambda t: t.view(B, L, H, -1).transpose(1, 2)
    qh, kh, vh = heads(q), heads(k).transpose(2, 3), heads(v)
    attn = torch.matmul(qh, kh) / math.sqrt(qh.shape[-1])
    idx = torch.arange(L, device=q.device)
    attn = attn.masked_fill((idx.view(1, L) >= idx.view(L, 1)).view(1, 1, L, L), -1e4)
    start = torch.ones(L, 1, device=q.device)
    start[0] = 0
    attn = torch.nn.functional.dropout(torch.softmax(attn, 3) * start, p_drop, training=p_drop > 0)
    return (attn @ vh).transpose(1, 2).reshape(B * L, -1)


def bench_attention(B, H, L, p_drop, warmup, reps, inner):
    from evae import ops
    g = torch.Generator(device="cuda").manual_seed(B)
    q, k, v, go = (torch.randn(B * L, H * 4, device="cuda", generator=g).requires_grad_(i < 3) for i in range(4))

    def run(fn):
        out = fn()
        out.backward(go)
        q.grad = k.grad = v.grad = None

    variants = {"hip_fused": lambda: run(lambda: ops.causal_attn(q, k, v, B, L, H, p_drop)),
                "torch_composed": lambda: run(lambda: torch_attention(q, k, v, B, L, H, p_drop))}
    # same numbers without dropout (the two draw different masks)
    with torch.no_grad():
        diff = float((ops.causal_attn(q, k, v, B, L, H, 0.0) - torch_attention(q, k, v, B, L, H, 0.0)).abs().max())
    res = {"B": B, "H": H, "L": L, "dh": 4, "p_drop": p_drop, "max_abs_diff_forward_no_dropout": diff}
    peak = {}
    for name, fn in variants.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    times = {name: [] for name in variants}
    for _ in range(reps):                      # alternate the variants window by window
        for name, fn in variants.items():
            times[name].append(timed(fn, inner))
    for name in variants:
        res[name] = dict(stats(times[name]), peak_extra_mib=peak[name])
    res["speedup_median"] = res["torch_composed"]["median_ms"] / res["hip_fused"]["median_ms"]
    return res


def bench_step(B, warmup, reps):
    from argparse import Namespace
    from utils.optimizer import AdamNormGrad
    from utils.utils import importing_model
    N, C = 2000, 500
    args = Namespace(prior="exemplar_prior", input_type="binary", input_size=[1, 28, 28], hidden_size=300, z1_size=40, z2_size=40,
                     model_name="pixelcnn", device="cuda", number_components=C, training_set_size=N, approximate_prior=False,
                     approximate_k=10, no_mask=False, no_attention=False, same_variational_var=False, use_logit=False, lambd=1e-4,
                     bottleneck=6, dataset_name="dynamic_mnist", continuous=False, batch_size=B, dynamic_binarization=False,
                     warmup=100, S=50)
    torch.manual_seed(1)
    model = importing_model(args)(args).cuda().train()
    opt = AdamNormGrad(model.parameters(), lr=5e-4)
    rs = np.random.RandomState(2)
    data = torch.from_numpy((rs.rand(N, 784) < 0.13).astype(np.float32))
    ds = torch.utils.data.TensorDataset(data, torch.arange(N).reshape(-1, 1))
    batches = [(data[s:s + B].cuda(), torch.arange(s, s + B).reshape(-1, 1).cuda()) for s in range(0, N - B + 1, B)]
    state = {"i": 0, "loss": None}

    def step():
        x, idx = batches[state["i"] % len(batches)]
        state["i"] += 1
        opt.zero_grad()
        loss, _, _ = model.calculate_loss((x, idx), 1.0, average=True, dataset=ds)
        loss.backward()
        opt.step()
        state["loss"] = loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    first = float(state["loss"])
    torch.cuda.reset_peak_memory_stats()
    ms = [timed(step, 1) for _ in range(reps)]
    return dict(stats(ms), B=B, exemplars=C, dataset_rows=N, peak_allocated_mib=torch.cuda.max_memory_allocated() / 2 ** 20,
                loss_after_warmup=first, loss_last=float(state["loss"]), what="eager step: forward, backward, AdamNormGrad; dropout on")


def _step_args(B, N, C, use_graph):
    from argparse import Namespace
    return Namespace(prior="exemplar_prior", input_type="binary", input_size=[1, 28, 28], hidden_size=300, z1_size=40, z2_size=40,
                     model_name="pixelcnn", device="cuda", number_components=C, training_set_size=N, approximate_prior=False,
                     approximate_k=10, no_mask=False, no_attention=False, same_variational_var=False, use_logit=False, lambd=1e-4,
                     bottleneck=6, dataset_name="dynamic_mnist", continuous=False, batch_size=B, dynamic_binarization=False,
                     warmup=100, S=50, use_hip_graph=use_graph)


def step_leg(out_path, rounds):
    """captured against eager pixelcnn steps, epochs alternated (see the module docstring)"""
    import time
    from evae.graph import GraphedTrainStep
    from utils.optimizer import AdamNormGrad
    from utils.training import pixelcnn_step_eligible, train_one_epoch
    from utils.utils import importing_model
    N, C = 2000, 500
    rs = np.random.RandomState(2)
    data = torch.from_numpy((rs.rand(N, 784) < 0.13).astype(np.float32))
    ds = torch.utils.data.TensorDataset(data, torch.arange(N).reshape(-1, 1), torch.zeros(N))
    recs = []
    for B in (100, 10):
        steps = N // B
        loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False)
        paths = {}
        for name, use_graph in (("captured", True), ("eager", False)):
            a = _step_args(B, N, C, use_graph)
            assert pixelcnn_step_eligible(a), "this configuration is not one the captured pixelcnn step takes"
            torch.manual_seed(1)
            model = importing_model(a)(a).cuda()
            opt = AdamNormGrad(model.parameters(), lr=5e-4)
            paths[name] = (a, model, opt, [])
            train_one_epoch(1, a, loader, model, opt)                 # warm-up epoch: workspaces, the capture
        torch.cuda.synchronize()
        for r in range(rounds):
            for name in ("captured", "eager"):
                a, model, opt, ts = paths[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = train_one_epoch(2 + r, a, loader, model, opt)   # (ends in the read-back of the epoch's sums)
                ts.append((time.perf_counter() - t0) * 1e3 / steps)
                assert all(math.isfinite(v) for v in res)
        runner = list(paths["captured"][1]._graphed_steps.values())[0]
        assert runner.graph is not None and not runner.failed and runner.replays >= rounds * steps
        assert not getattr(paths["eager"][1], "_graphed_steps", None)
        rec = {"model": "pixelcnn", "B": B, "exemplars": C, "dataset_rows": N, "steps_per_epoch": steps, "epochs_timed": rounds,
               "replays": runner.replays}
        for name in ("captured", "eager"):
            ts = sorted(round(t, 4) for t in paths[name][3])
            rec[name + "_ms_per_step"] = ts
            rec[name + "_p50_ms"], rec[name + "_min_ms"], rec[name + "_max_ms"] = ts[len(ts) // 2], ts[0], ts[-1]
            rec[name + "_spread_ms"] = round(ts[-1] - ts[0], 4)
        rec["eager_over_captured_p50"] = round(rec["eager_p50_ms"] / rec["captured_p50_ms"], 4)
        rec["captured_ahead_by_more_than_eager_spread"] = bool(rec["eager_p50_ms"] - rec["captured_p50_ms"] > rec["eager_spread_ms"])
        del paths
        torch.cuda.empty_cache()
        # the node count: a runner of its own with the graph kept (the timed one is the default, unkept kind)
        try:
            GraphedTrainStep.keep_graph = True
            a = _step_args(B, N, C, True)
            torch.manual_seed(1)
            model = importing_model(a)(a).cuda().train()
            probe = GraphedTrainStep(model, AdamNormGrad(model.parameters(), lr=5e-4), ds, B, False)
            for k in range(probe.warmup_steps + 1):
                probe(data[k * B:(k + 1) * B], torch.arange(k * B, (k + 1) * B).reshape(-1, 1), 1.0)
            assert probe.graph is not None and not probe.failed and probe.replays == 1
            rec["graph_nodes"] = probe.node_count()
            del probe, model
        except Exception as e:                       # (a figure that could not be taken is reported as such, never guessed)
            rec["graph_nodes"] = "not measured: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:160])
        finally:
            GraphedTrainStep.keep_graph = False
        torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    out = {"tool": "tools/pixelsnail_bench.py --step", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": "host clock around train_one_epoch (loader included, ends in a read-back), one warm-up epoch per path, then %d "
                     "epochs per path alternated between the two; per-epoch ms per step sorted; p50, min, max, spread = max - min"
                     % rounds,
           "not_measured": ["kernel times under a profiler", "B above 100", "any prior other than the exact exemplar prior"],
           "step_cases": recs}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help="the captured-step leg alone -> profiles/pixelsnail_step.json")
    ap.add_argument("--rounds", type=int, default=9, help="--step: timed epochs per path")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixelsnail_bench needs a GPU: nothing is measured without one")
    if a.step:
        return step_leg(a.out or os.path.join(ROOT, "profiles", "pixelsnail_step.json"), a.rounds)
    a.out = a.out or os.path.join(ROOT, "profiles", "pixelsnail.json")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": "device events around work that ends in a synchronise; warm-up %d; median / min / max of %d windows; "
                     "attention variants alternate window by window" % (a.warmup, a.reps),
           "attention": [bench_attention(100, 8, 784, 0.1, a.warmup, a.reps, 3), bench_attention(10, 8, 784, 0.1, a.warmup, a.reps, 10)],
           "train_step": bench_step(100, a.warmup, a.reps)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
