#!/usr/bin/env python3
"""VampPrior log_p_z: the fused mixture kernels (evae.ops.mixture_logp, csrc/evae_mixture.hip) against the torch composition the
model used before them, restated below.  GPU box only.  Device events around the whole call (all launches of a path), the
two paths alternated inside one timed loop, median and quartiles of N calls per path; outputs of the two compared at the
sizes that are timed.  Writes profiles/vampprior_bench.json (or the path given as the first argument).
  (100, 500, 40), (100, 1000, 40): the training shapes, forward and forward + backward (gradients to z, means, log-variance)
  (20000, 500, 40): the evaluator's shape (utils/evaluation.py::IWAE_ROWS_PER_LAUNCH rows), forward only
  --step: ms per training step of `vae` + vampprior (B = 100, C = 500 and 1000, MNIST-sized layers) through train_one_epoch,
  replayed from the captured graph against use_hip_graph = False: nine epochs of 200 steps per path, alternated between the two
  after a warm-up epoch each (every epoch's figure is kept: median, min and max are reported), host clock around an epoch that ends in a read-back.  Added to the same JSON under "step_cases"."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))
import torch                                                    # noqa: E402
from evae import ops                                            # noqa: E402

LOG_2PI = math.log(2.0 * math.pi)


def torch_composition(z, mu, lv, n_components):
    """what models/BaseModel.py::log_p_z did for prior == 'vampprior' (utils.distributions.log_normal_diag over [B x C x z])"""
    zz, m, l = z.unsqueeze(1), mu.unsqueeze(0), lv.unsqueeze(0)
    prob = torch.sum(-0.5 * (l + LOG_2PI + torch.pow(zz - m, 2) / torch.exp(l)), 2) - math.log(n_components)
    pmax, _ = torch.max(prob, 1)
    return pmax + torch.log(torch.sum(torch.exp(prob - pmax.unsqueeze(1)), 1))


def timed_pair(fa, fb, n, warm=5):
    """alternate the two paths; (sorted microseconds of a, of b)"""
    for _ in range(warm):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(n):
        for fn, ts in ((fa, ta), (fb, tb)):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ta), sorted(tb)


def stats(ts):
    return {"median_us": round(ts[len(ts) // 2], 1), "q1_us": round(ts[len(ts) // 4], 1), "q3_us": round(ts[3 * len(ts) // 4], 1)}


def write_doc(out_path, **fields):
    doc = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc.update({"tool": "tools/vampprior_bench.py", "device": torch.cuda.get_device_name(0)})
    doc.update(fields)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def step_mode(out_path, steps=200, rounds=9):
    import time
    from argparse import Namespace
    from models.VAE import VAE
    from utils.optimizer import AdamNormGrad
    from utils.training import train_one_epoch
    B, D = 100, 784
    recs = []
    for C in (500, 1000):
        N = B * steps
        g = torch.Generator(); g.manual_seed(C)
        x = (torch.rand(N, D, generator=g) < 0.2).float()
        ds = torch.utils.data.TensorDataset(x, torch.arange(N).reshape(-1, 1), torch.zeros(N))
        loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False)
        paths = {}
        for name, use_graph in (("captured", True), ("eager", False)):
            a = Namespace(prior="vampprior", input_type="binary", input_size=[1, 28, 28], hidden_size=300, z1_size=40, z2_size=40,
                          model_name="vae", device="cuda", number_components=C, training_set_size=N, approximate_prior=False,
                          approximate_k=10, no_mask=False, no_attention=False, same_variational_var=False, use_logit=False, lambd=1e-4,
                          bottleneck=6, dataset_name="dynamic_mnist", continuous=False, batch_size=B, dynamic_binarization=False,
                          warmup=100, S=50, pseudoinputs_mean=0.05, pseudoinputs_std=0.01, use_training_data_init=False,
                          use_hip_graph=use_graph)
            torch.manual_seed(7)
            model = VAE(a).cuda()
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
        rec = {"model": "vae", "B": B, "C": C, "steps_per_epoch": steps, "epochs_timed": rounds,
               "captured_ms_per_step": sorted(round(t, 4) for t in paths["captured"][3]),
               "eager_ms_per_step": sorted(round(t, 4) for t in paths["eager"][3]), "replays": runner.replays}
        for name in ("captured", "eager"):
            ts = rec[name + "_ms_per_step"]
            rec[name + "_median_ms"], rec[name + "_min_ms"], rec[name + "_max_ms"] = ts[rounds // 2], ts[0], ts[-1]
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    write_doc(out_path, step_timing="host clock around train_one_epoch (200 steps, loader included, ends in a read-back), epochs "
              "alternated between the two paths, per-epoch ms per step sorted, median", step_cases=recs)


def main():
    out_path = os.path.join(ROOT, "profiles", "vampprior_bench.json")
    argv = [a for a in sys.argv[1:] if a != "--step"]
    if argv:
        out_path = argv[0]
    assert torch.cuda.is_available(), "vampprior_bench needs a GPU"
    if "--step" in sys.argv[1:]:
        return step_mode(out_path)
    recs = []
    for B, C, Z, with_bwd, n in ((100, 500, 40, True, 200), (100, 1000, 40, True, 200), (20000, 500, 40, False, 20)):
        g = torch.Generator(device="cuda"); g.manual_seed(B + C)
        centre = torch.randn(10, Z, device="cuda", generator=g)
        z = centre[torch.randint(0, 10, (B,), device="cuda", generator=g)] + 0.35 * torch.randn(B, Z, device="cuda", generator=g)
        mu = centre[torch.randint(0, 10, (C,), device="cuda", generator=g)] + 0.35 * torch.randn(C, Z, device="cuda", generator=g)
        lv = torch.rand(C, Z, device="cuda", generator=g) * 8.0 - 6.0
        gout = torch.randn(B, device="cuda", generator=g)
        rec = {"B": B, "C": C, "z": Z, "pair_dims": B * C * Z}
        try:
            with torch.no_grad():
                a, b = ops.mixture_logp(z, mu, lv, C), torch_composition(z, mu, lv, C)
                rec["fwd_max_abs_diff"] = float((a - b).abs().max())
                ta, tb = timed_pair(lambda: ops.mixture_logp(z, mu, lv, C), lambda: torch_composition(z, mu, lv, C), n)
            rec["fwd_hip"], rec["fwd_torch"] = stats(ta), stats(tb)
        except torch.cuda.OutOfMemoryError as e:
            rec["fwd_torch"] = "does not fit: %s" % str(e).split("\n")[0]
            torch.cuda.empty_cache()
            with torch.no_grad():
                ta, _ = timed_pair(lambda: ops.mixture_logp(z, mu, lv, C), lambda: None, n)
            rec["fwd_hip"] = stats(ta)
        if with_bwd:
            leaves = [t.clone().requires_grad_(True) for t in (z, mu, lv)]

            def fb(fn):
                def run():
                    return torch.autograd.grad((fn(*leaves, C) * gout).sum(), leaves)
                return run
            ga, gb = fb(ops.mixture_logp)(), fb(torch_composition)()
            rec["bwd_max_rel_diff"] = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(ga, gb)]
            ta, tb = timed_pair(fb(ops.mixture_logp), fb(torch_composition), n)
            rec["fwd_bwd_hip"], rec["fwd_bwd_torch"] = stats(ta), stats(tb)
        else:
            rec["fwd_bwd_torch"] = "not measured: forward only at the evaluator's shape"
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    write_doc(out_path, timing="device events around the call, paths alternated, median / quartiles", cases=recs)


if __name__ == "__main__":
    main()
