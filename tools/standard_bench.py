#!/usr/bin/env python3
"""Standard-normal prior (--prior standard): ms per training step of `vae` at 784 / 300 / 40 with B = 100 on device-resident data.
GPU box only.  Two paths through train_one_epoch, alternated in one process after a warm-up epoch each:
  captured   the one-node step of evae/fused_std.py replayed from one hipGraph (the default);
  eager      the modular autograd path issued launch by launch (model._use_fused = False, use_hip_graph = False: what every
             standard-prior step was before the node existed).
Three timed epochs of 300 steps per path, host clock around an epoch that ends in a read-back; p50 and spread (max - min) of the
three per-epoch figures.  Also counts the launching C-ABI entry points of one captured-form step (issued eagerly through the
runner's step_eagerly: the launches the graph replays; the optimizer's entry is one launch pair).  Writes
profiles/standard_step.json (or the path given as the first argument) with the commit that ran."""
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))
import torch                                                    # noqa: E402
from evae import _lib                                           # noqa: E402

QUERIES = ("_bytes", "_applies", "_configure", "_ld", "_nks", "_nks_rows", "evae_version", "evae_last_error", "_images")


class DeviceLoader:
    """batches of a device-resident dataset in order (what a DataLoader over it hands out, without the host copies)"""

    def __init__(self, ds, batch_size):
        self.dataset, self.batch_size = ds, batch_size
        self.x, self.idx, self.y = (t.cuda() for t in ds.tensors)

    def __len__(self):
        return self.x.shape[0] // self.batch_size

    def __iter__(self):
        B = self.batch_size
        for s in range(0, len(self) * B, B):
            yield self.x[s:s + B], self.idx[s:s + B], self.y[s:s + B]


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return os.environ.get("EVAE_COMMIT", "unknown (no git metadata beside the tree that ran)")


def main():
    from argparse import Namespace
    from models.VAE import VAE
    from utils.optimizer import AdamNormGrad
    from utils.training import train_one_epoch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "standard_step.json")
    assert torch.cuda.is_available(), "standard_bench needs a GPU"
    B, D, steps, repeats = 100, 784, 300, 3
    N = B * steps
    g = torch.Generator(); g.manual_seed(26)
    x = (torch.rand(N, D, generator=g) < 0.2).float()
    ds = torch.utils.data.TensorDataset(x, torch.arange(N).reshape(-1, 1), torch.zeros(N))
    loader = DeviceLoader(ds, B)
    paths = {}
    for name, captured in (("captured", True), ("eager", False)):
        a = Namespace(prior="standard", input_type="binary", input_size=[1, 28, 28], hidden_size=300, z1_size=40, z2_size=40,
                      model_name="vae", device="cuda", number_components=1, training_set_size=N, approximate_prior=False,
                      approximate_k=10, no_mask=False, no_attention=False, same_variational_var=False, use_logit=False, lambd=1e-4,
                      bottleneck=6, dataset_name="dynamic_mnist", continuous=False, batch_size=B, dynamic_binarization=False,
                      warmup=100, S=50, use_hip_graph=captured)
        torch.manual_seed(7)
        model = VAE(a).cuda()
        model._use_fused = captured
        opt = AdamNormGrad(model.parameters(), lr=5e-4)
        paths[name] = (a, model, opt, [])
        train_one_epoch(1, a, loader, model, opt)                 # warm-up epoch: workspaces, the capture
    torch.cuda.synchronize()
    for r in range(repeats):
        for name in ("captured", "eager"):
            a, model, opt, ts = paths[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = train_one_epoch(2 + r, a, loader, model, opt)   # (ends in the read-back of the epoch's sums)
            ts.append((time.perf_counter() - t0) * 1e3 / steps)
            assert all(math.isfinite(v) for v in res)
    runner = list(paths["captured"][1]._graphed_steps.values())[0]
    assert runner.graph is not None and not runner.failed and runner.no_exemplars and runner.replays >= repeats * steps
    assert not getattr(paths["eager"][1], "_graphed_steps", None)
    # the launches of one captured-form step, by entry point
    xb, ib, _ = next(iter(loader))
    with _lib.count_calls("evae_") as counts:
        runner.step_eagerly(xb, ib, 1.0)
    torch.cuda.synchronize()
    launches = {k: v for k, v in sorted(counts.items()) if not k.endswith(QUERIES)}
    rec = {"tool": "tools/standard_bench.py", "device": torch.cuda.get_device_name(0), "commit": commit(), "model": "vae",
           "prior": "standard", "B": B, "layers": [D, 300, 40], "steps_per_epoch": steps, "epochs_timed": repeats,
           "timing": "host clock around train_one_epoch (device-resident batches, ends in a read-back), epochs alternated between "
                     "the two paths, ms per step",
           "replays": runner.replays, "captured_step_entry_points": launches, "captured_step_launching_calls": sum(launches.values())}
    for name in ("captured", "eager"):
        ts = sorted(round(t, 4) for t in paths[name][3])
        rec[name + "_ms_per_step"] = ts
        rec[name + "_p50_ms"], rec[name + "_spread_ms"] = ts[len(ts) // 2], round(ts[-1] - ts[0], 4)
    rec["captured_faster_by_more_than_the_spread"] = bool(
        rec["eager_p50_ms"] - rec["captured_p50_ms"] > max(rec["eager_spread_ms"], rec["captured_spread_ms"]))
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
