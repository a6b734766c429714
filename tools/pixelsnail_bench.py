#!/usr/bin/env python3
"""First measurements of the PixelSNAIL decoder (model_name 'pixelcnn') on the GPU -> profiles/pixelsnail.json.

  1. the fused causal-attention kernels (csrc/evae_attn.hip, forward + backward, dropout 0.1) against the same formula composed from
     torch ops on the same GPU (matmul, masked_fill(-1e4), softmax, start mask, dropout, matmul: reference utils/nn.py:351-359), at
     B = 100 and B = 10, H = 8, L = 784, dh = 4: time per forward+backward and peak memory of each variant;
  2. one eager training step of `pixelcnn` at B = 100 (exemplar prior, AdamNormGrad, dropout on).

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixelsnail.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixelsnail_bench needs a GPU: nothing is measured without one")
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
