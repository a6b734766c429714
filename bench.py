#!/usr/bin/env python3
"""Headline benchmark: training images/sec of `vae` + exemplar prior, dynamic_mnist-shaped synthetic
data, 25 000 exemplars, exact prior, batch 100 (BASELINE.json configs[1]).

A step is the body of the reference's training loop (utils/training.py:27-46): binarise the batch,
forward, sample + encode the C exemplars, exemplar prior, backward, AdamNormGrad -- all through the
drop-in API (models.VAE.VAE.calculate_loss -> loss.backward() -> utils.optimizer.AdamNormGrad.step),
i.e. through libevae_hip.so.  With --gpus N > 1 (launched by torch.distributed.run, one rank per GPU,
RCCL) the C exemplars are sharded across the ranks and the per-shard partial log-sum-exps are merged
(evae/shard.py, evae/fused_vae.py).  Default (--parallel replica, the split BASELINE.json's north_star names): the SAME
100-image batch on every rank, the 25 000 exemplars sharded N ways, one all-gather of the packed partial log-sum-exps
per step -- total work fixed, "strong" scaling.  The same line carries, as the nested object "dp", the data-parallel
measurement (--parallel dp): every rank trains on its OWN 100-image batch -- global batch 100 N, gradients averaged,
each rank scores the queries of all ranks against its exemplar shard and the partials return to their owners ("weak").

Prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype, ms_per_step = wall time of the --steps timed
steps / --steps).  A plain run sets up, warms up, times the steps and prints; --full adds what takes runs of its own:
  roofline     -- the dominant kernel (the fp32-MFMA GEMM behind GatedDense), algorithmic flops per
                  launch / mean launch duration measured with HIP events on eager probe steps after the timed region,
                  and inside the replayed graph from a child run under rocprofv3
  cpu_baseline -- the numpy oracle's train step (oracle/evae_oracle.py) timed on the host cores
  test_log_px, amdahl_ceiling, dp -- the IWAE evaluator, a child run at 200 exemplars, the data-parallel leg of --gpus N
--dump-outputs DIR writes the last timed step's (loss, -RE, KL) and the updated parameters as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))
sys.path.insert(1, os.path.join(ROOT, "tests"))          # golden_inputs: the synthetic-data generator

import numpy as np
import torch
import torch.distributed as dist

PEAK_FP32_MFMA_TFLOPS = 157.3        # /opt/skills/guides/MI355X_MICROARCH.md, dense fp32 MFMA
PEAK_BF16_MFMA_TFLOPS = 2500.0      # same guide: dense bf16 MFMA (no sparsity)
PEAK_HBM_GBS = 8000.0                # same guide: HBM3E
B, C, N_TRAIN, D, H, Z = 100, 25000, 50000, 784, 300, 40
# the MLP configurations that run through main(): model, exemplars, training-set size
MLP_CONFIGS = {"c1": ("vae", 1000, 50000), "c2": ("vae", 25000, 50000), "c4": ("hvae_2level", 11500, 23000),
               # c2 with the kNN-approximate prior (reference models/BaseModel.py:256-271): 25 000 candidates per step, top-10 of
               # every batch row among their cached latents, the B * k = 1000 slots re-encoded
               "c2a": ("vae", 25000, 50000)}
# untimed 10-step windows of replays in front of the timed region: a fixed count (the most the earlier stop-when-two-windows-agree
# rule ever took), so that the steps in front of the last timed one -- and with them its outputs -- do not depend on timing
RAMP_WINDOWS = 4
DUMP_BYTES = 64 << 20                 # --dump-outputs: the most it writes in all


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", default="c2", choices=("c1", "c2", "c2a", "c3", "c4", "c5", "iwae", "topk"),
                    help="BASELINE.json configuration (default c2 = the one the metric is quoted on): c1 vae C=1000; c2 vae "
                         "C=25000; c3 convhvae_2level C=25000; c4 hvae_2level C=11500 (N=23000); c5 single_conv 3x64x64, z=256, "
                         "approximate prior over 100 000 cached latents; iwae = the test log p(x) evaluator at c2 sizes; "
                         "topk = the cache + top-K scan at c2 and c5 sizes.  Every config prints the same JSON line with its "
                         "own roofline object.")
    ap.add_argument("--exemplars", type=int, default=None)
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a hipGraph")
    ap.add_argument("--parallel", choices=("replica", "dp"), default="replica",
                    help="with --gpus N > 1: 'replica' (default, BASELINE.json's north_star split) = the same 100-image batch on "
                         "every rank, only the 25 000 exemplars sharded: fixed total work, 'strong' scaling; 'dp' = every rank "
                         "trains on its own 100-image batch (global batch 100 N) against the sharded exemplar set ('weak' in "
                         "the batch).  The replica line carries the dp measurement as a nested object (--no-dp-line skips it).")
    ap.add_argument("--no-dp-line", action="store_true", help="with --gpus N > 1: do not run the second (dp) measurement")
    ap.add_argument("--no-amdahl", action="store_true", help="skip the amdahl_ceiling object (a second process at 200 exemplars)")
    ap.add_argument("--no-graph-profile", action="store_true",
                    help="headline line only: do not run the child process under rocprofv3 that times the kernels INSIDE the replayed graph")
    ap.add_argument("--no-ramp", action="store_true",
                    help="skip the untimed clock-ramp replays in front of the timed region (%d 10-step windows)" % RAMP_WINDOWS)
    ap.add_argument("--probe-warmup", type=int, default=20,
                    help="untimed eager steps in front of the probe steps (clock ramp after the host pause)")
    ap.add_argument("--probe-steps", type=int, default=20,
                    help="eager steps run after the timed region to time the dominant kernel with HIP events")
    ap.add_argument("--iwae-images", type=int, default=100,
                    help="test images for the IWAE test log p(x) leg (S=5000 samples each vs all 50 000 exemplars); 0 disables")
    ap.add_argument("--cpu-baseline-steps", type=int, default=80,
                    help="oracle steps timed for cpu_baseline (0 disables)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure: the roofline objects (eager probe steps, the child run "
                         "under rocprofv3), the CPU baselines, the IWAE leg, the amdahl_ceiling child and the nested dp measurement of "
                         "--gpus N.  Off: set up, warm up, time --steps steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, "
                         "at most 64 MB in all); same arguments, same inputs, run to run")
    return ap.parse_args()


def model_args(device, n_exemplars, sharded, shard_batch=False, model_name="vae", n_train=N_TRAIN):
    from argparse import Namespace
    return Namespace(prior="exemplar_prior", input_type="binary", input_size=[1, 28, 28], hidden_size=H,
                     z1_size=Z, z2_size=Z, model_name=model_name, device=device, number_components=n_exemplars,
                     training_set_size=n_train, approximate_prior=False, approximate_k=10, no_mask=False,
                     no_attention=False, same_variational_var=False, use_logit=False, lambd=1e-4,
                     bottleneck=6, dataset_name="dynamic_mnist", continuous=False, batch_size=B,
                     dynamic_binarization=True, warmup=100, S=5000, shard_exemplars=sharded, shard_batch=shard_batch)


def gated_flops(M, K, N):
    return 2.0 * M * K * 2 * N


def step_flops(model_name, n_ex, enc_rows=None):
    """Algorithmic flops of one training step: vae = C x 3.03 MFLOP + B x 5.7 MFLOP + 6 B C z.  enc_rows: the exemplar
    rows the encoder really runs over (a captured step encodes the DISTINCT rows of the draw: fewer flops, not a faster rate)."""
    if model_name != "vae":
        return None
    return (n_ex if enc_rows is None else enc_rows) * 3.0336e6 + B * 5.7e6 + 6.0 * B * n_ex * Z


def cpu_baseline(steps, C=C, N_TRAIN=N_TRAIN):
    """The oracle's restatement of the same training step on the host cores (numpy + its BLAS threads).  More BLAS
    threads are not faster on these hosts (64 threads: 170-180 images/s, 16 threads: 560-630 on the 2 x 64-core box), so
    a short calibration picks the thread count and `cores` reports the one used."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import evae_oracle as orc
    import golden_inputs as gi
    try:
        from threadpoolctl import threadpool_limits
    except Exception:                                   # no control over the BLAS pool: time it as it comes
        threadpool_limits = None
    rs = np.random.RandomState(0)
    data = gi.binary_images(0, N_TRAIN)
    state = {"p": orc.vae_init_params(np.random.RandomState(123)), "opt": {}, "s": 0}

    def one_step():
        s = state["s"]; state["s"] += 1
        bidx = np.arange(s * B, (s + 1) * B).reshape(-1, 1) % N_TRAIN
        x = data[bidx[:, 0]]
        eps = rs.standard_normal((B, Z)).astype(np.float32)
        ex_idx = rs.randint(0, N_TRAIN, size=(C,))
        t0 = time.perf_counter()
        orc.vae_train_step(state["p"], state["opt"], x, bidx, eps, data[ex_idx], ex_idx, beta=0.5)
        return time.perf_counter() - t0

    one_step()                                          # warms the BLAS threads / page faults
    threads, note = os.cpu_count(), ""
    if threadpool_limits is not None:
        best = None
        for nt in sorted({min(os.cpu_count(), n) for n in (64, 32, 16, 8)}, reverse=True):
            with threadpool_limits(limits=nt):
                dt = min(one_step(), one_step())
            if best is None or dt < best[0]:
                best = (dt, nt)
        threads = best[1]
        note = "; BLAS threads chosen by a 2-step calibration over 64/32/16/8"
    t_tot = 0.0
    ctx = threadpool_limits(limits=threads) if threadpool_limits is not None else None
    if ctx is not None:
        ctx.__enter__()
    try:
        for _ in range(steps):
            t_tot += one_step()
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return {"value": round(B * steps / t_tot, 2), "unit": "images/sec", "cores": threads,
            "kind": "port",
            "sample": "%d steps of the numpy oracle's vae train step (B=%d, C=%d, N=%d) on %d BLAS threads of a %d-CPU host%s"
                      % (steps, B, C, N_TRAIN, threads, os.cpu_count(), note)}


def graph_kernel_stats(steps=60):
    """Durations of the kernels INSIDE the replayed hipGraph: HIP event pairs cannot be read back from a replay, so a child process
    runs the same headline step under `rocprofv3 --kernel-trace --stats` (the command whose summary is committed under profiles/) and
    its per-kernel averages come back: {kernel name: (calls, average us)}, or (None, why not)."""
    import csv, glob, shutil, subprocess, tempfile
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rp):
        return None, "rocprofv3 not found"
    if any(k.startswith(("ROCPROFILER_", "ROCP_", "ROCPROF_")) for k in os.environ):
        return None, "this process is itself running under a profiler"
    d = tempfile.mkdtemp(prefix="evae_graphprof_", dir="/tmp")
    cmd = [rp, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "g", "--", sys.executable, os.path.abspath(__file__),
           "--config", "c2", "--steps", str(steps), "--warmup", "10", "--no-amdahl", "--cpu-baseline-steps", "0", "--iwae-images", "0",
           "--probe-steps", "0", "--probe-warmup", "0", "--no-graph-profile"]
    try:
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=300, capture_output=True, text=True)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return None, "rocprofv3 child failed (rc %d)" % r.returncode
        line_ = next((l for l in r.stdout.splitlines() if l.startswith("{")), None)
        ms = json.loads(line_)["ms_per_step"] if line_ else None
        out = {}
        for row in csv.DictReader(open(files[0])):
            out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
        return out, {"command": "rocprofv3 --kernel-trace --stats -- python bench.py --config c2 --steps %d --warmup 10 (no probe, no baselines)" % steps,
                     "ms_per_step_under_the_profiler": ms}
    except Exception as e:
        return None, "%s: %s" % (type(e).__name__, str(e)[:120])
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _blas_limit(n):
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=n)
    except Exception:
        import contextlib
        return contextlib.nullcontext()


def cpu_baseline_topk(q, cache, k, seconds=8.0):
    """The oracle's restatement of models/BaseModel.py:263-264 (fp64 expanded distance + ordered top-k) on the host, on as many of
    the bench's queries as fit the time budget (at least 4)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import evae_oracle as orc
    qn, cn = q.cpu().numpy(), cache.cpu().numpy()
    threads = min(os.cpu_count(), 16)
    with _blas_limit(threads):
        orc.nearest_exemplars_topk(qn[:2], cn, k)
        done, t_tot = 0, 0.0
        while done < len(qn) and (t_tot < seconds or done < 4):
            t0 = time.perf_counter()
            orc.nearest_exemplars_topk(qn[done:done + 4], cn, k)
            t_tot += time.perf_counter() - t0; done += 4
    return {"value": round(done / t_tot, 2), "unit": "queries/sec", "cores": threads, "kind": "port",
            "sample": "%d of the %d queries against all %d x %d cached latents through the numpy oracle (evae_oracle.nearest_exemplars_topk: "
                      "float64 distances + ordered top-%d), %d BLAS threads of a %d-CPU host" % (done, len(qn), cn.shape[0], cn.shape[1], k, threads, os.cpu_count())}


def cpu_baseline_iwae(n_images, S, n_train, seconds=20.0):
    """utils/evaluation.py:72-103 restated with the oracle's functions on the host: per test image S importance samples through
    encoder, decoder, log q and the exemplar prior over all n_train cached latents, log-mean-exp.  As many images as fit the budget."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import evae_oracle as orc
    import golden_inputs as gi
    p = orc.vae_init_params(np.random.RandomState(123))
    data = gi.binary_images(0, n_train)
    test = gi.binary_images(2, max(n_images, 1))
    rs = np.random.RandomState(5)
    threads = min(os.cpu_count(), 16)
    with _blas_limit(threads):
        centres, clv, _ = orc.vae_q_z(p, data, prior=True)
        cidx = np.arange(n_train)
        done, t_tot = 0, 0.0
        while done < n_images and (t_tot < seconds or done < 1):
            t0 = time.perf_counter()
            acc = []
            for s0 in range(0, S, 500):                 # the reference's own mini-batches of S (utils/evaluation.py:86-93)
                x = np.repeat(test[done:done + 1], 500, axis=0)
                eps = rs.standard_normal((500, Z)).astype(np.float32)
                r = orc.vae_calculate_loss(p, x, None, eps, ("embedding", centres, clv, cidx), training=False)
                acc.append(-r["loss"])
            a_ = np.concatenate(acc).astype(np.float64)
            _ = a_.max() + np.log(np.exp(a_ - a_.max()).mean())
            t_tot += time.perf_counter() - t0; done += 1
    return {"value": round(done / t_tot, 4), "unit": "images/sec", "cores": threads, "kind": "port",
            "sample": "%d test image(s), S = %d importance samples each against all %d cached latents, through the numpy oracle's vae functions "
                      "(%d BLAS threads of a %d-CPU host; the real reference in the build container: 5.81 s per image on 8 cores, "
                      "bench/ref_cpu_container.json)" % (done, S, n_train, threads, os.cpu_count())}


NO_PORT = ("no CPU port of this model exists: the numpy oracle restates the `vae` path (SURVEY 8c); %s is held to goldens generated by "
           "importing the real reference (tests/golden, tools/gen_goldens.py) and to float64 torch restatements inside the tests, neither "
           "of which may be imported by bench.py.  The reference itself cannot travel to the GPU box")


def pmc_traffic(name, expect=None):
    """HBM bytes per launch of a named kernel from the committed PMC passes (profiles/<round>_pmc/<name>.json, written by
    tools/profile_collect.py from `rocprofv3 --pmc` runs of the same launch): counters cannot be read from inside the
    process, so the bench line carries the file's number and says where it came from.  expect: the kernel symbol the launch
    this number is attached to runs -- a file whose pass profiled another kernel is refused (VERDICT r03 weak #3a: the
    dominant launch once carried the counters of a different template instance)."""
    for rnd in ("r06_pmc", "r05_pmc", "r04_pmc", "r03_pmc", "r02_pmc"):
        path = os.path.join(ROOT, "profiles", rnd, str(name) + ".json")
        if os.path.exists(path):
            try:
                d = json.load(open(path))
            except Exception:
                continue
            if expect is not None and expect not in str(d.get("kernel_symbol", d.get("kernel", ""))):
                return None, "refused: profiles/%s/%s.json profiled `%s`, this launch runs `%s`" % (rnd, name, d.get("kernel"), expect)
            return (d.get("hbm_bytes_per_launch"),
                    "file:profiles/%s/%s.json (rocprofv3 --pmc of `%s`%s, not measured in this run)"
                    % (rnd, name, d.get("kernel"), (" at commit " + d["commit"][:12]) if d.get("commit") else ""))
    return None, None


def pmc_rows(name):
    """exemplar rows the committed PMC pass of `name` ran at (None: no file / an older file without the field = 25 000)"""
    for rnd in ("r06_pmc", "r05_pmc", "r04_pmc", "r03_pmc", "r02_pmc"):
        path = os.path.join(ROOT, "profiles", rnd, str(name) + ".json")
        if os.path.exists(path):
            try:
                return int(json.load(open(path)).get("rows", 25000))
            except Exception:
                return None
    return None


FABRIC_BOUND_BPS = 5e12     # counter bytes / launch time at or above this: the launch sits at the memory fabric, not the matrix pipe


def bound_label(traffic_bytes, us, default="mfma"):
    """'fabric' when the PMC pass of this launch moved >= 5 TB/s through HBM / the L2-miss path (such a
    launch is traffic-bound whatever its flop count says), else the pipe it computes on."""
    if traffic_bytes and us and traffic_bytes / (us * 1e-6) >= FABRIC_BOUND_BPS:
        return "fabric"
    return default


def mfma_roofline(kern, flops, executed, pipe, us, traffic, tsrc, **more):
    """achieved = ALGORITHMIC flops per launch / mean launch time, frac = achieved / dense peak of the pipe the
    launch computes on.  The flops actually issued to that pipe (3 x / 6 x algorithmic for the byte / split-bf16 kernels) are
    reported separately as pipe_busy_frac -- an occupancy figure that agrees with SQ_VALU_MFMA_BUSY_CYCLES, not a roofline
    fraction."""
    peak = PEAK_BF16_MFMA_TFLOPS if pipe == "bf16-mfma" else PEAK_FP32_MFMA_TFLOPS
    tf = flops / us / 1e6
    r = {"bound": bound_label(traffic, us), "kernel": kern, "achieved": round(tf, 2), "peak": peak, "unit": "TFLOP/s",
         "frac": round(tf / peak, 4), "pipe": pipe, "pipe_busy_frac": round(executed / us / 1e6 / peak, 4),
         "executed_tflops": round(executed / us / 1e6, 2), "frac_of_fp32_mfma_peak": round(tf / PEAK_FP32_MFMA_TFLOPS, 4),
         "traffic": traffic, "traffic_source": tsrc, "avg_launch_us": round(us, 2), "flops_per_launch": round(flops)}
    r.update(more)
    return r


def time_launches(fn, reps=4, pairs=12, warm=6):
    """Mean duration (us) of one call of fn: `reps` back-to-back calls between one HIP event pair (amortises the pair's own
    ~5 us), `pairs` pairs, after `warm` untimed calls (clock ramp)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(pairs):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return 1e3 * sum(a.elapsed_time(b) for a, b in evs) / (pairs * reps)


def line(metric, value, unit, a, dt, workload, roof, extra=None, world=1, launch="eager"):
    out = {"metric": metric, "value": value, "unit": unit, "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": round(1e3 * dt / a.steps, 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic", "config": {"workload": workload, "launch": launch}, "roofline": roof,
           "cpu_baseline": None}
    out.update(extra or {})
    return out


def dump_outputs(d, arrays):
    """--dump-outputs: one d/<name>.npy per array, float64 for float64 and integer arrays, float32 otherwise.  When the files
    would together exceed DUMP_BYTES, every array over an equal share of it is replaced by a fixed sample of its flattened elements
    (positions drawn without replacement by numpy's RandomState(0), ascending), so two runs write the same elements."""
    os.makedirs(d, exist_ok=True)
    out = {}
    for name, v in arrays.items():
        v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        out[name] = v.astype(np.float64 if (v.dtype == np.float64 or v.dtype.kind in "iub") else np.float32)
    room = DUMP_BYTES - 256 * len(out)          # (each file's .npy header)
    if sum(v.nbytes for v in out.values()) > room:
        share = room // len(out)
        for name, v in out.items():
            if v.nbytes > share:
                k = share // v.itemsize
                out[name] = v.reshape(-1)[np.sort(np.random.RandomState(0).choice(v.size, k, replace=False))]
    for name, v in out.items():
        np.save(os.path.join(d, name + ".npy"), v)


def step_arrays(model, out3):
    """What a training step hands its caller: (loss, -RE, KL) of the step (GraphedTrainStep's return value) and the parameters
    after the optimizer's update."""
    arr = {} if out3 is None else {"loss_negre_kl": out3}
    arr.update(("param." + n, p) for n, p in model.named_parameters())
    return arr


def conv_roofline(a, c5, runner, n_ex):
    """--full, c3 / c5: the dominant kernel, timed with HIP events at the shape it has in the step."""
    from evae import ops
    with torch.no_grad():
        if c5:
            # a residual block of the decoder (96 channels, 32 x 32, the batch's 100 images) as the step launches it: the window
            # kernel over pixel images with bias + residual + the next block's ELU image in the epilogue (csrc/evae_conv_win.h)
            nimg, ci, co, k_, hw = B, 96, 96, 3, 32
            pr = ops.res_window_probe(nimg, ci, hw, k_)
            us = time_launches(pr["fwd"], reps=4)
            us_d = time_launches(pr["dgrad"], reps=4)
            us_w = time_launches(pr["wgrad"], reps=4)
            del pr
            flops = 2.0 * nimg * hw * hw * ci * k_ * k_ * co
            kern = ("residual block 96 -> 96, 3x3, 32 x 32, %d images on pixel images (evae_cw_res_fwd: conv_win_kernel<3, 4, 2, 576>, "
                    "bias + residual + ELU image in the epilogue)" % nimg)
        else:
            # the gated 5 x 5 layer of q_z_layers over the exemplar images the step encodes, as the stack launches it: the window
            # kernel over pre-split pixel images (csrc/evae_conv_win.h)
            dd0 = getattr(runner, "dedup", None) if runner is not None else None
            nimg, ci, co, k_, hw = (dd0["cap"] if dd0 else n_ex), 32, 64, 5, 14
            pr = ops.conv_window_probe(nimg, ci, hw, co, k_, 1, out_planar=True)
            us = time_launches(pr["fwd"], reps=2)
            us_d = time_launches(pr["dgrad"], reps=2)
            us_w = time_launches(pr["wgrad"], reps=2)
            del pr
            flops = 2.0 * nimg * hw * hw * ci * k_ * k_ * 2 * co
            kern = ("gated conv 32 -> 64, 5x5, 14 x 14, %d images on pixel images (evae_cw_fwd_gated: conv_win_kernel<0, 2, 2, 320>, input "
                    "window resident in LDS, gate + output image in the epilogue)" % nimg)
    traffic, tsrc = pmc_traffic("res96_fwd" if c5 else "cw5_fwd", expect="conv_win_kernel<3, 4, 2, 576>" if c5 else "conv_win_kernel<0, 2, 2, 320>")
    roof = mfma_roofline(kern, flops, 6.0 * flops, "bf16-mfma", us, traffic, tsrc)
    if c5:
        roof["kernels"] = [
            {"launch": "its data gradient dx = dy + ELU'(x) conv_transpose(dy, w) (evae_cw_res_bwd_data: conv_win_kernel<4, 4, 2, 576>)",
             "us": round(us_d, 1), "frac": round(flops / us_d / 1e6 / PEAK_BF16_MFMA_TFLOPS, 4)},
            {"launch": "its weight gradient over pixel images (evae_cw_bwd_weight_plain: conv_wgrad_win_kernel<9, 224, 8, 2, false> x 3 channel-group pairs + finish)",
             "us": round(us_w, 1), "frac": round(flops / us_w / 1e6 / PEAK_BF16_MFMA_TFLOPS, 4)}]
    else:
        roof["kernels"] = [
            {"launch": "data gradient + gate derivative of the layer below (evae_cw_bwd_data_gate: conv_win_kernel<1, 4, 1, 576>)",
             "us": round(us_d, 1), "frac": round(flops / us_d / 1e6 / PEAK_BF16_MFMA_TFLOPS, 4)},
            {"launch": "weight gradient over pixel images (evae_cw_bwd_weight: conv_wgrad_win_kernel<13 | 12, 192, 8, 1, false> + finish)",
             "us": round(us_w, 1), "frac": round(flops / us_w / 1e6 / PEAK_BF16_MFMA_TFLOPS, 4)}]
    return roof


def other_config(a, dev, rank, world, rccl_ranks=1, backend=None):
    """c3 / c5 (the convolutional configurations), iwae (the test log p(x) evaluator), topk (cache + top-K): the same JSON
    line as the headline, each with the roofline object of ITS dominant kernel.  Single GPU."""
    assert world == 1 or a.config == "iwae", "--config %s runs on one GPU" % a.config
    from argparse import Namespace
    import golden_inputs as gi
    from evae import ops
    torch.manual_seed(14); torch.cuda.manual_seed(14)
    if a.config in ("c3", "c5"):
        from utils.utils import importing_model
        from utils.optimizer import AdamNormGrad
        from evae.graph import GraphedTrainStep
        c5 = a.config == "c5"
        n_train = 100000 if c5 else N_TRAIN
        n_ex = a.exemplars if a.exemplars is not None else (100000 if c5 else C)
        isz = [3, 64, 64] if c5 else [1, 28, 28]
        args = Namespace(prior="exemplar_prior", input_type="continuous" if c5 else "binary", input_size=isz, hidden_size=H,
                         z1_size=256 if c5 else Z, z2_size=Z, model_name="single_conv" if c5 else "convhvae_2level",
                         device=str(dev), number_components=n_ex, training_set_size=n_train, approximate_prior=c5,
                         approximate_k=10, no_mask=False, no_attention=False, same_variational_var=False, use_logit=False,
                         lambd=1e-4, bottleneck=1, dataset_name="celeba" if c5 else "fashion_mnist", continuous=c5, batch_size=B,
                         dynamic_binarization=False, warmup=100, S=5000, shard_exemplars=False, shard_batch=False)
        model = importing_model(args)(args).to(dev)
        opt = AdamNormGrad(model.parameters(), lr=5e-4)
        Dn = isz[0] * isz[1] * isz[2]
        if c5:       # 100 000 x 12 288 floats = 4.9 GB: generated on the device, handed to the model as its resident copy
            data_dev = (torch.randint(0, 256, (n_train, Dn), device=dev, dtype=torch.int16).float() + 0.5) / 256
            dataset = torch.utils.data.TensorDataset(data_dev, torch.arange(n_train).reshape(-1, 1), torch.zeros(n_train))
        else:
            data = torch.from_numpy(gi.binary_images(0, n_train))
            dataset = torch.utils.data.TensorDataset(data, torch.arange(n_train).reshape(-1, 1), torch.zeros(n_train))
        data_dev = model.resident_data(dataset)
        idx_all = torch.arange(n_train, device=dev).reshape(-1, 1)
        model.train()
        cache = None
        if c5:
            with torch.no_grad():
                cache = tuple(model.cache_z(dataset))
        # c5: the approximate prior of a convolutional model stays on eager launches: its `unique` leaves ~100 images to re-encode
        # (after the first step the refreshed cache rows share their neighbours), the B * k = 1000 static slots of a captured step
        # re-encode all 1000 -- r03: 45.3 ms/step replayed (EVAE_C5_GRAPH=1) against 23 ms of GPU work eager
        eager_c5 = c5 and os.environ.get("EVAE_C5_GRAPH", "0") == "0"
        runner = None if (eager_c5 or a.no_graph) else GraphedTrainStep(model, opt, dataset, B, False)
        if runner is not None and cache is not None:
            cache = runner.set_cache(cache)       # static buffers: the captured launches read and refresh them in place

        last = [None]                            # the eager step's (loss, RE, KL): --dump-outputs

        def step(i):
            s_ = (i * B) % (n_train - B)
            if runner is not None:
                return runner(data_dev[s_:s_ + B], idx_all[s_:s_ + B], 0.5)
            opt.zero_grad()
            loss, RE, KL = model.calculate_loss((data_dev[s_:s_ + B], idx_all[s_:s_ + B]), 0.5, average=True, cache=cache,
                                                dataset=dataset)
            loss.backward()
            opt.step()
            last[0] = (loss, RE, KL)
        for i in range(a.warmup):
            step(i)
        torch.cuda.synchronize()
        out3 = None
        t0 = time.perf_counter()
        for i in range(a.steps):
            out3 = step(a.warmup + i)
        t_issue = time.perf_counter() - t0       # the host has issued every launch (eager legs: is the step host-bound?)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if a.dump_outputs:
            if out3 is None and last[0] is not None:
                loss, RE, KL = (t_.detach().reshape(()) for t_ in last[0])
                out3 = torch.stack((loss, -RE, KL))
            dump_outputs(a.dump_outputs, step_arrays(model, out3))
        roof = conv_roofline(a, c5, runner, n_ex) if a.full else None
        wl = ("single_conv (fully_conv) + exemplar_prior, 3x64x64 continuous, z=256, approximate prior: top-10 over %d cached "
              "latents, <= 1000 exemplars re-encoded per step, batch %d (BASELINE.json configs[4], one GPU)" % (n_ex, B)) if c5 else \
             ("convhvae_2level + exemplar_prior, fashion_mnist-shaped binary 28x28, N=%d, batch %d, %d exemplars, exact prior "
              "(BASELINE.json configs[2])" % (n_train, B, n_ex))
        dd_ = getattr(runner, "dedup", None) if runner is not None else None
        ex_rows = None if not dd_ else {
            "drawn": n_ex, "encoded_per_step": dd_["cap"], "distinct_in_the_last_step": dd_["distinct"],
            "note": "the exemplars are drawn WITH replacement (reference models/BaseModel.py:245); the captured step encodes the distinct "
                    "images of the draw once (a fixed %d rows, padded with multiplicity 0), the prior sees every draw (ops.ExpandRowsFn); same "
                    "loss and gradients as encoding every draw (tests/test_gpu_model.py::"
                    "test_graphed_modular_step_over_distinct_exemplar_rows_matches_eager); EVAE_DEDUP=0 encodes every draw.  The roofline "
                    "kernel below is timed at all %d images" % (dd_["cap"], n_ex)}
        print(json.dumps(line("training images/sec", round(B * a.steps / dt, 1), "images/sec", a, dt, wl, roof,
                              extra={"exemplar_rows": ex_rows, "host_issue_ms_per_step": round(1e3 * t_issue / a.steps, 3),
                                     "cpu_baseline": None,
                                     "cpu_baseline_reason": NO_PORT % ("single_conv (fully_conv)" if c5 else "convhvae_2level")},
                              launch="eager" if runner is None or runner.graph is None else "hipGraph replay of the whole step")))
        return
    if a.config == "iwae":
        from models.VAE import VAE
        from utils.evaluation import calculate_likelihood, load_all_pseudo_input
        import contextlib, io
        # --gpus N: the [N_train x z] latent cache is split into contiguous row blocks, one per rank (cached / eval
        # mode); every rank scores the same test images against its block, one all-gather of the packed [3 x 4S] partials per call
        args = model_args(str(dev), C, sharded=world > 1)
        model = VAE(args).to(dev)
        data = torch.from_numpy(gi.binary_images(0, N_TRAIN))
        dataset = torch.utils.data.TensorDataset(data, torch.arange(N_TRAIN).reshape(-1, 1), torch.zeros(N_TRAIN))
        nimg = a.iwae_images
        test = torch.from_numpy(gi.binary_images(2, nimg))
        loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(test, torch.zeros(nimg)), batch_size=100)
        model.eval()
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            emb = load_all_pseudo_input(args, model, dataset)
            cz, clv = emb[0], emb[1]
            calculate_likelihood(args, model, torch.utils.data.DataLoader(
                torch.utils.data.TensorDataset(test[:4], torch.zeros(4)), batch_size=4), S=args.S, exemplars_embedding=emb)
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(max(1, a.steps // 50)):
                ll = calculate_likelihood(args, model, loader, S=args.S, exemplars_embedding=emb)
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            n_pass = max(1, a.steps // 50)
            dt = time.perf_counter() - t0
            if world > 1:
                tt = torch.tensor([dt], device=dev, dtype=torch.float64)
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                dt = float(tt.item())
            if rank == 0 and a.dump_outputs:
                dump_outputs(a.dump_outputs, {"neg_log_px": np.array([float(ll)], dtype=np.float64)})
            if a.full:
                # dominant kernel: the prior's forward for one evaluator pass (4 images x S samples against all N exemplars)
                zq = cz[:1] + 0.3 * torch.randn(4 * args.S, Z, device=dev)
                lv = clv[0].contiguous()
                us = time_launches(lambda: ops.prior_lse_fwd(zq, cz, lv), reps=2)
        n_loc = int(cz.shape[0])                     # this rank's rows of the cache
        roof = None
        if a.full:
            flops = 2.0 * 4 * args.S * n_loc * Z
            traffic, tsrc = pmc_traffic("prior_iwae")
            executed, pipe = ops.gemm_pipe(n_loc, 4 * args.S, False, flops)      # streaming split-bf16 kernel when the pipe is on
            kname = ("evae::prior_x6_lse_kernel<3> (+ staging pass and split merge; csrc/evae_prior_gemm.hip)" if pipe == "bf16-mfma"
                     else "evae::prior_fwd_mfma_kernel<5, 4> (+ the split merge)")
            roof = mfma_roofline(kname + ": 4 x %d importance samples x %d exemplars x z=%d, distance on the matrix cores, online "
                                         "log-sum-exp" % (args.S, n_loc, Z), flops, executed, pipe, us, traffic if world == 1 else None, tsrc if world == 1 else None)
        a.steps = n_pass * nimg
        cpu_iwae = world == 1 and a.cpu_baseline_steps > 0 and a.full
        if rank == 0:
            print(json.dumps(line("IWAE test log p(x) images/sec", round(n_pass * nimg / dt, 2), "images/sec", a, dt,
                                  "utils.evaluation.calculate_likelihood: vae, S=%d importance samples per test image against all %d "
                                  "training exemplars (the test-log-p(x) half of BASELINE.json's metric), %d test images per pass"
                                  % (args.S, N_TRAIN, nimg), roof, world=world,
                                  extra={"neg_log_px": round(float(ll), 3), "rccl_ranks": rccl_ranks, "backend": backend,
                                         "cpu_baseline": cpu_baseline_iwae(4, args.S, N_TRAIN) if cpu_iwae else None,
                                         "cpu_baseline_reason": None if cpu_iwae else "rank 0 at N = 1 only / --cpu-baseline-steps 0 / no --full",
                                         "parallelism": "single GPU" if world == 1 else
                                         "latent cache row-sharded x%d (%d rows on rank 0), same test images on every rank, one "
                                         "all-gather of packed partial log-sum-exps per call" % (world, n_loc),
                                         "collectives": None if world == 1 else
                                         {"per_call": 1, "bytes_per_call": 12 * 4 * args.S, "list": ["all_gather partial (max, sumexp, nmask) [3 x 4S]"]}})))
        if world > 1:
            dist.destroy_process_group()
        return
    # topk: models/BaseModel.py:263-264 (distance + topk over the candidate cache), utils/knn_on_latent.py:4-9
    res, last = [], {}
    for tag, Bq, N, zd in (("c2", 100, 25000, 40), ("c5", 100, 100000, 256)):
        if tag != "c5" and not a.full:       # the headline is config 5's size
            continue
        z_np, c_np = gi.clustered_latents(3, Bq, N, zd)
        q = torch.from_numpy(z_np).to(dev); cache = torch.from_numpy(c_np).to(dev)
        us = time_launches(lambda: last.__setitem__(tag, ops.pairdist_topk(q, cache, 10, want_val=False)), reps=2)      # k = 10 (approximate_k)
        res.append((tag, Bq, N, zd, us))
    tag, Bq, N, zd, us = res[-1]
    if a.dump_outputs:
        idx_ = last["c5"][0] if isinstance(last["c5"], (tuple, list)) else last["c5"]
        dump_outputs(a.dump_outputs, {"topk_indices": idx_})
    kk = 10
    algo_bytes = lambda Bq_, N_, z_: 4.0 * (N_ * z_ + Bq_ * z_) + 8.0 * Bq_ * kk      # ONE pass over the cache
    bytes_ = algo_bytes(Bq, N, zd)
    gbs = bytes_ / us / 1e3
    traffic, tsrc = pmc_traffic("topk_c5")
    roof = {"bound": "hbm", "kernel": "evae_pairdist_topk at config 5 (B=%d queries, N=%d cached latents, z=%d, k=10): screening GEMM "
                                      "+ exact re-ranking; algorithmic bytes = 4 (N z + B z) + 8 B k: one streaming pass over the [N x z] cache" % (Bq, N, zd),
            "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4), "traffic": traffic,
            "traffic_source": tsrc, "avg_launch_us": round(us, 2), "bytes_per_launch": round(bytes_),
            "other_sizes": {r[0]: {"B": r[1], "N": r[2], "z": r[3], "us": round(r[4], 2),
                                   "GB/s": round(algo_bytes(r[1], r[2], r[3]) / r[4] / 1e3, 1),
                                   "frac": round(algo_bytes(r[1], r[2], r[3]) / r[4] / 1e3 / PEAK_HBM_GBS, 4)} for r in res}}
    a.steps = 1
    cb = cpu_baseline_topk(q, cache, kk) if (a.cpu_baseline_steps > 0 and a.full) else None
    print(json.dumps(line("top-K cache scan", round(Bq / (us * 1e-6), 1), "queries/sec", a, us * 1e-6,
                          "evae_pairdist_topk: k=10 nearest cached latents per query, bit-exact indices (config 5 sizes; config 2 "
                          "sizes in roofline.other_sizes with --full)", roof,
                          extra={"cpu_baseline": cb, "cpu_baseline_reason": None if cb else "--cpu-baseline-steps 0 / no --full"})))


def capture_probe():
    """Child process of a multi-GPU run: capture an all-reduce and an all-gather into a hipGraph, replay, check."""
    rank = int(os.environ.get("RANK", 0)); world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = 0 if os.environ.get("EVAE_BENCH_ONE_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if os.environ.get("EVAE_BENCH_ONE_DEVICE") == "1":
        dist.init_process_group("gloo")
    else:
        dist.init_process_group("nccl", device_id=dev)
    x = torch.full((256,), float(rank + 1), device=dev)
    out = torch.empty(256 * world, device=dev)
    y = x.clone()
    dist.all_reduce(y); dist.all_gather_into_tensor(out, x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        y.copy_(x)
        dist.all_reduce(y)
        dist.all_gather_into_tensor(out, x)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ok = abs(float(y[0].item()) - world * (world + 1) / 2.0) < 1e-3 and abs(float(out[-1].item()) - world) < 1e-3
    dist.destroy_process_group()
    sys.exit(0 if ok else 1)


def amdahl_ceiling(ms_full, n_ex, small=200):
    """Replica mode (--parallel replica: the same batch on every rank, only the exemplars sharded) has a replicated part -- the batch
    rows' own forward / backward, the optimizer, the prior's merge -- that no rank count shrinks.  Measured here as the step at
    C = `small` exemplars (a second process on this box, same kernels): t(R ranks) >= t_small + (t_full - t_small) / R, before any
    collective.  The driver computes scaling efficiency itself; this is the ceiling those numbers are bounded by."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--exemplars", str(small), "--steps", "300", "--warmup", "30", "--iwae-images", "0",
           "--cpu-baseline-steps", "0", "--probe-steps", "0", "--probe-warmup", "0", "--no-amdahl"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        ms_small = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["ms_per_step"]
    except Exception as e:                     # a reported extra, never a reason to lose the bench line
        return {"error": "%s: %s" % (type(e).__name__, str(e)[:120])}
    sharded = max(ms_full - ms_small, 0.0)
    return {"mode": "replica (exemplars sharded, batch replicated), collectives not counted", "ms_per_step_full": round(ms_full, 4),
            "ms_per_step_at_%d_exemplars" % small: ms_small, "replicated_fraction": round(ms_small / ms_full, 3),
            "max_speedup": {str(R): round(ms_full / (ms_small + sharded / R), 2) for R in (2, 4, 8)},
            "note": "t(R) >= t(C = %d) + (t(C = %d) - t(C = %d)) / R; dp mode (--parallel dp) and growth in the exemplar count are not bound by it" % (small, n_ex, small)}


def main():
    if "--capture-probe" in sys.argv:
        capture_probe()
        return
    a = parse()
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    os.environ.setdefault("LOCAL_WORLD_SIZE", str(world))
    from evae import hostcpu
    hostcpu.limit_host_threads()     # the eager legs (c5, iwae, topk) otherwise wake a 256-thread pool per host op: cgroup throttling
    # test hook (tests/test_gpu_sharded.py style): several ranks on ONE GPU over gloo, since RCCL refuses duplicate devices
    one_device = os.environ.get("EVAE_BENCH_ONE_DEVICE") == "1"
    if one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_device:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    rccl_ranks, backend = 1, None
    if world > 1:
        t1 = torch.ones(1, device=dev)
        dist.all_reduce(t1)                              # a real collective: every rank contributed
        rccl_ranks, backend = int(round(float(t1.item()))), dist.get_backend()
    if a.config in ("c3", "c5", "iwae", "topk"):
        return other_config(a, dev, rank, world, rccl_ranks, backend)
    model_name, c_default, n_train = MLP_CONFIGS[a.config]
    n_ex = a.exemplars if a.exemplars is not None else c_default

    # Can this RCCL build capture collectives into a hipGraph (and replay them without hanging)?  A capture that fails
    # half-way cannot be recovered from in-process (the collective library's internal streams and torch's RNG state stay
    # in capture mode), so the question is put to a throw-away child process per rank, under a timeout; the ranks then
    # agree on the verdict.
    if world > 1 and not a.no_graph:
        import subprocess
        env = dict(os.environ, MASTER_PORT=str(int(os.environ.get("MASTER_PORT", "29500")) + 17))
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--capture-probe"], env=env, timeout=90,
                                stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
        except Exception:
            rc = 1
        flag = torch.tensor([1.0 if rc == 0 else 0.0], device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if flag.item() < 0.5:
            if rank == 0:
                print("bench: RCCL collectives cannot be captured into a hipGraph here; launching eagerly", file=sys.stderr)
            a.no_graph = True

    import golden_inputs as gi
    from evae import ops
    from models.VAE import VAE
    from utils.optimizer import AdamNormGrad
    from utils.training import set_beta

    # synthetic dynamic_mnist-shaped training set: binary 28x28, N=50 000, seed 0
    data = torch.from_numpy(gi.binary_images(0, n_train))
    dataset = torch.utils.data.TensorDataset(data, torch.arange(n_train).reshape(-1, 1), torch.arange(n_train) % 10)
    dp = world > 1 and a.parallel == "dp"
    args = model_args("cuda:%d" % local_rank, n_ex, sharded=world > 1, shard_batch=dp, model_name=model_name, n_train=n_train)
    approx = a.config == "c2a"
    args.approximate_prior = approx
    torch.manual_seed(14)                    # same weights and (CPU-generator) exemplar draws on every rank
    torch.cuda.manual_seed(14)
    from utils.utils import importing_model
    model = importing_model(args)(args).to(dev)
    if dp:
        torch.cuda.manual_seed(14 + rank)    # data-parallel batches: every rank its own eps / binarisation stream
    opt = AdamNormGrad(model.parameters(), lr=5e-4)
    data_dev = model.resident_data(dataset)  # one upload; exemplar gathers read HBM from here on
    idx_all = torch.arange(n_train, device=dev).reshape(-1, 1)
    idx_host = torch.arange(n_train).reshape(-1, 1)      # what a DataLoader over the training set hands out
    beta = set_beta(args, 50)
    model.train()
    cache = None
    if approx:                                # the per-epoch latent cache of utils.training.train_one_epoch
        with torch.no_grad():
            cache = tuple(model.cache_z(dataset))
    nb = n_train // B
    loss_acc = torch.zeros((), device=dev)

    def batch_start(i):                      # data-parallel: rank r takes the r-th batch of every group of `world`
        return (((i * world + rank) if dp else i) % nb) * B

    def eager_step(i):
        s = batch_start(i)
        x = torch.bernoulli(data_dev[s:s + B])                     # dynamic binarisation (training.py:31)
        opt.zero_grad()
        loss, RE, KL = model.calculate_loss((x, idx_all[s:s + B]), beta, average=True, dataset=dataset, cache=cache)
        loss.backward()
        opt.step()
        loss_acc.add_(loss.detach())
        state["last"] = (loss, RE, KL)

    from evae.graph import GraphedTrainStep
    graphed = None if a.no_graph else GraphedTrainStep(model, opt, dataset, B, True)
    if graphed is not None and cache is not None:
        cache = graphed.set_cache(cache)      # static buffers: the captured launches read and refresh them in place

    state = {"graphed": graphed, "last": None}

    def step(i):
        g = state["graphed"]
        if g is None:
            return eager_step(i)
        s = batch_start(i)
        try:
            out = g(data_dev[s:s + B], idx_host[s:s + B], beta)     # one hipGraph launch (after 3 eager warm-ups)
        except Exception as e:                                      # capture refused (e.g. by the collective
            if g.graph is not None and g._calls > g.warmup_steps + 1:  # library): keep measuring, eagerly
                raise
            print("bench: hipGraph capture failed (%s); continuing with eager launches" % type(e).__name__,
                  file=sys.stderr)
            state["graphed"] = None
            model._exemplar_indices_override = None
            torch.cuda.synchronize()
            return eager_step(i)
        # the step's losses are accumulated in g.totals by the captured graph itself

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # the collectives of ONE step, counted where they are issued (not declared): the first warm-up step runs under counting
    # wrappers of the torch.distributed entry points the step uses
    coll_seen = []
    if world > 1:
        _orig = {n_: getattr(dist, n_) for n_ in ("all_reduce", "all_gather_into_tensor", "broadcast", "all_gather", "reduce_scatter_tensor")}

        def _counting(n_):
            def f(*ar, **kw):
                t_ = ar[1] if n_ == "all_gather_into_tensor" else ar[0]
                coll_seen.append((n_, int(t_.numel() * t_.element_size()) if torch.is_tensor(t_) else 0))
                return _orig[n_](*ar, **kw)
            return f
        for n_ in _orig:
            setattr(dist, n_, _counting(n_))
    try:
        if a.warmup > 0:
            step(0)
    finally:
        if world > 1:
            for n_, f_ in _orig.items():
                setattr(dist, n_, f_)
    for i in range(1, a.warmup):
        step(i)
    # Untimed, in front of the timed region (VERDICT r02 #3b): (1) the capture happens here whatever --warmup says (the runner
    # needs its eager warm-up calls + the capturing call), (2) RAMP_WINDOWS 10-step windows of replays: the clocks take tens of
    # milliseconds to come up after the host-side setup, and a 20-step timed region is 14 ms.  ramp_settled: the last two windows
    # agreed to 2 % (window times are max-reduced over the ranks).
    n_pre = a.warmup
    g_ = state["graphed"]
    while g_ is not None and state["graphed"] is g_ and g_.graph is None and not g_.failed and n_pre < a.warmup + 8:
        step(n_pre); n_pre += 1
    fence()
    ramp_replays, ramp_ms, prev, ramp_settled = 0, 0.0, None, None
    for _ in range(0 if a.no_ramp else RAMP_WINDOWS):
        tw = time.perf_counter()
        for _ in range(10):
            step(n_pre); n_pre += 1
        torch.cuda.synchronize()
        w_ms = 1e3 * (time.perf_counter() - tw)
        if world > 1:
            tws = torch.tensor([w_ms], device=dev, dtype=torch.float64)
            dist.all_reduce(tws, op=dist.ReduceOp.MAX)
            w_ms = float(tws.item())
        ramp_replays += 10; ramp_ms += w_ms
        if prev is not None:
            ramp_settled = abs(w_ms - prev) <= 0.02 * max(w_ms, prev)
        prev = w_ms
    fence()
    # one event behind every step of the timed region (no synchronisation: read back after the closing fence) so that a short
    # window carries its own spread -- p50 / p90 / max of the per-step device times (VERDICT r03 weak #3e)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(a.steps):
        step(n_pre + i)
        marks[i + 1].record()
    t_issue = time.perf_counter() - t0          # host time to ISSUE the steps (graph launches); the fence below waits for the device
    fence()
    dt = time.perf_counter() - t0
    per_step_raw = [marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps)]
    per_step = sorted(per_step_raw)
    step_ms = {"p50": round(per_step[len(per_step) // 2], 4), "p90": round(per_step[min(len(per_step) - 1, (9 * len(per_step)) // 10)], 4),
               "min": round(per_step[0], 4), "max": round(per_step[-1], 4)} if per_step else None
    ops.prior_train_check()          # the one-launch prior's co-residency guard: raises if any block of any step gave up (outside the timed region)
    n_done = n_pre + a.steps
    g_ = state["graphed"]
    if rank == 0 and a.dump_outputs:             # before the probe steps below train the model on
        if g_ is not None:
            out3 = g_.out
        elif state["last"] is not None:
            loss, RE, KL = (t_.detach().reshape(()) for t_ in state["last"])
            out3 = torch.stack((loss, -RE, KL))
        else:
            out3 = None
        dump_outputs(a.dump_outputs, step_arrays(model, out3))
    loss_sum = float(loss_acc.item()) + (float(g_.totals[0].item()) if g_ is not None else 0.0)
    # Per-kernel timing of the dominant kernel: HIP-event pairs around every GatedDense forward launch.
    # Event pairs cannot be read back from inside a replayed graph, so the same steps are run eagerly right
    # after the timed region (identical kernels, identical shapes); the rocprofv3 summary of the whole
    # command (profiles/) reports the same average for this kernel.
    graphed = state["graphed"]
    dd_ = getattr(graphed, "dedup", None) if graphed is not None else None
    enc_rows = dd_["cap"] if dd_ else None
    # the clocks sag during the host pause above and take ~12 eager steps (30 ms) to come back: untimed steps first,
    # otherwise the event pairs time the launch at a lower clock than the timed region (and rocprof's trace of it) ran at
    def probe_step(i):
        # the runner's own step issued eagerly (same control block, same rows -- the distinct exemplar rows when it encodes those --
        # same optimizer form); plain eager steps when the capture was refused
        if graphed.graph is None:
            return eager_step(i)
        s_ = batch_start(i)
        graphed.step_eagerly(data_dev[s_:s_ + B], idx_host[s_:s_ + B], beta)
    probing = graphed is not None and a.full        # (the roofline object: --full only)
    for i in range(a.probe_warmup if probing else 0):
        probe_step(n_done + i)
    ops.PROBE = {"records": [], "min_flops": 2e9 if n_ex >= 10000 and not approx else 2e8}
    for i in range(a.probe_steps if probing else 0):
        probe_step(n_done + a.probe_warmup + i)
    fence()
    probe, ops.PROBE = ops.PROBE, None
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    final_loss = loss_sum / n_done
    # every rank's parameters after all these steps: the same bits (replica mode reduces only the encoder's gradients and
    # relies on it; evae/shard.py::check_replicas raises on every rank when they differ)
    replicas_identical = None
    if world > 1 and not dp:
        from evae import shard as _shard
        replicas_identical = bool(_shard.check_replicas(model.parameters()))

    # roofline: every big GEMM launch of the probe steps was bracketed with a HIP event pair (evae.ops.probed); the dominant
    # kernel is the launch with the largest share of a step
    agg = {}
    for name, e0, e1, fl, ex, pipe in probe["records"]:
        r = agg.setdefault(name, {"us": 0.0, "n": 0, "flops": fl, "executed": ex, "pipe": pipe})
        r["us"] += 1e3 * e0.elapsed_time(e1); r["n"] += 1
    PEAKS = {"fp32-mfma": PEAK_FP32_MFMA_TFLOPS, "bf16-mfma": PEAK_BF16_MFMA_TFLOPS}
    # PMC pass (tools/kernel_probe.py names) of each launch family at the headline sizes: its counter bytes label the bound
    # (launch-name prefix, probe file, kernel symbol that launch runs)
    Cm = enc_rows if enc_rows else C            # exemplar rows of the step's large launches
    pmc_of = (("dense_bwd_weight_u8", "u8wgrad1", "u8_gemm_kernel<false>"),
              ("gated_dense_fwd_u8 M=%d K=%d N=%d (uint8 rows, three bf16 terms; output + its" % (Cm, D, H), "u8fwd1_img", "u8p_gemm_kernel<4, 2>"),
              ("gated_dense_fwd_u8", "u8fwd1", "u8p_gemm_kernel<4, 2>"),
              ("dense_bwd_data M=%d N=%d+%d K=%d (pre-split" % (Cm, H, H, H), "dgrad2_p6", "gemm_p6_kernel<9, 128, true>"),
              ("dense_bwd_data M=%d N=%d+" % (Cm, H), "dgrad2", "gemm_x6_kernel<9"),
              ("dense_bwd_data M=%d N=%d K=%d (gate-backward epilogue -> pre-split" % (Cm, Z, H), "hdgrad2_img", "gemm_x6_kernel<2, 0, 128, 3>"),
              ("dense_bwd_weight M=%d N=%d K=%d (+db; pre-split" % (Cm + B, 2 * H, H), "wgrad2_p6", "gemm_p6_kernel<3, 64, false>"),
              ("dense_bwd_weight M=%d N=%d K=%d" % (Cm + B, Z, H), "hwgrad", "narrow_wgrad_mfma_kernel"),
              ("dense_bwd_weight M=", "wgrad2", "gemm_kernel<false, false, 3"),
              ("gated_dense_fwd M=%d K=%d N=%d (pre-split" % (Cm, H, H), "fwd2_p6", "gemm_p6_kernel<1, 128, true>"),
              ("gated_dense_fwd M=%d K=%d" % (Cm, H), "fwd2", "gemm_x6_kernel<1"))
    headline = a.config == "c2" and n_ex == C
    kernels = []
    for name, r in agg.items():
        us = r["us"] / r["n"]
        pm = next(((f, sym) for pre, f, sym in pmc_of if name.startswith(pre)), None) if headline else None
        traffic, traffic_src = pmc_traffic(*pm) if pm else (None, None)
        if traffic is not None and traffic_src and pm:
            prows = pmc_rows(pm[0])
            if prows is not None and prows != Cm:
                traffic_src += "; the PMC pass ran this launch at %d exemplar rows, the step runs it at %d" % (prows, Cm)
        if r["pipe"] == "hbm":       # a streaming launch: algorithmic bytes / time against the HBM peak
            kernels.append({"launch": name, "pipe": "hbm", "avg_launch_us": round(us, 2), "launches": r["n"],
                            "algorithmic_tb_per_s": round(r["flops"] / us / 1e6, 3), "frac": round(r["flops"] / us / 1e6 / (PEAK_HBM_GBS / 1000.0), 4),
                            "bound": "hbm", "traffic": traffic, "traffic_source": traffic_src, "bytes_per_launch": round(r["flops"])})
            continue
        peak = PEAKS[r["pipe"]]
        kernels.append({"launch": name, "pipe": r["pipe"], "avg_launch_us": round(us, 2), "launches": r["n"],
                        "algorithmic_tflops": round(r["flops"] / us / 1e6, 2), "frac": round(r["flops"] / us / 1e6 / peak, 4),
                        "executed_tflops": round(r["executed"] / us / 1e6, 2),
                        "pipe_busy_frac": round(r["executed"] / us / 1e6 / peak, 4),
                        "bound": bound_label(traffic, us), "traffic": traffic, "traffic_source": traffic_src,
                        "flops_per_launch": round(r["flops"])})
    # ... and the same launches INSIDE the replayed graph: a child run under rocprofv3; the eager event pairs above
    # time a launch alone-ish (the host paces eager steps), inside the replay it shares the machine with the side stream's launches
    gstats, gsrc = (None, "not the headline configuration on one GPU") if not (headline and world == 1 and state["graphed"] is not None and rank == 0) \
        else (None, "--no-graph-profile") if a.no_graph_profile else (None, "no --full") if not a.full else graph_kernel_stats()
    sym_of = {pre: sym for pre, _, sym in pmc_of}
    for k_ in kernels:
        k_["in_graph_avg_launch_us"] = None
        sym = next((sy for pre, sy in sym_of.items() if k_["launch"].startswith(pre)), None) if gstats else None
        hit = [(n_, v_) for n_, v_ in (gstats or {}).items() if sym and sym in n_]
        if len(hit) == 1 and "finish" in k_["launch"]:
            # an entry that brackets several launches (pre-passes / split-K GEMM / finish): its GEMM kernel alone, inside the replay
            k_["kernel_symbol"] = hit[0][0][:120]
            k_["in_graph_gemm_kernel_us"] = round(hit[0][1][1], 2)
        elif len(hit) == 1:
            us_g = hit[0][1][1]
            k_["kernel_symbol"] = hit[0][0][:120]
            k_["in_graph_avg_launch_us"] = round(us_g, 2)
            k_["in_graph_calls"] = hit[0][1][0]
            per = k_.get("flops_per_launch") if k_["pipe"] != "hbm" else k_.get("bytes_per_launch")
            if k_["pipe"] == "hbm":
                k_["in_graph_frac"] = round(per / us_g / 1e6 / (PEAK_HBM_GBS / 1000.0), 4)
            else:
                k_["in_graph_algorithmic_tflops"] = round(per / us_g / 1e6, 2)
                k_["in_graph_frac"] = round(per / us_g / 1e6 / PEAKS[k_["pipe"]], 4)
    key_us = lambda k_: k_["in_graph_avg_launch_us"] if k_["in_graph_avg_launch_us"] is not None else k_["avg_launch_us"]
    kernels.sort(key=lambda k_: -key_us(k_))
    roof = None
    if kernels:
        # entries that bracket several launches (a weight gradient = pre-passes / split-K GEMM + finish) are listed, the
        # roofline object itself is the longest SINGLE kernel launch -- of the replayed graph when the child run delivered
        single = [k_ for k_ in kernels if "finish" not in k_["launch"] and k_["pipe"] != "hbm"]
        dom = (single or kernels)[0]
        in_graph = dom["in_graph_avg_launch_us"] is not None
        if in_graph:                              # the roofline numbers of the replay, the eager ones kept beside them
            dom = dict(dom, eager_avg_launch_us=dom["avg_launch_us"], eager_frac=dom["frac"], avg_launch_us=dom["in_graph_avg_launch_us"],
                       algorithmic_tflops=dom["in_graph_algorithmic_tflops"], frac=dom["in_graph_frac"],
                       executed_tflops=round(dom["executed_tflops"] * dom["avg_launch_us"] / dom["in_graph_avg_launch_us"], 2),
                       pipe_busy_frac=round(dom["pipe_busy_frac"] * dom["avg_launch_us"] / dom["in_graph_avg_launch_us"], 4),
                       launches=dom.get("in_graph_calls", dom["launches"]))
        gem = [(k_, k_["in_graph_avg_launch_us"] if k_["in_graph_avg_launch_us"] is not None else k_.get("in_graph_gemm_kernel_us"))
               for k_ in kernels if k_["pipe"] != "hbm"]
        gem = [(k_, u_) for k_, u_ in gem if u_ is not None and k_["flops_per_launch"] >= 2e9]
        agg_g = None
        if gem:
            tf_ = sum(k_["flops_per_launch"] for k_, _ in gem); tu_ = sum(u_ for _, u_ in gem)
            agg_g = {"launches": len(gem), "kernels": [k_["launch"][:60] for k_, _ in gem], "flops": round(tf_), "us": round(tu_, 1), "algorithmic_tflops": round(tf_ / tu_ / 1e6, 1),
                     "frac_of_bf16_mfma_peak": round(tf_ / tu_ / 1e6 / PEAK_BF16_MFMA_TFLOPS, 4),
                     "frac_of_fp32_mfma_peak": round(tf_ / tu_ / 1e6 / PEAK_FP32_MFMA_TFLOPS, 4),
                     "note": "time-weighted over the step's large GEMM launches as they run inside the replayed graph"}
        roof = {"bound": dom["bound"], "kernel": dom["launch"] + (" -- the longest launch of the REPLAYED step (rocprofv3 kernel trace of a child run of this command)"
                                                                  if in_graph else " -- the longest launch of the step issued eagerly under HIP events"),
                "timing_source": (gsrc if in_graph else {"eager_event_pairs": True, "in_graph": gsrc}),
                "gemm_aggregate": agg_g,
                "achieved": dom["algorithmic_tflops"], "peak": PEAKS[dom["pipe"]], "unit": "TFLOP/s", "frac": dom["frac"],
                "pipe": dom["pipe"], "pipe_busy_frac": dom["pipe_busy_frac"], "executed_tflops": dom["executed_tflops"],
                "frac_of_fp32_mfma_peak": round(dom["algorithmic_tflops"] / PEAK_FP32_MFMA_TFLOPS, 4),
                "traffic": dom["traffic"], "traffic_source": dom["traffic_source"],
                "launches": dom["launches"], "avg_launch_us": dom["avg_launch_us"], "flops_per_launch": dom["flops_per_launch"],
                "note": "achieved / frac = ALGORITHMIC flops per launch / mean launch time (HIP events) / dense peak of the pipe "
                        "the launch computes on (SURVEY 8d).  pipe bf16-mfma: fp32 products evaluated as bf16 partial products with "
                        "fp32 accumulation -- three per product on the uint8 first-layer kernels, six on the split-bf16 GEMM -- so "
                        "the pipe issues 3 x / 6 x the algorithmic flops; that occupancy is pipe_busy_frac, not the roofline "
                        "fraction.  bound = 'fabric' when the launch's PMC pass moved >= 5 TB/s",
                "step_algorithmic_tflops": round(step_flops(model_name, n_ex, enc_rows) / (dt / a.steps) / 1e12, 2) if step_flops(model_name, n_ex) else None,
                "kernels": kernels}

    # second half of BASELINE.json's metric: test log p(x) (IWAE, S = 5000, all N_train exemplars as the prior)
    iwae = None
    if world == 1 and a.iwae_images > 0 and a.config == "c2" and a.full:
        from utils.evaluation import calculate_likelihood
        test = torch.from_numpy(gi.binary_images(2, a.iwae_images))
        test_ds = torch.utils.data.TensorDataset(test, torch.zeros(len(test)))
        loader = torch.utils.data.DataLoader(test_ds, batch_size=100)
        import contextlib, io
        model.eval()
        with torch.no_grad():
            cz, clv = model.cache_z(dataset)
            emb = (cz, clv, torch.arange(len(cz)))
            with contextlib.redirect_stdout(io.StringIO()):
                calculate_likelihood(args, model, torch.utils.data.DataLoader(
                    torch.utils.data.TensorDataset(test[:2], torch.zeros(2)), batch_size=2), S=args.S, exemplars_embedding=emb)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                ll = calculate_likelihood(args, model, loader, S=args.S, exemplars_embedding=emb)
                torch.cuda.synchronize()
                t_ll = time.perf_counter() - t1
        model.train()
        iwae = {"neg_log_px": round(ll, 3), "images": a.iwae_images, "S": args.S, "exemplars": n_train,
                "ms_per_image": round(1e3 * t_ll / a.iwae_images, 3),
                "note": "utils.evaluation.calculate_likelihood on the first %d synthetic test images (SURVEY 8d) after the "
                        "benchmark's few training steps of a random-init model: a smoke value of the evaluator (timing + finite, "
                        "parity is tests/), NOT a model-quality number" % a.iwae_images}

    gb = B * world if dp else B              # images per step over all ranks
    # collectives of one step, per rank (payload bytes sent = received per rank for an all-gather of R such pieces)
    n_param = sum(p_.numel() for p_ in model.parameters())
    if world == 1:
        coll = {"count": 0, "bytes": 0, "list": []}
    elif dp:
        lst = [("all_gather z", 4 * B * Z), ("all_gather batch indices", 8 * B), ("all_gather partial (max, sumexp, nmask)", 12 * B * world),
               ("all_gather (lse, coefficient)", 8 * B), ("all_reduce dz", 4 * B * world * Z), ("all_reduce parameter gradients", 4 * n_param)]
        coll = {"count": len(lst), "bytes": sum(b_ for _, b_ in lst), "list": lst}
    else:
        # replicated batch: only the encoder q(z | .) sees the rank's exemplar shard -- the flat all-reduce carries its six tensors
        n_enc = sum(p_.numel() for nm_, p_ in model.named_parameters() if nm_.startswith(("q_z_layers", "q_z_mean")))
        lst = [("all_gather partial (max, sumexp, nmask)", 12 * B), ("all_reduce (dz, dlogvar)", 4 * (B * Z + Z)),
               ("all_reduce encoder gradients (the others are identical on every rank)" if model_name == "vae"
                else "all_reduce parameter gradients", 4 * (n_enc if model_name == "vae" else n_param))]
        coll = {"count": len(lst), "bytes": sum(b_ for _, b_ in lst), "list": lst}
    if world > 1:
        coll["issued_in_one_step"] = {"count": len(coll_seen), "list": coll_seen}     # counted, see above
    # second measurement of a multi-GPU run: the data-parallel mode, same process group, its own model / optimizer / runner
    dp_line = None
    if world > 1 and not dp and not a.no_dp_line and a.full:
        try:
            from evae.graph import GraphedTrainStep as _G
            args2 = model_args("cuda:%d" % local_rank, n_ex, sharded=True, shard_batch=True, model_name=model_name, n_train=n_train)
            torch.manual_seed(14); torch.cuda.manual_seed(14)
            model2 = importing_model(args2)(args2).to(dev)
            torch.cuda.manual_seed(14 + rank)
            opt2 = AdamNormGrad(model2.parameters(), lr=5e-4)
            model2.train()
            run2 = None if state["graphed"] is None else _G(model2, opt2, dataset, B, True)

            def step2(i):
                s_ = (((i * world + rank)) % nb) * B
                if run2 is not None:
                    return run2(data_dev[s_:s_ + B], idx_host[s_:s_ + B], beta)
                x_ = torch.bernoulli(data_dev[s_:s_ + B])
                opt2.zero_grad()
                l_, _, _ = model2.calculate_loss((x_, idx_all[s_:s_ + B]), beta, average=True, dataset=dataset)
                l_.backward()
                opt2.step()
            for i in range(a.warmup):
                step2(i)
            fence()
            t2 = time.perf_counter()
            for i in range(a.steps):
                step2(a.warmup + i)
            fence()
            dt2 = time.perf_counter() - t2
            tt = torch.tensor([dt2], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt2 = float(tt.item())
            lst2 = [("all_gather z", 4 * B * Z), ("all_gather batch indices", 8 * B),
                    ("all_gather partial (max, sumexp, nmask)", 12 * B * world), ("all_gather (lse, coefficient)", 8 * B),
                    ("all_reduce dz", 4 * B * world * Z), ("all_reduce parameter gradients", 4 * n_param)]
            dp_line = {"value": round(B * world * a.steps / dt2, 1), "unit": "images/sec", "ms_per_step": round(1e3 * dt2 / a.steps, 4),
                       "scaling": "weak", "global_batch": B * world,
                       "parallelism": "dp%d (own %d-image batch per rank) x exemplar-shard x%d" % (world, B, world),
                       "collectives": {"count": len(lst2), "bytes": sum(b_ for _, b_ in lst2)},
                       "launch": "eager" if (run2 is None or run2.graph is None) else "hipGraph replay of the whole step"}
        except Exception as e:                                          # the main line stands on its own
            dp_line = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    if rank == 0:
        out = {
            "metric": "training images/sec", "value": round(gb * a.steps / dt, 1), "unit": "images/sec",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(1e3 * dt / a.steps, 4),
            "higher_is_better": True, "scaling": "weak" if dp else "strong", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "arithmetic": ("fp32 results throughout.  Large forward / data-gradient GEMMs run on the bf16 matrix pipe with every "
                           "fp32 operand split into three bf16 terms (24 mantissa bits) and six partial products accumulated in "
                           "fp32 (csrc/evae_gemm_x6.h); the uint8 image store (k/255 data) feeds the first encoder layer as bytes "
                           "(exact in bf16) times a three-term split of the weights.  Both carry fp32-GEMM accuracy: tests hold "
                           "them to the fp32-MFMA kernel's bar against the fp64 oracle and compare the two kernels' errors; "
                           "EVAE_X6=0 / EVAE_U8_STORE=0 put everything back on v_mfma_f32_32x32x2_f32"),
            "config": {"workload": "%s + exemplar_prior, %s-shaped binary 28x28, N=%d, batch %d per GPU, "
                                   "%d %s (BASELINE.json configs[%d]%s)"
                                   % (model_name, "omniglot" if a.config == "c4" else "dynamic_mnist", n_train, B, n_ex,
                                      "candidates per step, approximate prior: top-10 per batch row over their cached latents, 1000 "
                                      "exemplar slots re-encoded" if approx else "exemplars in total, exact prior",
                                      {"c1": 0, "c2": 1, "c2a": 1, "c4": 3}[a.config],
                                      " with --approximate_prior True" if approx else ""),
                       "global_batch": gb, "exemplars": n_ex,
                       "parallelism": ("single GPU" if world == 1 else
                                       ("dp%d (own %d-image batch per rank) x exemplar-shard x%d, partial-LSE exchange over RCCL"
                                        % (world, B, world)) if dp else
                                       ("replicated batch, exemplar-shard x%d" % world)),
                       "launch": "eager" if graphed is None else "hipGraph replay of the whole step"},
            "collectives": coll, "rccl_ranks": rccl_ranks, "backend": backend,
            "dp": dp_line,
            "host_issue_ms_per_step": round(1e3 * t_issue / a.steps, 4), "ramp_replays": ramp_replays, "ramp_ms": round(ramp_ms, 2), "ramp_settled": ramp_settled,
            "untimed_steps": n_pre,
            "step_ms": step_ms,
            **({"per_step_ms": [round(t_, 4) for t_ in per_step_raw]} if os.environ.get("EVAE_BENCH_DUMP_STEPS") == "1" else {}),
            "mean_loss": round(final_loss, 4), "mean_loss_f64": final_loss, "steps_in_mean_loss": n_done,
            "replicas_identical": replicas_identical,
            "exemplar_rows": (None if not dd_ else
                              {"drawn": n_ex, "encoded_per_step": dd_["cap"], "distinct_in_the_last_step": dd_["distinct"],
                               "note": "the reference draws its exemplars WITH replacement (models/BaseModel.py:245): %d draws from %d "
                                       "images name ~%d distinct ones.  The captured step encodes a fixed %d rows (the distinct ones, "
                                       "padded with multiplicity 0); the prior still sees all %d draws (centres gathered from the distinct "
                                       "rows' encodings, leave-one-out mask and denominator on the draws), a distinct row's gradient is "
                                       "its multiplicity x one draw's.  Same loss and gradients as encoding every draw "
                                       "(tests/test_gpu_model.py::test_graphed_step_over_distinct_exemplar_rows_matches_eager); "
                                       "EVAE_DEDUP=0 encodes every draw.  roofline.kernels[] time the step's own launches (the same control block and rows, "
                                       "issued eagerly: GraphedTrainStep.step_eagerly)" % (n_ex, n_train, dd_["distinct"], dd_["cap"], n_ex)}),
            "roofline": roof,
            "test_log_px": iwae,
            "cpu_baseline": None,
        }
        if world == 1 and a.cpu_baseline_steps > 0 and model_name == "vae" and not approx and a.full:
            out["cpu_baseline"] = cpu_baseline(a.cpu_baseline_steps, n_ex, n_train)
        else:
            out["cpu_baseline_reason"] = ("rank 0 at N = 1 only" if world > 1 else "--cpu-baseline-steps 0" if a.cpu_baseline_steps <= 0 else
                                          "no --full" if not a.full else
                                          (NO_PORT % "hvae_2level") if model_name != "vae" else
                                          "the oracle's training step restates the exact prior; the approximate (cache + top-k) step is held to "
                                          "golden G10 of the real reference")
        if world == 1 and a.config == "c2" and a.exemplars is None and not a.no_amdahl and a.full:
            out["amdahl_ceiling"] = amdahl_ceiling(1e3 * dt / a.steps, n_ex)
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
