#!/usr/bin/env python3
"""pixelcnn generation: args.pixelcnn_sampler = 'passes' (784 truncated-height decoder passes, models/PixelCNN.py) against 'cached'
(one launch of the decode kernel, csrc/evae_pixel_decode.hip) on the same model and latents, B = 10 and B = 100.  GPU box only.
Device events around whole pixelcnn_generate calls (latent images, uniforms, weight packing and the launch included for 'cached'),
the two samplers alternated: one warm-up call each, then three timed calls each.  Writes the per-call times, their spread
(max - min), the ratio of medians, the decode launch alone (cache allocation included) and the kernel's resource figures to
profiles/pixelsnail_generate.json (or the path given as the first argument).  There is no pass bar: `faster` says whether 'cached'
beat 'passes' by more than three times the larger spread.  The 'passes' sampler takes seconds per call at B = 100: run under a time limit of a few minutes.

Large batches (`scale` in the output): whole 'cached' pixelcnn_generate calls at B = 10 ... 2048 with the images per workgroup forced
to each of --images-per-block (1, 2, 4 or auto = the library's table; default: all four), the choices alternated within a batch
size, one warm-up + three timed calls each, median and spread; `beats_1` says whether a choice beat 1 by more than three times the
larger spread of the two (the bar for moving a batch range in evae_pixel_decode_choose_images).  Then one call at B = 4096 on
'auto', which runs in chunks of models.PixelCNN.PIXEL_DECODE_CHUNK_IMAGES.  --skip-passes leaves the 'passes' comparison out."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "exemplar-vae_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                                                    # noqa: E402

TIMED, BATCHES = 3, (10, 100)
SCALE_BATCHES, CHUNKED_BATCH = (10, 100, 256, 257, 384, 512, 550, 768, 1024, 2048), 4096


def kernel_resources():
    """registers, scratch and occupancy of the decode kernel from the compiler's resource report (the file alone, compiled to a
    temporary object), LDS and images per workgroup from the library"""
    from evae import _lib
    lib = _lib.load()
    out = {"images_per_block": int(lib.evae_pixel_decode_images_per_block()), "threads_per_block": 256,
           "lds_bytes_per_block": int(lib.evae_pixel_decode_lds_bytes()), "cache_bytes_per_image": 4 * int(lib.evae_pixel_decode_cache_floats()),
           "instances": {str(g): {"lds_bytes_per_block": int(lib.evae_pixel_decode_lds_bytes_for(g))} for g in (1, 2, 4)}}
    src = os.path.join(ROOT, "exemplar-vae_amd", "csrc", "evae_pixel_decode.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        with tempfile.TemporaryDirectory() as tmp:
            rep = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-x", "hip",
                                  "-c", src, "-o", os.path.join(tmp, "pd.o")], capture_output=True, text=True, timeout=300).stderr
    except (OSError, subprocess.SubprocessError) as e:
        out["compiler_report"] = "not available: %s" % (e,)
        return out
    pats = (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                     ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                     ("sgpr_spills_to_vgpr_lanes", r"SGPRs Spill: (\d+)"), ("vgpr_spills", r"VGPRs Spill: (\d+)"))
    for g in (1, 2, 4):                                         # one report per instance; the top-level figures are the default's
        at = rep.find("pixel_decode_kernelILi%dE" % g)
        block = rep[at:] if at >= 0 else ""
        for key, pat in pats:
            m = re.search(pat, block)
            out["instances"][str(g)][key] = int(m.group(1)) if m else None
    out.update({k: v for k, v in out["instances"][str(out["images_per_block"])].items() if k != "lds_bytes_per_block"})
    return out


def timed_call(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def scale_cases(model, choices):
    """whole 'cached' pixelcnn_generate calls with the images per workgroup forced (the model asks ops.pixel_decode_choose_images)"""
    import numpy as np
    from evae import ops
    from models import PixelCNN
    table = ops.pixel_decode_choose_images
    model.args.pixelcnn_sampler = "cached"
    out = []

    def run(z1, z2, g):
        ops.pixel_decode_choose_images = table if g == "auto" else (lambda B: g)
        try:
            assert model.pixelcnn_generate(z1, z2).shape == (z1.shape[0], 784)
        finally:
            ops.pixel_decode_choose_images = table

    for B in SCALE_BATCHES + (CHUNKED_BATCH,):
        rs = np.random.RandomState(290 + B)
        z1 = torch.from_numpy(rs.randn(B, 40).astype(np.float32)).cuda()
        z2 = torch.from_numpy(rs.randn(B, 40).astype(np.float32)).cuda()
        gs = ["auto"] if B == CHUNKED_BATCH else list(choices)
        n_timed = 1 if B == CHUNKED_BATCH else TIMED
        ms = {str(g): [] for g in gs}
        for g in gs:                                            # one warm-up each
            run(z1, z2, g)
        torch.cuda.synchronize()
        for _ in range(n_timed):                                # alternated
            for g in gs:
                ms[str(g)].append(round(timed_call(lambda: run(z1, z2, g)), 3))
                print("B = %4d  G = %-4s  %.3f ms" % (B, g, ms[str(g)][-1]), flush=True)
        med = {g: sorted(v)[len(v) // 2] for g, v in ms.items()}
        spread = {g: round(max(v) - min(v), 3) for g, v in ms.items()}
        case = {"B": B, "auto_is": table(min(B, PixelCNN.PIXEL_DECODE_CHUNK_IMAGES)), "launches": -(-B // PixelCNN.PIXEL_DECODE_CHUNK_IMAGES),
                "ms_per_call": ms, "median_ms": med, "spread_ms": spread}
        if "1" in med:
            case["beats_1"] = {g: bool(med["1"] - med[g] > 3.0 * max(spread["1"], spread[g])) for g in med if g not in ("1", "auto")}
        out.append(case)
    del model.args.pixelcnn_sampler
    return out


def main():
    if not torch.cuda.is_available():
        sys.exit("tools/pixelsnail_generate_bench.py needs a GPU")
    import numpy as np
    import smoke_case
    from utils.utils import importing_model
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "pixelsnail_generate.json"))
    ap.add_argument("--images-per-block", choices=("1", "2", "4", "auto"), default=None,
                    help="the one choice the large batches run at (default: 1, 2, 4 and auto, alternated)")
    ap.add_argument("--skip-passes", action="store_true", help="leave the 'passes' against 'cached' comparison out")
    opts = ap.parse_args()
    out_path = opts.out
    ipb = opts.images_per_block
    choices = (1, 2, 4, "auto") if ipb is None else ((ipb if ipb == "auto" else int(ipb)),)
    args = smoke_case.vae_args(model_name="pixelcnn", number_components=6, training_set_size=6)
    torch.manual_seed(271)
    model = importing_model(args)(args).cuda().eval()
    cases = []
    for B in (() if opts.skip_passes else BATCHES):
        rs = np.random.RandomState(290 + B)
        z1 = torch.from_numpy(rs.randn(B, 40).astype(np.float32)).cuda()
        z2 = torch.from_numpy(rs.randn(B, 40).astype(np.float32)).cuda()

        def run(sampler):
            model.args.pixelcnn_sampler = sampler
            out = model.pixelcnn_generate(z1, z2)
            assert out.shape == (B, 784)

        ms = {"passes": [], "cached": []}
        for s in ms:                                            # one warm-up each
            run(s)
        torch.cuda.synchronize()
        for _ in range(TIMED):                                  # alternated
            for s in ms:
                ms[s].append(round(timed_call(lambda: run(s)), 3))
                print("B = %3d  %-6s  %.3f ms" % (B, s, ms[s][-1]), flush=True)
        # the decode launch alone (packed weights, latent images and uniforms made before the first event)
        from evae import ops
        with torch.no_grad():
            packed, latent = ops.pixel_decode_pack(model.pixelcnn, model.p_x_mean), model._decoder_images(z1, z2)
            u = torch.rand(B, 784, device="cuda")
            launch = [round(timed_call(lambda: ops.pixel_decode(packed, latent, torch.zeros(B, 784, device="cuda"), u=u)), 3)
                      for _ in range(TIMED + 1)][1:]
        med = {s: sorted(v)[len(v) // 2] for s, v in ms.items()}
        spread = {s: round(max(v) - min(v), 3) for s, v in ms.items()}
        gain = med["passes"] - med["cached"]
        cases.append({"B": B, "ms_per_call": ms, "median_ms": med, "spread_ms": spread,
                      "ratio_of_medians_passes_over_cached": round(med["passes"] / med["cached"], 2),
                      "decode_launch_alone_ms": launch, "decode_launch_us_per_pixel": round(sorted(launch)[len(launch) // 2] * 1e3 / 784, 2),
                      "faster": bool(gain > 3.0 * max(spread.values()))})
    if hasattr(model.args, "pixelcnn_sampler"):
        del model.args.pixelcnn_sampler
    scale = scale_cases(model, choices)
    doc = {"tool": "tools/pixelsnail_generate_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "device events around whole pixelcnn_generate calls; samplers alternated, 1 warm-up + %d timed calls each" % TIMED,
           "kernel": kernel_resources(), "cases": cases, "scale": scale,
           "not_measured": (["'passes' against 'cached' (--skip-passes)"] if opts.skip_passes else [])
           + ["'passes' above B = 100", "B above %d" % CHUNKED_BATCH, "cyclic generation end to end", "the kernel under a profiler"]}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["cases"]))
    print(json.dumps([{k: c[k] for k in ("B", "auto_is", "median_ms", "spread_ms")} for c in scale]))


if __name__ == "__main__":
    main()
