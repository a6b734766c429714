#!/usr/bin/env python3
"""pixelcnn generation: args.pixelcnn_sampler = 'passes' (784 truncated-height decoder passes, models/PixelCNN.py) against 'cached'
(one launch of the decode kernel, csrc/evae_pixel_decode.hip) on the same model and latents, B = 10 and B = 100.  GPU box only.
Device events around whole pixelcnn_generate calls (latent images, uniforms, weight packing and the launch included for 'cached'),
the two samplers alternated: one warm-up call each, then three timed calls each.  Writes the per-call times, their spread
(max - min), the ratio of medians, the decode launch alone (cache allocation included) and the kernel's resource figures to
profiles/pixelsnail_generate.json (or the path given as the first argument).  There is no pass bar: `faster` says whether 'cached'
beat 'passes' by more than three times the larger spread.  The 'passes' sampler takes seconds per call at B = 100: run under a time limit of a few minutes."""
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


def kernel_resources():
    """registers, scratch and occupancy of the decode kernel from the compiler's resource report (the file alone, compiled to a
    temporary object), LDS and images per workgroup from the library"""
    from evae import _lib
    lib = _lib.load()
    out = {"images_per_block": int(lib.evae_pixel_decode_images_per_block()), "threads_per_block": 256,
           "lds_bytes_per_block": int(lib.evae_pixel_decode_lds_bytes()), "cache_bytes_per_image": 4 * int(lib.evae_pixel_decode_cache_floats())}
    src = os.path.join(ROOT, "exemplar-vae_amd", "csrc", "evae_pixel_decode.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        with tempfile.TemporaryDirectory() as tmp:
            rep = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-x", "hip",
                                  "-c", src, "-o", os.path.join(tmp, "pd.o")], capture_output=True, text=True, timeout=300).stderr
    except (OSError, subprocess.SubprocessError) as e:
        out["compiler_report"] = "not available: %s" % (e,)
        return out
    block = rep[rep.find("pixel_decode_kernel"):]
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                     ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)"),
                     ("sgpr_spills_to_vgpr_lanes", r"SGPRs Spill: (\d+)"), ("vgpr_spills", r"VGPRs Spill: (\d+)")):
        m = re.search(pat, block)
        out[key] = int(m.group(1)) if m else None
    return out


def timed_call(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    if not torch.cuda.is_available():
        sys.exit("tools/pixelsnail_generate_bench.py needs a GPU")
    import numpy as np
    import smoke_case
    from utils.utils import importing_model
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pixelsnail_generate.json")
    args = smoke_case.vae_args(model_name="pixelcnn", number_components=6, training_set_size=6)
    torch.manual_seed(271)
    model = importing_model(args)(args).cuda().eval()
    cases = []
    for B in BATCHES:
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
    del model.args.pixelcnn_sampler
    doc = {"tool": "tools/pixelsnail_generate_bench.py", "device": torch.cuda.get_device_name(0),
           "method": "device events around whole pixelcnn_generate calls; samplers alternated, 1 warm-up + %d timed calls each" % TIMED,
           "kernel": kernel_resources(), "cases": cases,
           "not_measured": ["B above 100 (DESIGN.md 3.4d has the decode launch alone up to B = 1024, for 1, 2 and 4 images per workgroup)",
                            "cyclic generation end to end", "the kernel under a profiler"]}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["cases"]))


if __name__ == "__main__":
    main()
