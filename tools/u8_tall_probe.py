#!/usr/bin/env python3
"""The byte layer's forward launch alone (evae_gated_dense_fwd_u8 and _timg; K = 784, N = 300, rows gathered from a 50 000-row
store) at several row counts: HIP event pairs in bench.py's time_launches pattern, two passes per entry point.
usage: u8_tall_probe.py <out json> [M ...]   (default 13056 19968: one and two rounds of 256-row blocks on 256 CUs)
EVAE_U8_TALL=2 / 3 forces 256- / 448-row blocks, unset the host rule decides (csrc/evae_tile_map.h::u8_fwd_block_rows);
EVAE_PROBE_TREE=<dir> times the library of another checkout (an A/B against a parent build).  -> profiles/u8fwd_tall.json"""
import ctypes as C, json, os, sys
root = os.path.abspath(os.environ.get("EVAE_PROBE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); outp = sys.argv[1]
Ms = [int(v) for v in sys.argv[2:]] or [13056, 19968]
sys.path.insert(0, os.path.join(root, "exemplar-vae_amd"))
import torch
from evae import ops, _lib
lib = _lib.load(); dev = torch.device("cuda"); p, st = ops._p, ops._stream
torch.manual_seed(0)
R, D, H = 50000, 784, 300


def time_launches(fn, reps=4, pairs=12, warm=6):
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
    ts = sorted(1e3 * a.elapsed_time(b) / reps for a, b in evs)
    return {"mean_us": round(sum(ts) / len(ts), 2), "min_us": round(ts[0], 2), "median_us": round(ts[len(ts) // 2], 2), "max_us": round(ts[-1], 2)}


q = (torch.randint(0, 256, (R, D), device=dev) * (torch.rand(R, D, device=dev) < 0.2)).to(torch.uint8)
store = torch.zeros(R * D + 64, dtype=torch.uint8, device=dev); xs = store[:R * D].view(R, D); xs.copy_(q)
wh = torch.randn(H, D, device=dev) * 0.05; wg = torch.randn(H, D, device=dev) * 0.05; b = torch.zeros(H, device=dev)
prep = ops.u8_prepare(wh, wg)
res = {"tree": root, "EVAE_U8_TALL": os.environ.get("EVAE_U8_TALL"), "device": torch.cuda.get_device_name(0),
       "cus": torch.cuda.get_device_properties(0).multi_processor_count, "K": D, "N": H, "sizes": {}}
for M in Ms:
    rows = torch.randint(0, R, (M,), device=dev)
    out = torch.empty(M, H, device=dev); so = torch.empty(M, H, device=dev)
    nks = lib.evae_p6_nks_rows(M + 100)
    img = torch.zeros(lib.evae_p6_image_bytes(H + 1, nks), dtype=torch.uint8, device=dev)
    plain = lambda: _lib.check(lib.evae_gated_dense_fwd_u8(p(xs), p(rows), M, D, D, 1.0 / 255.0, p(prep), p(b), p(b), H, p(out), p(so), st()), "fwd")
    timg = lambda: _lib.check(lib.evae_gated_dense_fwd_u8_timg(p(xs), p(rows), M, D, D, 1.0 / 255.0, p(prep), p(b), p(b), H, p(out), p(so),
                                                               p(img), nks, 0, 0, st()), "fwd_timg")
    r = {"fwd_u8": time_launches(plain), "fwd_u8_timg": time_launches(timg)}
    # second pass, so that a clock ramp shows
    r["fwd_u8_again"] = time_launches(plain); r["fwd_u8_timg_again"] = time_launches(timg)
    res["sizes"][str(M)] = r
    print(M, json.dumps(r), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(outp)), exist_ok=True)
with open(outp, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", outp)
