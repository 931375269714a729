#!/usr/bin/env python
"""Host time per call of two lit-draw entry points on a small frame (64 x 40, 12 point lights): vqhip_forward_lighting and vqhip_forward_lighting_from_materials_quad,
called through ctypes with arguments built once. A batch of calls is timed with the host clock and nothing waits inside it (beyond the constant ring's own wait for
the call 32 back); the device is drained between batches. Prints one JSON line: the median and the fastest batch, in microseconds per call. For an A/B of the host
code, run it once per process and library (VQHIP_LIBRARY_PATH), alternating: profiles/r23a_lit_front_ends.md."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqengine_amd import abi, capi, synth      # noqa: E402

W, H = 64, 40


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--calls", type=int, default=200, help="calls per batch")
    args = ap.parse_args()
    ctx = capi.Context(0)
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    dev = lambda a: torch.from_numpy(a).cuda()                                       # noqa: E731
    gb = [dev(g) for g in synth.gbuffer(W, H)]
    pf, _ = synth.per_frame(points=synth.point_lights(12), spots=synth.spot_lights(2), directional=synth.directional_light())
    pv = synth.per_view(W, H)
    out = capi.empty_image(H, W, abi.FMT_RGBA16F, "cuda")
    gbuf = abi.GBuffer(*(g.data_ptr() for g in gb), W, H, W)
    ip = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(3)]      # every pixel: material 0, uv 0
    quv = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    inter = abi.Interpolants(ip[0].data_ptr(), ip[1].data_ptr(), ip[2].data_ptr(), W, H, W)
    mats = (abi.MaterialDesc * 1)()
    light = (C.byref(pf), C.byref(pv), None, 0, None, None, C.c_void_p(out.data_ptr()), W, abi.FMT_RGBA16F)
    calls = {"vqhip_forward_lighting": (lib.vqhip_forward_lighting, (hnd, st, C.byref(gbuf)) + light),
             "vqhip_forward_lighting_from_materials_quad": (lib.vqhip_forward_lighting_from_materials_quad,
                                                            (hnd, st, C.byref(inter), mats, 1, None) + light + (None, C.c_void_p(quv.data_ptr()), 0))}
    result = {"library": capi.lib_path(), "frame": [W, H], "calls_per_batch": args.calls}
    for name, (fn, a) in calls.items():
        for _ in range(args.calls):                                                  # warm-up: the kernels' first launch, the ring's first lap
            assert fn(*a) == 0, ctx.lib.vqhip_last_error(hnd)
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.batches):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn(*a)
            per_call.append((time.perf_counter() - t0) / args.calls * 1e6)
            torch.cuda.synchronize()
        result[name] = {"median_us": round(statistics.median(per_call), 3), "min_us": round(min(per_call), 3)}
    ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
