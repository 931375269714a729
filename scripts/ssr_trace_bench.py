"""vqhip_ssr_classify and vqhip_ssr_intersect (docs/DESIGN_DETAILS.md §7.11) on synth.ssr_room and on a white-noise synth.ssr_surfaces frame at 1920x1080 and
3840x2160: one JSON line per mode.
  --mode time  (needs the GPU): in one process, per step and alternating, the calls of the reflection chain that stand next to each other —
               vqhip_depth_hierarchy, vqhip_ssr_environment_fallback, vqhip_ssr_classify, vqhip_ssr_intersect; device events around each call, warm-up,
               the median over the steps. The ray count is read back once, outside the timed window.
  --mode stats (CPU only): rays traced, mean and max iterations per ray, the share of each loop exit and of rays with confidence > 0, from the numpy
               statement of the contract (tests/ssr_trace_ref.py, environment term off).
Kernel registers and occupancy: hipcc -Rpass-analysis=kernel-resource-usage on csrc/ssr_trace.hip (profiles/r9a_ssr_trace.md)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqengine_amd import abi, synth   # noqa: E402

F16, N10 = abi.FMT_RGBA16F, abi.FMT_R10G10B10A2_UNORM


def frames(w, h, spec_mips):
    r = synth.ssr_room(w, h, spec_mips)
    scene, depth, packed, _ = synth.ssr_surfaces(w, h, seed=0xBE00 + w)
    nz = np.random.default_rng(w).integers(0, 256, (128, 128, 2), dtype=np.uint8)
    return [("ssr_room", r["cb"], r["scene"], r["depth"], r["packed"], r["noise"]),
            ("white_noise", synth.ssr_constants(w, h, spec_mips), scene, depth, packed, nz)]


def unorm8(x):
    x = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1))).astype(np.float32)
    return (x * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def mode_stats(sizes):
    from tests import depth_ref
    from tests import ssr_trace_ref as R
    rows = []
    for w, h in sizes:
        for name, cb, scene, depth, packed, nz in frames(w, h, 5):
            sc = scene.astype(np.float16)
            c = R.classify(sc, depth, cb)
            st = {}
            R.intersect(c["rays"], c["rays"].size, sc, depth_ref.hierarchy(depth), packed, N10, unorm8(sc[..., 3].astype(np.float32)), nz, cb, None,
                        np.zeros((h, w, 4), np.float16), stats=st)
            ex = np.bincount(st["exit"], minlength=3) / max(1, st["exit"].size)
            rows.append({"frame": name, "width": w, "height": h, "rays": int(c["rays"].size), "denoiser_tiles": int(c["tiles"].size),
                         "iterations_mean": round(float(st["iterations"].mean()), 3), "iterations_max": int(st["iterations"].max()),
                         "exit_iteration_cap": round(float(ex[0]), 5), "exit_below_most_detailed_mip": round(float(ex[1]), 5), "exit_low_occupancy": round(float(ex[2]), 5),
                         "confidence_above_0": round(float((st["confidence"] > 0).mean()), 4)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return {"bench": "ssr_trace_stats", "rows": rows}


def mode_time(sizes, steps, warmup):
    import torch
    from vqengine_amd import capi
    ctx = capi.Context(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    eq = synth.equirect(256, 128)
    chain = dev(eq.reshape(-1, 4))
    # a prefiltered environment of the library's own making (sizes of the smallest BASELINE config); its content does not change what is timed
    n_mips = abi.mip_level_count(256, 128)
    flat = torch.zeros((abi.mip_chain_px(256, 128, n_mips), 4), dtype=torch.float32, device="cuda")
    flat[: 256 * 128] = chain
    ctx._ck(ctx.lib.vqhip_mip_chain_min_rgba32f(ctx._h, ctx._stream(), flat.data_ptr(), 256, 128, n_mips))
    spec_mips = abi.specular_mip_count(64)
    spec = torch.zeros((abi.cube_px(64, spec_mips), 4), dtype=torch.float16, device="cuda")
    ctx._ck(ctx.lib.vqhip_conv_specular(ctx._h, ctx._stream(), flat.data_ptr(), 256, 128, n_mips, 64, abi.CONV_SEQUENTIAL, spec.data_ptr(), F16))
    lut = torch.zeros((64, 64, 2), dtype=torch.float16, device="cuda")
    ctx._ck(ctx.lib.vqhip_brdf_lut(ctx._h, ctx._stream(), lut.data_ptr(), 64, 128, abi.FMT_RG16F))
    diffuse = torch.zeros((6, 8, 8, 4), dtype=torch.float16, device="cuda")
    env = capi.make_envmap(diffuse, spec, 64, spec_mips, lut)
    torch.cuda.synchronize()
    rows = []
    for w, h in sizes:
        for name, cb, scene, depth, packed, nz in frames(w, h, spec_mips):
            sc, dp, nm, nzd = dev(scene.astype(np.float16)), dev(depth), dev(packed.view(np.int32)), dev(nz)
            levels = ctx.depth_hierarchy(dp)
            rad, r8 = ctx.ssr_environment_fallback(sc, F16, dp, nm, N10, cb, env, F16, extract_roughness=True)
            rays, counters, tiles = ctx.ssr_classify(sc, F16, levels[0], cb)
            torch.cuda.synchronize()
            n_rays, n_tiles = (int(v) for v in counters.cpu().numpy().view(np.uint32))
            runs = [("depth_hierarchy", lambda: ctx.depth_hierarchy(dp)),
                    ("environment_fallback", lambda: ctx.ssr_environment_fallback(sc, F16, dp, nm, N10, cb, env, F16, extract_roughness=True, out=rad)),
                    ("classify", lambda: ctx.ssr_classify(sc, F16, levels[0], cb))]
            runs.append(("intersect", lambda: ctx.ssr_intersect(rays, counters, sc, F16, levels, nm, N10, r8, nzd, cb, env, rad, F16)))
            times = {k: [] for k, _ in runs}
            for step in range(warmup + steps):
                for k, fn in runs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record()
                    torch.cuda.synchronize()
                    if step >= warmup:
                        times[k].append(e0.elapsed_time(e1))
            row = {"frame": name, "width": w, "height": h, "rays": n_rays, "denoiser_tiles": n_tiles}
            for k, _ in runs:
                row[k] = {"ms": round(float(np.median(times[k])), 4), "min_ms": round(min(times[k]), 4), "max_ms": round(max(times[k]), 4)}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    ctx.close()
    return {"bench": "ssr_trace_time", "steps": steps, "warmup": warmup, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["time", "stats"], default="time")
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    if args.mode == "stats":
        print(json.dumps(mode_stats(sizes)))
    else:
        print(json.dumps(mode_time(sizes, args.steps, args.warmup)))


if __name__ == "__main__":
    main()
