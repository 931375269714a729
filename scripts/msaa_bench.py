"""vqhip_forward_lighting_msaa against vqhip_forward_lighting on the cfg3 frame (3840x2160, 64 point lights + IBL, RGBA16F): one JSON line.
In one process, alternating per step: forward_lighting on layer 0, then the MSAA call with two layers at split fractions 0, 2, 5, 15 %
(synth.gbuffer_msaa "edges"). Device events, warm-up; the median over steps. Kernel times: a rocprofv3 --kernel-trace --stats run of its own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqengine_amd import abi, capi, synth   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fractions", default="0,0.02,0.05,0.15")
    args = ap.parse_args()
    W, H = args.width, args.height
    ctx = capi.Context(0)
    eq = torch.from_numpy(synth.equirect(2048, 2048)).cuda()              # bench.py's cfg3 IBL inputs
    chain, n = ctx.mip_chain(eq)
    pre = ctx.envmap_prefilter(chain, 2048, 2048, n, 64, 0.010, 128, abi.CONV_SEQUENTIAL)
    lut = ctx.brdf_lut(1024, 2048, abi.FMT_RG16F)
    env = capi.make_envmap(pre["diffuse_blurred"], pre["specular"], 128, pre["spec_mips"], lut)
    pf, extra = synth.per_frame(points=synth.point_lights(64, seed=0x6400), hdri_offset=0.3)
    pv = synth.per_view(W, H, max_env_lod=pre["spec_mips"])
    fractions = [float(f) for f in args.fractions.split(",")]
    cases = []
    for f in fractions:
        gbs, cov = synth.gbuffer_msaa(W, H, 2, f, seed=0x6400)
        own = np.stack([(c != 0) & (c != 0xF) for c in cov]).any(0)
        cases.append((f, int(own.sum()), [[torch.from_numpy(p).cuda() for p in g] for g in gbs], [torch.from_numpy(c).cuda() for c in cov]))
    out = torch.empty((H, W, 4), dtype=torch.float16, device="cuda")
    base = lambda: ctx.forward_lighting(cases[0][2][0], pf, pv, out=out, out_fmt=abi.FMT_RGBA16F, extra_point=extra, env=env)   # noqa: E731
    runs = [("forward_lighting", base)] + [(f"msaa_{c[0]:g}", (lambda c=c: ctx.forward_lighting_msaa(c[2], c[3], pf, pv, out=out, out_fmt=abi.FMT_RGBA16F,
                                                                                                  extra_point=extra, env=env))) for c in cases]
    times = {k: [] for k, _ in runs}
    for step in range(args.warmup + args.steps):
        for k, fn in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if step >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"bench": "msaa", "width": W, "height": H, "lights": 64, "env": True, "out_fmt": "RGBA16F", "steps": args.steps, "warmup": args.warmup,
           "forward_lighting_ms": round(med["forward_lighting"], 4),
           "msaa": [{"split_fraction_requested": f, "split_pixels": s, "split_fraction": round(s / (W * H), 4), "ms": round(med[f"msaa_{f:g}"], 4),
                     "ratio": round(med[f"msaa_{f:g}"] / med["forward_lighting"], 4), "spread_ms": [round(min(times[f"msaa_{f:g}"]), 4), round(max(times[f"msaa_{f:g}"]), 4)]}
                    for f, s, _, _ in cases],
           "forward_lighting_spread_ms": [round(min(times["forward_lighting"]), 4), round(max(times["forward_lighting"]), 4)]}
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
