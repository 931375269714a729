"""The depth chain of an MSAA frame (docs/DESIGN_DETAILS.md §7.10) at 1280x720, 1920x1080 and 3840x2160: one JSON line.
  (a) fused    : vqhip_msaa_resolve_surfaces(hierarchy) — resolve + level 0 + the whole chain (tile kernel + tail); 16 B/px in, 4 * 4/3 B/px out
  (b) hierarchy: vqhip_depth_hierarchy on a resolved plane (MSAA off) — 4 B/px in, 4 * 4/3 B/px out
  (c) surfaces : the normals + roughness resolve kernel (R10G10B10A2 in and out, RGBA16F scene colour, interior pixels mostly)
In one process, the three alternating per step; device events around each call, warm-up, the median over steps. Bytes are counted from the shapes (what the
algorithm must move), divided by the median time, and set against the streaming-copy rate of the chip. Kernel times: a rocprofv3 --kernel-trace --stats
run of its own (profiles/r8a_depth_chain.md)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqengine_amd import abi, capi, synth   # noqa: E402

COPY_RATE = 6.29e12          # B/s, streaming copy on this chip (read + write counted)


def chain_px(w, h):
    return sum(r * c for r, c in abi.depth_hierarchy_shapes(w, h))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1280x720,1920x1080,3840x2160")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    ctx = capi.Context(0)
    out = {"bench": "depth_chain", "steps": args.steps, "warmup": args.warmup, "copy_rate_TBps": COPY_RATE / 1e12, "sizes": []}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(W)
        ms = torch.from_numpy((0.05 + 0.9 * rng.random((H, W, 4), dtype=np.float32)).astype(np.float32)).cuda()
        plane = ms.min(dim=-1).values.contiguous()
        cov = [torch.full((H, W), 0xF, dtype=torch.uint8, device="cuda"), torch.zeros((H, W), dtype=torch.uint8, device="cuda")]
        edge = torch.from_numpy(rng.random((H, W)) < 0.05).cuda()                      # 5 % of the pixels split between the two layers
        cov[0][edge], cov[1][edge] = 0x3, 0xC
        normals = [torch.from_numpy(synth.packed_unit_normals((H, W), seed=k).view(np.int32)).cuda() for k in range(2)]
        gb1 = [torch.from_numpy(rng.random((H, W, 4), dtype=np.float32)).cuda() for _ in range(2)]
        scene = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
        runs = [("fused", lambda: ctx.msaa_resolve_surfaces(ms, hierarchy=True)),
                ("hierarchy", lambda: ctx.depth_hierarchy(plane)),
                ("surfaces", lambda: ctx.msaa_resolve_surfaces(ms, cov, normals=normals, roughness=gb1, out_normals_fmt=abi.FMT_R10G10B10A2_UNORM,
                                                               scene_color=scene, scene_fmt=abi.FMT_RGBA16F))]
        times = {k: [] for k, _ in runs}
        for step in range(args.warmup + args.steps):
            for k, fn in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                if step >= args.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        px, cpx = W * H, chain_px(W, H)
        # bytes by construction. surfaces: 16 depth samples + 1 coverage byte per layer + one 4-byte normal and one 16-byte gb1 record per OWNING layer
        # (about 1.05 per pixel here) read, 4 (normals) + 2 (alpha) written
        by = {"fused": 16 * px + 4 * cpx, "hierarchy": 4 * px + 4 * cpx, "surfaces": int((16 + 2 + 1.05 * (4 + 16) + 4 + 2) * px)}
        row = {"width": W, "height": H, "levels": abi.mip_level_count(W, H), "tiles": ((W + 63) // 64) * ((H + 63) // 64)}
        for k, _ in runs:
            med = float(np.median(times[k]))
            row[k] = {"us": round(med, 2), "min_us": round(min(times[k]), 2), "max_us": round(max(times[k]), 2), "bytes": by[k],
                      "TBps": round(by[k] / (med * 1e-6) / 1e12, 3), "share_of_copy_rate": round(by[k] / (med * 1e-6) / COPY_RATE, 3)}
        out["sizes"].append(row)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
