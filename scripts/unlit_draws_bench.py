"""vqhip_unlit_draws (docs/DESIGN_DETAILS.md §7.23) on the town of scripts/shadow_raster_bench.py under the main camera of scripts/editor_passes_bench.py, at
1920 x 1080 and 3840 x 2160, against the depth vqhip_scene_depth rasterises for the town. One point light hangs above each of the town's 20 spheres:
  gizmos   unlit_scene.light_mesh_draws: the sphere scaled by 0.1 at every light (a sphere of radius GIZMO_RADIUS, ten times the engine's, so that a gizmo
           covers pixels from this camera) — small, far apart
  bounds   unlit_scene.light_bounds_draws at full range (RANGE): 20 large volumes that overlap each other and most of the screen — the worst case
each in both modes (opaque = UNLIT_PSO, blend = UNLIT_BLEND_PSO), with the bytes the fill must move (per pixel 4 B of depth in, 4 B of writer out, and for every
touched pixel 8 B of colour out, 8 B in for every pixel when blending; per tile the 8-byte box of every triangle, from L2) against the measured time.
Modes:
  (default)    every figure by benchlib.timing._stage_stats (spin-up by time, batches between device events, the median batch); one JSON line
  --mode loop  --steps calls of each, for `rocprofv3 --kernel-trace --stats -- python scripts/unlit_draws_bench.py --mode loop` (per-kernel times)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from vqengine_amd import abi   # noqa: E402
from vqengine_amd import shadow_scene as S   # noqa: E402
from vqengine_amd import unlit_scene as US   # noqa: E402
import shadow_raster_bench as B   # noqa: E402
from editor_passes_bench import AT, EYE, FAR, FOV, HBM_COPY_GBPS, NEAR, SIZES   # noqa: E402

RANGE = 40.0
GIZMO_RADIUS = 10.0
LIFT = 8.0                       # a light sits this far above its sphere's centre: outside the sphere (radius <= 6), so that its gizmo is not hidden in it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=("time", "loop"))
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from benchlib.timing import _stage_stats
    from vqengine_amd import capi
    ctx = capi.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    meshes = B.town()
    sphere = meshes[2][0]
    rng = np.random.default_rng(0x7035)
    lights = [{"type": "point", "position": tuple(wd[3, :3] + (0.0, LIFT, 0.0)), "color": tuple(rng.uniform(0.2, 1.0, 3)), "brightness": float(rng.uniform(500.0, 3000.0)), "range": RANGE}
              for wd in meshes[2][1]]
    dsphere = (dev(sphere[0]), dev(sphere[1].astype(np.int32)))
    dgizmo = dev(sphere[0] * np.float32(GIZMO_RADIUS))
    results = []
    for (w, h) in SIZES:
        vp = S.look_at_lh(EYE, AT, (0.0, 1.0, 0.0)) @ S.perspective_fov_lh(FOV, w / h, NEAR, FAR)
        depth_draws = []
        for (p, i), worlds, cull in meshes:
            dp, di = dev(p), dev(i.astype(np.int32))
            for c in range(0, len(worlds), abi.SCENE_DEPTH_MAX_INSTANCES):
                wvp, _ = S.instance_matrices(worlds[c:c + abi.SCENE_DEPTH_MAX_INSTANCES], vp)
                depth_draws.append(capi.ShadowDraw(dp, di, dev(wvp), None, cull))
        z = ctx.scene_depth(depth_draws, w, h, 1)
        depth = z["depth"].view(h, w)
        color = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
        sets = {"gizmos": US.light_mesh_draws(lights, EYE, vp, sphere),            # the device mesh below is the sphere times GIZMO_RADIUS for this set
                "bounds_opaque": US.light_bounds_draws(lights, vp, sphere, blended=False),
                "bounds_blend": US.light_bounds_draws(lights, vp, sphere, blended=True)}
        dd = {k: [capi.UnlitDraw(dgizmo if k == "gizmos" else dsphere[0], dsphere[1], dev(d["cb"]), abi.CULL_BACK) for d in v] for k, v in sets.items()}
        calls, outs = {}, {}
        for name, key, blend in (("gizmos_opaque", "gizmos", False), ("gizmos_blend", "gizmos", True), ("bounds_opaque", "bounds_opaque", False),
                                 ("bounds_blend", "bounds_blend", True)):
            calls[name], outs[name] = ctx.unlit_draws_prepared(dd[key], w, h, color, depth, blend=blend)
        tris = sum(d.indices.numel() // 3 for d in dd["gizmos"])
        row = {"width": w, "height": h, "lights": len(lights), "triangles": tris, "slots": tris * abi.UNLIT_SLOTS_PER_TRIANGLE, "range": RANGE}
        for name, call in calls.items():
            call()
            torch.cuda.synchronize()
            touched = int((outs[name]["writer"] != -1).sum())
            blend = name.endswith("blend")
            tiles = ((w + 31) // 32) * ((h + 31) // 32)
            moved = 8 * w * h + 8 * touched + (8 * w * h if blend else 0)
            row[name] = {"touched_pixels": touched, "plane_bytes": moved, "plane_floor_ms": moved / (HBM_COPY_GBPS * 1e6),
                         "box_bytes_scanned": tiles * tris * 8}
            if a.mode == "loop":
                for _ in range(a.steps):
                    call()
                torch.cuda.synchronize()
                continue
            row[name]["time"] = _stage_stats(call, spin_s=0.3, batch_s=0.15)
        results.append(row)
        del calls, outs, z, depth, color
        torch.cuda.empty_cache()
    if a.mode == "time":
        print(json.dumps({"bench": "unlit_draws", "device": torch.cuda.get_device_name(0), "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
