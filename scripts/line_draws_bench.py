"""vqhip_line_draws (docs/DESIGN_DETAILS.md §7.24) on the town of scripts/shadow_raster_bench.py under the main camera of scripts/editor_passes_bench.py, at
1920 x 1080 and 3840 x 2160, against the depth vqhip_scene_depth rasterises for the town. Three workloads, the members of RenderSceneBoundingVolumes this call adds:
  boxes        line_scene.bounding_box_draws: the bounding box of every mesh instance of the town (121), in batches of 512 — one instanced draw of the cube
  bounds_wire  line_scene.light_bounds_wire_draws: the 20 lights of scripts/unlit_draws_bench.py at Range 40, their spheres as wire
  axes         line_scene.vertex_axes_draws: the vertex axes of one selected building
and the yardstick in the same process: vqhip_unlit_draws, opaque, on the same lights' bounds (the solid half of the same pass).
Modes:
  (default)    every figure by benchlib.timing._stage_stats (spin-up by time, batches between device events, the median batch); one JSON line
  --mode loop  --steps calls of each, for `rocprofv3 --kernel-trace --stats -- python scripts/line_draws_bench.py --mode loop` (per-kernel times)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from vqengine_amd import abi   # noqa: E402
from vqengine_amd import line_scene as LS   # noqa: E402
from vqengine_amd import shadow_scene as S   # noqa: E402
from vqengine_amd import unlit_scene as US   # noqa: E402
import shadow_raster_bench as B   # noqa: E402
from editor_passes_bench import AT, EYE, FAR, FOV, NEAR, SIZES   # noqa: E402
from unlit_draws_bench import LIFT, RANGE   # noqa: E402

AXIS_SIZE = 1.0


def instance_boxes(meshes):
    """the world-space bounding box of every instance of every mesh"""
    out = []
    for (p, _), worlds, _ in meshes:
        p4 = np.concatenate([np.asarray(p, dtype=np.float64)[:, :3], np.ones((len(p), 1))], axis=1)
        for wd in worlds:
            q = (p4 @ np.asarray(wd, dtype=np.float64))[:, :3]
            out.append((q.min(axis=0), q.max(axis=0)))
    return out


def with_frames(positions):
    """position, normal, tangent per vertex: the normal points away from the mesh's centre, the tangent lies across it"""
    p = np.asarray(positions, dtype=np.float32)[:, :3]
    n = p / np.maximum(np.linalg.norm(p, axis=1, keepdims=True), 1e-6)
    t = np.cross(n, (0.0, 1.0, 0.3))
    return np.concatenate([p, n, t], axis=1).astype(np.float32)


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
    boxes = instance_boxes(meshes)
    building = (with_frames(meshes[1][0][0]), np.asarray(meshes[1][0][1]), meshes[1][1][0])
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
        wire = lambda d: capi.WireframeDraw(dev(d["vertices"]), dev(np.asarray(d["indices"]).astype(np.int32)), dev(d["matrices"]), dev(d["color"]))   # noqa: E731
        sets = {"boxes": [wire(d) for d in LS.bounding_box_draws(boxes, vp)],
                "bounds_wire": [wire(d) for d in LS.light_bounds_wire_draws(lights, vp, sphere)],
                "axes": [capi.VertexAxesDraw(dev(d["vertices"]), dev(np.asarray(d["indices"]).astype(np.int32)), dev(d["cb"]))
                         for d in LS.vertex_axes_draws([building], vp, AXIS_SIZE)]}
        solid = [capi.UnlitDraw(dev(d["vertices"]), dev(np.asarray(d["indices"]).astype(np.int32)), dev(d["cb"]), abi.CULL_BACK)
                 for d in US.light_bounds_draws(lights, vp, sphere, blended=False)]
        calls, outs = {}, {}
        for name, draws in sets.items():
            calls[name], outs[name] = ctx.line_draws_prepared(draws, w, h, color, depth)
        calls["bounds_solid_unlit_draws"], outs["bounds_solid_unlit_draws"] = ctx.unlit_draws_prepared(solid, w, h, color, depth, blend=False)
        lines = {"boxes": sum(d.indices.numel() * d.matrices.shape[0] for d in sets["boxes"]), "bounds_wire": sum(d.indices.numel() for d in sets["bounds_wire"]),
                 "axes": sum(3 * d.indices.numel() for d in sets["axes"])}
        tiles = ((w + 31) // 32) * ((h + 31) // 32)
        row = {"width": w, "height": h, "lights": len(lights), "boxes": len(boxes), "range": RANGE}
        for name, call in calls.items():
            call()
            torch.cuda.synchronize()
            row[name] = {"touched_pixels": int((outs[name]["writer"] != -1).sum())}
            if name in lines:
                row[name].update(lines=lines[name], draws=len(sets[name]), box_bytes_scanned=tiles * lines[name] * 8)
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
        print(json.dumps({"bench": "line_draws", "device": torch.cuda.get_device_name(0), "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
