"""The two editor passes (docs/DESIGN_DETAILS.md §7.21) on the town of scripts/shadow_raster_bench.py under a main camera, at 1920 x 1080 and 3840 x 2160:
  object_ids   vqhip_object_ids alone over the owner plane of the pass's cull-NONE depth call, in both forms (interp_form wave | lane), with the bytes the
               resolve must move (4 B of owner in, 16 B of ids out per pixel) against the measured time
  chain        the whole ObjectID pass: vqhip_scene_depth with every cull mode NONE + vqhip_object_ids
  outline_1    vqhip_outline with one sphere selected;  outline_20  with all 20 spheres selected (selection and writer planes on)
Modes:
  (default)    every figure by benchlib.timing._stage_stats (spin-up by time, batches between device events, the median batch); one JSON line
  --mode loop  --steps calls of each, for `rocprofv3 --kernel-trace --stats -- python scripts/editor_passes_bench.py --mode loop` (per-kernel times)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from vqengine_amd import abi   # noqa: E402
from vqengine_amd import outline_scene as OS   # noqa: E402
from vqengine_amd import shadow_scene as S   # noqa: E402
from vqengine_amd import surface_scene as SS   # noqa: E402
import shadow_raster_bench as B   # noqa: E402

HBM_COPY_GBPS = 6290.0           # the measured float4 copy rate of this chip
EYE, AT, FOV, NEAR, FAR = (0.0, 45.0, -150.0), (0.0, 5.0, 0.0), np.radians(60.0), 0.5, 400.0
SIZES = ((1920, 1080), (3840, 2160))


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
    sphere_v, sphere_i = SS.uv_sphere(1.0, 48, 47)                     # the town's sphere with normals: the engine's vertex
    assert np.array_equal(sphere_v[:, :3], meshes[2][0][0])
    dsphere_v, dsphere_i = dev(sphere_v), dev(sphere_i.astype(np.int32))
    rng = np.random.default_rng(0x7034)
    results = []
    for (w, h) in SIZES:
        view = S.look_at_lh(EYE, AT, (0.0, 1.0, 0.0))
        proj = S.perspective_fov_lh(FOV, w / h, NEAR, FAR)
        depth_draws, id_draws = [], []
        for k, ((p, i), worlds, _) in enumerate(meshes):
            dp, di = dev(p), dev(i.astype(np.int32))
            for c in range(0, len(worlds), abi.SCENE_DEPTH_MAX_INSTANCES):                          # at most 64 instances to a draw
                chunk = worlds[c:c + abi.SCENE_DEPTH_MAX_INSTANCES]
                wvp, _ = S.instance_matrices(chunk, view @ proj)
                depth_draws.append(capi.ShadowDraw(dp, di, dev(wvp), None, abi.CULL_NONE))        # the ObjectID pass: cull NONE for every draw
                obj = rng.integers(1, 2 ** 20, size=(len(chunk), 4)).astype(np.int32)
                id_draws.append(capi.ObjectIdDraw(di.numel(), dev(obj), k + 1, 10 + k))
        tris = sum((d.indices.numel() // 3) * d.wvp.shape[0] for d in depth_draws)
        depth_call, z = ctx.scene_depth_prepared(depth_draws, w, h, 1, primitive=True)
        ids_call, ids = ctx.object_ids_prepared(id_draws, w, h, z["primitive"])
        color = torch.zeros((h, w, 4), dtype=torch.float16, device="cuda")
        spheres = meshes[2][1]
        sel = [capi.OutlineDraw(dsphere_v, dsphere_i, dev(OS.outline_data(wd, view, proj))) for wd in spheres]
        # the one sphere: the one whose centre lands nearest to the middle of the screen
        centres = np.array([(np.array([0, 0, 0, 1.0]) @ wd @ view @ proj) for wd in spheres])
        ndc = centres[:, :2] / centres[:, 3:4]
        one = int(np.argmin(np.where(centres[:, 3] > NEAR, (ndc ** 2).sum(axis=1), np.inf)))
        out1_call, out1 = ctx.outline_prepared([sel[one]], w, h, color)
        out20_call, out20 = ctx.outline_prepared(sel, w, h, color)

        def chain():
            depth_call()
            ids_call()
        calls = {"object_ids_wave": ("wave", ids_call), "object_ids_lane": ("lane", ids_call), "depth_cull_none": (None, depth_call), "chain": (None, chain),
                 "outline_1": (None, out1_call), "outline_20": (None, out20_call)}
        depth_call(); ids_call(); out20_call()
        torch.cuda.synchronize()
        owned = int((z["primitive"] != -1).sum())
        row = {"width": w, "height": h, "draws": len(depth_draws), "instanced_triangles": tris, "owned_pixels": owned,
               "ids_bytes_moved": 20 * w * h, "ids_copy_floor_ms": 20 * w * h / (HBM_COPY_GBPS * 1e6),
               "outline_20": {"triangles": sum(d.indices.numel() // 3 for d in sel), "marked": int(out20["selection"].sum()), "written": int((out20["writer"] != -1).sum())}}
        out1_call()
        torch.cuda.synchronize()
        row["outline_1"] = {"sphere": one, "triangles": sel[one].indices.numel() // 3, "marked": int(out1["selection"].sum()), "written": int((out1["writer"] != -1).sum())}
        for name, (form, call) in calls.items():
            ctx.set_option("interp_form", form)
            if a.mode == "loop":
                for _ in range(a.steps):
                    call()
                torch.cuda.synchronize()
                continue
            st = _stage_stats(call, spin_s=0.3, batch_s=0.15)
            row.setdefault("ms", {})[name] = st
        ctx.set_option("interp_form", None)
        if a.mode == "time":
            for form in ("wave", "lane"):
                row[f"ids_gb_per_s_{form}"] = row["ids_bytes_moved"] / (row["ms"][f"object_ids_{form}"]["ms"] * 1e6)
        results.append(row)
        del depth_call, ids_call, out1_call, out20_call, z, ids, out1, out20, color
        torch.cuda.empty_cache()
    if a.mode == "time":
        print(json.dumps({"bench": "editor_passes", "device": torch.cuda.get_device_name(0), "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
