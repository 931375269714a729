"""vqhip_shadow_depth (docs/DESIGN_DETAILS.md §7.16) on the engine's shadow-map layout — one 2048^2 directional map, five 1024^2 spot maps and thirty 1024^2
point-light faces, all 36 views in ONE call — with two seeded scenes: one JSON line. Needs the GPU.
  town     a ground grid of 128 x 128 cells, 100 boxes (one draw, 100 instances) and 20 spheres of 4416 triangles (one draw, 20 instances): 122 288 triangles a view
  grid1m   a jittered grid of 708 x 708 cells, 1 002 528 triangles a view, in the first 12 views of the layout (the directional map, the five spot maps, six
           faces: a third of it, since the work buffer holds six records per instanced triangle; --views N for another number)
  (default)        the whole call timed by benchlib.timing._stage_stats (spin-up by time, seven batches between device events, the median batch) for each tile size
                   of k_raster_fill (option raster_tile: 32 and 64), with triangles/s, covered texels/s and the bytes of the maps against the HBM write rate.
  --mode loop      N calls and a synchronise: the workload of a `rocprofv3 --kernel-trace --stats` run of its own (kernel times come from there, not from events).
The descriptors are built once (Context.shadow_depth_prepared): the timed call is the C entry point, not the Python that fills its structures."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqengine_amd import abi   # noqa: E402
from vqengine_amd import shadow_scene as S   # noqa: E402

HBM_WRITE_GBPS = 6290.0          # B/s / 1e9: the measured float4 copy rate of this chip, the floor for storing the maps once
LAYOUT = (2048, 1024, 1024)      # SceneRendering.cpp:1128, 1166, 1219
NEAR, FAR = 0.5, 400.0


def town(seed=0x7031):
    rng = np.random.default_rng(seed)
    ground = S.grid(128, 240.0, 0.3, seed)
    boxes = [S.scaling(rng.uniform(2.0, 9.0, 3)) @ S.rotation_y(rng.uniform(0, 6.28)) @ S.translation((rng.uniform(-100, 100), rng.uniform(2, 9), rng.uniform(-100, 100)))
             for _ in range(100)]
    spheres = [S.scaling(rng.uniform(2.0, 6.0)) @ S.translation((rng.uniform(-100, 100), rng.uniform(3, 20), rng.uniform(-100, 100))) for _ in range(20)]
    return [(ground, [np.eye(4)], abi.CULL_NONE), (S.box((1, 1, 1)), boxes, abi.CULL_BACK), (S.uv_sphere(1.0, 48, 47), spheres, abi.CULL_BACK)]


def grid1m(seed=0x7032):
    return [(S.grid(708, 240.0, 0.3, seed), [np.eye(4)], abi.CULL_NONE)]


def light_views(n_views, seed=0x7033):
    """(dim, view-projection, linear, position, far) of the layout's first n_views views: directional, spots, then the faces of the point lights"""
    rng = np.random.default_rng(seed)
    out = [(LAYOUT[0], S.directional_view_proj((0.3, -1.0, 0.2), 150.0, (260.0, 260.0), NEAR, FAR), False, (0, 0, 0), 1.0)]
    for _ in range(abi.NUM_SHADOWING_LIGHTS__SPOT):
        pos = (rng.uniform(-60, 60), rng.uniform(25, 45), rng.uniform(-60, 60))
        out.append((LAYOUT[1], S.spot_view_proj(pos, (rng.uniform(-0.4, 0.4), -1.0, rng.uniform(-0.4, 0.4)), NEAR, FAR, up=(0, 0, 1)), False, pos, FAR))
    for _ in range(abi.NUM_SHADOWING_LIGHTS__POINT):
        pos = (rng.uniform(-60, 60), rng.uniform(8, 25), rng.uniform(-60, 60))
        out += [(LAYOUT[2], S.point_face_view_proj(pos, f, NEAR, 150.0), True, pos, 150.0) for f in range(6)]
    return out[:n_views]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=("time", "loop"))
    ap.add_argument("--scene", default="both", choices=("town", "grid1m", "both"))
    ap.add_argument("--views", type=int, default=0, help="views of the layout to draw (default: 36 for town, 12 for grid1m)")
    ap.add_argument("--tile", type=int, nargs="*", default=[32, 64])
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from benchlib.timing import _stage_stats
    from vqengine_amd import capi
    ctx = capi.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    results = []
    for name in (("town", "grid1m") if a.scene == "both" else (a.scene,)):
        meshes = town() if name == "town" else grid1m()
        lights = light_views(a.views or (36 if name == "town" else 12))
        dmesh = [(dev(p), dev(i.astype(np.int32)), worlds, cull) for (p, i), worlds, cull in meshes]
        views, maps = [], []
        for dim, vp, linear, pos, far in lights:
            draws = []
            for p, i, worlds, cull in dmesh:
                wvp, world = S.instance_matrices(worlds, vp)
                draws.append(capi.ShadowDraw(p, i, dev(wvp), dev(world), cull))
            maps.append(torch.empty((dim, dim), dtype=torch.float32, device="cuda"))
            views.append(capi.ShadowView(maps[-1], draws, linear, pos, far))
        triangles = sum(v.instanced_triangles() for v in views)
        call, work = ctx.shadow_depth_prepared(views)
        map_bytes = sum(4 * m.numel() for m in maps)
        row = {"scene": name, "views": len(views), "instanced_triangles": triangles, "work_bytes": work.numel(), "map_bytes": map_bytes,
               "map_store_floor_ms": map_bytes / (HBM_WRITE_GBPS * 1e6), "tiles": {}}
        for tile in a.tile:
            ctx.set_option("raster_tile", tile)
            call()
            torch.cuda.synchronize()
            if a.mode == "loop":
                for _ in range(a.steps):
                    call()
                torch.cuda.synchronize()
                continue
            covered = int(sum(int((m != 1.0).sum()) for m in maps))
            records = int(work[:4 * len(views)].view(torch.int32).sum())
            st = _stage_stats(call, spin_s=0.5, batch_s=0.25)
            row["tiles"][str(tile)] = {"call": st, "records": records, "covered_texels": covered, "triangles_per_s": triangles / (st["ms"] * 1e-3),
                                       "covered_texels_per_s": covered / (st["ms"] * 1e-3), "map_store_gb_per_s": map_bytes / (st["ms"] * 1e6)}
        ctx.set_option("raster_tile", None)
        results.append(row)
        del views, maps, work, call, dmesh
        torch.cuda.empty_cache()
    if a.mode == "time":
        print(json.dumps({"bench": "shadow_raster", "device": torch.cuda.get_device_name(0), "layout": LAYOUT, "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
