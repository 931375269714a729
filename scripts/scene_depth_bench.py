"""vqhip_scene_depth (docs/DESIGN_DETAILS.md §7.17) on the town of scripts/shadow_raster_bench.py — a ground grid of 128 x 128 cells, 100 instanced boxes (two
draws of 50: the pre-pass takes at most 64 instances a draw) and 20 instanced spheres, 122 288 triangles — seen from a camera above its edge, at 1920 x 1080 and
3840 x 2160, with 1 and 4 samples per pixel, depth + primitive + two layers of masks at 4x: one JSON line. Needs the GPU.
  (default)        the whole call timed by benchlib.timing._stage_stats (spin-up by time, seven batches between device events, the median batch) for each size,
                   sample count and (at 1 sample) tile size of k_scene_fill, with triangles/s, covered samples/s, the output bytes against the HBM write rate
                   and how many records the tiles queue (max / median / sum over the tiles, from the boxes in the work buffer).
  --mode loop      N calls of every configuration and a synchronise: the workload of a `rocprofv3 --kernel-trace --stats` run of its own (per-kernel times come
                   from there, not from events).
The descriptors are built once (Context.scene_depth_prepared): the timed call is the C entry point, not the Python that fills its structures."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vqengine_amd import shadow_scene as S   # noqa: E402
from shadow_raster_bench import town   # noqa: E402

HBM_WRITE_GBPS = 6290.0          # B/s / 1e9: the measured float4 copy rate of this chip, the floor for storing the outputs once
SIZES = ((1920, 1080), (3840, 2160))
CHUNK = 50                       # instances per draw: at most abi.SCENE_DEPTH_MAX_INSTANCES
EYE, AT, FOV_Y, NEAR, FAR = (-110.0, 28.0, -125.0), (10.0, 2.0, 5.0), np.radians(60.0), 0.5, 600.0


def draws_of(w, h, dev, capi):
    vp = S.camera_view_proj(EYE, AT, FOV_Y, w / h, NEAR, FAR)
    out = []
    for (p, i), worlds, cull in town():
        dp, di = dev(p), dev(i.astype(np.int32))
        for first in range(0, len(worlds), CHUNK):
            wvp, _ = S.instance_matrices(worlds[first:first + CHUNK], vp)
            out.append(capi.ShadowDraw(dp, di, dev(wvp), None, cull))
    return out


def tile_queue_lengths(work, records, w, h, tile):
    """how many records each tile of k_scene_fill queues, from the pixel boxes the setup kernel left in the work buffer (8 B each, behind the 256-byte counter
    block): a 2-D difference array over the tile grid. Returns (max, median, sum) over the tiles."""
    import torch
    bb = work[256:256 + 8 * records].view(torch.int32).to(torch.int64).reshape(-1, 2)
    i0, i1, j0, j1 = (bb[:, 0] & 0xFFFF) // tile, ((bb[:, 0] >> 16) & 0xFFFF) // tile, (bb[:, 1] & 0xFFFF) // tile, ((bb[:, 1] >> 16) & 0xFFFF) // tile
    tx, ty = (w + tile - 1) // tile, (h + tile - 1) // tile
    d = torch.zeros((ty + 1) * (tx + 1), dtype=torch.int64, device=work.device)
    one = torch.ones_like(i0)
    for jj, ii, sign in ((j0, i0, 1), (j0, i1 + 1, -1), (j1 + 1, i0, -1), (j1 + 1, i1 + 1, 1)):
        d.index_add_(0, jj * (tx + 1) + ii, sign * one)
    n = d.reshape(ty + 1, tx + 1).cumsum(0).cumsum(1)[:ty, :tx].reshape(-1)
    return int(n.max()), int(n.median()), int(n.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=("time", "loop"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=2)
    a = ap.parse_args()
    import torch
    from benchlib.timing import _stage_stats
    from vqengine_amd import capi
    ctx = capi.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    results = []
    for w, h in SIZES:
        draws = draws_of(w, h, dev, capi)
        triangles = sum((d.indices.numel() // 3) * d.wvp.shape[0] for d in draws)
        for samples in (1, 4):
            layers = a.layers if samples == 4 else 0
            call, res = ctx.scene_depth_prepared(draws, w, h, samples, primitive=True, layers=layers)
            out_bytes = sum(t.numel() * t.element_size() for k, v in res.items() if k != "work" for t in (v if isinstance(v, list) else [v]))
            for tile in ((32, 64) if samples == 1 else (32,)):
                ctx.set_option("raster_tile", tile)
                call()
                torch.cuda.synchronize()
                if a.mode == "loop":
                    for _ in range(a.steps):
                        call()
                    torch.cuda.synchronize()
                    continue
                covered = int((res["primitive"] != -1).sum())
                records = int(res["work"][:4].view(torch.int32)[0])
                qmax, qmed, qsum = tile_queue_lengths(res["work"], records, w, h, tile)
                st = _stage_stats(call, spin_s=0.5, batch_s=0.25)
                results.append({"width": w, "height": h, "samples": samples, "layers": layers, "tile": tile, "draws": len(draws), "instanced_triangles": triangles,
                                "records": records, "tile_queue": {"max": qmax, "median": qmed, "sum": qsum}, "covered_samples": covered, "work_bytes": res["work"].numel(), "output_bytes": out_bytes,
                                "output_store_floor_ms": out_bytes / (HBM_WRITE_GBPS * 1e6), "call": st, "triangles_per_s": triangles / (st["ms"] * 1e-3),
                                "covered_samples_per_s": covered / (st["ms"] * 1e-3)})
            ctx.set_option("raster_tile", None)
            del call, res
            torch.cuda.empty_cache()
    if a.mode == "time":
        print(json.dumps({"bench": "scene_depth", "device": torch.cuda.get_device_name(0), "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
