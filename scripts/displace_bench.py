"""vqhip_displace_meshes (docs/DESIGN_DETAILS.md §7.22) measured:
  big      one grid of 1024 x 1024 = 1 Mi vertices (the engine's 44-byte vertex) under a 4096 x 4096 height map, identity tiling
  batch    256 meshes of 289 vertices each in ONE call, two 64 x 64 height maps between them
each at both output strides (full = 44 bytes out per vertex, positions = 12), with the bytes the kernel must move — the vertex read, the stream written, the four
texels of each vertex — set against the measured time and this chip's copy rate; and
  depth    the vqhip_scene_depth call that follows at 1920 x 1080, over the displaced 12-byte stream and over the flat mesh (the rasteriser is unchanged: reported only)
Modes:
  (default)    every figure by benchlib.timing._stage_stats (spin-up by time, batches between device events, the median batch); one JSON line
  --mode loop  --steps calls of each, for `rocprofv3 --kernel-trace --stats -- python scripts/displace_bench.py --mode loop` (per-kernel times)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vqengine_amd import abi   # noqa: E402
from vqengine_amd import shadow_scene as S   # noqa: E402
from vqengine_amd import surface_scene as SS   # noqa: E402

HBM_COPY_GBPS = 6290.0           # the measured float4 copy rate of this chip
F = np.float32


def big_grid(n=1024, size=200.0):
    """surface_scene.grid's layout for n x n VERTICES, built without its per-cell loop: (vertices float32 [n * n, 11], indices int32 [6 (n - 1)^2])"""
    u = np.linspace(-0.5 * size, 0.5 * size, n)
    x, z = np.meshgrid(u, u, indexing="xy")
    v = np.zeros((n * n, 11), dtype=F)
    v[:, 0], v[:, 2] = x.reshape(-1), z.reshape(-1)
    v[:, 4], v[:, 6] = 1.0, 1.0
    v[:, 9], v[:, 10] = (x.reshape(-1) / size + 0.5), (z.reshape(-1) / size + 0.5)
    j, i = np.mgrid[0:n - 1, 0:n - 1]
    a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
    idx = np.stack([a, d, c, a, c, b], axis=-1).reshape(-1).astype(np.int32)       # clockwise seen from +y
    return v, idx


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

    def texture(w, h, seed):
        chain, mips = SS.heightmap_chain(w, h, "hill", seed, 1)        # level 0 is all the call reads
        t = dev(chain)
        return abi.Texture2D(t.data_ptr(), w, h, mips, 0), t

    verts, idx = big_grid()
    nv = verts.shape[0]
    dverts, didx = dev(verts), dev(idx)
    hm, hm_keep = texture(4096, 4096, 1)
    calls, outs = {}, {}
    for name, compact in (("big_full", False), ("big_positions", True)):
        calls[name], o = ctx.displace_meshes_prepared([capi.DisplaceJob(dverts, hm, (1.0, 1.0, 0.0, 0.0), 30.0, compact)])
        outs[name] = o[0]
    sv, _ = SS.grid(16, 4.0)
    small = [dev(sv) for _ in range(256)]
    maps = [texture(64, 64, 2), texture(64, 64, 3)]
    for name, compact in (("batch_full", False), ("batch_positions", True)):
        calls[name], outs[name] = ctx.displace_meshes_prepared([capi.DisplaceJob(m, maps[k & 1][0], (2.0, 2.0, 0.1 * (k % 7), 0.0), 1.5, compact)
                                                                for k, m in enumerate(small)])
    for c in calls.values():
        c()
    torch.cuda.synchronize()
    moved = float((outs["big_positions"][:, 1] != dverts[:, 1]).float().mean())

    w, h = 1920, 1080
    vp = S.camera_view_proj((0.0, 120.0, -190.0), (0.0, 10.0, 0.0), np.radians(60.0), w / h, 0.5, 600.0)
    wvp, _ = S.instance_matrices([S.translation((0.0, 0.0, 0.0))], vp)
    dwvp = dev(wvp)
    depth = {}
    for name, pos in (("depth_displaced", outs["big_positions"]), ("depth_flat", dverts)):
        calls[name], depth[name] = ctx.scene_depth_prepared([capi.ShadowDraw(pos, didx, dwvp, None, abi.CULL_BACK)], w, h, 1, primitive=True)
    for name in depth:
        calls[name]()
    torch.cuda.synchronize()
    covered = {name: int((z["depth"] < 1).sum()) for name, z in depth.items()}

    small_v = sv.shape[0]
    bytes_moved = {"big_full": nv * (44 + 44 + 16), "big_positions": nv * (44 + 12 + 16),
                   "batch_full": 256 * small_v * (44 + 44 + 16), "batch_positions": 256 * small_v * (44 + 12 + 16)}
    row = {"vertices_big": nv, "vertices_batch": 256 * small_v, "moved_fraction_big": moved, "triangles_big": idx.size // 3, "depth_covered_pixels": covered,
           "bytes_moved": bytes_moved, "ms": {}}
    for name, call in calls.items():
        if a.mode == "loop":
            for _ in range(a.steps):
                call()
            torch.cuda.synchronize()
            continue
        row["ms"][name] = _stage_stats(call, spin_s=0.3, batch_s=0.15)
    if a.mode == "time":
        row["gb_per_s"] = {k: b / (row["ms"][k]["ms"] * 1e6) for k, b in bytes_moved.items()}
        row["fraction_of_copy_rate"] = {k: g / HBM_COPY_GBPS for k, g in row["gb_per_s"].items()}
        row["copy_floor_ms"] = {k: b / (HBM_COPY_GBPS * 1e6) for k, b in bytes_moved.items()}
        print(json.dumps({"bench": "heightmap_displacement", "device": torch.cuda.get_device_name(0), "hbm_copy_gb_per_s": HBM_COPY_GBPS, "results": row}))
    del hm_keep
    ctx.close()


if __name__ == "__main__":
    main()
