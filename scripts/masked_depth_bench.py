"""The alpha-tested rasterisers (docs/DESIGN_DETAILS.md §7.19) on a room with a few hundred masked cards — 300 instanced cards (six draws of 50) with a 256 x 256
checker of 16-texel cells and its full mip chain, inside a box room seen from within — at 1920 x 1080 with 1 and 4 samples, and as one 2048 x 2048 spot-light
view. Needs the GPU. The workload of a `rocprofv3 --kernel-trace --stats` run of its own: per-kernel times come from there (profiles/r17a_masked_depth.md).
  --variant masked   vqhip_scene_masked_depth / vqhip_shadow_masked_depth with the cards masked
  --variant opaque   the same entry points, every material NULL: the existing kernels' instantiations
  --variant base     vqhip_scene_depth / vqhip_shadow_depth (this variant runs on a tree from before the masked entry points, too)
  --tile 32 64       every configuration once per value of the raster_tile option (default: the option's default alone)
  --mode time        instead of the loop: each configuration timed between device events (benchlib.timing._stage_stats), one JSON line
The descriptors are built once (Context.*_prepared): the timed call is the C entry point, not the Python that fills its structures."""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="masked", choices=("masked", "opaque", "base"))
ap.add_argument("--mode", default="loop", choices=("loop", "time"))
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--cards", type=int, default=300)
ap.add_argument("--tile", type=int, nargs="*", default=[None])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose vqengine_amd is measured")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.tree))
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # benchlib
from vqengine_amd import abi, capi   # noqa: E402
from vqengine_amd import shadow_scene as S   # noqa: E402
from vqengine_amd import surface_scene as SS   # noqa: E402

F = np.float32
CHUNK = 50
EYE, AT = (0.0, 0.5, -9.0), (0.0, 0.0, 0.0)
LIGHT, LIGHT_DIR = (0.0, 9.0, -6.0), (0.0, -0.8, 0.55)


def card_mesh():
    """surface_scene.card(1, 1) spelt out, so that --variant base runs on a tree that has no such helper"""
    v = [np.array([(2 * a - 1), (2 * b - 1), 0.0, 0, 0, -1, 1, 0, 0, a, b], dtype=np.float64) for (a, b) in ((0, 0), (0, 1), (1, 1), (1, 0))]
    return np.array(v, dtype=F), np.array([0, 1, 2, 0, 2, 3], dtype=np.int64)


def card_worlds(n, seed=17):
    rng = np.random.default_rng(seed)
    return [S.scaling(rng.uniform(0.3, 0.9, 3)) @ S.rotation_x(rng.uniform(-0.6, 0.6)) @ S.rotation_y(rng.uniform(-0.9, 0.9)) @
            S.translation((rng.uniform(-7, 7), rng.uniform(-4, 4), rng.uniform(-5, 8))) for _ in range(n)]


def checker_chain(size=256, cell=16):
    y, x = np.mgrid[0:size, 0:size]
    img = np.full((size, size, 4), 160, dtype=np.uint8)
    img[..., 3] = np.where(((x // cell) + (y // cell)) % 2 == 1, 255, 0)
    return SS.mip_chain_rgba8(img)


def main():
    import torch
    ctx = capi.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    masked = ARGS.variant == "masked"
    new_entry = ARGS.variant != "base"
    tex = mat = None
    if masked:
        chain, mips = checker_chain()
        dchain = dev(chain)
        tex = abi.Texture2D(dchain.data_ptr(), 256, 256, mips, 0)
        mat = abi.MaterialDesc()
        mat.data.uvScaleOffset = abi.float4(1.0, 1.0, 0.0, 0.0)
        mat.data.textureConfig = 1.0
        mat.texDiffuse = abi.Texture2D(dchain.data_ptr(), 256, 256, mips, abi.MATERIAL_ALPHA_MASKED)
    rv, ri = SS.room((10.0, 6.0, 12.0))
    cv, ci = card_mesh()
    drv, dri, dcv, dci = dev(rv), dev(ri.astype(np.int32)), dev(cv), dev(ci.astype(np.int32))
    worlds = card_worlds(ARGS.cards)

    def draws_of(view_proj):
        Draw = capi.MaskedDraw if new_entry else capi.ShadowDraw
        kw = dict(material=mat, texture=tex) if masked else {}
        wvp, world = S.instance_matrices([np.eye(4)], view_proj)
        out = [Draw(drv, dri, dev(wvp), dev(world), abi.CULL_NONE)]
        for first in range(0, len(worlds), CHUNK):
            wvp, world = S.instance_matrices(worlds[first:first + CHUNK], view_proj)
            out.append(Draw(dcv, dci, dev(wvp), dev(world), abi.CULL_NONE, **kw))
        return out
    w, h = 1920, 1080
    cam = draws_of(S.camera_view_proj(EYE, AT, np.radians(70.0), w / h, 0.1, 60.0))
    lit = draws_of(S.spot_view_proj(LIGHT, LIGHT_DIR, 0.1, 40.0))
    calls = {}
    for samples in (1, 4):
        prep = ctx.scene_masked_depth_prepared if new_entry else ctx.scene_depth_prepared
        calls[f"scene_{w}x{h}_s{samples}"] = prep(cam, w, h, samples, primitive=True, layers=2 if samples == 4 else 0)
    smap = torch.empty((2048, 2048), dtype=torch.float32, device="cuda")
    prep = ctx.shadow_masked_depth_prepared if new_entry else ctx.shadow_depth_prepared
    calls["shadow_2048"] = prep([capi.ShadowView(smap, lit)])
    results = {}
    for name, (call, res), tile in [(n + (f"_tile{t}" if t else ""), c, t) for n, c in calls.items() for t in ARGS.tile]:
        ctx.set_option("raster_tile", tile)
        call()
        torch.cuda.synchronize()
        if ARGS.mode == "loop":
            for _ in range(ARGS.steps):
                call()
            torch.cuda.synchronize()
            continue
        from benchlib.timing import _stage_stats
        results[name] = _stage_stats(call, spin_s=0.5, batch_s=0.25)
        if name.startswith("scene"):
            results[name]["owned_samples"] = int((res["primitive"] != -1).sum())
        else:
            results[name]["covered_texels"] = int((smap < 1.0).sum())
    if ARGS.mode == "time":
        print(json.dumps({"bench": "masked_depth", "variant": ARGS.variant, "cards": ARGS.cards, "device": torch.cuda.get_device_name(0), "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
