"""Helper-lane derivatives for the lit draw (docs/DESIGN_DETAILS.md §7.20) at 3840 x 2160 on §7.18's two scenes (scripts/scene_interpolants_bench.py: the room from
inside, the field of 320 instanced spheres), at 1 sample and at 4 samples with four layers (one call per layer). Needs the GPU. Within one process, alternating:
  resolve    vqhip_scene_interpolants against vqhip_scene_quad_interpolants (both with the svPosition planes)
  lit draw   vqhip_forward_lighting_from_materials against its _quad form, vqhip_gbuffer_from_materials against its _quad form, on the resolve's planes with the
             12-material table of §7.1 (synth.material_set(12, max_dim=1024), the one scripts/bench_gbuffer.py builds: 56 maps), SSAO on; PSMain also under
             the opt-in 4-wave cap (option psmain_waves)
  (default)  the driver: every step as a child process under its own `timeout`, stops at the first step that fails, writes profiles/r19a_quad_derivatives.md
  --step SCENE SAMPLES   one step: one JSON line
Derivable: +16 B/px written by the resolve, +16 B/px read by the producer, two more `den` and four more quotients per owned pixel in the resolve."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import scene_interpolants_bench as B          # noqa: E402
from vqengine_amd import surface_scene as SS  # noqa: E402

W, H = B.W, B.H
STEP_TIMEOUT_S = 300


def step(scene, samples):
    import torch
    from benchlib.timing import _stage_stats
    from vqengine_amd import abi, capi, synth
    ctx = capi.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    specs, vp, pvp = B.SCENES[scene]()
    draws, culls = [], []
    for (v, idx), worlds, material, cull in specs:
        wvp, world, normal, prev = SS.instance_matrices_full(worlds, vp, pvp)
        draws.append(capi.SurfaceDraw(dev(v), dev(idx.astype(np.int32)), dev(wvp), dev(world), dev(normal), dev(prev), material))
        culls.append(cull)
    z = ctx.scene_depth([d.depth_draw(c) for d, c in zip(draws, culls)], W, H, samples, primitive=samples == 1, layers=4 if samples == 4 else 0)
    owners = [z["primitive"]] if samples == 1 else z["layer_primitive"]
    torch.cuda.synchronize()
    plain = [ctx.scene_interpolants_prepared(draws, W, H, o, sv=True) for o in owners]
    quad = [ctx.scene_quad_interpolants_prepared(draws, W, H, o, sv=True) for o in owners]

    def alternate(a, b, rounds=2):
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(_stage_stats(a, spin_s=0.3, batch_s=0.15)["ms"])
            tb.append(_stage_stats(b, spin_s=0.3, batch_s=0.15)["ms"])
        return ta, tb
    res_plain, res_quad = alternate(lambda: [c() for c, _ in plain], lambda: [c() for c, _ in quad])
    torch.cuda.synchronize()
    same = all(torch.equal(p[k].view(torch.int32), q[k].view(torch.int32)) for (_, p), (_, q) in zip(plain, quad) for k in ("ip0", "ip1", "ip2", "sv_curr", "sv_prev"))

    datas, texsets = synth.material_set(12, max_dim=1024)
    dmats, keep, nmaps = (abi.MaterialDesc * 12)(), [], 0
    for i, (d, ts) in enumerate(zip(datas, texsets)):
        dmats[i].data = d
        for slot, img in ts.items():
            chain, nm = ctx.mip_chain_rgba8(dev(img))
            keep.append(chain)
            setattr(dmats[i], slot, abi.Texture2D(chain.data_ptr(), img.shape[1], img.shape[0], nm, 0))
            nmaps += 1
    ssao = dev(synth.ssao_image(W, H))
    pf, extra = synth.per_frame(points=synth.point_lights(64), spots=synth.spot_lights(2), directional=synth.directional_light())
    pv = synth.per_view(W, H)
    ips = [([r[k] for k in ("ip0", "ip1", "ip2")], r["quad_uv"]) for _, r in quad]
    col = capi.empty_image(H, W, abi.FMT_RGBA16F, ctx.device)
    gb = tuple(torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(4))
    fwd_plain, fwd_quad = alternate(lambda: [ctx.forward_lighting_from_materials(ip, dmats, pf, pv, ssao=ssao, out=col, extra_point=extra) for ip, _ in ips],
                                    lambda: [ctx.forward_lighting_from_materials_quad(ip, dmats, pf, pv, q, ssao=ssao, out=col, extra_point=extra) for ip, q in ips])
    ctx.set_option("psmain_waves", "4")                # the opt-in 4-wave cap of the fused kernel (default 6)
    fwd4_plain, fwd4_quad = alternate(lambda: [ctx.forward_lighting_from_materials(ip, dmats, pf, pv, ssao=ssao, out=col, extra_point=extra) for ip, _ in ips],
                                      lambda: [ctx.forward_lighting_from_materials_quad(ip, dmats, pf, pv, q, ssao=ssao, out=col, extra_point=extra) for ip, q in ips])
    ctx.set_option("psmain_waves", None)
    gb_plain, gb_quad = alternate(lambda: [ctx.gbuffer_from_materials(ip, dmats, pf.fAmbientLightingFactor, ssao, out=gb) for ip, _ in ips],
                                  lambda: [ctx.gbuffer_from_materials_quad(ip, dmats, pf.fAmbientLightingFactor, q, ssao=ssao, out=gb) for ip, q in ips])
    print(json.dumps({"scene": scene, "samples": samples, "layers": len(owners), "width": W, "height": H, "maps": nmaps, "five_planes_same_bits": bool(same),
                      "resolve_ms": {"plain": res_plain, "quad": res_quad}, "forward_ms": {"plain": fwd_plain, "quad": fwd_quad}, "forward_4waves_ms": {"plain": fwd4_plain, "quad": fwd4_quad},
                      "gbuffer_ms": {"plain": gb_plain, "quad": gb_quad}, "device": torch.cuda.get_device_name(0)}))
    ctx.close()


def driver(out_md):
    results, failed = [], None
    for scene in B.SCENES:
        for samples in (1, 4):
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", scene, str(samples)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                failed = f"step {scene} samples {samples} ended with status {r.returncode}: {r.stderr[-1500:]}"
                break
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(r.stdout.strip().splitlines()[-1], flush=True)
        if failed:
            break
    f = lambda t: " / ".join(f"{m:.3f}" for m in t)      # noqa: E731
    lines = ["# Helper-lane derivatives for the lit draw at 3840 x 2160 (scripts/quad_interpolants_bench.py)", "",
             f"Device: {results[0]['device'] if results else 'none'}. Median batch between device events; each form timed twice, alternating with its sibling, in one",
             f"process; at 4 samples a row is the four calls of a frame. Resolve: both forms with the svPosition planes. Lit draw: 12 materials, {results[0]['maps'] if results else 0} maps, SSAO, 64 point",
             "lights, on the resolve's planes. The sibling columns are the parent's kernels (unchanged instantiations), measured in the same session.", "",
             "| scene | samples | resolve ms | quad resolve ms | PSMain ms | PSMain _quad ms | PSMain, 4 waves, ms | PSMain _quad, 4 waves, ms | G-buffer ms | G-buffer _quad ms | five planes same bits |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        lines.append(f"| {r['scene']} | {r['samples']} | {f(r['resolve_ms']['plain'])} | {f(r['resolve_ms']['quad'])} | {f(r['forward_ms']['plain'])} | {f(r['forward_ms']['quad'])} | {f(r['forward_4waves_ms']['plain'])} | {f(r['forward_4waves_ms']['quad'])} | "
                     f"{f(r['gbuffer_ms']['plain'])} | {f(r['gbuffer_ms']['quad'])} | {'yes' if r['five_planes_same_bits'] else 'NO'} |")
    if failed:
        lines += ["", f"The run stopped early: {failed}"]
    with open(out_md, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(os.path.splitext(out_md)[0] + "_bench.json", "w") as fh:
        json.dump({"bench": "quad_derivatives", "results": results, "failed": failed}, fh)
        fh.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", nargs=2, metavar=("SCENE", "SAMPLES"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19a_quad_derivatives.md"))
    a = ap.parse_args()
    if a.step:
        step(a.step[0], int(a.step[1]))
    else:
        sys.exit(driver(a.out))
