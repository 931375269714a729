"""vqhip_scene_interpolants (docs/DESIGN_DETAILS.md §7.18) at 3840 x 2160 on two scenes — the room of the tests seen from inside (26 large triangles: nearly every
wave shares one owner) and a field of 320 instanced spheres (337 920 triangles a few pixels across: most waves hold many owners) — at 1 sample and at 4 samples
with four layers (one call per layer), with and without the svPosition planes. Needs the GPU.
  (default)   the driver: runs every step as a child process under its own `timeout`, stops at the first step that fails, and writes
              profiles/r16a_scene_interpolants.md (and the JSON beside it): the time per call, GB/s against the bytes the call must move, the share of the
              HBM write rate, the A/B of the one-owner-per-wave path (option interp_form: both forms compared bit for bit, then timed alternately) and
              scripts/ubench/f64_rate's binary64 issue rates if that program has been built (make -C scripts/ubench).
  --step SCENE SAMPLES SV   one step: one JSON line. The owner planes come from vqhip_scene_depth on the same draws; the timed call is the C entry point
              (Context.scene_interpolants_prepared), timed by benchlib.timing._stage_stats (spin-up by time, batches between device events, the median batch).
There is no earlier time to compare with: the call is new."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vqengine_amd import shadow_scene as S    # noqa: E402
from vqengine_amd import surface_scene as SS  # noqa: E402

HBM_WRITE_GBPS = 6290.0          # the measured float4 copy rate of this chip
W, H = 3840, 2160
STEP_TIMEOUT_S = 240
ROOM_MIN, ROOM_MAX = np.array([-3.0, -2.0, -5.0]), np.array([4.0, 2.5, 6.0])
OCCLUDERS = (((2.5, 0.6, -0.9), (0.2, 0.5, 0.6)), ((-1.8, -0.5, 1.2), (0.2, 0.4, 0.5)), ((0.7, 1.6, -0.8), (0.5, 0.15, 0.4)),
             ((-0.6, -1.2, 0.9), (0.4, 0.15, 0.5)), ((-0.9, 0.5, 3.5), (0.6, 0.4, 0.25)), ((0.8, -0.4, -3.0), (0.5, 0.5, 0.25)))


def room_draws():
    """(vertices, indices, worlds, material, cull) per draw: the room from inside and its six occluders"""
    vp = S.camera_view_proj((0.5, 0.2, -1.0), (0.9, 0.0, 2.0), np.radians(70.0), W / H, 0.1, 15.0)
    pvp = S.camera_view_proj((0.42, 0.25, -1.1), (0.95, -0.05, 2.0), np.radians(70.0), W / H, 0.1, 15.0)
    centre, half = 0.5 * (ROOM_MIN + ROOM_MAX), 0.5 * (ROOM_MAX - ROOM_MIN)
    return [(SS.room(tuple(half)), [S.translation(centre)], 0, 0), (SS.box((1.0, 1.0, 1.0)), [S.scaling(h) @ S.translation(c) for c, h in OCCLUDERS], 1, 0)], vp, pvp


def sphere_field_draws(n=320, seed=16):
    """320 spheres of 1056 triangles in five draws of 64 instances, scattered through the frustum"""
    rng = np.random.default_rng(seed)
    vp = S.camera_view_proj((0.0, 2.0, -14.0), (0.0, 0.0, 6.0), np.radians(60.0), W / H, 0.5, 80.0)
    pvp = S.camera_view_proj((0.1, 2.0, -14.2), (0.0, 0.0, 6.0), np.radians(60.0), W / H, 0.5, 80.0)
    mesh = SS.uv_sphere(1.0, 24, 23)
    worlds = [S.scaling(rng.uniform(0.4, 1.3)) @ S.rotation_y(rng.uniform(0, 6.28)) @ S.translation((rng.uniform(-16, 16), rng.uniform(-7, 9), rng.uniform(-4, 30)))
              for _ in range(n)]
    return [(mesh, worlds[k:k + 64], k // 64, 2) for k in range(0, n, 64)], vp, pvp


SCENES = {"room": room_draws, "sphere_field": sphere_field_draws}


def step(scene, samples, sv):
    import torch
    from benchlib.timing import _stage_stats
    from vqengine_amd import capi
    ctx = capi.Context(0)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    specs, vp, pvp = SCENES[scene]()
    draws, culls = [], []
    for (v, idx), worlds, material, cull in specs:
        wvp, world, normal, prev = SS.instance_matrices_full(worlds, vp, pvp)
        draws.append(capi.SurfaceDraw(dev(v), dev(idx.astype(np.int32)), dev(wvp), dev(world), dev(normal), dev(prev), material))
        culls.append(cull)
    triangles = sum((d.indices.numel() // 3) * d.wvp.shape[0] for d in draws)
    z = ctx.scene_depth([d.depth_draw(c) for d, c in zip(draws, culls)], W, H, samples, primitive=samples == 1, layers=4 if samples == 4 else 0)
    owners = [z["primitive"]] if samples == 1 else z["layer_primitive"]
    torch.cuda.synchronize()
    calls, owned = [], []
    for o in owners:                                   # one set of targets per layer, as a frame would hold them
        call, res = ctx.scene_interpolants_prepared(draws, W, H, o, sv=sv)
        calls.append((call, res))
        owned.append(int((o != -1).sum()))

    def frame():
        for call, _ in calls:
            call()
    frame()
    torch.cuda.synchronize()
    uniform_waves = []
    for o in owners:                                   # share of 8 x 8 blocks (one wave each) whose 64 pixels hold one q
        b = o.reshape(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64)
        uniform_waves.append(float((b.min(dim=1).values == b.max(dim=1).values).float().mean()))
    # A/B of the one-owner-per-wave path: the same bits first, then both forms timed alternately; the default form's time is the one reported as `call`
    planes = {}
    for form in ("lane", "wave"):
        ctx.set_option("interp_form", form)
        frame()
        torch.cuda.synchronize()
        planes[form] = [t.clone() for _, res in calls for k, t in res.items() if k != "work"]
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(planes["lane"], planes["wave"]))
    del planes
    forms = {"lane": [], "wave": []}
    for _ in range(2):
        for form in ("lane", "wave"):
            ctx.set_option("interp_form", form)
            forms[form].append(_stage_stats(frame, spin_s=0.3, batch_s=0.15)["ms"])
    ctx.set_option("interp_form", None)
    st = _stage_stats(frame, spin_s=0.5, batch_s=0.25)
    px = W * H * len(owners)
    moved = px * (4 + (80 if sv else 48))              # the owner word read, the planes written
    ms = st["ms"]
    print(json.dumps({"scene": scene, "samples": samples, "layers": len(owners), "sv": bool(sv), "width": W, "height": H, "draws": len(draws),
                      "instanced_triangles": triangles, "owned_pixels": owned, "uniform_wave_share": uniform_waves, "call": st,
                      "forms_ms": forms, "forms_same_bits": bool(same), "ms_per_call": ms / len(owners),
                      "bytes_moved": moved, "gbps": moved / (ms * 1e6), "share_of_hbm_write_rate": moved / (ms * 1e6) / HBM_WRITE_GBPS,
                      "store_floor_ms": moved / (HBM_WRITE_GBPS * 1e6), "device": torch.cuda.get_device_name(0)}))
    ctx.close()


def driver(out_md):
    results, failed = [], None
    for scene in SCENES:
        for samples in (1, 4):
            for sv in (0, 1):
                cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", scene, str(samples), str(sv)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    failed = f"step {scene} samples {samples} sv {sv} ended with status {r.returncode}: {r.stderr[-1500:]}"
                    break
                results.append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(r.stdout.strip().splitlines()[-1], flush=True)
            if failed:
                break
        if failed:
            break
    f64 = None
    exe = os.path.join(ROOT, "scripts", "ubench", "f64_rate")
    if not failed and os.path.exists(exe):
        r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
        if r.returncode == 0:
            f64 = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(f64), flush=True)
        else:
            failed = f"f64_rate ended with status {r.returncode}: {r.stderr[-500:]}"
    lines = ["# vqhip_scene_interpolants at 3840 x 2160 (scripts/scene_interpolants_bench.py)", "",
             f"Device: {results[0]['device'] if results else 'none'}. Times are the median batch between device events of the whole call (table copy + kernel),",
             "one call per owner plane; at 4 samples the row is the four calls of a frame. Bytes moved = 4 B/px of owner read + 48 B/px (80 B/px with the",
             f"svPosition planes) written; the share is against the chip's measured float4 copy rate, {HBM_WRITE_GBPS:.0f} GB/s (BASELINE.md). Vertex, index and matrix",
             "fetches are not counted: they hit in cache. There is no earlier time to compare with: the call is new.", "",
             "The last columns are the A/B of the one-owner-per-wave path (option `interp_form`): each form timed twice, alternating, in the same process; the",
             "two forms' planes were compared bit for bit at this size first.", "",
             "| scene | samples | sv planes | calls | ms (all calls) | ms per call | GB/s | share of the copy rate | store floor ms | waves with one owner | lane form ms | wave form ms | same bits |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        lines.append(f"| {r['scene']} ({r['instanced_triangles']} triangles, {r['draws']} draws) | {r['samples']} | {'yes' if r['sv'] else 'no'} | {r['layers']} | "
                     f"{r['call']['ms']:.3f} | {r['ms_per_call']:.3f} | {r['gbps']:.0f} | {100 * r['share_of_hbm_write_rate']:.0f} % | {r['store_floor_ms']:.3f} | "
                     f"{', '.join(f'{100 * u:.0f} %' for u in r['uniform_wave_share'])} | {' / '.join(f'{m:.3f}' for m in r['forms_ms']['lane'])} | "
                     f"{' / '.join(f'{m:.3f}' for m in r['forms_ms']['wave'])} | {'yes' if r['forms_same_bits'] else 'NO'} |")
    if f64:
        lines += ["", "## Binary64 issue rates (scripts/ubench/f64_rate)", "",
                  "G lane-operations/s, 8 independent chains per lane, 8 waves per SIMD: " +
                  ", ".join(f"`{k}` {v}" for k, v in f64.items() if k not in ("bench", "unit")) + "."]
    if failed:
        lines += ["", f"The run stopped early: {failed}"]
    with open(out_md, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(os.path.splitext(out_md)[0] + "_bench.json", "w") as fh:
        json.dump({"bench": "scene_interpolants", "results": results, "f64_rate": f64, "failed": failed}, fh)
        fh.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", nargs=3, metavar=("SCENE", "SAMPLES", "SV"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16a_scene_interpolants.md"))
    a = ap.parse_args()
    if a.step:
        step(a.step[0], int(a.step[1]), bool(int(a.step[2])))
    else:
        sys.exit(driver(a.out))
