"""vqhip_cacao (docs/DESIGN_DETAILS.md §7.14) at 1920 x 1080 and 3840 x 2160 (--size W H for another): one JSON line. Needs the GPU. The frame is synth.cacao_room
ray-cast at 960 x 540 and enlarged by texel replication (the ray cast of eight million pixels would dominate the run); default settings, quality HIGH,
blurPassCount 2, R10G10B10A2_UNORM normals.
  (default)        the whole call — five kernels on torch's current stream — timed by benchlib.timing._stage_stats (spin-up by time, seven batches between device
                   events, the median batch), next to a device-to-device copy of the call's total traffic as the bandwidth yardstick.
  --mode loop      N calls and a synchronise: the workload of a `rocprofv3 --kernel-trace --stats` run of its own (kernel times come from there, not from events).
  --mode kernels   FILE reads the kernel summary of such a run (its rocpd database *.db, or a kernel_stats.csv) and prints, per kernel, the average time next to the bytes the kernel must move (from the shapes,
                   every plane counted once per kernel) and the HBM rate that implies.
Bytes, with P = W * H pixels and T = hw * hh texels per slice: prepare depths reads 4 P and writes the four R16F mips of four slices; prepare normals reads 4 P
and writes 16 T; generate reads the depth mips and the normals and writes 8 T; the blur reads 8 T and writes 8 T; apply reads 8 T and writes P."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqengine_amd import abi, cacao, synth   # noqa: E402

KERNELS = ("k_cacao_prepare_depths", "k_cacao_prepare_normals", "k_cacao_generate", "k_cacao_blur", "k_cacao_apply")


def kernel_bytes(w, h, blur=2):
    hw, hh = abi.cacao_half_dims(w, h)
    p, t = w * h, hw * hh
    mips = sum(4 * abi.mip_dim(hw, k) * abi.mip_dim(hh, k) * 2 for k in range(abi.CACAO_DEPTH_MIPS))
    b = {"k_cacao_prepare_depths": 4 * p + mips, "k_cacao_prepare_normals": 4 * p + 16 * t, "k_cacao_generate": mips + 16 * t + 8 * t,
         "k_cacao_blur": 16 * t if blur else 0, "k_cacao_apply": 8 * t + p}
    return b


def frame(w, h):
    k = max(1, w // 960)
    f = synth.cacao_room(w // k, h // k)
    depth, packed = (np.repeat(np.repeat(f[key], k, 0), k, 1)[:h, :w] for key in ("depth", "packed"))
    sh, pp = cacao.constants(w, h, f["proj"], f["normals_to_view"])
    return np.ascontiguousarray(depth), np.ascontiguousarray(packed.view(np.int32)), sh, pp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=("time", "loop", "kernels"))
    ap.add_argument("--size", type=int, nargs=2, action="append")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blur", type=int, default=2)
    ap.add_argument("csv", nargs="?")
    a = ap.parse_args()
    sizes = [tuple(s) for s in a.size] if a.size else [(1920, 1080), (3840, 2160)]
    if a.mode == "kernels":
        rows = {}
        if a.csv.endswith(".db"):
            import sqlite3
            found = [(n, int(c), float(avg) * 1e3, None, None) for n, c, avg in sqlite3.connect(a.csv).execute("select name, total_calls, average from top_kernels")]   # average in us
        else:
            found = [(r["Name"], int(r["Calls"]), float(r["AverageNs"]), float(r["MinNs"]), float(r["MaxNs"])) for r in csv.DictReader(open(a.csv))]
        for name, calls, avg, lo, hi in found:
            for k in KERNELS:
                if k + "(" in name:
                    rows.setdefault(k, []).append((calls, avg, lo, hi))
        # one stats file holds the kernels of every size that ran: the caller profiles one size per run
        w, h = sizes[0]
        by = kernel_bytes(w, h, a.blur)
        out = {"bench": "cacao_kernels", "width": w, "height": h, "kernels": []}
        for k in KERNELS:
            for calls, avg, lo, hi in rows.get(k, []):
                out["kernels"].append({"kernel": k, "calls": calls, "avg_us": avg / 1e3, "min_us": lo and lo / 1e3, "max_us": hi and hi / 1e3, "bytes": by[k],
                                       "gb_per_s": by[k] / avg if avg else None})
        print(json.dumps(out))
        return
    import torch
    from benchlib.timing import _stage_stats
    from vqengine_amd import capi
    ctx = capi.Context(0)
    results = []
    for (w, h) in sizes:
        depth, packed, sh, pp = frame(w, h)
        d, n = torch.from_numpy(depth).cuda(), torch.from_numpy(packed).cuda()
        work = torch.empty((capi.cacao_work_bytes(w, h),), dtype=torch.uint8, device="cuda")
        out = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        call = lambda: ctx.cacao(d, n, abi.FMT_R10G10B10A2_UNORM, sh, pp, blur_passes=a.blur, work=work, out=out)
        if a.mode == "loop":
            for _ in range(a.steps):
                call()
            torch.cuda.synchronize()
            continue
        total = sum(kernel_bytes(w, h, a.blur).values())
        src, dst = torch.empty((total // 2,), dtype=torch.uint8, device="cuda"), torch.empty((total // 2,), dtype=torch.uint8, device="cuda")
        st = _stage_stats(call)
        cp = _stage_stats(lambda: dst.copy_(src))
        results.append({"width": w, "height": h, "blur_passes": a.blur, "call": st, "bytes_by_kernel": kernel_bytes(w, h, a.blur), "bytes_total": total,
                        "gb_per_s_of_the_call": total / (st["ms"] * 1e6), "copy_same_bytes": cp, "copy_gb_per_s": total / (cp["ms"] * 1e6),
                        "work_bytes": capi.cacao_work_bytes(w, h)})
    if a.mode == "time":
        print(json.dumps({"bench": "cacao", "device": torch.cuda.get_device_name(0), "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
