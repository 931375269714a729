"""vqhip_cacao (docs/DESIGN_DETAILS.md §7.14) or, with --quality highest, vqhip_adaptive_cacao (§7.15) at 1920 x 1080 and 3840 x 2160 (--size W H for another): one
JSON line. Needs the GPU. The frame is synth.cacao_room ray-cast at 960 x 540 and enlarged by texel replication (the ray cast of eight million pixels would dominate
the run); default settings at the chosen quality, blurPassCount 2, R10G10B10A2_UNORM normals. --quality both times the two calls next to each other on one card.
  (default)        the whole call — five kernels on torch's current stream — timed by benchlib.timing._stage_stats (spin-up by time, seven batches between device
                   events, the median batch), next to a device-to-device copy of the call's total traffic as the bandwidth yardstick.
  --mode loop      N calls and a synchronise: the workload of a `rocprofv3 --kernel-trace --stats` run of its own (kernel times come from there, not from events).
  --mode kernels   FILE reads the kernel summary of such a run (its rocpd database *.db, or a kernel_stats.csv) and prints, per kernel, the average time next to the bytes the kernel must move (from the shapes,
                   every plane counted once per kernel) and the HBM rate that implies.
  --mode taps      (no GPU) the tap-count histogram of the HIGHEST frame from tests/cacao_adaptive_ref.py, and the taps a wave executes (its longest lane) against
                   the taps its lanes need (their mean).
Bytes, with P = W * H pixels and T = hw * hh texels per slice: prepare depths reads 4 P and writes the four R16F mips of four slices; prepare normals reads 4 P
and writes 16 T; generate reads the depth mips and the normals and writes 8 T; the blur reads 8 T and writes 8 T; apply reads 8 T and writes P. HIGHEST, with M = iw * ih map texels: the base pass reads the mips and 16 T and writes 8 T; the
importance kernel reads 8 T and writes M; A and B read M and write M; the adaptive generate reads the mips, 16 T, the base values 8 T and M, and writes 8 T."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqengine_amd import abi, cacao, synth   # noqa: E402

KERNELS = ("k_cacao_prepare_depths", "k_cacao_prepare_normals", "k_cacao_generate", "k_cacao_blur", "k_cacao_apply")
ADAPTIVE_KERNELS = ("k_cacao_prepare_depths", "k_cacao_prepare_normals", "k_cacao_generate_base", "k_cacao_importance", "k_cacao_importance_a", "k_cacao_importance_b",
                    "k_cacao_generate_adaptive", "k_cacao_blur", "k_cacao_apply")


def kernel_bytes(w, h, blur=2, quality="high"):
    hw, hh = abi.cacao_half_dims(w, h)
    p, t = w * h, hw * hh
    mips = sum(4 * abi.mip_dim(hw, k) * abi.mip_dim(hh, k) * 2 for k in range(abi.CACAO_DEPTH_MIPS))
    b = {"k_cacao_prepare_depths": 4 * p + mips, "k_cacao_prepare_normals": 4 * p + 16 * t, "k_cacao_generate": mips + 16 * t + 8 * t,
         "k_cacao_blur": 16 * t if blur else 0, "k_cacao_apply": 8 * t + p}
    if quality == "highest":
        iw, ih = abi.cacao_half_dims(hw, hh)
        m = iw * ih
        del b["k_cacao_generate"]
        b.update({"k_cacao_generate_base": mips + 16 * t + 8 * t, "k_cacao_importance": 8 * t + m, "k_cacao_importance_a": 2 * m, "k_cacao_importance_b": 2 * m,
                  "k_cacao_generate_adaptive": mips + 16 * t + 8 * t + m + 8 * t})
    return b


def frame(w, h, quality="high"):
    k = max(1, w // 960)
    f = synth.cacao_room(w // k, h // k)
    depth, packed = (np.repeat(np.repeat(f[key], k, 0), k, 1)[:h, :w] for key in ("depth", "packed"))
    s = cacao.settings() if quality == "highest" else None                       # FFX_CACAO_DEFAULT_SETTINGS are HIGHEST; None: the same at HIGH
    sh, pp = cacao.constants(w, h, f["proj"], f["normals_to_view"], s)
    return np.ascontiguousarray(depth), np.ascontiguousarray(packed.view(np.int32)), sh, pp


def tap_statistics(w, h, blur):
    """the HIGHEST frame of the timed size through the numpy statement: what the adaptive loop has to do, without a GPU"""
    from tests import cacao_adaptive_ref as A
    depth, packed, sh, pp = frame(w, h, "highest")
    st = A.frame(depth, packed.view(np.uint32), abi.FMT_R10G10B10A2_UNORM, sh, pp, blur)["stats"]
    hist = st["tap_histogram"]
    return {"width": w, "height": h, "tap_histogram": {str(i): int(n) for i, n in enumerate(hist) if n}, "mean_taps": float((hist * np.arange(len(hist))).sum() / hist.sum()),
            "counter": st["counter"], "limiter": st["limiter"], "wave_max_mean": st["wave_max_mean"], "wave_mean_mean": st["wave_mean_mean"],
            "waves": int(len(st["wave_max"])), "waves_with_differing_lanes": int((st["wave_max"] > st["wave_mean"]).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=("time", "loop", "kernels", "taps"))
    ap.add_argument("--quality", default="high", choices=("high", "highest", "both"))
    ap.add_argument("--size", type=int, nargs=2, action="append")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blur", type=int, default=2)
    ap.add_argument("csv", nargs="?")
    a = ap.parse_args()
    sizes = [tuple(s) for s in a.size] if a.size else [(1920, 1080), (3840, 2160)]
    if a.mode == "taps":
        print(json.dumps({"bench": "cacao_taps", "results": [tap_statistics(w, h, a.blur) for (w, h) in sizes]}))
        return
    if a.mode == "kernels":
        names = ADAPTIVE_KERNELS if a.quality == "highest" else KERNELS
        rows = {}
        if a.csv.endswith(".db"):
            import sqlite3
            found = [(n, int(c), float(avg) * 1e3, None, None) for n, c, avg in sqlite3.connect(a.csv).execute("select name, total_calls, average from top_kernels")]   # average in us
        else:
            found = [(r["Name"], int(r["Calls"]), float(r["AverageNs"]), float(r["MinNs"]), float(r["MaxNs"])) for r in csv.DictReader(open(a.csv))]
        for name, calls, avg, lo, hi in found:
            for k in names:
                if k + "(" in name:
                    rows.setdefault(k, []).append((calls, avg, lo, hi))
        # one stats file holds the kernels of every size that ran: the caller profiles one size per run
        w, h = sizes[0]
        by = kernel_bytes(w, h, a.blur, a.quality)
        out = {"bench": "cacao_kernels", "quality": a.quality, "width": w, "height": h, "kernels": []}
        for k in names:
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
    for (w, h), quality in ((s, q) for s in sizes for q in (("high", "highest") if a.quality == "both" else (a.quality,))):
        depth, packed, sh, pp = frame(w, h, quality)
        d, n = torch.from_numpy(depth).cuda(), torch.from_numpy(packed).cuda()
        work_bytes = capi.adaptive_cacao_work_bytes(w, h) if quality == "highest" else capi.cacao_work_bytes(w, h)
        work = torch.empty((work_bytes,), dtype=torch.uint8, device="cuda")
        out = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        if quality == "highest":
            call = lambda: ctx.adaptive_cacao(d, n, abi.FMT_R10G10B10A2_UNORM, sh, pp, blur_passes=a.blur, work=work, out=out)
        else:
            call = lambda: ctx.cacao(d, n, abi.FMT_R10G10B10A2_UNORM, sh, pp, blur_passes=a.blur, work=work, out=out)
        if a.mode == "loop":
            for _ in range(a.steps):
                call()
            torch.cuda.synchronize()
            continue
        by = kernel_bytes(w, h, a.blur, quality)
        total = sum(by.values())
        src, dst = torch.empty((total // 2,), dtype=torch.uint8, device="cuda"), torch.empty((total // 2,), dtype=torch.uint8, device="cuda")
        st = _stage_stats(call)
        cp = _stage_stats(lambda: dst.copy_(src))
        results.append({"width": w, "height": h, "quality": quality, "blur_passes": a.blur, "call": st, "bytes_by_kernel": by, "bytes_total": total,
                        "gb_per_s_of_the_call": total / (st["ms"] * 1e6), "copy_same_bytes": cp, "copy_gb_per_s": total / (cp["ms"] * 1e6),
                        "work_bytes": work_bytes})
    if a.mode == "time":
        print(json.dumps({"bench": "cacao", "device": torch.cuda.get_device_name(0), "results": results}))
    ctx.close()


if __name__ == "__main__":
    main()
