"""bench.py's N > 1 control flow on REAL kernels, on a one-GPU box: the ranks share the GPU (VQ_BENCH_SHARE_GPU=1: control plane over gloo,
the C ABI's RCCL calls served by tests/cpp/libmock_rccl.so through shared memory) and rank 0 recomputes the whole frame untiled and compares
it byte for byte with the composite (VQ_BENCH_VERIFY=1). RCCL itself is not exercised here (one GPU); everything the product adds around it
is: vqhip_rowtile, the halo exchange and the composite through the C ABI, the second stream / second communicator, the double buffering
and the drain — for the weak-scaling cfg3 frame and for the strong-scaling cfg5 frame (7680x4320, 256 lights, uneven 1440-row tiles)."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(ranks, extra_args, **more_env):
    env = dict(os.environ, VQ_BENCH_SHARE_GPU="1", VQ_BENCH_VERIFY="1", VQ_BENCH_SPINUP="4", VQ_BENCH_SUSTAINED_S="0.05", MASTER_ADDR="127.0.0.1")
    env.update(more_env)
    # a fault is injected by running bench.main() with a Pipeline subclass (tests/bench_fault_harness.py): nothing of it lives in bench.py
    script = os.path.join(ROOT, "tests", "bench_fault_harness.py") if "VQ_TEST_FAULT" in more_env else os.path.join(ROOT, "bench.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), script, "--gpus", str(ranks), "--steps", "4", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--no-second-mode"] + extra_args
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def _check_rccl(d, ranks, mode):
    r = d["rccl"]                                            # read back from the communicator (vqhip_comm_query), the stand-in reports version 0
    assert r["nranks_seen"] == ranks and r["rank_seen"] == 0 and r["version"] == 0 and r["library_path"].endswith("libmock_rccl.so"), r
    assert r["composite_overlap_mode"] == mode, r


@pytest.mark.parametrize("ranks,composite,overlap,mode", [(2, "root", "auto", "one-comm"), (2, "all", "off", "off"), (3, "root", "on", "one-comm"),
                                                          (2, "root", "two-comms", "two-comms")])
def test_cfg3_weak_scaling_flow_matches_the_untiled_frame(ranks, composite, overlap, mode):
    """3 ranks: the middle tile exchanges halos with both neighbours. Headline only (--no-extras)."""
    d = _run(ranks, ["--config", "cfg3", "--composite", composite, "--composite-overlap", overlap, "--no-extras"])
    assert d["n_gpus"] == ranks and d["scaling"] == "weak" and d["config"]["frame_height"] == 2160 * ranks
    assert d["verify"]["mismatching_bytes"] == 0, d["verify"]
    _check_rccl(d, ranks, mode)
    assert "cfg5_strong" not in d


@pytest.mark.parametrize("ranks,post", [(2, "chain"), (3, "chain"), (2, "fused"), (3, "fused"), (2, "split")])
def test_every_post_form_flow_matches_the_untiled_frame(ranks, post):
    """bench.py --post chain (the default): every rank runs blur X + blur Y + tonemap as ONE kernel over its tile (vqhip_post_process_tile) and the neighbours exchange 10
    rows of SCENE COLOUR right behind the shade kernel; --post fused / split: blur X, exchange of X-blurred rows, blur Y (+ tonemap). In every form the composited frame
    equals the untiled frame of the two-kernel chain byte for byte (3 ranks: the middle tile has two halos)."""
    d = _run(ranks, ["--config", "cfg3", "--post", post, "--no-extras"])
    assert d["n_gpus"] == ranks and d["verify"]["mismatching_bytes"] == 0, d["verify"]
    if post == "chain":
        assert "ONE kernel" in d["config"]["post"] and d["stages"]["post_chain_bytes_per_px"] == 12
    else:
        assert "ONE kernel" not in d["config"]["post"]


def test_every_run_also_times_cfg5_strong_scaling():
    """The --full invocation at N = 3: the cfg3 headline (weak) AND the cfg5 strong-scaling object the >= 6x target is defined on
    (one 7680x4320 frame, 256 lights, 1440 rows per rank), with its stage figures and the communicator's own report."""
    d = _run(3, [])
    assert d["config"]["name"] == "cfg3" and d["scaling"] == "weak" and d["verify"]["mismatching_bytes"] == 0
    c = d["cfg5_strong"]
    assert c["frame"] == [7680, 4320] and c["tile_rows"] == 1440 and c["lights"] == 256 and c["scaling"] == "strong"
    for k in ("value", "ms_per_step", "shade_ms", "halo_ms", "composite_ms", "frame_latency_ms", "post_chain_ms"):
        assert c[k] > 0, (k, c)
    assert abs(c["value"] - 7680 * 4320 / (c["ms_per_step"] * 1e-3) / 1e6) < 0.01 * c["value"]
    assert c["composite_overlapped"] is True
    _check_rccl(d, 3, "one-comm")
    for k in ("cfg2", "ibl_load", "coherent_scene", "tile_curve", "widened"):      # single-GPU objects
        assert k not in d


def test_cfg5_strong_scaling_flow_matches_the_untiled_frame():
    d = _run(3, ["--config", "cfg5", "--no-extras"])
    assert d["n_gpus"] == 3 and d["scaling"] == "strong" and d["config"]["frame_height"] == 4320 and d["config"]["tile_rows"] == 1440
    assert d["config"]["lights"] == 256 and d["verify"]["mismatching_bytes"] == 0, d["verify"]


def test_overlap_watchdog_falls_back_to_one_stream_order():
    """--composite-overlap auto: when the first overlapped steps do not complete in time (forced here), every rank aborts its communicator,
    builds a new one and runs the composite in stream order; the frame is still the untiled one."""
    d = _run(2, ["--config", "cfg3", "--no-extras"], VQ_TEST_FAULT="overlap_timeout")
    assert d["verify"]["mismatching_bytes"] == 0, d["verify"]
    assert d["config"]["composite_overlap"] is False and d["rccl"]["composite_overlap_mode"] == "off" and d["rccl"]["fallback"], d["rccl"]


def test_a_missing_stream_wait_corrupts_the_frame_under_the_asynchronous_transport():
    """The stand-in for RCCL is asynchronous like RCCL (tests/cpp/mock_rccl.cpp: the transfers of a group run on the communicator's worker thread behind an event of
    the caller's stream, later work on that stream waits on a signal word, ncclGroupEnd returns at once), so the orderings between the main stream and the composite's
    stream are real orderings, not only control flow. The verified step starts from zeroed output buffers on a drained device: leaving out the wait that puts the
    composite behind the post kernel (tests/bench_fault_harness.py, VQ_TEST_FAULT) must deliver a wrong frame. The synchronous form of the stand-in ($VQMOCK_RCCL_SYNC=1, rounds 1-4) still runs
    the unbroken flow to the right frame."""
    args = ["--config", "cfg3", "--composite-overlap", "two-comms", "--no-extras"]       # the composite's communicator has its own worker: it starts as soon as its stream lets it
    d = _run(2, args, VQMOCK_RCCL_SYNC="1")
    assert d["verify"]["mismatching_bytes"] == 0, d["verify"]
    worst = 0
    for attempt, spin in enumerate(("4", "12", "40")):        # a race can be lost: three attempts with different amounts of work queued in front of the verified step
        d = _run(2, args, VQ_TEST_FAULT="drop_post_wait", VQ_BENCH_SPINUP=spin)
        worst = max(worst, d["verify"]["mismatching_bytes"])
        if worst > 1000:
            break
    if worst == 0:                                            # lost three times: not a defect of the product — report it without failing the suite
        pytest.skip("the unordered composite ran after the post kernel in all three attempts on this box: the fault was not observable")
    assert worst > 1000, d["verify"]


def test_gpus_n_without_a_launcher_starts_its_own_ranks():
    """`python bench.py --gpus 2` — the shape of the driver's N = 1 command, no torchrun around it: bench.py starts the two ranks itself and rank 0
    prints one line with n_gpus 2. Without the share-one-GPU debug aid and with fewer GPUs than ranks it must refuse loudly."""
    import torch
    clean = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "VQ_BENCH_SHARE_GPU")}
    env = dict(clean, VQ_BENCH_SHARE_GPU="1", VQ_BENCH_VERIFY="1", VQ_BENCH_SPINUP="4")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--no-extras", "--no-cpu-baseline",
                        "--no-second-mode"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl"]["nranks_seen"] == 2 and d["config"]["frame_height"] == 4320 and d["verify"]["mismatching_bytes"] == 0
    if torch.cuda.device_count() < 2:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--no-extras"], cwd=ROOT, env=clean,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and "--gpus 2" in p.stderr and not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_single_gpu_line_carries_the_contract_fields():
    """`python bench.py --full` (N = 1, defaults shortened): one JSON line with the driver's contract fields, the roofline and cpu_baseline objects,
    counter constants that belong to the current kernel sources, and the self-audit extras (engine lowering, cold start, isolated post kernels)."""
    env = dict(os.environ, VQ_BENCH_SPINUP="30", VQ_BENCH_SUSTAINED_S="0.5", VQ_BENCH_VERIFY="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "6", "--warmup", "2", "--full"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, "bench.py must print exactly one line on stdout"
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "stages", "engine_lowering", "dxc_lowering", "cold_start", "frame_latency_ms", "valu_issue", "pmc_constants", "rccl",
              "cfg5_strong", "cfg2", "ibl_load", "coherent_scene", "tile_curve", "sustained", "widened", "other_post_form", "two_frames_in_flight", "cfg1", "engine_max",
              "notes", "digest"):
        assert k in d, k
    assert d["two_frames_in_flight"]["frames_in_flight"] == 2 and d["two_frames_in_flight"]["ms_per_step"] > 0
    assert d["verify"]["mismatching_bytes"] == 0 and d["verify"]["buffers"] == 2, d["verify"]      # the frame loop's two streams / two buffer pairs deliver the two-kernel chain's bytes
    assert d["config"]["post_stream"].startswith("own")
    oc = d["other_post_form"]                                # the headline runs the one-kernel chain; the companion is the two-kernel path
    assert oc["form"] == "fused" and oc["bytes_per_px"] == 28 and oc["ms_per_step"] > 0 and abs(oc["value"] - 3840 * 2160 / (oc["ms_per_step"] * 1e-3) / 1e6) < 0.01 * oc["value"]
    su = d["sustained"]                                      # ~0.5 s of the headline's step here (VQ_BENCH_SUSTAINED_S), same order as `value`
    assert su["steps"] >= 200 and su["steps"] % 2 == 0 and su["value"] > 0
    assert abs(su["value"] - 3840 * 2160 * su["steps"] / su["seconds"] / 1e6) < 0.01 * su["value"]
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["unit"] == "Mpix/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 3840 * 2160 / (d["ms_per_step"] * 1e-3) / 1e6) < 0.01 * d["value"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    assert isinstance(r["traffic"], int) and r["traffic"] > 597196800 // 2
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "Mpix/s" and c["sample"]
    assert "stale" in d["pmc_constants"]                     # that the constants belong to the current kernel sources is a CPU test: tests/test_bench_meta.py::test_pmc_constants_are_current
    assert d["engine_lowering"]["fresnel_pow"] == "exp2_log2" and d["engine_lowering"]["value"] > 0
    assert d["dxc_lowering"]["arithmetic"] == "dxc" and d["dxc_lowering"]["value"] > 0
    iso = d["stages"]["isolated"]
    assert iso["post_chain_ms"] > 0 and d["stages"]["post_chain_bytes_per_px"] == 12 and d["stages"]["shade_ms"] > 0
    # loose upper bounds (no inequality BETWEEN measured times — boxes differ — but a 10x regression of a stage must still fail): round-6 figures 0.95 / 0.048 / 0.075 / 0.071 / 2.5 ms
    assert d["stages"]["shade_ms"] < 9.5 and iso["post_chain_ms"] < 0.48 and d["cfg2"]["shade_ms"] < 0.75 and d["cfg1"]["shade_ms"] < 0.71 and d["engine_max"]["shade_ms"] < 25.0
    assert d["stages"]["post_chain_in_loop_ms"] > 0 and abs(d["stages"]["post_chain_alone_ms"] - iso["post_chain_ms"]) < 1e-6      # two timing bases, two keys
    # the spot-light + PCF caster path is timed in every run: BASELINE cfg1 with its own CPU baseline, and the cbuffer's limits at 4K
    c1, em = d["cfg1"], d["engine_max"]
    assert c1["lights"] == {"point": 0, "spot": 0, "point_casters": 0, "spot_casters": 2, "directional": 1, "directional_shadowing": 1} and c1["cpu_baseline"]["value"] > 0
    assert em["lights"]["point"] == 100 and em["lights"]["spot"] == 20 and em["lights"]["point_casters"] == 5 and em["lights"]["spot_casters"] == 5 and em["coherent_content"]["shade_ms"] > 0
    ed = d["ibl_load"]["engine_default"]                     # the engine's default IBL sizes
    assert ed["spec_mips"] == 9 and ed["source_mips"] == 13 and ed["conv_specular_ms"] > 0 and ed["prefilter_ms"] > ed["conv_specular_ms"]
    # the driver's record keeps `roofline` whole and the last ~2 000 characters of the line: the second-tier figures must sit there
    kernels = [o["kernel"] for o in r["others"]]
    assert any("k_post_chain" in k for k in kernels) and any("cfg2" in k for k in kernels) and any("k_conv_diffuse_ordered" in k for k in kernels) and any("cfg1" in k for k in kernels)
    pc = next(o for o in r["others"] if "k_post_chain" in o["kernel"])
    assert abs(pc["frac"] - pc["bytes"] / (pc["ms"] * 1e-3) / 8e12) < 0.02 * pc["frac"]
    assert r["valu"]["frac_spec"] > 0 and r["valu"]["frac_issue"] is not None
    assert list(d)[-1] == "digest" and list(d)[-4:-1] == ["valu_issue", "cfg5_strong", "stages"]
    tail = lines[0][-2000:]
    assert '"digest"' in tail and '"post_chain_alone_ms"' in tail and '"cfg2_hbm_frac"' in tail and '"cfg1_shade_ms"' in tail, "the digest must fit the last 2 000 characters of the line"
    assert not any(isinstance(v, str) and len(v) > 80 for v in d["stages"].values()), "the prose of `stages` belongs in `notes`"
    # the other BASELINE configs ride in the same line
    c5 = d["cfg5_strong"]
    assert c5["frame"] == [7680, 4320] and c5["tile_rows"] == 4320 and c5["lights"] == 256 and c5["shade_ms"] > 0 and c5["ms_per_step"] > 0 and c5["halo_ms"] == 0
    c2 = d["cfg2"]
    assert c2["shade_ms"] > 0 and abs(c2["hbm_frac"] - 72 * 1920 * 1080 / (c2["shade_ms"] * 1e-3) / 8e12) < 0.02 * c2["hbm_frac"] and c2["valu_frac_model"] > 0
    ib = d["ibl_load"]
    for k in ("mip_chain_ms", "prefilter_ms", "brdf_lut_ms", "conv_diffuse_ms", "conv_specular_ms", "brdf_lut_warm_ms", "total_ms", "warm_total_ms", "mip_chain_warm_ms", "prefilter_warm_ms", "conv_diffuse_valu_frac_model"):
        assert ib[k] > 0, k
    wd = d["widened"]                                        # the SURVEY 8f kernels at 4K
    for k in ("gbuffer_producer_textured", "gbuffer_producer_textureless", "psmain_fused", "skydome_all_sky", "fsr_easu_1440p_to_4k", "fsr_rcas_4k", "ssr_env_fallback_4k",
              "psmain_fused_mrt", "scene_normals_prepass"):
        assert wd[k]["ms"] > 0 and wd[k]["bytes_per_px"] > 0 and wd[k]["hbm_frac"] > 0, (k, wd[k])
        assert wd[k]["ms_min"] <= wd[k]["ms"] <= wd[k]["ms_max"] and wd[k]["batches"] >= 5, (k, wd[k])          # median of >= 5 batches, with its spread
    assert wd["hdr_decode_2048"]["ms"] > 0
    co = d["coherent_scene"]
    assert co["shade_ms"] > 0 and 0.05 < co["slow_path_pixel_fraction_round2"] < 0.3            # a property of the synthetic content, not a timing
    tc = d["tile_curve"]["tiles"]
    assert [t["tile_rows"] for t in tc] == [4320, 2160, 1080, 540] and all(t["step_ms"] > 0 for t in tc)
    assert tc[3]["modelled_speedup_serial_half_link"] <= tc[3]["modelled_speedup_overlapped_peak_link"] <= tc[3]["compute_speedup"]
    assert d["rccl"]["nranks_seen"] == 1


def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    """`python bench.py --steps K --warmup W --dump-outputs DIR` (no --full): the headline fields and nothing that takes runs of its own, and the last timed step's
    frame and scene colour as float32 .npy files (a seeded 2^20-pixel sample of the 4K tile) that two runs with the same arguments reproduce bit for bit."""
    import numpy as np
    env = dict(os.environ, VQ_BENCH_SPINUP="30")
    dumps = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--dump-outputs", str(out)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, "bench.py must print exactly one line on stdout"
        d = json.loads(lines[0])
        assert d["steps"] == 5 and d["warmup"] == 2 and d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and "4K,64 lights" in d["metric"]
        assert d["ms_per_step"] > 0 and abs(d["value"] - 3840 * 2160 / (d["ms_per_step"] * 1e-3) / 1e6) < 0.01 * d["value"]
        for k2 in ("cfg5_strong", "cfg2", "ibl_load", "widened", "cpu_baseline", "engine_lowering", "dxc_lowering", "cold_start", "sustained", "frame_latency_ms"):
            assert k2 not in d, k2
        files = sorted(os.listdir(out))
        assert files == ["frame_rgba8.npy", "scene_color_rgba16f.npy"], files
        arrs = {f: np.load(out / f) for f in files}
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        for a in arrs.values():
            assert a.dtype == np.float32 and a.shape == (1 << 20, 4)
        fr = arrs["frame_rgba8.npy"]
        assert np.isfinite(fr).all() and fr.min() >= 0 and fr.max() <= 255 and (fr == np.round(fr)).all() and fr[:, :3].std() > 1
        dumps.append(arrs)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f].view(np.uint32), dumps[1][f].view(np.uint32)), f
