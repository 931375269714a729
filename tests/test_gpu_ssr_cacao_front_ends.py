"""What the shared host front ends of screen-space reflections and CACAO (capi.hip: ssrFrame, Plane, the overlap helpers, cacaoCall; capi.py: the _check_* helpers
and Context._cacao) could break: what a refusal says, and which of two refusals a call that is wrong twice gets. Every text is compared with
tests/golden/ssr_cacao_refusals.json, which scripts/record_ssr_cacao_refusals.py wrote from the library and the bindings as they were while each entry point had a
check ladder of its own. Three parts:
  * the six refusal tests of the SSR and CACAO modules, run as they stand on a listening context: every refusal they provoke, whole and in order;
  * for each of the eight entry points, calls with two faults on different rungs of its ladder: the code and the text, and the outputs keep their sentinel;
  * every distinct ValueError of the bindings ssr_intersect, ssr_prefilter, ssr_resolve_temporal, ssr_reproject, cacao and adaptive_cacao.
No frame here is larger than 40 x 24 beyond what the six refusal tests use themselves. All tensors come from a memory pool of their own (refusal_listener.
fresh_allocations): several of the refusal tests put an output on a smaller buffer, and which neighbour it then reaches first is a matter of where the tensors lie."""
import ctypes as C
import json
import os

import pytest
import torch

from tests import ref_cases
from tests import test_gpu_cacao as TC
from tests import test_gpu_cacao_adaptive as TA
from tests import test_gpu_ssr as TF
from tests import test_gpu_ssr_denoise as TD
from tests import test_gpu_ssr_reproject as TR
from tests import test_gpu_ssr_trace as TT
from tests.refusal_listener import Listening, fresh_allocations
from vqengine_amd import abi, cacao, capi, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssr_cacao_refusals.json")
W, H = 40, 24
H8, W8 = (H + 7) // 8, (W + 7) // 8
F16, F32, N10, R11, M16, U8 = abi.FMT_RGBA16F, abi.FMT_RGBA32F, abi.FMT_R10G10B10A2_UNORM, abi.FMT_R11G11B10_FLOAT, abi.FMT_RG16F, abi.FMT_RGBA8_UNORM
SENTINEL = -7.0
INV, UNS = abi.VQHIP_ERR_INVALID_ARG, abi.VQHIP_ERR_UNSUPPORTED


def make_small():
    e = ref_cases.small_env()
    keep = []
    return {"e": e, "henv": ref_cases.host_env(e), "denv": ref_cases.dev_env(e, keep), "keep": keep}


@pytest.fixture(scope="module")
def small():
    return make_small()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def said(entry, rc, text):
    return f"{entry} -> {rc}: {text}"


# ---- 1. the refusal tests as they stand --------------------------------------------------------------------------------------------------------------------------------
LISTENED = {"ssr_environment_fallback": lambda c, small: TF.test_argument_checks(c), "ssr_trace": TT.test_argument_refusals,
            "ssr_denoise": lambda c, small: TD.test_argument_refusals(c), "ssr_reproject": lambda c, small: TR.test_argument_refusals(c),
            "cacao": lambda c, small: TC.test_refusals_launch_nothing(c), "adaptive_cacao": lambda c, small: TA.test_refusals_launch_nothing(c)}


def listen(ctx, small, which):
    """-> every refusal of that test, in order, as text"""
    refused = []
    with fresh_allocations():
        LISTENED[which](Listening(ctx, [], refused), small)
    return [said(*r) for r in refused]


@pytest.mark.parametrize("which", sorted(LISTENED))
def test_refusal_tests_hear_what_they_heard(ctx, small, golden, which):
    got, want = listen(ctx, small, which), golden["library"][which]
    assert len(got) == len(want) and len(got) >= 8, f"{which}: the refusal test provoked {len(got)} refusals, {len(want)} are recorded"
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{which}: refusal {k} of the test's cases"


# ---- 2. calls that are wrong twice --------------------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return t.data_ptr() if t is not None else None


def _cb(small, dims=None, **fields):
    cb = synth.ssr_constants(W, H, small["e"]["spec_mips"])
    if dims:
        cb.bufferDimensions[0], cb.bufferDimensions[1] = dims
    for k, v in fields.items():
        setattr(cb, k, v)
    return cb


def _planes():
    """device tensors of the shapes the SSR entry points take at W x H; outputs hold the sentinel (a refused call reads and writes nothing)"""
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")                                      # noqa: E731
    s = lambda shape, dtype=torch.float16: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")               # noqa: E731
    return dict(scene=z((H, W, 4), torch.float16), depth=z((H, W), torch.float32), normals=z((H, W), torch.int32), r8=z((H, W), torch.uint8),
                noise=z((128, 128, 2), torch.uint8), rays=z((H * W,), torch.int32), counters=z((2,), torch.int32), tiles=z((H8 * W8,), torch.int32),
                levels=z((2 * H * W,), torch.float32), avg=z((H8, W8), torch.int32), rad=z((H, W, 4), torch.float16), rep=z((H, W, 4), torch.float16),
                var=z((H, W), torch.float16), cnt16=z((H, W), torch.float16), depth_hist=z((H, W), torch.float32), normals_hist=z((H, W), torch.int32),
                r8_hist=z((H, W), torch.uint8), rad_hist=z((H, W, 4), torch.float16), motion=z((H, W, 2), torch.float16), var_hist=z((H, W), torch.float16),
                cnt_hist=z((H, W), torch.float16), o_r=s((H, W, 4)), o_v=s((H, W)), o_c=s((H, W)), o_a=torch.full((H8, W8), 7, dtype=torch.int32, device="cuda"))


def _ssr_calls(ctx, small, t):
    """-> {entry point: (call(**overrides), [(case, overrides)])}; every case names two faults, the one on the earlier rung first"""
    lib, hnd, env, noenv = ctx.lib, ctx._h, small["denv"], abi.EnvMap(None, 0, None, 0, 0, None, 0)

    def fallback(scene=t["scene"], sfmt=F16, nfmt=N10, ofmt=F16, cb=_cb(small), env=env, pitch=0):
        return lib.vqhip_ssr_environment_fallback(hnd, None, _p(scene), sfmt, pitch, _p(t["depth"]), 0, _p(t["normals"]), nfmt, 0, W, H, cb, env, _p(t["o_r"]), ofmt, 0, None)

    def classify(fmt=F16, pitch=0, cb=_cb(small), rays=t["rays"]):
        return lib.vqhip_ssr_classify(hnd, None, _p(t["scene"]), fmt, pitch, _p(t["depth"]), 0, None, 0, cb, _p(rays), _p(t["counters"]), _p(t["tiles"]))

    def intersect(cb=_cb(small), lfmt=F16, nfmt=N10, ofmt=F16, pitch=0, env=env, out=t["o_r"], noise=t["noise"]):
        return lib.vqhip_ssr_intersect(hnd, None, _p(t["rays"]), _p(t["counters"]), _p(t["scene"]), lfmt, pitch, _p(t["levels"]), _p(t["normals"]), nfmt, 0, _p(t["r8"]),
                                       _p(noise), cb, env, _p(out), ofmt, 0)

    def prefilter(depth=t["depth"], nfmt=N10, afmt=R11, rfmt=F16, rpitch=0, cb=_cb(small), out=t["o_r"], ofmt=F16, ovar=t["o_v"]):
        return lib.vqhip_ssr_prefilter(hnd, None, _p(t["tiles"]), _p(t["counters"]), _p(depth), 0, _p(t["normals"]), nfmt, 0, _p(t["r8"]), _p(t["avg"]), afmt, _p(t["rad"]), rfmt,
                                       rpitch, _p(t["var"]), 0, cb, _p(out), ofmt, 0, _p(ovar), 0)

    def resolve(r8=t["r8"], afmt=R11, pfmt=F16, spitch=0, cb=_cb(small), out=t["o_r"], ofmt=F16, ovar=t["o_v"]):
        return lib.vqhip_ssr_resolve_temporal(hnd, None, _p(t["tiles"]), _p(t["counters"]), _p(r8), _p(t["avg"]), afmt, _p(t["rad"]), F16, 0, _p(t["rep"]), pfmt, 0, _p(t["var"]), 0,
                                              _p(t["cnt16"]), spitch, cb, _p(out), ofmt, 0, _p(ovar), 0)

    surfaces = dict(tile_list=t["tiles"], counters=t["counters"], depth=t["depth"], normals=t["normals"], roughness=t["r8"], depth_history=t["depth_hist"],
                    normal_history=t["normals_hist"], roughness_history=t["r8_hist"], radiance=t["rad"], radiance_history=t["rad_hist"], motion_vectors=t["motion"],
                    variance_history=t["var_hist"], sample_count_history=t["cnt_hist"], out_reprojected=t["o_r"], out_average=t["o_a"], out_variance=t["o_v"],
                    out_sample_count=t["o_c"])
    fmts = dict(normals_fmt=N10, normal_history_fmt=N10, radiance_fmt=F16, radiance_history_fmt=F16, motion_fmt=M16, out_reprojected_fmt=F16, out_average_fmt=R11)

    def reproject(cb=_cb(small), **over):
        s = abi.SSRReprojectSurfaces()
        for k, v in surfaces.items():
            v = over.get(k, v)
            setattr(s, k, _p(v))
        for k, v in fmts.items():
            setattr(s, k, over.get(k, v))
        for k, v in over.items():
            if k.endswith("_pitch_px"):
                setattr(s, k, v)
        return lib.vqhip_ssr_reproject(hnd, None, s, cb)

    return {
        "vqhip_ssr_environment_fallback": (fallback, [
            ("NULL scene, RGBA8 scene", dict(scene=None, sfmt=U8)), ("R10G10B10A2 radiance, RGBA16F normals", dict(ofmt=N10, nfmt=F16)),
            ("RGBA16F normals, no env", dict(nfmt=F16, env=noenv)), ("no env, short pitch", dict(env=noenv, pitch=W - 1)),
            ("mip count above the cube's, short pitch", dict(cb=_cb(small, envMapSpecularIrradianceCubemapMipLevelCount=small["e"]["spec_mips"] + 1), pitch=W - 1))]),
        "vqhip_ssr_classify": (classify, [
            ("NULL ray list, zero width", dict(rays=None, cb=_cb(small, dims=(0, H)))), ("zero width, height above 4096", dict(cb=_cb(small, dims=(0, 4097)))),
            ("width above 4096, RGBA8 scene", dict(cb=_cb(small, dims=(4097, H)), fmt=U8)), ("RGBA8 scene, short pitch", dict(fmt=U8, pitch=W - 1))]),
        "vqhip_ssr_intersect": (intersect, [
            ("NULL blue noise, RGBA8 lit scene", dict(noise=None, lfmt=U8)), ("width above 4096, RGBA8 lit scene", dict(cb=_cb(small, dims=(4097, H)), lfmt=U8)),
            ("R10G10B10A2 radiance, RGBA16F normals", dict(ofmt=N10, nfmt=F16)), ("RGBA16F normals, 257 intersections", dict(nfmt=F16, cb=_cb(small, maxTraversalIntersections=257))),
            ("mostDetailedMip 6, no env", dict(cb=_cb(small, mostDetailedMip=6), env=noenv)), ("short pitch, radiance on the lit scene", dict(pitch=W - 1, out=t["scene"]))]),
        "vqhip_ssr_prefilter": (prefilter, [
            ("NULL depth, RGBA16F normals", dict(depth=None, nfmt=F16)), ("RGBA16F normals, zero width", dict(nfmt=F16, cb=_cb(small, dims=(0, H)))),
            ("height above 4096, RGBA8 radiance", dict(cb=_cb(small, dims=(W, 4097)), rfmt=U8)), ("RGBA16F average, short radiance pitch", dict(afmt=F16, rpitch=W - 1)),
            ("short radiance pitch, output on the radiance", dict(rpitch=W - 1, out=t["rad"])), ("both outputs on the radiance", dict(out=t["rad"], ovar=t["rad"]))]),
        "vqhip_ssr_resolve_temporal": (resolve, [
            ("NULL roughness, R11G11B10 reprojected", dict(r8=None, pfmt=R11)), ("R11G11B10 reprojected, width above 4096", dict(pfmt=R11, cb=_cb(small, dims=(4097, H)))),
            ("R10G10B10A2 output, RGBA16F average", dict(ofmt=N10, afmt=F16)), ("short sample-count pitch, output on the reprojected radiance", dict(spitch=W - 1, out=t["rep"])),
            ("output on the reprojected radiance, variance on the sample count", dict(out=t["rep"], ovar=t["cnt16"]))]),
        "vqhip_ssr_reproject": (reproject, [
            ("NULL depth, zero width", dict(depth=None, cb=_cb(small, dims=(0, H)))), ("width above 4096, RGBA16F normals", dict(cb=_cb(small, dims=(4097, H)), normals_fmt=F16)),
            ("R11G11B10 normal history, RGBA8 radiance", dict(normal_history_fmt=R11, radiance_fmt=U8)), ("RGBA16F motion, RGBA16F average", dict(motion_fmt=F16, out_average_fmt=F16)),
            ("RGBA16F average, short depth pitch", dict(out_average_fmt=F16, depth_pitch_px=W - 1)),
            ("short variance-output pitch, short motion pitch", dict(out_variance_pitch_px=W - 1, motion_pitch_px=W - 1)),
            ("short sample-count-output pitch, variance on the sample count", dict(out_sample_count_pitch_px=W - 1, out_variance=t["o_c"])),
            ("variance on the sample count, reprojected on the radiance", dict(out_variance=t["o_c"], out_reprojected=t["rad"])),
            ("reprojected on the radiance history, variance on the variance history", dict(out_reprojected=t["rad_hist"], out_variance=t["var_hist"]))]),
    }


def _cacao_calls(ctx):
    w, h = 37, 23
    f = TC.inputs("room", w, h)
    sh, pp = TC.consts("room", w, h)
    sha, ppa = TA.consts("room", w, h)
    sh64, pp64 = TC.consts("room", 64, 48)
    bad_map = cacao.constants(w, h, f["proj"], f["normals_to_view"], cacao.settings())
    bad_map[0].ImportanceMapDimensions[0] += 1.0
    d, n = torch.zeros((h, w), dtype=torch.float32, device="cuda"), torch.zeros((h, w), dtype=torch.int32, device="cuda")
    work = torch.full((capi.adaptive_cacao_work_bytes(w, h),), 0x3C, dtype=torch.uint8, device="cuda")
    ao = torch.full((h, w), 0x5A, dtype=torch.uint8, device="cuda")
    lib, hnd, st = ctx.lib, ctx._h, ctx._stream()
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)                                              # noqa: E731

    def high(depth=d, dpitch=w * 4, fmt=N10, shared=sh, per_pass=pp, quality=abi.CACAO_QUALITY_HIGH, blur=2, wbytes=capi.cacao_work_bytes(w, h), width=w):
        return lib.vqhip_cacao(hnd, st, p(depth), dpitch, p(n), fmt, w * 4, C.byref(shared), per_pass, quality, blur, p(work), wbytes, p(ao), w, width, h)

    def highest(depth=d, dpitch=w * 4, fmt=N10, shared=sha, per_pass=ppa, blur=2, wbytes=work.numel(), out=ao, width=w):
        return lib.vqhip_adaptive_cacao(hnd, st, p(depth), dpitch, p(n), fmt, w * 4, C.byref(shared), per_pass, blur, p(work), wbytes, p(out), w, width, h)
    calls = {
        "vqhip_cacao": (high, [
            ("NULL depth, zero width", dict(depth=None, width=0)), ("width above 16384, qualityLevel 99", dict(width=abi.CACAO_MAX_DIM + 1, quality=99)),
            ("quality HIGHEST, RGBA16F normals", dict(quality=abi.CACAO_QUALITY_HIGHEST, fmt=F16)), ("quality MEDIUM, blurPassCount 9", dict(quality=abi.CACAO_QUALITY_MEDIUM, blur=9)),
            ("blurPassCount 9, short depth pitch", dict(blur=9, dpitch=w * 4 - 4)), ("workBytes one short, constants of another frame", dict(wbytes=capi.cacao_work_bytes(w, h) - 1, shared=sh64, per_pass=pp64))]),
        "vqhip_adaptive_cacao": (highest, [
            ("NULL depth, zero width", dict(depth=None, width=0)), ("width above 16384, RGBA16F normals", dict(width=abi.CACAO_MAX_DIM + 1, fmt=F16)),
            ("RGBA16F normals, blurPassCount -1", dict(fmt=F16, blur=-1)), ("blurPassCount 9, short depth pitch", dict(blur=9, dpitch=w * 4 - 4)),
            ("HIGH's workBytes, importance map of another size", dict(wbytes=capi.cacao_work_bytes(w, h), shared=bad_map[0])),
            ("importance map of another size, ao on the work buffer", dict(shared=bad_map[0], out=work))]),
    }
    return calls, lambda: bool((ao == 0x5A).all() and (work == 0x3C).all())


def wrong_twice(ctx, small):
    """-> {"<entry point>: <case>": what the library said}; asserts that every call was refused and that no output was touched"""
    out = {}
    with fresh_allocations():
        t = _planes()
        cacao_calls, cacao_untouched = _cacao_calls(ctx)
        for entry, (call, cases) in {**_ssr_calls(ctx, small, t), **cacao_calls}.items():
            assert 3 <= len(cases)
            for case, over in cases:
                rc = call(**over)
                assert rc in (INV, UNS), f"{entry}: {case}: status {rc}"
                out[f"{entry}: {case}"] = said(entry, rc, (ctx.lib.vqhip_last_error(ctx._h) or b"").decode())
        torch.cuda.synchronize()
        assert all(bool((t[k] == SENTINEL).all()) for k in ("o_r", "o_v", "o_c")) and bool((t["o_a"] == 7).all()) and cacao_untouched(), "a refused call wrote to an output"
    return out


def test_calls_wrong_twice_get_the_refusal_they_got(ctx, small, golden):
    got, want = wrong_twice(ctx, small), golden["wrong_twice"]
    assert sorted(got) == sorted(want)
    for case in got:
        assert got[case] == want[case], case


# ---- 3. the bindings' own refusals ----------------------------------------------------------------------------------------------------------------------------------------
def _variants(t):
    """the three ways a tensor of the right size can be wrong"""
    doubled = t.repeat_interleave(2, dim=-1)
    return {"dtype": t.to(torch.float64), "shape": t[:-1], "strides": doubled[..., ::2]}


def python_refusals(ctx, small):
    """-> {"<binding>: <argument> <what is wrong with it>": the ValueError's text}. `ctx` is a capi.Context or one of an earlier capi.py"""
    out = {}
    with fresh_allocations():
        t = _planes()
        cb, env = _cb(small), small["denv"]
        levels = ctx.depth_hierarchy(t["depth"])
        sh, pp = TC.consts("room", W, H)
        bindings = {
            "ssr_intersect": (ctx.ssr_intersect, dict(ray_list=t["rays"], counters=t["counters"], lit_scene=t["scene"], lit_fmt=F16, hierarchy=levels, normals=t["normals"], normal_fmt=N10,
                                                      roughness8=t["r8"], blue_noise=t["noise"], cb=cb, env=env, radiance=t["rad"], radiance_fmt=F16)),
            "ssr_prefilter": (ctx.ssr_prefilter, dict(tile_list=t["tiles"], counters=t["counters"], depth=t["depth"], normals=t["normals"], normal_fmt=N10, roughness8=t["r8"], average=t["avg"],
                                                      avg_fmt=R11, radiance=t["rad"], radiance_fmt=F16, variance=t["var"], cb=cb, out=t["o_r"], out_variance=t["o_v"])),
            "ssr_resolve_temporal": (ctx.ssr_resolve_temporal, dict(tile_list=t["tiles"], counters=t["counters"], roughness8=t["r8"], average=t["avg"], avg_fmt=R11, radiance=t["rad"],
                                                                    radiance_fmt=F16, reprojected=t["rep"], reprojected_fmt=F16, variance=t["var"], sample_count=t["cnt16"], cb=cb,
                                                                    out=t["o_r"], out_variance=t["o_v"])),
            "ssr_reproject": (ctx.ssr_reproject, dict(tile_list=t["tiles"], counters=t["counters"], depth=t["depth"], normals=t["normals"], normal_fmt=N10, roughness8=t["r8"],
                                                      depth_history=t["depth_hist"], normal_history=t["normals_hist"], normal_history_fmt=N10, roughness8_history=t["r8_hist"],
                                                      radiance=t["rad"], radiance_fmt=F16, radiance_history=t["rad_hist"], radiance_history_fmt=F16, motion=t["motion"], motion_fmt=M16,
                                                      variance_history=t["var_hist"], sample_count_history=t["cnt_hist"], cb=cb, out_reprojected=t["o_r"], out_average=t["o_a"],
                                                      out_variance=t["o_v"], out_sample_count=t["o_c"])),
            "cacao": (ctx.cacao, dict(depth=t["depth"], normals=t["normals"], normal_fmt=N10, shared=sh, per_pass=pp, work=torch.zeros((capi.cacao_work_bytes(W, H),), dtype=torch.uint8, device="cuda"),
                                      out=torch.zeros((H, W), dtype=torch.uint8, device="cuda"))),
        }
        bindings["adaptive_cacao"] = (ctx.adaptive_cacao, dict(bindings["cacao"][1], work=torch.zeros((capi.adaptive_cacao_work_bytes(W, H),), dtype=torch.uint8, device="cuda")))
        # argument -> the ways it is made wrong: all three where the argument stands for one of the helpers, the dtype alone where the same helper has been through all three
        all3, one = ("dtype", "shape", "strides"), ("dtype",)
        wrong = {
            "ssr_intersect": dict(normals=all3, roughness8=all3, blue_noise=one, ray_list=all3, counters=all3, lit_scene=one, radiance=one),
            "ssr_prefilter": dict(depth=all3, normals=one, tile_list=all3, counters=one, roughness8=one, average=all3, radiance=one, variance=all3, out=one, out_variance=all3),
            "ssr_resolve_temporal": dict(tile_list=one, counters=one, roughness8=one, average=one, reprojected=one, variance=one, sample_count=all3, out_variance=one),
            "ssr_reproject": dict(tile_list=all3, counters=one, depth=all3, depth_history=one, roughness8=all3, roughness8_history=one, variance_history=all3, sample_count_history=one,
                                  normals=all3, normal_history=one, radiance=one, radiance_history=one, motion=one, out_reprojected=one, out_average=all3, out_variance=all3,
                                  out_sample_count=one),
            "cacao": dict(depth=all3, normals=all3, work=("dtype", "strides"), out=all3),
            "adaptive_cacao": dict(depth=all3, normals=all3, work=("dtype", "strides"), out=all3),
        }
        for name, (call, good) in bindings.items():
            for arg, ways in wrong[name].items():
                for way in ways:
                    with pytest.raises(ValueError) as e:
                        call(**dict(good, **{arg: _variants(good[arg])[way]}))
                    out[f"{name}: {arg} with the wrong {way}"] = str(e.value)
        for name, over in (("ssr_intersect", dict(cb=_cb(small, dims=(W + 1, H)))), ("ssr_intersect", dict(hierarchy=t["depth"])), ("ssr_reproject", dict(motion_fmt=F16)),
                           ("ssr_intersect", dict(normals=t["scene"], normal_fmt=F32)), ("ssr_prefilter", dict(normals=t["scene"], normal_fmt=F32)),
                           ("ssr_prefilter", dict(average=t["scene"], avg_fmt=F32)), ("ssr_reproject", dict(normal_history=t["scene"], normal_history_fmt=F32)),
                           ("ssr_reproject", dict(out_average=t["scene"], avg_fmt=F32)), ("cacao", dict(normals=t["scene"], normal_fmt=F32)),
                           ("adaptive_cacao", dict(normals=t["scene"], normal_fmt=F32))):
            call, good = bindings[name]
            with pytest.raises(ValueError) as e:
                call(**dict(good, **over))
            out[f"{name}: {', '.join(sorted(over))} that do not fit"] = str(e.value)
        torch.cuda.synchronize()
        assert all(bool((t[k] == SENTINEL).all()) for k in ("o_r", "o_v", "o_c")) and bool((t["o_a"] == 7).all()), "a refused call wrote to an output"
    return out


def test_bindings_raise_what_they_raised(ctx, small, golden):
    got, want = python_refusals(ctx, small), golden["python"]
    assert sorted(got) == sorted(want)
    for case in got:
        assert got[case] == want[case], case
