"""CPU side of vqhip_scene_interpolants (docs/DESIGN_DETAILS.md §7.18): that the test set holds every class of pixel the contract distinguishes (from the
statement's own statistics); exactness where the contract promises it; I2's weights against §7.16 R6's (b_i / w_i) / sum form; an exact rational cross-check of
I2 / I3 whose figure §7.18 carries; and the boundary (struct layouts, symbols, the work-size helper, the refusal without a context, the host-side producers)."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import scene_interp_cases as IC
from tests import scene_interp_ref as I
from vqengine_amd import abi, capi
from vqengine_amd import shadow_scene as S
from vqengine_amd import surface_scene as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, F64, U32 = np.float32, np.float64, np.uint32
NEW_SYMBOLS = {"vqhip_scene_interpolants", "vqhip_scene_interpolants_work_bytes"}
CLASSES = ("no_owner", "behind", "outside", "later_instance", "later_draw")


def as_f32(bits):
    return np.ascontiguousarray(bits, dtype=U32).view(F)


# ---- (a) the set holds every class ------------------------------------------------------------------------------------------------------------------------------------
def test_the_test_set_holds_every_class_of_pixel():
    total = dict.fromkeys(CLASSES, 0)
    outside_in_layer, owned_in_layer = [0] * 4, [0] * 4
    for name, sc in IC.cases().items():
        for k, (_, st) in enumerate(IC.expected(name)):
            for c in CLASSES:
                total[c] += st[c]
            if sc["samples"] == 4:
                outside_in_layer[k] += st["outside"]
                owned_in_layer[k] += st["owned"]
    print("pixels per class over the set:", total, "owned per 4x layer:", owned_in_layer, "centre outside the owner per 4x layer:", outside_in_layer)
    for c in CLASSES:
        assert total[c] > 0, f"no pixel of class {c}"
    assert all(n > 0 for n in owned_in_layer), "a layer of the 4x cases owns nothing"       # pixels in the second, third and fourth layer
    assert sum(outside_in_layer) > 0                                                        # a 4x layer pixel whose centre lies outside its owner
    # the room's wall triangles cross w = 0, the boxes own pixels in instances > 0, the occluders are a second draw
    st = IC.expected("room_64x40_s1")[0][1]
    assert st["behind"] > 0 and st["later_draw"] > 0 and st["no_owner"] == 0
    assert IC.expected("boxes_64x40_s1")[0][1]["later_instance"] > 0 and IC.expected("sphere_16x16_s1")[0][1]["owned"] > 0


# ---- (b) exactness ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_attributes_constant_over_a_triangle_come_out_bit_exact():
    """the room's and the boxes' per-face normals and tangents are equal at the three vertices of every triangle: the stored value is the vertex stage's, bit for
    bit, at every owned pixel — pixels whose owner crosses w = 0 and 4x pixels that extrapolate included; materialIndex is stored as it is. The one exception
    I3's sum has is the sign of a zero: a0 + l1 (a1 - a0) with a0 = -0 is -0 + (+-0), which is +0 unless l1 is negative; §7.18 says so."""
    checked = 0
    for name in ("room_64x40_s1", "room_129x67_s4", "boxes_64x40_s4", "boxes_16x16_s1"):
        sc = IC.cases()[name]
        for owner, (out, _) in zip(IC.owners(name)[0], IC.expected(name)):
            has, attrs, mat, *_ = I.gather(sc, owner)
            flat = np.all(attrs[..., 0, 3:9].view(U32) == attrs[..., 1, 3:9].view(U32), axis=-1) & np.all(attrs[..., 0, 3:9].view(U32) == attrs[..., 2, 3:9].view(U32), axis=-1)
            assert flat[has].all(), "the case's faces are flat"
            for plane, lo in (("ip1", 3), ("ip2", 6)):
                got, want = out[plane][has][:, :3], attrs[has][:, 0, lo:lo + 3].view(U32)
                zero = (want & 0x7FFFFFFF) == 0
                assert np.array_equal(got[~zero], want[~zero]) and ((got[zero] & 0x7FFFFFFF) == 0).all()
            assert np.array_equal(out["ip2"][..., 3][has].view(np.int32), mat[has]) and (out["ip2"][..., 3][~has] == 0xFFFFFFFF).all()
            checked += int(has.sum())
    assert checked > 5000


def test_uv_on_a_triangle_parallel_to_the_image_plane_is_affine():
    """w equal at the three vertices: the perspective-correct weights are the screen-space ones. uv = the pixel centre's position in a quad that covers the
    target exactly, so the stored uv is ((i + 0.5) / W, (j + 0.5) / H) to the rounding of I2 / I3 (a few binary64 ulps, then one binary32 rounding)."""
    w, h = 64, 32                                                                # powers of two: the vertex stage and the centres are exact
    v = np.zeros((4, 11), dtype=F)
    v[:, :3] = [(-1, 1, 0.5), (1, 1, 0.5), (1, -1, 0.5), (-1, -1, 0.5)]
    v[:, 3:9] = (0, 0, -1, 1, 0, 0)
    v[:, 9:11] = [(0, 0), (1, 0), (1, 1), (0, 1)]
    m = 3.0 * np.eye(4, dtype=F)[None]                                            # clip = 3 (x, y, z, 1): w = 3 everywhere
    mats = (m, np.eye(4, dtype=F)[None], np.eye(4, dtype=F)[None], m)
    sc = IC.scene(w, h, 1, [IC.draw(v, [0, 1, 2, 0, 2, 3], mats, 5)])
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    owner = np.where(ii * h >= jj * w, 0, 1).astype(U32)                          # the diagonal splits the quad; either triangle gives the same affine map
    for own in (owner, np.zeros_like(owner), np.ones_like(owner)):                 # ... also where the centre lies outside the owner
        out = I.interpolate(sc, own)
        u, vv = as_f32(out["ip0"][..., 3]), as_f32(out["ip1"][..., 3])
        assert np.array_equal(u, ((ii + 0.5) / w).astype(F)) and np.array_equal(vv, ((jj + 0.5) / h).astype(F))
        assert (out["ip2"][..., 3] == 5).all() and np.array_equal(as_f32(out["sv_curr"][..., 3]), np.full((h, w), 3.0, dtype=F))


# ---- (c) I2 against R6's form ------------------------------------------------------------------------------------------------------------------------------------------
def test_weights_agree_with_the_screen_space_form_where_all_w_are_positive():
    """§7.16 R6 interpolates with k_i = b_i / w_i over their sum, b_i the screen-space barycentrics. For triangles in front of the camera that is the same function
    as I2's homogeneous determinants; evaluated in binary64 at the pixel centre from the unsnapped projections, the attributes agree to the cancellation of the
    edge functions. The largest difference in binary32 ulps of the attribute is recorded (printed; §7.18 quotes it) — measured at the value, which is without
    bound where an attribute passes through zero inside a triangle (clip x and y do, on every triangle that crosses an axis of the screen), and measured in ulps
    of the triangle's largest vertex value of that attribute, where the bound asserted is one binary32 ulp: both are binary64 evaluations, so their errors are
    2^-53 of that scale times the conditioning of the edge functions, 2^-29 binary32 ulps times that conditioning; a triangle that owns a pixel centre after the
    16.8 snap cannot be conditioned as badly as 2^29."""
    worst, where, worst_scaled = 0.0, None, 0.0
    for name, sc in IC.cases().items():
        W, H = sc["width"], sc["height"]
        for k, owner in enumerate(IC.owners(name)[0]):
            has, attrs, *_ = I.gather(sc, owner)
            m = has & np.all(attrs[..., I.CLIP + 3] > 0, axis=-1)
            if not m.any():
                continue
            l1, l2, _, _ = I.weights(attrs, W, H)
            X, Y = I.pixel_centres(W, H)
            X, Y = np.broadcast_to(X, m.shape)[m], np.broadcast_to(Y, m.shape)[m]
            a = attrs[m].astype(F64)                                               # [n, 3, 19]
            w = a[..., I.CLIP + 3]
            sx, sy = a[..., I.CLIP] / w, a[..., I.CLIP + 1] / w
            e = lambda p, q: (sx[:, p] - X) * (sy[:, q] - Y) - (sx[:, q] - X) * (sy[:, p] - Y)      # noqa: E731
            kk = np.stack([e(1, 2) / w[:, 0], e(2, 0) / w[:, 1], e(0, 1) / w[:, 2]], axis=1)
            lam = kk / kk.sum(axis=1, keepdims=True)
            r6 = (lam[:, :, None] * a).sum(axis=1)
            mine = (a[:, 0] + l1[m][:, None] * (a[:, 1] - a[:, 0])) + l2[m][:, None] * (a[:, 2] - a[:, 0])
            ulp = np.spacing(np.maximum(np.abs(r6).astype(F), F(2.0 ** -126))).astype(F64)
            u = np.abs(mine - r6) / ulp
            if u.max() > worst:
                worst, where = float(u.max()), (name, k)
            scale = np.spacing(np.maximum(np.abs(a).max(axis=1).astype(F), F(2.0 ** -126))).astype(F64)      # one ulp of the triangle's largest vertex value
            worst_scaled = max(worst_scaled, float((np.abs(mine - r6) / scale).max()))
    print(f"I2 / I3 against R6's form in binary64: max {worst!r} binary32 ulps at the value at {where}; {worst_scaled!r} ulps of the triangle's largest vertex value")
    assert worst_scaled < 1.0, "the two forms are not the same function"


# ---- (d) exact rational cross-check --------------------------------------------------------------------------------------------------------------------------------------
def _round_to_f32(v):
    """the binary32 value nearest to the Fraction v (ties to even; no overflow in this test set), with the exponent of its ulp"""
    if v == 0:
        return Fraction(0), -149
    e = max(int(np.floor(np.log2(float(abs(v))))) - 23, -149)
    while abs(v) >= Fraction(2) ** (e + 24):
        e += 1
    while e > -149 and abs(v) < Fraction(2) ** (e + 23):
        e -= 1
    return Fraction(round(v / Fraction(2) ** e)) * Fraction(2) ** e, e


def _exact_pixel(attrs, i, j, W, H):
    """I2 / I3 in exact rational arithmetic on the binary32 vertex values: [19] Fractions, or None where den is 0"""
    c = [[Fraction(float(attrs[v, I.CLIP + o])) for o in (0, 1, 3)] for v in range(3)]
    X, Y = Fraction(2 * i + 1, W) - 1, 1 - Fraction(2 * j + 1, H)
    D = lambda a, b: X * (a[1] * b[2] - a[2] * b[1]) - Y * (a[0] * b[2] - a[2] * b[0]) + (a[0] * b[1] - a[1] * b[0])      # noqa: E731
    k = (D(c[1], c[2]), D(c[2], c[0]), D(c[0], c[1]))
    den = k[0] + k[1] + k[2]
    if den == 0:
        return None
    l1, l2 = k[1] / den, k[2] / den
    a = [[Fraction(float(attrs[v, n])) for n in range(I.N_ATTR)] for v in range(3)]
    return [a[0][n] + l1 * (a[1][n] - a[0][n]) + l2 * (a[2][n] - a[0][n]) for n in range(I.N_ATTR)]


def test_exact_rational_cross_check():
    """A seeded sample of owned pixels — at least 2 000, drawn from every case and layer — evaluated in exact rational arithmetic. "Including every pixel of
    classes (a)" is read as: every CLASS of the coverage test occurs in the sample (up to 12 pixels of each class per owner plane, then up to 40 more of any
    kind), not every pixel of those classes; §7.18 says the same. The sample is evaluated
    on the same binary32 vertex values. The largest deviation of the statement's stored value from the correctly rounded exact value, in binary32 ulps — at the
    value, and in ulps of the triangle's largest vertex value of the attribute (the first is without bound where an attribute passes through zero) — is a
    RECORD, not a tolerance: §7.18 carries it with its case and pixel, and this test asserts the committed figure (correctly rounded arithmetic and seeded
    scenes: deterministic). Pixels whose exact den is 0 are listed, not compared."""
    rng = np.random.default_rng(0x718)
    worst, where, n_px, zero_den, worst_scaled, where_scaled = Fraction(0), None, 0, [], Fraction(0), None
    per_class = dict.fromkeys(("behind", "outside", "later_instance", "later_draw"), 0)
    for name, sc in IC.cases().items():
        W, H = sc["width"], sc["height"]
        for k, (owner, (out, st)) in enumerate(zip(IC.owners(name)[0], IC.expected(name))):
            has, attrs, *_ = I.gather(sc, owner)
            picks = set()
            for c in per_class:                                                  # up to 12 of each class, then up to 40 more of any kind
                cand = np.argwhere(st["masks"][c])
                for p in cand[rng.permutation(len(cand))[:12]]:
                    picks.add((int(p[0]), int(p[1])))
                    per_class[c] += 1
            cand = np.argwhere(has)
            picks |= {(int(p[0]), int(p[1])) for p in cand[rng.permutation(len(cand))[:40]]}
            stored = np.stack([out["ip0"][..., 0], out["ip0"][..., 1], out["ip0"][..., 2], out["ip1"][..., 0], out["ip1"][..., 1], out["ip1"][..., 2],
                               out["ip2"][..., 0], out["ip2"][..., 1], out["ip2"][..., 2], out["ip0"][..., 3], out["ip1"][..., 3],
                               *(out["sv_curr"][..., n] for n in range(4)), *(out["sv_prev"][..., n] for n in range(4))], axis=-1).view(F)
            for (j, i) in sorted(picks):
                exact = _exact_pixel(attrs[j, i], i, j, W, H)
                if exact is None:
                    zero_den.append((name, k, i, j))
                    continue
                n_px += 1
                for n in range(I.N_ATTR):
                    r, e = _round_to_f32(exact[n])
                    dev = abs(Fraction(float(stored[j, i, n])) - r) / Fraction(2) ** e
                    if dev > worst:
                        worst, where = dev, (name, k, i, j, n)
                    big = max(abs(Fraction(float(attrs[j, i, v, n]))) for v in range(3))
                    dev = abs(Fraction(float(stored[j, i, n])) - r) / Fraction(2) ** _round_to_f32(big)[1]
                    if dev > worst_scaled:
                        worst_scaled, where_scaled = dev, (name, k, i, j, n)
    print(f"I2 / I3 exact cross-check: {n_px} pixels, classes {per_class}; max {float(worst)!r} binary32 ulps at the value at {where}; "
          f"max {float(worst_scaled)!r} ulps of the triangle's largest vertex value at {where_scaled}; exact den == 0 at {zero_den}")
    assert n_px >= 2000 and all(v > 0 for v in per_class.values())
    doc = open(os.path.join(ROOT, "docs", "DESIGN_DETAILS.md")).read()
    section = doc[doc.index("### 7.18"):]
    name, k, i, j, n = where
    assert f"**{float(worst)!r}** binary32 ulps" in section and f"`{name}`" in section and f"pixel ({i}, {j})" in section, "§7.18 does not carry the measured figure"
    name, k, i, j, n = where_scaled
    assert f"**{float(worst_scaled)!r}** ulps of the triangle's largest vertex value" in section and f"`{name}`, layer {k}, pixel ({i}, {j})" in section
    assert f"{n_px} pixels" in section and f"exact `den` is 0 at {len(zero_den)} of them" in section


# ---- (e) boundary ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    declared = set(re.findall(r"VQHIP_API\s+[\w\s\*]+?\b(vqhip_scene_interpolants\w*)\s*\(", src))
    assert declared == NEW_SYMBOLS
    lib = capi.load_library()
    for s in declared:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.vqhip_abi_version() == abi.ABI_VERSION == 3                     # additions only
    assert "stays with the caller. */\ntypedef struct vqhip_interpolants" not in src
    section = src[src.index("The lit draw's interpolants from meshes"):]
    for word in ("UNPINNED", "NO OWNER", "0x7FC00000", "centroid", "uv LOD", "same order"):
        assert word in section, f"{word} is not stated in the header section"


def test_struct_layout_equals_the_c_header(tmp_path):
    structs = (("vqhip_scene_surface_draw", abi.SceneSurfaceDraw), ("vqhip_scene_interpolant_targets", abi.SceneInterpolantTargets))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vqhip.h"\nint main(void){\n'
    for cname, t in structs:
        prog += f'printf("%zu", sizeof({cname}));\n' + "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in t._fields_) + 'printf("\\n");\n'
    prog += "return 0;}\n"
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    lines = subprocess.check_output([str(tmp_path / "t")]).decode().strip().split("\n")
    for (cname, t), line in zip(structs, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_], cname
    assert (C.sizeof(abi.SceneSurfaceDraw), C.sizeof(abi.SceneInterpolantTargets)) == (72, 48)


def test_work_size_function():
    f = capi.load_library().vqhip_scene_interpolants_work_bytes
    assert f(0) == 256 and f(1) == 256 and f(3) == 256 and f(4) == 512            # 80 bytes per draw, rounded up to 256
    counts = (1, 4, 100, 2000, 20000)
    sizes = [f(n) for n in counts]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    for n, s in zip(counts, sizes):
        assert n * abi.SURFACE_JOB_BYTES <= s < n * abi.SURFACE_JOB_BYTES + 256
    assert f(-1) == 0
    assert capi.scene_interpolants_work_bytes(2000) == f(2000)


def test_call_without_a_context_is_refused():
    lib = capi.load_library()
    tg = abi.SceneInterpolantTargets()
    buf = (C.c_uint8 * 4096)()
    rc = lib.vqhip_scene_interpolants(None, None, None, 0, 16, 16, buf, 0, C.byref(tg), buf, 4096)
    assert rc == abi.VQHIP_ERR_INVALID_ARG and b"ctx is NULL" in lib.vqhip_last_error(None)


# ---- the host-side producers ------------------------------------------------------------------------------------------------------------------------------------------
def test_full_vertex_meshes():
    v, idx = SS.box((0.5, 1.0, 2.0))
    assert v.shape == (24, 11) and v.dtype == F and idx.shape == (36,)
    p, n, t = v[:, :3].astype(F64), v[:, 3:6].astype(F64), v[:, 6:9].astype(F64)
    for tri in idx.reshape(-1, 3):
        g = np.cross(p[tri[1]] - p[tri[0]], p[tri[2]] - p[tri[0]])               # the winding of shadow_scene.box (checked below): this product points outwards
        assert np.dot(g, n[tri[0]]) > 0 and np.array_equal(n[tri[0]], n[tri[1]]) and np.array_equal(n[tri[0]], n[tri[2]])
        assert abs(np.dot(n[tri[0]], t[tri[0]])) == 0 and np.array_equal(t[tri[0]], t[tri[2]])
    assert set(map(tuple, v[:, 9:11])) == {(0, 0), (0, 1), (1, 1), (1, 0)}
    # the same solid as shadow_scene's box: the same set of corner positions, the same number of triangles per face direction
    p0, i0 = S.box((0.5, 1.0, 2.0))
    assert set(map(tuple, p0)) == set(map(tuple, v[:, :3])) and len(i0) == len(idx)
    for tri in i0.reshape(-1, 3):
        q = p0[tri].astype(F64)
        assert np.dot(np.cross(q[1] - q[0], q[2] - q[0]), q.sum(axis=0)) > 0
    rv, ri = SS.room((0.5, 1.0, 2.0))
    assert np.array_equal(rv[:, 3:6], -v[:, 3:6]) and np.array_equal(ri.reshape(-1, 3), idx.reshape(-1, 3)[:, ::-1])
    sv, si = SS.uv_sphere(2.0, 24, 22)
    sp, sidx = S.uv_sphere(2.0, 24, 22)
    assert np.array_equal(sv[:, :3], sp) and np.array_equal(si, sidx) and sv.shape[1] == 11
    assert np.allclose(np.linalg.norm(sv[:, 3:6], axis=1), 1, atol=1e-6) and np.allclose((sv[:, 3:6] * sv[:, 6:9]).sum(axis=1), 0, atol=1e-6)
    assert sv[:, 9].min() >= 0 and sv[:, 9].max() < 1 and sv[0, 10] == 0 and sv[-1, 10] == 1
    gv, gi = SS.grid(5, 4.0, 0.3, seed=2)
    gp, gidx = S.grid(5, 4.0, 0.3, seed=2)
    assert np.array_equal(gv[:, :3], gp) and np.array_equal(gi, gidx) and (gv[:, 4] == 1).all() and (gv[:, 6] == 1).all()
    assert gv[:, 9:11].min() == 0 and gv[:, 9:11].max() == 1


def test_instance_matrices_full():
    world = S.scaling((2.0, 0.5, 3.0)) @ S.rotation_y(0.7) @ S.rotation_x(-0.4) @ S.translation((1.0, 2.0, 3.0))
    vp = S.camera_view_proj((0, 0, -3), (0, 0, 0), 1.0, 1.5, 0.1, 10.0)
    pvp = S.camera_view_proj((0.1, 0, -3), (0, 0, 0), 1.0, 1.5, 0.1, 10.0)
    wvp, w, n, prev = SS.instance_matrices_full([world, np.eye(4)], vp, pvp)
    assert all(m.shape == (2, 4, 4) and m.dtype == F and m.flags["C_CONTIGUOUS"] for m in (wvp, w, n, prev))
    assert np.array_equal(wvp[0], (world @ vp).astype(F)) and np.array_equal(prev[0], (world @ pvp).astype(F)) and np.array_equal(w[0], world.astype(F))
    rot = (S.rotation_y(0.7) @ S.rotation_x(-0.4))
    assert np.allclose(n[0], rot, atol=1e-6) and np.array_equal(n[1], np.eye(4, dtype=F))      # the rotation alone (Batching.cpp:281): no scale, no translation
    _, _, _, moved = SS.instance_matrices_full([world], vp, pvp, prev_worlds=[world @ S.translation((0.5, 0, 0))])
    assert np.array_equal(moved[0], (world @ S.translation((0.5, 0, 0)) @ pvp).astype(F))
