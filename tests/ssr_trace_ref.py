"""The contract of vqhip_ssr_classify and vqhip_ssr_intersect (docs/DESIGN_DETAILS.md §7.11) in numpy binary32: the ray decision of
ClassifyReflectionTiles.hlsl:ClassifyTiles in this library's order (8 x 8 tiles row-major, lanes of RemapLane8x8 inside a tile), and Intersect.hlsl:CSMain +
ffx_sssr.h for every entry of the list — every expression as written, one rounding per operation, in either arithmetic reading. All rays of a 64-ray group march
in LOCKSTEP, so WaveActiveCountBits(true) at an iteration is exactly the number of the group's rays still inside the loop.
Shared primitives come from the CPU oracle's exports (sin / cos of the arithmetic contract, the cube and LUT fetches, pow, UNORM8 decode); numpy's own binary32
add / mul / div / sqrt are the IEEE operations. Nothing under oracle/ knows these passes: this file is the checker."""
import ctypes as C

import numpy as np

from tests import oracle_lib as O
from tests.depth_ref import _fma32, decode_normals01, normalize32
from vqengine_amd import abi

F = np.float32
FLT_MAX = F(3.402823466e+38)
TWO_PI = F(2.0) * F(3.14159265358979)             # 2.0 * M_PI with M_PI = 3.14159265358979f
LANES = np.arange(64)
LANE_X, LANE_Y = (LANES & 1) | ((LANES >> 2) & 6), ((LANES >> 1) & 3) | ((LANES >> 3) & 4)      # FFX_DNSR_Reflections_RemapLane8x8


def matrix(m):
    return np.array([[m.m[i][j] for j in range(4)] for i in range(4)], F)


def pow_half(mip):
    """pow(0.5, mip) of FFX_SSSR_GetMipResolution: 2^-mip exactly for mip 0..12 (asserted by tests/test_ssr_trace_cpu.py)"""
    return np.ldexp(F(1.0), -np.asarray(mip, np.int64)).astype(F)


# ---- classification ---------------------------------------------------------------------------------------------------------------------------
def classify(scene, depth, cb, variance=None):
    """scene: [H,W,4] float16 | float32 (alpha = roughness); depth float32 [H,W]; variance None | float16 [H,W]. Returns a dict: rays uint32 [n] (PackRayCoords, in
    the contract's order), counters uint32 [2], tiles uint32 [m] ((y << 16) | x of the listed tiles' first pixel, tile order)."""
    w, h = int(cb.bufferDimensions[0]), int(cb.bufferDimensions[1])
    tx, ty = (w + 7) // 8, (h + 7) // 8
    x = (np.arange(tx)[None, :, None] * 8 + LANE_X[None, None, :]) + np.zeros((ty, 1, 1), np.int64)
    y = (np.arange(ty)[:, None, None] * 8 + LANE_Y[None, None, :]) + np.zeros((1, tx, 1), np.int64)
    on = (x < w) & (y < h)
    xc, yc = np.minimum(x, w - 1), np.minimum(y, h - 1)
    rough = np.where(on, np.asarray(scene)[..., 3].astype(F)[yc, xc], F(0))                       # a load outside the texture reads 0
    z = np.where(on, np.asarray(depth, F)[yc, xc], F(0))
    with np.errstate(invalid="ignore"):
        reflective = z < F(1.0)
        glossy = rough < F(cb.roughnessThreshold)
        needs = on & glossy & reflective
        den = needs & ~(rough < F(0.04))
        spq = int(cb.samplesPerQuad)
        base = (((x & 1) | (y & 1)) == 0) if spq == 1 else ((x & 1) == (y & 1)) if spq == 2 else np.ones_like(on)
        needs = needs & (~den | base)
        if cb.temporalVarianceGuidedTracingEnabled:
            var = np.where(on, np.asarray(variance).astype(F)[yc, xc], F(0)) if variance is not None else np.zeros(on.shape, F)
            needs = needs | (den & ~needs & (var > F(cb.varianceThreshold)))
    copy = ~needs & den
    ch = (spq != 4) & base & copy[..., LANES ^ 1]
    cv = (spq == 1) & base & copy[..., LANES ^ 2]
    cd = (spq == 1) & base & copy[..., LANES ^ 3]
    packed = ((cd.astype(np.uint32) << 31) | (cv.astype(np.uint32) << 30) | (ch.astype(np.uint32) << 29) | ((y.astype(np.uint32) & 0x3FFF) << 15)
              | (x.astype(np.uint32) & 0x7FFF)).astype(np.uint32)
    rays = packed[needs]                                                                        # C order: tile row, tile column, lane
    tile_hit = (glossy & reflective).any(-1)                                                    # as written (:126): not masked by the screen test
    tiles = (((y[..., 0].astype(np.uint32) & 0xFFFF) << 16) | (x[..., 0].astype(np.uint32) & 0xFFFF))[tile_hit]
    return {"rays": rays, "counters": np.array([rays.size, tiles.size], np.uint32), "tiles": tiles.astype(np.uint32)}


# ---- intrinsics (§7.11) -----------------------------------------------------------------------------------------------------------------------
def _min2(a, b):
    return np.where((b < a) | np.isnan(a), b, a)


def _max2(a, b):
    return np.where((b > a) | np.isnan(a), b, a)


def _sat(x):
    return np.where(x > 0, np.where(x < 1, x, F(1)), F(0)).astype(F)


def _ftoi(x):
    """float -> int of Texture.Load: truncation, NaN -> 0, saturating"""
    x = np.where(np.isnan(x), F(0), x).astype(np.float64)
    return np.clip(np.trunc(x), -2147483648.0, 2147483647.0).astype(np.int64)


def _dot(a, b, dxc):
    if dxc:
        return _fma32(a[2], b[2], _fma32(a[1], b[1], a[0] * b[0]))
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalize(v, dxc):
    n = normalize32(np.stack(v, -1), dxc)
    return n[..., 0], n[..., 1], n[..., 2]


def _length(v, dxc):
    return np.sqrt(_dot(v, v, dxc))


def _reflect(i, n, dxc):
    t = F(2.0) * _dot(n, i, dxc)
    return tuple(i[k] - t * n[k] for k in range(3))


def _cross(a, b):
    return a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]


def _mul_m(M, x, y, z, w):
    """mul(M_hlsl, float4(v, w)) == the row vector times the row-major matrix, summed left to right"""
    w = F(w)
    return tuple(((x * M[0, j] + y * M[1, j]) + z * M[2, j]) + w * M[3, j] for j in range(4))


def _inv_project(M, u, v, z):
    cy = F(1.0) - v
    px, py = F(2.0) * u - F(1.0), F(2.0) * cy - F(1.0)
    p = _mul_m(M, px, py, z, 1.0)
    return p[0] / p[3], p[1] / p[3], p[2] / p[3]


def _smoothstep(lo, hi, x):
    t = _sat((x - lo) / (hi - lo))
    return (t * t) * (F(3.0) - F(2.0) * t)


def _oracle_math(fn, a):
    return O.math_array(fn, np.ascontiguousarray(a, F).ravel()).reshape(np.shape(a))


def load_depth(levels, x, y, mip):
    """FFX_SSSR_LoadDepth: outside the level, or a level that does not exist: 0.0"""
    out = np.zeros(np.shape(x), F)
    for l in np.unique(mip):
        if 0 <= l < len(levels):
            lv = levels[l]
            m = (mip == l) & (x >= 0) & (y >= 0) & (x < lv.shape[1]) & (y < lv.shape[0])
            out[m] = lv[y[m], x[m]]
    return out


def _load_normal(normals01, x, y, dxc):
    h, w = normals01.shape[:2]
    ok = (x >= 0) & (y >= 0) & (x < w) & (y < h)
    n = np.where(ok[..., None], normals01[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], F(0))
    return _normalize(tuple(F(2.0) * n[..., k] - F(1.0) for k in range(3)), dxc)


def _environment(env, rot, direction, ndotv, roughness, pow5_explog):
    """SampleEnvironmentMap (Intersect.hlsl:132-137): level 0 of the cube along envMapRotation * direction, EnvironmentBRDF with metallic 1"""
    lib = O.load()
    d = np.ascontiguousarray(np.stack([(direction[0] * rot[0, k] + direction[1] * rot[1, k]) + direction[2] * rot[2, k] for k in range(3)], -1), F)
    n = d.shape[0]
    pre, sb = np.zeros((n, 4), F), np.zeros((n, 2), F)
    nv, ro = np.ascontiguousarray(ndotv, F), np.ascontiguousarray(roughness, F)
    cube, lut = C.c_void_p(env.specular_cube), C.c_void_p(env.brdf_lut)
    f_cube, f_lut = lib.vqo_sample_cube_lod_rgba16f, lib.vqo_sample_2d_rg16f_clamp
    f_cube.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p]
    f_lut.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]
    pd, pp, ps = d.ctypes.data, pre.ctypes.data, sb.ctypes.data
    for i in range(n):
        f_cube(cube, env.spec_res0, env.spec_mips, pd + 12 * i, 0.0, pp + 16 * i)
        f_lut(lut, env.lut_size, env.lut_size, float(nv[i]), float(ro[i]), ps + 8 * i)
    f0 = F(0.04) + F(1.0) * (F(0.0) - F(0.04))
    x = F(1.0) - nv
    if pow5_explog:
        p5 = O.math_array(2, x, np.full_like(x, F(5.0)))
    else:
        x2 = x * x
        p5 = x * (x2 * x2)
    ks = f0 + (np.maximum(F(1.0) - ro, f0) - f0) * p5
    kd = (F(1.0) - ks) * (F(1.0) - F(1.0))
    diffuse = F(0.0) * F(0.0)
    k = ks * sb[:, 0] + sb[:, 1]
    return tuple(kd * diffuse + pre[:, c] * k for c in range(3))


# ---- the march and the hit validation --------------------------------------------------------------------------------------------------------------
def march(ox, oy, oz, dx, dy, dz, mirror, mdm, live, levels, w, h, max_iter, min_occ):
    """FFX_SSSR_HierarchicalRaymarch (ffx_sssr.h:86-127) for rays laid out [groups, 64], all float32 / int64 / bool arrays of that shape: the rays of a row march in
    lockstep and WaveActiveCountBits(true) is the number of the row's rays inside the loop. Returns a dict: px, py, pz (the hit), iterations, low (left by the
    occupancy term), mip (on leaving), top (the highest level loaded from)."""
    fw, fh = F(w), F(h)
    G = ox.shape[0]
    with np.errstate(all="ignore"):
        res_x, res_y = fw * pow_half(mdm), fh * pow_half(mdm)
        ix, iy, iz = (np.where(d != 0, F(1.0) / d, FLT_MAX).astype(F) for d in (dx, dy, dz))
        mip = mdm.copy()
        rinv_x, rinv_y = F(1.0) / res_x, F(1.0) / res_y
        e2 = F(0.005) * np.ldexp(F(1.0), mdm).astype(F)
        uo_x, uo_y = e2 / fw, e2 / fh
        uo_x, uo_y = np.where(dx < 0, -uo_x, uo_x), np.where(dy < 0, -uo_y, uo_y)
        fo_x, fo_y = np.where(dx < 0, F(0), F(1)).astype(F), np.where(dy < 0, F(0), F(1)).astype(F)
        pl_x, pl_y = (np.floor(res_x * ox) + fo_x) * rinv_x + uo_x, (np.floor(res_y * oy) + fo_y) * rinv_y + uo_y
        t = _min2(pl_x * ix - ox * ix, pl_y * iy - oy * iy).astype(F)
        px, py, pz = ox + t * dx, oy + t * dy, oz + t * dz
        it = np.zeros((G, 64), np.int64)
        low = np.zeros((G, 64), bool)
        top = mip.copy()                                                                        # the highest level each ray loaded from
        inl = live & (it < max_iter) & (mip >= mdm)
        while inl.any():
            cnt = np.broadcast_to(inl.sum(1, keepdims=True), inl.shape)[inl]                    # WaveActiveCountBits(true) of each ray's group
            s = lambda a: a[inl]
            mpx, mpy = s(res_x) * s(px), s(res_y) * s(py)
            sz = load_depth(levels, _ftoi(mpx), _ftoi(mpy), s(mip))
            top[inl] = np.maximum(s(top), s(mip))
            lo = ~s(mirror) & (cnt <= min_occ)
            ql_x, ql_y = (np.floor(mpx) + s(fo_x)) * s(rinv_x) + s(uo_x), (np.floor(mpy) + s(fo_y)) * s(rinv_y) + s(uo_y)
            tx, ty = ql_x * s(ix) - s(ox) * s(ix), ql_y * s(iy) - s(oy) * s(iy)
            tz = sz * s(iz) - s(oz) * s(iz)
            tz = np.where(s(dz) > 0, tz, FLT_MAX).astype(F)
            tmin = _min2(_min2(tx, ty), tz).astype(F)
            above = sz > s(pz)
            skipped = (tmin.view(np.uint32) != tz.view(np.uint32)) & above
            tn = np.where(above, tmin, s(t)).astype(F)
            npx, npy, npz = s(ox) + tn * s(dx), s(oy) + tn * s(dy), s(oz) + tn * s(dz)
            nm = s(mip) + np.where(skipped, 1, -1)
            f_res, f_inv = np.where(skipped, F(0.5), F(2.0)).astype(F), np.where(skipped, F(2.0), F(0.5)).astype(F)
            nrx, nry, nix, niy = s(res_x) * f_res, s(res_y) * f_res, s(rinv_x) * f_inv, s(rinv_y) * f_inv
            ni = s(it) + 1
            t[inl], px[inl], py[inl], pz[inl], mip[inl] = tn, npx, npy, npz, nm
            res_x[inl], res_y[inl], rinv_x[inl], rinv_y[inl], it[inl], low[inl] = nrx, nry, nix, niy, ni, lo
            nxt = np.zeros_like(inl)
            nxt[inl] = (ni < max_iter) & (nm >= s(mdm)) & ~lo
            inl = nxt
    return {"px": px, "py": py, "pz": pz, "iterations": it, "low": low, "mip": mip, "top": top}


def validate_hit(px, py, pz, u, v, wray, valid, levels, normals01, inv_proj, w, h, thickness, dxc=False):
    """FFX_SSSR_ValidateHit (ffx_sssr.h:129-173) under valid_hit: the confidence, and the texel int2(screen_size * hit.xy)"""
    fw, fh = F(w), F(h)
    with np.errstate(all="ignore"):
        sample = valid & ~((px < 0) | (py < 0) | (px > 1) | (py > 1))
        sample &= ~((np.abs(px - u) < F(2.0) / fw) & (np.abs(py - v) < F(2.0) / fh))
        hx, hy = _ftoi(fw * px), _ftoi(fh * py)
        sz = load_depth(levels, hx // 2, hy // 2, np.ones_like(hx))
        hn = _load_normal(normals01, hx, hy, dxc)
        sample &= ~(sz == F(1.0)) & ~(_dot(hn, wray, dxc) > 0)
        vs, vh = _inv_project(inv_proj, px, py, sz), _inv_project(inv_proj, px, py, pz)
        dist = _length(tuple(vs[k] - vh[k] for k in range(3)), dxc)
        fov_x, fov_y = F(0.05) * (fh / fw), F(0.05) * F(1.0)
        bx = _smoothstep(F(0), fov_x, px) * (F(1.0) - _smoothstep(F(1.0) - fov_x, F(1.0), px))
        by = _smoothstep(F(0), fov_y, py) * (F(1.0) - _smoothstep(F(1.0) - fov_y, F(1.0), py))
        c = F(1.0) - _smoothstep(F(0), F(thickness), dist)
        conf = np.where(sample, (bx * by) * (c * c), F(0)).astype(F)
    return conf, hx, hy


# ---- intersection -----------------------------------------------------------------------------------------------------------------------------
def intersect(rays, count, lit, levels, normals, normal_fmt, roughness8, noise, cb, env, radiance, dxc=False, pow5_explog=False, groups=None, stats=None):
    """rays: uint32 ray list, count: how many entries are live; lit [H,W,4] (float16 | float32); levels: the depth pyramid (list of float32 arrays, level 0 first);
    normals in normal_fmt; roughness8 uint8 [H,W]; noise uint8 [128,128,2]; env: abi.EnvMap over HOST arrays (None: the environment term is 0 — for the march statistics alone); radiance: the image to write into (a copy is
    returned, in its dtype). groups: None = every 64-ray group, else the group indices to march (the others are not written). stats: a dict that receives per
    marched ray `iterations`, `exit` (0 iteration cap, 1 mip < mostDetailedMip, 2 low occupancy), `confidence`, `ray` (its index in the list), `mirror`, `top_mip` (the highest level it loaded from)."""
    w, h = int(cb.bufferDimensions[0]), int(cb.bufferDimensions[1])
    count = min(int(count), w * h)
    out = np.array(radiance, copy=True)
    n_groups = (count + 63) // 64
    gsel = np.arange(n_groups) if groups is None else np.asarray(sorted(set(int(g) for g in groups if 0 <= int(g) < n_groups)), np.int64)
    if gsel.size == 0:
        return out
    ridx = (gsel[:, None] * 64 + LANES[None, :])
    live = ridx < count
    G = gsel.size
    packed = np.where(live, np.asarray(rays, np.uint32)[np.minimum(ridx, max(count - 1, 0))], np.uint32(0)).astype(np.uint32)
    cx, cy = (packed & 0x7FFF).astype(np.int64), ((packed >> 15) & 0x3FFF).astype(np.int64)
    inv_vp, proj, inv_proj, view, inv_view, rot = (matrix(m) for m in (cb.invViewProjection, cb.projection, cb.invProjection, cb.view, cb.invView, cb.envMapRotation))
    fw, fh = F(w), F(h)
    max_iter, min_occ, mdm_cb = int(cb.maxTraversalIntersections), int(cb.minTraversalOccupancy), int(cb.mostDetailedMip)
    normals01 = decode_normals01(normals, normal_fmt)
    with np.errstate(all="ignore"):
        u = (cx.astype(F) + F(0.5)) * F(cb.inverseBufferDimensions[0])
        v = (cy.astype(F) + F(0.5)) * F(cb.inverseBufferDimensions[1])
        wn = _load_normal(normals01, cx, cy, dxc)
        on = (cx < w) & (cy < h)
        rough = np.where(on, np.asarray(roughness8)[np.minimum(cy, h - 1), np.minimum(cx, w - 1)].astype(F) / F(255.0), F(0))
        mirror = rough < F(0.041)
        mdm = np.where(mirror, 0, mdm_cb).astype(np.int64)
        res_x, res_y = fw * pow_half(mdm), fh * pow_half(mdm)
        z = load_depth(levels, _ftoi(u * res_x), _ftoi(v * res_y), mdm)
        vray = _inv_project(inv_proj, u, v, z)
        dir_v = _normalize(vray, dxc)
        N = _mul_m(view, wn[0], wn[1], wn[2], 0.0)[:3]
        # CreateTBN
        zk = np.abs(N[2]) > 0
        k1, k2 = np.sqrt(N[1] * N[1] + N[2] * N[2]), np.sqrt(N[0] * N[0] + N[1] * N[1])
        zero = np.zeros_like(u)
        U = (np.where(zk, zero, N[1] / k2), np.where(zk, -N[2] / k1, -N[0] / k2), np.where(zk, N[1] / k1, zero))
        B = _cross(N, U)
        nd = tuple(-c for c in dir_v)
        Ve = (_dot(nd, U, False), _dot(nd, B, False), _dot(nd, N, False))
        nz = np.asarray(noise)[cy & 127, cx & 127].astype(F) / F(255.0)
        U1, U2 = nz[..., 0], nz[..., 1]
        # SampleGGXVNDF
        Vh = _normalize((rough * Ve[0], rough * Ve[1], Ve[2]), dxc)
        lensq = Vh[0] * Vh[0] + Vh[1] * Vh[1]
        rs = F(1.0) / np.sqrt(lensq)
        pos = lensq > 0
        T1 = (np.where(pos, -Vh[1] * rs, F(1)), np.where(pos, Vh[0] * rs, F(0)), np.where(pos, F(0.0) * rs, F(0)))
        T2 = _cross(Vh, T1)
        rr = np.sqrt(U1)
        phi = TWO_PI * U2
        sn, cs = _oracle_math(3, phi), _oracle_math(4, phi)
        t1 = rr * cs
        t2 = rr * sn
        sh = F(0.5) * (F(1.0) + Vh[2])
        t2 = (F(1.0) - sh) * np.sqrt(F(1.0) - t1 * t1) + sh * t2
        nhz = np.sqrt(_max2(np.zeros_like(t1), (F(1.0) - t1 * t1) - t2 * t2))
        Nh = tuple((t1 * T1[k] + t2 * T2[k]) + nhz * Vh[k] for k in range(3))
        Ne = _normalize((rough * Nh[0], rough * Nh[1], _max2(np.zeros_like(t1), Nh[2])), dxc)
        Rt = _reflect(tuple(-c for c in Ve), Ne, dxc)
        Rv = tuple((Rt[0] * U[k] + Rt[1] * B[k]) + Rt[2] * N[k] for k in range(3))
        # ProjectDirection
        pp = _mul_m(proj, vray[0] + Rv[0], vray[1] + Rv[1], vray[2] + Rv[2], 1.0)
        ppx = F(0.5) * (pp[0] / pp[3]) + F(0.5)
        ppy = F(1.0) - (F(0.5) * (pp[1] / pp[3]) + F(0.5))
        ppz = pp[2] / pp[3]
        ox, oy, oz = u, v, z
        dx, dy, dz = ppx - ox, ppy - oy, ppz - oz
        r = march(ox, oy, oz, dx, dy, dz, mirror, mdm, live, levels, w, h, max_iter, min_occ)
        px, py, pz, it, low, mip, top = r["px"], r["py"], r["pz"], r["iterations"], r["low"], r["mip"], r["top"]
        valid = it <= max_iter
        wo, wh = _inv_project(inv_vp, ox, oy, oz), _inv_project(inv_vp, px, py, pz)
        wray = tuple(wh[k] - wo[k] for k in range(3))
        conf, hx, hy = validate_hit(px, py, pz, u, v, wray, valid, levels, normals01, inv_proj, w, h, cb.depthBufferThickness, dxc)
        ray_len = _max2(np.zeros_like(u), _length(wray, dxc)).astype(F)
        take = (conf > 0) & (hx >= 0) & (hy >= 0) & (hx < w) & (hy < h)
        litf = np.asarray(lit)
        rad = np.where(take[..., None], litf[np.clip(hy, 0, h - 1), np.clip(hx, 0, w - 1), :3].astype(F), F(0))
        rw = _mul_m(inv_view, Rv[0], Rv[1], Rv[2], 0.0)[:3]
        ndotv = _sat(_dot(N, nd, dxc))
        m = live
        if env is None:                                                                          # statistics only (scripts/ssr_trace_bench.py): no environment term
            envc = tuple(np.zeros(int(m.sum()), F) for _ in range(3))
        else:
            envc = _environment(env, rot, tuple(c_[m] for c_ in rw), ndotv[m], rough[m], pow5_explog)
        res = np.stack([envc[k] + conf[m] * (rad[m][:, k] - envc[k]) for k in range(3)] + [ray_len[m]], -1).astype(F)
    val = res.astype(out.dtype)
    xs, ys, pk = cx[m], cy[m], packed[m]
    for bit, fx, fy in ((None, 0, 0), (29, 1, 0), (30, 0, 1), (31, 1, 1)):
        sel = np.ones(xs.shape, bool) if bit is None else ((pk >> np.uint32(bit)) & 1).astype(bool)
        tx_, ty_ = xs ^ fx, ys ^ fy
        sel &= (tx_ < w) & (ty_ < h)                                                             # a store outside the UAV is dropped
        out[ty_[sel], tx_[sel]] = val[sel]
    if stats is not None:
        stats.update(iterations=it[m], exit=np.where(low[m], 2, np.where(mip[m] < mdm[m], 1, 0)), confidence=conf[m], ray=ridx[m], mirror=mirror[m],
                     top_mip=top[m])
    return out
