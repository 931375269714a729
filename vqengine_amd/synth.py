"""Seeded synthetic inputs of the BASELINE.json configs. numpy only, CPU side;
every generator is keyed so that any row range of a frame can be produced independently (row-tiled
multi-GPU ranks generate just their tile and still agree with the single-GPU frame).

Parameter sources in the reference: light defaults Source/Engine/Scene/Light.cpp:58-73, brightness range
Data/Levels/Default.xml:202-308, fAmbientLightingFactor 0.055 Source/Engine/Scene/SceneViews.h:61,
sun radiance cf. MaxCLL values in Data/EnvironmentMaps.ini."""
import numpy as np

from . import abi

ROW_CHUNK = 32


def _chunk_rng(seed, chunk):
    return np.random.Generator(np.random.Philox(key=[int(seed), int(chunk)]))


def gbuffer_rows(width, frame_height, row0, row1, seed=0xC0FFEE):
    """Rows [row0,row1) of the 4 float4 G-buffer planes of a width x frame_height frame.
    Returns 4 float32 arrays [row1-row0, width, 4]."""
    planes = [np.empty((row1 - row0, width, 4), np.float32) for _ in range(4)]
    c0, c1 = row0 // ROW_CHUNK, (row1 + ROW_CHUNK - 1) // ROW_CHUNK
    for ch in range(c0, c1):
        r = _chunk_rng(seed, ch)
        n = ROW_CHUNK
        rows = np.arange(ch * ROW_CHUNK, ch * ROW_CHUNK + n)
        u = r.random((n, width, 16), dtype=np.float32)
        g = [np.empty((n, width, 4), np.float32) for _ in range(4)]
        # gb0 = (P, ao): P on a height field over [-50,50]^2, y in [-5,5]
        cols = np.arange(width, dtype=np.float32)
        g[0][..., 0] = (-50.0 + 100.0 * (cols + 0.5) / width)[None, :]
        g[0][..., 1] = -5.0 + 10.0 * u[..., 0]
        g[0][..., 2] = (-50.0 + 100.0 * (rows.astype(np.float32) + 0.5) / frame_height)[:, None]
        g[0][..., 3] = 0.055 * (0.3 + 0.7 * u[..., 1])
        # gb1 = (N, roughness): uniform upper hemisphere (+Y up), perturbed by +-1e-3 and NOT renormalised
        z = u[..., 2]
        phi = 2.0 * np.pi * u[..., 3]
        rad = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        g[1][..., 0] = rad * np.cos(phi) + (u[..., 4] - 0.5) * 2e-3
        g[1][..., 1] = z + (u[..., 5] - 0.5) * 2e-3
        g[1][..., 2] = rad * np.sin(phi) + (u[..., 6] - 0.5) * 2e-3
        g[1][..., 3] = 0.05 + 0.95 * u[..., 7]
        # gb2 = (diffuse linear, metalness in {0,1} w.p. 1/2 else U[0,1])
        g[2][..., 0:3] = u[..., 8:11]
        m = u[..., 11]
        g[2][..., 3] = np.where(m < 0.25, 0.0, np.where(m < 0.5, 1.0, (m - 0.5) * 2.0))
        # gb3 = (emissive colour, intensity): zero for 95 % of the pixels
        em = u[..., 12] > 0.95
        g[3][..., 0:3] = np.where(em[..., None], u[..., 13:16], 0.0)
        g[3][..., 3] = np.where(em, 5.0 * ((u[..., 12] - 0.95) * 20.0), 0.0)
        lo, hi = max(row0, ch * ROW_CHUNK), min(row1, (ch + 1) * ROW_CHUNK)
        for k in range(4):
            planes[k][lo - row0:hi - row0] = g[k][lo - ch * ROW_CHUNK:hi - ch * ROW_CHUNK].astype(np.float32)
    return planes


def gbuffer(width, height, seed=0xC0FFEE, coherent=False):
    return (gbuffer_rows_coherent if coherent else gbuffer_rows)(width, height, 0, height, seed)


def _hash01(a, b, c):
    """Integer hash of (a, b, c) -> float32 in [0,1): material parameters of a region, independent of how the frame is cut into rows."""
    h = (np.asarray(a, np.uint64) * np.uint64(0x9E3779B1) + np.asarray(b, np.uint64) * np.uint64(0x85EBCA77) + np.uint64(c) * np.uint64(0xC2B2AE3D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15); h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(12); h = (h * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    return (h >> np.uint64(8)).astype(np.float32) / np.float32(1 << 24)


def gbuffer_rows_coherent(width, frame_height, row0, row1, seed=0xC0FFEE):
    """A SURFACE-COHERENT frame, next to the white-noise one of gbuffer_rows (which stays the BASELINE workload): what the engine's rasteriser
    hands to PSMain on real content. Rolling terrain over [-50,50]^2 seen from above (P on a smooth height field, N = the field's analytic normal
    with a fine normal-map ripple, NOT renormalised), materials in 96 x 64-pixel regions: per-region albedo / metalness / roughness with a
    little per-pixel grain, 12 % of the regions POLISHED (roughness 0, 0.01, 0.02 or 0.03: the GGX EPSILON early-out range, shade.hip), 3 % emissive.
    Any row range can be produced on its own (row-tiled ranks agree with the untiled frame)."""
    planes = [np.empty((row1 - row0, width, 4), np.float32) for _ in range(4)]
    c0, c1 = row0 // ROW_CHUNK, (row1 + ROW_CHUNK - 1) // ROW_CHUNK
    cols = np.arange(width, dtype=np.float32)
    X = (-50.0 + 100.0 * (cols + 0.5) / width)[None, :].astype(np.float32)
    for ch in range(c0, c1):
        r = _chunk_rng(seed ^ 0x5EED, ch)
        n = ROW_CHUNK
        rows = np.arange(ch * ROW_CHUNK, ch * ROW_CHUNK + n)
        u = r.random((n, width, 6), dtype=np.float32)
        Z = (-50.0 + 100.0 * (rows.astype(np.float32) + 0.5) / frame_height)[:, None].astype(np.float32)
        g = [np.empty((n, width, 4), np.float32) for _ in range(4)]
        # height field and its gradient
        hgt = 3.0 * np.sin(0.11 * X) * np.cos(0.07 * Z) + 1.2 * np.sin(0.31 * X + 0.23 * Z) + 0.4 * np.cos(0.9 * Z)
        dhx = 3.0 * 0.11 * np.cos(0.11 * X) * np.cos(0.07 * Z) + 1.2 * 0.31 * np.cos(0.31 * X + 0.23 * Z)
        dhz = -3.0 * 0.07 * np.sin(0.11 * X) * np.sin(0.07 * Z) + 1.2 * 0.23 * np.cos(0.31 * X + 0.23 * Z) - 0.4 * 0.9 * np.sin(0.9 * Z)
        # fine ripple (a tiling normal map) on top of the geometric normal
        dhx = dhx + 0.15 * np.sin(5.3 * X) * np.cos(4.1 * Z)
        dhz = dhz + 0.15 * np.cos(4.7 * X) * np.sin(5.9 * Z)
        inv = (1.0 / np.sqrt(dhx * dhx + dhz * dhz + 1.0)).astype(np.float32)
        g[0][..., 0] = np.broadcast_to(X, (n, width)); g[0][..., 1] = hgt; g[0][..., 2] = np.broadcast_to(Z, (n, width))
        g[0][..., 3] = 0.055 * (0.55 + 0.45 * np.cos(0.5 * X) * np.sin(0.4 * Z) ** 2)
        g[1][..., 0] = -dhx * inv; g[1][..., 1] = inv; g[1][..., 2] = -dhz * inv
        # material regions
        bx = (np.arange(width) // 96)[None, :] + np.zeros((n, 1), np.int64)
        by = (rows // 64)[:, None] + np.zeros((1, width), np.int64)
        hk = lambda c: _hash01(bx, by, c + (int(seed) & 0xFFFF) * 16)      # noqa: E731
        kind = hk(0)
        rough = np.where(kind < 0.12, np.floor(hk(1) * 4.0) * 0.01, 0.05 + 0.95 * hk(1)).astype(np.float32)
        rough = np.where(kind < 0.12, rough, np.clip(rough + 0.02 * (u[..., 0] - 0.5), 0.05, 1.0)).astype(np.float32)
        g[1][..., 3] = rough
        metal = np.where(kind < 0.12, 1.0, np.where(hk(2) < 0.5, 0.0, np.where(hk(2) < 0.7, 1.0, hk(3)))).astype(np.float32)
        for c in range(3):
            g[2][..., c] = np.clip(0.1 + 0.85 * hk(4 + c) + 0.06 * (u[..., 1 + c] - 0.5), 0.0, 1.0)
        g[2][..., 3] = metal
        em = hk(7) > 0.97
        for c in range(3):
            g[3][..., c] = np.where(em, hk(8 + c), 0.0)
        g[3][..., 3] = np.where(em, 1.0 + 4.0 * hk(11), 0.0)
        lo, hi = max(row0, ch * ROW_CHUNK), min(row1, (ch + 1) * ROW_CHUNK)
        for k in range(4):
            planes[k][lo - row0:hi - row0] = g[k][lo - ch * ROW_CHUNK:hi - ch * ROW_CHUNK].astype(np.float32)
    return planes


def point_lights(n, seed=0x1600):
    """n PointLight records: pos U([-50,50]x[0,20]x[-50,50]), colour U[0.2,1]^3, brightness U[100,1500], range U[20,200]."""
    r = np.random.Generator(np.random.Philox(key=[int(seed), 0x11]))
    arr = (abi.PointLight * n)()
    for i in range(n):
        u = r.random(8, dtype=np.float32)
        l = arr[i]
        l.position.set((-50 + 100 * u[0], 20 * u[1], -50 + 100 * u[2]))
        l.range = float(np.float32(20 + 180 * u[3]))
        l.color.set((0.2 + 0.8 * u[4], 0.2 + 0.8 * u[5], 0.2 + 0.8 * u[6]))
        l.brightness = float(np.float32(100 + 1400 * u[7]))
        l.attenuation.set((1.0, 0.0, 0.0))
        l.depthBias = 0.0
    return arr


def spot_lights(n, seed=0x5907):
    r = np.random.Generator(np.random.Philox(key=[int(seed), 0x22]))
    arr = (abi.SpotLight * n)()
    for i in range(n):
        u = r.random(12, dtype=np.float32)
        l = arr[i]
        l.position.set((-40 + 80 * u[0], 10 + 20 * u[1], -40 + 80 * u[2]))
        l.color.set((0.2 + 0.8 * u[3], 0.2 + 0.8 * u[4], 0.2 + 0.8 * u[5]))
        l.brightness = float(np.float32(500 + 1500 * u[6]))
        d = np.array([u[7] - 0.5, -1.0, u[8] - 0.5], np.float32)
        l.spotDir.set(d * 3.0)                       # deliberately not unit length: the shader normalises (Lighting.hlsl:60)
        outer = np.float32(np.deg2rad(20 + 25 * u[9]))
        l.outerConeAngle = float(outer)
        l.innerConeAngle = float(np.float32(outer * (0.6 + 0.3 * u[10])))
        l.depthBias = 5e-5
        l.range = 0.0                                # unset by the CPU side, Light.cpp:108-121
    return arr


def per_frame(points=None, spots=None, directional=None, ambient=0.055, hdri_offset=0.0):
    """PerFrameData with up to 100 point lights in the cbuffer array; returns (PerFrameData, extra PointLight array or None)."""
    pf = abi.PerFrameData()
    n = len(points) if points is not None else 0
    k = min(n, abi.NUM_LIGHTS__POINT)
    pf.Lights.numPointLights = k
    for i in range(k):
        pf.Lights.point_lights[i] = points[i]
    extra = None
    if n > k:
        extra = (abi.PointLight * (n - k))(*[points[i] for i in range(k, n)])
    if spots is not None:
        pf.Lights.numSpotLights = len(spots)
        for i in range(len(spots)):
            pf.Lights.spot_lights[i] = spots[i]
    if directional is not None:
        pf.Lights.directional = directional
    pf.f2PointLightShadowMapDimensions = abi.float2(1024.0, 1024.0)          # SceneRendering.cpp:439-441
    pf.f2SpotLightShadowMapDimensions = abi.float2(1024.0, 1024.0)
    pf.f2DirectionalLightShadowMapDimensions = abi.float2(2048.0, 2048.0)
    pf.fAmbientLightingFactor = ambient
    pf.fHDRIOffsetInRadians = hdri_offset
    return pf, extra


def per_view(width, height, camera=(0.0, 10.0, -60.0), max_env_lod=0, diffuse_only=0):
    pv = abi.PerViewLightingData()
    for m in (pv.matView, pv.matViewToWorld, pv.matProjInverse):
        for i in range(4):
            m.m[i][i] = 1.0
    pv.CameraPosition.set(camera)
    pv.MaxEnvMapLODLevels = float(max_env_lod)
    pv.ScreenDimensions = abi.float2(float(width), float(height))
    pv.EnvironmentMapDiffuseOnlyIllumination = diffuse_only
    return pv


def directional_light(direction=(0.3, -1.0, 0.2), color=(1.0, 0.95, 0.9), brightness=0.9, shadowing=0, enabled=1, depth_bias=5e-5):
    d = abi.DirectionalLight()
    d.lightDirection.set(direction)
    d.color.set(color)
    d.brightness = brightness
    d.depthBias = depth_bias
    d.shadowing = shadowing
    d.enabled = enabled
    return d


def equirect(width, height, seed=0xE9):
    """RGBA32F equirect [H,W,4]: smooth sky gradient + 8 Gaussian 'suns' with peak radiance up to 2.6e4."""
    r = np.random.Generator(np.random.Philox(key=[int(seed), 0x33]))
    v = (np.arange(height, dtype=np.float32) + 0.5) / height
    u = (np.arange(width, dtype=np.float32) + 0.5) / width
    uu, vv = np.meshgrid(u, v)
    sky = np.stack([0.25 + 0.35 * (1 - vv), 0.35 + 0.4 * (1 - vv), 0.55 + 0.45 * (1 - vv)], -1)
    ground = np.stack([0.18 + 0.05 * np.sin(12 * uu), 0.15 + 0.05 * np.cos(9 * uu), 0.10 + 0.0 * uu], -1)
    t = np.clip((vv - 0.5) * 8.0 + 0.5, 0, 1)[..., None]
    img = sky * (1 - t) + ground * t
    for _ in range(8):
        cu, cv = r.random(), 0.05 + 0.4 * r.random()
        sig = 0.004 + 0.02 * r.random()
        peak = 10 ** (1.5 + 2.9 * r.random())          # 30 .. 2.5e4
        col = 0.6 + 0.4 * r.random(3)
        du = np.minimum(np.abs(uu - cu), 1 - np.abs(uu - cu))
        img += (peak * np.exp(-(du * du + (vv - cv) ** 2) / (2 * sig * sig)))[..., None] * col
    out = np.empty((height, width, 4), np.float32)
    out[..., :3] = img.astype(np.float32)
    out[..., 3] = 1.0
    return out


def hdr_image(width, height, seed=0x70E, scale=4.0):
    """RGBA32F scene-colour-like image for blur/tonemap tests: log-uniform radiance with a few hot pixels."""
    r = np.random.Generator(np.random.Philox(key=[int(seed), 0x44]))
    img = np.exp(r.uniform(-6, np.log(scale), (height, width, 4))).astype(np.float32)
    hot = r.random((height, width)) > 0.999
    img[hot, :3] *= 500.0
    img[..., 3] = r.random((height, width), dtype=np.float32)
    return img


# ---- inputs of the G-buffer producer -------------------------------------------------------
def interpolants(width, height, n_materials, seed=0x1A7E):
    """PSInput planes (ForwardLighting.hlsl:42-53) of a synthetic view: a ground plane receding towards the top of the
    image (so the uv footprint — hence the mip level — grows with the row), material indices in 97x61-pixel blocks
    (odd sizes: pixel quads straddle material borders), a sky band of no-geometry pixels and a few stray / invalid indices.
    Returns 3 float32 arrays [H,W,4]: (P, u), (N, v), (T, asfloat(int32 index))."""
    r = np.random.Generator(np.random.Philox(key=[int(seed), 0x1F]))
    ys, xs = np.meshgrid(np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    t = (ys + 0.5) / height
    s = (xs + 0.5) / width
    z = (4.0 + 120.0 * (1.0 - t) ** 3).astype(np.float32)
    px = ((s - 0.5) * z * 1.4).astype(np.float32)
    py = (0.25 * np.sin(px * 0.7) * np.cos(z * 0.3)).astype(np.float32)
    ip0 = np.empty((height, width, 4), np.float32)
    ip1 = np.empty_like(ip0)
    ip2 = np.empty_like(ip0)
    ip0[..., 0], ip0[..., 1], ip0[..., 2] = px, py, z
    ip0[..., 3] = px * 0.37 + 0.11                      # uv.x
    ip1[..., 3] = z * 0.37 - 0.05                       # uv.y
    # interpolated (unnormalised) normal / tangent, deliberately not orthogonal
    ip1[..., 0] = 0.35 * np.sin(px * 1.3) + 0.02 * (r.random((height, width), dtype=np.float32) - 0.5)
    ip1[..., 1] = 1.3
    ip1[..., 2] = 0.35 * np.cos(z * 0.9) + 0.02 * (r.random((height, width), dtype=np.float32) - 0.5)
    ip2[..., 0] = 0.9
    ip2[..., 1] = 0.15 * np.sin(z * 0.5)
    ip2[..., 2] = 0.2 * np.cos(px * 0.4)
    bx, by = (xs.astype(np.int64) // 97), (ys.astype(np.int64) // 61)
    idx = ((bx * 5 + by * 3) % max(n_materials, 1)).astype(np.int32)
    idx[ys < height * 0.08] = -1                        # sky
    stray = r.random((height, width)) > 0.9995
    idx[stray] = np.where(r.random(int(stray.sum())) > 0.5, -7, n_materials + 3).astype(np.int32)
    ip2[..., 3] = idx.view(np.float32)
    return ip0, ip1, ip2


def clip_positions(width, height, seed=0x5C11):
    """PSInput.svPositionCurr / svPositionPrev (ForwardLighting.hlsl:49-52) of a synthetic view: clip-space positions whose xy / w land near the pixel's NDC
    position, w = view depth in [0.3, 120] growing towards the top of the image like synth.interpolants; the previous frame is the same geometry under a
    slightly different camera (a few pixels of motion, more for near geometry). Two float32 arrays [H,W,4]."""
    r = np.random.Generator(np.random.Philox(key=[int(seed), 0x2B]))
    ys, xs = np.meshgrid(np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    t, s = (ys + 0.5) / height, (xs + 0.5) / width
    w = (0.3 + 120.0 * (1.0 - t) ** 3).astype(np.float32)
    cur = np.empty((height, width, 4), np.float32)
    cur[..., 0] = (2.0 * s - 1.0) * w
    cur[..., 1] = (1.0 - 2.0 * t) * w
    cur[..., 2] = w - 0.1
    cur[..., 3] = w
    prev = cur.copy()
    prev[..., 0] += np.float32(0.03) + 0.002 * (r.random((height, width), dtype=np.float32) - 0.5)
    prev[..., 1] -= np.float32(0.011) + 0.002 * (r.random((height, width), dtype=np.float32) - 0.5)
    prev[..., 3] *= np.float32(1.004)
    return cur, prev


def material_set(n, seed=0x3A7, max_dim=256, same_size=False):
    """n materials: (list of abi.MaterialData, list of {slot: uint8 [H,W,4] level 0}) with power-of-two texture sizes
    (non-square allowed), random scalar parameters and uv tiling. textureConfig normally mirrors the bound maps
    (Material::GetTextureConfig, Material.cpp:23-36); materials 3k+1 carry a deliberately inconsistent config (bit set
    without a map / map without its bit) to exercise the null-SRV and ignored-map branches."""
    r = np.random.Generator(np.random.Philox(key=[int(seed), 0x77]))
    bits = {"texDiffuse": 0, "texNormals": 1, "texLocalAO": 2, "texRoughness": 4, "texMetalness": 5, "texEmissive": 7, "texOcclRoughMetal": 8}
    datas, texsets = [], []
    for i in range(n):
        d = abi.MaterialData()
        d.diffuse.set(tuple(r.uniform(0.2, 1.0, 3))); d.alpha = 1.0
        d.emissiveColor.set(tuple(r.uniform(0.0, 1.0, 3))); d.emissiveIntensity = float(r.uniform(0, 3)) if i % 3 == 0 else 0.0
        d.specular.set((1.0, 1.0, 1.0)); d.normalMapMipBias = float(r.choice([0.0, -0.5, 0.75, 1.0]))
        d.uvScaleOffset = abi.float4(float(r.uniform(0.3, 6.0)), float(r.uniform(0.3, 6.0)), float(r.uniform(-1, 1)), float(r.uniform(-1, 1)))
        d.roughness, d.metalness, d.displacement = float(r.uniform(0.05, 1.0)), float(r.uniform(0, 1)), 0.0
        texs, cfg = {}, 0
        if same_size:                                   # one square size per material (how material sets are normally authored)
            mw = mh = int(2 ** r.integers(max(3, int(np.log2(max_dim)) - 1), int(np.log2(max_dim)) + 1))
        for slot in abi.MATERIAL_TEXTURE_SLOTS:
            if i == 0 or r.random() < 0.6:              # material 0 binds every map
                w = int(2 ** r.integers(3, int(np.log2(max_dim)) + 1)); h = int(2 ** r.integers(3, int(np.log2(max_dim)) + 1))
                if same_size:
                    w, h = mw, mh
                yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
                img = np.empty((h, w, 4), np.float32)
                for c in range(4):
                    fx, fy, ph = r.integers(1, 5), r.integers(1, 5), r.uniform(0, 6.28)
                    img[..., c] = 0.5 + 0.35 * np.sin(2 * np.pi * (fx * xx / w + fy * yy / h) + ph) + 0.15 * (r.random((h, w)) - 0.5)
                if slot == "texNormals":                # mostly +Z tangent-space normals
                    img[..., 2] = 0.75 + 0.25 * img[..., 2]
                    if i % 4 == 2:
                        img[: h // 2] = 0.0            # a region of all-zero normals: the length(Normal) < 0.01 branch
                texs[slot] = np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)
                cfg |= 1 << bits[slot]
        if i % 3 == 1:
            cfg ^= (1 << 0) | (1 << 4) | (1 << 8)
        d.textureConfig = float(cfg)
        datas.append(d)
        texsets.append(texs)
    return datas, texsets


def ssao_image(width, height, seed=0x55A0):
    r = np.random.Generator(np.random.Philox(key=[int(seed), 0x0A]))
    return r.integers(96, 256, (height, width), dtype=np.uint8)


# ---- Radiance .hdr files (the reference's HDRI assets, Data/EnvironmentMaps.ini) ----------------
def float_to_rgbe(rgb):
    """float [...,3] -> uint8 [...,4] RGBE (Ward's float2rgbe: mantissas scaled by 256/2^e of the largest channel)."""
    rgb = np.asarray(rgb, np.float64)
    v = rgb.max(-1)
    out = np.zeros(rgb.shape[:-1] + (4,), np.uint8)
    ok = v >= 1e-32
    m, e = np.frexp(np.where(ok, v, 1.0))
    scale = np.where(ok, m * 256.0 / np.where(ok, v, 1.0), 0.0)[..., None]
    out[..., :3] = np.clip(np.floor(rgb * scale), 0, 255).astype(np.uint8)
    out[..., 3] = np.where(ok, e + 128, 0).astype(np.uint8)
    out[~ok] = 0
    return out


def _rle_plane(row):
    """New-style Radiance run-length coding of one byte plane of a scanline: runs of >= 4 equal bytes, else literals <= 128."""
    out = bytearray()
    n, i = len(row), 0
    while i < n:
        run = 1
        while i + run < n and run < 127 and row[i + run] == row[i]:
            run += 1
        if run >= 4:
            out += bytes((128 + run, int(row[i])))
            i += run
            continue
        j = i
        while j < n and j - i < 128:
            r = 1
            while j + r < n and r < 4 and row[j + r] == row[j]:
                r += 1
            if r >= 4:
                break
            j += 1
        out += bytes((j - i,)) + bytes(int(b) for b in row[i:j])
        i = j
    return bytes(out)


def hdr_file_bytes(rgbe, rle=True, magic=b"#?RADIANCE", extra_header=(b"# synthetic", b"EXPOSURE=1.0")):
    """A complete .hdr file for the uint8 [H,W,4] RGBE image: header + run-length coded (or flat) scanlines."""
    h, w = rgbe.shape[:2]
    head = magic + b"\n" + b"".join(l + b"\n" for l in extra_header) + b"FORMAT=32-bit_rle_rgbe\n\n" + b"-Y %d +X %d\n" % (h, w)
    if not rle or w < 8 or w >= 32768:
        return head + np.ascontiguousarray(rgbe).tobytes()
    body = bytearray()
    for y in range(h):
        body += bytes((2, 2, w >> 8, w & 255))
        for k in range(4):
            body += _rle_plane(rgbe[y, :, k])
    return head + bytes(body)


# ---- SSR environment fallback: the inputs of ClassifyReflectionTiles.hlsl ---------------------------------------
def _look_at_lh(eye, at, up):
    """DirectX::XMMatrixLookAtLH: row-major, row-vector convention (float64)."""
    eye, at, up = (np.asarray(v, np.float64) for v in (eye, at, up))
    z = at - eye
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = x, y, z
    m[3, :3] = [-x @ eye, -y @ eye, -z @ eye]
    return m


def _perspective_fov_lh(fov_y, aspect, zn, zf):
    """DirectX::XMMatrixPerspectiveFovLH (float64)."""
    h = 1.0 / np.tan(0.5 * fov_y)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1], m[2, 2], m[2, 3], m[3, 2] = h / aspect, h, zf / (zf - zn), 1.0, -zn * zf / (zf - zn)
    return m


def _set_matrix(dst, m):
    for i in range(4):
        for j in range(4):
            dst.m[i][j] = float(np.float32(m[i, j]))


def ssr_constants(width, height, spec_mips, hdri_yaw=0.3, roughness_threshold=0.2, camera=(3.0, 10.0, -60.0), look_at=(0.0, 2.0, 0.0)):
    """FFX_SSSRConstants as VQRenderer::RenderReflections fills it (SceneRendering.cpp:2221-2242) for a LookAtLH / PerspectiveFovLH camera;
    envMapRotation == GetHDRIRotationMatrix (:2185-2195: float cos / sin of -yaw)."""
    cb = abi.SSSRConstants()
    view = _look_at_lh(camera, look_at, (0.0, 1.0, 0.0))
    proj = _perspective_fov_lh(np.pi / 3.0, width / height, 0.1, 1500.0)
    _set_matrix(cb.view, view)
    _set_matrix(cb.invView, np.linalg.inv(view))
    _set_matrix(cb.projection, proj)
    _set_matrix(cb.invProjection, np.linalg.inv(proj))
    _set_matrix(cb.invViewProjection, np.linalg.inv(view @ proj))
    _set_matrix(cb.prevViewProjection, view @ proj)
    c, s = float(np.cos(np.float32(-hdri_yaw), dtype=np.float32)), float(np.sin(np.float32(-hdri_yaw), dtype=np.float32))
    rot = np.zeros((4, 4))
    rot[0, :3], rot[1, :3], rot[2, :3] = [c, 0, s], [0, 1, 0], [-s, 0, c]
    _set_matrix(cb.envMapRotation, rot)
    cb.bufferDimensions[0], cb.bufferDimensions[1] = width, height
    cb.inverseBufferDimensions[0], cb.inverseBufferDimensions[1] = float(np.float32(1.0) / np.float32(width)), float(np.float32(1.0) / np.float32(height))
    cb.temporalStabilityFactor, cb.depthBufferThickness, cb.roughnessThreshold, cb.varianceThreshold = 0.7, 0.015, roughness_threshold, 0.0
    cb.maxTraversalIntersections, cb.minTraversalOccupancy, cb.mostDetailedMip, cb.samplesPerQuad = 128, 4, 0, 1
    cb.envMapSpecularIrradianceCubemapMipLevelCount = spec_mips
    return cb


def ssr_surfaces(width, height, seed=0x55E7, sky_fraction=0.1):
    """(scene colour float32 [H,W,4] with the roughness in alpha, NDC depth float32 [H,W], normals as R10G10B10A2_UNORM uint32 [H,W] and as the decoded
    float32 [H,W,4] values): white-noise surfaces — roughness U[0,1] (a fifth below the 0.2 ray threshold), unit normals on the whole sphere encoded
    n * 0.5 + 0.5 and quantised to 10 bits, depth U[0.9, 1) with `sky_fraction` of the pixels on the far plane (1.0)."""
    r = _chunk_rng(seed, 0)
    scene = r.random((height, width, 4), dtype=np.float32) * np.array([4.0, 4.0, 4.0, 1.0], np.float32)
    depth = (0.9 + 0.0999 * r.random((height, width), dtype=np.float32)).astype(np.float32)
    depth[r.random((height, width), dtype=np.float32) < sky_fraction] = 1.0
    n = r.normal(size=(height, width, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    q = np.clip(np.floor((n * 0.5 + 0.5) * 1023.0 + 0.5), 0, 1023).astype(np.uint32)
    packed = (q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (np.uint32(3) << 30)).astype(np.uint32)
    n01 = np.concatenate([q.astype(np.float32) / np.float32(1023.0), np.ones((height, width, 1), np.float32)], axis=-1)
    return scene, depth, packed, n01


def _matrix_of(m):
    return np.array([[m.m[i][j] for j in range(4)] for i in range(4)], np.float64)


def ssr_room(width, height, spec_mips=1, seed=0x5500A, **constants):
    """A deterministic scene that SSR rays can actually hit, for vqhip_ssr_classify / vqhip_ssr_intersect: a floor (y = 0), a back wall and two side walls of a room
    open to the sky, and a few axis-aligned boxes standing on the floor, ray-cast (float64) through the pixel centres of the LookAtLH / PerspectiveFovLH camera whose
    matrices ssr_constants(width, height, spec_mips, **constants) fills. Returns a dict:
      cb      abi.SSSRConstants (ssr_constants)
      depth   float32 [H,W]   NDC z in [0, 1) of the nearest surface, sky = 1
      packed  uint32 [H,W]    face normals, n * 0.5 + 0.5 quantised to R10G10B10A2_UNORM;   n01 float32 [H,W,4]: the decoded values
      scene   float32 [H,W,4] the lit scene; alpha = roughness: the floor in world-space stripes of mirror (0.02), glossy (0.06 .. 0.16) and rough (0.6) bands, the back
              wall glossy, the side walls rough, the boxes mirror / glossy / rough in turn; sky pixels 0.9
      noise   uint8 [128,128,2] a seeded stand-in for g_blue_noise_texture (white, not blue: the contract only needs two UNORM8 numbers per pixel)"""
    cb = ssr_constants(width, height, spec_mips, **constants)
    view, proj = _matrix_of(cb.view), _matrix_of(cb.projection)
    inv_view = np.linalg.inv(view)
    eye = inv_view[3, :3]
    xs = (np.arange(width) + 0.5) / width * 2.0 - 1.0
    ys = 1.0 - (np.arange(height) + 0.5) / height * 2.0
    dv = np.stack(np.broadcast_arrays(xs[None, :] / proj[0, 0], ys[:, None] / proj[1, 1], 1.0), -1)          # view-space direction with z = 1
    d = dv @ inv_view[:3, :3]                                                                                  # row vectors
    big = 1e30
    t_best = np.full((height, width), big)
    nrm = np.zeros((height, width, 3))
    obj = np.full((height, width), -1, np.int64)

    def plane(axis, value, normal, lo, hi, ident):
        nonlocal t_best, nrm, obj
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (value - eye[axis]) / d[..., axis]
        p = eye + t[..., None] * d
        ok = (t > 0) & (t < t_best) & np.isfinite(t)
        for a in range(3):
            if a != axis:
                ok &= (p[..., a] >= lo[a]) & (p[..., a] <= hi[a])
        t_best = np.where(ok, t, t_best)
        nrm[ok] = normal
        obj[ok] = ident

    plane(1, 0.0, (0, 1, 0), (-45, 0, -90), (45, 0, 40), 0)          # floor
    plane(2, 40.0, (0, 0, -1), (-45, 0, 0), (45, 32, 0), 1)          # back wall
    plane(0, -45.0, (1, 0, 0), (0, 0, -90), (0, 32, 40), 2)          # side walls
    plane(0, 45.0, (-1, 0, 0), (0, 0, -90), (0, 32, 40), 3)
    boxes = [((-30, 0, 5), (-18, 14, 17)), ((-8, 0, -12), (4, 9, -2)), ((12, 0, 8), (26, 20, 22)), ((20, 0, -30), (28, 6, -22)), ((-26, 0, -34), (-16, 11, -26))]
    for k, (lo, hi) in enumerate(boxes):
        for axis in range(3):
            for value, sgn in ((lo[axis], -1.0), (hi[axis], 1.0)):
                n = [0.0, 0.0, 0.0]
                n[axis] = sgn
                plane(axis, float(value), tuple(n), lo, hi, 4 + k)
    hit = obj >= 0
    p = eye + np.where(hit, t_best, 1.0)[..., None] * d
    pv = np.concatenate([p, np.ones((height, width, 1))], -1) @ view @ proj
    depth = np.where(hit, pv[..., 2] / pv[..., 3], 1.0).astype(np.float32)
    depth = np.where(hit, np.minimum(depth, np.nextafter(np.float32(1), np.float32(0))), np.float32(1.0)).astype(np.float32)
    n = np.where(hit[..., None], nrm, [0.0, 0.0, -1.0])
    q = np.clip(np.floor((n * 0.5 + 0.5) * 1023.0 + 0.5), 0, 1023).astype(np.uint32)
    packed = (q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (np.uint32(3) << 30)).astype(np.uint32)
    n01 = np.concatenate([q.astype(np.float32) / np.float32(1023.0), np.ones((height, width, 1), np.float32)], axis=-1)
    stripe = np.floor((p[..., 0] + 45.0) / 7.5).astype(np.int64) % 6
    floor_rough = np.array([0.02, 0.06, 0.6, 0.1, 0.02, 0.16])[stripe]
    box_rough = np.array([0.02, 0.12, 0.5, 0.08, 0.02])
    rough = np.full((height, width), 0.9)
    rough = np.where(obj == 0, floor_rough, rough)
    rough = np.where(obj == 1, 0.1, rough)
    rough = np.where((obj == 2) | (obj == 3), 0.45, rough)
    for k in range(len(boxes)):
        rough = np.where(obj == 4 + k, box_rough[k], rough)
    palette = np.array([[0.35, 0.33, 0.30], [0.9, 0.55, 0.2], [0.2, 0.5, 0.9], [0.3, 0.8, 0.4], [2.5, 0.4, 0.3], [0.3, 2.0, 0.6], [0.4, 0.5, 3.0], [1.5, 1.4, 0.2], [0.9, 0.2, 1.6]])
    shade = 0.6 + 0.4 * np.sin(0.35 * p[..., 0]) * np.cos(0.27 * p[..., 1] + 0.19 * p[..., 2])
    rgb = np.where(hit[..., None], palette[np.clip(obj, 0, len(palette) - 1)] * shade[..., None], [0.6, 0.7, 1.1])
    scene = np.concatenate([rgb, rough[..., None]], -1).astype(np.float32)
    noise = _chunk_rng(seed, 0).integers(0, 256, (abi.SSR_BLUE_NOISE_SIZE, abi.SSR_BLUE_NOISE_SIZE, 2), dtype=np.uint8)
    return {"cb": cb, "depth": depth, "packed": packed, "n01": n01, "scene": scene, "noise": noise}


def gbuffer_msaa(width, height, layers=2, split_fraction=0.05, seed=0x4A4A, mode="edges"):
    """Fragment layers of a 4x MSAA frame for vqhip_forward_lighting_msaa: (list of `layers` G-buffers as from gbuffer(), list of uint8 [H,W]
    coverage planes). mode "edges": layer 0 is gbuffer(width, height, seed); the others are other records. Random discs and triangles
    (straight edges), each given one of the layers, are painted over layer 0 and evaluated at D3D's standard 4x sample positions
    (abi.MSAA_SAMPLE_POSITIONS): the masks are disjoint and leave no gap, and shapes are added until about `split_fraction` of the
    pixels have samples of more than one layer (0: every mask of layer 0 is 0xF). mode "random": arbitrary coverage bytes."""
    if not 1 <= layers <= abi.MSAA_MAX_LAYERS:
        raise ValueError("layers must be 1..4")
    gbs = [gbuffer(width, height, seed=seed if k == 0 else (seed + 0x9E37 * k) & 0xFFFFFFFF) for k in range(layers)]
    rng = np.random.default_rng(seed)
    if mode == "random":
        return gbs, [rng.integers(0, 256, (height, width), dtype=np.uint8) for _ in range(layers)]
    if mode != "edges":
        raise ValueError(f"unknown mode {mode!r}")
    ids = np.zeros((height, width, 4), np.int8)                         # layer of each sample
    split = np.zeros((height, width), bool)
    n_split = 0
    target = split_fraction * width * height
    if layers > 1 and split_fraction > 0:
        pos = np.array(abi.MSAA_SAMPLE_POSITIONS, np.float64) / 16.0
        # shape size: about 200 shapes reach the target (a boundary of length l splits about l pixels), small enough for the
        # fraction (the boundaries of overlapping shapes saturate near 0.8 / radius); a bounded number of tries
        size = max(1.5, min(16.0, 0.5 / split_fraction, target / (200 * 2 * np.pi)))
        for _ in range(200000):
            if n_split >= target:
                break
            cx, cy = rng.uniform(0, width), rng.uniform(0, height)
            r = size * rng.uniform(0.5, 1.5)
            x0, x1 = max(0, int(cx - r) - 1), min(width, int(cx + r) + 2)
            y0, y1 = max(0, int(cy - r) - 1), min(height, int(cy + r) + 2)
            if x0 >= x1 or y0 >= y1:
                continue
            sx = (np.arange(x0, x1) + 0.5)[None, :, None] + pos[None, None, :, 0]
            sy = (np.arange(y0, y1) + 0.5)[:, None, None] + pos[None, None, :, 1]
            sx, sy = np.broadcast_arrays(sx, sy)
            if rng.random() < 0.5:                                      # disc
                inside = (sx - cx) ** 2 + (sy - cy) ** 2 < r * r
            else:                                                       # triangle: three straight edges
                a = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.4, 0.4, 3)
                vx, vy = cx + r * np.cos(a), cy + r * np.sin(a)
                inside = np.ones(sx.shape, bool)
                for i in range(3):
                    j = (i + 1) % 3
                    inside &= (vx[j] - vx[i]) * (sy - vy[i]) - (vy[j] - vy[i]) * (sx - vx[i]) > 0
            blk = ids[y0:y1, x0:x1]
            blk[inside] = rng.integers(0, layers)
            now = (blk != blk[..., :1]).any(-1)
            n_split += int(now.sum()) - int(split[y0:y1, x0:x1].sum())
            split[y0:y1, x0:x1] = now
    cov = [np.zeros((height, width), np.uint8) for _ in range(layers)]
    for s in range(4):
        for k in range(layers):
            cov[k] |= ((ids[..., s] == k).astype(np.uint8) << s)
    return gbs, cov


def depth_msaa(width, height, coverage, seed=0xD397, plant=False):
    """Per-sample NDC depth float32 [H,W,4] consistent with the masks of gbuffer_msaa: every layer is a smooth depth field (a tilted plane with a
    ripple) evaluated at D3D's 4x sample positions, so samples of one layer differ by the field's slope; nearer layers (lower index) are nearer; a sample
    no layer owns holds the clear value 1.0. plant=True additionally plants, in seeded pixels, exact ties between samples (pairs, triples, all four equal)
    and the exact values 0.0 and 1.0 on owned samples."""
    layers = len(coverage)
    rng = np.random.default_rng(seed)
    pos = np.array(abi.MSAA_SAMPLE_POSITIONS, np.float64) / 16.0
    sx = (np.arange(width) + 0.5)[None, :, None] + pos[None, None, :, 0]
    sy = (np.arange(height) + 0.5)[:, None, None] + pos[None, None, :, 1]
    depth = np.ones((height, width, 4), np.float32)
    taken = np.zeros((height, width, 4), bool)
    for k in range(layers):
        gx, gy = rng.uniform(-0.04, 0.04, 2) / max(width, height)
        ph, fr = rng.uniform(0, 2 * np.pi), rng.uniform(0.02, 0.08)
        lo = 0.05 + 0.9 * k / layers                                           # layer k lies in [lo, lo + 0.9 / layers): nearer layers nearer
        f = 0.5 + gx * (sx - width / 2) + gy * (sy - height / 2) + 0.2 * np.sin(fr * sx + ph) * np.cos(fr * sy)
        d = (lo + (0.9 / layers) * np.clip(0.5 + 0.6 * (f - 0.5), 0.0, 0.999)).astype(np.float32)
        mine = (((coverage[k][..., None] >> np.arange(4)) & 1) != 0) & ~taken
        depth[mine] = d[mine]
        taken |= mine
    if plant:
        n = min(max(8, width * height // 16), 20000)
        ys, xs = rng.integers(0, height, n), rng.integers(0, width, n)
        kind = rng.integers(0, 6, n)
        for y, x, c in zip(ys, xs, kind):
            px = depth[y, x]
            if c == 0:
                px[1] = px[0]
            elif c == 1:
                px[3] = px[2] = px[1]
            elif c == 2:
                px[:] = px[rng.integers(0, 4)]
            elif c == 3:
                px[rng.integers(0, 4)] = 0.0
            elif c == 4:
                px[rng.integers(0, 4)] = 1.0
            else:
                px[[0, 2]] = px[[0, 2]].min()
    return depth


def packed_unit_normals(shape, seed=0x9A11):
    """Random unit vectors encoded n * 0.5 + 0.5 and packed to R10G10B10A2_UNORM words (alpha 3), uint32 of `shape` — per-layer pre-pass normals"""
    r = np.random.default_rng(seed)
    n = r.normal(size=tuple(shape) + (3,))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    q = np.clip(np.floor((n * 0.5 + 0.5) * 1023.0 + 0.5), 0, 1023).astype(np.uint32)
    return (q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (np.uint32(3) << 30)).astype(np.uint32)


def encode_r11g11b10(rgb):
    """float [..., 3] (>= 0, or +inf) -> DXGI R11G11B10_FLOAT words uint32 [...]: each channel through binary16 (round to nearest even), the mantissa then cut to
    6 / 6 / 5 bits — one valid encoder; the library only decodes the format"""
    with np.errstate(over="ignore"):
        hb = np.maximum(np.asarray(rgb, np.float32), np.float32(0)).astype(np.float16).view(np.uint16).astype(np.uint32)
    return ((hb[..., 0] >> 4) | ((hb[..., 1] >> 4) << 11) | ((hb[..., 2] >> 5) << 22)).astype(np.uint32)


def ssr_denoise_planes(width, height, seed=0xD6E0, radiance=None, history_amplitude=0.6, average_amplitude=0.25, zero_variance_fraction=0.15):
    """Stand-ins for the planes the denoiser's Reproject pass hands to vqhip_ssr_prefilter / vqhip_ssr_resolve_temporal, seeded. radiance: None = white noise
    U[0, 4) float32 [H,W,4] (alpha a ray length), or the traced radiance to build the other planes around. Returns a dict:
      radiance     float32 [H,W,4]
      variance     float16 [H,W]    U[0, 0.5), `zero_variance_fraction` of the pixels exactly 0 (those are copied by the prefilter)
      sample_count float16 [H,W]    integers 0 .. 32, a tenth of them 0 and a tenth 1
      reprojected  float32 [H,W,4]  radiance * (1 + history_amplitude * U[-1, 1)) per channel: part of it inside the clip box, part outside
      average      float32 [H8,W8,4] the 8 x 8 block mean of the radiance (partial blocks over their pixels) * (1 + average_amplitude * U[-1, 1)), alpha 0
      average_r11  uint32 [H8,W8]   the same texture encoded R11G11B10_FLOAT (encode_r11g11b10)
      roughness8   uint8 [H,W]      R8_UNORM roughness: 15 % mirror (< 0.04), 60 % glossy below the 0.2 threshold, 25 % rough"""
    r = _chunk_rng(seed, 0)
    h, w = height, width
    if radiance is None:
        radiance = r.random((h, w, 4), dtype=np.float32) * np.float32(4.0)
    rad = np.asarray(radiance).astype(np.float32)
    variance = (r.random((h, w), dtype=np.float32) * np.float32(0.5)).astype(np.float16)
    variance[r.random((h, w), dtype=np.float32) < zero_variance_fraction] = 0
    pick = r.random((h, w), dtype=np.float32)
    count = np.where(pick < 0.1, 0, np.where(pick < 0.2, 1, r.integers(2, 33, (h, w)))).astype(np.float16)
    rep = rad.copy()
    rep[..., :3] *= (1.0 + history_amplitude * (2.0 * r.random((h, w, 3), dtype=np.float32) - 1.0)).astype(np.float32)
    h8, w8 = (h + 7) // 8, (w + 7) // 8
    pad = np.zeros((h8 * 8, w8 * 8, 3), np.float64)
    cnt = np.zeros((h8 * 8, w8 * 8, 1), np.float64)
    pad[:h, :w], cnt[:h, :w] = np.where(np.isfinite(rad[..., :3]), rad[..., :3], 0.0), 1.0
    mean = pad.reshape(h8, 8, w8, 8, 3).sum((1, 3)) / cnt.reshape(h8, 8, w8, 8, 1).sum((1, 3))
    avg = np.zeros((h8, w8, 4), np.float32)
    avg[..., :3] = (mean * (1.0 + average_amplitude * (2.0 * r.random((h8, w8, 3)) - 1.0))).astype(np.float32)
    kind = r.random((h, w), dtype=np.float32)
    rough = np.where(kind < 0.15, r.integers(0, 11, (h, w)), np.where(kind < 0.75, r.integers(11, 51, (h, w)), r.integers(51, 256, (h, w)))).astype(np.uint8)
    return {"radiance": rad, "variance": variance, "sample_count": count, "reprojected": rep, "average": avg, "average_r11": encode_r11g11b10(avg[..., :3]),
            "roughness8": rough}


def ssr_smooth_surfaces(width, height, seed=0x5A00):
    """(NDC depth float32 [H,W], normals as R10G10B10A2_UNORM uint32 [H,W], decoded float32 [H,W,4]) of one gently curved surface: normals within a few degrees of
    one direction, depth a shallow ramp — neighbouring pixels pass the prefilter's pow(dot, 512) and depth weights, so all 15 taps of a pixel carry weight (on
    ssr_surfaces' white noise nearly every tap's weight vanishes)"""
    r = _chunk_rng(seed, 0)
    ys, xs = np.mgrid[0:height, 0:width]
    n = np.array([0.2, 0.9, -0.4])[None, None, :] + 0.02 * r.normal(size=(height, width, 3)) + 0.03 * np.stack([np.sin(0.3 * xs), np.cos(0.2 * ys), np.sin(0.1 * (xs + ys))], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    q = np.clip(np.floor((n * 0.5 + 0.5) * 1023.0 + 0.5), 0, 1023).astype(np.uint32)
    packed = (q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (np.uint32(3) << 30)).astype(np.uint32)
    n01 = np.concatenate([q.astype(np.float32) / np.float32(1023.0), np.ones((height, width, 1), np.float32)], axis=-1)
    depth = (0.5 + 0.02 * (xs + 2.0 * ys) / (width + 2.0 * height) + 0.002 * r.random((height, width))).astype(np.float32)
    return depth, packed, n01


def _pack_normals(n):
    q = np.clip(np.floor((n * 0.5 + 0.5) * 1023.0 + 0.5), 0, 1023).astype(np.uint32)
    packed = (q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (np.uint32(3) << 30)).astype(np.uint32)
    return packed, np.concatenate([q.astype(np.float32) / np.float32(1023.0), np.ones(n.shape[:2] + (1,), np.float32)], axis=-1)


def ssr_reproject_frames(width, height, seed=0x4E90):
    """A designed pair of frames for vqhip_ssr_reproject (docs/DESIGN_DETAILS.md §7.13): the current frame and the history the previous one left, with a camera that
    moved in between (cb.prevViewProjection is the previous camera's). Column bands, left to right:
      A  x < 0.30 w          flat near-mirror (roughness 5 / 255), identical normals, no motion: the hit-point reprojection wins and the early-out is taken
      B  0.30 w .. 0.55 w    glossy, normals perturbed by a few degrees, moved one pixel per frame; the history is the current frame shifted: surface reprojection accepted
      C  0.55 w .. 0.70 w    upper half: as B with the history radiance far from the local mean: discarded. lower half: white-noise normals that differ between the
                             frames and a depth step: the 3 x 3 search and the 2 x 2 path
      E  0.70 w .. 0.82 w    as B with motion vectors of 3 (1.5 in uv): the surface uv leaves [0, 1] and is sampled clamped
      F  x >= 0.82 w         rough (>= 0.6): not glossy
    A frame whose size is no multiple of 8 has partial tiles on its right and bottom edges. Returns a dict: cb; depth, depth_hist float32 [H,W]; packed, packed_hist uint32
    [H,W] with n01, n01_hist float32 [H,W,4]; roughness8, roughness8_hist uint8 [H,W]; radiance (alpha = ray length), radiance_hist float32 [H,W,4]; motion float32
    [H,W,2]; variance_hist, sample_count_hist float16 [H,W]."""
    r = _chunk_rng(seed, 0)
    h, w = height, width
    cb = ssr_constants(w, h, 1)
    prev = ssr_constants(w, h, 1, camera=(3.2, 10.0, -59.9))
    _set_matrix(cb.prevViewProjection, _matrix_of(prev.view) @ _matrix_of(prev.projection))
    ys, xs = np.mgrid[0:h, 0:w]
    band = np.digitize(xs / w, [0.30, 0.55, 0.70, 0.82])                          # 0 A, 1 B, 2 C, 3 E, 4 F
    lower = ys >= h // 2
    edges = (band == 2) & lower
    depth = (0.990 + 0.004 * (xs + 2.0 * ys) / (w + 2.0 * h) + 0.0002 * r.random((h, w))).astype(np.float32)           # 10 .. 17 units from the camera
    depth = np.where(edges & ((xs + ys) % 7 < 3), depth + np.float32(0.005), depth).astype(np.float32)
    base = np.array([0.2, 0.9, -0.4])
    n = base[None, None, :] + np.where((band == 0)[..., None], 0.0, 0.06 * r.normal(size=(h, w, 3)))
    wild = r.normal(size=(h, w, 3))
    n = np.where(edges[..., None], wild, n)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    packed, n01 = _pack_normals(n)
    rough = np.select([band == 0, band == 4], [5, r.integers(153, 256, (h, w))], r.integers(20, 31, (h, w))).astype(np.uint8)
    colour = np.array([1.2, 0.8, 0.5], np.float32)
    rad = np.empty((h, w, 4), np.float32)
    rad[..., :3] = colour * (0.6 + 0.8 * r.random((h, w, 3), dtype=np.float32))
    rad[..., 3] = 4.0 * r.random((h, w), dtype=np.float32)
    dx = np.where(band == 0, 0, 1)                                                # pixels per frame; band E's vectors are overwritten below
    motion = np.zeros((h, w, 2), np.float32)
    motion[..., 0] = (2.0 * dx / w).astype(np.float32)
    motion[band == 3] = (3.0, -0.5)

    def shifted(a):                                                               # history[y, x - 1] = current[y, x] where the surface moved
        return np.where((dx > 0).reshape(dx.shape + (1,) * (a.ndim - 2)), np.roll(a, -1, axis=1), a)
    depth_hist = shifted(depth)
    n_hist = shifted(n)
    other = r.normal(size=(h, w, 3))
    n_hist = np.where(edges[..., None], other / np.linalg.norm(other, axis=-1, keepdims=True), n_hist)
    packed_hist, n01_hist = _pack_normals(n_hist)
    rough_hist = shifted(rough)
    rad_hist = np.empty((h, w, 4), np.float32)
    rad_hist[..., :3] = colour * (0.95 + 0.1 * r.random((h, w, 3), dtype=np.float32))
    rad_hist[..., 3] = 0.0
    rad_hist[(band == 2) & ~lower, :3] += np.float32(4.0)
    variance_hist = (r.random((h, w), dtype=np.float32) * np.float32(0.5)).astype(np.float16)
    count_hist = r.integers(0, 33, (h, w)).astype(np.float16)
    return {"cb": cb, "depth": depth, "depth_hist": depth_hist, "packed": packed, "n01": n01, "packed_hist": packed_hist, "n01_hist": n01_hist,
            "roughness8": rough, "roughness8_hist": rough_hist, "radiance": rad, "radiance_hist": rad_hist, "motion": motion,
            "variance_hist": variance_hist, "sample_count_hist": count_hist}


def ssr_reproject_threshold_frames():
    """16 x 16 frames for vqhip_ssr_reproject in which every glossy pixel's disocclusion factor is EXACTLY 0.9 (word 3f666666), in both arithmetic readings: RGBA32F
    normals, the pixel's own (0, 1, 0) exactly, the history's normalize((2 hx - 1, 1, 0)) with hx the word 3f34ae3a — then dot(n, hn) is hn.y and
    exp((-|1 - hn.y|) * 1.4) rounds to 0.9 under the contract's exp; no motion, a camera that did not move, one depth everywhere (the depth term is exp(-0) = 1) and the
    history radiance within the local variance (surface reprojection is accepted; the hit candidate fails the 0.9999 similarity). 0.9 is neither > 0.9 nor < 0.9:
    no early-out, no search, no 2 x 2 path, the history is kept. The 8 x 8 pixels in the middle are glossy (their 9 x 9 neighbourhoods lie inside the frame), the rest rough. Same dict as ssr_reproject_frames."""
    w = h = 16
    f = ssr_reproject_frames(w, h, seed=0x0909)
    rng = np.random.default_rng(0x0909)
    f["cb"].prevViewProjection = ssr_constants(w, h, 1).prevViewProjection
    f["roughness8"][:] = 200
    f["roughness8"][4:12, 4:12] = 25
    f["roughness8_hist"][:] = 25
    f["motion"][:] = 0
    f["depth"][:] = 0.99
    f["depth_hist"][:] = 0.99
    f["radiance"][..., :3] = 1.0 + 0.6 * (rng.random((h, w, 3), dtype=np.float32) - 0.5)
    f["radiance"][..., 3] = 0.0
    f["radiance_hist"][..., :3] = 1.0
    f["n01"][..., :3] = (0.5, 1.0, 0.5)
    f["n01_hist"][..., :3] = (np.array([0x3F34AE3A], np.uint32).view(np.float32)[0], 1.0, 0.5)
    return f


def ssr_motion_vectors(depth, cb):
    """float32 [H,W,2]: the screen-space motion (NDC units: current minus previous position, as vqhip_forward_lighting_mrt writes it) of a STATIC scene seen at
    NDC depth `depth` through cb's camera, whose previous camera is cb.prevViewProjection — float64, rounded once. Sky pixels (depth 1) move like the far plane."""
    h, w = depth.shape
    x = (np.arange(w) + 0.5) / w * 2.0 - 1.0
    y = 1.0 - (np.arange(h) + 0.5) / h * 2.0
    ndc = np.stack(np.broadcast_arrays(x[None, :], y[:, None], depth.astype(np.float64), 1.0), -1)
    world = ndc @ _matrix_of(cb.invViewProjection)
    world /= world[..., 3:]
    prev = world @ _matrix_of(cb.prevViewProjection)
    return (ndc[..., :2] - prev[..., :2] / prev[..., 3:]).astype(np.float32)


# ---- FidelityFX CACAO (docs/DESIGN_DETAILS.md §7.14): the inputs of vqhip_cacao -----------------------------------------------------------------
CACAO_ROOM_CAMERA = {"camera": (-44.5, 0.6, -89.0), "look_at": (44.0, 6.0, 10.0)}   # in a corner of the room, low above the floor: view depths from ~1 to ~150


def cacao_room(width, height, **constants):
    """ssr_room seen by a camera close to the floor (CACAO_ROOM_CAMERA unless `constants` names another), as vqhip_cacao's inputs. Near pixels get sampling discs of
    more than a hundred half-resolution texels (depth mips 2 and 3), far ones a few texels (mip 0); box and wall silhouettes and the floor and the side wall at grazing
    angles give depth edges, creases normal edges (tests/test_cacao_cpu.py pins the shares at 1280 x 720).
    Returns a dict: depth float32 [H,W] (NDC z, the resolved scene depth), packed uint32 [H,W] / n01 float32 [H,W,4] (world-space normals as Tex_SceneNormals holds them,
    R10G10B10A2_UNORM and its decoded values), proj / normals_to_view float32 [4,4] as VQRenderer::RenderAmbientOcclusion stores them (SceneRendering.cpp:1525-1526:
    SceneView.proj and SceneView.view, row-major, row-vector convention)."""
    args = dict(CACAO_ROOM_CAMERA)
    args.update(constants)
    room = ssr_room(width, height, **args)
    return {"depth": room["depth"], "packed": room["packed"], "n01": room["n01"], "proj": _matrix_of(room["cb"].projection).astype(np.float32),
            "normals_to_view": _matrix_of(room["cb"].view).astype(np.float32)}


def cacao_noise(width, height, seed=0xCAC0):
    """White-noise inputs of vqhip_cacao with the camera of cacao_room: NDC depths whose view-space values are log-uniform in [0.15, 100] (neighbouring texels differ by
    factors: every depth edge closes, taps land on unrelated depths, and with a radius scaled to the frame size every mip is selected), unit normals on the whole sphere. Same dict as cacao_room."""
    cb = ssr_constants(width, height, 1, **CACAO_ROOM_CAMERA)
    room = {"proj": _matrix_of(cb.projection).astype(np.float32), "normals_to_view": _matrix_of(cb.view).astype(np.float32)}
    r = _chunk_rng(seed, 0)
    z = 0.15 * np.exp(r.random((height, width)) * np.log(100.0 / 0.15))
    p = room["proj"].astype(np.float64)
    depth = (p[2, 2] + p[3, 2] / z).astype(np.float32)                               # NDC z of view depth z
    n = r.normal(size=(height, width, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    packed, n01 = _pack_normals(n)
    return {"depth": depth, "packed": packed, "n01": n01, "proj": room["proj"], "normals_to_view": room["normals_to_view"]}
