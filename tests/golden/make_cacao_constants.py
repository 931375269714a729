"""Regenerates tests/golden/cacao_constants.json: the output of the reference's own FFX_CACAO_UpdateBufferSizeInfo / _UpdateConstants / _UpdatePerPassConstants
(Source/Renderer/Libs/AMDFidelityFX/CACAO/ffx_cacao.cpp) for the cases tests/test_cacao_cpu.py checks the host mirror (vqengine_amd/cacao.py) against.
Compiles that file from where the reference lies together with the small driver below and runs it; needs the reference's sources, so it is run by hand where
they exist:   python tests/golden/make_cacao_constants.py <reference root>
The fixture holds recorded numbers only (every float as its bit pattern)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vqengine_amd import synth                                          # noqa: E402

DRIVER = r"""
#include "ffx_cacao.h"
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static void dump(const FFX_CACAO_Constants* c) {
    const unsigned* w = (const unsigned*)c;
    printf("[");
    for (size_t i = 0; i < sizeof(*c) / 4; ++i) printf("%s%u", i ? "," : "", w[i]);
    printf("]");
}
int main(int argc, char** argv) {
    /* argv: width height, then 16 projection words, then 16 normals-to-view words */
    unsigned width = (unsigned)atoi(argv[1]), height = (unsigned)atoi(argv[2]);
    FFX_CACAO_Matrix4x4 proj, ntv;
    for (int i = 0; i < 16; ++i) { unsigned u = (unsigned)strtoul(argv[3 + i], 0, 10); memcpy(&proj.elements[i / 4][i % 4], &u, 4); }
    for (int i = 0; i < 16; ++i) { unsigned u = (unsigned)strtoul(argv[19 + i], 0, 10); memcpy(&ntv.elements[i / 4][i % 4], &u, 4); }
    FFX_CACAO_Settings s = FFX_CACAO_DEFAULT_SETTINGS;
    FFX_CACAO_BufferSizeInfo b;
    memset(&b, 0, sizeof(b));
    FFX_CACAO_UpdateBufferSizeInfo(width, height, FFX_CACAO_FALSE, &b);
    const unsigned* bw = (const unsigned*)&b;
    printf("{\"buffer_size_info\":[");
    for (size_t i = 0; i < sizeof(b) / 4; ++i) printf("%s%u", i ? "," : "", bw[i]);
    printf("],\"default_settings\":[%u,%u,%u,%u,%u,%u,%u,%d,%u,%u,%u,%u,%u,%u,%d,%u,%u],", bits(s.radius), bits(s.shadowMultiplier), bits(s.shadowPower), bits(s.shadowClamp),
           bits(s.horizonAngleThreshold), bits(s.fadeOutFrom), bits(s.fadeOutTo), (int)s.qualityLevel, bits(s.adaptiveQualityLimit), s.blurPassCount, bits(s.sharpness),
           bits(s.temporalSupersamplingAngleOffset), bits(s.temporalSupersamplingRadiusOffset), bits(s.detailShadowStrength), (int)s.generateNormals,
           bits(s.bilateralSigmaSquared), bits(s.bilateralSimilarityDistanceSigma));
    FFX_CACAO_Constants c;
    memset(&c, 0, sizeof(c));
    FFX_CACAO_UpdateConstants(&c, &s, &b, &proj, &ntv);
    printf("\"shared\":"); dump(&c);
    printf(",\"per_pass\":[");
    for (int p = 0; p < 4; ++p) {
        FFX_CACAO_Constants q;
        memset(&q, 0, sizeof(q));
        FFX_CACAO_UpdateConstants(&q, &s, &b, &proj, &ntv);
        FFX_CACAO_UpdatePerPassConstants(&q, &s, &b, p);
        printf("%s", p ? "," : ""); dump(&q);
    }
    printf("]}\n");
    return 0;
}
"""

SIZES = ((1280, 720), (125, 93), (3840, 2160))
CAMERAS = ({"camera": (-44.5, 0.6, -89.0), "look_at": (44.0, 6.0, 10.0)}, {"camera": (3.0, 10.0, -60.0), "look_at": (0.0, 2.0, 0.0)})


def matrices(width, height, k):
    """Projection 0: the left-handed one of synth.ssr_constants (60 degrees, 0.1 .. 1500). Projection 1: a RIGHT-handed one, 45 degrees, 0.5 .. 300
    (XMMatrixPerspectiveFovRH: elements[2][2] < 0, so FFX_CACAO_UpdateConstants takes its `depthLinearizeMul * depthLinearizeAdd < 0` branch), with the other view."""
    cb = synth.ssr_constants(width, height, 1, **CAMERAS[k])
    proj = synth._matrix_of(cb.projection)
    if k == 1:
        zn, zf, hh = 0.5, 300.0, 1.0 / np.tan(0.5 * np.pi / 4.0)
        proj = np.zeros((4, 4))
        proj[0, 0], proj[1, 1], proj[2, 2], proj[2, 3], proj[3, 2] = hh / (width / height), hh, zf / (zn - zf), -1.0, zn * zf / (zn - zf)
    return proj.astype(np.float32), synth._matrix_of(cb.view).astype(np.float32)


def main(reference_root):
    src = os.path.join(reference_root, "Source", "Renderer", "Libs", "AMDFidelityFX", "CACAO")
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        drv, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(drv, "w").write(DRIVER)
        subprocess.check_call(["g++", "-std=c++17", "-O0", "-ffp-contract=off", "-I", src, drv, os.path.join(src, "ffx_cacao.cpp"), "-o", exe, "-lm"])
        for (w, h) in SIZES:
            for k in range(len(CAMERAS)):
                proj, ntv = matrices(w, h, k)
                words = [str(int(x)) for x in np.concatenate([proj.ravel().view(np.uint32), ntv.ravel().view(np.uint32)])]
                out = json.loads(subprocess.check_output([exe, str(w), str(h)] + words))
                out.update(width=w, height=h, projection=k, proj=[int(x) for x in proj.ravel().view(np.uint32)], normals_to_view=[int(x) for x in ntv.ravel().view(np.uint32)])
                cases.append(out)
    path = os.path.join(ROOT, "tests", "golden", "cacao_constants.json")
    with open(path, "w") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(cases)} cases")


if __name__ == "__main__":
    main(sys.argv[1])
