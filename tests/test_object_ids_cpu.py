"""CPU side of vqhip_object_ids (docs/DESIGN_DETAILS.md §7.21): rule P0 — the numpy statement the GPU tests compare against, held against its per-pixel scalar
transcription and against values worked out by hand —, the ObjectID pass's chain on the statement of §7.17 at cull NONE, and the boundary: symbols, struct layout
against gcc, the work-size function, the refusal without a context, the documents, the C++ adaptor against tests/cpp/mock_engine/."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tests import object_ids_cases as PC
from tests import object_ids_ref as P
from tests import scene_depth_cases as SC
from tests import scene_depth_ref as V
from vqengine_amd import abi, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"vqhip_object_ids", "vqhip_object_ids_work_bytes"}


# ---- P0 ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_p0_by_hand():
    """the table's boundaries, worked out from its definition: an instance boundary, the last q of a draw, q = total, 0xFFFFFFFF; empty draws own nothing"""
    t = PC.table()
    assert P.instanced_triangles(t) == PC.TABLE_TOTAL

    def at(q):
        return tuple(int(v) for v in P.resolve(t, np.array([[q]], dtype=np.uint32))[0, 0])

    def want(d, inst):
        return (int(t[d]["obj_id"][inst, 0]), t[d]["mesh_id"], t[d]["material_id"], int(t[d]["obj_id"][inst, 3]))
    assert at(0) == want(1, 0) and at(3) == want(1, 0)                              # the last q of draw 1 (the empty draw 0 in front of it owns nothing)
    assert at(4) == want(3, 0) and at(5) == want(3, 0) and at(6) == want(3, 1)      # the instance boundary inside draw 3: two triangles per instance
    assert at(7) == want(3, 1) and at(8) == want(3, 2) and at(9) == want(3, 2)
    assert at(10) == want(4, 0) and at(11) == want(4, 1) and at(73) == want(4, 63)  # 64 instances of one triangle
    assert at(74) == want(6, 0) and at(78) == want(6, 0)                            # past the empty draw 5
    assert at(79) == (0, 0, 0, 0) and at(80) == (0, 0, 0, 0)                        # q = total and beyond: the clear colour
    assert at(0xFFFFFFFF) == (0, 0, 0, 0) and at(0x80000000) == (0, 0, 0, 0) and at(0xFFFFFFFE) == (0, 0, 0, 0)
    assert want(3, 0)[2] == 2**31 - 1 and want(4, 0)[1] == -2**31                   # the ids travel as int32, whatever their value
    for ids in (900, 901, 902, 903, 904, 905, 906, 907):                            # nothing of an empty draw ever shows
        for name, plane in PC.owner_planes(16, 16).items():
            got = P.resolve(t, plane)
            assert not (got[..., 1] == ids).any() and not (got[..., 2] == ids).any(), (name, ids)


def test_p0_statement_equals_its_scalar_transcription():
    t = PC.table()
    for (w, h) in ((16, 16), (37, 9)):
        for name, plane in PC.owner_planes(w, h).items():
            a, b = P.resolve(t, plane), P.resolve_scalar(t, plane)
            assert a.dtype == np.int32 and a.shape == (h, w, 4) and np.array_equal(a, b), name
    assert (P.resolve([], PC.owner_planes(16, 16)["garbage"]) == 0).all()           # no draws at all: every pixel the clear colour
    assert (P.resolve([P.id_draw(0, np.ones((1, 4)), 1, 1)], PC.owner_planes(16, 16)["garbage"]) == 0).all()
    # the owner plane may come as int32 (the binding's dtype): the bits count
    plane = PC.owner_planes(16, 16)["boundaries"]
    assert np.array_equal(P.resolve(t, plane.view(np.int32)), P.resolve(t, plane))


def test_garbage_owner_plane_yields_only_table_values_or_zeros():
    t = PC.table()
    got = P.resolve(t, PC.owner_planes(64, 40)["garbage"]).reshape(-1, 4)
    allowed = {(0, 0, 0, 0)}
    for d in t:
        if d["num_indices"]:
            allowed |= {(int(o[0]), d["mesh_id"], d["material_id"], int(o[3])) for o in d["obj_id"]}
    seen = set(map(tuple, got.tolist()))
    assert seen <= allowed and len(seen) > 20 and (0, 0, 0, 0) in seen


def test_chain_on_the_statement_of_the_depth_pass():
    """boxes (64 instances) and room at cull NONE: every owned pixel names the draw and instance its q belongs to; the unread objID columns never show; forcing the
    cull mode matters: under a draw list that culls front faces the pre-pass's own plane would give other ids"""
    for name in ("boxes_64x40", "room_64x40", "boxes_16x16"):
        owner, draws, ids = PC.chain_expected(name)
        assert np.array_equal(ids, P.resolve_scalar(draws, owner)), name
        q = owner.view(np.uint32)
        owned = q != P.NO_OWNER
        assert owned.any() and ((ids[~owned] == 0).all())
        assert not (ids == 0x0BADF00D).any() and not (ids == -0x0BADF00D).any()
        scene = PC.chain_cases()[name]
        first = 0
        for k, (d, idd) in enumerate(zip(scene["draws"], draws)):
            tris, n = len(d["indices"]) // 3, np.asarray(d["wvp"]).shape[0]
            mine = owned & (q >= first) & (q < first + tris * n)
            assert (ids[mine][:, 1] == idd["mesh_id"]).all() and (ids[mine][:, 0] == 1000 * (k + 1) + (q[mine] - first) // tris).all()
            first += tris * n
    assert len(set(PC.chain_expected("boxes_64x40")[2][..., 0].reshape(-1).tolist())) > 10           # many instances on screen
    assert len(set(PC.chain_expected("room_64x40")[2][..., 1].reshape(-1).tolist()) - {0}) == 2      # both draws of the room
    # the room's walls under a draw list that culls front faces: the pre-pass's plane loses them, the ObjectID pass (cull NONE whatever iFaceCull says) keeps them
    culled = V.rasterize(SC.room_scene(16, 16, 1, cull=V.CULL_FRONT))["primitive"]
    forced = PC.chain_expected("room_16x16")[0]
    assert np.array_equal(V.rasterize(PC.cull_none(SC.room_scene(16, 16, 1, cull=V.CULL_FRONT)))["primitive"], forced)
    assert (culled != forced).sum() > 100 and (forced != P.NO_OWNER).all()


# ---- boundary -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "vqhip.h")).read()
    declared = set(re.findall(r"VQHIP_API\s+[\w\s\*]+?\b(vqhip_object_ids\w*)\s*\(", src))
    assert declared == NEW_SYMBOLS
    lib = capi.load_library()
    for s in declared:
        assert s in capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.vqhip_abi_version() == abi.ABI_VERSION == 3                          # additions only
    assert "#define VQHIP_ABI_VERSION 3 " in src
    section = src[src.index("The ObjectID pass (picking)"):]
    for word in ("P0", "VQHIP_CULL_NONE", "clear colour", "HasDiffuseMap", "Material::IsAlphaMasked", "Any owner content is safe", "Out of scope", "Magnifier"):
        assert word in section, f"{word} is not stated in the header section"


def test_struct_layout_equals_the_c_header(tmp_path):
    structs = (("vqhip_object_id_draw", abi.ObjectIdDraw),)
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vqhip.h"\nint main(void){\n'
    for cname, t in structs:
        prog += f'printf("%zu", sizeof({cname}));\n' + "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n, _ in t._fields_) + 'printf("\\n");\n'
    prog += "return 0;}\n"
    (tmp_path / "t.c").write_text(prog)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    lines = subprocess.check_output([str(tmp_path / "t")]).decode().strip().split("\n")
    for (cname, t), line in zip(structs, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_], cname
    assert C.sizeof(abi.ObjectIdDraw) == 24


def test_work_size_function():
    f = capi.load_library().vqhip_object_ids_work_bytes
    assert f(0) == 256 and f(1) == 256 and f(8) == 256 and f(9) == 512              # 32 bytes per draw, rounded up to 256
    counts = (1, 9, 100, 2000, 20000)
    sizes = [f(n) for n in counts]
    assert all(s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    for n, s in zip(counts, sizes):
        assert n * abi.OBJECT_ID_JOB_BYTES <= s < n * abi.OBJECT_ID_JOB_BYTES + 256
    assert f(-1) == 0
    assert capi.object_ids_work_bytes(2000) == f(2000)


def test_call_without_a_context_is_refused():
    lib = capi.load_library()
    buf = (C.c_uint8 * 8192)()
    rc = lib.vqhip_object_ids(None, None, None, 0, 16, 16, buf, 0, buf, 0, buf, 8192)
    assert rc == abi.VQHIP_ERR_INVALID_ARG and b"ctx is NULL" in lib.vqhip_last_error(None)


def test_documents_state_the_pass():
    doc = open(os.path.join(ROOT, "docs", "DESIGN_DETAILS.md")).read()
    section = doc[doc.index("### 7.21"):]
    for word in ("**P0**", "vqhip_object_ids", "VQHIP_CULL_NONE", "HasDiffuseMap", "tests/object_ids_ref.py", "OutlinePass", "Magnifier"):
        assert word in section, f"{word} is not stated in §7.21"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "vqhip_object_ids" in design
    assert "vqhip_object_ids" in open(os.path.join(ROOT, "README.md")).read()
    assert "RenderObjectIDPass" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_cpp_adaptor_builds_the_calls_from_the_pass(tmp_path):
    """tests/cpp/test_passes_object_ids.cpp (vqhip::ObjectIDPass) against tests/cpp/mock_engine/, with the command line tests/test_masked_depth_cpu.py uses"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = tmp_path / "test_passes_object_ids"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    lib = os.path.join(ROOT, "vqengine_amd", "lib")
    r = subprocess.run([hipcc, "-std=c++17", "-O2", "-Wall", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I.", "-I../../include", "-I/opt/rocm/include",
                        "test_passes_object_ids.cpp", "-o", str(exe), "-L../../vqengine_amd/lib", "-lvqhip", "-L/opt/rocm/lib", "-lamdhip64",
                        f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=cpp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "object id adaptor OK" in r.stdout, (r.returncode, r.stdout, r.stderr)
