"""docs/DESIGN_DETAILS.md §7.21 P0 (the contract of vqhip_object_ids) stated in numpy: the ObjectID pass's int4 target from an owner plane. `resolve` is the
statement the GPU tests compare against, bit for bit; `resolve_scalar` is its per-pixel transcription (a linear walk over the draws, no search, no cumulative
sums), which tests/test_object_ids_cpu.py holds it against. A draw is a dict: num_indices, obj_id (int32 [n, 4]), mesh_id, material_id."""
import numpy as np

NO_OWNER = 0xFFFFFFFF
MAX_INSTANCES = 64


def id_draw(num_indices, obj_id, mesh_id, material_id):
    obj_id = np.ascontiguousarray(obj_id, dtype=np.int32).reshape(-1, 4)
    assert num_indices % 3 == 0 and 1 <= obj_id.shape[0] <= MAX_INSTANCES
    return {"num_indices": int(num_indices), "obj_id": obj_id, "mesh_id": int(mesh_id), "material_id": int(material_id)}


def instanced_triangles(draws):
    return sum((d["num_indices"] // 3) * d["obj_id"].shape[0] for d in draws)


def resolve(draws, owner):
    """int32 [H, W, 4]: (objID[instance].x, meshID, materialID, objID[instance].w) of the draw and instance that own q, (0, 0, 0, 0) where q owns nothing"""
    q = np.ascontiguousarray(owner).view(np.uint32).astype(np.int64)
    jobs = [d for d in draws if d["num_indices"]]                                   # a draw without indices owns no q
    out = np.zeros(q.shape + (4,), dtype=np.int32)
    if not jobs:
        return out
    tris = np.array([d["num_indices"] // 3 for d in jobs], dtype=np.int64)
    count = tris * np.array([d["obj_id"].shape[0] for d in jobs], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(count)[:-1]])
    total = int(count.sum())
    owned = q < total                                                               # 0xFFFFFFFF is far beyond any total the call accepts (< 2^29)
    job = np.searchsorted(first, q[owned], side="right") - 1                        # the last job whose first is <= q
    inst = (q[owned] - first[job]) // tris[job]
    base = np.concatenate([[0], np.cumsum([d["obj_id"].shape[0] for d in jobs])[:-1]])
    obj = np.concatenate([d["obj_id"] for d in jobs], axis=0)[base[job] + inst]
    out[owned] = np.stack([obj[:, 0], np.array([d["mesh_id"] for d in jobs], dtype=np.int32)[job],
                           np.array([d["material_id"] for d in jobs], dtype=np.int32)[job], obj[:, 3]], axis=1)
    return out


def resolve_scalar(draws, owner):
    """the same, one pixel and one draw at a time"""
    q_plane = np.ascontiguousarray(owner).view(np.uint32)
    h, w = q_plane.shape
    out = np.zeros((h, w, 4), dtype=np.int32)
    for j in range(h):
        for i in range(w):
            q = int(q_plane[j, i])
            if q == NO_OWNER:
                continue
            first = 0
            for d in draws:
                tris, n = d["num_indices"] // 3, d["obj_id"].shape[0]
                if tris and q < first + tris * n:
                    inst = (q - first) // tris
                    out[j, i] = (d["obj_id"][inst, 0], d["mesh_id"], d["material_id"], d["obj_id"][inst, 3])
                    break
                first += tris * n
    return out
