"""The Gaussian checkpoint format either side of the rasterizer: `point_cloud.ply` as written by
`GaussianModel.save_ply` and read by `load_ply` (reference scene/gaussian_model.py:264-360), without the `plyfile`
dependency (absent from this image).  Binary little-endian, one `vertex` element, every property `float`:

    x y z | nx ny nz | nd | f_dc_0..2 | f_rest_0..(3(K-1)-1) | opacity | scale_0..2 | rot_0..3

`nx,ny,nz` hold the raw `_normal` parameter and `nd` the raw `_offset` (the reference overwrites the conventional
zero normals with them, :283-284); SH blocks are stored channel-major -- `features.transpose(1, 2).flatten(1)` -- i.e.
f_rest_j = coefficient (1 + j % (K-1)) of colour channel j // (K-1).  All values are the RAW (pre-activation) parameters."""
import numpy as np


def attribute_names(n_rest):
    """construct_list_of_attributes (gaussian_model.py:264-277) for 3 DC and `n_rest` higher-order SH values."""
    names = ["x", "y", "z", "nx", "ny", "nz", "nd"]
    names += ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(n_rest)]
    return names + ["opacity"] + ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)]


def save_ply(path, xyz, normal, offset, features_dc, features_rest, opacity, scaling, rotation):
    """Arrays as the model holds them: xyz (P,3), normal (P,3), offset (P,1), features_dc (P,1,3), features_rest (P,K-1,3),
    opacity (P,1), scaling (P,3), rotation (P,4).  numpy arrays or anything `np.asarray` accepts (detached CPU tensors)."""
    a = lambda t: np.asarray(t, dtype=np.float32)
    xyz = a(xyz); P = xyz.shape[0]
    f_dc = a(features_dc).transpose(0, 2, 1).reshape(P, -1)
    f_rest = a(features_rest).transpose(0, 2, 1).reshape(P, -1)
    table = np.concatenate([xyz, a(normal).reshape(P, 3), a(offset).reshape(P, 1), f_dc, f_rest, a(opacity).reshape(P, 1),
                            a(scaling).reshape(P, 3), a(rotation).reshape(P, 4)], axis=1).astype("<f4")
    names = attribute_names(f_rest.shape[1])
    assert table.shape[1] == len(names)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % P
    header += "".join("property float %s\n" % n for n in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(table).tobytes())


def load_ply(path, max_sh_degree=None):
    """Returns a dict of float32 arrays in the model's layout (see save_ply); checks the SH count like the reference (:326)."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or not lines[1].startswith("format binary_little_endian"):
        raise ValueError("load_ply reads binary little-endian PLY files")
    P, props, in_vertex = 0, [], False
    types = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "int": "<i4", "int32": "<i4"}
    for ln in lines[2:]:
        t = ln.split()
        if t[:2] == ["element", "vertex"]:
            P, in_vertex = int(t[2]), True
        elif t[:1] == ["element"]:
            in_vertex = False
        elif t[:1] == ["property"] and in_vertex:
            props.append((t[2], types[t[1]]))
    rec = np.frombuffer(raw, dtype=np.dtype(props), count=P, offset=end)
    col = lambda n: np.asarray(rec[n], np.float32)
    rest = sorted([n for n, _ in props if n.startswith("f_rest_")], key=lambda s: int(s.split("_")[-1]))
    if max_sh_degree is not None and len(rest) != 3 * (max_sh_degree + 1) ** 2 - 3:
        raise ValueError("PLY holds %d f_rest values, expected %d" % (len(rest), 3 * (max_sh_degree + 1) ** 2 - 3))
    K1 = len(rest) // 3
    out = {"xyz": np.stack([col("x"), col("y"), col("z")], 1), "normal": np.stack([col("nx"), col("ny"), col("nz")], 1),
           "offset": col("nd").reshape(-1, 1), "opacity": col("opacity").reshape(-1, 1),
           "features_dc": np.stack([col("f_dc_0"), col("f_dc_1"), col("f_dc_2")], 1).reshape(P, 3, 1).transpose(0, 2, 1).copy(),
           "features_rest": (np.stack([col(n) for n in rest], 1).reshape(P, 3, K1).transpose(0, 2, 1).copy() if K1 else np.zeros((P, 0, 3), np.float32)),
           "scaling": np.stack([col(n) for n in sorted([n for n, _ in props if n.startswith("scale_")], key=lambda s: int(s.split("_")[-1]))], 1),
           "rotation": np.stack([col(n) for n in sorted([n for n, _ in props if n.startswith("rot")], key=lambda s: int(s.split("_")[-1]))], 1)}
    return out


MESH_VERTEX_PROPS = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def save_mesh(path, mesh):
    """A triangle mesh (tsdf.TriangleMesh or anything with vertices / faces / colors / normals) as Open3D's write_triangle_mesh writes it with
    write_vertex_colors=True, write_vertex_normals=True (render.py:361-364): binary little-endian, vertex `x y z nx ny nz` (float) `red green
    blue` (uchar, round(255 clamp(c, 0, 1)), halves rounded up), face `list uchar int vertex_indices`."""
    v = _np(mesh.vertices).astype("<f4").reshape(-1, 3)
    n = _np(mesh.normals).astype("<f4").reshape(-1, 3)
    c = np.floor(255.0 * np.clip(_np(mesh.colors).astype(np.float64).reshape(-1, 3), 0.0, 1.0) + 0.5).astype("u1")
    f = _np(mesh.faces).astype("<i4").reshape(-1, 3)
    rec = np.empty(v.shape[0], dtype=np.dtype(MESH_VERTEX_PROPS))
    for i, k in enumerate("xyz"):
        rec[k] = v[:, i]; rec["n" + k] = n[:, i]
    for i, k in enumerate(("red", "green", "blue")):
        rec[k] = c[:, i]
    frec = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]))
    frec["n"] = 3
    frec["idx"] = f
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % v.shape[0]
    header += "".join("property %s %s\n" % ("float" if t == "<f4" else "uchar", k) for k, t in MESH_VERTEX_PROPS)
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % f.shape[0]
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def load_mesh(path):
    """Reads what save_mesh writes -> dict of numpy arrays: vertices (V,3) f32, normals (V,3) f32, colors (V,3) uint8, faces (F,3) int32."""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or not lines[1].startswith("format binary_little_endian"):
        raise ValueError("load_mesh reads binary little-endian PLY files")
    V = F = 0
    props = []
    for ln in lines[2:]:
        t = ln.split()
        if t[:2] == ["element", "vertex"]:
            V = int(t[2])
        elif t[:2] == ["element", "face"]:
            F = int(t[2])
        elif t[:1] == ["property"] and t[1] != "list":
            props.append((t[2], {"float": "<f4", "uchar": "u1"}[t[1]]))
        elif t[:2] == ["property", "list"] and t[2:4] != ["uchar", "int"]:
            raise ValueError("load_mesh expects `list uchar int` faces")
    rec = np.frombuffer(raw, dtype=np.dtype(props), count=V, offset=end)
    frec = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("idx", "<i4", (3,))]), count=F, offset=end + rec.nbytes)
    if F and not np.all(frec["n"] == 3):
        raise ValueError("load_mesh reads triangle meshes only")
    st = lambda ks: np.stack([np.asarray(rec[k]) for k in ks], 1)
    return {"vertices": st("xyz").astype(np.float32), "normals": st(["nx", "ny", "nz"]).astype(np.float32),
            "colors": st(["red", "green", "blue"]).astype(np.uint8), "faces": np.asarray(frec["idx"], np.int32).reshape(-1, 3)}
