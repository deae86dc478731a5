"""Mesh writers beside nerf_sh.gen_mesh.save_obj (the reference's nerf_sh/gen_mesh.py:133-158, which writes `v x y z [r g b]` and
`f a b c` and knows no normals): binary PLY with optional normals and colours, and OBJ with `vn` records.  Host numpy only."""
import numpy as np


def _check(vertices, triangles, normals, vert_rgb):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(triangles, np.int64).reshape(-1, 3)
    for name, a in (("normals", normals), ("vert_rgb", vert_rgb)):
        if a is not None and np.asarray(a).shape != v.shape:
            raise ValueError(f"{name} has shape {np.asarray(a).shape}, the vertices {v.shape}")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"triangle indices outside [0, {len(v)})")
    return v, f


def rgb_to_uchar(vert_rgb):
    """round(255 c) of colours in [0, 1] (clipped), uint8."""
    return np.rint(np.clip(np.asarray(vert_rgb, np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def save_ply(vertices, triangles, path, normals=None, vert_rgb=None):
    """Binary little-endian PLY: per vertex `x y z` float32, then `nx ny nz` float32 if normals are given, then `red green blue`
    uchar (round(255 c)) if colours are; per face a uchar count (3) and three int indices."""
    v, f = _check(vertices, triangles, normals, vert_rgb)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if vert_rgb is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.zeros(len(v), np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        n = np.asarray(normals, np.float64)
        rec["nx"], rec["ny"], rec["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if vert_rgb is not None:
        c = rgb_to_uchar(vert_rgb)
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    if f.size and f.max() >= 2 ** 31:
        raise ValueError("PLY `int` face indices hold fewer than 2^31 vertices")
    faces = np.zeros(len(f), np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    faces["n"], faces["i"] = 3, f
    names = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    header += [f"property {names[t]} {name}" for name, t in fields]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(faces.tobytes())


def load_ply(path):
    """What save_ply wrote: (vertices float32 [V,3], triangles int32 [T,3], normals float32 [V,3] or None, colours uint8 [V,3]
    or None).  Reads this module's own layout only (binary little-endian, triangles)."""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").splitlines()
    if lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    types = {"float": "<f4", "uchar": "u1"}
    n_vert = n_face = None
    fields, element = [], None
    for line in lines[2:-1]:
        tok = line.split()
        if tok[0] == "element":
            element = tok[1]
            if element == "vertex":
                n_vert = int(tok[2])
            elif element == "face":
                n_face = int(tok[2])
            else:
                raise ValueError(f"{path}: unexpected element {element}")
        elif tok[0] == "property" and element == "vertex":
            fields.append((tok[2], types[tok[1]]))
        elif tok != ["property", "list", "uchar", "int", "vertex_indices"]:
            raise ValueError(f"{path}: unexpected header line {line!r}")
    vdt = np.dtype(fields)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    if len(blob) != end + n_vert * vdt.itemsize + n_face * fdt.itemsize:
        raise ValueError(f"{path}: {len(blob)} bytes, the header announces {end + n_vert * vdt.itemsize + n_face * fdt.itemsize}")
    rec = np.frombuffer(blob, vdt, n_vert, end)
    faces = np.frombuffer(blob, fdt, n_face, end + n_vert * vdt.itemsize)
    if n_face and not (faces["n"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    have = set(vdt.names)
    pick = lambda names: np.stack([rec[n] for n in names], 1) if set(names) <= have else None
    return pick(("x", "y", "z")), faces["i"].copy(), pick(("nx", "ny", "nz")), pick(("red", "green", "blue"))


def save_obj_normals(vertices, triangles, path, normals, vert_rgb=None):
    """OBJ with one normal per vertex: `v x y z [r g b]`, `vn x y z`, then 1-based `f a//a b//b c//c`; four decimals as
    gen_mesh.save_obj writes them."""
    v, f = _check(vertices, triangles, normals, vert_rgb)
    n = np.asarray(normals, np.float64)
    with open(path, "w") as fh:
        if vert_rgb is None:
            fh.writelines("v %.4f %.4f %.4f\n" % tuple(p) for p in v)
        else:
            fh.writelines("v %.4f %.4f %.4f %.4f %.4f %.4f\n" % (*p, *c) for p, c in zip(v, np.asarray(vert_rgb)))
        fh.writelines("vn %.4f %.4f %.4f\n" % tuple(p) for p in n)
        fh.writelines("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in (f + 1))


def save_mesh(vertices, triangles, path, normals=None, vert_rgb=None, fmt=None):
    """One call for the CLIs: PLY when fmt == "ply" or (fmt is None and) the path ends in .ply, else OBJ -- through
    gen_mesh.save_obj when there are no normals, so that such a file is byte for byte what it was."""
    if fmt == "ply" or (fmt is None and str(path).lower().endswith(".ply")):
        save_ply(vertices, triangles, path, normals=normals, vert_rgb=vert_rgb)
    elif normals is not None:
        save_obj_normals(vertices, triangles, path, normals, vert_rgb=vert_rgb)
    else:
        from .nerf_sh.gen_mesh import save_obj
        save_obj(vertices, triangles, path, vert_rgb=vert_rgb)
