"""PLY wire format of DQO-MAP's Gaussian maps: the host-side formatter / parser, and the device-side vertex table
(pack_rows / unpack_rows: dqo_map_pack_rows / dqo_map_unpack_rows, csrc/map_checkpoint.hip) that FusedMapper.save_model / load_model
move with one copy per table.

Reads and writes the files of /root/reference/SLAM/gaussian_pointcloud.py:
    construct_list_of_attributes :557-588   x y z nx ny nz f_dc_0..2 f_rest_0..(3(D+1)^2-4) opacity scale_0..2 rot_0..3 [confidence]
    save_model_ply :641-684                  one "vertex" element, every property float32, normals written as zeros,
                                             f_dc / f_rest flattened CHANNEL-major ([P, K, 3] -> transpose -> [P, 3 K])
    load :132-207                            the inverse; a missing confidence column reads as zeros
The reference goes through the third-party `plyfile` package (not vendored, not installed here), which writes
`format binary_little_endian 1.0` for native-endian float32 records; this module writes / parses that layout directly with numpy
(and also reads `format ascii 1.0`).  Values are RAW parameters (logit opacity, log scales, unnormalised quaternions), exactly what
the reference stores.

read_mesh_ply reads the other PLY of an evaluation: the ground-truth triangle mesh eval_pcd loads with trimesh (SLAM/eval.py:236), as
the two arrays dqo_eval.sample_surface takes.  write_mesh_ply writes such a file — the mesh of dqo_eval.TsdfVolume.extract, with vertex
colours — in the layout read_mesh_ply reads; write_mesh_ply_normals adds the vertex normals of dqo_eval.mesh_normals.
"""
import numpy as np


def attribute_names(n_rest, include_confidence=True):
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(n_rest)]
    names += ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    if include_confidence:
        names.append("confidence")
    return names


def save_model_ply(path, xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence=None, include_confidence=True):
    """xyz [P,3], shs [P,M,3] (coefficient 0 = f_dc, 1.. = f_rest), opacity_raw [P,1], scaling_raw [P,3], rotation_raw [P,4],
    confidence [P,1] or None (zeros).  Tensors or arrays; nothing is written for an empty map (gaussian_pointcloud.py:642-643)."""
    a = lambda t: np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, np.float32)
    xyz, shs, op, sc, rot = a(xyz), a(shs), a(opacity_raw).reshape(-1, 1), a(scaling_raw), a(rotation_raw)
    P = xyz.shape[0]
    if P == 0:
        return
    f_dc = shs[:, :1, :].transpose(0, 2, 1).reshape(P, -1)     # [P,1,3] -> [P,3,1] -> [P,3]
    f_rest = shs[:, 1:, :].transpose(0, 2, 1).reshape(P, -1)   # [P,K,3] -> [P,3,K] -> [P,3K]: channel-major
    cols = [xyz, np.zeros_like(xyz), f_dc, f_rest, op, sc, rot]
    if include_confidence:
        cols.append(np.zeros((P, 1), np.float32) if confidence is None else a(confidence).reshape(-1, 1))
    table = np.ascontiguousarray(np.concatenate(cols, axis=1), dtype="<f4")
    names = attribute_names(f_rest.shape[1], include_confidence)
    assert table.shape[1] == len(names)
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {P}\n" + "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(table.tobytes())


def write_vertex_table(path, table, n_rest, include_confidence=True):
    """The file save_model_ply writes, from its finished vertex table: `table` float32 [rows, C] (array or host tensor, C-contiguous;
    C = 9 + n_rest + 8 (+ 1), the columns of attribute_names(n_rest, include_confidence)).  The header, then the table's bytes as they
    are — no value is converted.  Nothing is written for zero rows (gaussian_pointcloud.py:642-643).  Returns the row count."""
    t = table.numpy() if hasattr(table, "numpy") else np.asarray(table)
    names = attribute_names(n_rest, include_confidence)
    if t.ndim != 2 or t.shape[1] != len(names) or t.dtype != np.float32 or not t.flags["C_CONTIGUOUS"]:
        raise ValueError(f"write_vertex_table: the table must be C-contiguous float32 [rows, {len(names)}], got {t.dtype} {t.shape}")
    rows = t.shape[0]
    if rows == 0:
        return 0
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {rows}\n" + "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(t.data)  # (native float32 is little-endian here, as in save_model_ply; no copy of the table is made)
    return rows


def read_vertex_table(path):
    """(property names, float32 [rows, len(names)] table) of a map file, binary or ascii; a binary table keeps every value's bits."""
    return _read_table(path)


def pack_workspace(P, device):
    """dqo_map_pack_rows' workspace for a map of P rows: zero when first used, then left to pack_rows."""
    import torch
    import _dqo_native as N
    return torch.zeros((N.lib().dqo_map_pack_workspace_bytes(int(P)),), dtype=torch.uint8, device=device)


def pack_rows(xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence=None, alive=None, stable=None, include_confidence=True, out=None,
              header=None, workspace_buffer=None):
    """(table, header): the vertex table of the map's live rows, on the device (dqo_map_pack_rows, include/dqo_raster.h).  Buffers are
    contiguous float32 device tensors of P rows (shs [P,M,3]); alive / stable uint8 [P] or None.  table float32 [P, C] (`out`, or new:
    rows at and behind U + S keep their bytes), header int32 [2] = {U, S} — the unstable cloud's rows first, then the stable cloud's.
    Nothing is read back."""
    import torch
    import _dqo_native as N
    N.require_gpu(xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence, alive, stable, out, header, workspace_buffer)
    P, M = int(xyz.shape[0]), int(shs.shape[1])
    C = 6 + 3 * M + 8 + (1 if include_confidence else 0)
    for t, n, dt in ((xyz, 3 * P, torch.float32), (shs, 3 * M * P, torch.float32), (opacity_raw, P, torch.float32),
                     (scaling_raw, 3 * P, torch.float32), (rotation_raw, 4 * P, torch.float32), (confidence, P, torch.float32),
                     (alive, P, torch.uint8), (stable, P, torch.uint8)):
        if t is not None and (t.dtype != dt or t.numel() != n or not t.is_contiguous()):
            raise RuntimeError(f"pack_rows: every buffer is contiguous, of the map's {P} rows and of its own type (got {t.dtype} {tuple(t.shape)})")
    dev = xyz.device
    if out is None:
        out = torch.empty((P, C), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != C or not out.is_contiguous():
        raise RuntimeError(f"pack_rows: out must be a contiguous float32 [rows, {C}] table")
    if header is None:
        header = torch.empty((2,), dtype=torch.int32, device=dev)
    if workspace_buffer is None:
        workspace_buffer = pack_workspace(P, dev)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_map_pack_rows(P, M, 1 if include_confidence else 0, N.ptr(xyz), N.ptr(shs), N.ptr(opacity_raw), N.ptr(scaling_raw),
                                          N.ptr(rotation_raw), N.ptr(confidence), N.ptr(alive), N.ptr(stable), N.ptr(out), int(out.shape[0]),
                                          N.ptr(header), N.ptr(workspace_buffer), workspace_buffer.numel(), N.current_stream()))
    return out, header


def pack_rows_by_object(xyz, shs, opacity_raw, scaling_raw, rotation_raw, gaussian_object, confidence=None, alive=None, stable=None,
                        include_confidence=False, out=None, header=None, workspace_buffer=None):
    """(table, header): the vertex data of every per-object file of save_model_ply_obj in one table, on the device
    (dqo_map_pack_rows_by_object, include/dqo_raster.h).  Buffers as pack_rows'; gaussian_object int32 [P], an id in [0, 64) = the row's
    object.  table float32 [P, C] (`out`, or new): the alive rows that have an object, ordered by (stable != 0, object id, row index);
    rows at and behind the total keep their bytes.  header int32 [2,64]: header[c, g] = the rows of cloud c (0 unstable, 1 stable),
    object g — object_file_slices turns its host copy into file names and slices.  include_confidence defaults to False, as
    mapper.py:1587-1588 passes.  Nothing is read back."""
    import torch
    import _dqo_native as N
    N.require_gpu(xyz, shs, opacity_raw, scaling_raw, rotation_raw, gaussian_object, confidence, alive, stable, out, header, workspace_buffer)
    P, M = int(xyz.shape[0]), int(shs.shape[1])
    C = 6 + 3 * M + 8 + (1 if include_confidence else 0)
    for t, n, dt in ((xyz, 3 * P, torch.float32), (shs, 3 * M * P, torch.float32), (opacity_raw, P, torch.float32),
                     (scaling_raw, 3 * P, torch.float32), (rotation_raw, 4 * P, torch.float32), (confidence, P, torch.float32),
                     (alive, P, torch.uint8), (stable, P, torch.uint8), (gaussian_object, P, torch.int32)):
        if t is not None and (t.dtype != dt or t.numel() != n or not t.is_contiguous()):
            raise RuntimeError(f"pack_rows_by_object: every buffer is contiguous, of the map's {P} rows and of its own type (got {t.dtype} "
                               f"{tuple(t.shape)})")
    dev = xyz.device
    if out is None:
        out = torch.empty((P, C), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != C or not out.is_contiguous():
        raise RuntimeError(f"pack_rows_by_object: out must be a contiguous float32 [rows, {C}] table")
    if header is None:
        header = torch.empty((2, 64), dtype=torch.int32, device=dev)
    elif header.dtype != torch.int32 or header.numel() != 128 or not header.is_contiguous():
        raise RuntimeError("pack_rows_by_object: header must be a contiguous int32 [2,64] tensor")
    if workspace_buffer is None:
        workspace_buffer = pack_workspace(P, dev)
    with torch.cuda.device(dev):
        N.check(N.lib().dqo_map_pack_rows_by_object(P, M, 1 if include_confidence else 0, N.ptr(xyz), N.ptr(shs), N.ptr(opacity_raw),
                                                    N.ptr(scaling_raw), N.ptr(rotation_raw), N.ptr(confidence), N.ptr(alive), N.ptr(stable),
                                                    N.ptr(gaussian_object), N.ptr(out), int(out.shape[0]), N.ptr(header),
                                                    N.ptr(workspace_buffer), workspace_buffer.numel(), N.current_stream()))
    return out, header


def object_file_slices(path, header):
    """[(file name, first table row, rows)] of the per-object files of a map saved under the prefix `path`, from the HOST copy of
    pack_rows_by_object's header ([2][64] counts, any nesting numpy can flatten): the reference's names — path + "_obj" +
    "{}.ply".format(id) for the unstable cloud, path + "_stable_obj" + ... for the stable one (mapper.py:1587-1588,
    gaussian_pointcloud.py:637) — in table order, only for the objects a cloud has rows of (np.unique, :593)."""
    counts = np.asarray(header, np.int64).reshape(2, 64)
    files, first = [], 0
    for c, tag in ((0, "_obj"), (1, "_stable_obj")):
        for g in range(64):
            n = int(counts[c, g])
            if n > 0:
                files.append((path + tag + "{}.ply".format(g), first, n))
            first += n
    return files


def unpack_rows(table, first_row, xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence=None):
    """The inverse (dqo_map_unpack_rows): the rows of `table` (float32 [n, C] on the device, with or without the confidence column) into
    rows [first_row, first_row + n) of the buffers; a table without the column writes zeros into `confidence`."""
    import torch
    import _dqo_native as N
    N.require_gpu(table, xyz, shs, opacity_raw, scaling_raw, rotation_raw, confidence)
    P, M = int(xyz.shape[0]), int(shs.shape[1])
    C = 6 + 3 * M + 8
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] not in (C, C + 1) or not table.is_contiguous():
        raise RuntimeError(f"unpack_rows: the table must be contiguous float32 [n, {C}] or [n, {C + 1}], got {table.dtype} {tuple(table.shape)}")
    for t, n in ((xyz, 3 * P), (shs, 3 * M * P), (opacity_raw, P), (scaling_raw, 3 * P), (rotation_raw, 4 * P), (confidence, P)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous()):
            raise RuntimeError(f"unpack_rows: every buffer is contiguous float32 of the map's {P} rows")
    with torch.cuda.device(xyz.device):
        N.check(N.lib().dqo_map_unpack_rows(P, M, int(table.shape[0]), int(first_row), 1 if table.shape[1] == C + 1 else 0, N.ptr(table),
                                            N.ptr(xyz), N.ptr(shs), N.ptr(opacity_raw), N.ptr(scaling_raw), N.ptr(rotation_raw),
                                            N.ptr(confidence), N.current_stream()))


def _read_table(path):
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, count, props, in_vertex = None, None, [], False
        while True:
            line = fh.readline()
            if not line:
                raise ValueError(f"{path}: truncated header")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    count = int(tok[2])
                elif count is not None:
                    raise ValueError(f"{path}: elements after 'vertex' are not supported")
            elif tok[0] == "property" and in_vertex:
                if tok[1] not in ("float", "float32"):
                    raise ValueError(f"{path}: property {tok[-1]} has type {tok[1]}, the map format is all float32")
                props.append(tok[2])
            elif tok[0] == "end_header":
                break
        if count is None:
            raise ValueError(f"{path}: no vertex element")
        if fmt in ("binary_little_endian", "binary_big_endian"):
            dt = "<f4" if fmt == "binary_little_endian" else ">f4"
            data = np.frombuffer(fh.read(4 * count * len(props)), dtype=dt)
            if data.size != count * len(props):
                raise ValueError(f"{path}: truncated vertex data")
            table = data.reshape(count, len(props)).astype(np.float32)
        elif fmt == "ascii":
            table = np.loadtxt(fh, dtype=np.float32, max_rows=count, ndmin=2)
            if table.shape != (count, len(props)):
                raise ValueError(f"{path}: bad ascii vertex table")
        else:
            raise ValueError(f"{path}: unknown format {fmt}")
    return props, table


def load_model_ply(path, max_sh_degree=3):
    """dict(xyz [P,3], shs [P,(D+1)^2,3], opacity_raw [P,1], scaling_raw [P,3], rotation_raw [P,4], confidence [P,1]) as float32
    arrays — the reference's `load` (gaussian_pointcloud.py:132-207) with f_dc / f_rest merged into one SH tensor."""
    props, table = _read_table(path)
    col = {n: i for i, n in enumerate(props)}
    get = lambda names: table[:, [col[n] for n in names]]
    rest = sorted((n for n in props if n.startswith("f_rest_")), key=lambda n: int(n.split("_")[-1]))
    K = (max_sh_degree + 1) ** 2 - 1
    assert len(rest) == 3 * K, f"{path}: {len(rest)} f_rest columns, degree {max_sh_degree} needs {3 * K}"
    P = table.shape[0]
    f_dc = get(["f_dc_0", "f_dc_1", "f_dc_2"]).reshape(P, 3, 1).transpose(0, 2, 1)
    f_rest = get(rest).reshape(P, 3, K).transpose(0, 2, 1)
    scales = sorted((n for n in props if n.startswith("scale_")), key=lambda n: int(n.split("_")[-1]))
    rots = sorted((n for n in props if n.startswith("rot")), key=lambda n: int(n.split("_")[-1]))
    conf = get(["confidence"]) if "confidence" in col else np.zeros((P, 1), np.float32)
    return dict(xyz=get(["x", "y", "z"]), shs=np.ascontiguousarray(np.concatenate([f_dc, f_rest], 1)), opacity_raw=get(["opacity"]),
                scaling_raw=get(scales), rotation_raw=get(rots), confidence=conf)


_PLY_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
                "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_MESH_COUNT_TYPES = ("uchar", "uint8", "int", "int32", "uint", "uint32")
_MESH_INDEX_TYPES = ("int", "int32", "uint", "uint32")


def read_mesh_ply(path):
    """(vertices float32 [V,3], faces int32 [F,3]) of a triangle mesh file — what trimesh.load(gt_meshfile) gives eval_pcd
    (SLAM/eval.py:236) of the reference's ground-truth meshes, read with numpy on the host.

    Accepted: `format ascii 1.0` and `format binary_little_endian 1.0`; a `vertex` element whose x, y, z are float / float32, anywhere
    among other scalar properties (normals, uchar colours), which are skipped; then a `face` element whose only property is
    `property list <uchar|uint8|int|int32|uint|uint32> <int|int32|uint|uint32> vertex_indices` (or vertex_index).  All faces are
    triangles, or all are quads: a quad (a, b, c, d) becomes (a, b, c), (a, c, d) in file order, as trimesh's loader splits it.  The
    face table is read as one structured array, not face by face.  Everything else raises RuntimeError naming the file and the
    reason.  Index values are NOT checked here (an index of 2^31 or more wraps negative): dqo_mesh_sample counts the faces whose
    indices are outside [0, V) and gives them no sample."""
    def bad(why):
        return RuntimeError(f"{path}: {why}")

    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise bad("not a PLY file")
        fmt, elements = None, []  # elements: [name, count, [(kind, ...)]]
        while True:
            line = fh.readline()
            if not line:
                raise bad("truncated header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1] if len(tok) > 1 else None
            elif tok[0] == "element" and len(tok) == 3:
                elements.append([tok[1], int(tok[2]), []])
            elif tok[0] == "property" and elements:
                elements[-1][2].append(tuple(tok[1:]))
            elif tok[0] == "end_header":
                break
            else:
                raise bad(f"unexpected header line {line.decode('ascii', 'replace').strip()!r}")
        if fmt == "binary_big_endian":
            raise bad("format binary_big_endian is not supported (ascii and binary_little_endian are)")
        if fmt not in ("ascii", "binary_little_endian"):
            raise bad(f"unknown format {fmt}")
        names = [e[0] for e in elements]
        for need in ("vertex", "face"):
            if need not in names:
                raise bad(f"no {need} element")
        if names != ["vertex", "face"]:
            raise bad(f"elements {names}: a mesh file holds 'vertex' then 'face' and nothing else")
        (_, V, vprops), (_, F, fprops) = elements
        if V < 0 or F < 0:
            raise bad("negative element count")
        fields = []
        for prop in vprops:
            if len(prop) != 2 or prop[0] not in _PLY_SCALARS:
                raise bad(f"vertex property {' '.join(prop)!r}: only scalar properties are supported")
            if prop[1] in ("x", "y", "z") and prop[0] not in ("float", "float32"):
                raise bad(f"vertex coordinate {prop[1]} has type {prop[0]}: float / float32 only (double coordinates are not supported)")
            fields.append((prop[1], "<" + _PLY_SCALARS[prop[0]]))
        vnames = [n for n, _ in fields]
        if len(set(vnames)) != len(vnames) or not all(c in vnames for c in "xyz"):
            raise bad("the vertex element needs one x, one y and one z property")
        if len(fprops) != 1:
            raise bad(f"the face element has {len(fprops)} properties: exactly one list of vertex indices is supported")
        fp = fprops[0]
        if (len(fp) != 4 or fp[0] != "list" or fp[1] not in _MESH_COUNT_TYPES or fp[2] not in _MESH_INDEX_TYPES
                or fp[3] not in ("vertex_indices", "vertex_index")):
            raise bad(f"face property {' '.join(fp)!r}: expected 'list <uchar|uint8|int|int32|uint|uint32> <int|int32|uint|uint32> "
                      "vertex_indices'")
        if fmt == "binary_little_endian":
            vdt = np.dtype(fields)
            raw = fh.read(vdt.itemsize * V)
            if len(raw) != vdt.itemsize * V:
                raise bad("truncated vertex data")
            vt = np.frombuffer(raw, dtype=vdt)
            vertices = np.stack([vt["x"], vt["y"], vt["z"]], axis=1).astype(np.float32) if V else np.zeros((0, 3), np.float32)
            cdt, idt = np.dtype("<" + _PLY_SCALARS[fp[1]]), np.dtype("<" + _PLY_SCALARS[fp[2]])
            if F == 0:
                return vertices, np.zeros((0, 3), np.int32)
            first = fh.read(cdt.itemsize)
            if len(first) != cdt.itemsize:
                raise bad("truncated face data")
            n = int(np.frombuffer(first, dtype=cdt)[0])
            if n not in (3, 4):
                raise bad(f"a face of {n} vertices: all faces must be triangles, or all quads")
            fdt = np.dtype([("n", cdt), ("v", idt, (n,))])
            raw = first + fh.read(fdt.itemsize * F - cdt.itemsize)
            if len(raw) != fdt.itemsize * F:
                raise bad("truncated face data (or faces of mixed sizes)")
            ft = np.frombuffer(raw, dtype=fdt)
            if not (ft["n"] == n).all():
                raise bad("faces of mixed sizes: all faces must be triangles, or all quads")
            idx = ft["v"]
        else:
            import warnings
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # (loadtxt warns about an empty table: reported below as truncated)
                    vt = np.loadtxt(fh, dtype=np.float64, max_rows=V, ndmin=2) if V else np.zeros((0, len(fields)))
            except ValueError as e:
                raise bad(f"bad ascii vertex table ({e})")
            if vt.shape != (V, len(fields)):
                raise bad("truncated vertex data")
            vertices = np.ascontiguousarray(vt[:, [vnames.index(c) for c in "xyz"]], dtype=np.float32)
            if F == 0:
                return vertices, np.zeros((0, 3), np.int32)
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ft = np.loadtxt(fh, dtype=np.int64, max_rows=F, ndmin=2)
            except ValueError as e:
                raise bad(f"faces of mixed sizes, or a bad ascii face table: all faces must be triangles, or all quads ({e})")
            if ft.shape[0] != F or ft.shape[1] < 1:
                raise bad("truncated face data")
            n = int(ft[0, 0])
            if n not in (3, 4):
                raise bad(f"a face of {n} vertices: all faces must be triangles, or all quads")
            if not (ft[:, 0] == n).all() or ft.shape[1] != n + 1:
                raise bad("faces of mixed sizes: all faces must be triangles, or all quads")
            idx = ft[:, 1:]
    idx = idx.astype(np.int64).astype(np.int32)  # (an index of 2^31 or more wraps negative: out of range for the device step)
    if n == 4:
        idx = idx[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3)
    return vertices, np.ascontiguousarray(idx, dtype=np.int32)


def _write_mesh(who, path, vertices, faces, normals, colors):
    a = lambda t, dt: np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=dt)
    v, f = a(vertices, np.float32), a(faces, np.int32)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"{who}: vertices must be [V,3] and faces [F,3], got {v.shape} and {f.shape}")
    V, F = v.shape[0], f.shape[0]
    columns = [("x", v[:, 0]), ("y", v[:, 1]), ("z", v[:, 2])]
    if normals is not None:
        n = a(normals, np.float32)
        if n.shape != (V, 3):
            raise ValueError(f"{who}: normals must be [{V},3], got {n.shape}")
        columns += [("nx", n[:, 0]), ("ny", n[:, 1]), ("nz", n[:, 2])]
    fields = [(k, "<f4") for k, _ in columns]
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {V}\n" + "".join(f"property float {k}\n" for k, _ in columns)
    if colors is not None:
        c = a(colors, np.float32)
        if c.shape != (V, 3):
            raise ValueError(f"{who}: colors must be [{V},3], got {c.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += f"element face {F}\nproperty list uchar int vertex_indices\nend_header\n"
    vt = np.zeros((V,), dtype=np.dtype(fields))
    for k, col in columns:
        vt[k] = col
    if colors is not None:
        with np.errstate(invalid="ignore"):
            c8 = np.rint(255.0 * np.clip(np.nan_to_num(c.astype(np.float64), nan=0.0), 0.0, 1.0)).astype(np.uint8)
        vt["red"], vt["green"], vt["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    ft = np.zeros((F,), dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    ft["n"], ft["v"] = 3, f
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vt.tobytes())
        fh.write(ft.tobytes())
    return V, F


def write_mesh_ply(path, vertices, faces, colors=None):
    """A triangle mesh file that read_mesh_ply reads back: `format binary_little_endian 1.0`, a `vertex` element of float x y z and, with
    colors, uchar red green blue = round(255 * clamp(c, 0, 1)), then a `face` element `property list uchar int vertex_indices`.
    vertices [V,3], faces [F,3] (indices, written as int32), colors [V,3] in [0, 1] or None; arrays or tensors (a device tensor is copied
    to the host: cut the buffers of dqo_eval.TsdfVolume.extract at its written counts first).  Returns (V, F)."""
    return _write_mesh("write_mesh_ply", path, vertices, faces, None, colors)


def write_mesh_ply_normals(path, vertices, faces, normals, colors=None):
    """write_mesh_ply with vertex normals — the mesh of dqo_eval.mesh_normals: the `vertex` element is float x y z nx ny nz and, with
    colors, uchar red green blue (open3d's property order; the colour bytes as write_mesh_ply writes them).  normals [V,3] float32.
    read_mesh_ply skips the extra scalars, so the file reads back.  Returns (V, F)."""
    return _write_mesh("write_mesh_ply_normals", path, vertices, faces, normals, colors)
