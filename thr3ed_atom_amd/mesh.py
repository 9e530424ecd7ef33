"""Iso-surface extraction of a ReLU field: the level set sigma = iso_level of a VoxelGrid's density as a closed, oriented,
coloured triangle mesh, computed by the HIP kernels of csrc/mesh_kernels.hip (rf_mesh_tiles / rf_mesh_count / rf_mesh_emit).

The field is the renderer's density -- post(interp(pre(D * rho))), zero on and outside the AABB -- sampled on a lattice of
``subdivisions`` points per voxel and axis plus one guard plane on every face of the AABB (so every surface closes), split into
Kuhn tetrahedra.  The ReLU after the trilinear interpolation puts surfaces inside voxels; subdivisions > 1 resolve them.  The
full contract, including the canonical vertex and face order, is in DESIGN.md ("Iso-surface extraction").
"""
import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib, _marshal

MAX_SUBDIVISIONS = 8


class Mesh(NamedTuple):
    vertices: Tensor  # [V, 3] float32
    faces: Tensor  # [T, 3] int64 vertex indices, (v1 - v0) x (v2 - v0) pointing out of {sigma > iso_level}
    colours: Optional[Tensor]  # [V, 3] float32: sigmoid(C0 * degree-0 SH coefficient) -- the colour render_diffuse composites
    normals: Optional[Tensor]  # [V, 3] float32: -grad of the interpolated pre-activated density, normalised (0 where it is 0)


def extract_mesh(voxel_grid, iso_level: float, subdivisions: int = 1, colours: bool = True, normals: bool = True) -> Mesh:
    """The mesh of {sigma > iso_level} of ``voxel_grid`` (any storage, any density mode), on the grid's device."""
    if isinstance(subdivisions, bool) or not isinstance(subdivisions, (int, np.integer)) or not 1 <= int(subdivisions) <= MAX_SUBDIVISIONS:
        raise ValueError(f"subdivisions must be an integer in [1, {MAX_SUBDIVISIONS}], got {subdivisions!r}")
    iso = float(iso_level)
    if not math.isfinite(iso) or abs(iso) > float(np.finfo(np.float32).max):
        raise ValueError(f"iso_level must be a finite float32 value, got {iso_level!r}")
    m = int(subdivisions)
    lib = _lib.load()
    with torch.no_grad():
        grid = voxel_grid.to_rf_grid()  # (waits for parameters still arriving, like a render)
        dev = voxel_grid.kernel_tensors()[0].device
        stream = _marshal.stream(dev)
        tiles = lib.rf_mesh_tiles(C.byref(grid), m)
        if tiles < 0:
            _lib.check(int(tiles), "rf_mesh_tiles")
        counts = torch.empty((2, tiles), dtype=torch.int64, device=dev)
        _lib.check(lib.rf_mesh_count(C.byref(grid), m, iso, counts.data_ptr(), stream), "rf_mesh_count")
        ends = torch.cumsum(counts, dim=1)
        offsets = ends - counts
        num_vertices, num_faces = (int(v) for v in ends[:, -1].tolist())
        if num_vertices >= 2**31:
            raise ValueError(f"the mesh has {num_vertices} vertices: PLY stores int32 indices (use fewer subdivisions)")
        keys = torch.empty(num_vertices, dtype=torch.int64, device=dev)
        vertices = torch.empty((num_vertices, 3), dtype=torch.float32, device=dev)
        cols = torch.empty((num_vertices, 3), dtype=torch.float32, device=dev) if colours else None
        nrms = torch.empty((num_vertices, 3), dtype=torch.float32, device=dev) if normals else None
        face_edges = torch.empty((num_faces, 3), dtype=torch.int64, device=dev)
        if num_vertices or num_faces:
            _lib.check(
                lib.rf_mesh_emit(C.byref(grid), m, iso, offsets.data_ptr(), num_vertices, num_faces, keys.data_ptr(), vertices.data_ptr(),
                                 _marshal.ptr(cols), _marshal.ptr(nrms), face_edges.data_ptr(), stream),
                "rf_mesh_emit",
            )
        # the vertices come out in ascending edge key: a face's vertex index is the position of its edge key
        faces = torch.searchsorted(keys, face_edges)
    return Mesh(vertices, faces, cols, nrms)


def to8b(x: np.ndarray) -> np.ndarray:
    """The reference's to8b (utils/imaging_utils.py:38): clip to [0, 1], scale by 255, truncate."""
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def write_ply(mesh: Mesh, path: str) -> None:
    """Binary little-endian PLY: vertex x y z, nx ny nz (float), red green blue (uchar); face list (uchar count, int indices).
    Missing normals are written as 0, missing colours as 255."""
    v = mesh.vertices.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
    f = mesh.faces.detach().cpu().numpy().reshape(-1, 3)
    n = len(v)
    if n >= 2**31:
        raise ValueError("PLY stores int32 vertex indices")
    nrm = np.zeros((n, 3), "<f4") if mesh.normals is None else mesh.normals.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
    rgb = np.full((n, 3), 255, np.uint8) if mesh.colours is None else to8b(mesh.colours.detach().cpu().numpy().reshape(-1, 3))
    vdt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                    ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    vert = np.empty(n, vdt)
    for i, name in enumerate(("x", "y", "z")):
        vert[name] = v[:, i]
    for i, name in enumerate(("nx", "ny", "nz")):
        vert[name] = nrm[:, i]
    for i, name in enumerate(("red", "green", "blue")):
        vert[name] = rgb[:, i]
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    face = np.empty(len(f), fdt)
    face["n"] = 3
    face["i"] = f.astype("<i4")
    header = (
        "ply\nformat binary_little_endian 1.0\n"
        f"element vertex {n}\n"
        "property float x\nproperty float y\nproperty float z\n"
        "property float nx\nproperty float ny\nproperty float nz\n"
        "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        f"element face {len(f)}\n"
        "property list uchar int vertex_indices\n"
        "end_header\n"
    )
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


def read_ply(path: str):
    """Parse a PLY written by ``write_ply``: (vertices [V,3] f32, normals [V,3] f32, colours [V,3] uint8, faces [T,3] int64)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = nf = None
    for line in lines:
        if line.startswith("element vertex "):
            nv = int(line.split()[-1])
        elif line.startswith("element face "):
            nf = int(line.split()[-1])
    vdt = np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])
    fdt = np.dtype([("k", "u1"), ("i", "<i4", (3,))])
    vert = np.frombuffer(data, vdt, count=nv, offset=end)
    face = np.frombuffer(data, fdt, count=nf, offset=end + nv * vdt.itemsize)
    if end + nv * vdt.itemsize + nf * fdt.itemsize != len(data) or (nf and not (face["k"] == 3).all()):
        raise ValueError(f"{path}: malformed body")
    return vert["p"].copy(), vert["n"].copy(), vert["c"].copy(), face["i"].astype(np.int64)
