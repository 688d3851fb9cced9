"""Mesh export: a voxel grid leaves the package as a coloured triangle mesh.

``density_lattice`` samples the rendered density field on a regular lattice (``holo_density_lattice``), ``surface_nets``
extracts the isosurface of any lattice field on the GPU (``holo_surface_count`` / ``holo_surface_emit``: one vertex per
crossed cell, fixed output order, no atomics), ``vertex_attributes`` evaluates the implicit function's analytic normals and
colours at the vertices, ``extract_mesh`` composes the three, ``save_ply`` / ``load_ply`` write and read binary PLY with
numpy only.  The algorithm is pinned in ``include/holo_abi.h``; build-side addition (the reference makes meshes from depth
maps only)."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, runtime

LATTICE_MIN, LATTICE_MAX = 2, 1024


def half_extent(resol: int, volume_extent: float) -> float:
    """The renderer's half extent (R-1)/R * volume_extent / 2, in the library's float32 arithmetic."""
    return float(np.float32(0.5) * np.float32(resol - 1) * (np.float32(volume_extent) / np.float32(resol)))


def default_density_level(voxel_size: float, opacity_level: float = 0.5) -> float:
    """ln 2 / voxel_size * (-log2(1 - opacity_level)): the density at which one voxel's length of material reaches
    ``opacity_level`` (1 - exp(-density * voxel_size) = opacity_level)."""
    if not 0.0 < opacity_level < 1.0:
        raise ValueError(f"opacity_level must be in (0, 1), got {opacity_level}")
    return math.log(2.0) / voxel_size * (-math.log2(1.0 - opacity_level))


def _check_resolution(m) -> int:
    if isinstance(m, bool) or int(m) != m or not LATTICE_MIN <= int(m) <= LATTICE_MAX:
        raise ValueError(f"the lattice has {LATTICE_MIN} <= resolution <= {LATTICE_MAX} points per axis, got {m!r}")
    return int(m)


def _grid_of(fn, grid: torch.Tensor) -> torch.Tensor:
    if grid.dim() == 5 and grid.shape[0] != 1:
        raise ValueError(f"one grid at a time: got a batch of {grid.shape[0]}")
    if tuple(grid.shape) != (1, fn.n_hidden, fn.resol, fn.resol, fn.resol):
        raise ValueError(f"voxel grid must be (1,{fn.n_hidden},{fn.resol}^3), got {tuple(grid.shape)}")
    runtime.require_device(grid, "mesh export")
    return grid.detach().contiguous().float()


def density_lattice(implicit_function, voxel_grid_features: torch.Tensor, resolution: int) -> torch.Tensor:
    """Density of ``implicit_function`` (a ``HoloVoxelGridImplicitFunction``) on ``voxel_grid_features`` at the
    ``resolution``^3 points of the regular lattice over the grid's volume: (m, m, m) float32 indexed [z][y][x], the value
    the implicit function returns at the float32 point ``i * spacing - h`` of every axis (include/holo_abi.h)."""
    m = _check_resolution(resolution)
    grid = _grid_of(implicit_function, voxel_grid_features)
    dev = grid.device
    L, h = runtime.lib(), implicit_function.native_handle(dev)
    field = torch.empty(m, m, m, dtype=torch.float32, device=dev)
    ws = runtime.workspace(implicit_function, dev, L.holo_density_lattice_workspace_bytes(h))
    _lib.check(L, L.holo_density_lattice(h, runtime.ptr(grid), m, runtime.ptr(field), runtime.ptr(ws), ws.numel(),
                                         runtime.stream_ptr(dev)), "holo_density_lattice")
    return field


def surface_nets(field: torch.Tensor, level: float, half_extent: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Surface nets of the (m, m, m) lattice ``field`` ([z][y][x], spanning [-half_extent, half_extent] per axis) at
    ``level``: ``verts (V, 3) float32`` world positions and ``faces (F, 3) int32``, closed (the outermost lattice layer is
    never inside), normals towards lower values, in the fixed order of include/holo_abi.h.  The host reads the two counts
    between the counting and the emitting call to size the outputs: one device synchronisation, here and not in the library."""
    if field.dim() != 3 or not field.shape[0] == field.shape[1] == field.shape[2]:
        raise ValueError(f"field must be (m, m, m), got {tuple(field.shape)}")
    m = _check_resolution(field.shape[0])
    if not math.isfinite(level) or not (math.isfinite(half_extent) and half_extent > 0):
        raise ValueError("level must be finite and half_extent > 0")
    runtime.require_device(field, "surface_nets")
    field = field.detach().contiguous().float()
    dev = field.device
    L, ctx, st = runtime.lib(), runtime.ctx(dev), runtime.stream_ptr(dev)
    ws = torch.empty(int(L.holo_surface_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    _lib.check(L, L.holo_surface_count(ctx, runtime.ptr(field), m, float(level), runtime.ptr(counts), runtime.ptr(ws),
                                       ws.numel(), st), "holo_surface_count")
    n_verts, n_tris = (int(v) for v in counts.tolist())  # (synchronises)
    verts = torch.empty(n_verts, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(n_tris, 3, dtype=torch.int32, device=dev)
    if n_verts == 0 and n_tris == 0:
        return verts, faces
    _lib.check(L, L.holo_surface_emit(ctx, runtime.ptr(field), m, float(level), float(half_extent), runtime.ptr(verts),
                                      n_verts, runtime.ptr(faces), n_tris, runtime.ptr(ws), ws.numel(), st),
               "holo_surface_emit")
    if ws[:8].view(torch.int32).tolist() != [0, 0]:
        raise _lib.HoloError("holo_surface_emit: the mesh did not fit the counted capacities")
    return verts, faces


def vertex_attributes(implicit_function, voxel_grid_features: torch.Tensor, verts: torch.Tensor,
                      colours: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Outward unit normals (the negated analytic gradient direction of the density, ``holo_implicit_normals``; zero where
    the gradient is) and, with ``colours``, the implicit function's colour in [0, 1] at every vertex for a ray arriving
    head-on, i.e. travelling along the gradient (``holo_implicit_eval``, one direction per point)."""
    grid = _grid_of(implicit_function, voxel_grid_features)
    dev = grid.device
    pts = verts.detach().reshape(-1, 3).contiguous().float()
    n = pts.shape[0]
    grad_dir = torch.zeros(n, 3, dtype=torch.float32, device=dev)
    col = torch.zeros(n, 3, dtype=torch.float32, device=dev) if colours else None
    if n == 0:
        return grad_dir, col
    L, h, st = runtime.lib(), implicit_function.native_handle(dev), runtime.stream_ptr(dev)
    nbytes = max(L.holo_implicit_workspace_bytes(h, n, 1, 0), L.holo_render_workspace_bytes(h, 1, 0))
    ws = runtime.workspace(implicit_function, dev, nbytes)
    _lib.check(L, L.holo_implicit_normals(h, runtime.ptr(grid), runtime.ptr(pts), n, runtime.ptr(grad_dir), runtime.ptr(ws),
                                          ws.numel(), st), "holo_implicit_normals")
    if colours:
        dens = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(L, L.holo_implicit_eval(h, runtime.ptr(grid), runtime.ptr(pts), runtime.ptr(grad_dir), n, 1,
                                           runtime.ptr(dens), runtime.ptr(col), runtime.ptr(ws), ws.numel(), st),
                   "holo_implicit_eval")
    return -grad_dir, col


def extract_mesh(implicit_function, voxel_grid_features: torch.Tensor, resolution: Optional[int] = None,
                 opacity_level: float = 0.5, density_level: Optional[float] = None,
                 colours: bool = True) -> Dict[str, object]:
    """The isosurface ``density = density_level`` of the field the renderer integrates, as a closed coloured mesh:
    ``verts (V, 3) float32``, ``faces (F, 3) int32``, ``normals (V, 3)`` (outward), ``colours (V, 3)`` in [0, 1] (None
    without ``colours``) and the ``density_level`` used.

    ``resolution`` None means ``2 R - 1`` lattice points per axis (the voxel centres and the points between them).
    ``density_level`` None means ``default_density_level(voxel_size, opacity_level)``; it must be > 0 (there the final
    LeakyReLU of the density is the identity).  Whether ``opacity_level = 0.5`` suits a trained checkpoint has not been
    measured: no checkpoint is available to this build."""
    fn = implicit_function
    m = _check_resolution(2 * fn.resol - 1 if resolution is None else resolution)
    if density_level is None:
        density_level = default_density_level(float(fn.volume_extent) / fn.resol, opacity_level)
    density_level = float(density_level)
    if not (math.isfinite(density_level) and density_level > 0.0):
        raise ValueError(f"density_level must be > 0, got {density_level}")
    field = density_lattice(fn, voxel_grid_features, m)
    verts, faces = surface_nets(field, density_level, half_extent(fn.resol, fn.volume_extent))
    normals, col = vertex_attributes(fn, voxel_grid_features, verts, colours)
    return {"verts": verts, "faces": faces, "normals": normals, "colours": col, "density_level": density_level}


# ---- PLY (binary little-endian 1.0): x y z nx ny nz float32, red green blue uchar; faces `list uchar int vertex_indices`
_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                          ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
_PLY_PROPERTIES = ["property float x", "property float y", "property float z", "property float nx", "property float ny",
                   "property float nz", "property uchar red", "property uchar green", "property uchar blue"]


def _numpy(a, dtype, cols):
    if a is not None and hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(-1, cols))


def save_ply(path: str, verts, faces, normals=None, colours=None) -> str:
    """Writes the mesh (tensors or arrays) as binary little-endian PLY.  Missing normals are written as zeros, missing
    colours as mid grey; colours in [0, 1] are rounded to 8 bits."""
    v = _numpy(verts, np.float32, 3)
    f = _numpy(faces, np.int32, 3)
    nrm = _numpy(normals, np.float32, 3) if normals is not None else np.zeros_like(v)
    col = _numpy(colours, np.float32, 3) if colours is not None else np.full_like(v, 0.5)
    if nrm.shape != v.shape or col.shape != v.shape:
        raise ValueError("normals and colours must have one row per vertex")
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("faces index past the vertices")
    rows = np.zeros(len(v), _VERTEX_DTYPE)
    for k, name in enumerate(("x", "y", "z")):
        rows[name] = v[:, k]
        rows["n" + name] = nrm[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rows[name] = np.rint(np.clip(col[:, k], 0.0, 1.0) * 255.0).astype(np.uint8)
    tris = np.zeros(len(f), _FACE_DTYPE)
    tris["n"] = 3
    tris["v"] = f
    header = ["ply", "format binary_little_endian 1.0", "comment holo_diffusion_amd surface nets",
              f"element vertex {len(v)}", *_PLY_PROPERTIES, f"element face {len(f)}",
              "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rows.tobytes())
        fh.write(tris.tobytes())
    return path


def load_ply(path: str) -> Dict[str, np.ndarray]:
    """Reads the subset ``save_ply`` writes: ``verts``, ``normals`` (float32), ``colours`` (float32, byte / 255) and
    ``faces`` (int32).  Anything else is refused."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = [ln for ln in data[:end].decode("ascii").split("\n") if ln and not ln.startswith("comment")]
    body = data[end + len(b"end_header\n"):]
    if (len(lines) != 14 or lines[1] != "format binary_little_endian 1.0" or lines[3:12] != _PLY_PROPERTIES
            or lines[13] != "property list uchar int vertex_indices" or not lines[2].startswith("element vertex ")
            or not lines[12].startswith("element face ")):
        raise ValueError(f"{path}: only the layout written by save_ply is read")
    nv, nf = int(lines[2].split()[2]), int(lines[12].split()[2])
    if len(body) != nv * _VERTEX_DTYPE.itemsize + nf * _FACE_DTYPE.itemsize:
        raise ValueError(f"{path}: truncated or oversized body")
    rows = np.frombuffer(body, _VERTEX_DTYPE, nv)
    tris = np.frombuffer(body, _FACE_DTYPE, nf, offset=nv * _VERTEX_DTYPE.itemsize)
    if nf and (tris["n"] != 3).any():
        raise ValueError(f"{path}: only triangles are read")
    return {"verts": np.stack([rows["x"], rows["y"], rows["z"]], axis=1).astype(np.float32).reshape(-1, 3),
            "normals": np.stack([rows["nx"], rows["ny"], rows["nz"]], axis=1).astype(np.float32).reshape(-1, 3),
            "colours": (np.stack([rows["red"], rows["green"], rows["blue"]], axis=1).astype(np.float32) / np.float32(255.0)
                        ).reshape(-1, 3),
            "faces": tris["v"].astype(np.int32).reshape(-1, 3)}
