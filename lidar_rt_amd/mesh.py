"""Surface meshes from posed range images through ``csrc/liblrt_mesh.so``: projective TSDF fusion into a dense grid, then marching cubes.

    grid = TsdfGrid(origin, voxel, dims, trunc=None, device="cuda", intensity=True)  # tsdf, weight, intensity: all zeros
    integrate(grid, depth, mask, sensor2world, inclination, data_type="KITTI", sensor2ego=None, intensity=None, min_depth=0.0, max_depth=80.0)
    mesh = extract(grid, min_weight=1)                                        # Mesh: vertices (V, 3) f32 in the grid frame, faces (T, 3) i32, ...
    write_ply(path, mesh); ply = read_ply(path)                               # binary little-endian, world x y z as doubles

    python -m lidar_rt_amd.mesh --data DIR --out mesh.ply [--voxel 0.1] [--trunc M] [--frames train|test|all] [--static-only] [--device cpu]
                                [--sweep stored [--sweep-ref 0.5] [--sweep-direction cw]]

``--sweep stored`` fuses under the sweep model: each frame's stored twist (and column times) through ``sweep_fuse.integrate_sweep``, so that the
motion of the sensor within a sweep does not shear the surface.

``include/lrt_mesh.h`` states every rule and ``csrc/lrt_mesh_math.h`` is its text for the device and the host.

* The grid is dense, axis-aligned and C-order ``(X, Y, Z)``; voxel ``(i, j, k)`` has its centre at ``(float) (voxel (i + 0.5))`` per axis in the grid
  frame, which sits at ``origin`` (float64) in the world: ``grid2sensor = inverse(sensor2world) @ translate(origin)``, computed in float64 on the
  host.  "The image is the index": every voxel centre is projected into every range image by ``range_image``'s own rule (``lrt_project_math.h``).
* ``integrate``: a voxel takes part in a frame iff its centre is a kept point of the projection, the pixel's mask is set and its depth > 0;
  ``sdf = depth - r32`` (skipped below ``-trunc``), ``d = min(1, sdf / trunc)``; the running means ``D``, ``I`` and the count ``Wt`` are float64
  across the frames of one call and rounded to float32 once at its end.  One launch per call.  The state is updated in place.
* ``extract``: the vertices are the emitted edges (crossed, touching an active cell) ascending by ``(voxel, axis)``; the faces come from
  ``mc_table()`` -- GENERATED from a stated rule, not typed in -- ascending by cell.  Normals ``(v1 - v0) x (v2 - v0)`` point from negative to
  positive tsdf, towards free space.  At most four launches and one host read of the two totals.
* HIP tensors go through the library; a missing library is a ``MeshError``, not a quiet fall-back.  CPU tensors go to the numpy twins
  (``integrate_reference``, ``extract_reference``), which are equal to the device bit for bit while ``range_image``'s ``margin >= 1e-9``
  (only ``atan2`` and ``hypot`` may differ in the last bit between the device and the host); ``integrate_reference`` returns that margin.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time
from collections import Counter
from types import SimpleNamespace

import numpy as np
import torch

from . import range_image as ri

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LRT_MESH_LIB") or os.path.join(HERE, "csrc", "liblrt_mesh.so")
TABLE_PATH = os.path.join(HERE, "csrc", "lrt_mesh_tables.h")
EXPORTS = ("lrt_mesh_abi_version", "lrt_mesh_last_error", "lrt_mesh_integrate", "lrt_mesh_work_bytes", "lrt_mesh_count", "lrt_mesh_write")  # include/lrt_mesh.h
ABI_VERSION = 1
BLOCK = 256                                                                  # LRT_MESH_BLOCK
SCAN_PASS = 256                                                              # LRT_MESH_SCAN_PASS
MAX_VOXELS = 2 ** 31 - 1                                                     # LRT_MESH_MAX_VOXELS
MAX_FRAMES = 65536                                                           # LRT_MESH_MAX_FRAMES
MAX_OUTPUT = 2 ** 31 - 1                                                     # LRT_MESH_MAX_OUTPUT
DEFAULT_MAX_VOXELS = 2 ** 28

_lib = None


class MeshError(RuntimeError):
    pass


def load():
    """Load liblrt_mesh.so (after torch, so that both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MeshError(f"{LIB_PATH} is missing: build it with `python -m lidar_rt_amd.build` (hipcc --offload-arch=gfx950). "
                        "mesh has no fall-back on a HIP device.")
    lib = C.CDLL(LIB_PATH)
    vp, ci, ll, d = C.c_void_p, C.c_int, C.c_longlong, C.c_double
    lib.lrt_mesh_abi_version.restype = ci
    lib.lrt_mesh_last_error.restype = C.c_char_p
    lib.lrt_mesh_integrate.restype = ci
    lib.lrt_mesh_integrate.argtypes = [ci, ci, ci, ci, d, d, vp, vp, vp, ll, vp, ci, ci, vp, vp, vp, vp, ci, d, d, d, d, vp]
    lib.lrt_mesh_work_bytes.restype = ll
    lib.lrt_mesh_work_bytes.argtypes = [ci, ci, ci]
    lib.lrt_mesh_count.restype = ci
    lib.lrt_mesh_count.argtypes = [ci, ci, ci, ci, vp, vp, ci, vp, ll, vp, vp]
    lib.lrt_mesh_write.restype = ci
    lib.lrt_mesh_write.argtypes = [ci, ci, ci, ci, d, vp, vp, vp, ll, ll, ll, vp, vp, vp, vp]
    if lib.lrt_mesh_abi_version() != ABI_VERSION:
        raise MeshError("liblrt_mesh.so ABI version mismatch; rebuild with `python -m lidar_rt_amd.build --force`")
    _lib = lib
    return lib


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ---- 1. the triangle table ----------------------------------------------------------------------------------------------------------------------------------
#
# Corner n of a cell sits at offset (n & 1, n >> 1 & 1, n >> 2 & 1); edge e = 4 a + o runs along axis a from the corner whose offsets along the other
# two axes (ascending) are the bits of o (lrt_mesh_math.h: mh_edge_corner).

def corner_pos(n):
    return np.array([n & 1, n >> 1 & 1, n >> 2 & 1], np.float64)


def edge_corners(e):
    """(the corner edge e starts from, the corner it ends at)."""
    a, o = e >> 2, e & 3
    b, c = (1, 2) if a == 0 else ((0, 2) if a == 1 else (0, 1))
    n0 = ((o & 1) << b) | ((o >> 1 & 1) << c)
    return n0, n0 | (1 << a)


EDGE_CORNER = np.array([edge_corners(e)[0] for e in range(12)], np.int64)


def _on_face(e, face):
    """Does edge e lie on face (axis, side)?"""
    a, s = face
    return (e >> 2) != a and (edge_corners(e)[0] >> a & 1) == s


def _face_of_segment(e1, e2):
    """The face (axis, side) that two edges of a segment share."""
    f, = [(a, s) for a in range(3) for s in (0, 1) if _on_face(e1, (a, s)) and _on_face(e2, (a, s))]
    return f


def mc_table():
    """[config] -> [(e0, e1, e2), ...] for the 256 configurations (bit n set iff corner n has tsdf < 0), from this rule:

    1. on each face of the cube the crossed edges are joined into segments;
    2. on an ambiguous face (the inside corners on a diagonal) each inside corner is cut off on its own;
    3. each segment is directed so that, seen from outside the cube, the inside (negative) corners it cuts off lie on its right -- the segments then
       chain into cycles whose fan normals point from negative to positive tsdf;
    4. each cycle is fan-triangulated from its lowest edge number that lies on no face the cycle crosses twice (that is: on no ambiguous face
       whose two segments both belong to it), going round the cycle from there; cycles in ascending order of their lowest edge.

    Two cells that share a face apply the same rule to it, so the surface is watertight by construction.  The exception in 4 is what makes that
    true of the fan's chords as well: a chord from an apex on a face that the cycle crosses twice lies in that face, and the cell on the other side,
    whose cycle crosses it twice too, would draw the same chord -- an edge of four triangles.  No chord lies in any other face."""
    table = []
    for cfg in range(256):
        neg = [(cfg >> n) & 1 == 1 for n in range(8)]
        crossed = [e for e in range(12) if neg[edge_corners(e)[0]] != neg[edge_corners(e)[1]]]
        nxt = {}
        for a in range(3):
            for s in (0, 1):
                normal = np.zeros(3)
                normal[a] = 2.0 * s - 1.0
                fe = [e for e in crossed if (e >> 2) != a and (edge_corners(e)[0] >> a & 1) == s]
                if not fe:
                    continue
                inside = [n for n in range(8) if (n >> a & 1) == s and neg[n]]
                if len(fe) == 2:
                    pairs = [(fe[0], fe[1], inside[0])]
                else:                                                      # four crossed edges: the two inside corners lie on a diagonal
                    assert len(fe) == 4 and len(inside) == 2
                    pairs = [tuple(e for e in fe if n in edge_corners(e)) + (n,) for n in inside]
                for e1, e2, ref in pairs:
                    m1 = 0.5 * (corner_pos(edge_corners(e1)[0]) + corner_pos(edge_corners(e1)[1]))
                    m2 = 0.5 * (corner_pos(edge_corners(e2)[0]) + corner_pos(edge_corners(e2)[1]))
                    side = float(np.cross(m2 - m1, normal) @ (corner_pos(ref) - m1))
                    src, dst = (e1, e2) if side > 0 else (e2, e1)
                    assert src not in nxt
                    nxt[src] = dst
        assert sorted(nxt) == crossed and sorted(nxt.values()) == crossed
        tris, seen = [], set()
        for e in crossed:
            if e in seen:
                continue
            cyc = [e]
            x = nxt[e]
            while x != e:
                cyc.append(x)
                x = nxt[x]
            seen.update(cyc)
            # the apex: the lowest edge on no face that the cycle crosses twice (a face's two segments in one cycle: a chord from an apex on that
            # face would lie in it, and the cell on its other side would draw the same chord)
            twice = [f for f, n in Counter(_face_of_segment(cyc[k], cyc[(k + 1) % len(cyc)]) for k in range(len(cyc))).items() if n > 1]
            apex = min(x for x in cyc if not any(_on_face(x, f) for f in twice))
            r = cyc.index(apex)
            cyc = cyc[r:] + cyc[:r]
            tris += [(cyc[0], cyc[k], cyc[k + 1]) for k in range(1, len(cyc) - 1)]
        table.append(tris)
    return table


def table_arrays(table=None):
    """(ntri (256,) int64, tri (256, max_tri, 3) int64, -1 padded) of a table (default: mc_table())."""
    table = mc_table() if table is None else table
    mt = max(len(t) for t in table)
    ntri = np.array([len(t) for t in table], np.int64)
    tri = np.full((256, mt, 3), -1, np.int64)
    for c, t in enumerate(table):
        if t:
            tri[c, :len(t)] = np.asarray(t, np.int64)
    return ntri, tri


def table_header(table=None):
    """The text of csrc/lrt_mesh_tables.h for a table (default: mc_table())."""
    ntri, tri = table_arrays(table)
    mt = tri.shape[1]
    out = ["// lrt_mesh_tables.h -- GENERATED by lidar_rt_amd.mesh.table_header() from mc_table()'s rule; do not edit.  tests/test_mesh.py regenerates",
           "// it and compares.  mh_ntri[c]: the triangles of configuration c; mh_tri[c][3 m + q]: edge q of its triangle m (-1 pads).",
           "#ifndef LRT_MESH_TABLES_H_INCLUDED", "#define LRT_MESH_TABLES_H_INCLUDED", "",
           "#ifndef MH_TABLE_SPACE", "#define MH_TABLE_SPACE", "#endif", "",
           f"#define MH_MAX_TRI {mt}", "",
           "MH_TABLE_SPACE static const unsigned char mh_ntri[256] = {"]
    for r in range(0, 256, 32):
        out.append("    " + ", ".join(str(int(x)) for x in ntri[r:r + 32]) + ",")
    out += ["};", "", "MH_TABLE_SPACE static const signed char mh_tri[256][3 * MH_MAX_TRI] = {"]
    for c in range(256):
        out.append("    {" + ", ".join(str(int(x)) for x in tri[c].reshape(-1)) + "},")
    out += ["};", "", "#endif /* LRT_MESH_TABLES_H_INCLUDED */", ""]
    return "\n".join(out)


# ---- 2. the grid --------------------------------------------------------------------------------------------------------------------------------------------

class TsdfGrid(SimpleNamespace):
    """origin (3,) float64 [world], voxel, dims (X, Y, Z), trunc, and the state: tsdf (X, Y, Z) float32, weight int32 (0 = unobserved), intensity
    float32 or None.  A fresh grid is all zeros."""

    def __init__(self, origin, voxel, dims, trunc=None, device="cpu", intensity=True):
        origin = np.asarray(origin, np.float64).reshape(-1)
        dims = tuple(int(x) for x in dims)
        voxel = float(voxel)
        trunc = 3.0 * voxel if trunc is None else float(trunc)
        if origin.size != 3 or not np.all(np.isfinite(origin)):
            raise MeshError(f"TsdfGrid: origin {origin.tolist()} (three finite numbers)")
        if len(dims) != 3 or min(dims) < 1 or math.prod(dims) > MAX_VOXELS:
            raise MeshError(f"TsdfGrid: dims {dims} (three, each at least 1, X Y Z at most {MAX_VOXELS})")
        if not (voxel > 0.0 and math.isfinite(voxel)) or not (trunc > 0.0 and math.isfinite(trunc)):
            raise MeshError(f"TsdfGrid: voxel {voxel}, trunc {trunc} (both positive)")
        dev = torch.device(device)
        super().__init__(origin=origin, voxel=voxel, dims=dims, trunc=trunc,
                         tsdf=torch.zeros(dims, dtype=torch.float32, device=dev), weight=torch.zeros(dims, dtype=torch.int32, device=dev),
                         intensity=torch.zeros(dims, dtype=torch.float32, device=dev) if intensity else None)

    @property
    def device(self):
        return self.tsdf.device

    def to(self, device):
        g = TsdfGrid(self.origin, self.voxel, self.dims, self.trunc, "cpu", intensity=False)
        g.tsdf, g.weight = self.tsdf.to(device), self.weight.to(device)
        g.intensity = None if self.intensity is None else self.intensity.to(device)
        return g

    def clone(self):
        g = self.to(self.device)
        g.tsdf, g.weight = g.tsdf.clone(), g.weight.clone()
        g.intensity = None if g.intensity is None else g.intensity.clone()
        return g


def centres(voxel, n):
    """(n,) float32: (float) (voxel (i + 0.5)), one rounding of a float64 product (mh_centre)."""
    return (float(voxel) * (np.arange(n, dtype=np.float64) + 0.5)).astype(np.float32)


def grid2sensor(origin, sensor2world):
    """(F, 3, 4) float64 = inverse(sensor2world) @ translate(origin), on the host."""
    S = np.asarray(sensor2world.detach().cpu().numpy() if torch.is_tensor(sensor2world) else sensor2world, np.float64)
    if S.ndim == 2:
        S = S[None]
    if S.ndim != 3 or S.shape[1:] != (4, 4):
        raise MeshError(f"integrate: sensor2world must be (F, 4, 4) (it is {tuple(S.shape)})")
    tr = np.eye(4)
    tr[:3, 3] = np.asarray(origin, np.float64)
    return np.ascontiguousarray(np.stack([np.linalg.inv(s) @ tr for s in S])[:, :3, :]) if len(S) else np.zeros((0, 3, 4))


def _frames(grid, depth, mask, sensor2world, inclination, data_type, sensor2ego, intensity, min_depth, max_depth, transforms=None):
    """The checked arguments of a call: (depth, mask uint8, intensity or None (F, H, W) on the grid's device, T (F, 3, 4), inc, off, yaw).
    ``transforms``: the (F, 3, 4) float64 grid2sensor to use as they are, instead of deriving them from ``sensor2world``."""
    if not isinstance(grid, TsdfGrid):
        raise MeshError("integrate: grid must be a TsdfGrid")
    dev = grid.device
    if not torch.is_tensor(depth) or depth.dtype != torch.float32 or depth.dim() not in (2, 3) or depth.device != dev:
        raise MeshError(f"integrate: depth must be a float32 (H, W) or (F, H, W) tensor on {dev}")
    depth = depth.detach().contiguous()
    depth = depth if depth.dim() == 3 else depth[None]
    F, H, W = (int(x) for x in depth.shape)
    if F > MAX_FRAMES or H < 1 or W < 1 or F * H * W > MAX_VOXELS:
        raise MeshError(f"integrate: {F} frames of {H} x {W} pixels (at most {MAX_FRAMES} frames, F H W at most {MAX_VOXELS})")
    if not torch.is_tensor(mask) or tuple(mask.shape[-2:]) != (H, W) or mask.numel() != F * H * W or mask.device != dev:
        raise MeshError(f"integrate: mask must be an ({F}, {H}, {W}) tensor on {dev}")
    mask = mask.detach().reshape(F, H, W)
    mask = mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else (mask != 0).to(torch.uint8).contiguous()
    if (grid.intensity is None) != (intensity is None):
        raise MeshError("integrate: the grid's intensity and the frames' intensity go together (both or neither)")
    if intensity is not None:
        if not torch.is_tensor(intensity) or intensity.dtype != torch.float32 or intensity.numel() != F * H * W or intensity.device != dev:
            raise MeshError(f"integrate: intensity must be a float32 ({F}, {H}, {W}) tensor on {dev}")
        intensity = intensity.detach().reshape(F, H, W).contiguous()
    T = grid2sensor(grid.origin, sensor2world) if transforms is None else np.ascontiguousarray(np.asarray(transforms, np.float64).reshape(-1, 3, 4))
    if T.shape[0] != F:
        raise MeshError(f"integrate: {T.shape[0]} poses for {F} frames")
    inc = ri._host_array("inclination", inclination, np.float64).reshape(-1)
    if inc.size != 2 and (inc.size != H or H < 3):
        raise MeshError(f"integrate: inclination holds 2 bounds or one angle per row of at least 3 ({H}); it holds {inc.size}")
    d = np.diff(inc)
    if not np.all(np.isfinite(inc)) or not (np.all(d > 0) or np.all(d < 0)):
        raise MeshError("integrate: the inclination must be finite and strictly monotonic")
    off, yaw = ri.convention(data_type, sensor2ego)
    min_depth, max_depth = float(min_depth), float(max_depth)
    if not (0.0 <= min_depth < max_depth <= ri.FLT_MAX):
        raise MeshError(f"integrate: depths ({min_depth}, {max_depth}] (0 <= min < max)")
    return depth, mask, intensity, T, inc, off, yaw, min_depth, max_depth


def project_centres(cen, H, W, inclination, data_type, sensor2ego, T, min_depth, max_depth):
    """``project_points_reference``'s own decision for the voxel centres ``cen`` (N, 3) float32 as points under one transform T (3, 4):
    (pixel (N, 2) int32 [w, h], r32 (N) float32, drop (N) uint8, margin).  The function is called as it is; its results are not changed."""
    r = ri.project_points_reference(cen, H, W, inclination, None, data_type, sensor2ego, T, max_depth, min_depth, True)
    return r.pixel.numpy(), r.range_bits.view(np.float32), r.drop.numpy(), r.margin


# ---- 3. integration -----------------------------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def integrate_reference(grid, depth, mask, sensor2world, inclination, data_type="KITTI", sensor2ego=None, intensity=None, min_depth=0.0,
                        max_depth=80.0, transforms=None):
    """The numpy twin of ``integrate`` on a grid of CPU tensors, updated in place.  Returns ``margin``: the smallest distance of any voxel centre
    that reached the projection's view test from a rounding boundary (``range_image.project_points_reference``), over the frames of the call.
    ``transforms``: the (F, 3, 4) float64 grid2sensor of the frames, used as they are (``sensor2world`` is not read then): what
    ``map_registration.align_to_grid`` returns as ``G``."""
    if grid.device.type != "cpu":
        raise MeshError("integrate_reference: the twin works on a grid of CPU tensors")
    depth, mask, intensity, T, inc, off, yaw, min_depth, max_depth = _frames(grid, depth, mask, sensor2world, inclination, data_type, sensor2ego,
                                                                             intensity, min_depth, max_depth, transforms)
    F, H, W = depth.shape
    X, Y, Z = grid.dims
    cx, cy, cz = centres(grid.voxel, X), centres(grid.voxel, Y), centres(grid.voxel, Z)
    cen = np.stack(np.meshgrid(cx, cy, cz, indexing="ij"), -1).reshape(-1, 3)
    D = grid.tsdf.numpy().reshape(-1).astype(np.float64)
    Wt = grid.weight.numpy().reshape(-1).astype(np.float64)
    I = grid.intensity.numpy().reshape(-1).astype(np.float64) if intensity is not None else None
    seen = np.zeros(D.shape, bool)
    margin = math.inf
    trunc = float(grid.trunc)
    for f in range(F):
        pix, r32, drop, m = project_centres(cen, H, W, inc, data_type, sensor2ego, T[f], min_depth, max_depth)
        margin = min(margin, m)
        kept = np.nonzero(drop == ri.KEEP)[0]
        p = pix[kept, 1].astype(np.int64) * W + pix[kept, 0]
        dimg = depth[f].numpy().reshape(-1)[p]
        ok = (mask[f].numpy().reshape(-1)[p] != 0) & (dimg > 0)
        sdf = dimg.astype(np.float64) - r32[kept].astype(np.float64)
        ok &= ~(sdf < -trunc)
        v, sdf, p = kept[ok], sdf[ok], p[ok]
        s = sdf / trunc
        d = np.where(s < 1.0, s, 1.0)
        wt = Wt[v]
        D[v] = (wt * D[v] + d) / (wt + 1.0)
        if I is not None:
            I[v] = (wt * I[v] + intensity[f].numpy().reshape(-1)[p].astype(np.float64)) / (wt + 1.0)
        Wt[v] = wt + 1.0
        seen[v] = True
    ts, we = grid.tsdf.numpy().reshape(-1), grid.weight.numpy().reshape(-1)
    ts[seen] = D[seen].astype(np.float32)
    we[seen] = Wt[seen].astype(np.int32)
    if I is not None:
        grid.intensity.numpy().reshape(-1)[seen] = I[seen].astype(np.float32)
    return margin


def _upload(a: np.ndarray, dev) -> torch.Tensor:
    """A small host array on the device without a host wait: through pinned memory, which the allocator keeps until the copy has run."""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


@torch.no_grad()
def integrate(grid, depth, mask, sensor2world, inclination, data_type="KITTI", sensor2ego=None, intensity=None, min_depth=0.0, max_depth=80.0):
    """Fuse F posed range images into ``grid`` in place (see the module text): ``depth`` (F, H, W) or (H, W) float32, ``mask`` of the same shape,
    ``sensor2world`` (F, 4, 4) host data, ``intensity`` as ``depth`` iff the grid holds one.  One launch on a HIP device (none for F == 0); a CPU
    grid goes to ``integrate_reference`` and its margin is returned (None on a HIP device)."""
    if isinstance(grid, TsdfGrid) and grid.device.type != "cuda":
        return integrate_reference(grid, depth, mask, sensor2world, inclination, data_type, sensor2ego, intensity, min_depth, max_depth)
    depth, mask, intensity, T, inc, off, yaw, min_depth, max_depth = _frames(grid, depth, mask, sensor2world, inclination, data_type, sensor2ego,
                                                                             intensity, min_depth, max_depth)
    lib = load()
    dev = grid.device
    F, H, W = depth.shape
    X, Y, Z = grid.dims
    for name in ("tsdf", "weight") + (("intensity",) if grid.intensity is not None else ()):
        if not getattr(grid, name).is_contiguous():
            raise MeshError(f"integrate: the grid's {name} must be contiguous")
    if F == 0:
        return None                                                            # nothing to fuse: no launch
    d_T, d_inc = _upload(T, dev), _upload(inc, dev)
    with torch.cuda.device(dev):
        rc = lib.lrt_mesh_integrate(dev.index, X, Y, Z, grid.voxel, grid.trunc, grid.tsdf.data_ptr(), grid.weight.data_ptr(),
                                    None if grid.intensity is None else grid.intensity.data_ptr(), F, d_T.data_ptr(), H, W, depth.data_ptr(),
                                    mask.data_ptr(), None if intensity is None else intensity.data_ptr(), d_inc.data_ptr(), int(inc.size), off, yaw,
                                    min_depth, max_depth, _stream(dev))
    if rc != 0:
        raise MeshError(f"lrt_mesh_integrate failed ({rc}): {lib.lrt_mesh_last_error().decode()}")
    return None


# ---- 4. extraction ------------------------------------------------------------------------------------------------------------------------------------------

class Mesh(SimpleNamespace):
    """vertices (V, 3) float32 in the grid frame, faces (T, 3) int32, intensity (V) float32 or None, origin (3,) float64: the world point of a
    vertex is ``origin + vertex`` in float64 (``world()``)."""

    def world(self):
        return np.asarray(self.origin, np.float64)[None] + self.vertices.detach().cpu().numpy().astype(np.float64)


def _min_weight(min_weight):
    mw = int(min_weight)
    if mw < 1:
        raise MeshError(f"extract: min_weight {mw} (at least 1: weight 0 is unobserved)")
    return mw


_TABLE = None


def _table():
    global _TABLE
    if _TABLE is None:
        _TABLE = table_arrays()
    return _TABLE


def _cells_and_edges(grid, mw):
    """(ts (X, Y, Z) float32, neg, act (X-1, Y-1, Z-1) bool, v, ax): the active cells and the emitted edges ascending by (v, axis)."""
    X, Y, Z = grid.dims
    ts = grid.tsdf.detach().cpu().numpy().reshape(X, Y, Z)
    obs = grid.weight.detach().cpu().numpy().reshape(X, Y, Z) >= mw
    neg = ts < 0
    act = np.ones((max(X - 1, 0), max(Y - 1, 0), max(Z - 1, 0)), bool)
    for n in range(8):
        a, b, c = n & 1, n >> 1 & 1, n >> 2 & 1
        act &= obs[a:X - 1 + a, b:Y - 1 + b, c:Z - 1 + c]
    A = np.zeros((X + 1, Y + 1, Z + 1), bool)
    A[1:X, 1:Y, 1:Z] = act                                                     # A[i + 1, j + 1, k + 1] = act[i, j, k]
    emit = np.zeros((X, Y, Z, 3), bool)
    crossed = (obs[:-1] & obs[1:] & (neg[:-1] != neg[1:]))
    emit[:-1, :, :, 0] = crossed & (A[1:X, 1:, 1:] | A[1:X, :-1, 1:] | A[1:X, 1:, :-1] | A[1:X, :-1, :-1])
    crossed = (obs[:, :-1] & obs[:, 1:] & (neg[:, :-1] != neg[:, 1:]))
    emit[:, :-1, :, 1] = crossed & (A[1:, 1:Y, 1:] | A[:-1, 1:Y, 1:] | A[1:, 1:Y, :-1] | A[:-1, 1:Y, :-1])
    crossed = (obs[:, :, :-1] & obs[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:]))
    emit[:, :, :-1, 2] = crossed & (A[1:, 1:, 1:Z] | A[:-1, 1:, 1:Z] | A[1:, :-1, 1:Z] | A[:-1, :-1, 1:Z])
    v, ax = np.nonzero(emit.reshape(-1, 3))                                    # ascending by (v, axis)
    return ts, neg, act, v, ax


def emitted_edges(grid, min_weight=1):
    """(v, axis) int64 arrays of the emitted edges in vertex order: vertex m lies on the edge from voxel v[m] to v[m] + e_axis[m]."""
    _, _, _, v, ax = _cells_and_edges(grid, _min_weight(min_weight))
    return v, ax


def _vertex_t(da, db):
    """t = d_a / (d_a - d_b) in float64 (mh_t)."""
    return da / (da - db)


@torch.no_grad()
def extract_reference(grid, min_weight=1, table=None):
    """The numpy twin of ``extract`` (see the module text) on a grid of any device; CPU tensors out.  ``table``: another triangle table (as
    ``mc_table()`` returns it), for the tests' negative controls."""
    mw = _min_weight(min_weight)
    ntri, tri = _table() if table is None else table_arrays(table)
    X, Y, Z = grid.dims
    N = X * Y * Z
    ts, neg, act, v, ax = _cells_and_edges(grid, mw)
    V = v.size
    vid = np.full((N, 3), -1, np.int64)
    vid[v, ax] = np.arange(V)
    stride = np.array([Y * Z, Z, 1], np.int64)
    u = v + stride[ax]
    t = _vertex_t(ts.reshape(-1)[v].astype(np.float64), ts.reshape(-1)[u].astype(np.float64))
    idx = np.stack(np.unravel_index(v, (X, Y, Z)), 1)
    cen = [centres(grid.voxel, n + 1) for n in (X, Y, Z)]
    verts = np.empty((V, 3), np.float32)
    for q in range(3):
        ca = cen[q][idx[:, q]].astype(np.float64)
        cb = cen[q][idx[:, q] + (ax == q)].astype(np.float64)
        verts[:, q] = (ca + t * (cb - ca)).astype(np.float32)
    vint = None
    if grid.intensity is not None:
        it = grid.intensity.detach().cpu().numpy().reshape(-1)
        ia, ib = it[v].astype(np.float64), it[u].astype(np.float64)
        vint = torch.from_numpy((ia + t * (ib - ia)).astype(np.float32))
    ci, cj, ck = np.nonzero(act)
    cell = (ci * Y + cj) * Z + ck                                              # ascending: nonzero walks C order
    cfg = np.zeros(cell.size, np.int64)
    for n in range(8):
        cfg |= neg[ci + (n & 1), cj + (n >> 1 & 1), ck + (n >> 2 & 1)].astype(np.int64) << n
    nt = ntri[cfg]
    rep = np.repeat(np.arange(cell.size), nt)
    m = np.arange(rep.size) - np.repeat(np.cumsum(nt) - nt, nt)
    e = tri[cfg[rep], m]                                                       # (T, 3) edge numbers
    cn = EDGE_CORNER[e]
    corner_voxel = cell[rep][:, None] + (cn & 1) * stride[0] + (cn >> 1 & 1) * stride[1] + (cn >> 2 & 1) * stride[2]
    faces = vid[corner_voxel, e >> 2]
    if faces.size and faces.min() < 0:
        raise MeshError("extract_reference: a triangle on an edge that is not emitted (the table uses an edge that is not crossed)")
    return Mesh(vertices=torch.from_numpy(verts), faces=torch.from_numpy(faces.astype(np.int32).reshape(-1, 3)), intensity=vint,
                origin=np.asarray(grid.origin, np.float64).copy())


def work_bytes(dims) -> int:
    X, Y, Z = (int(x) for x in dims)
    n = int(load().lrt_mesh_work_bytes(X, Y, Z))
    if n < 0:
        raise MeshError(f"extract: a grid of {X} x {Y} x {Z} voxels")
    return n


@torch.no_grad()
def extract(grid, min_weight=1, workspace=None):
    """The mesh of a grid (see the module text).  On a HIP device: count and scan, one host read of the totals (V, T), then vertices and faces --
    at most four launches.  A CPU grid goes to ``extract_reference``."""
    mw = _min_weight(min_weight)
    if grid.device.type != "cuda":
        if workspace is not None:
            raise MeshError("extract: a workspace with a grid on the CPU")
        return extract_reference(grid, mw)
    lib = load()
    dev = grid.device
    X, Y, Z = grid.dims
    for name in ("tsdf", "weight") + (("intensity",) if grid.intensity is not None else ()):
        if not getattr(grid, name).is_contiguous():
            raise MeshError(f"extract: the grid's {name} must be contiguous")
    nbytes = work_bytes(grid.dims)
    if workspace is not None:
        if not (torch.is_tensor(workspace) and workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == dev
                and workspace.numel() >= nbytes and workspace.data_ptr() % 256 == 0):
            raise MeshError(f"extract: the workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}, 256-byte aligned")
        ws = workspace
    else:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.lrt_mesh_count(dev.index, X, Y, Z, grid.tsdf.data_ptr(), grid.weight.data_ptr(), mw, ws.data_ptr(), ws.numel(), totals.data_ptr(),
                                _stream(dev))
    if rc != 0:
        raise MeshError(f"lrt_mesh_count failed ({rc}): {lib.lrt_mesh_last_error().decode()}")
    V, T = (int(x) for x in totals.cpu().tolist())                            # the one host read
    if V > MAX_OUTPUT or T > MAX_OUTPUT:
        raise MeshError(f"extract: {V} vertices and {T} faces (a vertex id and a face row are int32: at most {MAX_OUTPUT} each)")
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((T, 3), dtype=torch.int32, device=dev)
    vint = None if grid.intensity is None else torch.empty((V,), dtype=torch.float32, device=dev)
    if V or T:
        with torch.cuda.device(dev):
            rc = lib.lrt_mesh_write(dev.index, X, Y, Z, grid.voxel, grid.tsdf.data_ptr(), None if vint is None else grid.intensity.data_ptr(),
                                    ws.data_ptr(), ws.numel(), V, T, verts.data_ptr() if V else None, None if vint is None or not V else vint.data_ptr(),
                                    faces.data_ptr() if T else None, _stream(dev))
        if rc != 0:
            raise MeshError(f"lrt_mesh_write failed ({rc}): {lib.lrt_mesh_last_error().decode()}")
    return Mesh(vertices=verts, faces=faces, intensity=vint, origin=np.asarray(grid.origin, np.float64).copy())


# ---- 5. PLY -------------------------------------------------------------------------------------------------------------------------------------------------

_PLY_VERTEX = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("intensity", "<f4")])
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path, mesh):
    """Binary little-endian PLY: world ``x y z`` as doubles (``origin + vertex`` in float64), ``intensity`` float (0 without one), faces as
    ``list uchar int``."""
    pts = mesh.world()
    V = pts.shape[0]
    faces = mesh.faces.detach().cpu().numpy().astype(np.int32).reshape(-1, 3)
    vert = np.zeros(V, _PLY_VERTEX)
    vert["x"], vert["y"], vert["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if mesh.intensity is not None:
        vert["intensity"] = mesh.intensity.detach().cpu().numpy()
    face = np.zeros(faces.shape[0], _PLY_FACE)
    face["n"], face["v"] = 3, faces
    head = ("ply\nformat binary_little_endian 1.0\ncomment lidar_rt_amd.mesh\n"
            f"element vertex {V}\nproperty double x\nproperty double y\nproperty double z\nproperty float intensity\n"
            f"element face {faces.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(vert.tobytes())
        f.write(face.tobytes())


def read_ply(path):
    """The PLY that ``write_ply`` writes: namespace(points (V, 3) float64 world, intensity (V) float32, faces (T, 3) int32)."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise MeshError(f"{path}: not a PLY file")
    lines = [ln.split() for ln in raw[:end].decode("ascii").splitlines()]
    if ["format", "binary_little_endian", "1.0"] not in lines:
        raise MeshError(f"{path}: only binary little-endian PLY is read")
    counts, props, elem = {}, {}, None
    for ln in lines:
        if ln and ln[0] == "element":
            elem = ln[1]
            counts[elem], props[elem] = int(ln[2]), []
        elif ln and ln[0] == "property":
            props[elem].append(tuple(ln[1:]))
    if props.get("vertex") != [("double", "x"), ("double", "y"), ("double", "z"), ("float", "intensity")] or \
            props.get("face") != [("list", "uchar", "int", "vertex_indices")]:
        raise MeshError(f"{path}: not the layout of write_ply")
    body = raw[end + len(b"end_header\n"):]
    V, T = counts["vertex"], counts["face"]
    vert = np.frombuffer(body, _PLY_VERTEX, V)
    face = np.frombuffer(body, _PLY_FACE, T, offset=V * _PLY_VERTEX.itemsize)
    if T and not np.all(face["n"] == 3):
        raise MeshError(f"{path}: a face that is not a triangle")
    return SimpleNamespace(points=np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float64), intensity=vert["intensity"].astype(np.float32),
                           faces=face["v"].astype(np.int32).reshape(-1, 3))


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------------------------------

def _quat_rotation(q):
    w, x, y, z = (float(a) for a in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def load_frames(root, which="train", static_only=False, sweep="off", sweep_ref=0.5, sweep_direction="cw"):
    """The frames of a sequence directory for fusion: (meta, [dict(id, depth, intensity, mask, sensor2world float64, world points, valid,
    excluded)], inclination).  ``static_only``: the valid pixels whose return lies inside a tracking box present in that frame are excluded
    (``scene_init.assign_to_boxes``'s rule).  ``sweep="stored"``: every frame also carries its ``twist`` (6,) and ``tau`` (W,) float64 from its
    file, as ``sequence.load_sequence(sweep="stored")`` reads them (a frame without a twist is refused with its file's name; one without column
    times takes ``sweep.column_times(W, sweep_ref, sweep_direction)``), and its world points are ``sweep_fuse.sweep_points``'s."""
    from . import scene_init
    from . import sweep as sweep_mod
    if sweep not in ("off", "stored"):
        raise MeshError(f"load_frames: sweep {sweep!r} ('off' or 'stored')")
    with open(os.path.join(root, "meta.json")) as f:
        meta = json.load(f)
    test = [int(t) for t in meta.get("test_frames", [])]
    every = [int(t) for t in meta["frames"]]
    ids = {"all": every, "test": [i for i in every if i in set(test)], "train": [i for i in every if i not in set(test)] or every}[which]
    if not ids:
        raise MeshError(f"{root}: no {which} frames")
    s2e = meta.get("sensor2ego")
    s2e = None if s2e is None else np.asarray(s2e, np.float64)
    boxes = None
    if static_only and os.path.exists(os.path.join(root, "boxes.npz")):
        boxes = dict(np.load(os.path.join(root, "boxes.npz")))
    out, inc0, dirs = [], None, None
    for fid in ids:
        z = np.load(os.path.join(root, "frames", f"{fid:06d}.npz"))
        inc = z["inclination"].astype(np.float64).reshape(-1)
        if inc0 is None:
            inc0 = inc
            d = sweep_mod.sweep_rays(torch.eye(4, dtype=torch.float32)[:3].contiguous(), None, int(meta["height"]), int(meta["width"]),
                                 inc.tolist() if inc.size > 2 else (float(inc[0]), float(inc[1])), meta["data_type"],
                                 None if s2e is None else torch.as_tensor(s2e, dtype=torch.float32))[1]
            dirs = d.numpy().astype(np.float64)
        elif not np.array_equal(inc, inc0):
            raise MeshError(f"{root}: frame {fid} has another inclination than frame {ids[0]}; one call fuses frames of one projection rule")
        depth = z["depth"].astype(np.float32)
        mask = z["mask"].astype(bool)
        S = z["sensor2world"].astype(np.float64).reshape(4, 4)
        valid = mask & (depth > 0)
        motion = {}
        if sweep == "stored":
            from . import sweep_fuse
            path = os.path.join(root, "frames", f"{fid:06d}.npz")
            if "twist" not in z.files:
                raise MeshError(f"{path}: no stored twist (--sweep stored needs one per frame)")
            try:
                tau = z["tau"].astype(np.float64).reshape(-1) if "tau" in z.files else sweep_mod.column_times(int(meta["width"]), sweep_ref, sweep_direction).numpy()
            except sweep_mod.SweepError as e:
                raise MeshError(str(e)) from None
            motion = dict(twist=z["twist"].astype(np.float64).reshape(6), tau=tau)
            world = sweep_fuse.sweep_points(depth, S, motion["twist"], inc, meta["data_type"], s2e, tau=tau)
        else:
            world = (dirs * depth[..., None].astype(np.float64)) @ S[:3, :3].T + S[:3, 3]
        excluded = np.zeros_like(valid)
        if boxes is not None and fid in [int(x) for x in boxes["frames"]]:
            k = [int(x) for x in boxes["frames"]].index(fid)
            A = boxes["translation"].shape[0]
            poses = np.concatenate([boxes["translation"][:, k], boxes["quaternion"][:, k]], 1).astype(np.float32)
            label = scene_init.assign_to_boxes_reference(torch.from_numpy(world.astype(np.float32)), torch.zeros(world.shape, dtype=torch.float32),
                                                         torch.from_numpy(valid), torch.from_numpy(poses), torch.from_numpy(boxes["size"].astype(np.float32)),
                                                         torch.from_numpy(boxes["valid"][:, k].reshape(A)))[0].numpy()
            excluded = valid & (label > 0)
        out.append(dict(id=fid, depth=depth, intensity=z["intensity"].astype(np.float32), mask=valid & ~excluded, sensor2world=S, world=world,
                        valid=int(valid.sum()), excluded=int(excluded.sum()), **motion))
    return meta, out, inc0


def fuse_frames(grid, frames, inc, meta, batch, max_depth, sweep="off"):
    """Fuse the frames ``load_frames`` returned into ``grid``, ``batch`` frames per call.  ``sweep="stored"``: through ``sweep_fuse.integrate_sweep``
    with the frames' twists; a call takes frames of one ``tau``, so a batch ends where the column times change.  Returns None, or with the CPU twin
    of the sweep fusion dict(unseen, fused) summed over the calls."""
    dev = grid.device
    s2e = meta.get("sensor2ego")
    s2e = None if s2e is None else np.asarray(s2e, np.float64)
    incl = inc if inc.size > 2 else (float(inc[0]), float(inc[1]))
    counts = None
    b = 0
    while b < len(frames):
        e = min(b + batch, len(frames))
        if sweep == "stored":
            e = next((k for k in range(b + 1, e) if not np.array_equal(frames[k]["tau"], frames[b]["tau"])), e)
        chunk = frames[b:e]
        st = lambda k, dt: torch.from_numpy(np.stack([f[k] for f in chunk]).astype(dt)).to(dev)
        args = (grid, st("depth", np.float32), st("mask", np.bool_), np.stack([f["sensor2world"] for f in chunk]), incl)
        if sweep == "stored":
            from . import sweep_fuse
            r = sweep_fuse.integrate_sweep(*args, np.stack([f["twist"] for f in chunk]), meta["data_type"], s2e, st("intensity", np.float32), 0.0,
                                           max_depth, tau=chunk[0]["tau"])
            if r is not None:
                counts = counts or {"unseen": 0, "fused": 0}
                counts["unseen"] += r.unseen
                counts["fused"] += r.fused
        else:
            integrate(*args, meta["data_type"], s2e, st("intensity", np.float32), 0.0, max_depth)
        b = e
    return counts


def grid_bounds(frames, voxel, trunc, bounds=None):
    """(origin (3,) float64, dims): ``bounds`` (x0 y0 z0 x1 y1 z1), or the used returns' world extent padded by ``trunc`` and snapped to the voxel."""
    if bounds is not None:
        lo, hi = np.asarray(bounds[:3], np.float64), np.asarray(bounds[3:], np.float64)
        if not np.all(hi > lo):
            raise MeshError(f"--bounds {list(bounds)}: every upper bound must exceed its lower bound")
        origin = lo
    else:
        pts = [f["world"][f["mask"]] for f in frames]
        pts = np.concatenate(pts) if pts else np.zeros((0, 3))
        if not len(pts):
            raise MeshError("no valid return in the frames: give --bounds")
        lo, hi = pts.min(0) - trunc, pts.max(0) + trunc
        origin = np.floor(lo / voxel) * voxel
    dims = tuple(max(1, int(math.ceil((h - o) / voxel))) for o, h in zip(origin, hi))
    return origin, dims


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m lidar_rt_amd.mesh", description=(
        "Fuse a sequence's range images into a TSDF grid (projective: every voxel into every image) and extract its surface by marching cubes. "
        "Frames are fused with one pose per frame (--sweep off), or under the sweep model with each frame's stored twist (--sweep stored), which "
        "compensates the rolling-shutter shear of a moving sensor (train --sweep)."))
    ap.add_argument("--data", required=True, help="a sequence directory (lidar_rt_amd.sequence)")
    ap.add_argument("--out", default="mesh.ply", help="the PLY to write; mesh.json goes next to it")
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--trunc", type=float, default=None, help="metres (default: 3 voxels)")
    ap.add_argument("--min-weight", type=int, default=1)
    ap.add_argument("--max-depth", type=float, default=80.0)
    ap.add_argument("--frames", choices=("train", "test", "all"), default="train")
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--max-voxels", type=int, default=DEFAULT_MAX_VOXELS, help="a larger grid is refused, never coarsened")
    ap.add_argument("--batch", type=int, default=16, help="frames per integrate call")
    ap.add_argument("--static-only", action="store_true", help="drop the returns inside a tracking box present in their frame")
    ap.add_argument("--device", default="cuda", help="cuda (the library) or cpu (the numpy twins)")
    ap.add_argument("--sweep", choices=("off", "stored"), default="off", help="stored: fuse under the sweep model with each frame's stored twist (sweep_fuse.integrate_sweep)")
    ap.add_argument("--sweep-ref", type=float, default=0.5, help="--sweep: the part of the sweep at which a frame's pose holds, for frames that store no column times")
    ap.add_argument("--sweep-direction", choices=("cw", "ccw"), default="cw", help="--sweep: cw = time rises with the column index, for frames that store no column times")
    a = ap.parse_args(argv)
    t0 = time.perf_counter()
    voxel = float(a.voxel)
    trunc = 3.0 * voxel if a.trunc is None else float(a.trunc)
    if a.batch < 1:
        raise SystemExit("--batch must be at least 1")
    try:
        meta, frames, inc = load_frames(a.data, a.frames, a.static_only, a.sweep, a.sweep_ref, a.sweep_direction)
    except MeshError as e:
        if a.sweep == "off":
            raise
        raise SystemExit(str(e)) from None
    origin, dims = grid_bounds(frames, voxel, trunc, a.bounds)
    n = math.prod(dims)
    if n > a.max_voxels:
        raise SystemExit(f"the grid needs {dims[0]} x {dims[1]} x {dims[2]} = {n} voxels at --voxel {voxel}, more than --max-voxels {a.max_voxels}: "
                         "raise --max-voxels, give --bounds or a coarser --voxel")
    dev = torch.device(a.device)
    grid = TsdfGrid(origin, voxel, dims, trunc, dev, intensity=True)
    counts = fuse_frames(grid, frames, inc, meta, a.batch, a.max_depth, a.sweep)
    mesh = extract(grid, a.min_weight)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write_ply(a.out, mesh)
    report = {"args": vars(a), "grid": {"origin": origin.tolist(), "voxel": voxel, "dims": list(dims), "trunc": trunc},
              "frames": [f["id"] for f in frames], "pixels": {str(f["id"]): {"valid": f["valid"], "excluded": f["excluded"]} for f in frames},
              "totals": {"vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0]), "observed_voxels": int((grid.weight > 0).sum()),
                         "voxels": n, "seconds": round(time.perf_counter() - t0, 3)}}
    report["sweep"] = {"mode": a.sweep, **(counts or {})}
    with open(os.path.join(os.path.dirname(os.path.abspath(a.out)), "mesh.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report["totals"]))
    return report


if __name__ == "__main__":
    main(sys.argv[1:])
