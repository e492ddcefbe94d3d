"""Build the native pieces in-tree:

* ``csrc/liblrt_hip.so``  -- HIP kernels + C ABI (hipcc --offload-arch=gfx950).  No torch dependency; loadable through ctypes
  (``lidar_rt_amd._capi``).
* ``csrc/liblrt_hip_legacy.so`` -- the same sources with ``-DLRT_LEGACY``: the CROSS-CHECK library of the tests (env ``LRT_HIP_LIB``),
  which also carries the retired kernel generations (bwd_mode 1 / 2, colours inside the trace kernel, the level-by-level tree build) as
  independent implementations.  Nothing in the product loads it.
* ``diff_lidar_tracer/_C_ext.*.so`` -- the PyTorch-ROCm C++ extension (pybind11, ``csrc/lrt_torch_ext.cpp``): the reference's
  ``_C`` module surface with at::Tensor arguments on top of the C ABI.  Host code only; it links liblrt_hip.so.

* ``csrc/liblrt_loss.so`` -- the fused range-image training loss (``csrc/lrt_loss.hip``, C ABI ``include/lrt_loss.h``): a second product
  library with its own source list, content hash and stamp, so that the tracer library's ``source_hash()`` (which keys committed profiles)
  does not move with it.  Loaded by ``lidar_rt_amd.losses``.

* ``csrc/liblrt_gridcd.so`` -- the Chamfer term on the range-image grid (``csrc/lrt_gridcd.hip``, C ABI ``include/lrt_gridcd.h``): a third product
  library on the loss library's pattern (own source list, content hash and stamp).  Loaded by ``lidar_rt_amd.grid_chamfer``.

* ``csrc/liblrt_init.so`` -- the scene initialisation from range images (``csrc/lrt_init.hip``, C ABI ``include/lrt_init.h``): a fourth product
  library on the same pattern.  Loaded by ``lidar_rt_amd.scene_init``.

* ``csrc/liblrt_metrics.so`` -- the fused evaluation metrics (``csrc/lrt_metrics.hip``, C ABI ``include/lrt_metrics.h``): a fifth product
  library on the same pattern.  Loaded by ``lidar_rt_amd.metrics``.

* ``csrc/liblrt_adam.so`` -- the fused Adam step over an asset's parameter groups (``csrc/lrt_adam.hip``, C ABI ``include/lrt_adam.h``): a sixth product
  library on the same pattern.  Loaded by ``lidar_rt_amd.optim``.

* ``csrc/liblrt_densify.so`` -- the fused densify-and-prune of an asset (``csrc/lrt_densify.hip``, C ABI ``include/lrt_densify.h``): a seventh product
  library on the same pattern.  Loaded by ``lidar_rt_amd.densify``.

* ``csrc/liblrt_project.so`` -- the range-image projection of point clouds (``csrc/lrt_project.hip``, C ABI ``include/lrt_project.h``): an eighth product
  library on the same pattern.  Loaded by ``lidar_rt_amd.range_image``.

* ``csrc/liblrt_sweep.so`` -- the sweep rays of a moving sensor and their pose and twist gradients (``csrc/lrt_sweep.hip``, C ABI ``include/lrt_sweep.h``):
  a ninth product library on the same pattern.  Loaded by ``lidar_rt_amd.sweep``.

* ``csrc/liblrt_refine.so`` -- the inference of the ray-drop refinement network (``csrc/lrt_refine.hip``, C ABI ``include/lrt_refine.h``): a tenth
  product library on the same pattern.  Loaded by ``lidar_rt_amd.raydrop_refine``.

* ``csrc/liblrt_sweepproj.so`` -- the range-image projection under the sweep model (``csrc/lrt_sweepproj.hip``, C ABI ``include/lrt_sweepproj.h``): an
  eleventh product library on the same pattern.  Loaded by ``lidar_rt_amd.sweep_project``.

* ``csrc/liblrt_unproject.so`` -- the point clouds of range images (``csrc/lrt_unproject.hip``, C ABI ``include/lrt_unproject.h``): a twelfth product
  library on the same pattern.  Loaded by ``lidar_rt_amd.unproject``.

* ``csrc/liblrt_actorsweep.so`` -- actors that move within a sweep (``csrc/lrt_actorsweep.hip``, C ABI ``include/lrt_actorsweep.h``): a thirteenth
  product library on the same pattern.  Loaded by ``lidar_rt_amd.actor_sweep``.

* ``csrc/liblrt_beams.so`` -- the beam rays: the sweep rays with per-beam elevation and azimuth offsets, and their pose, twist and table gradients
  (``csrc/lrt_beams.hip``, C ABI ``include/lrt_beams.h``): a fourteenth product library on the same pattern.  Loaded by ``lidar_rt_amd.beams``.

* ``csrc/liblrt_reg.so`` -- the scan registration: projective point-to-plane ICP between two range images (``csrc/lrt_reg.hip``, C ABI
  ``include/lrt_reg.h``): a fifteenth product library on the same pattern.  Loaded by ``lidar_rt_amd.registration``.

* ``csrc/liblrt_segment.so`` -- the range-image segmentation: ground, connected segments, free-space evidence, segment tables and track
  bounds (``csrc/lrt_segment.hip``, C ABI ``include/lrt_segment.h``): a sixteenth product library on the same pattern.  Loaded by
  ``lidar_rt_amd.segmentation``.

* ``csrc/liblrt_place.so`` -- the place matcher: one ring-by-sector descriptor per scan and every scan against every earlier scan at every yaw
  (``csrc/lrt_place.hip``, C ABI ``include/lrt_place.h``): a seventeenth product library on the same pattern.  Loaded by ``lidar_rt_amd.place``.

* ``csrc/liblrt_mesh.so`` -- surface meshes from range images: projective TSDF fusion and marching cubes (``csrc/lrt_mesh.hip``, C ABI
  ``include/lrt_mesh.h``): an eighteenth product library on the same pattern.  Loaded by ``lidar_rt_amd.mesh``.

* ``csrc/liblrt_raycast.so`` -- range images of a fused TSDF grid: one marching ray per lane (``csrc/lrt_raycast.hip``, C ABI
  ``include/lrt_raycast.h``): a nineteenth product library on the same pattern.  Loaded by ``lidar_rt_amd.raycast``.

* ``csrc/liblrt_sweepfuse.so`` -- TSDF fusion of range images of a moving sensor: every voxel centre under the sweep model (``csrc/lrt_sweepfuse.hip``,
  C ABI ``include/lrt_sweepfuse.h``): a twentieth product library on the same pattern.  Loaded by ``lidar_rt_amd.sweep_fuse``.

* ``csrc/liblrt_mapreg.so`` -- scan-to-map registration: range images aligned to the fused TSDF grid, one trilinear sample per pixel
  (``csrc/lrt_mapreg.hip``, C ABI ``include/lrt_mapreg.h``): a twenty-first product library on the same pattern.  Loaded by
  ``lidar_rt_amd.map_registration``.

``python -m lidar_rt_amd.build`` rebuilds what is stale (``--force``: everything).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, "liblrt_hip.so")
SOURCES = ["lrt_kernels.hip", "lrt_chamfer.hip", "lrt_preprocess.hip"]
HEADERS = ["lrt_math.h", "lrt_device_guard.h", "lrt_build.inc", "lrt_backward.inc", "lrt_trace_legacy.inc", "lrt_collect.inc", "lrt_collect4.inc", "lrt_radix.inc", "lrt_near.inc", "lrt_bucket.inc", os.path.join("..", "..", "include", "lrt.h"),
           os.path.join("..", "..", "include", "lrt_chamfer.h"), os.path.join("..", "..", "include", "lrt_knn.h"),
           os.path.join("..", "..", "include", "lrt_preprocess.h")]
ARCH = "gfx950"


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


# -fno-slp-vectorize (round 5): the SLP vectoriser turns the kernels' scalar float chains into v_pk_* pairs and pays for it in register moves
# and pressure -- k_bwd_reduce4 needs 94 VGPRs with it and 69 without (5 -> 7 workgroups per CU), k_fwd_colour 126 -> 110, the build's
# record kernels lose 4 us; k_fwd_cr4 (explicit two-wide types where they pay) is unchanged.  tools/ab_build.sh and tools/kres.sh use the same flags.
CODEGEN_FLAGS = ["-O3", "-munsafe-fp-atomics", "-fno-slp-vectorize"]
STAMP = os.path.join(CSRC, "liblrt_hip.srchash")       # the hash of the sources the in-tree library was compiled from (travels with it; git-ignored)
LIB_LEGACY = os.path.join(CSRC, "liblrt_hip_legacy.so")
STAMP_LEGACY = os.path.join(CSRC, "liblrt_hip_legacy.srchash")
# the loss library: same arch and code-generation flags, its own sources (lrt_device_guard.h is shared, read-only)
LOSS_LIB = os.path.join(CSRC, "liblrt_loss.so")
LOSS_STAMP = os.path.join(CSRC, "liblrt_loss.srchash")
LOSS_SOURCES = ["lrt_loss.hip"]
LOSS_HEADERS = ["lrt_loss_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_loss.h")]
# the grid Chamfer library: the same pattern once more
GRIDCD_LIB = os.path.join(CSRC, "liblrt_gridcd.so")
GRIDCD_STAMP = os.path.join(CSRC, "liblrt_gridcd.srchash")
GRIDCD_SOURCES = ["lrt_gridcd.hip"]
GRIDCD_HEADERS = ["lrt_gridcd_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_gridcd.h")]
# the scene-initialisation library: once more (it reads the grid Chamfer operator's arithmetic header; that one's hash does not read back)
INIT_LIB = os.path.join(CSRC, "liblrt_init.so")
INIT_STAMP = os.path.join(CSRC, "liblrt_init.srchash")
INIT_SOURCES = ["lrt_init.hip"]
INIT_HEADERS = ["lrt_init_math.h", "lrt_gridcd_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_init.h")]
# the evaluation-metrics library: once more
METRICS_LIB = os.path.join(CSRC, "liblrt_metrics.so")
METRICS_STAMP = os.path.join(CSRC, "liblrt_metrics.srchash")
METRICS_SOURCES = ["lrt_metrics.hip"]
METRICS_HEADERS = ["lrt_metrics_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_metrics.h")]
# the optimizer library: once more
ADAM_LIB = os.path.join(CSRC, "liblrt_adam.so")
ADAM_STAMP = os.path.join(CSRC, "liblrt_adam.srchash")
ADAM_SOURCES = ["lrt_adam.hip"]
ADAM_HEADERS = ["lrt_adam_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_adam.h")]
# the densification library: once more
DENSIFY_LIB = os.path.join(CSRC, "liblrt_densify.so")
DENSIFY_STAMP = os.path.join(CSRC, "liblrt_densify.srchash")
DENSIFY_SOURCES = ["lrt_densify.hip"]
DENSIFY_HEADERS = ["lrt_densify_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_densify.h")]
# the projection library: once more
PROJECT_LIB = os.path.join(CSRC, "liblrt_project.so")
PROJECT_STAMP = os.path.join(CSRC, "liblrt_project.srchash")
PROJECT_SOURCES = ["lrt_project.hip"]
PROJECT_HEADERS = ["lrt_project_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_project.h")]
# the sweep-ray library: once more
SWEEP_LIB = os.path.join(CSRC, "liblrt_sweep.so")
SWEEP_STAMP = os.path.join(CSRC, "liblrt_sweep.srchash")
SWEEP_SOURCES = ["lrt_sweep.hip"]
SWEEP_HEADERS = ["lrt_sweep_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_sweep.h")]
# the ray-drop refinement library: once more
REFINE_LIB = os.path.join(CSRC, "liblrt_refine.so")
REFINE_STAMP = os.path.join(CSRC, "liblrt_refine.srchash")
REFINE_SOURCES = ["lrt_refine.hip"]
REFINE_HEADERS = ["lrt_refine_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_refine.h")]

SWEEPPROJ_LIB = os.path.join(CSRC, "liblrt_sweepproj.so")
SWEEPPROJ_STAMP = os.path.join(CSRC, "liblrt_sweepproj.srchash")
SWEEPPROJ_SOURCES = ["lrt_sweepproj.hip"]
SWEEPPROJ_HEADERS = ["lrt_sweepproj_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_sweepproj.h")]
# the un-projection library: once more
UNPROJECT_LIB = os.path.join(CSRC, "liblrt_unproject.so")
UNPROJECT_STAMP = os.path.join(CSRC, "liblrt_unproject.srchash")
UNPROJECT_SOURCES = ["lrt_unproject.hip"]
UNPROJECT_HEADERS = ["lrt_unproject_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_unproject.h")]
# the actor-sweep library: once more (it reads the rule headers of the projection and the two sweep libraries; their hashes do not read back)
ACTORSWEEP_LIB = os.path.join(CSRC, "liblrt_actorsweep.so")
ACTORSWEEP_STAMP = os.path.join(CSRC, "liblrt_actorsweep.srchash")
ACTORSWEEP_SOURCES = ["lrt_actorsweep.hip"]
ACTORSWEEP_HEADERS = ["lrt_actorsweep_math.h", "lrt_sweepproj_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h",
                      os.path.join("..", "..", "include", "lrt_actorsweep.h")]
# the beam-ray library: once more (it reads the sweep rays' rule header and ABI constants; their hashes do not read back)
BEAMS_LIB = os.path.join(CSRC, "liblrt_beams.so")
BEAMS_STAMP = os.path.join(CSRC, "liblrt_beams.srchash")
BEAMS_SOURCES = ["lrt_beams.hip"]
BEAMS_HEADERS = ["lrt_beams_math.h", "lrt_sweep_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_beams.h"),
                 os.path.join("..", "..", "include", "lrt_sweep.h")]
# the registration library: once more (it reads the rule headers of the projection and the sweep rays; their hashes do not read back)
REG_LIB = os.path.join(CSRC, "liblrt_reg.so")
REG_STAMP = os.path.join(CSRC, "liblrt_reg.srchash")
REG_SOURCES = ["lrt_reg.hip"]
REG_HEADERS = ["lrt_reg_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_reg.h")]
# the segmentation library: once more (it reads the same two rule headers, as they are)
SEGMENT_LIB = os.path.join(CSRC, "liblrt_segment.so")
SEGMENT_STAMP = os.path.join(CSRC, "liblrt_segment.srchash")
SEGMENT_SOURCES = ["lrt_segment.hip"]
SEGMENT_HEADERS = ["lrt_segment_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_segment.h")]
# the place-matcher library: once more (its rule header reads no other)
PLACE_LIB = os.path.join(CSRC, "liblrt_place.so")
PLACE_STAMP = os.path.join(CSRC, "liblrt_place.srchash")
PLACE_SOURCES = ["lrt_place.hip"]
PLACE_HEADERS = ["lrt_place_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_place.h")]
# the mesh library: once more (it reads the projection's rule header, as it is, and its generated triangle table)
MESH_LIB = os.path.join(CSRC, "liblrt_mesh.so")
MESH_STAMP = os.path.join(CSRC, "liblrt_mesh.srchash")
MESH_SOURCES = ["lrt_mesh.hip"]
MESH_HEADERS = ["lrt_mesh_math.h", "lrt_mesh_tables.h", "lrt_project_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_mesh.h")]
# the ray-casting library: once more (its rule header reads no other)
RAYCAST_LIB = os.path.join(CSRC, "liblrt_raycast.so")
RAYCAST_STAMP = os.path.join(CSRC, "liblrt_raycast.srchash")
RAYCAST_SOURCES = ["lrt_raycast.hip"]
RAYCAST_HEADERS = ["lrt_raycast_math.h", "lrt_device_guard.h", os.path.join("..", "..", "include", "lrt_raycast.h")]
# the sweep-fusion library: once more (it reads the rule headers of the mesh, the projection and the two sweep libraries; their hashes do not read back)
SWEEPFUSE_LIB = os.path.join(CSRC, "liblrt_sweepfuse.so")
SWEEPFUSE_STAMP = os.path.join(CSRC, "liblrt_sweepfuse.srchash")
SWEEPFUSE_SOURCES = ["lrt_sweepfuse.hip"]
SWEEPFUSE_HEADERS = ["lrt_sweepfuse_math.h", "lrt_mesh_math.h", "lrt_sweepproj_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h",
                     os.path.join("..", "..", "include", "lrt_sweepfuse.h")]
MAPREG_LIB = os.path.join(CSRC, "liblrt_mapreg.so")
MAPREG_STAMP = os.path.join(CSRC, "liblrt_mapreg.srchash")
MAPREG_SOURCES = ["lrt_mapreg.hip"]
MAPREG_HEADERS = ["lrt_mapreg_math.h", "lrt_raycast_math.h", "lrt_project_math.h", "lrt_sweep_math.h", "lrt_device_guard.h",
                  os.path.join("..", "..", "include", "lrt_mapreg.h")]
MAPREG_BORROWED = ["lrt_reg_math.h"]     # the registration's rule header, included as it is: hashed here, listed with liblrt_reg.so's own files only


def is_stale(lib: str = LIB, stamp: str = STAMP) -> bool:
    """The library is rebuilt when it is missing or was compiled from OTHER sources: decided by the content hash written next to it,
    not by modification times (a checkout, a copy to the GPU box or a touched header change mtimes without changing a byte -- and the
    other way round).  A library without a stamp (built by hand) falls back to the mtime rule."""
    if not os.path.exists(lib):
        return True
    if os.path.exists(stamp):
        try:
            return open(stamp).read().strip() != source_hash()
        except OSError:
            return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def source_hash() -> str:
    """sha256 (first 16 hex digits) over the kernel sources and headers: stamps profiles that are only valid for this code."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SOURCES + HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())            # the same sources under other code-generation flags are another library
    return h.hexdigest()[:16]


def loss_source_hash() -> str:
    """source_hash() of the loss library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(LOSS_SOURCES + LOSS_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def loss_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(LOSS_LIB):
        return True
    try:
        return open(LOSS_STAMP).read().strip() != loss_source_hash()
    except OSError:
        return True


def build_loss(force: bool = False, verbose: bool = False) -> str:
    """liblrt_loss.so, compiled when stale; the resource gate runs on it on EVERY call, as on the tracer library."""
    if force or loss_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", LOSS_LIB] \
            + [os.path.join(CSRC, s) for s in LOSS_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(LOSS_STAMP, "w") as f:
            f.write(loss_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(LOSS_LIB)} is up to date (sources {loss_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(LOSS_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return LOSS_LIB


def gridcd_source_hash() -> str:
    """source_hash() of the grid Chamfer library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(GRIDCD_SOURCES + GRIDCD_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def gridcd_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(GRIDCD_LIB):
        return True
    try:
        return open(GRIDCD_STAMP).read().strip() != gridcd_source_hash()
    except OSError:
        return True


def build_gridcd(force: bool = False, verbose: bool = False) -> str:
    """liblrt_gridcd.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other two libraries."""
    if force or gridcd_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", GRIDCD_LIB] \
            + [os.path.join(CSRC, s) for s in GRIDCD_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(GRIDCD_STAMP, "w") as f:
            f.write(gridcd_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(GRIDCD_LIB)} is up to date (sources {gridcd_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(GRIDCD_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return GRIDCD_LIB


def init_source_hash() -> str:
    """source_hash() of the scene-initialisation library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(INIT_SOURCES + INIT_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def init_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(INIT_LIB):
        return True
    try:
        return open(INIT_STAMP).read().strip() != init_source_hash()
    except OSError:
        return True


def build_init(force: bool = False, verbose: bool = False) -> str:
    """liblrt_init.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other three libraries."""
    if force or init_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", INIT_LIB] \
            + [os.path.join(CSRC, s) for s in INIT_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(INIT_STAMP, "w") as f:
            f.write(init_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(INIT_LIB)} is up to date (sources {init_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(INIT_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return INIT_LIB


def metrics_source_hash() -> str:
    """source_hash() of the evaluation-metrics library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(METRICS_SOURCES + METRICS_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def metrics_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(METRICS_LIB):
        return True
    try:
        return open(METRICS_STAMP).read().strip() != metrics_source_hash()
    except OSError:
        return True


def build_metrics(force: bool = False, verbose: bool = False) -> str:
    """liblrt_metrics.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other four libraries."""
    if force or metrics_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", METRICS_LIB] \
            + [os.path.join(CSRC, s) for s in METRICS_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(METRICS_STAMP, "w") as f:
            f.write(metrics_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(METRICS_LIB)} is up to date (sources {metrics_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(METRICS_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return METRICS_LIB


def adam_source_hash() -> str:
    """source_hash() of the optimizer library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(ADAM_SOURCES + ADAM_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def adam_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(ADAM_LIB):
        return True
    try:
        return open(ADAM_STAMP).read().strip() != adam_source_hash()
    except OSError:
        return True


def build_adam(force: bool = False, verbose: bool = False) -> str:
    """liblrt_adam.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other five libraries."""
    if force or adam_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", ADAM_LIB] \
            + [os.path.join(CSRC, s) for s in ADAM_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(ADAM_STAMP, "w") as f:
            f.write(adam_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(ADAM_LIB)} is up to date (sources {adam_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(ADAM_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return ADAM_LIB


def densify_source_hash() -> str:
    """source_hash() of the densification library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(DENSIFY_SOURCES + DENSIFY_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def densify_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(DENSIFY_LIB):
        return True
    try:
        return open(DENSIFY_STAMP).read().strip() != densify_source_hash()
    except OSError:
        return True


def build_densify(force: bool = False, verbose: bool = False) -> str:
    """liblrt_densify.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other six libraries."""
    if force or densify_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", DENSIFY_LIB] \
            + [os.path.join(CSRC, s) for s in DENSIFY_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(DENSIFY_STAMP, "w") as f:
            f.write(densify_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(DENSIFY_LIB)} is up to date (sources {densify_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(DENSIFY_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return DENSIFY_LIB


def project_source_hash() -> str:
    """source_hash() of the projection library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(PROJECT_SOURCES + PROJECT_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def project_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(PROJECT_LIB):
        return True
    try:
        return open(PROJECT_STAMP).read().strip() != project_source_hash()
    except OSError:
        return True


def build_project(force: bool = False, verbose: bool = False) -> str:
    """liblrt_project.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other seven libraries."""
    if force or project_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", PROJECT_LIB] \
            + [os.path.join(CSRC, s) for s in PROJECT_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(PROJECT_STAMP, "w") as f:
            f.write(project_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(PROJECT_LIB)} is up to date (sources {project_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(PROJECT_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return PROJECT_LIB


def sweep_source_hash() -> str:
    """source_hash() of the sweep-ray library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SWEEP_SOURCES + SWEEP_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def sweep_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(SWEEP_LIB):
        return True
    try:
        return open(SWEEP_STAMP).read().strip() != sweep_source_hash()
    except OSError:
        return True


def build_sweep(force: bool = False, verbose: bool = False) -> str:
    """liblrt_sweep.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other eight libraries."""
    if force or sweep_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", SWEEP_LIB] \
            + [os.path.join(CSRC, s) for s in SWEEP_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(SWEEP_STAMP, "w") as f:
            f.write(sweep_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(SWEEP_LIB)} is up to date (sources {sweep_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(SWEEP_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return SWEEP_LIB


def refine_source_hash() -> str:
    """source_hash() of the ray-drop refinement library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(REFINE_SOURCES + REFINE_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def refine_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(REFINE_LIB):
        return True
    try:
        return open(REFINE_STAMP).read().strip() != refine_source_hash()
    except OSError:
        return True


def build_refine(force: bool = False, verbose: bool = False) -> str:
    """liblrt_refine.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other nine libraries."""
    if force or refine_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", REFINE_LIB] \
            + [os.path.join(CSRC, s) for s in REFINE_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(REFINE_STAMP, "w") as f:
            f.write(refine_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(REFINE_LIB)} is up to date (sources {refine_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(REFINE_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return REFINE_LIB


def sweepproj_source_hash() -> str:
    """source_hash() of the sweep-projection library: over ITS sources, headers (the two rule headers it reads included) and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SWEEPPROJ_SOURCES + SWEEPPROJ_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def sweepproj_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(SWEEPPROJ_LIB):
        return True
    try:
        return open(SWEEPPROJ_STAMP).read().strip() != sweepproj_source_hash()
    except OSError:
        return True


def build_sweepproj(force: bool = False, verbose: bool = False) -> str:
    """liblrt_sweepproj.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other ten libraries."""
    if force or sweepproj_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", SWEEPPROJ_LIB] \
            + [os.path.join(CSRC, s) for s in SWEEPPROJ_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(SWEEPPROJ_STAMP, "w") as f:
            f.write(sweepproj_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(SWEEPPROJ_LIB)} is up to date (sources {sweepproj_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(SWEEPPROJ_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return SWEEPPROJ_LIB


def unproject_source_hash() -> str:
    """source_hash() of the un-projection library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(UNPROJECT_SOURCES + UNPROJECT_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def unproject_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(UNPROJECT_LIB):
        return True
    try:
        return open(UNPROJECT_STAMP).read().strip() != unproject_source_hash()
    except OSError:
        return True


def build_unproject(force: bool = False, verbose: bool = False) -> str:
    """liblrt_unproject.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other eleven libraries."""
    if force or unproject_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", UNPROJECT_LIB] \
            + [os.path.join(CSRC, s) for s in UNPROJECT_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(UNPROJECT_STAMP, "w") as f:
            f.write(unproject_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(UNPROJECT_LIB)} is up to date (sources {unproject_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(UNPROJECT_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return UNPROJECT_LIB


def actorsweep_source_hash() -> str:
    """source_hash() of the actor-sweep library: over ITS sources, headers (the rule headers it reads included) and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(ACTORSWEEP_SOURCES + ACTORSWEEP_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def actorsweep_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(ACTORSWEEP_LIB):
        return True
    try:
        return open(ACTORSWEEP_STAMP).read().strip() != actorsweep_source_hash()
    except OSError:
        return True


def build_actorsweep(force: bool = False, verbose: bool = False) -> str:
    """liblrt_actorsweep.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other twelve libraries."""
    if force or actorsweep_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", ACTORSWEEP_LIB] \
            + [os.path.join(CSRC, s) for s in ACTORSWEEP_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(ACTORSWEEP_STAMP, "w") as f:
            f.write(actorsweep_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(ACTORSWEEP_LIB)} is up to date (sources {actorsweep_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(ACTORSWEEP_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return ACTORSWEEP_LIB


def beams_source_hash() -> str:
    """source_hash() of the beam-ray library: over ITS sources, headers (the sweep rays' rule header included) and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(BEAMS_SOURCES + BEAMS_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def beams_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(BEAMS_LIB):
        return True
    try:
        return open(BEAMS_STAMP).read().strip() != beams_source_hash()
    except OSError:
        return True


def build_beams(force: bool = False, verbose: bool = False) -> str:
    """liblrt_beams.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other thirteen libraries."""
    if force or beams_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", BEAMS_LIB] \
            + [os.path.join(CSRC, s) for s in BEAMS_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(BEAMS_STAMP, "w") as f:
            f.write(beams_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(BEAMS_LIB)} is up to date (sources {beams_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(BEAMS_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return BEAMS_LIB


def reg_source_hash() -> str:
    """source_hash() of the registration library: over ITS sources, headers (the two rule headers it reads included) and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(REG_SOURCES + REG_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def reg_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(REG_LIB):
        return True
    try:
        return open(REG_STAMP).read().strip() != reg_source_hash()
    except OSError:
        return True


def build_reg(force: bool = False, verbose: bool = False) -> str:
    """liblrt_reg.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other fourteen libraries."""
    if force or reg_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", REG_LIB] \
            + [os.path.join(CSRC, s) for s in REG_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(REG_STAMP, "w") as f:
            f.write(reg_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(REG_LIB)} is up to date (sources {reg_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(REG_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return REG_LIB


def segment_source_hash() -> str:
    """source_hash() of the segmentation library: over ITS sources, headers (the two rule headers it reads included) and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SEGMENT_SOURCES + SEGMENT_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def segment_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(SEGMENT_LIB):
        return True
    try:
        return open(SEGMENT_STAMP).read().strip() != segment_source_hash()
    except OSError:
        return True


def build_segment(force: bool = False, verbose: bool = False) -> str:
    """liblrt_segment.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other fifteen libraries."""
    if force or segment_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", SEGMENT_LIB] \
            + [os.path.join(CSRC, s) for s in SEGMENT_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(SEGMENT_STAMP, "w") as f:
            f.write(segment_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(SEGMENT_LIB)} is up to date (sources {segment_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(SEGMENT_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return SEGMENT_LIB


def place_source_hash() -> str:
    """source_hash() of the place-matcher library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(PLACE_SOURCES + PLACE_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def place_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(PLACE_LIB):
        return True
    try:
        return open(PLACE_STAMP).read().strip() != place_source_hash()
    except OSError:
        return True


def build_place(force: bool = False, verbose: bool = False) -> str:
    """liblrt_place.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other sixteen libraries."""
    if force or place_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", PLACE_LIB] \
            + [os.path.join(CSRC, s) for s in PLACE_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(PLACE_STAMP, "w") as f:
            f.write(place_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(PLACE_LIB)} is up to date (sources {place_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(PLACE_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return PLACE_LIB


def mesh_source_hash() -> str:
    """source_hash() of the mesh library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(MESH_SOURCES + MESH_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def mesh_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(MESH_LIB):
        return True
    try:
        return open(MESH_STAMP).read().strip() != mesh_source_hash()
    except OSError:
        return True


def build_mesh(force: bool = False, verbose: bool = False) -> str:
    """liblrt_mesh.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other seventeen libraries."""
    if force or mesh_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", MESH_LIB] \
            + [os.path.join(CSRC, s) for s in MESH_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(MESH_STAMP, "w") as f:
            f.write(mesh_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(MESH_LIB)} is up to date (sources {mesh_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(MESH_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return MESH_LIB


def raycast_source_hash() -> str:
    """source_hash() of the ray-casting library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(RAYCAST_SOURCES + RAYCAST_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def raycast_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(RAYCAST_LIB):
        return True
    try:
        return open(RAYCAST_STAMP).read().strip() != raycast_source_hash()
    except OSError:
        return True


def build_raycast(force: bool = False, verbose: bool = False) -> str:
    """liblrt_raycast.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other eighteen libraries."""
    if force or raycast_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", RAYCAST_LIB] \
            + [os.path.join(CSRC, s) for s in RAYCAST_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(RAYCAST_STAMP, "w") as f:
            f.write(raycast_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(RAYCAST_LIB)} is up to date (sources {raycast_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(RAYCAST_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return RAYCAST_LIB


def sweepfuse_source_hash() -> str:
    """source_hash() of the sweep-fusion library: over ITS sources, headers and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SWEEPFUSE_SOURCES + SWEEPFUSE_HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def sweepfuse_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(SWEEPFUSE_LIB):
        return True
    try:
        return open(SWEEPFUSE_STAMP).read().strip() != sweepfuse_source_hash()
    except OSError:
        return True


def build_sweepfuse(force: bool = False, verbose: bool = False) -> str:
    """liblrt_sweepfuse.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other nineteen libraries."""
    if force or sweepfuse_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", SWEEPFUSE_LIB] \
            + [os.path.join(CSRC, s) for s in SWEEPFUSE_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(SWEEPFUSE_STAMP, "w") as f:
            f.write(sweepfuse_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(SWEEPFUSE_LIB)} is up to date (sources {sweepfuse_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(SWEEPFUSE_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return SWEEPFUSE_LIB


def mapreg_source_hash() -> str:
    """source_hash() of the scan-to-map registration library: over ITS sources, headers, the borrowed rule header and the code-generation flags."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(MAPREG_SOURCES + MAPREG_HEADERS + MAPREG_BORROWED):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode()); h.update(fh.read())
    h.update(" ".join(CODEGEN_FLAGS).encode())
    return h.hexdigest()[:16]


def mapreg_is_stale() -> bool:
    """Missing, or compiled from other sources (the content hash stamped next to it; no stamp = rebuilt)."""
    if not os.path.exists(MAPREG_LIB):
        return True
    try:
        return open(MAPREG_STAMP).read().strip() != mapreg_source_hash()
    except OSError:
        return True


def build_mapreg(force: bool = False, verbose: bool = False) -> str:
    """liblrt_mapreg.so, compiled when stale; the resource gate runs on it on EVERY call, as on the other twenty libraries."""
    if force or mapreg_is_stale():
        cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + ["-std=c++17", "-fPIC", "-shared", "-o", MAPREG_LIB] \
            + [os.path.join(CSRC, s) for s in MAPREG_SOURCES]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)
        with open(MAPREG_STAMP, "w") as f:
            f.write(mapreg_source_hash() + "\n")
    elif verbose:
        print(f"{os.path.basename(MAPREG_LIB)} is up to date (sources {mapreg_source_hash()}): not recompiled (--force compiles anyway)", flush=True)
    from . import resources
    res = resources.check(MAPREG_LIB)
    if verbose:
        print(resources.table_md(res), flush=True)
    return MAPREG_LIB


EXT_SRC = os.path.join(CSRC, "lrt_torch_ext.cpp")
EXT_DIR = os.path.join(HERE, "diff_lidar_tracer")


def ext_path() -> str:
    import sysconfig
    return os.path.join(EXT_DIR, "_C_ext" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))


EXT_STAMP = os.path.join(EXT_DIR, "_C_ext.srchash")


def ext_hash() -> str:
    """Content hash of what the torch extension is compiled from (its source, the C ABI header) and against (the torch version)."""
    import hashlib
    h = hashlib.sha256()
    for f in (EXT_SRC, os.path.join(HERE, "..", "include", "lrt.h")):
        with open(f, "rb") as fh:
            h.update(fh.read())
    try:
        import torch
        h.update(torch.__version__.encode())
    except Exception:
        pass
    return h.hexdigest()[:16]


def ext_is_stale() -> bool:
    """Like the library: by the content hash stamped next to the extension, not by modification times (ADVICE r05 / VERDICT r05 weak 13)."""
    out = ext_path()
    if not os.path.exists(out):
        return True
    try:
        return open(EXT_STAMP).read().strip() != ext_hash()
    except OSError:
        return True


def build_ext(force: bool = False, verbose: bool = False) -> str:
    """The torch extension: one host-only C++ file against torch's headers (the include / library paths torch.utils.cpp_extension
    reports), linked with liblrt_hip.so through an $ORIGIN-relative rpath so that the in-tree pair travels together."""
    out = ext_path()
    if not force and not ext_is_stale():
        return out
    import sysconfig
    import torch
    from torch.utils import cpp_extension as ce
    rocm = os.environ.get("ROCM_HOME") or os.environ.get("ROCM_PATH") or "/opt/rocm"
    inc = [f"-I{p}" for p in ce.include_paths()] + [f"-I{rocm}/include", f"-I{sysconfig.get_paths()['include']}"]
    libdirs = ce.library_paths() + [f"{rocm}/lib"]
    cmd = (["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DTORCH_EXTENSION_NAME=_C_ext",
            "-DTORCH_API_INCLUDE_EXTENSION_H", f"-D_GLIBCXX_USE_CXX11_ABI={int(torch.compiled_with_cxx11_abi())}"] + inc + [EXT_SRC, "-o", out]
           + [f"-L{d}" for d in libdirs] + [f"-L{CSRC}", "-llrt_hip", "-lc10", "-lc10_hip", "-ltorch_cpu", "-ltorch_hip", "-ltorch", "-ltorch_python", "-lamdhip64",
              "-Wl,-rpath,$ORIGIN/../csrc"] + [f"-Wl,-rpath,{d}" for d in libdirs])
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=CSRC)
    with open(EXT_STAMP, "w") as f:
        f.write(ext_hash() + "\n")
    return out


def build(force: bool = False, verbose: bool = False, legacy: bool = True) -> str:
    """The product library, the resource gate on EVERY kernel it ships, the torch extension and (legacy=True) the cross-check library.
    The cross-check library's compile (3.3 min, the longer one) runs beside the product's (1.7 min) in a thread: a clean build takes the longer of the two."""
    legacy_job, legacy_err = None, []
    if legacy and (force or is_stale(LIB_LEGACY, STAMP_LEGACY)):
        import threading

        def _job():
            try:
                _build_lib(force, verbose, legacy=True)
            except BaseException as e:      # reported by the caller's thread below
                legacy_err.append(e)
        legacy_job = threading.Thread(target=_job, name="lrt-legacy-build"); legacy_job.start()
    try:
        lib = _build_product(force, verbose)
    finally:
        if legacy_job is not None:
            legacy_job.join()
    if legacy_err:
        raise legacy_err[0]
    return lib


def _build_product(force: bool, verbose: bool) -> str:
    lib = _build_lib(force, verbose)
    # the resource gate (lidar_rt_amd/resources.py): no shipped kernel may spill a vector register or use scratch.  Checked on every call,
    # also for a library that was not recompiled: the .so that ships is the one that must pass
    from . import resources
    res = resources.check(lib)
    if verbose:
        print(resources.table_md(res, r"^k_fwd_cr4<"), flush=True)
        print(f"{sum(1 for n in res if resources.is_own_kernel(n))} kernels of this project in {os.path.basename(lib)}, none spills", flush=True)
    build_ext(force, verbose)
    build_loss(force, verbose)
    build_gridcd(force, verbose)
    build_init(force, verbose)
    build_metrics(force, verbose)
    build_adam(force, verbose)
    build_densify(force, verbose)
    build_project(force, verbose)
    build_sweep(force, verbose)
    build_refine(force, verbose)
    build_sweepproj(force, verbose)
    build_unproject(force, verbose)
    build_actorsweep(force, verbose)
    build_beams(force, verbose)
    build_reg(force, verbose)
    build_segment(force, verbose)
    build_place(force, verbose)
    build_mesh(force, verbose)
    build_raycast(force, verbose)
    build_sweepfuse(force, verbose)
    build_mapreg(force, verbose)
    return lib


def _build_lib(force: bool = False, verbose: bool = False, legacy: bool = False) -> str:
    lib, stamp = (LIB_LEGACY, STAMP_LEGACY) if legacy else (LIB, STAMP)
    if not force and not is_stale(lib, stamp):
        if verbose:
            print(f"{os.path.basename(lib)} is up to date (sources {source_hash()}): not recompiled (--force compiles anyway)", flush=True)
        return lib
    cmd = [hipcc_path(), f"--offload-arch={ARCH}"] + CODEGEN_FLAGS + (["-DLRT_LEGACY"] if legacy else []) \
        + ["-std=c++17", "-fPIC", "-shared", "-Wno-unused-value", "-o", lib] + [os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=CSRC)
    with open(stamp, "w") as f:
        f.write(source_hash() + "\n")
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
