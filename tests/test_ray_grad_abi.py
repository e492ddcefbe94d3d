"""The ray-gradient entry point of the C ABI (lrt_backward_rays, ABI 5) and its two Python bindings, without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

from lidar_rt_amd import _capi
from lidar_rt_amd import build as lrt_build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(lrt_build.LIB):
        lrt_build.build()
    return C.CDLL(lrt_build.LIB)


def test_lrt_backward_rays_is_exported_and_declared(lib):
    assert hasattr(lib, "lrt_backward_rays")
    assert "lrt_backward_rays" in _capi.EXPORTS
    hdr = open(os.path.join(REPO, "include", "lrt.h")).read()
    decl = re.search(r"int lrt_backward_rays\(([^;]*)\);", hdr)
    assert decl and "float* d_ray_o" in decl.group(1) and "float* d_ray_d" in decl.group(1)


def test_abi_version_is_5_everywhere(lib):
    hdr = open(os.path.join(REPO, "include", "lrt.h")).read()
    want = int(re.search(r"#define\s+LRT_ABI_VERSION\s+(\d+)", hdr).group(1))
    assert want == 5 and _capi.ABI_VERSION == 5
    lib.lrt_abi_version.restype = C.c_int
    assert lib.lrt_abi_version() == 5


def test_lrt_backward_rays_refuses_a_null_state(lib):
    lib.lrt_backward_rays.restype = C.c_int
    rc = lib.lrt_backward_rays(*([None] + [0] * 2 + [None] * 2 + [0] * 3 + [None] * 17))
    assert rc == -1          # LRT_ERR_ARG


def test_both_bindings_take_ray_grads_out():
    from lidar_rt_amd.diff_lidar_tracer import _C
    assert "ray_grads_out" in inspect.signature(_C.trace_surfels_backward).parameters
    assert "ray_grads_out" in inspect.signature(_C._ct_trace_surfels_backward).parameters
    if getattr(_C, "_ext", None) is None:
        pytest.skip("the pybind11 extension is not built")
    assert "ray_grads_out" in _C._ext.trace_surfels_backward.__doc__
