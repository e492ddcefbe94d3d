"""Recipe that builds the reference's own Chamfer and simple-knn kernels for gfx950 (TEST INFRASTRUCTURE, not product code).

The two operators of the reference that need no OptiX (lib/utils/chamfer3D and submodules/simple-knn) are plain CUDA.  This recipe
copies their files out of a reference checkout into ``oracle/_ref/src/``, translates the copies with torch's hipify, and compiles
them into Python extension modules under ``oracle/_ref/``, so that ``tests/test_reference_pin_gpu.py`` can run the reference's
kernels against ``oracle/chamfer_oracle.c``.  Only this recipe is committed: ``oracle/_ref/`` is ignored by git, and no reference
text, translated text or object ever enters the repository.

Each module is built twice, from separate objects: ``<name>_nocontract`` with ``-ffp-contract=off`` (IEEE arithmetic as written,
unambiguous) and ``<name>`` with the compiler's own choice of contraction.  The two builds carry different module names because
pybind11 keeps one module object per name in a process.  ``oracle/_ref/manifest.json`` records the modules, the flags and the
sha256 of every reference file and every translated copy.

The reference tree is found through ``LRT_REFERENCE_DIR`` (default: the ``reference`` checkout beside this repository).  Without one
the recipe prints a line, writes no manifest and returns None; with one, a failing compile raises.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import subprocess
import sys
import sysconfig
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(_HERE, "_ref")
MANIFEST = os.path.join(REF_OUT, "manifest.json")
ARCH = "gfx950"

# module name -> (directory inside the reference tree, files copied, translation units compiled)
MODULES = {
    "ref_chamfer_3D": ("lib/utils/chamfer3D", ["chamfer3D.cu", "chamfer_cuda.cpp"], ["chamfer3D.cu", "chamfer_cuda.cpp"]),
    "ref_simple_knn": ("submodules/simple-knn", ["simple_knn.cu", "spatial.cu", "ext.cpp", "simple_knn.h", "spatial.h"],
                       ["simple_knn.cu", "spatial.cu", "ext.cpp"]),
}
VARIANTS = {"off": ["-ffp-contract=off"], "default": []}
SUFFIX = {"off": "_nocontract", "default": ""}             # appended to the module name (TORCH_EXTENSION_NAME)

# The only edits made to the copies before translation, each (file, old text, new text, reason).  All are outside kernel bodies.
EDITS = [
    ("simple_knn.cu", '#include "device_launch_parameters.h"\n', "",
     "a CUDA-toolkit header (editor hints for the launch variables) that ROCm does not ship"),
    ("simple_knn.cu", "#define __CUDACC__\n", "",
     "forces the CUDA compiler macro; its translation would redefine the macro the HIP compiler sets itself"),
    ("simple_knn.cu", "#include <cooperative_groups/reduce.h>\n", "",
     "unused by the file (no cg::reduce call), and ROCm has no header of that name"),
    ("simple_knn.cu", "<< <", "<<<", "the spaced launch bracket is not one token for the HIP compiler"),
    ("simple_knn.cu", ">> >", ">>>", "the spaced launch bracket is not one token for the HIP compiler"),
]


def reference_dir() -> str:
    return os.path.abspath(os.environ.get("LRT_REFERENCE_DIR") or os.path.join(_HERE, "..", "..", "reference"))


def _sha(path: str) -> str:
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def _common_flags():
    """Include / library paths and defines: the ones lidar_rt_amd.build.build_ext compiles the product's torch extension with."""
    import torch
    from torch.utils import cpp_extension as ce
    rocm = os.environ.get("ROCM_HOME") or os.environ.get("ROCM_PATH") or "/opt/rocm"
    inc = [f"-I{p}" for p in ce.include_paths()] + [f"-I{rocm}/include", f"-I{sysconfig.get_paths()['include']}"]
    libdirs = ce.library_paths() + [f"{rocm}/lib"]
    cflags = ["-O3", "-std=c++17", "-fPIC", "-w", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DTORCH_API_INCLUDE_EXTENSION_H",
              f"-D_GLIBCXX_USE_CXX11_ABI={int(torch.compiled_with_cxx11_abi())}"] + inc
    # -Bsymbolic: the two builds of a module define the same symbols; each must bind to its own kernels' host stubs
    ldflags = ["-shared", "-Wl,-Bsymbolic"] + [f"-L{d}" for d in libdirs] + ["-lc10", "-lc10_hip", "-ltorch_cpu", "-ltorch_hip", "-ltorch",
                                                                            "-ltorch_python", "-lamdhip64"] + [f"-Wl,-rpath,{d}" for d in libdirs]
    return cflags, ldflags, torch.__version__


def _stage_sources(ref: str):
    """Copy, edit and translate.  Returns {module: [translated unit paths]}, {reference file: sha256}, {translated copy: sha256}."""
    src_root = os.path.join(REF_OUT, "src")
    shutil.rmtree(src_root, ignore_errors=True)
    ref_sha = {}
    for name, (sub, files, _) in MODULES.items():
        os.makedirs(os.path.join(src_root, name))
        for f in files:
            p = os.path.join(ref, sub, f)
            if not os.path.exists(p):
                raise RuntimeError(f"reference tree {ref} lacks {sub}/{f}")
            ref_sha[f"{sub}/{f}"] = _sha(p)
            shutil.copyfile(p, os.path.join(src_root, name, f))
    for f, old, new, _ in EDITS:
        for name, (_, files, _) in MODULES.items():
            if f in files:
                p = os.path.join(src_root, name, f)
                text = open(p).read()
                if old not in text:
                    raise RuntimeError(f"{f}: expected text {old!r} not found; the reference changed, review the recipe's edits")
                open(p, "w").write(text.replace(old, new))
    from torch.utils.hipify import hipify_python
    res = hipify_python.hipify(project_directory=src_root, output_directory=src_root, includes=[os.path.join(src_root, "*")],
                               is_pytorch_extension=True, show_progress=False)
    units, out_sha = {}, {}
    for name, (_, files, tus) in MODULES.items():
        units[name] = []
        for f in files:
            src = os.path.join(src_root, name, f)
            r = res.get(src)
            out = r.hipified_path if r is not None and r.hipified_path else src
            out_sha[os.path.relpath(out, REF_OUT)] = _sha(out)
            if f in tus:
                units[name].append(out)
    return units, ref_sha, out_sha


def _recipe_key(ref_sha, cflags, ldflags, torch_version) -> str:
    h = hashlib.sha256()
    h.update(_sha(os.path.abspath(__file__)).encode())
    h.update(json.dumps([ref_sha, cflags, ldflags, torch_version, VARIANTS, ARCH], sort_keys=True).encode())
    return h.hexdigest()


def build(force: bool = False, verbose: bool = False):
    """Build the four modules and the manifest; returns the manifest's path, or None when there is no reference tree."""
    ref = reference_dir()
    if not os.path.isdir(ref):
        print(f"oracle/ref_build: no reference tree at {ref}; the reference binaries are not built (their tests will skip)", flush=True)
        return None
    cflags, ldflags, torch_version = _common_flags()
    ref_sha = {f"{sub}/{f}": _sha(os.path.join(ref, sub, f)) for sub, files, _ in MODULES.values() for f in files
               if os.path.exists(os.path.join(ref, sub, f))}
    key = _recipe_key(ref_sha, cflags, ldflags, torch_version)
    if not force and os.path.exists(MANIFEST):
        try:
            old = json.load(open(MANIFEST))
            if old.get("recipe_key") == key and all(os.path.exists(os.path.join(REF_OUT, m["path"])) for m in old["modules"]):
                return MANIFEST
        except (ValueError, KeyError, TypeError):
            pass
    if os.path.exists(MANIFEST):
        os.remove(MANIFEST)                                  # a manifest never describes a half-built set
    units, ref_sha, out_sha = _stage_sources(ref)
    hipcc = _hipcc()
    suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    jobs, links, modules = [], [], []
    for variant, vflags in VARIANTS.items():
        for base, tus in units.items():
            name = base + SUFFIX[variant]
            odir = os.path.join(REF_OUT, "obj", variant, base)
            shutil.rmtree(odir, ignore_errors=True)
            os.makedirs(odir)
            objs = []
            for tu in tus:
                obj = os.path.join(odir, os.path.splitext(os.path.basename(tu))[0] + ".o")
                lang = [] if tu.endswith(".cpp") else ["-x", "hip"]
                flags = [f"--offload-arch={ARCH}"] + vflags + cflags + [f"-DTORCH_EXTENSION_NAME={name}"]
                jobs.append([hipcc] + flags + lang + ["-c", tu, "-o", obj])
                objs.append(obj)
            out = os.path.join(REF_OUT, name + suffix)
            links.append([hipcc, f"--offload-arch={ARCH}"] + objs + ["-o", out] + ldflags)
            modules.append({"name": name, "base": base, "variant": variant, "path": os.path.relpath(out, REF_OUT),
                            "flags": [f"--offload-arch={ARCH}"] + vflags + [c for c in cflags if not c.startswith("-I")]})

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("oracle/ref_build: command failed:\n" + " ".join(cmd) + "\n" + r.stdout[-4000:])

    workers = max(1, min(len(jobs), int(os.environ.get("MAX_JOBS") or 0) or min(os.cpu_count() or 1, 16)))
    with ThreadPoolExecutor(workers) as ex:
        list(ex.map(run, jobs))
        list(ex.map(run, links))
    for m in modules:
        m["sha256"] = _sha(os.path.join(REF_OUT, m["path"]))
    manifest = {"recipe_key": key, "reference_dir": ref, "arch": ARCH, "torch": torch_version, "modules": modules,
                "edits": [{"file": f, "old": old, "new": new, "reason": why} for f, old, new, why in EDITS],
                "reference_sha256": ref_sha, "translated_sha256": out_sha}
    with open(MANIFEST + ".tmp", "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    os.replace(MANIFEST + ".tmp", MANIFEST)
    print(f"oracle/ref_build: {len(modules)} reference modules in {REF_OUT}", flush=True)
    return MANIFEST


def load(name: str, variant: str):
    """Import one built module by path: ``name`` is ref_chamfer_3D or ref_simple_knn, ``variant`` is off or default."""
    import importlib.machinery
    import importlib.util
    import torch  # noqa: F401  (the modules link against torch's libraries)
    man = json.load(open(MANIFEST))
    entry = next(m for m in man["modules"] if m["base"] == name and m["variant"] == variant)
    name, path = entry["name"], os.path.join(REF_OUT, entry["path"])
    loader = importlib.machinery.ExtensionFileLoader(name, path)
    spec = importlib.util.spec_from_file_location(name, path, loader=loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
