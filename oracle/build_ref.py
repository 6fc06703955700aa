"""TEST INFRASTRUCTURE: builds the reference project's own kernels for gfx950 into oracle/_ref/.

The reference is CUDA source.  torch's Python hipify translates it, a handful of mechanical adjustments make hipcc accept it,
and the objects are linked into two Python modules that expose the reference's three entry points
(``render_forward_cuda``, ``render_backward_cuda``, ``generate_render_layers_cuda``) with its own argument lists:

  dm2_ref_strict   -ffp-contract=off on device and host, as the oracle and the HIP kernels are built: bit-compared
  dm2_ref_shipped  the compiler's default contraction: the closest thing to the -fmad=true build the reference's users run

Neither is a CUDA build: both are the reference's text compiled by hipcc for gfx950.

All work happens in a temporary directory outside the repository, which is removed afterwards; oracle/_ref/ receives the linked
modules and MANIFEST.json only (source hash, recipe hash, flags, compiler version, file names).  Nothing of the reference,
translated or compiled, belongs in git: oracle/_ref/ is ignored.

The adjustments (identifiers and header names only):
  1. empty stub headers for glm/glm.hpp (included, unused), device_launch_parameters.h and cooperative_groups/reduce.h;
  2. spaced kernel-launch brackets are closed up;
  3. __trap() becomes abort() (it sits in a function nothing calls);
  4. the smoothstep overloads that return float2/float3/float4 are removed: their vector / and * are ambiguous against HIP's
     own vector operators and nothing uses them;
  5. CUB and cooperative groups need nothing: hipify maps them to hipCUB and hip/hip_cooperative_groups.h.
"""
from __future__ import annotations

import concurrent.futures
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import sysconfig
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "_ref")
MANIFEST = os.path.join(OUT_DIR, "MANIFEST.json")
ARCH = "gfx950"
SOURCES = ["cuda_impl/forward.cu", "cuda_impl/backward.cu", "cuda_impl/renderer.cu", "render.cu"]     # device objects
HOST_SOURCE = "ext.cpp"
STUB_HEADERS = ["glm/glm.hpp", "device_launch_parameters.h", "cooperative_groups/reduce.h"]
COMMON_FLAGS = ["-std=c++17", "-O2", "-fPIC", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1"]
VARIANTS = {"strict": ["-ffp-contract=off"], "shipped": []}
LINK_LIBS = ["-ltorch", "-ltorch_cpu", "-ltorch_hip", "-lc10", "-lc10_hip", "-ltorch_python"]
TEXT_EXT = (".cu", ".cuh", ".h", ".hpp", ".cpp", ".hip")


def reference_dir() -> str:
    return os.environ.get("DM2_REFERENCE", "/root/reference")


def module_name(variant: str) -> str:
    return "dm2_ref_" + variant


def _rocm() -> str:
    return os.environ.get("ROCM_PATH", "/opt/rocm")


def _hipcc() -> str:
    return os.environ.get("HIPCC", os.path.join(_rocm(), "bin", "hipcc"))


def _source_files(ref: str) -> list[str]:
    out = [HOST_SOURCE, "render.cu", "render.h"]
    for n in sorted(os.listdir(os.path.join(ref, "cuda_impl"))):
        if n.endswith(TEXT_EXT):
            out.append("cuda_impl/" + n)
    return out


def _hash_files(base: str, names: list[str]) -> str:
    h = hashlib.sha256()
    for n in names:
        h.update(n.encode() + b"\0")
        with open(os.path.join(base, n), "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()


def _hipcc_version() -> str:
    out = subprocess.run([_hipcc(), "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    return out.strip().splitlines()[0]


def _strip_vector_overloads(text: str, name: str) -> str:
    """Remove every definition of ``name`` whose return type is float2, float3 or float4: from the start of its declaration
    (qualifiers included) to the brace that closes its body."""
    pat = re.compile(r"(?:^[ \t]*(?:inline|static|__host__|__device__|__forceinline__)\b[^\n;{}()]*?|^[ \t]*)"
                     r"\bfloat[234]\s+" + re.escape(name) + r"\s*\(", re.M)
    while True:
        m = pat.search(text)
        if m is None:
            return text
        i = text.index("{", m.end())
        depth, j = 1, i + 1
        while depth:
            c = text[j]
            depth += (c == "{") - (c == "}")
            j += 1
        text = text[:m.start()] + text[j:]


def _adjust(text: str) -> str:
    text = re.sub(r"<<\s+<", "<<<", text)
    text = re.sub(r">>\s+>", ">>>", text)
    text = re.sub(r"\b__trap\s*\(\s*\)", "abort()", text)
    return _strip_vector_overloads(text, "smoothstep")


def _translate(src: str) -> dict[str, str]:
    """hipify the copied tree in place, apply the adjustments to every translated file.  -> {original path: translated path}."""
    import contextlib
    import io
    from torch.utils.hipify import hipify_python
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):   # (its progress report)
        res = hipify_python.hipify(project_directory=src, output_directory=src, includes=[os.path.join(src, "*")],
                                   show_detailed=False, show_progress=False, is_pytorch_extension=True)
    out = {}
    for orig, r in res.items():
        path = getattr(r, "hipified_path", None) or orig
        out[os.path.relpath(orig, src)] = path
    for path in sorted(set(out.values())):
        if os.path.isfile(path) and path.endswith(TEXT_EXT):
            with open(path) as f:
                t = f.read()
            with open(path, "w") as f:
                f.write(_adjust(t))
    return out


def _run(cmd: list[str], cwd: str) -> None:
    p = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("reference build failed (exit %d): %s\n%s" % (p.returncode, " ".join(cmd), p.stdout[-8000:]))


def _include_flags(work: str, moved: dict[str, str]) -> list[str]:
    from torch.utils import cpp_extension
    inc = [os.path.join(work, "stubs")] + sorted({os.path.dirname(p) for p in moved.values()})
    inc += cpp_extension.include_paths()
    inc += [sysconfig.get_paths()["include"], os.path.join(_rocm(), "include")]
    seen, flags = set(), []
    for d in inc:
        if d not in seen:
            seen.add(d)
            flags.append("-I" + d)
    return flags


def build(jobs: int | None = None, force: bool = False) -> bool:
    """Build both variants into oracle/_ref/.  -> True when modules are in place (built or up to date), False when skipped
    because the reference directory is absent.  A failed compile raises with the compiler's output and leaves oracle/_ref/
    without a manifest (so nothing half-written is ever loaded)."""
    ref = reference_dir()
    if not os.path.isdir(ref):
        print("oracle/build_ref: no reference at %s, skipped (oracle/_ref/ left as it is)" % ref)
        return False
    import torch  # noqa: F401  (hipify and the include / library paths come with it)
    from torch.utils import cpp_extension

    names = _source_files(ref)
    with open(os.path.abspath(__file__), "rb") as f:
        recipe_hash = hashlib.sha256(f.read()).hexdigest()
    ext_suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    want = dict(source_hash=_hash_files(ref, names), recipe_hash=recipe_hash, hipcc=_hipcc_version(), arch=ARCH,
                torch=torch.__version__,
                modules={v: module_name(v) + ext_suffix for v in VARIANTS},
                flags={v: COMMON_FLAGS + VARIANTS[v] for v in VARIANTS})
    if not force and os.path.isfile(MANIFEST):
        try:
            with open(MANIFEST) as f:
                have = json.load(f)
        except ValueError:
            have = None
        if have == want and all(os.path.isfile(os.path.join(OUT_DIR, m)) for m in want["modules"].values()):
            print("oracle/build_ref: oracle/_ref/ is up to date, skipped")
            return True

    jobs = jobs or min(8, os.cpu_count() or 1)
    work = tempfile.mkdtemp(prefix="dm2_ref_build_")
    repo = os.path.dirname(HERE)
    assert os.path.commonpath([os.path.realpath(work), os.path.realpath(repo)]) != os.path.realpath(repo), work
    try:
        src = os.path.join(work, "src")
        for n in names:
            os.makedirs(os.path.dirname(os.path.join(src, n)), exist_ok=True)
            shutil.copyfile(os.path.join(ref, n), os.path.join(src, n))
        for n in STUB_HEADERS:
            p = os.path.join(work, "stubs", n)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "w") as f:
                f.write("#pragma once\n")
        moved = _translate(src)
        inc = _include_flags(work, moved)

        tasks, objs = [], {v: [] for v in VARIANTS}
        for v, extra in VARIANTS.items():
            os.makedirs(os.path.join(work, "obj", v))
            define = "-DTORCH_EXTENSION_NAME=" + module_name(v)
            for s in SOURCES:
                o = os.path.join(work, "obj", v, os.path.basename(s) + ".o")
                objs[v].append(o)
                tasks.append([_hipcc(), "--offload-arch=" + ARCH, *COMMON_FLAGS, *extra, define, *inc, "-c", moved[s], "-o", o])
            o = os.path.join(work, "obj", v, HOST_SOURCE + ".o")
            objs[v].append(o)
            tasks.append([os.environ.get("CXX", "g++"), *COMMON_FLAGS, *extra, define, *inc, "-c", moved[HOST_SOURCE], "-o", o])
        tasks.sort(key=lambda c: 0 if "renderer" in c[-3] else 1)            # the longest compile (hipCUB) starts first
        with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as ex:
            for fut in [ex.submit(_run, c, work) for c in tasks]:
                fut.result()

        libdirs = ["-L" + d for d in cpp_extension.library_paths()]
        os.makedirs(os.path.join(work, "out"))
        for v in VARIANTS:
            _run([_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", os.path.join(work, "out", want["modules"][v]),
                  *objs[v], *libdirs, *LINK_LIBS], work)

        # publish: manifest away first, modules, manifest last
        os.makedirs(OUT_DIR, exist_ok=True)
        if os.path.exists(MANIFEST):
            os.remove(MANIFEST)
        for old in os.listdir(OUT_DIR):
            if old.startswith("dm2_ref_"):
                os.remove(os.path.join(OUT_DIR, old))
        for m in want["modules"].values():
            shutil.copyfile(os.path.join(work, "out", m), os.path.join(OUT_DIR, m + ".part"))
            os.replace(os.path.join(OUT_DIR, m + ".part"), os.path.join(OUT_DIR, m))
        with open(MANIFEST + ".part", "w") as f:
            json.dump(want, f, indent=1, sort_keys=True)
        os.replace(MANIFEST + ".part", MANIFEST)
        print("oracle/build_ref: built " + ", ".join(sorted(want["modules"].values())))
        return True
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    build(force="--force" in sys.argv[1:])
