#!/usr/bin/env python3
"""Mutation audit of the default render path: would a test fail if one line of the benchmarked kernels were wrong?

    python tools/mutation_audit.py check                    # no GPU, no compiler: every mutant still matches its source
    python tools/mutation_audit.py build [--only a,b]       # no GPU: one library per mutant, csrc/ab/mutants/<name>.so
    python tools/mutation_audit.py run   [--only a,b] [--budget S] [--reuse-t0] [--deselect ID]   # GPU: the quick gate against every mutant

The list is tools/mutants.json: {name, file, find, replace, why, kind} per entry; `find` occurs exactly once in `file`
(a path below dmesh2_renderer_amd/csrc).  A mutant changes a VALUE that ends up in an output tensor -- an operand, a
sign, a constant, a comparison on data, a select's arm, a dropped term, a swapped channel (KINDS below) -- and never an
address, a count of slots, a launch or LDS size, a barrier, fence or wait, a prefetch or a loop bound: a mutant runs on a
shared GPU.  `kind: "equivalent"` marks a mutant no input can tell from the original; its `why` is the argument.

build  brings the unmutated build up to date (make), then per mutant copies the sources to a scratch directory, applies
       the one replacement, recompiles only the translation units that include the changed file (transitively) with
       the Makefile's own flags, and links them with the unmutated objects of the rest.
run    times the quick gate on the unmutated library (t0), then starts one fresh child process per mutant:
       DM2_HIP_LIB=<so> timeout -k 10 <limit> python -m pytest -m gpu -x -q -p no:cacheprovider <gate>, limit =
       max(120 s, 2 t0).  Exit status 1: killed (the first failing test is recorded); 0: survived; anything else -- a
       time limit, an abort, a segmentation fault, a GPU fault in the output -- ends the whole run: nothing more is
       started.  One process at a time, no retries.  Results are merged into profiles/mutation_audit.json.

The quick gate is every tests/test_gpu_*.py without the full-size cases (GATE_K); per mutant the files that exercise
the mutated source come first (FIRST), so that -x ends a killed mutant quickly.  A mutant only a full-size case would
kill counts as a survivor on purpose: what can go wrong at 64 x 64 should be caught at 64 x 64.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmesh2_renderer_amd", "csrc")
LIST = os.path.join(ROOT, "tools", "mutants.json")
OUT_DIR = os.path.join(CSRC, "ab", "mutants")
RESULTS = os.path.join(ROOT, "profiles", "mutation_audit.json")

KINDS = {"operand", "sign", "constant", "comparison", "select arm", "dropped factor", "dropped term", "swapped channel",
         "equivalent"}
FIELDS = ("name", "file", "find", "replace", "why", "kind")
# the audited sources and how many non-equivalent mutants each must have
AUDITED = {"dm2_backward_fast.hip": 10, "dm2_forward_queue.hip": 8, "dm2_prep.hip": 4, "dm2_binning.hip": 4,
           "dm2_clip_fast.h": 4, "dm2_device_math.h": 4,
           # dm2_bwd_shared.h is the accumulator-row layout and the flush table: all but a few lines are addresses
           "dm2_bwd_shared.h": 2}
MIN_TOTAL = 40
MAX_EQUIVALENT = 6

GATE_K = "not full_size and not cfg"
# test files that exercise a source, in the order they go first
FIRST = {
    "dm2_prep.hip": ["test_gpu_prep", "test_gpu_general_cameras", "test_gpu_camera_grad"],
    "dm2_binning.hip": ["test_gpu_binning", "test_gpu_offscreen", "test_gpu_parity", "test_gpu_structured"],
    "dm2_forward_queue.hip": ["test_gpu_parity", "test_gpu_forward_decode", "test_gpu_straightline", "test_gpu_backward_replay",
                              "test_gpu_alpha", "test_gpu_sparse_upstream"],
    "dm2_backward_fast.hip": ["test_gpu_parity", "test_gpu_backward_replay", "test_gpu_alpha", "test_gpu_tie_queue",
                              "test_gpu_sparse_upstream"],
    "dm2_clip_fast.h": ["test_gpu_clippers", "test_gpu_tie_queue", "test_gpu_parity"],
    "dm2_device_math.h": ["test_gpu_parity", "test_gpu_clippers", "test_gpu_tie_queue", "test_gpu_backward_replay"],
    "dm2_bwd_shared.h": ["test_gpu_parity", "test_gpu_backward_replay", "test_gpu_prep"],
}
FATAL_TEXT = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR")


def load_list(path=LIST):
    with open(path) as f:
        return json.load(f)


def check(mutants=None, csrc=CSRC):
    """-> list of problems (empty: the list is sound).  Reads sources only."""
    mutants = load_list() if mutants is None else mutants
    bad, seen, per_file, n_equiv = [], set(), {}, 0
    for m in mutants:
        name = m.get("name", "?")
        for k in FIELDS:
            if not isinstance(m.get(k), str) or not m[k].strip() and k != "replace":
                bad.append(f"{name}: field {k!r} missing or empty")
        if any(k not in m for k in FIELDS):
            continue
        if not re.fullmatch(r"[a-z0-9_]+", name):
            bad.append(f"{name}: names are [a-z0-9_]+ (they become file names)")
        if name in seen:
            bad.append(f"{name}: listed twice")
        seen.add(name)
        if m["kind"] not in KINDS:
            bad.append(f"{name}: kind {m['kind']!r} is not one of {sorted(KINDS)}")
        if m["file"] not in AUDITED:
            bad.append(f"{name}: {m['file']} is not one of the audited sources")
            continue
        if m["find"] == m["replace"]:
            bad.append(f"{name}: replaces nothing")
        with open(os.path.join(csrc, m["file"])) as f:
            n = f.read().count(m["find"])
        if n != 1:
            bad.append(f"{name}: `find` occurs {n} times in {m['file']}, not once")
        if m["kind"] == "equivalent":
            n_equiv += 1
        else:
            per_file[m["file"]] = per_file.get(m["file"], 0) + 1
    for f, need in AUDITED.items():
        if per_file.get(f, 0) < need:
            bad.append(f"{f}: {per_file.get(f, 0)} non-equivalent mutants, at least {need} asked")
    if sum(per_file.values()) < MIN_TOTAL:
        bad.append(f"{sum(per_file.values())} non-equivalent mutants, at least {MIN_TOTAL} asked")
    if n_equiv > MAX_EQUIVALENT:
        bad.append(f"{n_equiv} equivalent mutants, at most {MAX_EQUIVALENT}")
    return bad


# ---- build -------------------------------------------------------------------------------------------------------------------

def _includes(path):
    with open(path) as f:
        return [os.path.basename(x) for x in re.findall(r'^#include "([^"]+)"', f.read(), re.M)]


def units_including(header_or_unit, csrc=CSRC):
    """The translation units (*.hip of the Makefile's SRCS) that include a file of csrc, transitively; a unit: itself."""
    units = _make_var("SRCS").split()
    if header_or_unit in units:
        return [header_or_unit]
    out = []
    for u in units:
        todo, seen = [u], set()
        while todo:
            x = todo.pop()
            if x in seen or not os.path.exists(os.path.join(csrc, x)):
                continue
            seen.add(x)
            todo += _includes(os.path.join(csrc, x))
        if header_or_unit in seen:
            out.append(u)
    return out


def _make_var(name):
    """A variable of csrc/Makefile as written (continuation lines joined), $(ARCH) / $(EXTRA) resolved."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        text = f.read().replace("\\\n", " ")
    m = re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M)
    if not m:
        raise SystemExit(f"csrc/Makefile has no {name}")
    return m.group(1).replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").strip()


def _build_one_unit(hipcc, flags, src_dir, unit, obj):
    subprocess.run([hipcc, *flags, "-c", unit, "-o", obj], cwd=src_dir, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def build(only=None, jobs=16):
    bad = check()
    if bad:
        raise SystemExit("mutants.json:\n  " + "\n  ".join(bad))
    jobs = max(1, min(int(jobs), 16))
    subprocess.check_call(["make", "-C", CSRC, "-j", str(jobs), "ARCH=gfx950"])
    hipcc = os.environ.get("HIPCC", _make_var("HIPCC"))
    flags = _make_var("HIPFLAGS").split()
    units = _make_var("SRCS").split()
    base_objs = {u: os.path.join(CSRC, "build", u[:-4] + ".o") for u in units}
    mutants = [m for m in load_list() if only is None or m["name"] in only]
    os.makedirs(OUT_DIR, exist_ok=True)
    work = tempfile.mkdtemp(prefix="dm2_mutants_")
    try:
        tasks = []
        for m in mutants:
            # the sources keep their place relative to include/ (dm2_state.h reaches it as ../../include/dm2_hip.h)
            src = os.path.join(work, m["name"], "dmesh2_renderer_amd", "csrc")
            os.makedirs(src)
            for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
                shutil.copy(p, src)
            shutil.copytree(os.path.join(ROOT, "include"), os.path.join(work, m["name"], "include"))
            p = os.path.join(src, m["file"])
            with open(p) as f:
                text = f.read()
            with open(p, "w") as f:
                f.write(text.replace(m["find"], m["replace"]))
            m["_src"], m["_units"] = src, units_including(m["file"])
            tasks += [(m, u) for u in m["_units"]]
        print(f"{len(mutants)} mutants, {len(tasks)} translation units to compile, -j{jobs}", flush=True)
        failed = {}
        with ThreadPoolExecutor(jobs) as pool:
            futs = [(m, u, pool.submit(_build_one_unit, hipcc, flags, m["_src"], u, os.path.join(m["_src"], u[:-4] + ".o")))
                    for m, u in tasks]
            for m, u, fu in futs:
                try:
                    fu.result()
                except subprocess.CalledProcessError as e:
                    failed[m["name"]] = e.stdout.decode(errors="replace")[-2000:]
        for m in mutants:
            if m["name"] in failed:
                continue
            objs = [os.path.join(m["_src"], u[:-4] + ".o") if u in m["_units"] else base_objs[u] for u in units]
            out = os.path.join(OUT_DIR, m["name"] + ".so")
            subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, *objs])
            print(f"built {os.path.relpath(out, ROOT)} ({len(m['_units'])} units)", flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if failed:        # a mutant that does not compile is a defect of the list
        for n, log in failed.items():
            print(f"---- {n} does not compile:\n{log}", file=sys.stderr)
        raise SystemExit(f"{len(failed)} mutants do not compile: {', '.join(failed)}")


# ---- run ---------------------------------------------------------------------------------------------------------------------

def gate_files(source=None):
    """The quick gate's files, relative to the repository; those that exercise `source` first."""
    files = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    first = [f for f in FIRST.get(source, []) if f in files]
    return [f"tests/{f}.py" for f in first + [f for f in files if f not in first]]


def gate_command(limit, source=None, deselect=()):
    return ["timeout", "-k", "10", str(int(limit)), sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
            "-k", GATE_K, *[f"--deselect={d}" for d in deselect], *gate_files(source)]


def _run_gate(limit, lib, source, deselect=(), echo=False):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    if lib:
        env["DM2_HIP_LIB"] = lib
    else:
        env.pop("DM2_HIP_LIB", None)
    t = time.time()
    p = subprocess.Popen(gate_command(limit, source, deselect), cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    chunks = []
    while True:                                   # (read as it comes: with `echo` the caller sees the gate's progress)
        c = os.read(p.stdout.fileno(), 65536)
        if not c:
            break
        chunks.append(c)
        if echo:
            sys.stdout.write(c.decode(errors="replace")); sys.stdout.flush()
    rc = p.wait()
    return rc, b"".join(chunks).decode(errors="replace"), time.time() - t


def _first_failure(out):
    m = re.search(r"^(?:FAILED|ERROR) (\S+)", out, re.M)
    return m.group(1) if m else None


def _save(res):
    os.makedirs(os.path.dirname(RESULTS), exist_ok=True)
    with open(RESULTS, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def run(only=None, budget=None, reuse_t0=False, deselect=()):
    bad = check()
    if bad:
        raise SystemExit("mutants.json:\n  " + "\n  ".join(bad))
    res = {"gate": "", "t0": None, "mutants": {}}
    if os.path.exists(RESULTS):
        with open(RESULTS) as f:
            res.update(json.load(f))
    mutants = [m for m in load_list() if only is None or m["name"] in only]
    missing = [m["name"] for m in mutants if not os.path.exists(os.path.join(OUT_DIR, m["name"] + ".so"))]
    if missing:
        raise SystemExit(f"not built (run `build` first): {', '.join(missing)}")
    start = time.time()
    res["gate"] = f"python -m pytest -m gpu -x -q -p no:cacheprovider -k \"{GATE_K}\" tests/test_gpu_*.py (the mutated source's files first)"
    print("gate:", " ".join(gate_command(0, None, deselect)[4:]), flush=True)
    if reuse_t0 and res.get("t0"):
        t0 = float(res["t0"])             # (a run split over several calls: the unmutated gate was timed by the first)
    else:
        # t0: the gate on the unmutated library, with a generous limit of its own
        rc, out, t0 = _run_gate(1100, None, None, deselect, echo=True)
        print(f"unmutated: exit {rc}, {t0:.1f} s", flush=True)
        if rc != 0:
            raise SystemExit("the quick gate does not pass on the unmutated library: nothing to audit against")
        res["t0"] = round(t0, 1)
    limit = max(120.0, 2.0 * t0)          # from the unmutated run, never from a mutant's
    _save(res)
    for m in mutants:
        if budget is not None and time.time() - start + min(t0, limit) > budget:
            print(f"budget: {m['name']} and what follows are left for another run", flush=True)
            break
        rc, out, secs = _run_gate(limit, os.path.join(OUT_DIR, m["name"] + ".so"), m["file"], deselect)
        fatal = rc not in (0, 1) or any(s in out for s in FATAL_TEXT)
        old = res["mutants"].get(m["name"], {})
        entry = {"file": m["file"], "kind": m["kind"], "seconds": round(secs, 1), "exit": rc,
                 "verdict": "not completed" if fatal else ("killed" if rc == 1 else "survived"),
                 "killed_by": None if fatal or rc == 0 else _first_failure(out)}
        # what the first run of this mutant said stays on record when it is run again against new tests
        entry["first_verdict"] = old.get("first_verdict", old.get("verdict", entry["verdict"]))
        res["mutants"][m["name"]] = entry
        _save(res)
        print(f"{m['name']}: {entry['verdict']} ({secs:.1f} s) {entry['killed_by'] or ''}", flush=True)
        if fatal:
            print(out[-3000:], flush=True)
            raise SystemExit(f"{m['name']} did not run to completion (exit {rc}): nothing more is started")
    v = [e["verdict"] for e in res["mutants"].values()]
    print(f"killed {v.count('killed')}, survived {v.count('survived')}, t0 = {res['t0']} s", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("check")
    b = sub.add_parser("build")
    b.add_argument("--only", help="comma-separated mutant names")
    b.add_argument("-j", "--jobs", type=int, default=16, help="at most 16")
    r = sub.add_parser("run")
    r.add_argument("--only", help="comma-separated mutant names")
    r.add_argument("--deselect", action="append", default=[], help="a test id left out of the gate (what did the suite catch before this test?)")
    r.add_argument("--reuse-t0", action="store_true", help="take t0 from profiles/mutation_audit.json (a run split over several calls)")
    r.add_argument("--budget", type=float, help="start no mutant that might end later than this many seconds into the run")
    a = ap.parse_args(argv)
    only = set(a.only.split(",")) if getattr(a, "only", None) else None
    if a.cmd == "check":
        bad = check()
        for x in bad:
            print(x, file=sys.stderr)
        print(f"{len(load_list())} mutants, {len(bad)} problems")
        return 1 if bad else 0
    if a.cmd == "build":
        build(only, a.jobs)
    else:
        run(only, a.budget, a.reuse_t0, tuple(a.deselect))
    return 0


if __name__ == "__main__":
    sys.exit(main())
