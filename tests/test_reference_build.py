"""oracle/build_ref.py's product: where the reference project's sources are present, build() must have left both reference
modules and their manifest in oracle/_ref/ (a missing manifest is a failure, not a skip), and both must import and expose the
reference's three entry points.  Importing needs no GPU.  Where neither the sources nor a manifest exist, there is nothing to
check."""
import os
import sys

import pytest

import reference_lib as RL
from util import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402


def _manifest_or_skip():
    have_sources = os.path.isdir(build_ref.reference_dir())
    m = RL.manifest()
    if m is None and not have_sources:
        pytest.skip("no reference sources and no reference build")
    assert m is not None, "the reference sources are present but build() left no oracle/_ref/MANIFEST.json"
    return m, have_sources


def test_manifest_describes_the_build():
    m, have_sources = _manifest_or_skip()
    assert set(m["modules"]) == set(RL.VARIANTS) == set(m["flags"])
    for v in RL.VARIANTS:
        assert m["modules"][v].startswith(build_ref.module_name(v))
        assert os.path.isfile(os.path.join(RL.REF_DIR, m["modules"][v])), m["modules"][v]
    assert "-ffp-contract=off" in m["flags"]["strict"] and "-ffp-contract=off" not in m["flags"]["shipped"]
    assert not any("xnack" in f or "sanitize" in f for fl in m["flags"].values() for f in fl)
    assert len(m["source_hash"]) == 64 and len(m["recipe_hash"]) == 64 and m["hipcc"]
    # oracle/_ref/ holds the modules and the manifest, nothing else (no translated source)
    assert sorted(os.listdir(RL.REF_DIR)) == sorted(["MANIFEST.json", *m["modules"].values()])
    if have_sources:
        ref = build_ref.reference_dir()
        assert m["source_hash"] == build_ref._hash_files(ref, build_ref._source_files(ref)), "oracle/_ref/ is stale: run build()"


@pytest.mark.parametrize("variant", RL.VARIANTS)
def test_modules_import_and_expose_the_entry_points(variant):
    _manifest_or_skip()
    mod = RL.load(variant)
    assert mod is not None and mod.__name__ == build_ref.module_name(variant)
    for name in RL.ENTRY_POINTS:
        assert callable(getattr(mod, name)), name


def test_adjustments_are_generic():
    """The recipe's text substitutions on made-up text: launch brackets closed up, __trap() replaced, the vector overloads of
    smoothstep removed to their closing brace, the scalar one and everything around kept."""
    src = ("__device__ float smoothstep(float lo, float hi, float t)\n{\n    return lo;\n}\n"
           "inline __host__ __device__ float3 smoothstep(float3 lo, float3 hi, float3 t)\n{\n    if (t.x) { return lo; }\n    return hi;\n}\n"
           "static float2 smoothstep (float2 q)\n{ return q; }\n"
           "void f() { k << <g, b >> > (1); if (0) __trap(); }\n")
    out = build_ref._adjust(src)
    assert out == ("__device__ float smoothstep(float lo, float hi, float t)\n{\n    return lo;\n}\n"
                   "\n\n"
                   "void f() { k <<<g, b >>> (1); if (0) abort(); }\n")
