"""The shim's per-slot lookup ops (texture, cube, volume, hash grid and the two mip-mapped ones) and the two chain ops, held
without a GPU to what tests/golden/lookup_shim_errors.json and lookup_shim_calls.json recorded (tests/shim_trace.py): every
error's type and whole message, which of two errors wins, and every word and pointer handed to the library."""
import json
import os

import pytest

import shim_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _families(table):
    return sorted({k.split("-")[0] for k in table})


@pytest.fixture(scope="module")
def errors():
    return shim_trace.errors()


@pytest.fixture(scope="module")
def calls():
    return shim_trace.calls()


ERRORS, CALLS = _golden("lookup_shim_errors.json"), _golden("lookup_shim_calls.json")


@pytest.mark.parametrize("family", _families(ERRORS))
def test_errors_keep_type_message_and_order(errors, family):
    assert sorted(errors) == sorted(ERRORS)
    for case in (k for k in ERRORS if k.split("-")[0] == family):
        assert errors[case] == ERRORS[case], case


@pytest.mark.parametrize("family", _families(CALLS))
def test_library_calls_keep_every_word_and_pointer(calls, family):
    assert sorted(calls) == sorted(CALLS)
    for case in (k for k in CALLS if k.split("-")[0] == family):
        assert json.loads(json.dumps(calls[case])) == CALLS[case], case


def test_the_tables_cover_what_they_claim():
    ops = ["texture", "texture_cube", "texture_volume", "hash_grid", "texture_mip", "texture_cube_mip"]
    assert _families(ERRORS) == sorted(ops + ["texture_mipmaps", "cube_prefilter"])
    assert _families(CALLS) == sorted(ops + ["texture_mipmaps", "cube_prefilter"])
    for op in ops:
        for way in ("forward", "backward"):
            both = [k for k in ERRORS if k.startswith(f"{op}-{way}-") and "+" in k]
            assert len(both) >= 3, (op, way)                              # two errors at once: which one wins
            assert ERRORS[f"{op}-{way}-valid"]["raw"][1].startswith("dmesh2_renderer_amd: all tensors must live on a ROCm GPU")
            assert ERRORS[f"{op}-{way}-valid"]["traced"] is None
        empty = [k for k in CALLS if k.startswith(f"{op}-") and "-empty-" in k]
        assert empty and all(CALLS[k]["calls"] == [] for k in empty)      # the empty grid launches nothing
        nothing = [k for k in CALLS if k.startswith(f"{op}-backward-nothing")]
        assert nothing and all(CALLS[k] == {"calls": [], "returns": [None] * len(CALLS[k]["returns"])} for k in nothing)
        assert all(len(v["calls"]) == 1 for k, v in CALLS.items() if k.startswith(f"{op}-") and "empty" not in k and "nothing" not in k)
