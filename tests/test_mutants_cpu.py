"""tools/mutants.json against the sources it mutates (tools/mutation_audit.py check): a kernel edit that orphans a mutant fails
here, without a GPU or a compiler, so the list does not rot; and profiles/mutation_audit.json, the record of its last run, names
the mutants of the list and a killing test that exists."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def audit():
    spec = importlib.util.spec_from_file_location("mutation_audit", os.path.join(ROOT, "tools", "mutation_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_mutant_matches_its_source_exactly_once(audit):
    assert audit.check() == []


def test_check_notices_an_orphaned_and_an_ambiguous_mutant(audit):
    ms = audit.load_list()
    gone = dict(ms[0], find=ms[0]["find"] + " /* no such text */")
    twice = dict(ms[1], find="const ")
    bad = audit.check([gone, twice] + ms[2:])
    assert any(b.startswith(gone["name"] + ":") and "occurs 0 times" in b for b in bad), bad
    assert any(b.startswith(twice["name"] + ":") and "not once" in b for b in bad), bad
    assert any("is not one of" in b for b in audit.check([dict(ms[0], kind="loop bound")] + ms[1:]))


def test_a_header_rebuilds_the_units_that_include_it_and_a_unit_only_itself(audit):
    assert audit.units_including("dm2_prep.hip") == ["dm2_prep.hip"]
    assert sorted(audit.units_including("dm2_clip_fast.h")) == ["dm2_backward_fast.hip", "dm2_debug.hip"]
    through = audit.units_including("dm2_device_math.h")                  # (dm2_stage.h, dm2_pairs.h, ... pass it on)
    assert "dm2_forward_queue.hip" in through and "dm2_binning.hip" in through and "dm2_prep.hip" not in through


def test_the_gate_puts_the_mutated_sources_files_first_and_leaves_none_out(audit):
    every = set(audit.gate_files())
    assert every and all(os.path.exists(os.path.join(ROOT, f)) for f in every)
    for src, first in audit.FIRST.items():
        files = audit.gate_files(src)
        assert set(files) == every and files[:len(first)] == [f"tests/{f}.py" for f in first], src


def test_the_recorded_run_is_of_this_list(audit):
    path = os.path.join(ROOT, "profiles", "mutation_audit.json")
    with open(path) as f:
        res = json.load(f)
    names = {m["name"]: m for m in audit.load_list()}
    assert set(res["mutants"]) <= set(names), sorted(set(res["mutants"]) - set(names))
    assert res["t0"] > 0
    for n, e in res["mutants"].items():
        assert e["verdict"] in ("killed", "survived"), (n, e)
        if e["verdict"] == "killed":
            path_, _, test = e["killed_by"].partition("::")
            assert os.path.exists(os.path.join(ROOT, path_)), (n, e)
            with open(os.path.join(ROOT, path_)) as f:
                assert f"def {test.split('[')[0]}(" in f.read(), (n, e)
        else:                                                              # a survivor on record is an equivalent mutant
            assert names[n]["kind"] == "equivalent", (n, e)


def test_the_design_table_agrees_with_the_recorded_run(audit):
    with open(os.path.join(ROOT, "profiles", "mutation_audit.json")) as f:
        res = json.load(f)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        rows = {ln.split("`")[1]: ln for ln in f if ln.startswith("| `") and ln.rstrip().endswith(("| yes |", "| no |"))}
    for m in audit.load_list():
        e = res["mutants"][m["name"]]
        if m["kind"] == "equivalent":
            assert e["verdict"] == "survived" and m["name"] not in rows, m["name"]
            continue
        row = rows[m["name"]]
        assert e["killed_by"].replace("tests/", "") in row, (m["name"], row)
        assert row.rstrip().endswith("| yes |" if e["first_verdict"] == "killed" else "| no |"), (m["name"], row)
