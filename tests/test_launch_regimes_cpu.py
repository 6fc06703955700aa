"""tests/launch_regimes.py against the sources, without a GPU: the sweep model is right for every CV, wrong variants of it are told
apart by the channel counts of tests/test_gpu_launch_regimes.py, the stepping lines it restates still stand in the four kernels,
the hash grid's level model agrees with tests/hash_grid_ref.py, and every row of the census quotes its launcher and names a test
that exists and whose parameters enter the row's regime."""
import os
import re

import numpy as np
import pytest

import hash_grid_ref as href
import launch_regimes as lr

NSLOTS = (1, 255, 256)


def _src(name):
    with open(os.path.join(lr.CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("nslots", NSLOTS)
def test_every_lane_of_every_sweep_visits_divmod(nslots):
    CVs = np.arange(1, 1101)
    wrong = lr.sweeps_wrong(nslots, CVs)
    assert not wrong.any(), CVs[wrong][:10]


def test_the_two_statements_of_the_model_agree():
    """``sweep`` lane by lane and ``sweeps_wrong`` on whole blocks: the same verdict on the model and on each wrong variant, at
    the channel counts of both generations of lists."""
    CVs = sorted({lr.wide_cv(op, C, sh) for op in lr.WIDE_OPS for C, sh in lr.wide_cases(op)} | {1, 2, 3, 4, 7, 16, 33})
    for variant in (None,) + lr.VARIANTS:
        for nslots in (3, 256):
            vec = lr.sweeps_wrong(nslots, CVs, variant)
            for CV, w in zip(CVs, vec):
                assert lr.sweep_is_right(nslots, CV, variant) == (not w), (variant, nslots, CV)


def _catchers(variant, CVs):
    """The CVs of ``CVs`` at which some block of the GPU module's shapes (a full one of 256 slots, a ragged one of 3, and the 80
    slots of the two-view shape) shows the variant."""
    CVs = np.asarray(sorted(CVs))
    wrong = np.zeros(len(CVs), bool)
    for nslots in (256, 3, 80):
        wrong |= lr.sweeps_wrong(nslots, CVs, variant)
    return set(CVs[wrong].tolist())


def test_wrong_variants_against_the_old_and_the_new_lists():
    """What separates the regimes.  Every variant is caught on both paths of the new lists.  A dq floored at 1 differs from the
    kernels only where CV > 256: no C <= 33 (CV <= 33 on either path) can tell it from them, and of the new values exactly the
    two with CV > 256 do.  The other two variants are wrong wherever a carry is due, which needs dr > 0: C = 3, 7 and 33 of the
    old scalar lists see them (no vector CV of the old texture, cube and volume lists does: 1, 2 and 4 all divide 256, so the
    carry of the vector path was first run by the mip op's C = 12 and 20), and so does every new value but CV = 256."""
    scalar = {lr.wide_cv("texture", C, sh) for C, sh in lr.wide_cases("texture") if lr.wide_cv("texture", C, sh) == C}
    vector = {lr.wide_cv("texture", C, sh) for C, sh in lr.wide_cases("texture") if lr.wide_cv("texture", C, sh) != C}
    assert scalar == {131, 256, 259} and vector == {3, 129, 256, 257}
    for variant in lr.VARIANTS:
        assert _catchers(variant, scalar) and _catchers(variant, vector), variant
    assert _catchers("dq floored at 1", lr.OLD_CS) == set()
    assert _catchers("dq floored at 1", range(1, 257)) == set()
    assert _catchers("dq floored at 1", scalar | vector) == {257, 259}
    carries = {C for C in lr.OLD_CS if 256 % C}
    assert _catchers("carry omitted", lr.OLD_CS) == carries and {3, 7, 33} <= carries
    assert _catchers("> for >= in the carry", lr.OLD_CS) <= carries and 3 in _catchers("> for >= in the carry", lr.OLD_CS)
    old_vector = {1, 2, 4}                               # C = 4, 8, 16 of the texture, cube and volume lists
    for variant in ("carry omitted", "> for >= in the carry"):
        assert _catchers(variant, old_vector) == set()
        assert _catchers(variant, scalar | vector) >= {3, 129, 131, 257, 259}, variant
    # the new lists are the smallest that enter every regime on both paths: one value per regime the old lists left out
    assert {lr.sweep_regime(CV) for CV in scalar} == set(lr.REGIMES[2:])
    assert {lr.sweep_regime(CV) for CV in vector} == {lr.REGIMES[0]} | set(lr.REGIMES[2:])
    assert {lr.sweep_regime(CV) for CV in lr.OLD_CS} == set(lr.REGIMES[:2])


@pytest.mark.parametrize("sweep", lr.SWEEPS, ids=[s[0] for s in lr.SWEEPS])
def test_the_sources_still_step_as_the_model_does(sweep):
    name, _, block, cv = sweep
    src = _src(name)
    for line in lr.stepping_lines(block, cv):
        assert src.count(line) == 1, (name, line, src.count(line))
    assert re.search(rf"constexpr int {block} = {lr.BLOCK};", src + _src("dm2_tex_core.h")), block


def test_the_shared_sweep_has_the_three_callers_the_census_lists():
    for name in os.listdir(lr.CSRC):
        if name.endswith(".hip"):
            assert ("tex_sweep<" in _src(name)) == (name in lr.TEX_SWEEP_CALLERS), name


@pytest.mark.parametrize("case", list(lr.HASH_CASES))
def test_hash_levels_against_the_reference(case):
    N, q, NL, lg, Fs = lr.HASH_CASES[case]
    R, dense = lr.hash_levels(N, q, NL, lg)
    assert R == href.resolutions(NL, N, q)
    assert [bool(dense >> v & 1) for v in range(NL)] == [href.is_dense(r, 1 << lg) for r in R]
    assert dense < 1 << 32 and max(R) <= 1 << 20 and all(F in (1, 2, 4, 8) for F in Fs)
    assert NL * max(Fs) << lg <= 0x7FFFFFFF


def test_hash_cases_are_what_their_names_say():
    lev = {k: lr.hash_levels(*v[:4]) for k, v in lr.HASH_CASES.items()}
    R, dense = lev["32 levels"]
    assert len(R) == 32 and R[0] ** 3 == 4096 and dense == 1 and R[-1] == 70
    assert lev["32 levels, 17 dense"][1] == (1 << 17) - 1
    assert lev["32 levels, all dense"][1] == 0xFFFFFFFF
    R, dense = lev["workload"]
    assert len(R) == 16 and R[:5] == [16, 24, 36, 54, 81] and dense == 0xF
    assert lev["finest 2^20"] == ([1 << 20], 0) and lev["finest 2^19, 2^20"] == ([1 << 19, 1 << 20], 0)
    assert lev["2^24 rows, dense"] == ([256], 1) and 256 ** 3 == 1 << 24 and lev["2^24 rows, hashed"] == ([257], 0)
    for bad in ((1 << 20, 32, 2, 16), ((1 << 20) + 1, 32, 1, 16), (16, 16, 2, 12), (16, 24, 33, 12), (16, 24, 2, 25)):
        with pytest.raises(ValueError):
            lr.hash_levels(*bad)


def test_every_row_quotes_its_launcher_and_names_a_test_that_exists():
    assert len(lr.TABLE) > 90
    for row in lr.TABLE:
        name = row["where"].split(":")[0]
        src = _src(name)
        assert row["condition"] in src, (row["op"], row["regime"], row["condition"])
        for fn in row["where"].split(":")[1].split(", "):
            assert re.search(rf"\b{re.escape(fn.split(' ')[0])}\b", src), (row["where"], fn)
        path, _, test = row["test"].partition("::")
        assert os.path.exists(os.path.join(lr.ROOT, path)), row
        with open(os.path.join(lr.ROOT, path)) as f:
            assert f"def {test}(" in f.read(), row


def test_the_new_modules_lists_enter_every_row_marked_as_theirs():
    mine = [r for r in lr.TABLE if r["test"].startswith(lr.NEW)]
    assert len(mine) > 40
    theirs = [r for r in lr.TABLE if r["enters"] is not None and not r["test"].startswith(lr.NEW)]
    assert len(theirs) == 19 and all(r["regime"].startswith("sweep") for r in theirs)      # the op files' lists, read from their sources
    for row in lr.TABLE:
        assert row["enters"] is not None or not (row["test"].startswith(lr.NEW) or row["regime"].startswith("sweep")), row
        if row["enters"] is not None:
            assert row["enters"](), (row["op"], row["kernel"], row["regime"])


def test_a_shrunk_list_orphans_its_row(monkeypatch):
    """Without its C = 3, 7 and 33 the texture file's list no longer enters the scalar sweep with a carry."""
    row = next(r for r in lr.TABLE if r["op"] == "texture" and r["kernel"] == "k_texture<scalar>" and r["regime"] == "sweep, " + lr.REGIMES[0])
    assert row["enters"]()
    real = lr.old_list
    monkeypatch.setattr(lr, "old_list", lambda path, name: tuple(C for C in real(path, name) if 256 % C == 0))
    assert not row["enters"]()


def test_the_design_document_prints_this_table():
    with open(os.path.join(lr.ROOT, "DESIGN.md")) as f:
        doc = f.read()
    assert "Launch regimes and who tests them" in doc
    for line in lr.markdown().splitlines():
        assert line in doc, line
