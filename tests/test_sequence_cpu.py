"""The scene sequence of tests/sequence.py keeps the properties the training-loop GPU tests rely on (CPU oracle's binning)."""
import sequence as seq


def test_sequence_conditions():
    got = {k: seq.binning(k) for k in seq.ORDER}
    R = {k: v[0] for k, v in got.items()}
    print({k: v[:2] for k, v in got.items()})
    # one shape: the same key of the binning-buffer hint, and stale scratch that holds ids of a scene with the same P and F
    assert len({v[2] for v in got.values()}) == 1 and len({v[3] for v in got.values()}) == 1
    assert got["S0"][3] == seq.F
    assert R["S0"] > 0 and abs(R["S1"] - R["S0"]) <= 0.1 * R["S0"], "S1 must be about the size of S0 (it is to fit S0's buffer)"
    assert R["S2"] >= 3 * R["S1"], "S2 must outgrow the buffer S1 left behind"
    assert abs(R["S3"] - R["S2"]) <= 0.1 * R["S2"], "S3 must be about the size of S2 (it is to fit S2's buffer)"
    assert R["S4"] > 0 and R["S4"] <= R["S3"] / 4, "S4 must be small enough for the hint to shrink"
    assert R["S5"] == 0 and got["S5"][1] == 0, "S5 must render nothing"
    assert got["S6"] == got["S0"]
    # every non-empty step has lists longer than one entry (the per-tile sort and the composite have work to do)
    assert all(got[k][1] > 1 for k in seq.ORDER if k != "S5")


def test_far_step_differs_from_its_twin_only_in_depth():
    a, b = seq.scene("S1"), seq.scene("S5")
    assert (a.verts[:, :2] == b.verts[:, :2]).all() and (a.verts[:, 2] - b.verts[:, 2] == seq.FAR_SHIFT).all()
    assert (a.faces == b.faces).all()
