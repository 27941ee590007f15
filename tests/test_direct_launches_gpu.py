"""
The launches of the nested-dissection solve (csrc/direct.hip: the launch list a handle builds at create, and the solve, the launch
count, the index accounting and the launch profile that walk it) on the smallest planes that reach every kind of launch
(tests/direct_launch_cases.py), for k = 1 .. 4 right-hand sides:

    record     x is, bit for bit, what the commit BEFORE the launch list computed, and info()'s shape and launch_profile()'s
               (lo, hi, sweep) rows are that commit's (tests/golden/direct_launch_bits.npz, recorded with that commit's library by
               tools/record_direct_launch_bits.py); a solve under "profile" = 3 has the bits of the unprofiled one
    sharded    the same for two ranks' handles in one process: part 0, the summed exchange (recorded too), part 1, x stitched by row
               ownership -- through a caller's exchange buffer and through the handles' own regions
    reports    the three reports agree with each other: as many profiled launches as info() counts, the up sweep first and levels
               descending, the down sweep after it and ascending, the tier first and last, the launches' words summing to the sweeps'
"""
import os

import numpy as np
import pytest
import torch

import direct_launch_cases as dc

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from largesteps import _native
    _native.lib()          # fail loudly if the extension is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def record():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", dc.GOLDEN))


@pytest.fixture(scope="module")
def runs(dev):
    """every case's run, computed once: unsharded by case, sharded by (case, exchange). The environment is the case's while its
    handles are constructed and the caller's again afterwards."""
    done = {}

    def get(case, exchange=None):
        key = (case, exchange)
        if key not in done:
            with pytest.MonkeyPatch.context() as mp:
                dc.set_env(case, mp.setenv, lambda name: mp.delenv(name, raising=False))
                M, B = dc.system(case, dev)
                done[key] = dc.run_sharded(case, M, B, exchange) if exchange else dc.run_unsharded(case, M, B)
        return done[key]
    return get


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@gpu
@pytest.mark.parametrize("case", list(dc.CASES))
def test_bits_and_launches_are_the_parent_commits(runs, record, case):
    r = runs(case)
    shape, rows = dc.shape_of(r["inf"]), dc.profile_rows(r["prof"])
    print(case, "shape", shape, "recorded", record[case + "/shape"].tolist())
    print(case, "profile", rows.tolist(), "recorded", record[case + "/profile"].tolist())
    if case in dc.TIERED:
        assert r["inf"]["tier_levels"] >= 1, "the library ran no tier: the case does not reach the tier's launches"
    assert shape == record[case + "/shape"].tolist(), "info()'s (launches, tier levels, tier workgroups, levels) is not the recorded one"
    assert rows.tolist() == record[case + "/profile"].tolist(), "launch_profile()'s (lo, hi, sweep) rows are not the recorded ones"
    for k in dc.KS:
        got, want = dc.digest(r["x"][k]), record[f"{case}/k{k}"]
        print(case, "k", k, "sha256", got.tobytes().hex()[:16], "recorded", want.tobytes().hex()[:16])
        assert np.array_equal(got, want), f"k = {k}: x differs from the record in at least one bit"
        assert _same_bits(r["x"][k], r["x_profiled"][k]), f"k = {k}: the profiled solve's x differs from the unprofiled one's"


@gpu
@pytest.mark.parametrize("exchange", dc.EXCHANGE)
@pytest.mark.parametrize("case", list(dc.SHARDED))
def test_sharded_bits_and_launches_are_the_parent_commits(runs, record, case, exchange):
    r = runs(case, exchange)
    key = f"{case}/{exchange}"
    print(key, "shape", r["shape"], "recorded", record[key + "/shape"].tolist(), "cut", r["cut"], "recorded", record[key + "/cut"].tolist())
    assert r["owned_once"], "ownership does not partition the rows"
    assert min(r["cut"]) >= 1, "the cut level is 0: part 1 would hold no up-sweep launch of a level"
    if case in dc.TIERED:
        assert all(s[1] >= 1 for s in r["shape"]), "the library ran no tier: the case does not reach the tier's launches"
    assert r["shape"] == record[key + "/shape"].tolist()
    assert r["cut"] == record[key + "/cut"].tolist()
    for rank, rows in enumerate(r["profile"]):
        print(key, "rank", rank, "part 1 profile", rows.tolist(), "recorded", record[f"{key}/profile{rank}"].tolist())
        assert rows.tolist() == record[f"{key}/profile{rank}"].tolist(), "part 1's (lo, hi, sweep) rows are not the recorded ones"
        assert 0 < len(rows) < r["shape"][rank][0], "both parts hold launches"
    for k in dc.KS:
        got, want = dc.digest(r["x"][k]), record[f"{key}/k{k}"]
        print(key, "k", k, "sha256", got.tobytes().hex()[:16], "recorded", want.tobytes().hex()[:16])
        assert np.array_equal(dc.digest(r["exch"][k]), record[f"{key}/exchange{k}"]), f"k = {k}: the summed exchange differs from the record"
        assert np.array_equal(got, want), f"k = {k}: the stitched x differs from the record in at least one bit"
        assert _same_bits(r["x"][k], r["x_profiled"][k]), f"k = {k}: the profiled solve's x differs from the unprofiled one's"


@gpu
@pytest.mark.parametrize("case", list(dc.CASES))
def test_the_three_reports_agree(runs, case):
    """launch count, launch profile and factor words of one handle (holds at the commit before the launch list too)"""
    r = runs(case)
    inf, prof = r["inf"], r["prof"]
    rows = dc.profile_rows(prof)
    print(case, "launches", inf["launches"], "profile", rows.tolist(), "words", [p["words"] for p in prof], inf["words_up"], inf["words_down"])
    assert len(prof) == inf["launches"]
    up, down = rows[rows[:, 2] == 0], rows[rows[:, 2] == 1]
    assert len(up) and len(down) and np.array_equal(rows, np.concatenate([up, down])), "the up sweep's launches come first"
    assert (np.diff(up[:, 0]) < 0).all() and (np.diff(up[:, 1]) < 0).all(), "up sweep: levels descend"
    assert (np.diff(down[:, 0]) > 0).all() and (np.diff(down[:, 1]) > 0).all(), "down sweep: levels ascend"
    levels, tier = inf["levels"], inf["tier_levels"]
    if tier:
        assert up[0].tolist() == [levels - tier, levels - 1, 0] and down[-1].tolist() == [levels - tier, levels - 1, 1]
    level_rows = rows[(rows[:, 0] < levels - tier)]
    assert (level_rows[:, 0] == level_rows[:, 1]).all(), "a launch above the tier runs one level"
    assert sum(p["words"] for p in prof) == inf["words_up"] + inf["words_down"]
