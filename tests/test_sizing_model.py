"""The numpy model of the sizing pass (tests/sizingmodel.py: searchsorted and nothing else) against the kernel body's generic form
(uz_phase_bounds over uz_lower_bounds_c -- uz_lb_level on the three index levels, uz_mid8_refine -- compiled for the CPU, tests/emu) on the
hand-built edge tables of tests/sizingcases.py.  The device's staged form is held to the same model by tests/test_sizing_gpu.py; this test
must pass before that one is trusted."""
import numpy as np
import pytest

import sizingcases
import sizingmodel
from emu import emu
from oracle import oracle as orc
from unfazed_amd import abi


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in sizingcases.all_cases()}


def _found(case):
    sv = abi.sites_view(case.sites)
    fv = abi.family_view(*case.sites.family_columns("kid", "dad", "mom"))
    return sv, orc.find(case.params, sv, fv, case.dnms_view(), abi.FIND_SECOND_WINDOW)


def assert_sizing_equal(want, got, het_off, what):
    """every array exactly; the first DNM (and het site) that differs is printed"""
    for k in ("bounds", "pre_win"):
        if not np.array_equal(want[k], got[k]):
            d = int(np.nonzero((want[k] != got[k]).any(axis=1))[0][0])
            raise AssertionError("%s: %s differs first at DNM %d: want %s got %s" % (what, k, d, want[k][d].tolist(), got[k][d].tolist()))
    for k in ("pre_ha", "pre_hl"):
        if not np.array_equal(want[k], got[k]):
            h = int(np.nonzero(want[k] != got[k])[0][0])
            d = int(np.searchsorted(het_off, h, "right")) - 1
            raise AssertionError("%s: %s differs first at het site %d (DNM %d, its site %d): want %d got %d" %
                                 (what, k, h, d, h - int(het_off[d]), int(want[k][h]), int(got[k][h])))


@pytest.mark.parametrize("name", [c.name for c in sizingcases.all_cases()])
def test_model_matches_the_generic_kernel_body(cases, name):
    case = cases[name]
    sv, found = _found(case)
    want = case.model(found)
    got = emu.phase_sizing(case.params, sv, abi.reads_view(case.reads), case.dnms_view(), found)
    assert_sizing_equal(want, got, found[3], name)
    assert int(found[0][case.n]) > 0  # the batch has candidates at all


def test_the_cases_reach_the_branches_they_are_named_for(cases):
    """Which named shape reaches which branch of k_phase_bounds, from the tables' indices (sizingmodel.branch_stats)."""
    st = {}
    for name in ("contig_sizes", "ties", "dense_5000", "dense_1500", "lanes_255"):
        sv, found = _found(cases[name])
        st[name] = cases[name].branches(found)
    cs = st["contig_sizes"]
    recs = {b["records"] for b in cs}
    assert set(sizingcases.CONTIG_RECORDS) <= recs
    assert any(not b["shared"] and b["records"] == 128 for b in cs) and any(b["shared"] and b["records"] == 129 for b in cs)  # mid level: above 128
    assert any(b["shared"] and not b["coarse"] and b["records"] == 8192 for b in cs) and any(b["coarse"] and b["records"] == 8193 for b in cs)
    assert any(b["coarse"] and b["records"] == 15818 for b in cs)
    assert any(b["shared"] and b["whole"] for b in cs) and any(b["shared"] and b["whole"] is False for b in cs)
    # the staged count: 64 in the middle of a contig, fewer near its end; never 0 -- the stage starts one cell below the lowest bound's, and a
    # contig with the mid level (more than 128 records) has a mid entry at or below every record but those of its first cell
    staged = sorted({b["staged"] for v in st.values() for b in v if b["staged"] is not None})
    assert staged[0] >= 1 and staged[0] <= 2 and staged[-1] == 64 and len(staged) > 4
    assert sum(b["far"] for b in st["dense_5000"]) > 100 and any(b["whole"] and b["staged"] < 64 for b in st["dense_5000"])
    assert sum(b["far"] for b in st["dense_1500"]) == 0 and any(b["whole"] is False for b in st["dense_1500"])
    assert any(b["coarse"] for b in st["ties"])  # (the 4100-run covers the contig's only coarse entry and both 4096-record boundaries)
    assert sum(b["far"] for b in st["lanes_255"]) == 0


def test_reduction_of_the_model_fills_distinct_bins(cases):
    """the big batch: a second round of the reduction's grid stride, at least three bins of the histogram"""
    case = cases["reduce_big"]
    assert case.n == 48 * 256 + 1
    sv, found = _found(case)
    red = sizingmodel.reduce_bounds(case.model(found)["bounds"])
    assert int((red["hist"] > 0).sum()) >= 3 and red["active"] == int(red["hist"].sum()) and 0 < red["active"] < case.n
    # by hand on three DNMs: b = [b0, b1, nh, nc, b4]
    small = sizingmodel.reduce_bounds(np.array([[2, 10, 3, 3, 1], [0, 0, 4, 0, 0], [100, 4000, 9, 7, 2]]))
    assert (small["mA"], small["mT"], small["mH"], small["mC"], small["active"]) == (100, 4000, 9, 7, 2)
    assert small["mM"] == 4000 + 4 * 100 * 3 and small["sumP"] == (10 + 16 + 3) + 0 + (4096 + 7)
    assert small["hist"][(92 + 20 + 3583) >> 8] == 1 and small["hist"][(37000 + 1000 + 3583) >> 8] == 1 and small["hist"].sum() == 2
