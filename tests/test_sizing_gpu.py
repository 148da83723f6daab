"""The sizing pass on the device (k_phase_bounds: 16-lane group search over the coarse and mid levels, 64 mid entries staged in LDS per
group, uz_mid8_refine, the far hand-off to uz_lower_bounds_c) and the reduction of its bounds (k_bounds_reduce), read back through
uz_phase_sizing_fetch and held EXACTLY to the numpy model of tests/sizingmodel.py (np.searchsorted; tests/test_sizing_model.py holds that
model to the kernel body's generic form on the CPU) on the hand-built edge tables of tests/sizingcases.py.  The results of the same call
are held to the oracle.

Which shape reaches which branch (tests/test_sizing_model.py asserts it from the tables' indices): contig_sizes -- no mid level up to 128
records, mid level from 129, coarse level from 8193 (one coarse entry) and on 15818 records (three), `whole` near every contig's end;
ties -- runs of equal starts across 8-, 64- and both 4096-record boundaries, the coarse entry inside the run; dense_5000 -- far chains,
`whole`, fewer than 64 staged entries; dense_1500 -- no far chain; a staged count of 0 cannot occur (the stage starts one cell below the
lowest bound's)."""
import numpy as np
import pytest

import sizingcases
import sizingmodel
from oracle import oracle as orc
from test_sizing_model import assert_sizing_equal
from unfazed_amd import abi
from unfazed_amd.engine import UnfazedHipError

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in sizingcases.all_cases()}
RUNS = [(n, "ascii") for n in CASES] + [(n, "staged") for n in sizingcases.BOTH_UPLOADS]


def test_sizing_fetch_before_any_batch_is_a_state_error(hip_lib):
    from unfazed_amd.engine import HipEngine
    e = HipEngine(0)
    try:
        with pytest.raises(UnfazedHipError, match=r"\(-4\)"):
            e.phase_sizing(1, 1)
    finally:
        e.close()


@pytest.mark.parametrize("name,upload", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_sizing_pass_equals_the_model(engine, name, upload):
    case = CASES[name]
    rt, sites, P = case.reads, case.sites, case.params
    cols = sites.family_columns("kid", "dad", "mom")
    sid = engine.upload_sites(sites)
    fid = engine.add_family(sid, *cols)
    rid = engine.upload_reads(rt) if upload == "ascii" else engine.upload_reads(rt, min_base_qual=P.min_gt_qual)
    try:
        # either build of the table ends in the same index build over the same headers
        hd = engine.reads_headers(rid, rt.n_segs)
        assert np.array_equal(hd["start"], rt.start) and np.array_equal(hd["end"], rt.end)
        dv = case.dnms_view()
        found = engine.find(fid, dv, P, abi.FIND_SECOND_WINDOW)
        co, ci, cf, ho, hi = found
        got_r = engine.phase_raw(fid, rid, dv, P, abi.FIND_SECOND_WINDOW)
        got = engine.phase_sizing(case.n, int(ho[case.n]))
        want = case.model(found)
        assert_sizing_equal(want, got, ho, "%s (%s upload)" % (name, upload))
        red = sizingmodel.reduce_bounds(want["bounds"])
        for k in ("mA", "mT", "mH", "mC", "active", "mM", "sumP"):
            assert got[k] == red[k], (name, k, got[k], red[k])
        assert np.array_equal(got["hist"], red["hist"]), (name, np.nonzero(got["hist"] != red["hist"])[0].tolist())
        # every site of a window is a candidate and a het site: the lists the model took are the oracle's
        sv, fv, rv = abi.sites_view(sites), abi.family_view(*cols), abi.reads_view(rt)
        ofound = orc.find(P, sv, fv, dv, abi.FIND_SECOND_WINDOW)
        for a, b in zip(found, ofound):
            assert np.array_equal(a, b)
        want_r = orc.phase(P, sv, rv, dv, ofound, keep_lists=False)
        for k in ("status", "counts", "origin", "evidence"):
            assert np.array_equal(want_r[k], got_r[k]), (name, k)
    finally:
        engine.free_reads(rid)
        engine.free_sites(sid)
