"""uz_phase_cnv_cohort: the DEL / DUP of several kids in one whole-region find and one K6 launch give what one uz_phase_cnv per kid gives --
counts, decisions and the site lists, which uz_phase_cnv_sites now takes from the dense array k_cnv_dense leaves -- and what the CPU oracle
gives, with and without read-backed counts to merge."""
import numpy as np
import pytest

import cohortcases as cc
from oracle import oracle as orc
from unfazed_amd import abi

pytestmark = pytest.mark.gpu

E_STATE = -4
KEYS = ("cnv_counts", "origin", "evidence", "etype")
# read-backed rows (dad_reads, mom_reads, dad_sites, mom_sites), one per event of cohortcases.cnv_batch.  Event 1 (every vote dad's) with
# reads for dad: READBACKED + ALLELE-BALANCE.  Event 2 (every vote mom's) with reads for dad, event 6 (dad's) with reads for mom: read-backed
# evidence for one parent against allele balance for the other, the input summarize_record's AMBIGUOUS_BOTH branch is written for -- its
# branch order never takes it (k_cnv_count keeps it as written), so the calls stay READBACKED + ALLELE-BALANCE for the allele-balance parent.
# Event 0 (137 : 136) and event 3 with reads for both: the ambiguous merges.
RB = np.array([[3, 3, 2, 2], [12, 1, 4, 1], [9, 0, 3, 0], [2, 5, 1, 2], [0, 0, 0, 0], [4, 0, 2, 0], [0, 7, 0, 3], [1, 1, 1, 1], [0, 0, 0, 0]], np.int32)


@pytest.fixture(scope="module")
def P():
    return abi.make_params(search_dist=cc.SEARCH_DIST)  # (the stage runs its find at search_dist 0 whatever this says)


@pytest.fixture(scope="module")
def per_kid(engine, P):
    """rb is None / RB -> per group: phase_cnv's dict (lists from uz_phase_cnv_sites) on families of their own; computed once"""
    rows, groups = cc.cnv_batch()
    sid = engine.upload_sites(cc.table())
    fams = cc.make_families(engine, sid)
    out = {}
    for name, rb in (("none", None), ("rb", RB)):
        out[name] = [engine.phase_cnv(fams[t], cc.view(rows[f: f + n]), P, rb_counts=None if rb is None else rb[f: f + n]) for t, f, n in groups]
    engine.free_sites(sid)
    return out


def _check(got, parts, groups, what):
    for (t, f, n), r in zip(groups, parts):
        for k in KEYS:
            assert np.array_equal(got[k][f: f + n], r[k]), (what, t, k)
        for d in range(n):
            for j in range(2):
                assert np.array_equal(got["lists"][f + d][j], r["lists"][d][j]), (what, t, d, j)


@pytest.mark.parametrize("name", ("none", "rb"))
def test_cohort_stage_equals_per_kid_stages(engine, per_kid, P, name):
    rows, groups = cc.cnv_batch()
    rb = None if name == "none" else RB
    sid = engine.upload_sites(cc.table())
    fams = cc.make_families(engine, sid)  # not scanned
    got = engine.phase_cnv_cohort([(fams[t], f, n) for t, f, n in groups], cc.view(rows), P, rb_counts=rb)
    _check(got, per_kid[name], groups, name)
    # the offsets of uz_phase_cnv_sites are the counts' running sums, and pos == NULL gives them alone
    n = len(rows)
    off = np.full(2 * n + 1, -1, np.int64)
    assert engine.L.uz_phase_cnv_sites(engine.h, off.ctypes.data, None) == 0
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(got["cnv_counts"].reshape(-1))]))
    pos = np.zeros(int(off[-1]), np.int32)
    assert engine.L.uz_phase_cnv_sites(engine.h, off.ctypes.data, pos.ctypes.data) == 0
    assert np.array_equal(pos, np.concatenate([x for pair in got["lists"] for x in pair]))
    engine.free_sites(sid)


def test_the_events_reach_the_paths_they_name(per_kid):
    rows, groups = cc.cnv_batch()
    cnt = np.concatenate([r["cnv_counts"] for r in per_kid["none"]])
    et = np.concatenate([r["etype"] for r in per_kid["rb"]])
    org = np.concatenate([r["origin"] for r in per_kid["rb"]])
    assert len(rows) == 9 and {r[4] for r in rows} == {abi.VT_DEL, abi.VT_DUP, abi.VT_OTHER_SV}
    assert cnt[0].sum() > 130 and cnt[0].min() > 0  # three ballot rounds and more, both parents
    assert cnt[1, 0] > 64 and cnt[1, 1] == 0 and cnt[2, 0] == 0 and cnt[2, 1] > 64  # every vote dad's / mom's
    assert cnt[4].sum() == 0 and cnt[5].sum() == 0 and cnt[6].sum() > 0  # no candidate; not a CNV
    assert et[1] == abi.ET_READBACKED | abi.ET_ALLELE_BALANCE and org[1] == abi.OR_DAD
    assert et[2] & abi.ET_ALLELE_BALANCE and org[2] == abi.OR_MOM and org[6] == abi.OR_DAD  # allele balance against the reads' parent
    assert (et & abi.ET_AMBIG_FLAG).any() and et[4] == 0


@pytest.mark.parametrize("name", ("none", "rb"))
def test_per_kid_stages_equal_the_oracle(per_kid, P, name):
    rows, groups = cc.cnv_batch()
    rb = None if name == "none" else RB
    sites_h = abi.sites_view(cc.table())
    for (t, f, n), r in zip(groups, per_kid[name]):
        w = orc.phase_cnv(P, sites_h, cc.family_held(cc.TRIOS[t]), cc.view(rows[f: f + n]), None if rb is None else rb[f: f + n])
        for k in KEYS:
            assert np.array_equal(r[k], w[k]), (name, t, k)
        for d in range(n):
            for j in range(2):
                assert np.array_equal(r["lists"][d][j], w["lists"][d][j]), (name, t, d, j)


def test_sites_before_any_stage_is_a_state_error(hip_lib):
    from unfazed_amd.engine import HipEngine
    e = HipEngine(0)
    try:
        off = np.zeros(3, np.int64)
        assert e.L.uz_phase_cnv_sites(e.h, off.ctypes.data, None) == E_STATE
    finally:
        e.close()
