"""The read stage's launch sequence (k_reads.hip: uz_launch_phase) after the clears moved into k_phase_bounds and the copies back became one
launch: a context that has run other batches gives a batch the results a FRESH context gives it.  (A context's first batch takes the exact
path, which the goldens and the oracle tests pin; every later one runs speculatively on the sizes of the batch before, with the state of
that batch -- het ranges, work cursors, give-up lists, the reduced sizing record -- still in the buffers.)"""
import os

import numpy as np
import pytest

from helpers import tables
from synth.small import SmallConfig, make_small
from unfazed_amd import abi
from unfazed_amd.engine import K_PHASE, HipEngine
from unfazed_amd.hostpath import concordant_cutoff

pytestmark = pytest.mark.gpu
KEYS = ("status", "counts", "origin", "evidence")
MODE = abi.FIND_SECOND_WINDOW
NO_CAND = 3  # this DNM of both batches names a contig the sites table does not have: no candidate sites


class World:
    def __init__(self):
        self.ds = make_small(SmallConfig(seed=977, n_dnms=30, cluster_prob=0.8))
        self.sites, reads = tables(self.ds)
        self.rt = list(reads.values())[0]
        kid = self.ds.dnms[0]["kid"]
        ped = self.ds.pedigrees[kid]
        self.cols = self.sites.family_columns(kid, ped["dad"], ped["mom"])
        self.P = abi.make_params()
        self.big, self.small = self.view(30), self.view(7)

    def view(self, n):
        sites, rt, dn = self.sites, self.rt, self.ds.dnms[:n]
        refs, alts = [], []
        for d in dn:
            j = int(sites.query(d["chrom"], d["start"], d["start"] + 1)[-1])
            refs.append(sites.ref_str[j].encode())
            alts.append(sites.alt_strs[j][0].encode())
        contig = [sites.contig_index[d["chrom"]] for d in dn]
        contig[NO_CAND] = -1
        return abi.dnms_view(contig, [rt.contig_index[d["chrom"]] for d in dn], [d["start"] for d in dn], [d["end"] for d in dn], [0] * n, refs, alts,
                             concordant_cutoff(rt.tlen, 151, 3))

    def engine(self):
        e = HipEngine(0)
        sid = e.upload_sites(self.sites)
        return e, e.add_family(sid, *self.cols), e.upload_reads(self.rt)


@pytest.fixture(scope="module")
def world():
    """the two batches and what a fresh engine gives for each (with the DNMs its HBM build redid)"""
    w = World()
    w.want, w.sizes, w.n_het = {}, {}, {}
    for name, dv in (("big", w.big), ("small", w.small)):
        e, fid, rid = w.engine()
        w.n_het[name] = int(e.find(fid, dv, w.P, MODE)[3][-1])  # (the sizing fetch fills pre_ha / pre_hl with that many entries)
        e.drop_derived()  # the read stage below classifies the sites and finds its windows itself, as on an engine that has done nothing
        r = e.phase_raw(fid, rid, dv, w.P, MODE)
        w.want[name] = (r, e.prof_units(K_PHASE))
        w.sizes[name] = e.phase_sizing(dv.view.n, w.n_het[name])  # the batch's own sizes: the sizing pass's reduced record
        e.close()
    assert w.want["small"][0]["status"][NO_CAND] == abi.ST_NO_CAND and (w.want["small"][0]["status"] == abi.ST_OK).any()
    assert (w.want["big"][0]["status"] == abi.ST_OK).sum() > (w.want["small"][0]["status"] == abi.ST_OK).sum()
    return w


def _same(want, got, what):
    for k in KEYS:
        assert np.array_equal(want[k], got[k]), "%s: %s differs" % (what, k)


def test_smaller_batch_behind_a_larger_one(world):
    w = world
    e, fid, rid = w.engine()
    try:
        _same(w.want["big"][0], e.phase_raw(fid, rid, w.big, w.P, MODE), "first batch")
        _same(w.want["small"][0], e.phase_raw(fid, rid, w.small, w.P, MODE), "its first 7 DNMs behind it")
        _same(w.want["big"][0], e.phase_raw(fid, rid, w.big, w.P, MODE), "the 30 again")
    finally:
        e.close()


def test_hbm_build_then_not(world):
    w = world
    e, fid, rid = w.engine()
    try:
        os.environ["UZ_TEST_PHASE_ARENA"] = "0"  # no DNM fits an arena of no bytes: everything through the HBM build
        try:
            _same(w.want["big"][0], e.phase_raw(fid, rid, w.big, w.P, MODE), "every DNM through the HBM build")
            assert e.prof_units(K_PHASE) > 0
        finally:
            os.environ.pop("UZ_TEST_PHASE_ARENA", None)
        _same(w.want["big"][0], e.phase_raw(fid, rid, w.big, w.P, MODE), "the same batch without the hook")
        assert e.prof_units(K_PHASE) == w.want["big"][1]
    finally:
        e.close()


def test_batch_that_outgrows_the_speculative_sizes(world):
    """The premise is held first: a batch is run on the maxima of the batch before plus an eighth plus 8 (uz_launch_phase: `room`), so the 30
    outgrow what the 7 leave when one of their maxima lies beyond that -- and the engine's own sizing record of each run must be the batch's."""
    w = world
    small, big = w.sizes["small"], w.sizes["big"]
    beyond = [k for k in ("mA", "mT", "mH", "mC") if big[k] > small[k] + small[k] // 8 + 8]
    assert beyond, "the 30 DNMs fit the speculative sizes the 7 leave: %s against %s" % ({k: big[k] for k in ("mA", "mT", "mH", "mC")}, {k: small[k] for k in ("mA", "mT", "mH", "mC")})
    e, fid, rid = w.engine()
    try:
        _same(w.want["small"][0], e.phase_raw(fid, rid, w.small, w.P, MODE), "the 7 first")
        e.phase_begin(fid, rid, w.big, w.P, MODE)
        _same(w.want["big"][0], e.phase_end(fid, rid, w.big, w.P, MODE), "the 30 behind them, begin / end")
        got = e.phase_sizing(30, w.n_het["big"])
        assert all(got[k] == big[k] for k in ("mA", "mT", "mH", "mC", "active", "mM", "sumP")) and np.array_equal(got["hist"], big["hist"])
        e.phase_begin(fid, rid, w.small, w.P, MODE)
        _same(w.want["small"][0], e.phase_end(fid, rid, w.small, w.P, MODE), "the 7 again, begin / end")
    finally:
        e.close()


def test_begin_and_end_with_a_find_in_between(world):
    w = world
    e, fid, rid = w.engine()
    try:
        e.phase_raw(fid, rid, w.small, w.P, MODE)  # (a first batch would run to its end inside phase_begin)
        e.phase_begin(fid, rid, w.big, w.P, MODE)
        found = e.find(fid, w.small, w.P, MODE, transient=True)
        stats = e.find_stats()
        got = e.phase_end(fid, rid, w.big, w.P, MODE)
        assert e.find_stats() == stats and stats[0] >= 1 and stats[1] >= 5  # (the read stage's copies are not the find's)
        _same(w.want["big"][0], got, "begin, a find of another batch, end")
        plain = e.find(fid, w.small, w.P, MODE)
        for a, b in zip(plain, found):
            assert np.array_equal(a, b)
    finally:
        e.close()
