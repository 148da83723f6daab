"""The hand-built read-stage edge panels (tests/readcases.py) through the engine by every route the product has.  For each route: records,
their order, stderr and the annotated site lists equal to the reference's recorded answers (tests/golden/read_edges.json) AND to the oracle's in
this process, and no UnfazedHipError (the kernel's guards -- error codes 1 to 4: a base, a unit or a quality bit that the host did not stage was
asked for -- fail the call loudly).  Bit-exact equality throughout."""
import copy

import pytest

from test_read_edges import RUN_IDS, assert_same_as_golden, assert_same_runs, oracle_run, panel, panel_tables, run_panel

pytestmark = pytest.mark.gpu


def check(name, run, got):
    assert_same_as_golden(name, run, got)
    assert_same_runs(got, oracle_run(name, run))


@pytest.fixture
def point_only(monkeypatch):
    """every table forced into the form a point-variant region table travels in (two-bit bases, qualities as counts + position lists, `end`
    derived, compact CIGAR), as test_link_form_of_a_point_variant_table_matches_oracle does"""
    from unfazed_amd.engine import HipEngine
    real = HipEngine.upload_reads

    def forced(self, reads, min_base_qual=None, point_only=False, **kw):
        return real(self, reads, min_base_qual=min_base_qual, point_only=True)

    monkeypatch.setattr(HipEngine, "upload_reads", forced)


@pytest.mark.parametrize("name,run", RUN_IDS)
def test_whole_tables_uploaded(engine, name, run):
    """route (a): run_host(engine, ...) on the tables as they are"""
    check(name, run, run_panel(engine, name, run))


@pytest.mark.parametrize("name,run", RUN_IDS)
def test_point_variant_link_form_forced(engine, point_only, name, run):
    """route (b)"""
    check(name, run, run_panel(engine, name, run))


@pytest.mark.parametrize("name,run", RUN_IDS)
def test_every_dnm_through_the_hbm_build(engine, monkeypatch, name, run):
    """route (c): UZ_TEST_PHASE_ARENA=0, no DNM fits the workgroup's LDS arena and k_phase<false> redoes every one in HBM scratch"""
    from unfazed_amd.engine import K_PHASE
    monkeypatch.setenv("UZ_TEST_PHASE_ARENA", "0")
    engine.prof_enable(True)
    try:
        got = run_panel(engine, name, run)
        redone = engine.prof_units(K_PHASE)
    finally:
        engine.prof_enable(False)
    check(name, run, got)
    assert redone == len(panel(name).cases)  # (every case has candidates and reads: all of them reach the read stage)


def test_the_128_site_ladder_is_redone_and_the_127_site_one_is_not(engine):
    """At the default arena size the arena build holds het indices in eight bits (phase_body.hpp `if (LDS && nh > 127) return 1`): the DNM with 128
    het sites is given up by both arena launches and redone by the HBM build, the one with 127 is not (its working arrays fit the arena of the
    second launch) -- engine.prof_units(K_PHASE) counts the DNMs of the last batch that took the HBM build.  Each ladder is run as a batch of its
    own, and both must give the records of the whole panel's run."""
    from helpers import run_host
    from unfazed_amd.engine import K_PHASE
    pn = panel("point")
    sites, reads = panel_tables("point")
    want = oracle_run("point", "default")[0]
    redone = {}
    engine.prof_enable(True)
    try:
        for c in pn.cases:
            if not hasattr(c, "n_het"):
                continue
            ds = copy.copy(pn.dataset)
            ds.dnms = [d for d in pn.dataset.dnms if d["start"] == c.pos]
            recs, dn, err = run_host(engine, ds, sites, reads)
            redone[c.n_het] = engine.prof_units(K_PHASE)
            assert len(dn[0]["het_sites"]) == c.n_het and list(recs) == [c.key]
            assert sorted(recs[c.key]["dad_reads"]) == sorted(want[c.key]["dad_reads"]) and recs[c.key]["mom_reads"] == want[c.key]["mom_reads"]
            assert sorted(recs[c.key]["dad_sites"]) == sorted(want[c.key]["dad_sites"])
    finally:
        engine.prof_enable(False)
    print("DNMs that took the HBM build, by het sites:", redone)
    assert redone == {127: 0, 128: 1}


@pytest.mark.parametrize("walk", ["device", "host"])
@pytest.mark.parametrize("name", ["point", "sv"])
def test_from_indexed_files(engine, tmp_path, monkeypatch, name, walk):
    """route (d): the panel written as files (filesio.dump_dataset + a BAI), phase_snvs / phase_svs through the session.  UZ_WALK=device: blocks
    inflated, walked and joined on the device, the table unpacked in HBM; UZ_WALK=host: the staged link form (unit masks, listed bases, quality
    bits with listed bases) built by the host's walk."""
    from filesio import dump_dataset, write_bai
    monkeypatch.setenv("UZ_WALK", walk)
    paths = dump_dataset(panel(name).dataset, str(tmp_path))
    for b in paths["bams"].values():
        write_bai(b)
    for run in panel(name).runs:
        check(name, run, run_panel(engine, name, run, bams=paths["bams"], sites_name=paths["sites"]))
