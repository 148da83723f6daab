"""UZ_CUTOFF_ROUTE=device through the product calls: a cohort of four kids from files (one BAM + BAI per kid, a BGZF multi-sample sites VCF + TBI),
phase_snvs and phase_svs, with insert_size_max_sample below, near and at the files' record counts.  The records and the kids' insert cutoffs must
be those of UZ_CUTOFF_ROUTE=host (the route of every other test: read_collector.py:11-25 on the head the source read when it was opened), the
heads of the four files are walked once for both calls, and with the switch unset nothing of the device route runs.  A parity test, not a truth
test."""
import contextlib
import io
import os

import numpy as np
import pytest

from helpers import norm_records
from synth.small import SmallConfig, make_small

pytestmark = pytest.mark.gpu

KIDS = ["kidA", "kidB", "kidC", "kidD"]


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    import gzip
    from filesio import dump_dataset, write_bai, write_bgzf_text, write_tbi
    ds = make_small(SmallConfig(seed=515, n_dnms=24, kids=KIDS, cluster_prob=0.5))
    paths = dump_dataset(ds, str(tmp_path_factory.mktemp("cutoff_route")))
    for b in paths["bams"].values():
        write_bai(b)
    text = gzip.open(paths["sites"], "rt").read()
    write_bgzf_text(paths["sites"], text)
    write_tbi(paths["sites"])
    return ds, paths


def _call(which, ds, paths, cap, fresh):
    """one product call -> (records, {kid: cutoff}, summed route counters); fresh: the session's tables, hosts and sources are dropped first"""
    from unfazed_amd import hostpath, session
    from unfazed_amd.snv_phaser import phase_snvs
    from unfazed_amd.sv_phaser import phase_svs
    if fresh:
        session._READS.clear()
        session._HOSTS.clear()
        session._STAGERS.clear()
        hostpath._CUTOFF_RANKS.clear()
        for k in [k for k in session._SITES if "@" in k]:
            del session._SITES[k]
    sv = which == "sv"
    dnms = [dict(chrom=d["chrom"], start=d["start"], end=d["start"] + 300 if sv else d["end"], kid=d["kid"], vartype="DEL" if sv else "POINT",
                 bam=paths["bams"][d["kid"]], cram_ref=None) for d in ds.dnms]
    with contextlib.redirect_stderr(io.StringIO()):
        if sv:
            recs = phase_svs(dnms, list(KIDS), ds.pedigrees, paths["sites"], 2, "38", False, 10 ** 9, False, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8], 20, 10, 5000,
                             cap, 3, 1, 151, 5)
        else:
            recs = phase_snvs(dnms, list(KIDS), ds.pedigrees, paths["sites"], 2, "38", False, 10 ** 9, False, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8], 20, 10, 5000,
                              cap, 3, 1, 151, 5)
    hosts = list(session._HOSTS.values())
    cut, stats = {}, {}
    for h in hosts:
        cut.update(h.cutoffs)
        for k in ("cutoff_device_files", "cutoff_host_files", "cutoff_walk_calls"):
            stats[k] = stats.get(k, 0) + h.stats[k]
    return norm_records(recs), cut, stats


def _bits(cut):
    return {k: (type(v), np.float64(v).tobytes()) for k, v in cut.items()}


def test_four_kids_by_both_routes(cohort, hip_lib, monkeypatch):
    from unfazed_amd.io_native import BamSource
    ds, paths = cohort
    n_records = max(BamSource(b, insert_size_max_sample=10 ** 7).tlen_head.size for b in paths["bams"].values())
    assert n_records > 250
    monkeypatch.setenv("UZ_HOST_CHUNKS", "0")
    for cap in (50, 199, n_records):
        want = {}
        monkeypatch.setenv("UZ_CUTOFF_ROUTE", "host")
        for which in ("snv", "sv"):
            want[which] = _call(which, ds, paths, cap, fresh=True)
            assert want[which][2] == dict(cutoff_device_files=0, cutoff_host_files=0, cutoff_walk_calls=0)
        assert len(want["snv"][0]) >= 4 and set(want["snv"][1]) == set(KIDS)  # a condition on the inputs: an empty result cannot pass
        monkeypatch.setenv("UZ_CUTOFF_ROUTE", "device")
        got_snv = _call("snv", ds, paths, cap, fresh=True)
        assert got_snv[2]["cutoff_device_files"] == 4 and got_snv[2]["cutoff_host_files"] == 0 and got_snv[2]["cutoff_walk_calls"] >= 1
        got_sv = _call("sv", ds, paths, cap, fresh=False)  # phase_svs behind phase_snvs: the same files make no further walk
        assert got_sv[2] == got_snv[2]
        for which, got in (("snv", got_snv), ("sv", got_sv)):
            assert _bits(got[1]) == _bits(want[which][1]), (cap, which)
            for kid in KIDS:
                assert {k: r for k, r in got[0].items() if r["kid"] == kid} == {k: r for k, r in want[which][0].items() if r["kid"] == kid}, (cap, which, kid)
        # a fresh host on the same files: the ranks are the process's, no walk is made
        from unfazed_amd import session
        session._HOSTS.clear()
        again = _call("sv", ds, paths, cap, fresh=False)
        assert again[2]["cutoff_walk_calls"] == 0 and again[2]["cutoff_device_files"] == 0 and _bits(again[1]) == _bits(want["sv"][1]) and again[0] == want["sv"][0]


def test_with_the_switch_unset_the_counters_stay_zero(cohort, hip_lib, monkeypatch):
    ds, paths = cohort
    monkeypatch.delenv("UZ_CUTOFF_ROUTE", raising=False)
    monkeypatch.setenv("UZ_HOST_CHUNKS", "0")
    recs, cut, stats = _call("snv", ds, paths, 199, fresh=True)
    assert stats == dict(cutoff_device_files=0, cutoff_host_files=0, cutoff_walk_calls=0) and set(cut) == set(KIDS)
    from unfazed_amd import session
    assert all(k[-1] == 199 for k in session._STAGERS if k[0] != "many")  # every source was opened with its head
