"""A cohort from files through the product call: 50 kids (some of them siblings: they share another kid's parents), one BAM + BAI per
kid, one BGZF multi-sample sites VCF + TBI, ONE phase_snvs call.  The trios' genotype columns are then made on the device from one sample
table (hostpath.PhasingHost.prepare_families); the records must be those of the CPU oracle backend run through the same host code (which
keeps the per-trio host route) and those of UZ_FAMILY_ROUTE=host.  A parity test, not a truth test."""
import contextlib
import io
import os

import pytest

from helpers import norm_records
from synth.small import SmallConfig, make_small

pytestmark = pytest.mark.gpu

KIDS = ["kid%02d" % i for i in range(50)]


def _indexed_files(ds, tmp_path):
    """the dataset as files, with a BAI next to every BAM and a TBI next to the BGZF sites VCF (as tests/test_host_chunks_gpu.py)"""
    import gzip
    from filesio import dump_dataset, write_bai, write_bgzf_text, write_tbi
    paths = dump_dataset(ds, str(tmp_path))
    for b in paths["bams"].values():
        write_bai(b)
    text = gzip.open(paths["sites"], "rt").read()
    write_bgzf_text(paths["sites"], text)
    write_tbi(paths["sites"])
    return paths


def _run(paths, ds, env, kids, backend=None, fresh=True, readlen=151):
    """one product call on the DNMs of `kids` -> (records, sorted stderr lines, DNMs, the call's PhasingHost objects); backend: instead of the
    session's own (HipEngine); fresh=False keeps the session's tables and hosts of the call before"""
    from unfazed_amd import session
    from unfazed_amd.snv_phaser import phase_snvs
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    own = session._BACKEND
    if backend is not None:
        session.set_backend(backend)
    if fresh:
        session._READS.clear()
        session._HOSTS.clear()
        for k in [k for k in session._SITES if "@" in k]:
            del session._SITES[k]
    try:
        dnms = [dict(chrom=d["chrom"], start=d["start"], end=d["end"], kid=d["kid"], vartype="POINT", bam=paths["bams"][d["kid"]], cram_ref=None)
                for d in ds.dnms if d["kid"] in kids]
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            recs = phase_snvs(dnms, list(kids), ds.pedigrees, paths["sites"], 2, "38", False, 10 ** 9, False, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8], 20, 10, 5000,
                              1000000, 3, 1, readlen, 5)
        hosts = list(session._HOSTS.values())
        return norm_records(recs), sorted(err.getvalue().splitlines()), len(dnms), hosts
    finally:
        if backend is not None:
            session.set_backend(own)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _stats(hosts):
    out = {}
    for h in hosts:
        for k, v in getattr(h, "stats", {}).items():
            out[k] = out.get(k, 0) + v
    return out


def test_fifty_kids_from_files_in_one_call(tmp_path, hip_lib):
    from oracle_backend import OracleBackend
    ds = make_small(SmallConfig(seed=2025, n_dnms=300, kids=KIDS, cluster_prob=0.5))
    for i in range(4, 50, 5):  # every fifth kid is a sibling of the kid before it
        prev = ds.pedigrees[KIDS[i - 1]]
        ds.pedigrees[KIDS[i]]["dad"], ds.pedigrees[KIDS[i]]["mom"] = prev["dad"], prev["mom"]
    assert len(ds.samples) == 150 and len(ds.dnms) == 300
    paths = _indexed_files(ds, tmp_path)

    want, err_w, n, hosts_o = _run(paths, ds, {"UZ_HOST_CHUNKS": "0"}, KIDS, backend=OracleBackend())
    # a condition on the inputs, not a measurement: an empty result cannot pass
    assert n == 300 and len(want) >= n // 10, len(want)
    assert len({r["kid"] for r in want.values()}) >= 40
    so = _stats(hosts_o)
    assert so.get("families_from_samples", 0) == 0 and so.get("families_host", 0) >= 40  # the oracle backend keeps the per-trio route

    got, err_g, _, hosts = _run(paths, ds, {"UZ_HOST_CHUNKS": "0"}, KIDS)
    sd = _stats(hosts)
    kids_seen = {d["kid"] for d in ds.dnms}
    assert got == want
    assert err_g == err_w
    for kid in KIDS:  # kid by kid, name lists included
        assert {k: r for k, r in got.items() if r["kid"] == kid} == {k: r for k, r in want.items() if r["kid"] == kid}, kid
    # the device route made every family, in one call, from one table that holds every named sample once
    assert sd["families_from_samples"] == len(kids_seen) and sd["families_from_samples_calls"] == 1 and sd["families_host"] == 0
    named = {s for k in kids_seen for s in (k, ds.pedigrees[k]["dad"], ds.pedigrees[k]["mom"])}
    assert sd["sample_tables"] == 1 and sd["samples_uploaded"] == len(named) < 3 * len(kids_seen)

    host_route, err_h, _, hosts_h = _run(paths, ds, {"UZ_HOST_CHUNKS": "0", "UZ_FAMILY_ROUTE": "host"}, KIDS)
    sh = _stats(hosts_h)
    assert host_route == want and err_h == err_w
    assert sh["families_from_samples"] == 0 and sh["families_from_samples_calls"] == 0 and sh["sample_tables"] == 0 and sh["families_host"] == len(kids_seen)


def test_a_second_call_extends_the_device_tables_without_uploading_a_sample_twice(hip_lib):
    """the same host over two calls (hostpath.PhasingHost.prepare_families): kids whose trios are new make a second sample table of their own
    samples only; a kid whose trio is known makes nothing"""
    import numpy as np
    from helpers import tables
    from unfazed_amd import abi
    from unfazed_amd.engine import HipEngine
    from unfazed_amd.hostpath import PhasingHost
    kids = ["kidA", "kidB", "kidC", "kidD", "kidE"]
    ds = make_small(SmallConfig(seed=77, n_dnms=30, kids=kids, cluster_prob=0.5))
    ds.pedigrees["kidB"]["dad"], ds.pedigrees["kidB"]["mom"] = ds.pedigrees["kidA"]["dad"], ds.pedigrees["kidA"]["mom"]
    sites, reads = tables(ds)
    eng = HipEngine(0)
    try:
        P = abi.make_params()
        host = PhasingHost(eng, sites, reads)
        trio = lambda k: (k, ds.pedigrees[k]["dad"], ds.pedigrees[k]["mom"])  # noqa: E731
        host.prepare_families([trio(k) for k in ("kidA", "kidB", "kidC")])
        assert host.stats == dict(families_from_samples=3, families_from_samples_calls=1, samples_uploaded=7, sample_tables=1, families_host=0)
        host.prepare_families([trio(k) for k in ("kidA", "kidD", "kidE")])  # kidA is known; kidD and kidE bring six new samples
        assert host.stats == dict(families_from_samples=5, families_from_samples_calls=2, samples_uploaded=13, sample_tables=2, families_host=0)
        host.prepare_families([trio(k) for k in ("kidB", "kidC")])  # nothing new
        assert host.stats["families_from_samples_calls"] == 2 and host.stats["samples_uploaded"] == 13
        host.prepare_families([trio("kidA")])  # one kid: not the cohort route's business
        n = sites.n_sites
        for k in kids:
            f = host.family(*trio(k))
            up = eng.add_family(host._sites_h, *sites.family_columns(*trio(k)))
            assert np.array_equal(eng.classify(f, P, n), eng.classify(up, P, n)), k
            a, b = eng.family_fetch(f, n), eng.family_fetch(up, n)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
        assert host.stats["families_host"] == 0
        os.environ["UZ_FAMILY_ROUTE"] = "host"
        try:
            other = PhasingHost(eng, sites, reads)
            other.prepare_families([trio(k) for k in kids])
            assert other.stats["sample_tables"] == 0 and not other._fam_h
            other.family(*trio("kidA"))
            assert other.stats["families_host"] == 1
        finally:
            del os.environ["UZ_FAMILY_ROUTE"]
    finally:
        eng.close()
