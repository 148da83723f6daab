"""The device BED route through the product: snv_phaser.phase_snvs_bed(...).lines() must equal summarize.bed_lines(phase_snvs(...)) byte for
byte -- single batches, the chunked route, cohort batches by both read routes, duplicated / SEX-CHROM / candidate-less DNMs -- with the same
stderr messages, and `python -m unfazed_amd` with UZ_BED_ROUTE=device must print what it prints with UZ_BED_ROUTE=host."""
import contextlib
import io
import os
import subprocess
import sys

import pytest

from synth.small import SmallConfig, make_small
from test_cli_golden import _argv, _inputs, _index_inputs
from test_cohort_files_gpu import _indexed_files, _stats
from unfazed_amd import summarize

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = [(False, False), (False, True), (True, False), (True, True)]  # (include_ambiguous, verbose)


def _call(fn, paths, dnms, pedigrees, env, **kw):
    """one product call in a fresh session -> (result, sorted stderr lines, summed stats of its hosts, the DNM dicts it was given)"""
    from unfazed_amd import session
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    session._READS.clear()
    session._HOSTS.clear()
    for k in [k for k in session._SITES if "@" in k]:
        del session._SITES[k]
    try:
        mine = [dict(d) for d in dnms]
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            out = fn(mine, list(pedigrees), pedigrees, paths["sites"], 2, "38", False, 10 ** 9, False, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8], 20, 10, 5000, 1000000, 3, 1,
                     151, 5, **kw)
        return out, sorted(err.getvalue().splitlines()), _stats(list(session._HOSTS.values())), mine
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _both(paths, dnms, pedigrees, env, flags=FLAGS, min_rows=1):
    """both routes for every flag pair; -> the stats of the last device-route call"""
    from unfazed_amd.snv_phaser import phase_snvs, phase_snvs_bed
    records, err_w, _, annotated = _call(phase_snvs, paths, dnms, pedigrees, env)
    assert any("candidate_sites" in d for d in annotated)
    stats = None
    for amb, verbose in flags:
        want = summarize.bed_lines(records, amb, verbose, 10)
        rows, err_g, stats, mine = _call(phase_snvs_bed, paths, dnms, pedigrees, env, include_ambiguous=amb, verbose=verbose)
        assert rows.lines() == want, (amb, verbose)
        assert err_g == err_w
        assert stats["bed_device_rows"] >= min_rows and stats["bed_calls"] >= 1 and stats.get("bed_host_rows", 0) == 0, stats
        assert not any("candidate_sites" in d or "het_sites" in d for d in mine)  # the caller's dicts are not annotated on this route
        if amb and not verbose:
            assert len(want) > 1  # (an empty body cannot pass)
    return stats


def _dnms(ds, paths, kids=None):
    return [dict(chrom=d["chrom"], start=d["start"], end=d["end"], kid=d["kid"], vartype="POINT", bam=paths["bams"][d["kid"]], cram_ref=None)
            for d in ds.dnms if kids is None or d["kid"] in kids]


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    g, ds, paths = _inputs(tmp_path_factory.mktemp("cli"))
    _index_inputs(paths)
    return g, ds, paths


def test_the_cli_dataset_four_flag_pairs(cli, hip_lib):
    g, ds, paths = cli
    _both(paths, _dnms(ds, paths), ds.pedigrees, {"UZ_HOST_CHUNKS": "0"})


def test_a_duplicated_a_sex_chrom_and_a_candidate_less_dnm(cli, hip_lib):
    g, ds, paths = cli
    dnms = _dnms(ds, paths)
    male = next(k for k, p in ds.pedigrees.items() if str(p["sex"]) == "1")
    bam = paths["bams"][male]
    extra = [dict(dnms[0]), dict(dnms[3]),  # keys that come again: one row each, at the first place
             dict(chrom="Y", start=5000000, end=5000001, kid=male, vartype="POINT", bam=bam, cram_ref=None),
             dict(chrom="chrX", start=90000000, end=90000001, kid=male, vartype="POINT", bam=bam, cram_ref=None),
             dict(chrom="2", start=3, end=4, kid=male, vartype="POINT", bam=bam, cram_ref=None)]  # no informative site near it
    records, err, _, _ = _call(__import__("unfazed_amd.snv_phaser", fromlist=["x"]).phase_snvs, paths, dnms[:5] + extra + dnms[5:], ds.pedigrees, {"UZ_HOST_CHUNKS": "0"})
    assert sum(r["evidence_type"] == "SEX-CHROM" for r in records.values()) == 2 and any("No usable informative sites" in ln for ln in err)
    _both(paths, dnms[:5] + extra + dnms[5:], ds.pedigrees, {"UZ_HOST_CHUNKS": "0"})


def test_three_chunks_through_the_chunked_route(tmp_path_factory, hip_lib, monkeypatch):
    from unfazed_amd import pipeline
    ds = make_small(SmallConfig(seed=77, n_dnms=24, kids=["kidA"], odd_read_prob=0.1))
    paths = _indexed_files(ds, tmp_path_factory.mktemp("chunks"))
    seen = []
    orig = pipeline.run_pipelined

    def spy(backend, params, mode, n, chunks, **kw):
        seen.append(len(chunks))
        return orig(backend, params, mode, n, chunks, **kw)
    monkeypatch.setattr(pipeline, "run_pipelined", spy)
    stats = _both(paths, _dnms(ds, paths), ds.pedigrees, {"UZ_HOST_CHUNK_DNMS": "4"})
    assert seen and min(seen) >= 3, seen
    assert stats["bed_calls"] >= 3


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    kids = ["kid%02d" % i for i in range(4)]
    ds = make_small(SmallConfig(seed=2031, n_dnms=24, kids=kids, cluster_prob=0.5, coverage_per_hap=9.0))
    paths = _indexed_files(ds, tmp_path_factory.mktemp("cohort"))
    return ds, paths, _dnms(ds, paths)


@pytest.mark.parametrize("route", ["kid", "cohort"])
def test_a_cohort_by_both_read_routes(cohort, hip_lib, route):
    """kid: every group's own table, laid end to end by uz_phase_cohort -- a row's names come from its group's table, its ids less the group's
    base; cohort: one table over the kids' files (uz_phase_cohort_joined)"""
    ds, paths, dnms = cohort
    stats = _both(paths, dnms, ds.pedigrees, {"UZ_HOST_CHUNKS": "0", "UZ_READS_ROUTE": route}, min_rows=4)
    assert stats["phase_cohort_calls"] >= 1
    assert (stats["read_tables"] == 1) == (route == "cohort")


def _cli_text(paths, run, route, dnms_path=None):
    argv = _argv(paths, run)
    if dnms_path is not None:
        argv[argv.index("-d") + 1] = dnms_path
    out = subprocess.run([sys.executable, "-m", "unfazed_amd"] + argv, cwd=ROOT, check=True, capture_output=True, text=True, env=dict(os.environ, UZ_BED_ROUTE=route))
    return out.stdout


def test_the_driver_prints_the_same_text_by_both_routes(cli, hip_lib):
    g, ds, paths = cli
    runs = [r for r in g["runs"] if r["output_type"] == "bed"]
    assert len(runs) >= 3
    for run in runs:
        host = _cli_text(paths, run, "host")
        assert host.count("\n") > 1 and _cli_text(paths, run, "device") == host


def test_the_driver_with_svs_mixed_in(cli, hip_lib, tmp_path):
    g, ds, paths = cli
    run = next(r for r in g["runs"] if r["output_type"] == "bed" and r["verbose"])
    d = _dnms(ds, paths)
    lines = ["%s\t%d\t%d\t%s\tPOINT" % (x["chrom"], x["start"], x["end"], x["kid"]) for x in d]
    lines += ["%s\t%d\t%d\t%s\tDEL" % (d[0]["chrom"], d[0]["start"], d[0]["start"] + 900, d[0]["kid"]),
              "%s\t%d\t%d\t%s\tDUP" % (d[1]["chrom"], max(1, d[1]["start"] - 400), d[1]["start"] + 400, d[1]["kid"])]
    mixed = tmp_path / "mixed.bed"
    mixed.write_text("\n".join(lines) + "\n")
    run = dict(run, dnms="mixed")
    paths = dict(paths, mixed=str(mixed))
    host = _cli_text(paths, run, "host")
    assert any(ln.split("\t")[3] in ("DEL", "DUP") for ln in host.splitlines()[1:]), host
    assert _cli_text(paths, run, "device") == host
