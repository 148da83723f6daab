"""The sample cells of a text VCF parsed on the device (uz_samples_from_text: k_vcf_tabs + k_vcf_cells, the settle round trip) against the host
route -- eager decode, SitesTable.sample_columns, upload_samples -- through uz_families_from_samples + uz_family_fetch + classify: every row
and every class byte equal.  Inputs: the hand-built edge table (tests/vcfcases.py), the reference's 3-sample VCFs, a synthetic 150-sample
file, and the 50-kid files of tests/test_cohort_files_gpu.py through the product call."""
import contextlib
import glob
import gzip
import io
import os

import numpy as np
import pytest

import vcfcases
from filesio import dump_dataset, vcf_text, write_bai, write_bgzf_text, write_tbi
from helpers import norm_records
from synth.small import SmallConfig, make_small
from unfazed_amd import abi, io_native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIDS = ["kid%02d" % i for i in range(50)]
SMALL_CHUNK = 4000  # bytes of text per chunk in the multi-chunk runs: 200 records span dozens of chunks, and the widest line exceeds it


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _whole(path, **kw):
    names = io_native.tabix_contigs(path)
    k = len(names)
    return io_native.read_vcf_table_regions(path, list(range(k)), [0] * k, [2 ** 31 - 1] * k, **kw)


def _indexed(path, text):
    write_bgzf_text(path, text)
    write_tbi(path)
    return path


def _trios(k):
    """every row as a kid once (the other two members: its neighbours)"""
    return [(r, (r + 1) % k, (r + 2) % k) for r in range(k)]


def _families(eng, table_h, k, n, P):
    t = _trios(k)
    fams = eng.families_from_samples(table_h, [x[0] for x in t], [x[1] for x in t], [x[2] for x in t])
    return [(eng.family_fetch(f, n), eng.classify(f, P, n)) for f in fams]


def _hold_routes_equal(eng, path, pick, want_unsettled=None, chunk=None):
    """both routes on one sites table -> the number of sites the device handed back"""
    from unfazed_amd.engine import UnfazedHipError
    eager, lazy = _whole(path), _whole(path, lazy=True)
    n, k = eager.n_sites, len(pick)
    P = abi.make_params()
    sites_h = eng.upload_sites(eager)
    try:
        up = eng.upload_samples(sites_h, eager.sample_columns([eager.samples[c] for c in pick]))
        want = _families(eng, up, k, n, P)
        with _env(UZ_VCF_CHUNK_BYTES=chunk):
            h, n_back = eng.samples_from_text(sites_h, lazy, pick, settle=False)
        if want_unsettled is not None:
            assert n_back == len(want_unsettled), (n_back, want_unsettled)
            assert list(eng.unsettled_sites(h, n_back)) == list(want_unsettled)
        if n_back:
            with pytest.raises(UnfazedHipError) as e:  # before settle: UZ_E_STATE
                eng.families_from_samples(h, [0], [0], [0])
            assert "(-4)" in str(e.value)
            eng.settle_samples(h, lazy, pick, n_back)
        got = _families(eng, h, k, n, P)
        for r, (w, g) in enumerate(zip(want, got)):
            assert np.array_equal(w[0][0], g[0][0]), ("gt of the trio of row", r)
            assert np.array_equal(w[0][1], g[0][1]), ("16-bit columns of the trio of row", r, np.argwhere(w[0][1] != g[0][1])[:5])
            assert np.array_equal(w[1], g[1]), ("class bytes of the trio of row", r)
        assert lazy.genotypes_deferred  # the host's genotype columns were never made
        return n_back
    finally:
        eng.free_sites(sites_h)


@pytest.fixture(scope="module")
def edge_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("edge")
    out = {}
    for n in (1, 63, 64, 65, 200):
        # (one record: the case with the most forms in it, so that the file is not all defaults)
        cases = [c for c in vcfcases.FILE_CASES if c["name"] == "ad_dot_ro_ao"] if n == 1 else None
        text, used = vcfcases.vcf_text(n, cases=cases)
        out[n] = (_indexed(str(d / ("edge%d.vcf.gz" % n)), text), used, text)
    return out


def _pick(n_pick, seed):
    p = [int(x) for x in np.random.default_rng(seed).permutation(vcfcases.NS)[:n_pick]]
    if n_pick > 1 and p == sorted(p):
        p.reverse()
    return p


@pytest.mark.parametrize("n_records", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("n_pick", [1, 3, 64, 65, 130])
def test_edge_table(engine, edge_files, n_pick, n_records):
    path, used, text = edge_files[n_records]
    pick = _pick(n_pick, 1000 * n_pick + n_records)
    assert n_pick == 1 or pick != sorted(pick)
    want = vcfcases.unsettled_records(used, pick)
    if n_records >= 63 and n_pick >= 3:
        assert 0 < len(want) < n_records  # a condition on the inputs: both kinds of record are there
    assert _hold_routes_equal(eng=engine, path=path, pick=pick, want_unsettled=want) == len(want)
    # the same in chunks of SMALL_CHUNK bytes
    widest = max(len(ln) for ln in text.split("\n")[3:])
    if n_records == 200:
        assert widest > SMALL_CHUNK and len(text) > 20 * SMALL_CHUNK
    assert _hold_routes_equal(eng=engine, path=path, pick=pick, want_unsettled=want, chunk=SMALL_CHUNK) == len(want)


def test_edge_table_wide_sites_reach_the_wide_list(engine, edge_files):
    """depths above 32767 are the host's business: their sites are handed back and stand in the settled table's wide list -- the class bytes of
    a trio with such a member come from the 32-bit depths"""
    path, used, _ = edge_files[200]
    deep = [i for i, c in enumerate(used) if c["name"] in ("depth_32768", "depth_two_to_30")]
    assert len(deep) >= 4
    pick = list(range(6))
    eager = _whole(path)
    cols = eager.sample_columns([eager.samples[c] for c in pick])
    assert cols.wide is not None and sorted(cols.wide[0]) == deep
    want = vcfcases.unsettled_records(used, pick)
    assert set(deep) <= set(want)
    _hold_routes_equal(eng=engine, path=path, pick=pick, want_unsettled=want)


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    """the 50-kid files of tests/test_cohort_files_gpu.py"""
    d = tmp_path_factory.mktemp("cohort")
    ds = make_small(SmallConfig(seed=2025, n_dnms=300, kids=KIDS, cluster_prob=0.5))
    for i in range(4, 50, 5):  # every fifth kid is a sibling of the kid before it
        prev = ds.pedigrees[KIDS[i - 1]]
        ds.pedigrees[KIDS[i]]["dad"], ds.pedigrees[KIDS[i]]["mom"] = prev["dad"], prev["mom"]
    assert len(ds.samples) == 150 and len(ds.dnms) == 300
    paths = dump_dataset(ds, str(d))
    for b in paths["bams"].values():
        write_bai(b)
    _indexed(paths["sites"], gzip.open(paths["sites"], "rt").read())
    return ds, paths, d


@pytest.mark.parametrize("which", ["trio_hets_snvs_chr22.vcf.gz", "trio_hets_svs_chr22.vcf.gz", "synthetic150"])
def test_plain_files_settle_on_the_device(engine, cohort, which):
    """n_unsettled == 0 is a condition on these inputs (every record of the two refdata files lies inside the grammar; the SV file reads RO / AO
    among 15 FORMAT keys): the test cannot pass with the host doing the work"""
    if which == "synthetic150":
        ds, _, d = cohort
        assert len(ds.sites) >= 2000
        path = _indexed(str(d / "plain150.vcf.gz"), vcf_text(ds.samples, ds.sites[:2000], ds.contigs))
        pick = [int(x) for x in np.random.default_rng(3).permutation(150)]
    else:
        path = os.path.join(ROOT, "tests", "golden", "refdata", which)
        pick = [2, 0, 1]
    assert _whole(path).n_sites == {"trio_hets_snvs_chr22.vcf.gz": 82, "trio_hets_svs_chr22.vcf.gz": 51, "synthetic150": 2000}[which]
    assert _hold_routes_equal(eng=engine, path=path, pick=pick, want_unsettled=[]) == 0
    assert _hold_routes_equal(eng=engine, path=path, pick=pick, want_unsettled=[], chunk=64 << 10) == 0


def _phase(paths, ds, kids, env, backend=None, sites=None):
    """one product call on the DNMs of `kids` -> (records, stats of the call's hosts, the hosts)"""
    from unfazed_amd import session
    from unfazed_amd.snv_phaser import phase_snvs
    own = session._BACKEND
    if backend is not None:
        session.set_backend(backend)
    session._READS.clear()
    session._HOSTS.clear()
    for k in [k for k in session._SITES if "@" in k]:
        del session._SITES[k]
    try:
        with _env(**env):
            dnms = [dict(chrom=d["chrom"], start=d["start"], end=d["end"], kid=d["kid"], vartype="POINT", bam=paths["bams"][d["kid"]], cram_ref=None)
                    for d in ds.dnms if d["kid"] in kids]
            err = io.StringIO()
            with contextlib.redirect_stderr(err):
                recs = phase_snvs(dnms, list(kids), ds.pedigrees, sites or paths["sites"], 2, "38", False, 10 ** 9, False, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8], 20, 10,
                                  5000, 1000000, 3, 1, 151, 5)
        hosts = list(session._HOSTS.values())
        stats = {}
        for h in hosts:
            for k, v in h.stats.items():
                stats[k] = stats.get(k, 0) + v
        return norm_records(recs), stats, hosts
    finally:
        if backend is not None:
            session.set_backend(own)


def test_errors_are_the_host_routes(cohort, hip_lib, tmp_path):
    """an unparsable genotype allele and a depth of -5 in a named sample's cell: the product call raises what it raises with UZ_SAMPLES_ROUTE=host"""
    ds, paths, _ = cohort
    kids = KIDS[:3]
    lines = gzip.open(paths["sites"], "rt").read().split("\n")
    head = [i for i, ln in enumerate(lines) if ln.startswith("#CHROM")][0]
    col = 9 + lines[head].split("\t")[9:].index(kids[1])
    dn = [d for d in ds.dnms if d["kid"] == kids[1]][0]
    rec = [i for i, ln in enumerate(lines) if i > head and ln.split("\t")[:2] == [dn["chrom"], str(dn["start"] + 1)]][0]
    for name, cell, exc, what in (("allele", "a/1:5,3:40", io_native.IoError, "unparsable genotype allele"), ("depth", "0/1:-5,3:40", ValueError, "negative allele depth")):
        f = lines[rec].split("\t")
        f[col] = cell
        text = "\n".join(lines[:rec] + ["\t".join(f)] + lines[rec + 1:])
        path = _indexed(str(tmp_path / (name + ".vcf.gz")), text)
        seen = []
        for route in ("host", "device"):
            with pytest.raises(exc) as e:
                _phase(paths, ds, kids, {"UZ_HOST_CHUNKS": "0", "UZ_SAMPLES_ROUTE": route}, sites=path)
            seen.append(str(e.value))
        assert what in seen[0] and seen[0] == seen[1], seen


def test_fifty_kids_through_the_product_call(cohort, hip_lib):
    from oracle_backend import OracleBackend
    ds, paths, _ = cohort
    want, so, _ = _phase(paths, ds, KIDS, {"UZ_HOST_CHUNKS": "0"}, backend=OracleBackend())
    assert len(want) >= 30 and so.get("samples_parsed_device", 0) == 0 and "samples_parsed_device" not in so
    got, sd, hosts = _phase(paths, ds, KIDS, {"UZ_HOST_CHUNKS": "0"})
    assert got == want
    kids_seen = {d["kid"] for d in ds.dnms}
    named = {s for k in kids_seen for s in (k, ds.pedigrees[k]["dad"], ds.pedigrees[k]["mom"])}
    assert sd["samples_parsed_device"] == len(named) > 0 and sd["sites_unsettled"] == 0
    assert sd["sample_tables"] == 1 and sd["samples_uploaded"] == len(named) and sd["families_from_samples"] == len(kids_seen) and sd["families_host"] == 0
    assert all(h.sites.genotypes_deferred for h in hosts)  # the table's host genotype columns were never filled
    host_route, sh, hosts_h = _phase(paths, ds, KIDS, {"UZ_HOST_CHUNKS": "0", "UZ_SAMPLES_ROUTE": "host"})
    assert host_route == want
    assert "samples_parsed_device" not in sh and "sites_unsettled" not in sh and sh["samples_uploaded"] == len(named) and sh["sample_tables"] == 1
    assert not any(h.sites.genotypes_deferred for h in hosts_h)
