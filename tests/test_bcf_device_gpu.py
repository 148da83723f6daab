"""The per-sample values of a BCF read on the device (uz_samples_from_bcf: k_bcf_cells, the settle round trip) against the host route -- eager
decode, SitesTable.sample_columns, upload_samples -- through uz_families_from_samples + uz_family_fetch + classify: every row and every class
byte equal.  Inputs: the hand-built edge table's BCF (tests/bcfcases.py), a synthetic 150-sample file, and six kids through the product call."""
import contextlib
import io
import os

import numpy as np
import pytest

import bcfcases
from helpers import norm_records
from unfazed_amd import abi, io_native

pytestmark = pytest.mark.gpu

SMALL_CHUNK = 600  # bytes of gathered values per chunk in the multi-chunk runs: 200 records span dozens of chunks, and the widest record exceeds it


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


def _trios(k):
    """every row as a kid once (the other two members: its neighbours)"""
    return [(r, (r + 1) % k, (r + 2) % k) for r in range(k)]


def _families(eng, table_h, k, n, P):
    t = _trios(k)
    fams = eng.families_from_samples(table_h, [x[0] for x in t], [x[1] for x in t], [x[2] for x in t])
    return [(eng.family_fetch(f, n), eng.classify(f, P, n)) for f in fams]


def _host_route(eng, path, pick):
    """the yardstick of one file and pick, computed once: the rows and class bytes of every trio by the host route"""
    eager = _whole(path)
    sites_h = eng.upload_sites(eager)
    try:
        up = eng.upload_samples(sites_h, eager.sample_columns([eager.samples[c] for c in pick]))
        return _families(eng, up, len(pick), eager.n_sites, abi.make_params())
    finally:
        eng.free_sites(sites_h)


def _hold_routes_equal(eng, path, pick, want, want_unsettled=None, chunk=None):
    """the device route on one sites table against `want` (_host_route) -> the number of sites the device handed back"""
    from unfazed_amd.engine import UnfazedHipError
    lazy = _whole(path, lazy=True)
    n, k = lazy.n_sites, len(pick)
    assert lazy.is_bcf and lazy.genotypes_deferred
    sites_h = eng.upload_sites(lazy)
    try:
        with _env(UZ_VCF_CHUNK_BYTES=chunk):
            h, n_back = eng.samples_from_bcf(sites_h, lazy, pick, settle=False)
        if want_unsettled is not None:
            assert n_back == len(want_unsettled), (n_back, want_unsettled)
            assert list(eng.unsettled_sites(h, n_back)) == list(want_unsettled)
        if n_back:
            with pytest.raises(UnfazedHipError) as e:  # before settle: UZ_E_STATE
                eng.families_from_samples(h, [0], [0], [0])
            assert "(-4)" in str(e.value)
            eng.settle_samples(h, lazy, pick, n_back)
        got = _families(eng, h, k, n, abi.make_params())
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
        cases = [c for c in bcfcases.FILE_CASES if c["name"] == "ad_dot_ro_ao"] if n == 1 else None
        data, used = bcfcases.bcf_bytes(n, cases=cases)
        out[n] = (bcfcases.write_indexed(str(d / ("edge%d.bcf" % n)), data), used)
    return out


def _pick(n_pick, how, seed):
    p = [int(x) for x in np.random.default_rng(seed).permutation(bcfcases.NS)[:n_pick]]
    if how == "reversed" or p == sorted(p):
        p = sorted(p, reverse=True)
    elif how == "duplicate":
        p[-1] = p[0]
    return p


def _gathered_bytes(case):
    return sum((n * bcfcases.SIZE[t] * bcfcases.NS + 3) // 4 * 4 for key, t, n in case["fields"] if key in ("GT", "AD", "RO", "AO", "GQ"))


@pytest.mark.parametrize("n_records", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("n_pick,how", [(3, "shuffled"), (64, "reversed"), (65, "duplicate")])
def test_edge_table(engine, edge_files, n_pick, how, n_records):
    path, used = edge_files[n_records]
    pick = _pick(n_pick, how, 1000 * n_pick + n_records)
    assert pick != sorted(pick) and (how != "duplicate" or len(set(pick)) < len(pick))
    want_back = bcfcases.unsettled_records(used, pick)
    if n_records >= 63:
        assert 0 < len(want_back) < n_records  # a condition on the inputs: both kinds of record are there
        kept = {c["name"] for c in used if c["name"] in ("gt_as_characters", "ad_as_floats", "gq_as_characters")}
        assert len(kept) == 3  # records the host keeps to itself by their types stand in the list too
    want = _host_route(engine, path, pick)
    assert _hold_routes_equal(engine, path, pick, want, want_unsettled=want_back) == len(want_back)
    # the same in chunks of SMALL_CHUNK gathered bytes
    if n_records == 200:
        sizes = [_gathered_bytes(c) for c in used]
        assert max(sizes) > SMALL_CHUNK and sum(sizes) > 24 * SMALL_CHUNK
    assert _hold_routes_equal(engine, path, pick, want, want_unsettled=want_back, chunk=SMALL_CHUNK) == len(want_back)


def test_edge_table_wide_sites_reach_the_wide_list(engine, edge_files):
    """depths above 32767 are the host's business: their sites are handed back and stand in the settled table's wide list -- the class bytes of
    a trio with such a member come from the 32-bit depths"""
    path, used = edge_files[200]
    deep = [i for i, c in enumerate(used) if c["name"] in ("depth_32768", "depth_two_to_30", "depth_32768_in_ro")]
    assert len(deep) >= 6
    pick = list(range(6))
    eager = _whole(path)
    cols = eager.sample_columns([eager.samples[c] for c in pick])
    assert cols.wide is not None and sorted(cols.wide[0]) == deep
    want_back = bcfcases.unsettled_records(used, pick)
    assert set(deep) <= set(want_back)
    _hold_routes_equal(engine, path, pick, _host_route(engine, path, pick), want_unsettled=want_back)


def test_a_depth_of_minus_five_raises_the_packs_error_on_settle(engine, tmp_path):
    data, used = bcfcases.bcf_bytes(5, cases=bcfcases.FILE_CASES[:4] + [c for c in bcfcases.CASES if c["name"] == "depth_minus_five"])
    path = bcfcases.write_indexed(str(tmp_path / "minus5.bcf"), data)
    eager, lazy = _whole(path), _whole(path, lazy=True)
    with pytest.raises(ValueError) as e0:
        eager.sample_columns(eager.samples[:3])
    sites_h = engine.upload_sites(lazy)
    try:
        h, n_back = engine.samples_from_bcf(sites_h, lazy, [0, 1, 2], settle=False)
        assert n_back == 1 and list(engine.unsettled_sites(h, 1)) == [4]
        with pytest.raises(ValueError) as e1:
            engine.settle_samples(h, lazy, [0, 1, 2], n_back)
        assert "negative allele depth" in str(e0.value) and str(e0.value) == str(e1.value)
    finally:
        engine.free_sites(sites_h)


def test_a_plain_file_settles_on_the_device(engine, tmp_path):
    """150 samples x 300 records, int8 GT, int16 AD, float GQ, no depth above 32767: n_unsettled == 0 is a condition on this input, so the
    equality cannot come from handing everything back"""
    rng = np.random.default_rng(17)
    ns, n = 150, 300
    alleles = rng.integers(-1, 3, (n, ns, 2))
    gt = ((alleles + 1) << 1 | rng.integers(0, 2, (n, ns, 2))).astype(np.int8)
    ad = rng.integers(-1, 400, (n, ns, 2)).astype(np.int16)
    ad[::7, ::5] = 32767
    gq = np.where(rng.random((n, ns)) < 0.1, -1.0, rng.random((n, ns)) * 120).astype(np.float32)
    samples = ["s%03d" % i for i in range(ns)]
    data = bcfcases.table_bcf_bytes(samples, ["chr1", "chr2"], np.repeat([0, 1], n // 2), np.tile(100 + 7 * np.arange(n // 2), 2), gt, ad, gq)
    path = bcfcases.write_indexed(str(tmp_path / "plain150.bcf"), data)
    t = _whole(path)
    assert t.n_sites == n and t.samples == samples and int(t.ref_depth.max()) == 32767 and len(set(t.gt.ravel())) == 4
    pick = [int(x) for x in rng.permutation(ns)]
    want = _host_route(engine, path, pick)
    assert _hold_routes_equal(engine, path, pick, want, want_unsettled=[]) == 0
    assert _hold_routes_equal(engine, path, pick, want, want_unsettled=[], chunk=16 << 10) == 0


def _phase(paths, ds, kids, env, sites):
    """one product call on the DNMs of `kids` -> (records, stats of the call's hosts, the hosts)"""
    from unfazed_amd import session
    from unfazed_amd.snv_phaser import phase_snvs
    session._READS.clear()
    session._HOSTS.clear()
    for k in [k for k in session._SITES if "@" in k]:
        del session._SITES[k]
    with _env(**env):
        dnms = [dict(chrom=d["chrom"], start=d["start"], end=d["end"], kid=d["kid"], vartype="POINT", bam=paths["bams"][d["kid"]], cram_ref=None)
                for d in ds.dnms if d["kid"] in kids]
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            recs = phase_snvs(dnms, list(kids), ds.pedigrees, sites, 2, "38", False, 10 ** 9, False, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8], 20, 10,
                              5000, 1000000, 3, 1, 151, 5)
    hosts = list(session._HOSTS.values())
    stats = {}
    for h in hosts:
        for k, v in h.stats.items():
            stats[k] = stats.get(k, 0) + v
    return norm_records(recs), stats, hosts


def test_six_kids_through_the_product_call(hip_lib, tmp_path):
    """the sites file as BCF + CSI: the route a call takes by default against UZ_SAMPLES_ROUTE=host"""
    from bcfio import write_bcf
    from filesio import dump_dataset, write_bai, write_csi
    from synth.small import SmallConfig, make_small
    from unfazed_amd.io_vcf import read_vcf
    kids = ["kid%d" % i for i in range(6)]
    ds = make_small(SmallConfig(seed=41, n_dnms=48, kids=kids, cluster_prob=0.5))
    paths = dump_dataset(ds, str(tmp_path))
    for b in paths["bams"].values():
        write_bai(b)
    smp, recs, _ = read_vcf(paths["sites"])
    sites = str(tmp_path / "sites.bcf")
    write_bcf(sites, smp, recs, ds.contigs, int16_depths=True)
    write_csi(sites)
    got, sd, hosts = _phase(paths, ds, kids, {"UZ_HOST_CHUNKS": "0", "UZ_SAMPLES_ROUTE": None}, sites)
    want, sh, hosts_h = _phase(paths, ds, kids, {"UZ_HOST_CHUNKS": "0", "UZ_SAMPLES_ROUTE": "host"}, sites)
    assert len(want) >= 6 and got == want
    kids_seen = {d["kid"] for d in ds.dnms}
    named = {s for k in kids_seen for s in (k, ds.pedigrees[k]["dad"], ds.pedigrees[k]["mom"])}
    assert len(kids_seen) == 6
    assert sd["samples_parsed_device"] == len(named) > 0 and sd["sites_unsettled"] == 0
    assert sd["sample_tables"] == 1 and sd["samples_uploaded"] == len(named) and sd["families_from_samples"] == len(kids_seen) and sd["families_host"] == 0
    assert all(h.sites.is_bcf and h.sites.genotypes_deferred for h in hosts)  # the table's host genotype columns were never filled
    assert "samples_parsed_device" not in sh and "sites_unsettled" not in sh and sh["samples_uploaded"] == len(named) and sh["sample_tables"] == 1
    assert all(h.sites.is_bcf for h in hosts_h) and not any(h.sites.genotypes_deferred for h in hosts_h)
