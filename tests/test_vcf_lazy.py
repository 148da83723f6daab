"""The lazy region decode of a text VCF (uz_vcf_decode_regions_lazy: everything but the sample cells) against the eager one, on the hand-built
edge table's VCF (tests/vcfcases.py) and the reference's VCFs under tests/golden/refdata/: the fixed columns at once, the four genotype
columns after uz_vcf_fill_samples, the kept offsets, uz_vcf_record_samples, and the product through the oracle backend on a lazy table."""
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest

import vcfcases
from filesio import write_bgzf_text, write_tbi
from unfazed_amd import io_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFDATA = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "refdata", "*.vcf.gz")))
EVERYTHING = ([0], [0], [2 ** 31 - 1])


def _whole(path, **kw):
    names = io_native.tabix_contigs(path)
    k = len(names)
    return io_native.read_vcf_table_regions(path, list(range(k)), [0] * k, [2 ** 31 - 1] * k, **kw)


@pytest.fixture(scope="module")
def table_vcf(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcfcases")
    text, used = vcfcases.vcf_text(2 * len(vcfcases.FILE_CASES) + 1)
    path = str(d / "cases.vcf.gz")
    write_bgzf_text(path, text)
    write_tbi(path)
    return path, text, used


def _same_columns(a, b, names):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert np.array_equal(x, y, equal_nan=(k == "gq")), k


FIXED = ("contig_off", "pos", "end", "sflags", "ref_base", "alt_base")
GENO = ("gt", "ref_depth", "alt_depth", "gq")


def test_the_eager_decode_holds_the_tables_values(table_vcf):
    """the yardstick itself: the decoder's values of every cell are the hand-written ones"""
    path, _, used = table_vcf
    t = _whole(path)
    assert t.n_sites == len(used) and t.samples == vcfcases.SAMPLES
    for i, c in enumerate(used):
        for s, (_, want, _) in enumerate(vcfcases.record_cells(c)):
            got = (int(t.gt[s, i]), int(t.ref_depth[s, i]), int(t.alt_depth[s, i]), float(t.gq[s, i]))
            assert got[:3] == tuple(want[:3]) and (got[3] == want[3] or (math.isnan(got[3]) and math.isnan(want[3]))), (c["name"], s, got, want)


@pytest.mark.parametrize("which", ["cases"] + [os.path.basename(p) for p in REFDATA])
def test_lazy_decode_equals_eager(which, table_vcf):
    path = table_vcf[0] if which == "cases" else [p for p in REFDATA if os.path.basename(p) == which][0]
    eager, lazy = _whole(path), _whole(path, lazy=True)
    assert lazy.genotypes_deferred and not eager.genotypes_deferred
    assert lazy.samples == eager.samples and lazy.contigs == eager.contigs and lazy.n_sites == eager.n_sites > 0
    _same_columns(eager, lazy, FIXED)
    n = eager.n_sites
    assert [lazy.ref_str[i] for i in range(n)] == [eager.ref_str[i] for i in range(n)]
    assert [lazy.alt_strs[i] for i in range(n)] == [eager.alt_strs[i] for i in range(n)]
    assert [lazy.lines[i] for i in range(n)] == [eager.lines[i] for i in range(n)]
    assert lazy.header == eager.header
    # the kept offsets: column 10 starts just behind the record's ninth tab (the line end when there is none)
    lib = io_native.load()
    v = io_native.vcf_samples_text(lazy)
    assert v.n_records == n and v.n_samples == len(eager.samples)
    text = C.string_at(v.text, v.text_bytes)
    at = np.ctypeslib.as_array(C.cast(v.samp_at, C.POINTER(C.c_uint64)), (n,))
    end = np.ctypeslib.as_array(C.cast(v.line_end, C.POINTER(C.c_uint64)), (n,))
    slot = np.ctypeslib.as_array(C.cast(v.fmt_slot, C.POINTER(C.c_int32)), (n, 5))
    for i in range(n):
        line = eager.lines[i]
        e = int(end[i])
        assert text[e - len(line.encode()): e].decode() == line and (e == len(text) or text[e: e + 1] == b"\n")
        cols = line.split("\t")
        start = e - len(line.encode())
        if len(cols) > 9:
            ninth = len("\t".join(cols[:9]).encode())
            assert int(at[i]) == start + ninth + 1 and text[int(at[i]) - 1: int(at[i])] == b"\t"
            keys = cols[8].split(":")
            want = [max([k for k, x in enumerate(keys) if x == name], default=-1) for name in ("GT", "AD", "RO", "AO", "GQ")]
            assert list(slot[i]) == want, (i, cols[8])
        else:
            assert int(at[i]) == e and list(slot[i]) == [-1] * 5
    # the handed-back records' reader: the eager columns at those records, in any order of records and samples, without filling the table
    rng = np.random.default_rng(5)
    rec = rng.permutation(n)[: max(1, n // 2)]
    pick = rng.permutation(len(eager.samples))[: min(7, len(eager.samples))]
    g = io_native.vcf_record_samples(lazy, rec, pick)
    for got, k in zip(g, GENO):
        assert np.array_equal(got, getattr(eager, k)[np.ix_(pick, rec)], equal_nan=(k == "gq")), k
    assert lazy.genotypes_deferred and lib.uz_vcf_is_lazy(lazy._native.ptr) == 1
    # the fill: idempotent, the eager values
    _same_columns(eager, lazy, GENO)
    assert not lazy.genotypes_deferred and lib.uz_vcf_is_lazy(lazy._native.ptr) == 0
    assert lib.uz_vcf_fill_samples(lazy._native.ptr, 3) == 0
    _same_columns(eager, lazy, GENO)
    s = eager.sample_columns(eager.samples[:3])
    z = lazy.sample_columns(eager.samples[:3])
    for k in GENO:
        assert np.array_equal(getattr(s, k), getattr(z, k)), k


def test_a_refused_cell_is_refused_by_every_entry_point(tmp_path):
    """an unparsable genotype allele: the eager decode fails; the lazy decode does not look, and the fill and the record reader fail as the
    eager decode does -- the table stays lazy"""
    bad = [c for c in vcfcases.CASES if c["name"] == "gt_letters"]
    text, _ = vcfcases.vcf_text(5, cases=vcfcases.FILE_CASES[:3] + bad)
    path = str(tmp_path / "bad.vcf.gz")
    write_bgzf_text(path, text)
    write_tbi(path)
    with pytest.raises(io_native.IoError) as e0:
        _whole(path)
    assert e0.value.code == -2 and "unparsable genotype allele" in str(e0.value)
    lazy = _whole(path, lazy=True)
    assert lazy.n_sites == 5
    with pytest.raises(io_native.IoError) as e1:
        io_native.vcf_record_samples(lazy, [3], [0])
    with pytest.raises(io_native.IoError) as e2:
        lazy.gt
    assert e1.value.code == e2.value.code == -2 and str(e1.value) == str(e2.value) == str(e0.value)
    assert lazy.genotypes_deferred
    good = io_native.vcf_record_samples(lazy, [0, 1, 2, 4], [1, 0])
    assert good[0].shape == (2, 4)


def test_bcf_and_the_whole_file_decode_stay_eager(tmp_path):
    t = io_native.read_vcf_table(REFDATA[0])
    assert not t.genotypes_deferred and t.gt.shape == (len(t.samples), t.n_sites)


def test_phase_snvs_through_the_oracle_on_a_lazy_table(tmp_path):
    """a consumer that needs the host columns (the oracle backend keeps the per-trio route) gets them through the fill: the records of the
    eager table"""
    import gzip
    from filesio import dump_dataset, write_bai
    from helpers import norm_records
    from oracle_backend import OracleBackend
    from synth.small import SmallConfig, make_small
    from unfazed_amd import session
    from unfazed_amd.snv_phaser import phase_snvs
    kids = ["kidA", "kidB", "kidC"]
    ds = make_small(SmallConfig(seed=11, n_dnms=24, kids=kids, cluster_prob=0.5))
    paths = dump_dataset(ds, str(tmp_path))
    for b in paths["bams"].values():
        write_bai(b)
    write_bgzf_text(paths["sites"], gzip.open(paths["sites"], "rt").read())
    write_tbi(paths["sites"])
    own = session._BACKEND
    real = io_native.read_vcf_table_regions
    made = []

    def run(lazy):
        session._READS.clear()
        session._HOSTS.clear()
        for k in [k for k in session._SITES if "@" in k]:
            del session._SITES[k]

        def decode(*a, **kw):
            kw["lazy"] = lazy
            t = real(*a, **kw)
            made.append((lazy, t, t.genotypes_deferred))
            return t

        io_native.read_vcf_table_regions = decode
        try:
            dnms = [dict(chrom=d["chrom"], start=d["start"], end=d["end"], kid=d["kid"], vartype="POINT", bam=paths["bams"][d["kid"]], cram_ref=None) for d in ds.dnms]
            return norm_records(phase_snvs(dnms, list(kids), ds.pedigrees, paths["sites"], 2, "38", False, 10 ** 9, True, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8], 20, 10,
                                           5000, 1000000, 3, 1, 151, 5))
        finally:
            io_native.read_vcf_table_regions = real

    session.set_backend(OracleBackend())
    try:
        want, got = run(False), run(True)
    finally:
        session.set_backend(own)
        session._HOSTS.clear()
    assert len(want) >= 3 and got == want
    assert [m[0] for m in made] == [False, True] and made[1][2] and not made[1][1].genotypes_deferred and not made[0][2]
