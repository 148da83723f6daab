"""The lazy region decode of a BCF (uz_vcf_decode_regions_lazy on NAME.bcf + NAME.bcf.csi: everything but the per-sample values) against the
eager one, on the hand-built edge table's BCF (tests/bcfcases.py): the fixed columns at once, the four genotype columns after
uz_vcf_fill_samples, the kept offsets and descriptors (uz_vcf_samples_bcf), uz_vcf_record_samples, and the product through the oracle backend
on a lazy table."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import bcfcases
from unfazed_amd import abi, io_native

FIXED = ("contig_off", "pos", "end", "sflags", "ref_base", "alt_base")
GENO = ("gt", "ref_depth", "alt_depth", "gq")
SIZES = (1, 63, 64, 65, 200)


def _whole(path, **kw):
    names = io_native.tabix_contigs(path)
    k = len(names)
    return io_native.read_vcf_table_regions(path, list(range(k)), [0] * k, [2 ** 31 - 1] * k, **kw)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bcfcases")
    out = {}
    for n in SIZES:
        # (one record: a case with the most forms in it, so that the file is not all defaults)
        cases = [c for c in bcfcases.FILE_CASES if c["name"] == "ad_dot_ro_ao"] if n == 1 else None
        data, used = bcfcases.bcf_bytes(n, cases=cases)
        out[n] = (bcfcases.write_indexed(str(d / ("cases%d.bcf" % n)), data, block_bytes=7000), data, used)
    return out


def _same_columns(a, b, names):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert np.array_equal(x, y, equal_nan=(k == "gq")), k


def test_the_eager_decode_holds_the_tables_values(files):
    """the yardstick itself: the decoder's values of every cell are the hand-written ones"""
    path, _, used = files[200]
    assert len({c["name"] for c in used}) == len(bcfcases.FILE_CASES)  # every case of the table stands in the file
    t = _whole(path)
    assert t.is_bcf and t.n_sites == len(used) and t.samples == bcfcases.SAMPLES
    for i, c in enumerate(used):
        for s, (_, want, _) in enumerate(bcfcases.record_cells(c)):
            got = (int(t.gt[s, i]), int(t.ref_depth[s, i]), int(t.alt_depth[s, i]), float(t.gq[s, i]))
            assert got[:3] == tuple(want[:3]) and (got[3] == want[3] or (math.isnan(got[3]) and math.isnan(want[3]))), (c["name"], s, got, want)


@pytest.mark.parametrize("n", SIZES)
def test_lazy_decode_equals_eager(n, files):
    path, data, used = files[n]
    eager, lazy = _whole(path), _whole(path, lazy=True)
    lib = io_native.load()
    assert lazy.genotypes_deferred and not eager.genotypes_deferred and lazy.is_bcf and eager.is_bcf
    assert lib.uz_vcf_is_lazy(lazy._native.ptr) == 1 and lib.uz_vcf_is_lazy(eager._native.ptr) == 0
    assert lazy.samples == eager.samples and lazy.contigs == eager.contigs and lazy.n_sites == eager.n_sites == n
    _same_columns(eager, lazy, FIXED)
    assert [lazy.ref_str[i] for i in range(n)] == [eager.ref_str[i] for i in range(n)]
    assert [lazy.alt_strs[i] for i in range(n)] == [eager.alt_strs[i] for i in range(n)]
    assert lazy.header == eager.header
    # the view: every array inside the data, where the file has it, with the descriptor the record states -- for the eager table too
    for table in (lazy, eager):
        v = io_native.vcf_samples_bcf(table)
        assert v.n_records == n and v.n_samples == bcfcases.NS
        blob = C.string_at(v.data, v.data_bytes)
        at = np.ctypeslib.as_array(C.cast(v.fld_at, C.POINTER(C.c_uint64)), (n, 5))
        desc = np.ctypeslib.as_array(C.cast(v.fld_desc, C.POINTER(C.c_uint32)), (n, 5))
        for i, c in enumerate(used):
            where = {key: (f, t, k) for f, (key, t, k) in enumerate(c["fields"])}
            cells = bcfcases.record_cells(c)
            for j, key in enumerate(("GT", "AD", "RO", "AO", "GQ")):
                if key not in where:
                    assert desc[i, j] == 0, (c["name"], key)
                    continue
                f, t, k = where[key]
                assert desc[i, j] == (t | k << 4), (c["name"], key)
                size = k * bcfcases.SIZE[t] * bcfcases.NS
                assert 0 < int(at[i, j]) and int(at[i, j]) + size <= v.data_bytes
                want = b"".join(bcfcases.entry_bytes(t, x) for raw, _, _ in cells for x in raw[f])
                assert blob[int(at[i, j]): int(at[i, j]) + size] == want, (c["name"], key)
    # the handed-back records' reader: the eager columns at those records, in any order of records and samples, a sample picked twice,
    # without filling the table -- on the lazy table and on the eager one
    rng = np.random.default_rng(5 + n)
    rec = rng.permutation(n)[: max(1, n // 2)]
    pick = [int(x) for x in rng.permutation(bcfcases.NS)[:9]]
    pick.append(pick[2])
    for table in (lazy, eager):
        g = io_native.vcf_record_samples(table, rec, pick)
        for got, k in zip(g, GENO):
            assert np.array_equal(got, getattr(eager, k)[np.ix_(pick, rec)], equal_nan=(k == "gq")), k
    assert lazy.genotypes_deferred and lib.uz_vcf_is_lazy(lazy._native.ptr) == 1
    # the fill: idempotent, the eager values
    _same_columns(eager, lazy, GENO)
    assert not lazy.genotypes_deferred and lib.uz_vcf_is_lazy(lazy._native.ptr) == 0
    assert lib.uz_vcf_fill_samples(lazy._native.ptr, 3) == 0
    _same_columns(eager, lazy, GENO)
    s, z = eager.sample_columns(eager.samples[:3]), lazy.sample_columns(eager.samples[:3])
    for k in GENO:
        assert np.array_equal(getattr(s, k), getattr(z, k)), k


def test_each_view_refuses_the_other_format(files, tmp_path):
    import vcfcases
    from filesio import write_bgzf_text, write_tbi
    lib = io_native.load()
    bcf = _whole(files[63][0], lazy=True)
    with pytest.raises(io_native.IoError) as e:
        io_native.vcf_samples_text(bcf)
    assert e.value.code == -5 and "BCF" in str(e.value)  # UZ_IO_E_ARG
    text, _ = vcfcases.vcf_text(5)
    path = str(tmp_path / "t.vcf.gz")
    write_bgzf_text(path, text)
    write_tbi(path)
    for lazy in (False, True):
        with pytest.raises(io_native.IoError) as e:
            io_native.vcf_samples_bcf(_whole(path, lazy=lazy))
        assert e.value.code == -5 and "text" in str(e.value)
    assert lib.uz_vcf_samples_bcf(None, C.byref(abi.VcfBcfView())) != 0


def test_the_whole_file_decode_stays_eager(files):
    t = io_native.read_vcf_table(files[65][0])
    assert t.is_bcf and not t.genotypes_deferred and t.gt.shape == (bcfcases.NS, 65)


def test_a_truncated_format_block_is_refused_at_decode(tmp_path):
    """the FORMAT block of the last record is cut short (its l_indiv says so: the record itself is whole): both decodes refuse the file, with
    the same message -- the lazy decode keeps every bounds check, the device is never handed such an array"""
    seen = []
    for cut in (3, 40):
        data, _ = bcfcases.bcf_bytes(7, truncate_last=cut)
        path = bcfcases.write_indexed(str(tmp_path / ("cut%d.bcf" % cut)), data)
        msgs = []
        for lazy in (False, True):
            with pytest.raises(io_native.IoError) as e:
                _whole(path, lazy=lazy)
            assert e.value.code == -2
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1] and "overruns its record" in msgs[0], msgs
        seen.append(msgs[0])
    # ... and a record whose sample count is not the header's
    data, _ = bcfcases.bcf_bytes(3)
    good = bytearray(data)
    last = len(data) - len(bcfcases.record_bytes(bcfcases.FILE_CASES[2], 120))
    n_fmt_sample = struct.unpack_from("<I", good, last + 8 + 20)[0]
    struct.pack_into("<I", good, last + 8 + 20, (n_fmt_sample & 0xFF000000) | (bcfcases.NS - 1))
    path = bcfcases.write_indexed(str(tmp_path / "count.bcf"), bytes(good))
    msgs = []
    for lazy in (False, True):
        with pytest.raises(io_native.IoError) as e:
            _whole(path, lazy=lazy)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "samples, header has" in msgs[0], msgs


def test_phase_snvs_through_the_oracle_on_a_lazy_bcf_table(tmp_path):
    """a consumer that needs the host columns (the oracle backend keeps the per-trio route) gets them through the fill: the records of the
    eager table"""
    from bcfio import write_bcf
    from filesio import dump_dataset, write_bai, write_csi
    from helpers import norm_records
    from oracle_backend import OracleBackend
    from synth.small import SmallConfig, make_small
    from unfazed_amd import session
    from unfazed_amd.io_vcf import read_vcf
    from unfazed_amd.snv_phaser import phase_snvs
    kids = ["kidA", "kidB", "kidC"]
    ds = make_small(SmallConfig(seed=11, n_dnms=24, kids=kids, cluster_prob=0.5))
    paths = dump_dataset(ds, str(tmp_path))
    for b in paths["bams"].values():
        write_bai(b)
    smp, recs, _ = read_vcf(paths["sites"])
    sites = str(tmp_path / "sites.bcf")
    write_bcf(sites, smp, recs, ds.contigs)
    write_csi(sites)
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
            return norm_records(phase_snvs(dnms, list(kids), ds.pedigrees, sites, 2, "38", False, 10 ** 9, True, [0.0, 0.2], [0.8, 1.0], [0.2, 0.8], 20, 10,
                                           5000, 1000000, 3, 1, 151, 5))
        finally:
            io_native.read_vcf_table_regions = real

    session.set_backend(OracleBackend())
    try:
        want, got = run(False), run(True)
    finally:
        session.set_backend(own)
        session._HOSTS.clear()
        for k in [k for k in session._SITES if "@" in k]:  # (the region tables of this test's batches: later tests start from a clean cache)
            del session._SITES[k]
    assert len(want) >= 3 and got == want
    assert [m[0] for m in made] == [False, True] and made[1][2] and not made[1][1].genotypes_deferred and not made[0][2]
    assert all(m[1].is_bcf for m in made)
