"""uz_bcf_rows on the device (k_bcfout_size, the scan, k_bcfout_fill; csrc/bcf_row.hpp is the body) through engine.bcf_rows: the hand-built panel
(tests/bcfrowcases.py) and a seeded fuzz of 600 records -- every line equal to the panel's literal byte for byte, off and samp_at, the records
handed back equal to the stated ones, the chunked cases under their UZ_BCFOUT_CHUNK_BYTES; the view of a decoded file; and the refusals, which
return their codes and leave the context fit for the next call."""
import numpy as np
import pytest

import bcfrowcases
from unfazed_amd import abi
from unfazed_amd.engine import UnfazedHipError

pytestmark = pytest.mark.gpu


def _view(case):
    data, rec_at = bcfrowcases.layout(case)
    return abi.bcf_lines_view(np.frombuffer(data, np.uint8), rec_at, case["dict"], case["contigs"], case["n_samples"])


def _holds(engine, case, monkeypatch, chunk=None):
    if chunk or case["chunk"]:
        monkeypatch.setenv("UZ_BCFOUT_CHUNK_BYTES", str(chunk or case["chunk"]))
    else:
        monkeypatch.delenv("UZ_BCFOUT_CHUNK_BYTES", raising=False)
    text, off, samp_at, hb = engine.bcf_rows(_view(case))
    want = bcfrowcases.expected(case)
    assert np.flatnonzero(hb).tolist() == case["hb"], case["name"]
    assert off[0] == 0 and (off[1:] >= off[:-1]).all() and int(off[-1]) == len(text) and len(off) == len(want) + 1
    for k, (line, samp) in enumerate(want):
        got = text[int(off[k]):int(off[k + 1])]
        assert got == line, (case["name"], k, got[:300], line[:300])
        assert int(samp_at[k]) == int(off[k]) + samp, (case["name"], k)


@pytest.mark.parametrize("case", bcfrowcases.CASES, ids=lambda c: c["name"])
def test_panel(engine, case, monkeypatch):
    _holds(engine, case, monkeypatch)


def test_fuzz(engine, monkeypatch):
    fuzz = bcfrowcases.fuzz_cases(20241022, 600)
    assert sum(len(c["lines"]) for c in fuzz) == 600 and any(c["hb"] for c in fuzz)
    for i, case in enumerate(fuzz):
        _holds(engine, case, monkeypatch, chunk=2048 if i % 3 == 0 else None)


def test_the_blocks_grow_from_call_to_call(hip_lib, monkeypatch):
    """a context's page-locked blocks start empty: a small call, one that outgrows every block (in chunks, so that the result block grows with text
    in it), the small call again -- each the panel's literals, and what a context of its own returns"""
    from unfazed_amd.engine import HipEngine
    small, large, chunk = bcfrowcases.BY_NAME["records/65"], bcfrowcases.BY_NAME["records/2049"], 32768
    assert len(bcfrowcases.layout(large)[0]) > 3 * chunk  # at least three chunks

    def call(e, case):
        text, off, samp_at, hb = e.bcf_rows(_view(case))
        return bytes(text), off.tolist(), samp_at.tolist(), hb.tolist()

    fresh = {}
    for case in (small, large):
        monkeypatch.setenv("UZ_BCFOUT_CHUNK_BYTES", str(chunk))
        e = HipEngine(0)
        try:
            fresh[case["name"]] = call(e, case)
        finally:
            e.close()
    e = HipEngine(0)
    try:
        for case in (small, large, small):
            _holds(e, case, monkeypatch, chunk=chunk)
            assert call(e, case) == fresh[case["name"]], case["name"]
    finally:
        e.close()


def test_the_view_of_a_decoded_file(engine, tmp_path, monkeypatch):
    from unfazed_amd import io_native
    monkeypatch.delenv("UZ_BCFOUT_CHUNK_BYTES", raising=False)
    case = bcfrowcases.BY_NAME["records/257"]
    path = str(tmp_path / "dnms.bcf")
    open(path, "wb").write(bcfrowcases.file_bytes(case))
    table = io_native.read_vcf_table(path)
    view = io_native.vcf_bcf_lines(table)
    assert int(view.n_records) == 257 and int(view.n_samples) == 3 and int(view.n_dict) == len(bcfrowcases.DICT) and int(view.n_contigs) == len(bcfrowcases.CONTIGS)
    data, rec_at, names, contigs = abi.bcf_lines_arrays(view)
    assert names == [x.encode() for x in bcfrowcases.DICT] and contigs == [x.encode() for x in bcfrowcases.CONTIGS]
    text, off, samp_at, hb = engine.bcf_rows(view)
    assert not hb.any() and text == b"".join(e[0] for e in bcfrowcases.expected(case))
    with pytest.raises(io_native.IoError):
        vcf = str(tmp_path / "t.vcf")
        open(vcf, "wb").write(bcfrowcases.text_file_bytes(case))
        io_native.vcf_bcf_lines(io_native.read_vcf_table(vcf))


def test_refusals_return_their_codes_and_the_next_call_succeeds(engine, monkeypatch):
    monkeypatch.delenv("UZ_BCFOUT_CHUNK_BYTES", raising=False)
    case = bcfrowcases.BY_NAME["records/65"]
    data, rec_at = bcfrowcases.layout(case)
    n = len(rec_at)
    arr = np.frombuffer(data, np.uint8)
    descends = rec_at.copy()
    descends[3], descends[4] = rec_at[4], rec_at[3]
    with pytest.raises(UnfazedHipError, match=r"\(-1\)"):  # UZ_E_ARG
        engine.bcf_rows(abi.bcf_lines_view(arr, descends, case["dict"], case["contigs"], 3))
    outside = rec_at.copy()
    outside[-1] = len(data) + 1
    with pytest.raises(UnfazedHipError, match=r"\(-1\)"):
        engine.bcf_rows(abi.bcf_lines_view(arr, outside, case["dict"], case["contigs"], 3))
    view = _view(case)
    view.dict_off = None  # a NULL table
    off, samp, hb, ptr = np.zeros(n + 1, np.int64), np.zeros(n, np.uint64), np.zeros(n, np.uint8), abi.C.c_void_p()
    assert engine.L.uz_bcf_rows(engine.h, abi.C.addressof(view), off.ctypes.data, samp.ctypes.data, abi.C.byref(ptr), hb.ctypes.data) == -1
    view = _view(case)
    assert engine.L.uz_bcf_rows(engine.h, abi.C.addressof(view), off.ctypes.data, None, abi.C.byref(ptr), hb.ctypes.data) == -1
    _holds(engine, case, monkeypatch)
