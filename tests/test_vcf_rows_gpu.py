"""uz_vcf_rows on the device (k_vcfout_size, the scan, k_vcfout_fill; csrc/vcf_row.hpp is the body) through engine.vcf_rows: the hand-built panel
(tests/vcfrowcases.py) and a seeded fuzz of 600 records, every record line equal to the host write_vcf_output's byte for byte, the records handed
back equal to the stated ones, the chunked cases under their UZ_VCFOUT_CHUNK_BYTES; and the refusals, which return their codes and leave the
context fit for the next call."""
import numpy as np
import pytest

import vcfrowcases
from unfazed_amd import abi
from unfazed_amd.engine import UnfazedHipError

pytestmark = pytest.mark.gpu


def _call(engine, case, d=None, ann=None):
    d = d or vcfrowcases.decode(case)
    ann = ann or vcfrowcases.annotations(case, d)
    view = abi.vcf_text_view(np.frombuffer(d["text"], np.uint8), d["samp_at"], d["line_end"], d["n_samples"])
    return engine.vcf_rows(view, d["line_at"], *ann)


def _holds(engine, case, tmp_path, monkeypatch):
    if case["chunk"]:
        monkeypatch.setenv("UZ_VCFOUT_CHUNK_BYTES", str(case["chunk"]))
    else:
        monkeypatch.delenv("UZ_VCFOUT_CHUNK_BYTES", raising=False)
    want = vcfrowcases.expected_rows(case, tmp_path)
    text, off, hb = _call(engine, case)
    assert np.flatnonzero(hb).tolist() == case["hb"], case["name"]
    assert off[0] == 0 and (off[1:] >= off[:-1]).all() and int(off[-1]) == len(text)
    for k, w in enumerate(want):
        got = text[int(off[k]):int(off[k + 1])]
        assert got == (b"" if w is None else w), (case["name"], k, got[:300], (w or b"")[:300])


@pytest.mark.parametrize("case", vcfrowcases.CASES, ids=lambda c: c["name"])
def test_panel(engine, case, tmp_path, monkeypatch):
    _holds(engine, case, tmp_path, monkeypatch)


def test_fuzz(engine, tmp_path, monkeypatch):
    fuzz = vcfrowcases.fuzz_cases(20240918, 600)
    assert sum(len(c["lines"]) for c in fuzz) == 600 and any(c["hb"] for c in fuzz)
    for i, case in enumerate(fuzz):
        case = dict(case, chunk=2048 if i % 3 == 0 else None)
        _holds(engine, case, tmp_path, monkeypatch)


def test_refusals_return_their_codes_and_the_next_call_succeeds(engine, tmp_path, monkeypatch):
    monkeypatch.delenv("UZ_VCFOUT_CHUNK_BYTES", raising=False)
    case = vcfrowcases.BY_NAME["records/65"]
    d = vcfrowcases.decode(case)
    off, col, gt, uops, uet = vcfrowcases.annotations(case, d)
    assert int(off[-1]) > 2
    bad = off.copy()
    bad[3] = bad[2] + 5
    bad[4] = bad[2]  # descends
    with pytest.raises(UnfazedHipError, match=r"\(-1\)"):
        _call(engine, case, d, (bad, col, gt, uops, uet))
    view = abi.vcf_text_view(np.frombuffer(d["text"], np.uint8), d["samp_at"], d["line_end"], d["n_samples"])
    out_off, out_hb, ptr = np.zeros(len(off), np.int64), np.zeros(len(off), np.uint8), abi.C.c_void_p()
    rc = engine.L.uz_vcf_rows(engine.h, abi.C.addressof(view), d["line_at"].ctypes.data, off.ctypes.data, None, None, None, None, out_off.ctypes.data,
                              abi.C.byref(ptr), out_hb.ctypes.data)
    assert rc == -1  # UZ_E_ARG: annotations without their table
    _holds(engine, case, tmp_path, monkeypatch)
