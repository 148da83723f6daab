"""uz_bgzf_deflate_coded with UZ_DF_CODE_DYNAMIC on the device against the host program of the same body (tests/bgzf_dyn_main.cpp over
unfazed_amd/csrc/deflate_dyn.hpp): the device's blocks must equal the program's byte for byte on every payload of the panel (tests/dyncases.py)
-- the test that fails on a device-only bug -- with the same split into stored, fixed and dynamic blocks; the device's own inflater must read
them back; and neither coder may leave anything behind that changes the other's bytes."""
import ctypes as C

import pytest

import bgzfoutcases as panel
import dyncases as dyn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_dyn_gpu")
    exe = dyn.build_program(d)
    if exe is None:  # (the sanitizers are not what this file is about)
        exe = dyn.build_program(d, san="undefined")
    assert exe is not None
    return dict(zip((name for name, _ in dyn.CASES), dyn.run_program(exe, dyn.CASES, d)))


def _split(kinds):
    return tuple(kinds.count(k) for k in (dyn.STORED, dyn.FIXED, dyn.DYNAMIC))


@pytest.mark.parametrize("name", [name for name, _ in dyn.CASES])
def test_the_device_writes_the_host_programs_bytes(engine, host, name):
    payload = dyn.BY_NAME[name]
    blocks, n_blocks, ms, kinds = engine.bgzf_deflate(payload, code="dynamic", kinds=True)
    assert ms is None and n_blocks == (len(payload) + panel.SLICE - 1) // panel.SLICE
    assert blocks == host[name][0]
    assert kinds == _split(host[name][1]) and sum(kinds) == n_blocks
    panel.check_blocks(payload, blocks)


@pytest.mark.parametrize("name", ["tiny/1", "aaa", "lit9", "deep/litlen", "zeros/65280", "across/65280", "random/65280", "text/vcf"])
def test_the_devices_inflater_reads_the_devices_blocks(engine, name):
    payload = dyn.BY_NAME[name]
    blocks, n_blocks, _ = engine.bgzf_deflate(payload, code="dynamic")
    back, nb, _ = engine.bgzf_inflate(blocks)
    assert nb == n_blocks and bytes(back) == payload


def test_the_slices_do_not_depend_on_the_chunk_size(engine, host, monkeypatch):
    payload = dyn.BY_NAME["text/vcf"]  # five slices: five chunks of one, or two of two and a short one
    monkeypatch.delenv("UZ_BGZF_CHUNK_BYTES", raising=False)
    whole = engine.bgzf_deflate(payload, code="dynamic")[0]
    assert whole == host["text/vcf"][0]
    for chunk in (65280, 130560, 130561, 1):
        monkeypatch.setenv("UZ_BGZF_CHUNK_BYTES", str(chunk))
        assert engine.bgzf_deflate(payload, code="dynamic")[0] == whole, chunk


def test_the_two_codes_leave_each_other_alone(engine, host):
    payload = dyn.BY_NAME["text/vcf"]
    dyn1 = engine.bgzf_deflate(payload, code="dynamic")[0]
    fix1 = engine.bgzf_deflate(payload, code="fixed")[0]
    dyn2 = engine.bgzf_deflate(payload, code="dynamic")[0]
    fix2 = engine.bgzf_deflate(payload, code="fixed")[0]
    assert dyn1 == dyn2 == host["text/vcf"][0] and fix1 == fix2 and len(dyn1) < len(fix1)
    assert fix1 == engine.bgzf_deflate(payload)[0]  # the default is the fixed code: today's call, today's 3-tuple
    assert len(engine.bgzf_deflate(payload)) == 3 and engine.bgzf_deflate(payload, kinds=True)[3] == (0, 5, 0)
    for name in ("lit9", "random/40000", "across/65280"):
        assert engine.bgzf_deflate(dyn.BY_NAME[name], code="fixed") == engine.bgzf_deflate(dyn.BY_NAME[name]), name


def test_the_measured_form_writes_the_same_bytes(engine, host):
    blocks, n_blocks, ms, kinds = engine.bgzf_deflate(dyn.BY_NAME["text/vcf"], repeat=2, code="dynamic", kinds=True)
    assert blocks == host["text/vcf"][0] and n_blocks == 5 and ms is not None and ms > 0 and kinds == (0, 0, 5)


def test_a_code_that_is_none_is_refused(engine):
    payload = dyn.BY_NAME["aaa"]
    buf = C.create_string_buffer(payload, len(payload))
    nb, size, ptr = C.c_int64(7), C.c_int64(7), C.c_void_p(1)
    for code in (2, -1, 7):
        rc = engine.L.uz_bgzf_deflate_coded(engine.h, buf, len(payload), code, None, C.byref(nb), C.byref(ptr), C.byref(size), 0, None)
        assert rc != 0 and b"code argument" in engine.L.uz_last_error(engine.h), code
    with pytest.raises(ValueError):
        engine.bgzf_deflate(payload, code="static")
    kinds = (C.c_int64 * 3)(9, 9, 9)
    assert engine.L.uz_bgzf_deflate_coded(engine.h, buf, len(payload), 1, kinds, C.byref(nb), C.byref(ptr), C.byref(size), 0, None) == 0
    assert list(kinds) == [0, 1, 0] and nb.value == 1 and size.value == 18 + 5 + 8


def test_no_bytes_no_blocks(engine):
    assert engine.bgzf_deflate(b"", code="dynamic") == (b"", 0, None)
    assert engine.bgzf_deflate(b"", code="dynamic", kinds=True) == (b"", 0, None, (0, 0, 0))
