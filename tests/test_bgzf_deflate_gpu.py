"""uz_bgzf_deflate on the device against the host program of the same body (tests/bgzf_body_main.cpp over unfazed_amd/csrc/deflate_body.hpp):
the device's blocks must equal the program's byte for byte on every payload of the panel (tests/bgzfoutcases.py) -- the test that fails on a
device-only bug -- and zlib and the device's own inflater must turn them back into the payload."""
import numpy as np
import pytest

import bgzfoutcases as panel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_blocks(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_body_gpu")
    exe = panel.build_program(d)
    if exe is None:  # (the sanitizers are not what this file is about)
        exe = panel.build_program(d, san="undefined")
    assert exe is not None
    return dict(zip((name for name, _ in panel.CASES), (blocks for blocks, _ in panel.run_program(exe, panel.CASES, d))))


@pytest.mark.parametrize("name", [name for name, _ in panel.CASES])
def test_the_device_writes_the_host_programs_bytes(engine, host_blocks, name):
    payload = panel.BY_NAME[name]
    blocks, n_blocks, ms = engine.bgzf_deflate(payload)
    assert ms is None and n_blocks == (len(payload) + panel.SLICE - 1) // panel.SLICE
    assert blocks == host_blocks[name]
    panel.check_blocks(payload, blocks)


@pytest.mark.parametrize("name", ["tiny/1", "aaa", "edge/65281", "zeros/65280", "across/65280", "random/65280", "collide/near", "text/vcf"])
def test_the_devices_inflater_reads_the_devices_blocks(engine, name):
    payload = panel.BY_NAME[name]
    blocks, n_blocks, _ = engine.bgzf_deflate(payload)
    back, nb, _ = engine.bgzf_inflate(blocks)
    assert nb == n_blocks and bytes(back) == payload


def test_the_slices_do_not_depend_on_the_chunk_size(engine, host_blocks, monkeypatch):
    payload = panel.BY_NAME["text/vcf"]  # five slices: five chunks of one, or two of two and a short one
    monkeypatch.delenv("UZ_BGZF_CHUNK_BYTES", raising=False)
    whole = engine.bgzf_deflate(payload)[0]
    assert whole == host_blocks["text/vcf"]
    for chunk in (65280, 130560, 130561, 1):
        monkeypatch.setenv("UZ_BGZF_CHUNK_BYTES", str(chunk))
        assert engine.bgzf_deflate(payload)[0] == whole, chunk


def test_a_chunk_of_more_than_1024_slices(engine, monkeypatch):
    """1025 slices: three chunks of at most 514 at the default size (the reference, held by zlib), one chunk of 1025 -- the scan's second tile -- at 1 GiB"""
    unit = panel.BY_NAME["text/vcf"]
    payload = (unit * (1025 * panel.SLICE // len(unit) + 1))[:1025 * panel.SLICE]
    monkeypatch.delenv("UZ_BGZF_CHUNK_BYTES", raising=False)
    chunked, n_blocks, _ = engine.bgzf_deflate(payload)
    assert n_blocks == 1025
    panel.check_blocks(payload, chunked)
    monkeypatch.setenv("UZ_BGZF_CHUNK_BYTES", str(1 << 30))
    whole, n_blocks, _ = engine.bgzf_deflate(payload)
    assert n_blocks == 1025 and whole == chunked


def test_a_second_call_gives_the_same_bytes(engine):
    payload = panel.BY_NAME["text/vcf"]
    first = engine.bgzf_deflate(payload)[0]
    other = engine.bgzf_deflate(panel.BY_NAME["across/65280"])[0]  # (the context's buffers are used in between)
    assert engine.bgzf_deflate(payload)[0] == first and other != first
    assert engine.bgzf_deflate(np.frombuffer(payload, np.uint8))[0] == first


def test_the_measured_form_writes_the_same_bytes(engine, host_blocks):
    blocks, n_blocks, ms = engine.bgzf_deflate(panel.BY_NAME["text/vcf"], repeat=2)
    assert blocks == host_blocks["text/vcf"] and n_blocks == 5 and ms is not None and ms > 0


def test_no_bytes_no_blocks(engine):
    assert engine.bgzf_deflate(b"") == (b"", 0, None)
    import ctypes as C
    nb, size, ptr = C.c_int64(7), C.c_int64(7), C.c_void_p(1)
    assert engine.L.uz_bgzf_deflate(engine.h, None, 0, C.byref(nb), C.byref(ptr), C.byref(size), 0, None) == 0
    assert nb.value == 0 and size.value == 0 and not ptr.value
    assert engine.L.uz_bgzf_deflate(engine.h, None, 5, C.byref(nb), C.byref(ptr), C.byref(size), 0, None) != 0  # UZ_E_ARG: no data
    assert b"no data" in engine.L.uz_last_error(engine.h)
