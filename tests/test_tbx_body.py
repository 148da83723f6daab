"""The index writer's line rules (unfazed_amd/csrc/tbx_key.hpp: __host__ __device__, what k_tbx_keys runs) without a device:
tests/tbx_key_main.cpp is built with g++ into a program of its own, the 64 bytes of a step a plain loop, and run as a child process under
AddressSanitizer + UBSan with nothing preloaded; every chunk is a heap block of its exact size.  The whole panel (tests/tbxcases.py) goes
through it at every chunk size, and every row must be the one the per-line model (tests/tbxmodel.py) states: kind, why, name length, bin, beg,
end, and "cut" exactly where the chunk's bytes end before the key columns do."""
import pytest

import tbxcases as panel
import tbxmodel as model


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("tbx_key")
    exe = panel.build_program(d)
    if exe is None:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=address,undefined")
    return exe, d


@pytest.mark.parametrize("chunk", [0] + list(panel.CHUNKS) + [64, 1])
def test_every_row_is_the_models(program, chunk):
    exe, d = program
    cases = panel.CASES if chunk != 1 else [c for c in panel.CASES if len(c[2]) < 2000]  # (one byte a chunk: every line is cut at every byte)
    got = panel.run_program(exe, cases, d, chunk)
    n_cut = 0
    for (name, preset, payload, _), rows in zip(cases, got):
        want = model.rows(payload, preset, chunk or None)
        assert len(rows) == len(want), name
        for r, w in zip(rows, want):
            bin_ = model.reg2bin(w["beg"], w["end"]) if w["kind"] == model.DATA else 0
            assert r == (w["at"], w["kind"], w["why"], w["name_len"], bin_, w["beg"], w["end"]), (name, chunk, w)
            n_cut += w["kind"] == model.CUT
    assert (n_cut > 0) == (chunk != 0)


def test_the_panel_cuts_where_it_was_built_to():
    for name, by_chunk in panel.HOST_ROWS.items():
        _, preset, payload, _ = panel.BY_NAME[name]
        for chunk, rows in by_chunk.items():
            assert model.host_rows(payload, preset, chunk) == rows, (name, chunk)
    for name in ("edge/cut-chrom", "edge/cut-pos", "edge/cut-ref", "edge/cut-end-key", "edge/cut-end-digits"):
        _, preset, payload, _ = panel.BY_NAME[name]
        for chunk in panel.CHUNKS:
            cut = [r for r in model.rows(payload, preset, chunk) if r["cut"]]
            assert len(cut) == 1 and cut[0]["at"] < panel.E < cut[0]["at"] + 80, (name, chunk)
