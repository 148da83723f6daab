"""The BGZF writer's body (unfazed_amd/csrc/deflate_body.hpp: __host__ __device__, what k_bgzf_deflate runs) without a device:
tests/bgzf_body_main.cpp is built with g++ into a program of its own, one host "wave" whose 64 lanes are a plain loop, and run as a child
process under AddressSanitizer + UBSan, with nothing preloaded.  Every slice's input and slot are heap blocks of their exact sizes.  The panel
(tests/bgzfoutcases.py) goes through it; zlib on the host is the judge of every block.

The 300 KB annotated-VCF text is also held to a size: the body's streams against zlib at level 1 with Z_FIXED on the same slices -- the same
code family, so the difference is the matcher alone.  Measured (profiles/bgzf_deflate_ratio.json): 105 675 bytes against 105 953, a ratio of
0.9974; the bound is that ratio plus one tenth.  The output is deterministic: the margin is room for retuning the matcher, not noise."""
import subprocess
import zlib

import pytest

import bgzfoutcases as panel

RATIO_MEASURED = 0.9974  # body bytes / zlib level 1 Z_FIXED bytes on text/vcf (profiles/bgzf_deflate_ratio.json)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_body")
    exe = panel.build_program(d)
    if exe is None:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=address,undefined")
    return exe, d


@pytest.fixture(scope="module")
def results(program):
    exe, d = program
    return dict(zip((name for name, _ in panel.CASES), panel.run_program(exe, panel.CASES, d)))


def test_the_panel_names_the_cases_the_rules_have():
    names = set(panel.BY_NAME)
    assert {"tiny/0", "tiny/1", "tiny/2", "tiny/3", "aaa", "edge/65280", "edge/65281", "zeros/65280", "ab/1000", "dist/32768", "dist/32769", "len/258",
            "len/259", "across/65280", "lit9", "all256", "random/65280", "random/40000", "collide/words", "collide/near", "text/vcf"} <= names
    for d in panel.DIST_EDGES:
        assert "dist/%d" % d in names
    for ln in panel.LEN_EDGES:
        assert "len/%d" % ln in names
    assert len(panel.BY_NAME["edge/65280"]) == panel.SLICE and len(panel.BY_NAME["edge/65281"]) == panel.SLICE + 1
    assert 250_000 <= len(panel.BY_NAME["text/vcf"]) <= 350_000 and len(panel.BY_NAME["text/vcf"]) % panel.SLICE
    assert all(144 <= b for b in panel.BY_NAME["lit9"]) and set(panel.BY_NAME["all256"]) == set(range(256))
    words = panel.colliding_words(40, 9)
    assert len(set(words)) == 40 and len({panel.body_hash(w) for w in words}) == 1


def test_the_stated_hash_is_the_bodys(program):
    exe, _ = program
    for four in (b"\x00\x00\x00\x00", b"abcd", b"\xff\xfe\xfd\xfc", b"chr1", panel.colliding_words(1, 9)[0]):
        run = subprocess.run([exe, "--hash", "%08x" % int.from_bytes(four, "little")], capture_output=True, text=True, timeout=60)
        assert run.returncode == 0 and int(run.stdout) == panel.body_hash(four), (four, run.stdout, run.stderr)


@pytest.mark.parametrize("name", [name for name, _ in panel.CASES])
def test_every_block_is_what_a_reader_takes(results, name):
    payload = panel.BY_NAME[name]
    blocks, stored = results[name]
    parts = panel.check_blocks(payload, blocks)
    assert len(stored) == len(parts)
    for (head, stream, _, _), st in zip(parts, stored):
        assert (stream[0] & 7) == (1 if st else 3)  # BFINAL and BTYPE 00 / 01
    if name == "tiny/0":
        assert blocks == b"" and stored == []


def test_bytes_that_do_not_compress_are_stored_and_fit(results):
    for name in ("random/65280", "random/40000"):
        blocks, stored = results[name]
        n = len(panel.BY_NAME[name])
        assert stored == [True] and len(blocks) == 18 + 5 + n + 8 <= 65536


def _matches(results, name):
    (_, stream, _, _), = panel.split_blocks(results[name][0])
    return [t for t in panel.tokens(stream) if isinstance(t, tuple)]


def test_the_matches_are_found(results):
    """a writer of literals alone would pass every reader's check: the panel's copies must come out as the very tokens they were built to be"""
    assert len(results["zeros/65280"][0]) < 1000 and len(results["ab/40000"][0]) < 1500 and len(results["across/65280"][0]) < 4000
    for name in panel.BY_NAME:
        if name.startswith("dist/"):
            d = int(name[5:])
            found = _matches(results, name)
            assert all(3 <= ln <= 258 and 1 <= dist <= 32768 for ln, dist in found), name
            assert ((40, d) in found) == (d <= 32768), name  # at 32 769 the copy is there and must not be taken
    for ln in panel.LEN_EDGES:
        found = _matches(results, "len/%d" % ln)
        assert ((min(ln, 258), 300) in found) == (ln >= 4), ln  # (the body's hash is of four bytes: a copy of three stays literals)
    assert _matches(results, "len/600")[-3:] == [(258, 300), (258, 300), (84, 300)]
    assert _matches(results, "aaa") == [] and _matches(results, "ab/1000")[0][1] % 2 == 0


def test_the_text_is_held_to_the_fixed_code_of_zlib(results):
    payload = panel.BY_NAME["text/vcf"]
    body = sum(len(p[1]) for p in panel.split_blocks(results["text/vcf"][0]))
    fixed = 0
    for at in range(0, len(payload), panel.SLICE):
        z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        fixed += len(z.compress(payload[at:at + panel.SLICE]) + z.flush())
    print("body %d bytes, zlib level 1 Z_FIXED %d bytes, ratio %.4f" % (body, fixed, body / fixed))
    assert body <= (RATIO_MEASURED + 0.1) * fixed
