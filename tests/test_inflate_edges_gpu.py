"""k_bgzf_inflate (csrc/k_inflate.hip) held to the hand-built DEFLATE streams of tests/deflatecases.py: every path of the decoder that
zlib's compressor reaches by luck or never -- the C++ slow path with each of its copy loops, the canonical walk of 11 .. 15-bit codes,
the largest distance and the other values no compressor emits, the literal window and the input window at every edge, every header
spelling, block sequences -- byte for byte against the plain expansion of each case's tokens (which tests/test_deflate_cases.py holds to
zlib and libdeflate), and one refused stream per rule of the decoder, each with the code it must report.

What these tests catch that tests/test_inflate_gpu.py does not, tried on an MI355X with one-line changes to the kernel (never committed):
  * the slow path's overlap loop without its upward correction (`r >= dist ? r - dist : r` -> `r`): the distance sweep of family C fails (the
    table had no distance at which the correction matters until the sweep was added), nothing of test_inflate_gpu.py does;
  * decode_long stopping at 14 bits: families A, C and E ("wide") fail with code 3, nothing of test_inflate_gpu.py does;
  * the canonical walk in assembly not advancing its symbol index, and the slow path's `dist == 1` loop one byte short: both files fail.
Two changes the issue proposed leave the output as it is by construction, and every test passes with them: the assembly walk bounded at 14
instead of 15 bits hands a 15-bit code to decode_long, which decodes it; without the `dist == 1` branch the modulo loop runs with
1.0f / 1 = 1.0f exactly, so k mod 1 is 0 for every k."""
import numpy as np
import pytest

import deflatecases as dc
from unfazed_amd.engine import UnfazedHipError

pytestmark = pytest.mark.gpu


def check(got, cases, what):
    off = 0
    for c in cases:
        assert bytes(got[off: off + len(c.payload)]) == c.payload, "%s: case %s" % (what, c.name)
        off += len(c.payload)
    assert off == len(got), what


def tables(cases, shift):
    """comp, in_off, out_off of the cases' frames laid end to end behind `shift` bytes: what uz_bgzf_inflate_to_host takes"""
    comp, ins, at = bytearray(b"\xA5" * shift), [], shift
    for c in cases:
        ins.append(at + len(c.frame) - 8 - len(c.stream))
        comp += c.frame
        at += len(c.frame)
    out_off = np.concatenate([[0], np.cumsum([c.isize for c in cases])]).astype(np.int64)
    return np.frombuffer(bytes(comp), np.uint8), np.asarray(ins, np.int64), out_off


@pytest.mark.parametrize("shift", range(4))
def test_valid_cases_in_one_batch(engine, shift):
    """all of them in one launch, the batch's first byte at every alignment"""
    cases = dc.valid()
    got, nb, _ = engine.bgzf_inflate(dc.pad_block(shift) + b"".join(c.frame for c in cases))
    assert nb == len(cases) + 1
    check(got, cases, "uz_bgzf_inflate, batch shifted by %d" % shift)


@pytest.mark.parametrize("shift", range(4))
def test_valid_cases_through_the_staged_route(engine, shift):
    """engine.inflate_blocks (uz_bgzf_inflate_to_host: what BamSource.select(inflate=...) calls), the offsets given directly"""
    cases = dc.valid()
    comp, in_off, out_off = tables(cases, shift)
    out = np.full(int(out_off[-1]), 0xEE, np.uint8)
    engine.inflate_blocks(comp, comp.size, in_off, out_off, out)
    check(out, cases, "uz_bgzf_inflate_to_host, batch shifted by %d" % shift)


ALONE = (["C/len%d-" % l for l in dc.C_LENGTHS] + ["C/sweep/"] + ["E/%s/k%d" % (kind, k) for kind in dc.E_KINDS for k in (1, 2)]
         + ["E/header/stored2%d" % d for d in range(0, 7)])  # (stored200 .. 209, ..., stored260)


@pytest.mark.parametrize("group", ALONE)
def test_one_block_per_launch(engine, group):
    """families C and E again, a lone wave each: no neighbour whose traffic hides a missing wait"""
    cases = [c for c in dc.valid() if c.name.startswith(group)]
    assert cases
    for c in cases:
        got, nb, _ = engine.bgzf_inflate(c.frame)
        assert nb == 1 and bytes(got) == c.payload, c.name


def test_every_case_of_c_and_e_runs_alone():
    want = [c.name for c in dc.valid() if c.family in "CE"]
    seen = [c.name for g in ALONE for c in dc.valid() if c.name.startswith(g)]
    assert sorted(seen) == sorted(want)


GOOD = [dc.bgzf_block(b"a good block in front " * 9, 6), dc.bgzf_block(bytes(range(256)) * 2, 1), dc.bgzf_block(b"", 6)]
GOOD_OUT = b"a good block in front " * 9 + bytes(range(256)) * 2


@pytest.mark.parametrize("name", [c.name for c in dc.refused()])
def test_refused_cases_name_the_block_and_the_rule(engine, name):
    """good x 3 + bad + good x 3: the refusal names block 3 and the rule that fired, on both routes, and the context decodes afterwards"""
    c = next(c for c in dc.refused() if c.name == name)
    with pytest.raises(UnfazedHipError) as e:
        engine.bgzf_inflate(b"".join(GOOD) + c.frame + b"".join(GOOD))
    assert "block 3:" in str(e.value) and "(code %d)" % c.code in str(e.value), (name, str(e.value))

    class G:
        def __init__(self, frame, n):
            self.frame, self.stream, self.isize = frame, frame[18:-8], n
    sandwich = [G(f, n) for f, n in zip(GOOD, (198, 512, 0))]
    comp, in_off, out_off = tables(sandwich + [c] + sandwich, 0)
    with pytest.raises(UnfazedHipError) as e:
        engine.inflate_blocks(comp, comp.size, in_off, out_off, np.zeros(max(1, int(out_off[-1])), np.uint8))
    assert "block 3 " in str(e.value) and "(code %d)" % c.code in str(e.value), (name, str(e.value))
    got, nb, _ = engine.bgzf_inflate(b"".join(GOOD) * 2)
    assert nb == 6 and bytes(got) == GOOD_OUT * 2


def test_the_distance_code_rule_is_the_host_inflaters(engine):
    """a distance code passes when it is complete, absent, or one code of one bit -- zlib's and libdeflate's rule; any other incomplete
    set is refused as bad code lengths although no symbol of the block uses the code's gap"""
    for c in dc.valid():
        if c.family == "H":
            got, nb, _ = engine.bgzf_inflate(c.frame)
            assert nb == 1 and bytes(got) == c.payload, c.name
    for name in ("R/dist-two-2-bit-codes", "R/dist-one-2-bit-code", "R/dist-three-2-bit-codes"):
        c = next(c for c in dc.refused() if c.name == name)
        with pytest.raises(UnfazedHipError, match=r"block 0: .*\(code 2\)"):
            engine.bgzf_inflate(c.frame)
