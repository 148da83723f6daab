"""The dynamic coder's body (unfazed_amd/csrc/deflate_dyn.hpp: __host__ __device__, what k_bgzf_deflate_dyn runs) without a device:
tests/bgzf_dyn_main.cpp is built with g++ into a program of its own, one host "wave" whose 64 lanes are a plain loop, and run as a child process
under AddressSanitizer + UBSan, with nothing preloaded.  Every slice's input, slot and token buffer are heap blocks of their exact sizes.  The
panel (tests/dyncases.py) goes through it and through the fixed coder's program (tests/bgzf_body_main.cpp); zlib on the host is the judge of
every block, tests/dynmodel.py looks inside.

The 15-bit limit.  deep/litlen and deep/litlen/full were built to reach it: 120 (127) values at 300 (509) copies and a Fibonacci tail, whose
BYTES have a Huffman code 17 (19) bits deep.  Their TOKENS do not: the parse finds two matches (one) in the shuffled bytes, a length symbol that
occurs twice stands beside the tail's 1, 2, 3, and the chain folds -- a plain heap builds a code of 13 (14) bits from the tokens, and so does
the builder, at Huffman's cost.  The limit is never met there, and "longest code exactly 15" cannot be asked of them; they are held to what is
true of them (dynamic, Kraft's sum 1, shorter than fixed, Huffman's cost, the three depths as measured).  deep/strict and deep/strict/full
are the same shape with a tail that survives stray symbols (each count above the sum of the two before it, with room): their tokens' code is
16 and 17 bits deep by the plain model and by the heap that breaks ties toward the shallower tree, so no optimal code fits, and they are held
to the rest: longest code exactly 15, Kraft's sum 1, shorter than the fixed form.  deep/codelen does the same for the 7-bit limit of the code
the lengths are sent in (seed 10 of a seeded search: unlimited depth 8).

The 300 KB annotated-VCF text is also held to a size: the coder's streams against zlib at level 1 with the default strategy on the same
slices.  Measured (profiles/bgzf_deflate_ratio.json): 84 467 bytes against 84 674, a ratio of 0.9976; the bound is that ratio plus one tenth.
The output is deterministic: the margin is room for retuning the matcher, not noise."""
import heapq
import random
import zlib

import pytest

import bgzfoutcases as panel
import dyncases as dyn
import dynmodel as model

RATIO_MEASURED = 0.9976  # dynamic route's bytes / zlib level 1 bytes on text/vcf (profiles/bgzf_deflate_ratio.json)
NAMES = [name for name, _ in dyn.CASES]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_dyn_body")
    exe, fixed = dyn.build_program(d), panel.build_program(d)
    if exe is None or fixed is None:
        pytest.skip("this toolchain cannot link the runtime of -fsanitize=address,undefined")
    return exe, fixed, d


@pytest.fixture(scope="module")
def results(programs):
    """name -> (payload, [(stream, kind, fixed coder's stream, fixed coder stored it?)] per slice)"""
    exe, fixed, d = programs
    out = {}
    for (name, payload), (blocks, kinds), (fblocks, fstored) in zip(dyn.CASES, dyn.run_program(exe, dyn.CASES, d), panel.run_program(fixed, dyn.CASES, d)):
        parts = panel.check_blocks(payload, blocks)
        fparts = panel.split_blocks(fblocks)
        assert len(parts) == len(kinds) == len(fparts) == len(fstored)
        out[name] = (payload, [(p[1], k, f[1], st) for p, k, f, st in zip(parts, kinds, fparts, fstored)])
    return out


@pytest.fixture(scope="module")
def inside(results):
    """name -> the model's block of every slice"""
    out = {}
    for name, (_, slices) in results.items():
        out[name] = []
        for stream, kind, _, _ in slices:
            blocks = model.read(stream)
            assert len(blocks) == 1 and blocks[0].btype == kind  # one block per slice; the kind byte is its BTYPE
            out[name].append(blocks[0])
    return out


def _dynamic(inside):
    return [(name, k, b) for name in NAMES for k, b in enumerate(inside[name]) if b.btype == dyn.DYNAMIC]


def test_the_panel_holds_the_fixed_coders_and_the_new_cases():
    assert [c for c in dyn.CASES[:len(panel.CASES)]] == panel.CASES
    assert set(DEEP) | {"deep/codelen"} <= set(dyn.BY_NAME)
    assert len(dyn.BY_NAME["deep/litlen"]) == 36608 and len(dyn.BY_NAME["deep/litlen/full"]) == 65251
    assert len(dyn.BY_NAME["deep/strict"]) == 30505 and len(dyn.BY_NAME["deep/strict/full"]) == 62474
    for name in DEEP:
        assert max(dyn.BY_NAME[name]) < 144  # (eight bits each in the fixed form: never stored)
    p = dyn.BY_NAME["deep/litlen"]
    assert sorted(p.count(bytes([v])) for v in range(132)) == sorted([300] * 120 + dyn.FIB_TAIL)


@pytest.mark.parametrize("name", NAMES)
def test_every_block_is_what_a_reader_takes_and_no_longer_than_the_fixed_coders(results, inside, name):
    payload, slices = results[name]  # (check_blocks has passed: gzip, header, BSIZE, CRC-32, ISIZE, zlib at eof, at most 5 + n)
    if name == "tiny/0":
        assert slices == []
    for k, ((stream, kind, fstream, fstored), block) in enumerate(zip(slices, inside[name])):
        n = len(payload[k * panel.SLICE:(k + 1) * panel.SLICE])
        assert len(stream) <= len(fstream) <= 5 + n, (name, k)
        if kind == dyn.FIXED:  # the fixed form, chosen: the fixed coder's bytes
            assert not fstored and stream == fstream, (name, k)
        elif kind == dyn.DYNAMIC:
            assert len(stream) < len(fstream), (name, k)
        else:
            assert fstored and stream == fstream and len(stream) == 5 + n and block.raw == payload[k * panel.SLICE:k * panel.SLICE + n], (name, k)
        if kind != dyn.STORED and not fstored:  # the parse is one rule
            fixed_tokens = model.read(fstream)[0].tokens
            if len(fstream) <= 8192:  # (the panel's reader shifts the whole stream per symbol: the long streams are left to the model, held to it here)
                assert fixed_tokens == panel.tokens(fstream), (name, k)
            assert block.tokens == fixed_tokens, (name, k)


def test_the_forms(results):
    kinds = {name: [k for _, k, _, _ in results[name][1]] for name in NAMES}
    assert kinds["lit9"] == [dyn.DYNAMIC] and len(results["lit9"][1][0][0]) < 5 + 5000 and results["lit9"][1][0][3]  # (the fixed coder stores it)
    for name in ("random/65280", "random/40000"):
        n = len(dyn.BY_NAME[name])
        assert kinds[name] == [dyn.STORED] and 18 + len(results[name][1][0][0]) + 8 == 18 + 5 + n + 8 <= 65536
    for name in ("tiny/1", "tiny/2", "tiny/3", "aaa"):
        assert kinds[name] == [dyn.FIXED], name  # the 17-bit-plus header cannot win
    for name in ("text/vcf", "zeros/65280", "ab/40000", "across/65280"):
        want = [dyn.DYNAMIC] * len(kinds[name])
        if name == "across/65280":  # (its third slice is 40 bytes)
            assert len(dyn.BY_NAME[name]) - 2 * panel.SLICE == 40
            want[-1] = kinds[name][-1]
        assert kinds[name] == want and len(want) >= 1, name
    assert len(kinds["text/vcf"]) == 5 and len(kinds["ab/40000"]) == 2


def test_the_lengths_cost_what_huffmans_cost(inside):
    """the cost of an optimal code is one number, though the tree is not"""
    seen = 0
    for name, k, b in _dynamic(inside):
        ll, dd = model.histograms(b.tokens)
        ll_lens, d_lens = b.ll_lens + [0] * (286 - b.hlit), b.d_lens + [0] * (30 - b.hdist)
        assert all((c > 0) == (ln > 0) for c, ln in zip(ll, ll_lens)), (name, k)
        assert max(ll_lens) <= 15 and max(d_lens) <= 15 and model.kraft(ll_lens) == 1, (name, k)
        used_d = sum(1 for c in dd if c)
        if used_d >= 2:
            assert all((c > 0) == (ln > 0) for c, ln in zip(dd, d_lens)) and model.kraft(d_lens) == 1, (name, k)
        else:  # two symbols at one bit, as zlib sends them: the used one and symbol 0 (symbol 1 beside symbol 0)
            assert sorted(d_lens)[-2:] == [1, 1] and sum(d_lens) == 2 and all(ln for c, ln in zip(dd, d_lens) if c), (name, k)
            assert d_lens[0] == 1 and (d_lens[1] == 1 or used_d == 1 and not dd[0] and not dd[1]), (name, k)
        if max(ll_lens) < 15:
            assert model.cost(ll, ll_lens) == model.huffman(ll)[0], (name, k)
        if max(d_lens) < 15 and used_d >= 2:
            assert model.cost(dd, d_lens) == model.huffman(dd)[0], (name, k)
        cl = [0] * 19
        for s, _ in b.cl_syms:
            cl[s] += 1
        assert all((c > 0) == (ln > 0) for c, ln in zip(cl, b.cl_lens)) and max(b.cl_lens) <= 7 and model.kraft(b.cl_lens) == 1, (name, k)
        if max(b.cl_lens) < 7:
            assert model.cost(cl, b.cl_lens) == model.huffman(cl)[0], (name, k)
        seen += 1
    assert seen >= 30


def test_the_header_sends_no_trailing_zero_and_uses_its_run_codes(inside):
    for name, k, b in _dynamic(inside):
        ll, _ = model.histograms(b.tokens)
        assert b.hlit == max(257, max(s for s, c in enumerate(ll) if c) + 1) and b.ll_lens[-1] > 0, (name, k)
        assert b.hdist >= 1 and b.d_lens[-1] > 0, (name, k)
        assert b.hclen >= 4 and (b.hclen == 4 or b.cl_lens[model.CL_ORDER[b.hclen - 1]] > 0), (name, k)
        assert all(ln == 0 for ln in (b.cl_lens[s] for s in model.CL_ORDER[b.hclen:])), (name, k)
    for name in ("text/line", "zeros/65280"):  # a header of plain lengths would pass every reader
        for b in inside[name]:
            assert b.btype == dyn.DYNAMIC and any(s >= 16 for s, _ in b.cl_syms), name
    # the run codes are the short way to say it: zeros/65280 uses three literal / length symbols out of 286 and says so in about twenty symbols
    b, = inside["zeros/65280"]
    assert b.hlit == 286 and len(b.cl_syms) <= 24 and sum(1 for s, _ in b.cl_syms if s == 18) >= 3


def _plain_depth(counts):
    """a heap-built Huffman code's depth, ties broken by age (the plain model)"""
    heap = [(c, i, 0) for i, c in enumerate(counts) if c]
    heapq.heapify(heap)
    serial = len(counts)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        serial += 1
        heapq.heappush(heap, (a[0] + b[0], serial, max(a[2], b[2]) + 1))
    return heap[0][2]


#        the case: (Huffman depth of its BYTES with end-of-block, of its TOKENS by the plain model, of its tokens at the least)
DEEP = {"deep/litlen": (17, 13, 13), "deep/litlen/full": (19, 14, 14), "deep/strict": (15, 16, 16), "deep/strict/full": (16, 17, 17)}


@pytest.mark.parametrize("name", sorted(DEEP))
def test_the_15_bit_limit_through_real_bytes(results, inside, name):
    payload, ((stream, kind, fstream, fstored),) = results[name]
    b, = inside[name]
    ll, _ = model.histograms(b.tokens)
    best_cost, least_depth = model.huffman(ll)
    of_bytes = _plain_depth([payload.count(bytes([v])) for v in range(256)] + [1])
    print(name, "Huffman depth: bytes %d, tokens %d (plain) %d (least); %d matches; longest code sent %d; cost %d against %d; %d bytes against %d fixed"
          % (of_bytes, _plain_depth(ll), least_depth, sum(1 for t in b.tokens if isinstance(t, tuple)), max(b.ll_lens), model.cost(ll, b.ll_lens),
             best_cost, len(stream), len(fstream)))
    # the preconditions, by the plain model: the bytes' code is deeper than 15 in the Fibonacci two, the tokens' in the strict two
    assert (of_bytes, _plain_depth(ll), least_depth) == DEEP[name] and (of_bytes > 15 or name.startswith("deep/strict"))
    assert kind == dyn.DYNAMIC and b.btype == 2 and not fstored and len(stream) < len(fstream)
    assert model.kraft(b.ll_lens) == 1 and max(b.ll_lens) <= 15
    if name.startswith("deep/strict"):  # no optimal code fits: the limit is met, and costs something
        assert least_depth > 15 and _plain_depth(ll) > 15
        assert max(b.ll_lens) == 15 and model.cost(ll, b.ll_lens) > best_cost
    else:  # one fits: it must have been found
        assert model.cost(ll, b.ll_lens) == best_cost and max(b.ll_lens) == least_depth


def test_the_7_bit_limit_through_real_bytes(results, inside):
    (stream, kind, fstream, _), = results["deep/codelen"][1]
    b, = inside["deep/codelen"]
    cl = [0] * 19
    for s, _ in b.cl_syms:
        cl[s] += 1
    best_cost, least_depth = model.huffman(cl)
    assert least_depth > 7  # the precondition: every optimal code of these counts is deeper than the limit
    assert kind == dyn.DYNAMIC and max(b.cl_lens) == 7 and model.kraft(b.cl_lens) == 1 and model.cost(cl, b.cl_lens) > best_cost
    assert len(stream) < len(fstream)


def _fib(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def _code_vectors():
    """[(limit, counts)].  The builder's counters are 32 bits wide (a slice has at most 65 281 tokens): Fibonacci counts over 286 symbols are
    Fibonacci's first thirty, then the thirtieth again."""
    fib30 = _fib(30)
    vectors = [(15, fib30), (15, fib30 + [fib30[-1]] * 256), (7, _fib(19)), (15, list(reversed(fib30))),
               (15, [1 << k for k in range(16)] + [1]), (7, [1, 1, 2, 4, 8, 16, 32, 64]), (15, [1 << k for k in range(20)]), (7, [1 << k for k in range(12)])]
    for n in (2, 3, 19, 30, 286):
        vectors.append((7 if n == 19 else 15, [5] * n))
    vectors += [(15, [0] * 9 + [7] + [0] * 20), (7, [3] + [0] * 18), (15, [0, 4, 0, 0, 9] + [0] * 281), (7, [0] * 17 + [1, 1]), (15, [0] * 286), (7, [0] * 19)]
    rng = random.Random(20241021)
    for k in range(200):
        n, limit = ((286, 15), (30, 15), (19, 7))[k % 3]
        shape = k % 4
        if shape == 0:
            counts = [rng.randrange(0, 300) for _ in range(n)]
        elif shape == 1:
            counts = [int(2 ** (rng.random() * 16)) if rng.random() < 0.7 else 0 for _ in range(n)]
        elif shape == 2:
            counts = [rng.choice((0, 1, 1, 2, 3, 1000, 60000)) for _ in range(n)]
        else:
            counts = [int(1.6 ** min(i, 38)) for i in range(n)]
            rng.shuffle(counts)
        vectors.append((limit, counts))
    return vectors


def test_the_builder_on_count_vectors(programs):
    exe, _, d = programs
    vectors = _code_vectors()
    assert len(vectors) >= 219
    over = 0
    for (limit, counts), lens in zip(vectors, dyn.run_code(exe, vectors, d)):
        used = sum(1 for c in counts if c)
        assert all((c > 0) == (ln > 0) for c, ln in zip(counts, lens)), (limit, counts, lens)
        assert max(lens, default=0) <= limit
        if used >= 2:
            assert model.kraft(lens) == 1, (limit, counts, lens)
        elif used == 1:
            assert sum(lens) == 1
        best_cost, least_depth = model.huffman(counts)
        if least_depth <= limit:
            assert model.cost(counts, lens) == best_cost, (limit, counts, lens)
        else:
            assert model.cost(counts, lens) >= best_cost, (limit, counts, lens)
            over += 1
    assert over >= 20  # (the limit is met by many of them)


def test_the_text_is_held_to_zlib_at_level_1(results):
    payload, slices = results["text/vcf"]
    body = sum(len(s[0]) for s in slices)
    level1 = 0
    for at in range(0, len(payload), panel.SLICE):
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        level1 += len(z.compress(payload[at:at + panel.SLICE]) + z.flush())
    print("dynamic route %d bytes, zlib level 1 %d bytes, ratio %.4f" % (body, level1, body / level1))
    assert body <= (RATIO_MEASURED + 0.1) * level1
