"""A plain reader of raw DEFLATE (RFC 1951), for looking inside the streams of the dynamic coder (unfazed_amd/csrc/deflate_dyn.hpp): zlib stays the
judge of whether a stream is valid; this says what it is made of.  Also the yardsticks of the code lengths: a heap-built Huffman code's cost and
depth, and Kraft's sum."""
import heapq
from fractions import Fraction

from bgzfoutcases import DEXTRA, DIST_EDGES, LBASE, LEXTRA

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


class Block:
    """one block of a stream: btype; for BTYPE 2 hlit / hdist / hclen (the counts, not the fields), cl_lens [19], cl_syms [(symbol, extra value)]
    as sent, ll_lens [hlit], d_lens [hdist]; for BTYPE 1 and 2 tokens (a literal as an int, a match as (length, distance)), for BTYPE 0 raw"""


def canonical(lens):
    """code lengths -> {(length, code): symbol}"""
    out, code = {}, 0
    for ln in range(1, max(lens, default=0) + 1):
        for sym, v in enumerate(lens):
            if v == ln:
                out[(ln, code)] = sym
                code += 1
        code <<= 1
    return out


def read(stream: bytes):
    """-> [Block] of a whole raw DEFLATE stream; asserts that it ends in its last byte with zero padding"""
    at, blocks = 0, []  # at: the bit position
    acc, have, fed = 0, 0, 0  # the bits taken from the bytes and not yet handed out

    def take(n):
        nonlocal at, acc, have, fed
        while have < n:
            assert fed < len(stream), "the stream ends inside a block"
            acc |= stream[fed] << have
            fed += 1
            have += 8
        v = acc & ((1 << n) - 1)
        acc >>= n
        have -= n
        at += n
        return v

    def sym_of(table):
        ln, code = 0, 0
        while True:
            code = (code << 1) | take(1)
            ln += 1
            assert ln <= 15, "no code of 15 bits or fewer"
            if (ln, code) in table:
                return table[(ln, code)]
    final = 0
    while not final:
        b = Block()
        final, b.btype = take(1), take(2)
        assert b.btype < 3
        if b.btype == 0:
            assert take(-at % 8) == 0
            n, nn = take(16), take(16)
            assert n ^ nn == 0xFFFF
            assert have == 0 and fed == at // 8
            b.raw = stream[fed:fed + n]
            assert len(b.raw) == n
            fed += n
            at += 8 * n
            blocks.append(b)
            continue
        if b.btype == 1:
            ll, dd = canonical(FIXED_LL), canonical([5] * 30)
        else:
            b.hlit, b.hdist, b.hclen = take(5) + 257, take(5) + 1, take(4) + 4
            assert b.hlit <= 286 and b.hdist <= 30
            b.cl_lens = [0] * 19
            for k in range(b.hclen):
                b.cl_lens[CL_ORDER[k]] = take(3)
            cl, lens, b.cl_syms = canonical(b.cl_lens), [], []
            while len(lens) < b.hlit + b.hdist:
                s = sym_of(cl)
                if s < 16:
                    b.cl_syms.append((s, 0))
                    lens.append(s)
                else:
                    x = take({16: 2, 17: 3, 18: 7}[s])
                    b.cl_syms.append((s, x))
                    assert s != 16 or lens
                    lens += [lens[-1]] * (3 + x) if s == 16 else [0] * ((3 if s == 17 else 11) + x)
            assert len(lens) == b.hlit + b.hdist
            b.ll_lens, b.d_lens = lens[:b.hlit], lens[b.hlit:]
            ll, dd = canonical(b.ll_lens), canonical(b.d_lens)
        b.tokens = []
        while True:
            s = sym_of(ll)
            if s == 256:
                break
            if s < 256:
                b.tokens.append(s)
                continue
            assert s <= 285
            length = LBASE[s - 257] + take(LEXTRA[s - 257])
            d = sym_of(dd)
            assert d < 30
            b.tokens.append((length, DIST_EDGES[d] + take(DEXTRA[d])))
        blocks.append(b)
    assert fed == len(stream) == (at + 7) // 8 and acc == 0  # zero padding to the byte, nothing behind it
    return blocks


def len_symbol(length):
    return 285 if length == 258 else max(k for k in range(28) if LBASE[k] <= length) + 257


def dist_symbol(dist):
    return max(k for k in range(30) if DIST_EDGES[k] <= dist)


def histograms(tokens):
    """-> (literal / length counts [286] with end-of-block counted once, distance counts [30])"""
    ll, dd = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            ll[len_symbol(t[0])] += 1
            dd[dist_symbol(t[1])] += 1
        else:
            ll[t] += 1
    return ll, dd


def huffman(counts):
    """a heap-built Huffman code over the non-zero counts -> (cost = sum of count * length, the longest length); one symbol costs one bit each"""
    used = [c for c in counts if c]
    if not used:
        return 0, 0
    if len(used) == 1:
        return used[0], 1
    heap = [(c, 0) for c in used]  # (weight, depth of the subtree)
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return cost, heap[0][1]


def huffman_depth_min(counts):
    """the smallest longest-length any optimal code of these counts can have (ties in the heap broken toward the shallower subtree)"""
    return huffman(counts)[1]


def cost(counts, lens):
    return sum(c * ln for c, ln in zip(counts, lens))


def kraft(lens):
    return sum((Fraction(1, 1 << ln) for ln in lens if ln), Fraction(0))
