"""Hand-built DEFLATE streams (RFC 1951) in BGZF frames: a writer that emits what it is told -- NOT a compressor -- and the table of
cases the device's inflater (csrc/k_inflate.hip) is held to at every edge of its decoder (tests/test_inflate_edges_gpu.py), checked
against zlib and libdeflate on the host (tests/test_deflate_cases.py).

A case is one BGZF block.  Its expected payload is what the writer's tokens expand to in plain Python, a match copied byte by byte:
that expansion is the reference, and the host test holds it to zlib.  A refused case carries the code k_bgzf_inflate reports for it
(the table in front of the kernel: 1 bad block type / stored length, 2 bad code lengths, 3 bad symbol, 4 output overrun or distance
before the block, 5 wrong size) and whether the DEFLATE stream itself is broken (`level` "stream": zlib refuses the raw stream) or only
disagrees with the size its frame declares ("frame": gzip refuses the member).

Two things the issue's list names cannot exist as VALID streams, and stand among the refused ones (code 2: symbol 256 is left without
a length) with the nearest valid case beside them:
  * HCLEN 4 -- the code-length code then has lengths for 16, 17, 18 and 0 only, so every length of both codes is 0 (`hclen-4`); the
    smallest header that can carry a code is HCLEN 5, whose only length is 8: 256 literal / length codes of eight bits (`F/hclen-5`);
  * an `18` run of 138 across the boundary between the two codes -- it would have to run over symbol 256 (`18x138-over-256`); the
    run that crosses has to start behind 256 (`F/18-and-17-across`: an `18` run of 36 from symbol 258 into the distance code, and a `17` run
    of 10 across the boundary in a second block).
"""
import random
import struct
import zlib

EOB = 256
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0] + [x for x in range(1, 14) for _ in (0, 1)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
DEFAULT_CL = {s: (4 if s < 13 else 5) for s in range(19)}  # complete: 13 / 16 + 6 / 32; every symbol has a code, so HCLEN is 19
BGZF_HEAD = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff"


class Bits:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def put(self, val, nbits):  # LSB first, as DEFLATE packs everything but Huffman codes
        self.acc |= (val & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        if self.n >= 64:
            k = self.n >> 3
            self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, code, nbits):  # a Huffman code: most significant bit first
        self.put(int(format(code, "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    def align(self):
        self.put(0, -(len(self.buf) * 8 + self.n) % 8)

    def raw(self, data):
        assert self.n % 8 == 0
        self.buf += self.acc.to_bytes(self.n // 8, "little") + data
        self.acc, self.n = 0, 0

    def count(self):
        return len(self.buf) * 8 + self.n

    def bytes(self):
        return bytes(self.buf) + self.acc.to_bytes((self.n + 7) // 8, "little")


def kraft(lens):
    """the code space the lengths use, in units of 2^-15: 32768 is a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


def canonical(lens):
    """{symbol: (code, length)} of RFC 1951's canonical code (the lengths may be a list or a {symbol: length})"""
    items = sorted(lens.items()) if isinstance(lens, dict) else list(enumerate(lens))
    count = [0] * 16
    for _, l in items:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in items:
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def as_list(lens, n_min):
    if isinstance(lens, dict):
        n = max([n_min] + [s + 1 for s, l in lens.items() if l])
        return [lens.get(s, 0) for s in range(n)]
    return list(lens)


def spell(lens, runs=True):
    """a header spelling of the lengths: plain, or with `17` / `18` for the runs of zeros (`16` only where a case asks for it)"""
    if not runs:
        return list(lens)
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == 0:
            j += 1
        z = j - i
        while z >= 3:
            r = min(z, 138)
            if z - r in (1, 2):  # (leave a run of at least three behind)
                r = z - 3 if z - 3 >= 3 else r
            out.append((18, r) if r >= 11 else (17, r))
            z -= r
        out += [0] * z
        i = j
        if i < len(lens):
            out.append(lens[i])
            i += 1
    return out


def unspell(spelling):
    out = []
    for it in spelling:
        if isinstance(it, tuple):
            out += [out[-1] if it[0] == 16 else 0] * it[1]
        else:
            out.append(it)
    return out


def length_token(length, dist, lsym=None):
    """(length symbol, extra, distance symbol, extra) of a match, the way a compressor spells it (lsym: another symbol that reaches the length)"""
    if lsym is None:
        lsym = 285 if length == 258 else 257 + max(i for i in range(28) if LBASE[i] <= length)
    ds = max(i for i in range(30) if DBASE[i] <= dist)
    t = (lsym, length - LBASE[lsym - 257], ds, dist - DBASE[ds])
    assert 0 <= t[1] < (1 << LEXTRA[lsym - 257]) and 0 <= t[3] < (1 << DEXTRA[ds])
    return t


class Stream:
    """one DEFLATE stream, block after block; .out is what the tokens expand to"""

    def __init__(self):
        self.w, self.out, self.marks = Bits(), bytearray(), []

    def _head(self, final, btype):
        self.w.put(1 if final else 0, 1)
        self.w.put(btype, 2)

    def stored(self, data, final=False, nlen=None):
        self._head(final, 0)
        self.w.align()
        self.w.put(len(data), 16)
        self.w.put(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
        self.w.raw(data)
        self.out += data
        return self

    def fixed(self, tokens, final=False):
        self._head(final, 1)
        self._tokens(canonical(FIXED_LIT), canonical(FIXED_DIST), tokens)
        return self

    def dynamic(self, lit_lens, dist_lens, tokens, final=False, spelling=None, runs=True, cl_lens=None, hclen=None, hlit=None, hdist=None):
        lit, dist = as_list(lit_lens, 257), as_list(dist_lens, 1)
        cl = dict(DEFAULT_CL if cl_lens is None else cl_lens)
        if hclen is None:
            hclen = max([4] + [k + 1 for k, s in enumerate(CL_ORDER) if cl.get(s, 0)])
        self._head(final, 2)
        self.w.put(len(lit) - 257 if hlit is None else hlit, 5)
        self.w.put(len(dist) - 1 if hdist is None else hdist, 5)
        self.w.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.w.put(cl.get(s, 0), 3)
        clc = canonical(cl)
        for it in (spell(lit + dist, runs) if spelling is None else spelling):
            sym, rep = it if isinstance(it, tuple) else (it, 0)
            self.w.code(*clc[sym])
            if sym == 16:
                self.w.put(rep - 3, 2)
            elif sym == 17:
                self.w.put(rep - 3, 3)
            elif sym == 18:
                self.w.put(rep - 11, 7)
        self._tokens(canonical(lit), canonical(dist), tokens)
        return self

    def _tokens(self, lit, dist, tokens):
        w, out = self.w, self.out
        for t in tokens:
            if isinstance(t, int):
                w.code(*lit[t])
                if t < 256:
                    out.append(t)
            elif t[0] == "run":      # ("run", byte, n): n literals
                c, l = lit[t[1]]
                if c == 0:
                    w.put(0, l * t[2])
                else:
                    for _ in range(t[2]):
                        w.code(c, l)
                out += bytes([t[1]]) * t[2]
            elif t[0] == "mark":     # the bit position of the next token
                self.marks.append(w.count())
            elif t[0] == "sym":      # a literal / length symbol and nothing behind it
                w.code(*lit[t[1]])
            elif t[0] == "dsym":     # a distance symbol and nothing behind it
                w.code(*dist[t[1]])
            elif t[0] == "bits":
                w.put(t[1], t[2])
            else:
                ls, lx, ds, dx = t
                w.code(*lit[ls])
                w.put(lx, LEXTRA[ls - 257])
                w.code(*dist[ds])
                w.put(dx, DEXTRA[ds])
                d = DBASE[ds] + dx
                if d <= len(out):  # (a refused case may reach in front of the block: nothing to expand)
                    for _ in range(LBASE[ls - 257] + lx):
                        out.append(out[-d])

    def bytes(self):
        return self.w.bytes()


def frame(stream: bytes, payload: bytes, isize=None, extra=b"") -> bytes:
    """the BGZF block around a DEFLATE stream (extra: subfields in front of BC)"""
    bsize = len(BGZF_HEAD) + 2 + len(extra) + 6 + len(stream) + 8
    assert bsize <= 65536
    return (BGZF_HEAD + struct.pack("<H", len(extra) + 6) + extra + b"BC\x02\x00" + struct.pack("<H", bsize - 1) + stream
            + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload) if isize is None else isize))


def bgzf_block(payload: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body = c.compress(payload) + c.flush()
    bsize = len(body) + 25
    assert bsize <= 65536 + 25
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize) + body
            + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def pad_block(nbytes: int) -> bytes:
    """an empty BGZF block that is 4 + nbytes bytes longer than the plainest one: shifts what follows by nbytes mod 4"""
    return frame(b"\x03\x00", b"", extra=b"PD" + struct.pack("<H", nbytes) + b"\x00" * nbytes)


class Case:
    def __init__(self, name, stream, payload, code=None, level=None, isize=None, extra=b""):
        self.name, self.family = name, name.split("/")[0]
        self.stream, self.payload, self.code, self.level = stream, bytes(payload), code, level
        self.isize = len(self.payload) if isize is None else isize
        self.frame = frame(stream, self.payload, isize, extra)


# ---- codes
LIT_ALL = [9] * 60 + [8] * 226           # all 286 symbols, complete: every code in the 10-bit direct table
DIST_FAST = [4, 4] + [5] * 28            # all 30 symbols, complete: every code in the 8-bit direct table
assert kraft(LIT_ALL) == 32768 and kraft(DIST_FAST) == 32768


def ladder(order):
    """one symbol at each length 1 .. 15 and two at 15 (complete), in the order given"""
    assert len(order) == 16 and len(set(order)) == 16
    return {s: min(k + 1, 15) for k, s in enumerate(order)}


def short_ladder(order):
    """lengths 1, 2, ..., n - 1, n - 1 (complete)"""
    return {s: min(k + 1, len(order) - 1) for k, s in enumerate(order)}


def dist_ladder(placed):
    """a distance code with lengths 1 .. 15, 15 in which placed = {symbol: length} holds; the other lengths go to the lowest free symbols"""
    slots = list(range(1, 16)) + [15]
    lens = {}
    for s, l in placed.items():
        slots.remove(l)
        lens[s] = l
    free = [s for s in range(30) if s not in placed]
    for l, s in zip(slots, free):
        lens[s] = l
    assert kraft(lens.values()) == 32768
    return lens


def dist_slow(syms):
    """the symbols (at most eight) at 15, 15, 14, ... 9 bits: each of them leaves the direct table"""
    return dist_ladder({s: l for s, l in zip(syms, [15, 15, 14, 13, 12, 11, 10, 9])})


_rng = random.Random(20240611)


def rnd(n):
    return bytes(_rng.getrandbits(8) for _ in range(n))


def lits(data):
    return list(data)


# ---- the valid cases
def family_a():
    out = []
    _rng.seed(97)
    # the literal / length code: one symbol at each length 1 .. 15, two at 15; literals at 10 .. 15
    base = [0x61, 257, 256, 0x62, 0x63, 0x64, 0x65, 0x66, 0x67, 0x70, 0x71, 0x72, 0x73, 0x74, 0x75, 0x76]
    variants = {"literals": (base, None), "eob-15": (base[:2] + [0x76] + base[3:15] + [256], None),
                "285-15": (base[:15] + [285], 285), "284-15": (base[:15] + [284], 284)}
    for name, (order, lsym) in variants.items():
        text = [s for s in order if s < 256]
        toks = text + text[::-1] + [(257, 0, 1, 0)] + text * 4 + [(257, 0, 0, 0)]
        if lsym == 285:
            toks += [(285, 0, 1, 0), 0x61, (285, 0, 0, 0)]
        if lsym == 284:
            toks += [(284, 31, 1, 0), 0x61, (284, 0, 0, 0), (284, 17, 1, 0)]
        toks += text[5:] + [EOB]
        s = Stream().dynamic(ladder(order), {0: 1, 1: 1}, toks, final=True)
        out.append(Case("A/lit-ladder/" + name, s.bytes(), s.out))
    # the distance code the same way; symbols 0, 3, 4 and 29 at 8, 9 and 15 bits
    lit = short_ladder([0x61, 257, 256, 0x62, 260, 0x63, 0x64])
    for ds in (0, 3, 4, 29):
        for l in (8, 9, 15):
            dl = dist_ladder({ds: l})
            filler = min(dl, key=lambda s: dl[s])  # the one-bit code
            s = Stream()
            if DBASE[ds] + (1 << DEXTRA[ds]) - 1 > 8:
                s.stored(rnd(DBASE[ds] + (1 << DEXTRA[ds]) - 1))
            toks = [0x61, 0x62, 0x63, 0x64, 0x61, 0x63, (257, 0, ds, 0), 0x62, (260, 0, filler, 0), (260, 0, ds, (1 << DEXTRA[ds]) - 1),
                    (257, 0, ds, (1 << DEXTRA[ds]) // 3), EOB]
            s.dynamic(lit, dl, toks, final=True)
            out.append(Case("A/dist-ladder/sym%d-len%d" % (ds, l), s.bytes(), s.out))
    return out


def family_b():
    out = []
    _rng.seed(98)
    for path in ("fast", "slow"):
        # every length symbol at extra 0 and at its largest extra; 258 as 284 + 31
        dl = DIST_FAST if path == "fast" else dist_slow([0, 2, 5])
        toks = lits(b"lengths!")
        for k, ls in enumerate(range(257, 286)):
            ds = (0, 2, 5)[k % 3]
            toks += [(ls, 0, ds, 0), 0x30 + k, (ls, (1 << LEXTRA[ls - 257]) - 1, ds, (1 if ds == 5 else 0)), 0x31 + k]
        toks += [(284, 31, 2, 0), EOB]
        s = Stream().dynamic(LIT_ALL, dl, toks, final=True)
        out.append(Case("B/lengths/" + path, s.bytes(), s.out))
        # every distance symbol at extra 0 and at its largest extra, up to 32768, behind a stored block of that many bytes
        s = Stream().stored(rnd(32768))
        groups = [list(range(30))] if path == "fast" else [list(range(g, min(g + 8, 30))) for g in range(0, 30, 8)]
        for gi, g in enumerate(groups):
            toks = []
            for ds in g:
                ls = 257 + ds % 20
                toks += [(ls, 0, ds, 0), 0x41 + ds, (ls, 0, ds, (1 << DEXTRA[ds]) - 1)]
            s.dynamic(LIT_ALL, DIST_FAST if path == "fast" else dist_slow(g), toks + [EOB], final=gi == len(groups) - 1)
        assert DBASE[29] + (1 << DEXTRA[29]) - 1 == 32768
        out.append(Case("B/distances/" + path, s.bytes(), s.out))
    return out


C_LENGTHS = (3, 63, 64, 65, 128, 129, 257, 258)
C_SOURCES = ("window", "chain", "stored", "block")


def c_distances(length):
    return sorted({d for d in (1, 2, 3, 63, 64, 65, length - 1, length, length + 1) if d >= 1})


def family_c():
    out = []
    _rng.seed(99)
    for length in C_LENGTHS:
        for dist in c_distances(length):
            for source in C_SOURCES:
                for path in ("fast", "slow"):
                    m = length_token(length, dist)
                    dl = DIST_FAST if path == "fast" else dist_ladder({m[2]: 9 + (length + dist) % 7})
                    n = dist + 7
                    n += 1 if n % 64 == 0 else 0  # (the literals in front are still in the window when the match comes)
                    pre = rnd(n)
                    tail = lits(b"end") + [EOB]
                    s = Stream()
                    if source == "window":
                        s.dynamic(LIT_ALL, dl, lits(pre) + [m] + tail, final=True)
                    elif source == "chain":
                        s.dynamic(LIT_ALL, dl, lits(pre) + [m, m, m] + tail, final=True)
                    elif source == "stored":
                        s.stored(pre).dynamic(LIT_ALL, dl, [m] + tail, final=True)
                    else:
                        s.dynamic(LIT_ALL, dl, lits(pre) + [EOB]).dynamic(LIT_ALL, dl, [m] + tail, final=True)
                    out.append(Case("C/len%d-dist%d/%s/%s" % (length, dist, source, path), s.bytes(), s.out))
    return out


def family_c_sweep():
    """every overlap distance under the longest match, by both paths: byte k of a run comes from k mod dist, which both copy loops take through a
    float reciprocal and one correction either way -- C_RECIPROCAL lists the distances at which 1.0f / dist rounds low enough for k * (1 / dist) to
    fall short of a whole quotient (the host test works them out again), and the hardware's own reciprocal may round others"""
    out = []
    _rng.seed(0xC2)
    for dist in range(2, 258):
        for path in ("fast", "slow"):
            m = length_token(258, dist)
            dl = DIST_FAST if path == "fast" else dist_ladder({m[2]: 9 + dist % 7})
            s = Stream().dynamic(LIT_ALL, dl, lits(rnd(dist + 3)) + [m, 0x2E, EOB], final=True)
            out.append(Case("C/sweep/dist%d/%s" % (dist, path), s.bytes(), s.out))
    return out


C_RECIPROCAL = (41, 47, 55, 61, 82, 83, 94, 97, 107, 109, 110, 115, 121, 122, 123, 141, 159, 164, 165, 166, 188, 189, 194, 209, 214, 218, 219, 220, 227,
                230, 235, 237, 242, 243, 244, 245, 246, 249)


def family_d():
    out = []
    _rng.seed(100)
    for n in (63, 64, 65, 128):
        text = rnd(n)
        s = Stream().dynamic(LIT_ALL, DIST_FAST, lits(text) + [EOB], final=True)
        out.append(Case("D/%d-literals/eob" % n, s.bytes(), s.out))
        for path in ("fast", "slow"):
            s = Stream().dynamic(LIT_ALL, DIST_FAST if path == "fast" else dist_slow([2]), lits(text) + [(259, 0, 2, 0), 0x2E, EOB], final=True)
            out.append(Case("D/%d-literals/match-%s" % (n, path), s.bytes(), s.out))
        for name, want in (("end-at-64s", 0), ("end-off-64s", 37)):  # the literals end the output exactly: ISIZE a multiple of 64, and not
            q = (want - n) % 64 or 64
            s = Stream().stored(rnd(q)).dynamic(LIT_ALL, DIST_FAST, lits(text) + [EOB], final=True)
            assert len(s.out) % 64 == want
            out.append(Case("D/%d-literals/%s" % (n, name), s.bytes(), s.out))
    return out


E_KINDS = {"apart": (5, 5), "dist1": (40, 1), "overlap": (40, 3), "wide": (140, 36)}  # dist >= len, dist == 1, 1 < dist < len; and see e_stream
E_SPAN = (-104, 24)  # where the match's length symbol starts, in bits from bit 2048 k of the stream: at every alignment of the stream's first
                     # byte in its dword (0, 8, 16 or 24 bits more) the positions -80 ... +23 of the input window are all there


def e_stream(n, kind):
    """n one-bit literals, five others, the match.  The first three kinds' codes are short, so their distance is in the bit buffer whether or
    not the buffer was filled up behind the length; "wide" has a length symbol of 15 + 5 bits and a distance symbol of 15 + 4, so that the
    13 bits a length can leave are too few: the distance is right only if the input window moved on in between"""
    length, dist = E_KINDS[kind]
    m = length_token(length, dist)
    if kind == "wide":
        lit = ladder([0x4C, 256, 0x61, 0x62, 0x63, 0x64, 0x65] + list(range(0x66, 0x6E)) + [m[0]])
        dl = dist_ladder({m[2]: 15})
    else:
        lit = short_ladder([0x4C, m[0], 256, 0x61, 0x62, 0x63, 0x64, 0x65])  # the literal 'L' costs one bit
        dl = {m[2]: 1, (m[2] + 1) % 30: 1}
    toks = [("run", 0x4C, n)] + lits(b"abcde") + [("mark",), m, 0x61, 0x64, EOB]
    return Stream().dynamic(lit, dl, toks, final=True)


def family_e():
    out = []
    _rng.seed(101)
    for kind in E_KINDS:
        at0 = e_stream(0, kind).marks[0]
        for k in (1, 2):
            for p in range(2048 * k + E_SPAN[0], 2048 * k + E_SPAN[1]):
                s = e_stream(p - at0, kind)
                assert s.marks[0] == p
                out.append(Case("E/%s/k%d/bit%d" % (kind, k, p), s.bytes(), s.out))
    # a stored block of 200 .. 260 bytes and a fixed block of 0 .. 7 nine-bit literals (one bit of phase each) in front of a dynamic header
    # spelled with plain lengths (158 bytes): the header loop runs out of its input window at every symbol, at every bit
    for n in range(200, 261):
        for t in range(8):
            s = Stream().stored(rnd(n)).fixed([0xC0 + t] * t + [EOB])
            s.dynamic(LIT_ALL, DIST_FAST, lits(b"header") + [length_token(9, 4), length_token(20, n)] + [EOB], final=True, runs=False)
            out.append(Case("E/header/stored%d-phase%d" % (n, t), s.bytes(), s.out))
    return out


def family_f():
    out = []
    _rng.seed(102)
    # a `16` as the first distance entry: it repeats the last literal / length entry's length (257: three bits)
    lit = {0x41: 1, 256: 2, 0x42: 3, 257: 3}
    dist = [3, 3, 3, 3, 1]
    sp = spell(as_list(lit, 257)) + [(16, 3), 3, 1]
    assert unspell(sp) == as_list(lit, 257) + dist
    s = Stream().dynamic(lit, dist, lits(b"ABBA") + [(257, 0, 0, 0), (257, 0, 3, 0), (257, 0, 4, 1), 0x42, (257, 0, 2, 0), EOB], final=True, spelling=sp)
    out.append(Case("F/16-first-distance-entry", s.bytes(), s.out))
    # an `18` run across the boundary (258 .. 285 and the first eight distance entries: 36 zeros), then a `17` run of 10 across it
    lit = as_list(short_ladder([0x41, 256, 257, 0x43]), 258)
    s = Stream().stored(rnd(40))
    sp = spell(lit[:257], runs=False) + [lit[257], (18, 36), 1, 1]
    assert unspell(sp) == lit + [0] * 28 + [0] * 8 + [1, 1]
    s.dynamic(lit + [0] * 28, [0] * 8 + [1, 1], lits(b"ACA") + [(257, 0, 8, 5), (257, 0, 9, 7), EOB], spelling=sp)
    lit2 = as_list(short_ladder([0x41, 256, 0x42, 279]), 280)
    sp = spell(lit2) + [(17, 10), 2, 2, 2, 2]
    assert unspell(sp) == lit2 + [0] * 6 + [0] * 4 + [2] * 4
    s.dynamic(lit2 + [0] * 6, [0] * 4 + [2] * 4, [(279, 0, 4, 1), 0x42, (279, 15, 7, 3), EOB], final=True, spelling=sp)
    out.append(Case("F/18-and-17-across", s.bytes(), s.out))
    # a `16` run of 6 that ends exactly at HLIT + HDIST
    lit = short_ladder([0x41, 256, 257, 0x42])
    sp = spell(as_list(lit, 257)) + [3, 3, (16, 6)]
    s = Stream().dynamic(lit, [3] * 8, lits(b"ABABBABAABBABAAB") + [(257, 0, 3, 0), (257, 0, 7, 2), EOB], final=True, spelling=sp)
    out.append(Case("F/16-run-ends-at-the-end", s.bytes(), s.out))
    # HLIT 286 with HDIST 30
    s = Stream().dynamic(LIT_ALL, DIST_FAST, lits(b"all the codes") + [(285, 0, 6, 3), EOB], final=True)
    out.append(Case("F/hlit-286-hdist-30", s.bytes(), s.out))
    # the shortest code-length header that can carry a code: HCLEN 5, lengths 0 and 8 only
    lit = [8] * 255 + [0, 8]
    s = Stream().dynamic(lit, [0], lits(bytes(range(0, 255, 7))) + [EOB], final=True, cl_lens={0: 1, 8: 1}, runs=False)
    out.append(Case("F/hclen-5", s.bytes(), s.out))
    # HCLEN 19 with its last entry, symbol 15, in use
    order = [0x61, 257, 256] + list(range(0x62, 0x6F))
    s = Stream().dynamic(ladder(order), {0: 1, 1: 1}, lits(bytes(range(0x61, 0x6F))) + [(257, 0, 1, 0), 0x6E, 0x6D, EOB], final=True)
    out.append(Case("F/hclen-19-with-15", s.bytes(), s.out))
    return out


def family_g():
    out = []
    _rng.seed(103)
    one_bit = short_ladder([0x4C, 258, 256, 0x61, 0x62])
    for t in range(8):  # fixed, dynamic, an empty stored block, dynamic, stored: the last block's header at every bit of its byte
        s = Stream().fixed([0x90 + t] * (t + 3) + [length_token(6, 2), 0x41, EOB])
        s.dynamic(LIT_ALL, DIST_FAST, lits(b"second") + [length_token(5, 8), EOB])
        s.stored(b"")
        s.dynamic(one_bit, {3: 1, 6: 1}, [0x61, 0x62, ("run", 0x4C, t), ("mark",), (258, 0, 6, 2), (258, 0, 3, 0), EOB])
        at = s.w.count()
        s.stored(b"the last block, stored", final=True)
        out.append((at % 8, Case("G/five-blocks/phase%d" % (at % 8), s.bytes(), s.out)))
    assert sorted(p for p, _ in out) == list(range(8))
    out = [c for _, c in sorted(out, key=lambda pc: pc[0])]
    text = (b"ACGTTGCAAGCT" * 11 + b"\t" + rnd(40) + b"IIIIIIIIIIIIHHHHGGGG##\n") * 90
    for name, mode in (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH)):  # zlib's flush markers: empty stored blocks between compressed ones
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = b"".join(c.compress(text[i: i + 1000]) + c.flush(mode) for i in range(0, len(text), 1000)) + c.flush()
        out.append(Case("G/zlib-%s-flush" % name, body, text))
    big = rnd(65536 - 18 - 8 - 5)  # the largest stored block a BGZF block can carry
    out.append(Case("G/largest-stored", Stream().stored(big, final=True).bytes(), big))
    s = Stream().dynamic(LIT_ALL, DIST_FAST, lits(b"a subfield in front of BC") + [length_token(11, 9), EOB], final=True)
    out.append(Case("G/extra-subfield", s.bytes(), s.out, extra=b"XY\x02\x00\xAB\xCD"))
    return out


# ---- the refused cases: one stream per rule
def refused_cases():
    out = []
    _rng.seed(1951)
    small = short_ladder([0x61, 256, 257, 0x62])
    one_dist = {0: 1, 1: 1}

    def add(name, code, level, s, isize=None):
        body = s.bytes() + (b"\x00" * 4 if level == "stream" else b"")
        out.append(Case("R/" + name, body, s.out, code=code, level=level, isize=len(s.out) if isize is None else isize))

    # 1: block type, stored lengths
    s = Stream()
    s.w.put(1, 1); s.w.put(3, 2)
    add("btype-3", 1, "stream", s)
    add("stored-len-nlen", 1, "stream", Stream().stored(b"abc", final=True, nlen=3))
    add("stored-past-isize", 1, "frame", Stream().stored(b"abcdefgh", final=True), isize=7)
    # 2: code lengths
    toks = lits(b"ab") + [EOB]
    add("hlit-30", 2, "stream", Stream().dynamic(small, one_dist, toks, final=True, hlit=30))
    add("hdist-30", 2, "stream", Stream().dynamic(small, one_dist, toks, final=True, hdist=30))
    add("cl-incomplete", 2, "stream", Stream().dynamic([2] * 4 + [0] * 252 + [0], [0], [], final=True, cl_lens={0: 1, 2: 2}, spelling=[2, 2, 2, 2]))
    add("cl-over-subscribed", 2, "stream", Stream().dynamic([1, 1], [0], [], final=True, cl_lens={0: 1, 1: 1, 2: 1}, spelling=[1, 1]))
    add("16-first", 2, "stream", Stream().dynamic(small, one_dist, [], final=True, spelling=[(16, 3)] + spell(as_list(small, 257))[1:]))
    add("run-past-the-end", 2, "stream", Stream().dynamic(small, one_dist, [], final=True, spelling=spell(as_list(small, 258)) + [1, (18, 11)]))
    add("no-256", 2, "stream", Stream().dynamic({0x61: 1, 0x62: 1}, one_dist, [0x61, 0x62], final=True))
    add("lit-over-subscribed", 2, "stream", Stream().dynamic({0x61: 1, 0x62: 1, 256: 1}, one_dist, [], final=True))
    add("lit-incomplete-two-codes", 2, "stream", Stream().dynamic({0x61: 2, 256: 2}, one_dist, [0x61, EOB], final=True))
    add("dist-over-subscribed", 2, "stream", Stream().dynamic(small, {0: 1, 1: 1, 2: 1}, toks, final=True))
    add("dist-two-2-bit-codes", 2, "stream", Stream().dynamic(small, {0: 2, 1: 2}, toks, final=True))
    add("dist-one-2-bit-code", 2, "stream", Stream().dynamic(small, {0: 2}, toks, final=True))
    add("dist-three-2-bit-codes", 2, "stream", Stream().dynamic(small, {0: 2, 1: 2, 2: 2}, toks, final=True))
    add("hclen-4", 2, "stream", Stream().dynamic([0] * 257, [0], [], final=True, cl_lens={18: 1, 0: 1}, spelling=[(18, 138), (18, 120)]))
    pre = as_list({0x61: 1}, 148)
    add("18x138-over-256", 2, "stream", Stream().dynamic(pre + [0] * 138, [0, 1], [], final=True, spelling=spell(pre) + [(18, 138), 0, 1]))
    # 3: symbols
    add("fixed-286", 3, "stream", Stream().fixed([0x61, ("sym", 286)], final=True))
    add("fixed-distance-30", 3, "stream", Stream().fixed(lits(b"abc") + [("sym", 257), ("dsym", 30)], final=True), isize=6)
    add("length-without-a-distance-code", 3, "stream", Stream().dynamic(small, [0], [0x61, ("sym", 257), ("bits", 0, 8)], final=True), isize=4)
    add("single-code-unused-bit", 3, "stream", Stream().dynamic({256: 1}, [0], [("bits", 1, 1)], final=True))
    # 4: the output's bounds
    add("distance-before-the-block", 4, "stream", Stream().dynamic(LIT_ALL, DIST_FAST, lits(b"abc") + [length_token(3, 4), EOB], final=True), isize=6)
    s = Stream().dynamic(LIT_ALL, DIST_FAST, lits(b"abcd") + [length_token(10, 2), EOB], final=True)
    add("match-past-isize", 4, "frame", s, isize=13)
    add("65-literals-into-64", 4, "frame", Stream().dynamic(LIT_ALL, DIST_FAST, lits(rnd(65)) + [EOB], final=True), isize=64)
    # 5: the size
    add("eob-short-of-isize", 5, "frame", Stream().dynamic(LIT_ALL, DIST_FAST, lits(b"ten bytes!") + [EOB], final=True), isize=11)
    return out


# the distance codes the rule of csrc/k_inflate.hip's build_table takes, as zlib and libdeflate do: none, one code of one bit, complete
def accepted_distance_codes():
    small = short_ladder([0x61, 256, 257, 0x62])
    out = []
    s = Stream().dynamic(small, [0], lits(b"abba") + [EOB], final=True)
    out.append(Case("H/no-distance-code", s.bytes(), s.out))
    s = Stream().dynamic(small, [1], lits(b"abba") + [(257, 0, 0, 0), 0x62, EOB], final=True)
    out.append(Case("H/one-1-bit-distance-code", s.bytes(), s.out))
    s = Stream().dynamic(small, [0, 0, 1], lits(b"abba") + [(257, 0, 2, 0), 0x62, EOB], final=True)
    out.append(Case("H/one-1-bit-distance-code-symbol-2", s.bytes(), s.out))
    s = Stream().dynamic(small, [2, 2, 2, 2], lits(b"abba") + [(257, 0, 3, 0), (257, 0, 0, 0), EOB], final=True)
    out.append(Case("H/complete-distance-code", s.bytes(), s.out))
    s = Stream().fixed(lits(b"abba") + [length_token(4, 4), length_token(3, 1), EOB], final=True)
    out.append(Case("H/fixed-distance-code", s.bytes(), s.out))
    return out


# refused by zlib and by the device, but not held against libdeflate
ZLIB_ONLY = {"R/single-code-unused-bit": "libdeflate gives a code of one single codeword both values of its bit (deflate_decompress.c: build_decode_table), "
                                         "zlib leaves the other value invalid, and the device follows zlib"}

_cache = {}


def valid():
    if "valid" not in _cache:
        _cache["valid"] = family_a() + family_b() + family_c() + family_c_sweep() + family_d() + family_e() + family_f() + family_g() + accepted_distance_codes()
    return _cache["valid"]


def refused():
    if "refused" not in _cache:
        _cache["refused"] = refused_cases()
    return _cache["refused"]
