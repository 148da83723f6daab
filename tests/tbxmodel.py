"""A plain per-line model of the tabix index the BGZF writer puts beside its file: the line rules of unfazed_amd/csrc/tbx_key.hpp and the table
rules of csrc/k_tbx.hip / unfazed_amd/tabix_index.py, written once more, line by line with split(), with none of their code.  Test infrastructure:
the body's host program, the host builder and the device's tables are all held to it (test_tbx_body.py, test_tbx_out_host.py, test_tbx_gpu.py),
and it is held to filesio.write_tbi (test_tbx_model.py)."""
import struct
import zlib

SLICE = 0xFF00
MAX_END = 1 << 29
META, DATA, CUT, BAD = 0, 1, 2, 3
WHY_EMPTY, WHY_CR, WHY_POS = 1, 2, 3
HEADERS = {"vcf": (2, 1, 2, 0, ord("#"), 0), "bed": (0x10000, 1, 2, 3, ord("#"), 0)}


def lines(payload: bytes):
    """(start, end) of every line: end is its '\\n', or the text's end"""
    out, at, n = [], 0, len(payload)
    while at < n:
        e = payload.find(b"\n", at)
        e = n if e < 0 else e
        out.append((at, e))
        at = e + 1
    return out


def _pos(field):
    return int(field) if 1 <= len(field) <= 10 and all(48 <= c <= 57 for c in field) else None


def key(line: bytes, preset: str):
    """one line without its '\\n' -> (kind, why, name, beg, end, walked): walked = the bytes of the key columns, whose end is the tab behind
    them or the line's end"""
    meta = line.startswith(b"#")
    want = 1 if meta else 8 if preset == "vcf" else 3
    cols = line.split(b"\t")
    walked = len(b"\t".join(cols[:want]))
    name = cols[0]
    if b"\r" in line[:walked]:
        return BAD, WHY_CR, name, 0, 0, walked
    if meta:
        return META, 0, name, 0, 0, walked
    if not line:
        return BAD, WHY_EMPTY, name, 0, 0, walked
    first = _pos(cols[1]) if len(cols) > 1 else None
    if preset == "bed":
        last = _pos(cols[2]) if len(cols) > 2 else None
        if first is None or last is None:
            return BAD, WHY_POS, name, 0, 0, walked
        return DATA, 0, name, first, max(last, first + 1), walked
    if not first:  # (no POS, or POS 0)
        return BAD, WHY_POS, name, 0, 0, walked
    beg = first - 1
    end = beg + max(1, len(cols[3]) if len(cols) > 3 else 0)
    if len(cols) > 7:
        for kv in cols[7].split(b";"):
            if kv.startswith(b"END=") and _pos(kv[4:]) is not None:
                end = max(end, _pos(kv[4:]))
    return DATA, 0, name, beg, end, walked


def rows(payload: bytes, preset: str, chunk=None):
    """the row of every line as the device states it with chunks of `chunk` bytes (None: one chunk) BEFORE the host settles any:
    dict(at, kind, why, name_len, beg, end, same, first, cut)"""
    out, n, prev_name = [], len(payload), None
    chunk = chunk or max(n, 1)
    for at, e in lines(payload):
        kind, why, name, beg, end, walked = key(payload[at:e], preset)
        lim = min(n, (at // chunk + 1) * chunk)
        cut = at + walked >= lim and lim < n  # the byte that ends the key columns is not in the chunk
        first = not out or out[-1]["at"] // chunk != at // chunk
        row = dict(at=at, kind=kind, why=why, name_len=len(name), beg=beg, end=end, same=int(name == prev_name), first=first, cut=cut)
        if cut:
            row.update(kind=CUT, why=0, name_len=0, beg=0, end=0)
        out.append(row)
        prev_name = name
    return out


def host_rows(payload: bytes, preset: str, chunk=None) -> int:
    """rows the entry point's host code has to settle: every chunk's first line and every cut line"""
    return sum(1 for r in rows(payload, preset, chunk) if r["first"] or r["cut"])


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def block_offsets(blocks: bytes):
    """compressed offset of every BGZF block of `blocks`, and behind them the offset of what follows (the end-of-file marker)"""
    at, out = 0, []
    while at < len(blocks):
        out.append(at)
        at += struct.unpack_from("<H", blocks, at + 16)[0] + 1
    return out + [at]


def tables(payload: bytes, preset: str, blocks: bytes):
    """-> (dict(names, bins {tid: {bin: [[v0, v1]]}}, linear [[..]], pseudo [(v0, v1, n)]), None) or (None, reason) for the file `blocks` + marker"""
    coff = block_offsets(blocks)

    def voff(t):
        return coff[-1] << 16 if t >= len(payload) else coff[t // SLICE] << 16 | t % SLICE
    names, bins, linear, pseudo = [], [], [], []
    prev, seen_data = None, False
    for at, e in lines(payload):
        kind, why, name, beg, end, _ = key(payload[at:e], preset)
        if kind == META:
            if seen_data:
                return None, "meta"
            prev = None
            continue
        if kind == BAD:
            return None, {WHY_EMPTY: "empty", WHY_CR: "cr", WHY_POS: "pos"}[why]
        if beg >= MAX_END or end > MAX_END:
            return None, "range"
        seen_data = True
        v0, v1 = voff(at), voff(e + 1)
        if prev is None or prev[0] != name:
            if name in names:
                return None, "contig"
            names.append(name)
            bins.append({})
            linear.append({})
            pseudo.append([v0, v1, 0])
        elif beg < prev[1]:
            return None, "order"
        ch = bins[-1].setdefault(reg2bin(beg, end), [])
        if ch and ch[-1][1] == v0:  # the record before this one is in the bin too: one chunk
            ch[-1][1] = v1
        else:
            ch.append([v0, v1])
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            linear[-1].setdefault(w, v0)
        pseudo[-1][1] = v1
        pseudo[-1][2] += 1
        prev = (name, beg, reg2bin(beg, end))
    lin = []
    for t in range(len(names)):
        k = max(linear[t]) + 1
        arr = [linear[t].get(w) for w in range(k)]
        for w in range(k - 2, -1, -1):
            if arr[w] is None:
                arr[w] = arr[w + 1]
        lin.append(arr)
    return dict(names=names, bins=bins, linear=lin, pseudo=[tuple(p) for p in pseudo]), None


def tbi_bytes(preset: str, T: dict) -> bytes:
    """the model's tables in the TBI layout (bins ascending, the pseudo-bin 37450 last, n_no_coor = 0)"""
    nm = b"".join(x + b"\0" for x in T["names"])
    out = bytearray(b"TBI\x01" + struct.pack("<i6ii", len(T["names"]), *HEADERS[preset], len(nm)) + nm)
    for t in range(len(T["names"])):
        out += struct.pack("<i", len(T["bins"][t]) + 1)
        for b in sorted(T["bins"][t]):
            out += struct.pack("<Ii", b, len(T["bins"][t][b]))
            for v0, v1 in T["bins"][t][b]:
                out += struct.pack("<QQ", v0, v1)
        v0, v1, count = T["pseudo"][t]
        out += struct.pack("<IiQQQQ", 37450, 2, v0, v1, count, 0)
        out += struct.pack("<i", len(T["linear"][t]))
        for v in T["linear"][t]:
            out += struct.pack("<Q", v)
    return bytes(out + struct.pack("<Q", 0))


def parse_tbi(raw: bytes):
    """an inflated .tbi -> dict(header (format, col_seq, col_beg, col_end, meta, skip), names, bins, linear, pseudo {tid: chunks})"""
    assert raw[:4] == b"TBI\x01"
    n_ref, *header, l_nm = struct.unpack_from("<8i", raw, 4)
    names = raw[36:36 + l_nm].split(b"\0")[:-1]
    assert len(names) == n_ref
    at, bins, linear, pseudo = 36 + l_nm, [], [], {}
    for t in range(n_ref):
        n_bin = struct.unpack_from("<i", raw, at)[0]
        at += 4
        mine = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", raw, at)
            at += 8
            chunks = [list(struct.unpack_from("<QQ", raw, at + 16 * k)) for k in range(n_chunk)]
            at += 16 * n_chunk
            if b == 37450:
                pseudo[t] = chunks
            else:
                assert b not in mine
                mine[b] = chunks
        bins.append(mine)
        n_intv = struct.unpack_from("<i", raw, at)[0]
        at += 4
        linear.append(list(struct.unpack_from("<%dQ" % n_intv, raw, at)))
        at += 8 * n_intv
    assert at == len(raw) or (at + 8 == len(raw) and raw[at:] == bytes(8))
    return dict(header=tuple(header), names=names, bins=bins, linear=linear, pseudo=pseudo)


def inflate(bgzf: bytes) -> bytes:
    """every BGZF block of a file inflated, CRC-32 and ISIZE checked; the end-of-file marker must be there"""
    at, out = 0, bytearray()
    assert bgzf.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    while at < len(bgzf):
        assert bgzf[at:at + 4] == b"\x1f\x8b\x08\x04"
        size = struct.unpack_from("<H", bgzf, at + 16)[0] + 1
        piece = zlib.decompress(bgzf[at + 18:at + size - 8], -15)
        assert struct.unpack_from("<II", bgzf, at + size - 8) == (zlib.crc32(piece) & 0xFFFFFFFF, len(piece))
        out += piece
        at += size
    return bytes(out)
