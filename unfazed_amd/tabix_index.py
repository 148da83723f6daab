"""The tabix index (.tbi) beside a BGZF outfile (outfile.write_output under UZ_OUT_INDEX=tbi): the file's layout, and the two routes to its tables.

  serialize(preset, tables)               the TBI bytes (SAM / tabix specification), not yet compressed
  from_device(data, dev)                  the tables of HipEngine.bgzf_deflate(..., index=...) (csrc/k_tbx.hip) -> tables
  build_host(data, block_sizes, preset)   the host route: the same rules as a plain loop over the text's lines; no device

A line's rules are stated in csrc/tbx_key.hpp and stated again here (line_key), per line and in plain Python:
  a line that begins with '#' is a meta line; an empty line, a '\\r' among a line's key columns, or a position that is not 1 to 10 digits is bad;
  VCF: beg = POS - 1, end = beg + max(1, len(REF)), raised to INFO/END where INFO holds "END=" + 1 to 10 digits at its start or behind a ';';
  BED: beg = column 2, end = max(column 3, beg + 1).
The table rules: the records of a contig stand together and ascend by beg; begin and end stay within 2^29 (the 14 / 5 binning scheme); no meta or
bad line stands among the data rows.  A text that breaks one has no index: (None, reason).  A record's chunk is [its line's virtual offset,
the next line's); a bin's chunks are its maximal runs of consecutive records; the 16 kb windows hold the smallest virtual offset of a record
that overlaps them, an empty one its successor's; the pseudo-bin 37450 holds (first offset, last end), (records, 0).

tables: dict(names=[bytes], n_intv=[n_refs], pseudo=[n_refs, 3] (v0, v1, records), runs=abi.TBX_RUN grouped by (tid, bin), within a bin in
file order, linear=the references' windows back to back)."""
import struct

import numpy as np

SLICE = 0xFF00
MAX_END = 1 << 29
PSEUDO_BIN = 37450
PRESETS = {"vcf": (2, 1, 2, 0), "bed": (0x10000, 1, 2, 3)}  # format, the columns of name / begin / end (meta '#', skip 0 in both)
TBX_RUN = np.dtype([("tid", np.uint32), ("bin", np.uint32), ("v0", np.uint64), ("v1", np.uint64)])  # (abi.TBX_RUN; this module needs no device)
REASONS = (  # (status bit of unfazed_hip.h UZ_TBX_S_*, what stderr says)
    (1, "a start below the previous record's on the same contig"),
    (2, "a begin or end beyond 2^29 (a .tbi's reach)"),
    (4, "a meta line among the data rows"),
    (8, "an empty line among the data rows"),
    (16, "a '\\r' in a line"),
    (32, "a position that is not 1 to 10 digits"),
    (64, "a line the device left unsettled"),
)
CONTIG_BACK = "a contig that comes back after another one"


def preset_of(data) -> str:
    """the preset a text asks for: "##fileformat=VCF" at byte 0 -> "vcf", anything else (our BED text starts with "#chrom") -> "bed\""""
    return "vcf" if bytes(data[:16]) == b"##fileformat=VCF" else "bed"


def reg2bin(beg: int, end: int) -> int:
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def _digits(data, a, b):
    """the 1 to 10 digits that fill data[a:b] -> their value, or None"""
    s = bytes(data[a:b])
    return int(s) if 1 <= len(s) <= 10 and s.isdigit() and s.isascii() else None


def line_key(data, at: int, n: int, preset: str):
    """the line at data[at] of a text of n bytes -> (kind, name, beg, end): kind "meta", "data", or the reason a bad line is bad.  Reads the key
    columns only"""
    meta = data[at:at + 1] == b"#"
    want = 1 if meta else 8 if preset == "vcf" else 3
    nl = data.find(b"\n", at, n)
    line_end = n if nl < 0 else nl
    ends, pos = [], at
    while len(ends) < want:
        tab = data.find(b"\t", pos, line_end)
        if tab < 0:
            ends.append(line_end)
            break
        ends.append(tab)
        pos = tab + 1
    name = bytes(data[at:ends[0]])
    if data.find(b"\r", at, ends[-1]) >= 0:
        return REASONS[4][1], name, 0, 0
    if meta:
        return "meta", name, 0, 0
    if line_end == at:
        return REASONS[3][1], name, 0, 0
    bad = (REASONS[5][1], name, 0, 0)
    first = _digits(data, ends[0] + 1, ends[1]) if len(ends) >= 2 else None
    if first is None:
        return bad
    if preset == "bed":
        last = _digits(data, ends[1] + 1, ends[2]) if len(ends) >= 3 else None
        if last is None:
            return bad
        return "data", name, first, max(last, first + 1)
    if first == 0:
        return bad
    beg = first - 1
    end = beg + max(1, ends[3] - ends[2] - 1 if len(ends) >= 4 else 0)
    if len(ends) == 8:
        a, b = ends[6] + 1, ends[7]
        c = a
        while c >= a:
            if data[c:c + 4] == b"END=" and c + 4 <= b:
                e = c + 4
                while e < b and e - (c + 4) <= 10 and data[e:e + 1].isdigit():
                    e += 1
                v = _digits(data, c + 4, e) if e == b or data[e:e + 1] == b";" else None
                if v is not None:
                    end = max(end, v)
            c = data.find(b";", c, b) + 1 or -1
    return "data", name, beg, end


def _tables(names, pseudo, runs, linear):
    runs = np.asarray(runs, TBX_RUN) if len(runs) else np.zeros(0, TBX_RUN)
    runs = runs[np.lexsort((runs["bin"], runs["tid"]))]  # (stable: a bin's chunks stay in file order)
    return dict(names=names, n_intv=np.asarray([len(x) for x in linear], np.int64), pseudo=np.asarray(pseudo, np.uint64).reshape(len(names), 3), runs=runs,
                linear=np.asarray([v for x in linear for v in x], np.uint64))


def build_host(data, block_sizes, preset: str):
    """data: the text (bytes-like); block_sizes: the compressed size of each of its BGZF blocks, one per SLICE bytes -> (tables, None), or
    (None, reason) for a text that has no index"""
    data = bytes(data) if not isinstance(data, (bytes, bytearray)) else data
    n = len(data)
    coff = np.concatenate([[0], np.cumsum(np.asarray(block_sizes, np.int64))])
    assert len(coff) - 1 == (n + SLICE - 1) // SLICE, "one block per slice of the text"
    eof_v = int(coff[-1]) << 16
    buf = np.frombuffer(data, np.uint8)
    starts = np.concatenate([[0], np.flatnonzero(buf == 10) + 1]) if n else np.zeros(0, np.int64)
    starts = starts[starts < n]
    voff = (coff[starts // SLICE] << 16) | (starts % SLICE)
    names, pseudo, runs, linear = [], [], [], []
    prev_name, prev_beg, prev_bin, seen_data = None, 0, -1, False
    for i, at in enumerate(starts.tolist()):
        kind, name, beg, end = line_key(data, at, n, preset)
        if kind == "meta":
            if seen_data:
                return None, REASONS[2][1]
            prev_name = None
            continue
        if kind != "data":
            return None, kind
        if beg >= MAX_END or end > MAX_END:
            return None, REASONS[1][1]
        v0, v1 = int(voff[i]), (int(voff[i + 1]) if i + 1 < len(starts) else eof_v)
        b = reg2bin(beg, end)
        if name != prev_name:
            if name in names:
                return None, CONTIG_BACK
            names.append(name)
            pseudo.append([v0, v1, 0])
            linear.append([])
            prev_bin = -1
        elif beg < prev_beg:
            return None, REASONS[0][1]
        seen_data = True
        if b != prev_bin:
            runs.append((len(names) - 1, b, v0, v1))
        else:
            runs[-1] = runs[-1][:3] + (v1,)
        pseudo[-1][1] = v1
        pseudo[-1][2] += 1
        lin = linear[-1]
        w1 = (end - 1) >> 14
        if len(lin) <= w1:
            lin.extend([0xFFFFFFFFFFFFFFFF] * (w1 + 1 - len(lin)))
        for w in range(beg >> 14, w1 + 1):
            if v0 < lin[w]:
                lin[w] = v0
        prev_name, prev_beg, prev_bin = name, beg, b
    for lin in linear:  # an empty window takes its successor's offset
        for w in range(len(lin) - 2, -1, -1):
            if lin[w] == 0xFFFFFFFFFFFFFFFF:
                lin[w] = lin[w + 1]
    return _tables(names, pseudo, runs, linear), None


def from_device(data, dev: dict):
    """dev: the last item of HipEngine.bgzf_deflate(data, ..., index=...) -> (tables, None), or (None, reason)"""
    for bit, text in REASONS:
        if dev["status"] & bit:
            return None, text
    refs = dev["refs"]
    view = memoryview(data)
    names = [bytes(view[int(o):int(o) + int(k)]) for o, k in zip(refs["name_off"], refs["name_len"])]
    if len(set(names)) != len(names):
        return None, CONTIG_BACK
    pseudo = np.stack([refs["v0"], refs["v1"], refs["n_rows"]], axis=1) if len(refs) else np.zeros((0, 3), np.uint64)
    return dict(names=names, n_intv=refs["n_intv"].astype(np.int64), pseudo=pseudo.astype(np.uint64), runs=dev["runs"], linear=dev["linear"]), None


def serialize(preset: str, tables: dict) -> bytes:
    """the .tbi's bytes before compression: magic, n_ref, format, col_seq, col_beg, col_end, meta, skip, l_nm, names; per reference its bins
    (ascending, the pseudo-bin last) with their chunks, and its linear index; n_no_coor = 0"""
    fmt, c_seq, c_beg, c_end = PRESETS[preset]
    names = tables["names"]
    nm = b"".join(x + b"\0" for x in names)
    out = [b"TBI\x01", struct.pack("<8i", len(names), fmt, c_seq, c_beg, c_end, ord("#"), 0, len(nm)), nm]
    runs, linear, lin_at = tables["runs"], np.ascontiguousarray(tables["linear"], "<u8"), 0
    ref_at = np.searchsorted(runs["tid"], np.arange(len(names) + 1))  # (grouped by tid first)
    for t in range(len(names)):
        mine = runs[ref_at[t]:ref_at[t + 1]]
        cut = np.concatenate([[0], np.flatnonzero(np.diff(mine["bin"].astype(np.int64))) + 1, [len(mine)]]) if len(mine) else np.zeros(1, np.int64)
        pairs = np.ascontiguousarray(np.stack([mine["v0"], mine["v1"]], axis=1), "<u8")
        out.append(struct.pack("<i", len(cut) - 1 + 1))
        for a, b in zip(cut[:-1].tolist(), cut[1:].tolist()):
            out.append(struct.pack("<Ii", int(mine["bin"][a]), b - a))
            out.append(pairs[a:b].tobytes())
        v0, v1, rows = (int(x) for x in tables["pseudo"][t])
        out.append(struct.pack("<Ii4Q", PSEUDO_BIN, 2, v0, v1, rows, 0))
        k = int(tables["n_intv"][t])
        out.append(struct.pack("<i", k))
        out.append(linear[lin_at:lin_at + k].tobytes())
        lin_at += k
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def block_sizes(blocks) -> list:
    """the sizes of BGZF blocks that stand back to back, from their BSIZE fields"""
    view, at, out = memoryview(blocks), 0, []
    while at < len(view):
        size = (view[at + 16] | view[at + 17] << 8) + 1
        out.append(size)
        at += size
    return out
