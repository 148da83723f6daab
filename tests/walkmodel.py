"""The device's BAM record walk, its mate-candidate filter and its extract (csrc/bamwalk_body.hpp, csrc/k_bamwalk.hip), stated in plain Python and
numpy from the SAM/BAM specification's record layout and the rules the kernels' comments cite.  It reads a file's bytes (struct, zlib) and the PLAN
the stage made (io_native.BamSource.select_kept: `.plan`) -- nothing of libunfazed_io's walk is called.  Test infrastructure: tests/walkcases.py is
the panel it is held to, tests/test_walk_cases.py holds it against the host's walk, tests/test_walk_cases_gpu.py holds the device to it."""
import os
import re
import struct
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the constants the panel is built against, restated with where they stand; constants_in_sources() reads them back from there
WIN = 16384         # csrc/k_bamwalk.hip: constexpr int WIN
WIN_RECS = 512      # csrc/k_bamwalk.hip: constexpr int WIN_RECS
EX_CAP = 768        # csrc/k_bamwalk.hip: constexpr int EX_CAP
FCAP = 1024         # csrc/bamwalk_body.hpp: constexpr int FCAP = 1024, RCAP = 256
RCAP = 256
SUB_EXTENT = 32768  # csrc/io_stage.cpp build_subtasks: const int32_t SUB_EXTENT
LSEQ_MAX = 65535    # csrc/bamwalk_body.hpp: ls > 0xFFFF; csrc/io_stage.cpp walk_task: lseq > 0xFFFF
INCOMPLETE, BAD = 1, 2  # include/uz_bamwalk.h: UZ_WALK_TASK_INCOMPLETE, UZ_WALK_TASK_BAD
AUX_MATE_SAME_TID, AUX_HAS_SA, AUX_DECODE_BAD, AUX_NO_SEQ = 1, 2, 4, 8  # include/uz_types.h: UZ_AUX_*
INT32_MAX = 2 ** 31 - 1
M64 = (1 << 64) - 1

FIELDS = ("voff", "src", "h1", "pos", "end", "tlen", "mpos", "mtid", "h2", "task", "flag", "l_seq", "n_cigar", "mapq", "l_name", "direct")


def constants_in_sources() -> dict:
    """the same constants as the sources state them today"""
    def grab(rel, pattern):
        m = re.search(pattern, open(os.path.join(ROOT, "unfazed_amd", "csrc", rel)).read())
        assert m, (rel, pattern)
        return int(m.group(1), 0)
    return dict(WIN=grab("k_bamwalk.hip", r"constexpr int WIN = (\d+);"), WIN_RECS=grab("k_bamwalk.hip", r"constexpr int WIN_RECS = (\d+);"),
                EX_CAP=grab("k_bamwalk.hip", r"constexpr int EX_CAP = (\d+);"), FCAP=grab("bamwalk_body.hpp", r"constexpr int FCAP = (\d+), RCAP = \d+;"),
                RCAP=grab("bamwalk_body.hpp", r"constexpr int FCAP = \d+, RCAP = (\d+);"), SUB_EXTENT=grab("io_stage.cpp", r"const int32_t SUB_EXTENT = (\d+);"),
                LSEQ_MAX=grab("bamwalk_body.hpp", r"ls < 0 \|\| ls > (0x[0-9A-Fa-f]+)"))


# ---------------------------------------------------------------------------------------------------------------- the file
def inflate_file(path):
    """-> (the inflated stream, per BGZF block: its offset in the file and its first byte in the stream [n + 1])"""
    raw = open(path, "rb").read()
    coff, at, parts, p, u = [], [], [], 0, 0
    while p < len(raw):
        xlen = struct.unpack_from("<H", raw, p + 10)[0]
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        data = zlib.decompress(raw[p + 12 + xlen: p + bsize - 8], -15)
        coff.append(p); at.append(u); parts.append(data)
        p += bsize; u += len(data)
    return b"".join(parts), np.array(coff, np.int64), np.array(at + [u], np.int64)


def header_of(data: bytes):
    """-> (contig names, contig lengths, where the first record starts)"""
    assert data[:4] == b"BAM\x01"
    off = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, off)[0]
    off += 4
    names, lens = [], []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", data, off)[0]
        names.append(data[off + 4: off + 4 + ln - 1].decode()); lens.append(struct.unpack_from("<i", data, off + 4 + ln)[0])
        off += 8 + ln
    return names, lens, off


def endpos(pos: int, flag: int, cigar) -> int:
    """htslib's bam_endpos: pos + 1 for an unmapped record or one without a CIGAR, else pos + max(1, the reference length of M, D, N, =, X)"""
    if (flag & 4) or len(cigar) == 0:
        return pos + 1
    rl = sum(int(w) >> 4 for w in cigar if (int(w) & 15) in (0, 2, 3, 7, 8))
    return pos + max(1, rl)


def parse_fixed(buf, at: int) -> dict:
    """the fixed part alone: what the walk's rules read before they know that the record holds what it declares"""
    ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, mref, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", buf, at + 4)
    return dict(at=at, bs=struct.unpack_from("<i", buf, at)[0], ref=ref, pos=pos, l_name=l_name, mapq=mapq, bin=bin_, n_cigar=n_cigar, flag=flag, l_seq=l_seq,
                mref=mref, mpos=mpos, tlen=tlen)


def parse_record(buf, at: int) -> dict:
    """the record whose block_size field stands at buf[at] (SAM spec 4.2), every field; `buf` indexable by int and slice -> bytes-like"""
    bs = struct.unpack_from("<i", buf, at)[0]
    p = at + 4
    ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, mref, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", buf, p)
    r = dict(at=at, bs=bs, ref=ref, pos=pos, l_name=l_name, mapq=mapq, bin=bin_, n_cigar=n_cigar, flag=flag, l_seq=l_seq, mref=mref, mpos=mpos, tlen=tlen)
    r["name"] = bytes(buf[p + 32: p + 32 + max(0, l_name - 1)])
    q = p + 32 + l_name
    r["cigar"] = np.frombuffer(bytes(buf[q: q + 4 * n_cigar]), "<u4")
    sq = q + 4 * n_cigar
    r["seq"] = bytes(buf[sq: sq + (l_seq + 1) // 2])
    r["qual"] = bytes(buf[sq + (l_seq + 1) // 2: sq + (l_seq + 1) // 2 + l_seq])
    r["tags"] = bytes(buf[sq + (l_seq + 1) // 2 + l_seq: p + bs])
    r["end"] = endpos(pos, flag, r["cigar"])
    return r


def records_of(data: bytes, first: int) -> list:
    out, at = [], first
    while at + 4 <= len(data):
        out.append(parse_record(data, at))
        at += 4 + out[-1]["bs"]
    assert at == len(data)
    return out


# ---------------------------------------------------------------------------------------------------------------- the name hashes
def hash1(name: bytes) -> int:
    """io_stage.cpp hash_name: 64-bit FNV-1a, then h ^= h >> 32; h *= 0x9E3779B97F4A7C15; h ^= h >> 29"""
    h = 1469598103934665603
    for b in name:
        h = ((h ^ b) * 1099511628211) & M64
    h ^= h >> 32
    h = (h * 0x9E3779B97F4A7C15) & M64
    h ^= h >> 29
    return h


def hash2(name: bytes) -> int:
    """include/uz_bamwalk.h uz_name_hash2: h = 0x9747B28C ^ n; per byte h ^= b; h *= 0x5BD1E995; h ^= h >> 15; then h ^= h >> 13; h *= ...; h ^= h >> 15"""
    m32 = 0xFFFFFFFF
    h = (0x9747B28C ^ len(name)) & m32
    for b in name:
        h ^= b
        h = (h * 0x5BD1E995) & m32
        h ^= h >> 15
    h ^= h >> 13
    h = (h * 0x5BD1E995) & m32
    h ^= h >> 15
    return h


# ---------------------------------------------------------------------------------------------------------------- the plan's bytes
class PlanBytes:
    """the gathered blocks of a plan, inflated back to back from the FILES (not from what the stage gathered): what the device holds in HBM"""

    def __init__(self, plan: dict, paths):
        self.plan = plan
        self.blk_at = np.asarray(plan["out_off"], np.int64)
        self.blk_coff = np.asarray(plan["blk_coff"], np.int64)
        files = plan.get("files")
        self.file_base = np.asarray(files["file_base"], np.int64) if files else np.array([0, 1 << 62], np.int64)
        self.ref_base = np.asarray(files["ref_base"], np.int64) if files else np.array([0, 0], np.int64)
        self.salt1 = [int(x) for x in files["salt1"]] if files else [0]
        self.salt2 = [int(x) for x in files["salt2"]] if files else [0]
        self.many = files is not None
        raws = [open(p, "rb").read() for p in paths]
        parts = []
        for k, coff in enumerate(self.blk_coff.tolist()):
            f = int(np.searchsorted(self.file_base, coff, side="right")) - 1
            raw, p = raws[f], coff - int(self.file_base[f])
            xlen = struct.unpack_from("<H", raw, p + 10)[0]
            bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
            data = zlib.decompress(raw[p + 12 + xlen: p + bsize - 8], -15)
            assert len(data) == int(self.blk_at[k + 1] - self.blk_at[k]), "the plan's block table has another size for block %d" % k
            parts.append(data)
        self.buf = b"".join(parts)
        self.n_ref_file = [len(header_of(inflate_file(p)[0])[0]) for p in paths]

    def file_of_task(self, t: int) -> int:
        """abi.hip task_files: the file of a task's first block (of the first span that has one)"""
        tc = self.plan["task"].reshape(-1, 10)[t]
        for sp in range(int(tc[2]), int(tc[3])):
            sc = self.plan["span"].reshape(-1, 6)[sp]
            if sc[4] < sc[5]:
                return int(np.searchsorted(self.file_base, self.blk_coff[int(sc[4])], side="right")) - 1
        return 0

    def voff_of(self, c: int, blk0: int, blk1: int) -> int:
        """the block that holds byte c: the first of the span's blocks whose end lies behind it (an empty block holds nothing; behind the last
        block: the last block)"""
        lo = blk0
        while lo + 1 < blk1 and self.blk_at[lo + 1] <= c:
            lo += 1
        return (int(self.blk_coff[lo]) << 16) | (c - int(self.blk_at[lo]))


def set_ref(r: int, ref_base: int, n_ref: int) -> int:
    """a refID in the numbering of a set of files (uz_bamwalk.h uz_walk_file): shifted when the file's header knows it, INT32_MAX when it does not"""
    return r if r < 0 else (r + ref_base if r < n_ref else INT32_MAX)


def walk_task(pb: PlanBytes, t: int, trace=None):
    """What walk task t emits, by the sequential rule -> (descriptors as dicts, flag).  Per span, from the span's start cursor: stop the span at
    voff >= span_end; stop the task at refID < 0, refID > tid or pos >= tb; skip other references; skip a record that lies wholly between two
    reach intervals.  The gathered bytes ending at or inside a record: INCOMPLETE; a block_size below 32, l_seq outside 0 .. 65535, l_name 0 or a
    record too small for what it declares: BAD.  trace: a list that takes (buffer offset, kind) of every record looked at."""
    plan, buf = pb.plan, pb.buf
    tid, tb, sp0, sp1, r0, r1, f0, f1, max_len, host = (int(x) for x in plan["task"].reshape(-1, 10)[t])
    reach = plan["reach"].reshape(-1, 2)[r0:r1].astype(np.int64)
    fetch = plan["fetch"].reshape(-1, 3)[f0:f1].astype(np.int64)
    f = pb.file_of_task(t) if pb.many else 0
    ref_base, n_ref = (int(pb.ref_base[f]), int(pb.ref_base[f + 1] - pb.ref_base[f])) if pb.many else (0, INT32_MAX)
    out, flag, stop = [], 0, False
    for sp in range(sp0, sp1):
        if stop or flag:
            break
        beg, span_end, cur, bend, blk0, blk1 = (int(x) for x in plan["span"].reshape(-1, 6)[sp])
        if blk0 >= blk1:
            stop = True
            break
        c = cur
        while True:
            if c + 4 > bend:
                flag |= INCOMPLETE
                break
            bs = struct.unpack_from("<i", buf, c)[0]
            if bs < 32:
                flag |= BAD
                break
            if c + 4 + bs > bend:
                flag |= INCOMPLETE
                break
            voff = pb.voff_of(c, blk0, blk1)
            if voff >= span_end:
                if trace is not None:
                    trace.append((c, "break"))
                break
            r = parse_fixed(buf, c)
            ref = set_ref(r["ref"], ref_base, n_ref) if pb.many else r["ref"]
            if ref != tid:
                if ref < 0 or ref > tid:
                    stop = True
                    if trace is not None:
                        trace.append((c, "stop"))
                    break
                if trace is not None:
                    trace.append((c, "skip"))
                c += 4 + bs
                continue
            if r["pos"] >= tb:
                stop = True
                if trace is not None:
                    trace.append((c, "stop"))
                break
            if r["l_seq"] < 0 or r["l_seq"] > LSEQ_MAX or r["l_name"] < 1 or 32 + r["l_name"] + 4 * r["n_cigar"] > bs:
                flag |= BAD
                if trace is not None:
                    trace.append((c, "bad"))
                break
            r = parse_record(buf, c)
            pos, end = r["pos"], r["end"]
            ahead = [k for k in range(len(reach)) if pos < reach[k][1]]  # the first interval that ends behind pos
            if ahead and end <= reach[ahead[0]][0]:
                if trace is not None:
                    trace.append((c, "gap"))
                c += 4 + bs
                continue
            if 32 + r["l_name"] + 4 * r["n_cigar"] + (r["l_seq"] + 1) // 2 + r["l_seq"] > bs:
                flag |= BAD
                if trace is not None:
                    trace.append((c, "bad"))
                break
            direct = bool(((fetch[:, 0] < end) & (fetch[:, 1] > pos)).any()) if len(fetch) else False
            mref = set_ref(r["mref"], ref_base, n_ref) if pb.many else r["mref"]
            out.append(dict(voff=voff, src=c + 4, h1=hash1(r["name"]) ^ pb.salt1[f], pos=pos, end=end, tlen=r["tlen"], mpos=r["mpos"], mtid=mref,
                            h2=hash2(r["name"]) ^ pb.salt2[f], task=t, flag=r["flag"], l_seq=r["l_seq"], n_cigar=r["n_cigar"], mapq=r["mapq"],
                            l_name=r["l_name"] - 1, direct=int(direct)))
            if trace is not None:
                trace.append((c, "emit"))
            c += 4 + bs
    return out, flag


def windows_of(pb: PlanBytes, t: int):
    """The LDS windows k_bam_walk stages for task t, as the header comment of the kernel describes them: a window starts at the cursor rounded down
    to 16 bytes and lists the records whose block_size field lies inside it (at most WIN_RECS); the next window starts at the first record not
    listed.  -> list of dict(w0, starts [buffer offsets of the listed records]) in order -- for the panel's shape assertions only (where a record
    lies in its window, which lane and batch hold it); the windows end with the span (a listed record may lie behind the one that ended the walk)."""
    plan, buf = pb.plan, pb.buf
    tc = plan["task"].reshape(-1, 10)[t]
    trace = []
    walk_task(pb, t, trace)
    last = {c: k for c, k in trace}
    wins = []
    for sp in range(int(tc[2]), int(tc[3])):
        beg, span_end, cur, bend, blk0, blk1 = (int(x) for x in plan["span"].reshape(-1, 6)[sp])
        if blk0 >= blk1:
            break
        c, done = cur, False
        while not done:
            w0 = c & ~15
            starts = []
            while len(starts) < WIN_RECS:
                if c + 4 > bend or c + 4 > w0 + WIN:
                    done = c + 4 > bend
                    break
                bs = struct.unpack_from("<i", buf, c)[0]
                if bs < 32 or c + 4 + bs > bend:
                    done = True
                    break
                starts.append(c)
                c += 4 + bs
            wins.append(dict(w0=w0, starts=starts, span=sp))
            if any(last.get(s) in ("break", "stop", "bad") for s in starts):
                done = True
        if any(last.get(s) in ("stop", "bad") for w in wins for s in w["starts"]):
            break
    return wins, last


def merge_subtasks(plan: dict, per_sub: list, flags: list):
    """the sub-tasks of a task of the stage joined (io_stage.cpp uz_stage_merge_subtasks): in order, without the records a later sub-task met again
    (they start in front of the stop of the one before); task = the stage's task; a flagged sub-task voids the whole task
    -> (descriptors, d_first [n_host + 1], flags [n_host])"""
    task = plan["task"].reshape(-1, 10)
    n_host = int(task[:, 9].max()) + 1 if len(task) else 0
    h_flags = [0] * n_host
    for u in range(len(task)):
        h_flags[int(task[u, 9])] |= flags[u]
    out, first = [], [0]
    for i in range(n_host):
        stop_before = -(2 ** 31)
        for u in range(len(task)):
            if int(task[u, 9]) != i:
                continue
            if not h_flags[i]:
                for d in per_sub[u]:
                    if d["pos"] < stop_before:
                        continue
                    out.append(dict(d, task=i))
            stop_before = int(task[u, 1])
        first.append(len(out))
    return out, first, h_flags


def mate_filter(desc: list, first: list) -> list:
    """keep a record if it is direct, or if h1 | 1 equals that of a direct record of the same task of the stage (the device's key merges two hashes
    that differ in bit 0 only: a record too many, never one too few) -> bool per descriptor"""
    keep = []
    for i in range(len(first) - 1):
        d = desc[first[i]: first[i + 1]]
        keys = {x["h1"] | 1 for x in d if x["direct"]}
        keep += [bool(x["direct"]) or (x["h1"] | 1) in keys for x in d]
    return keep


def walk_plan(plan: dict, paths):
    """the whole model of a plan -> dict(desc: every walked record per task of the stage, first, flags, keep: the filter's answer, sub_flags)"""
    pb = PlanBytes(plan, paths)
    nt = plan["task"].reshape(-1, 10).shape[0]
    per, fl = [], []
    for t in range(nt):
        d, f = walk_task(pb, t)
        per.append(d); fl.append(f)
    desc, first, h_flags = merge_subtasks(plan, per, fl)
    # (desc_all / first_all: what was walked until a flag was raised, for the comparison with a host that reads on where the device hands back)
    desc_all, first_all, _ = merge_subtasks(plan, per, [0] * nt)
    return dict(desc=desc, first=first, flags=h_flags, keep=mate_filter(desc, first), sub_flags=fl, pb=pb, desc_all=desc_all, first_all=first_all,
                keep_all=mate_filter(desc_all, first_all))


def desc_array(desc: list, dtype) -> np.ndarray:
    a = np.zeros(len(desc), dtype)
    for k in FIELDS:
        a[k] = np.array([d[k] for d in desc], dtype=a.dtype[k]) if desc else 0
    return a


# ---------------------------------------------------------------------------------------------------------------- the extract
def has_sa(tags: bytes) -> bool:
    """an SA tag among the optional fields (SAM spec 4.2.4: tag, type, value); a field of an unknown type, one cut off by the record's end or a B
    array with a negative count ends the search without one"""
    p, end = 0, len(tags)
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while p + 3 <= end:
        tag, typ = tags[p: p + 2], chr(tags[p + 2])
        p += 3
        if tag == b"SA":
            return True
        if typ in size:
            p += size[typ]
        elif typ in "ZH":
            z = tags.find(b"\0", p)
            if z < 0:
                return False
            p = z + 1
        elif typ == "B":
            if p + 5 > end or chr(tags[p]) not in size or chr(tags[p]) == "A":
                return False
            cnt = struct.unpack_from("<i", tags, p + 1)[0]
            if cnt < 0:
                return False
            p += 5 + cnt * size[chr(tags[p])]
        else:
            return False
    return False


def extract(buf, src: int, thr: int, bases: bool) -> dict:
    """what k_bam_extract writes for the kept record whose fixed part stands at buf[src]: the plain columns, the aux bits, every CIGAR word, the
    four-bit base codes as BAM packs them (pad nibble zero, the row padded with zeros to whole 32-base units) and one bit per base "quality below
    thr" (first quality 0xFF = no qualities: every bit set when thr > 0)"""
    r = parse_record(buf, src - 4)
    L, units = r["l_seq"], (r["l_seq"] + 31) >> 5
    noqual = L > 0 and r["qual"][0] == 0xFF
    aux = (AUX_MATE_SAME_TID if r["mref"] == r["ref"] else 0) | (AUX_HAS_SA if has_sa(r["tags"]) else 0) | \
        (AUX_DECODE_BAD if (r["n_cigar"] == 0 or L == 0 or noqual) else 0) | (0 if bases else AUX_NO_SEQ)
    row = bytearray(16 * units)
    row[: (L + 1) // 2] = r["seq"]
    if L & 1:
        row[(L + 1) // 2 - 1] &= 0xF0
    q = np.frombuffer(r["qual"], np.uint8).astype(np.int64)
    low = np.full(L, thr > 0, bool) if noqual else q < thr
    plane = np.zeros(units, np.uint32)
    for b in np.nonzero(low)[0].tolist():
        plane[b >> 5] |= np.uint32(1 << (b & 31))
    return dict(start=r["pos"], tlen=r["tlen"], flag=r["flag"], l_seq=L, n_cigar=r["n_cigar"], mapq=r["mapq"], aux=aux, cigar=r["cigar"].astype(np.uint32),
                row=bytes(row), plane=plane, name=r["name"], end=r["end"], low=low,
                codes=np.array([(r["seq"][b >> 1] >> (0 if b & 1 else 4)) & 15 for b in range(L)], np.uint8))


def codes_of(cols: dict, i: int) -> np.ndarray:
    """the four-bit base codes of record i of engine.reads_columns' answer, base by base"""
    L = int(cols["l_seq"][i])
    row = cols["seq4"][16 * int(cols["sq_off"][i]): 16 * int(cols["sq_off"][i]) + (L + 1) // 2]
    both = np.stack([row >> 4, row & 15], 1).reshape(-1)
    return both[:L].astype(np.uint8)


def row_of(cols: dict, i: int) -> bytes:
    """its whole base row: every unit, pad nibble and padding included"""
    units = (int(cols["l_seq"][i]) + 31) >> 5
    return cols["seq4"][16 * int(cols["sq_off"][i]): 16 * (int(cols["sq_off"][i]) + units)].tobytes()


def low_bits_of(cols: dict, i: int) -> np.ndarray:
    """its quality-plane row, one bool per base, and the units as they stand (the bits behind the last base included)"""
    L = int(cols["l_seq"][i])
    units = (L + 31) >> 5
    w = cols["qlow"][int(cols["qoff"][i]): int(cols["qoff"][i]) + units]
    bits = ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).reshape(-1).astype(bool)
    return bits[:L], w
