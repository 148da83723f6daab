"""BAM files built byte by byte for the tests of the device's record walk and extract (csrc/bamwalk_body.hpp, csrc/k_bamwalk.hip), in the pattern of
tests/headfiles.py: a record maker that takes every field, a file writer whose BGZF block cuts, empty blocks and compression level are the caller's,
and the PANEL -- named cases, each built against one constant or one rule's edge of the walk (tests/walkmodel.py restates the constants with where
they stand).  A case carries its file(s), its fetches, the UZ_STAGE_SLACK it needs, and `shape`: the assertion, from the plan and the file, that the
branch it aims at was reached.  Test infrastructure."""
import struct

import numpy as np

from headfiles import bgzf_block, read_blocks
import walkmodel as wm

BLOCK_MAX = 65280  # payload of a BGZF block as htslib cuts it; a stored (level 0) block of this size still fits the 16-bit BSIZE
CONTIGS = (("c0", 1 << 28), ("c1", 1 << 28), ("c2", 1 << 28))
OPS = "MIDNSHP=X"


def cig(*ops) -> list:
    """cig((5, "M"), (2, "D")) -> CIGAR words"""
    return [(n << 4) | OPS.index(op) for n, op in ops]


def pack_seq(codes) -> bytes:
    codes = list(codes) + [0]
    return bytes((codes[2 * k] << 4) | codes[2 * k + 1] for k in range((len(codes) - 1 + 1) // 2))


def rec(ref=0, pos=0, name=b"r", mapq=30, bin_=4680, cigar=(), flag=0, l_seq=0, mref=-1, mpos=-1, tlen=0, seq=None, qual=None, aux=b"", l_name=None, n_cigar=None,
        block_size=None, name_bytes=None) -> bytes:
    """one alignment record, every field the caller's (SAM spec 4.2).  name: without the terminator (name_bytes: the bytes as they stand instead);
    l_name / n_cigar / l_seq: what the fixed part DECLARES -- by default what the variable part holds; seq: packed bytes, qual: bytes (by default
    (l_seq + 1) / 2 and l_seq of them, made from pos); block_size: what the size field declares when it lies"""
    nb = name + b"\0" if name_bytes is None else name_bytes
    cw = b"".join(struct.pack("<I", c) for c in cigar)
    n_real = max(0, l_seq)
    if seq is None:
        seq = pack_seq([1 << ((pos + k) & 3) for k in range(n_real)]) if 0 < n_real <= 70000 else b""
    if qual is None:
        qual = bytes(30 + (pos + k) % 7 for k in range(n_real)) if 0 < n_real <= 70000 else b""
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(nb) if l_name is None else l_name, mapq, bin_, len(cigar) if n_cigar is None else n_cigar, flag, l_seq, mref, mpos,
                       tlen) + nb + cw + seq + qual + aux
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def read(pos, L=50, name=None, ref=0, flag=0, **kw) -> bytes:
    """an ordinary mapped read: L bases, one M"""
    return rec(ref=ref, pos=pos, name=name if name is not None else b"q%07d" % pos, cigar=cig((L, "M")), l_seq=L, flag=flag, **kw)


def tiny(pos, ref=0) -> bytes:
    """the smallest record: 37 bytes with its size field (l_name 1: the terminator alone; no CIGAR, no bases)"""
    return rec(ref=ref, pos=pos, name=b"")


def filler(pos, size, ref=0, name=b"f") -> bytes:
    """a record of exactly `size` bytes with its size field (>= 38), no CIGAR, no bases: its room is an aux Z field"""
    assert size >= 36 + len(name) + 1 + 4, size
    n = size - (36 + len(name) + 1) - 4
    return rec(ref=ref, pos=pos, name=name, aux=b"XZZ" + b"x" * n + b"\0")


def header_bytes(contigs) -> bytes:
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in contigs)
    out = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(contigs)))
    for name, length in contigs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    return bytes(out)


def write_bam(path, contigs, records, ends=(), empty_at=(), level=6, header_block=True):
    """-> dict(rec_off: where every record starts in the inflated stream, header: the header's bytes, total: the stream's, ends: where blocks end).
    ends: offsets of the inflated stream at which a BGZF block ends (further cuts keep every block within BLOCK_MAX); header_block: the header in a
    block of its own, so that offsets counted from the first record are offsets into the blocks a walk gathers; empty_at: stream offsets in front of
    which an empty block stands (each becomes a cut); a negative `ends` / `empty_at` entry e counts from the first record: -e - 1 bytes behind it"""
    hdr = header_bytes(contigs)
    out = bytearray(hdr)
    rec_off = []
    for r in records:
        rec_off.append(len(out))
        out += r
    fix = lambda e: e if e >= 0 else len(hdr) + (-e - 1)  # noqa: E731
    empty_at = sorted(fix(e) for e in empty_at)
    cuts = set(fix(e) for e in ends) | set(empty_at) | {len(out)} | ({len(hdr)} if header_block else set())
    cuts = sorted(c for c in cuts if 0 < c <= len(out))
    all_ends, at = [], 0
    for c in cuts:
        while c - at > BLOCK_MAX:
            at += BLOCK_MAX
            all_ends.append(at)
        all_ends.append(c)
        at = c
    with open(path, "wb") as fh:
        at = 0
        for e in all_ends:
            if at in empty_at:
                fh.write(bgzf_block(b"", level))
            fh.write(bgzf_block(bytes(out[at:e]), level))
            at = e
        fh.write(bgzf_block(b""))
    return dict(rec_off=rec_off, header=len(hdr), total=len(out), ends=all_ends)


class Case:
    """one named case of the panel.  records: the file's; twin: the records of its SOUND twin when `records` hold a malformed one (same lengths:
    both are written with stored blocks and the twin's index serves both); fetches: (tid, lo, hi, extra); flags: {task of the stage: bit} the model
    must give -- empty for every sound case; raises: what the host says of the malformed record -- raises_at "walk": its walk does; "extract": its
    walk keeps the record's bytes as they are (the descriptor route's keep_raw), the one-pass stage's extract refuses them, as k_bam_extract does; thr: the thresholds the table is built at;
    shape(ctx): asserts from the plan and the file that the aimed-at branch is reached -- ctx: dict(plan, pb: walkmodel.PlanBytes, model, info:
    write_bam's answer, case)"""

    def __init__(self, name, records, fetches, shape, contigs=CONTIGS, ends=(), empty_at=(), level=6, slack=None, flags=None, twin=None, raises=None, thr=(20,),
                 note="", raises_at="walk"):
        self.name, self.records, self.fetches, self.shape, self.contigs = name, records, fetches, shape, contigs
        self.ends, self.empty_at, self.level, self.slack, self.flags, self.twin, self.raises, self.thr, self.note, self.raises_at = ends, empty_at, level, slack, flags or {}, twin, raises, thr, note, raises_at
        if twin is not None:
            assert [len(a) for a in twin] == [len(b) for b in records]
            self.level = 0

    def write(self, folder) -> dict:
        """the case's file (and index) into `folder` -> dict(path, info)"""
        from filesio import write_bai
        path = str(folder / (self.name + ".bam"))
        info = write_bam(path, self.contigs, self.records, self.ends, self.empty_at, self.level)
        if self.twin is None:
            write_bai(path)
        else:
            sound = str(folder / (self.name + ".sound.bam"))
            write_bam(sound, self.contigs, self.twin, self.ends, self.empty_at, self.level)
            write_bai(sound, path + ".bai")
            a, b = read_blocks(path), read_blocks(sound)
            assert all(np.array_equal(a[k], b[k]) for k in ("off", "csize", "isize")), "the twins' block tables differ"
        return dict(path=path, info=info)

    def fetch_arrays(self):
        f = np.array(sorted(self.fetches), np.int64).reshape(-1, 4)
        return f[:, 0].astype(np.int32), f[:, 1].astype(np.int32), f[:, 2].astype(np.int32), f[:, 3].astype(np.uint16)


def one_base(tid, points):
    return [(tid, int(p), int(p) + 1, 0) for p in points]


# ---------------------------------------------------------------------------------------------------------------- shape helpers
def rec_buf(ctx, k: int) -> int:
    """buffer offset (in the plan's gathered bytes) of record k of the file: the first gathered block is the one of the first record"""
    info, pb = ctx["info"], ctx["pb"]
    first_blk = ctx["file_blocks"]["off"].tolist().index(int(pb.blk_coff[0]))
    return info["rec_off"][k] - int(ctx["file_at"][first_blk])


def where(ctx, k: int, task: int = 0):
    """(window number, offset in the window, index in the window's list) of record k in the windows of walk task `task`"""
    c = rec_buf(ctx, k)
    wins, last = wm.windows_of(ctx["pb"], task)
    for wi, w in enumerate(wins):
        if c in w["starts"]:
            return wi, c - w["w0"], w["starts"].index(c), last.get(c), wins
    raise AssertionError("record %d is in no window of task %d" % (k, task))


PANEL = []


def case(fn):
    PANEL.append(fn)
    return fn


# ---------------------------------------------------------------------------------------------------------------- the panel
READ50 = len(read(0, 50))  # 124 bytes
TB_FETCH = [(0, 2000, 2001, 0)]  # with the default slack of 1000 (io_stage.cpp REACH_SLACK_DEFAULT): reach [1000, 3001), tb = 3001
STOP_POS = 12000  # behind every reach interval of the small cases and inside the same 16 kb bin: the stage gathers these records with the others


def size_of(recs) -> int:
    return sum(len(r) for r in recs)


def pad_to(recs, off, pos, name=b"f"):
    """a filler behind `recs` so that the next record starts `off` bytes behind the first record"""
    recs.append(filler(pos, off - size_of(recs), name=name))


def tail(n=3, pos=STOP_POS, ref=0):
    """records behind every fetch: the walk of a sound case ends at one of them (pos >= tb), not at the end of its gathered bytes"""
    return [read(pos + 100 * k, 40, ref=ref) for k in range(n)]


def patch(r: bytes, off: int, fmt: str, val) -> bytes:
    """the same record with one field of its fixed part overwritten (off counts from the size field: 0 block_size, 12 l_name, 16 n_cigar, 20 l_seq)"""
    b = bytearray(r)
    struct.pack_into(fmt, b, off, val)
    return bytes(b)


def task_of(ctx, t=0):
    return [int(x) for x in ctx["plan"]["task"].reshape(-1, 10)[t]]


def is_direct(ctx, k: int) -> bool:
    """does the model call record k of the file direct (a fetch returns it: it passes the filter and is compared on the device)"""
    return any(d["src"] - 4 == rec_buf(ctx, k) and d["direct"] for d in ctx["model"]["desc_all"])


def kinds(ctx, t=0):
    """{record number in the file: what the model's walk of task t did with it}"""
    trace = []
    wm.walk_task(ctx["pb"], t, trace)
    by_buf = {rec_buf(ctx, k): k for k in range(len(ctx["info"]["rec_off"]))}
    return {by_buf[c]: kind for c, kind in trace}


def one_task(ctx):
    assert ctx["plan"]["task"].reshape(-1, 10).shape[0] == 1, "the case is built for one walk task"
    sc = ctx["plan"]["span"].reshape(-1, 6)[0]
    assert sc[2] == 0, "the walk does not start at the first record"


def _many_starts(name, size, more_than):
    def build():
        recs = [tiny(1000 + k) if size == 37 else filler(1000 + k, size, name=b"f%04d" % k) for k in range(1000 if size == 37 else 400)] + tail()

        def shape(ctx):
            one_task(ctx)
            wins, _ = wm.windows_of(ctx["pb"], 0)
            assert max(len(w["starts"]) for w in wins) > more_than and len(wins) >= 2
            assert all(len(w["starts"]) <= wm.WIN_RECS for w in wins)
        return Case(name, recs, [(0, 1100, 1300, 0)], shape, note="WIN / record size starts in one window: several 64-lane batches")
    build.__name__ = name
    return case(build)


_many_starts("starts_65", 200, 64)     # WIN = 16384 / 200: 82 starts, two batches
_many_starts("starts_129", 100, 128)   # 164 starts, three batches
_many_starts("starts_440", 37, 439)    # the smallest record (l_name 1, no CIGAR, l_seq 0): 443 starts, seven batches, below WIN_RECS = 512


def _win_place(name, at=None, end_at=None, want_win=0, note=""):
    def build():
        target = read(1990, 50)
        recs = [read(1000, 50)]
        pad_to(recs, at if at is not None else end_at - len(target), 1001)
        k = len(recs)
        recs += [target] + [read(1991 + i // 3, 50, name=b"w%03d" % i) for i in range(20)] + tail()

        def shape(ctx):
            one_task(ctx)
            wi, off, idx, kind, wins = where(ctx, k)
            assert kind == "emit" and wi == want_win and is_direct(ctx, k)
            if end_at is not None:
                assert off + len(target) == end_at and wi == 0  # WIN: ends on the window's last byte / one byte over
            elif want_win == 0:
                assert off + 4 == wm.WIN  # its size field ends on the window's edge: listed, read from memory
            else:
                assert wins[1]["w0"] == wm.WIN - 16 and off == at - (wm.WIN - 16) and idx == 0  # not listed in window 0: the next one restarts 16-byte aligned in front of it
        return Case(name, recs, TB_FETCH, shape, note=note)
    build.__name__ = name
    return case(build)


_win_place("win_ends_on_last_byte", end_at=wm.WIN)
_win_place("win_ends_one_byte_over", end_at=wm.WIN + 1)
_win_place("win_size_field_on_edge", at=wm.WIN - 4)
_win_place("win_restart_minus_3", at=wm.WIN - 3, want_win=1)
_win_place("win_restart_minus_1", at=wm.WIN - 1, want_win=1)


@case
def win_long_record():
    big = rec(pos=1010, name=b"big", cigar=cig(*[(10, "M")] * 1000), l_seq=10000, mref=0, mpos=1010)
    recs = [read(1000, 50), read(1005, 50), big] + [read(1960 + i, 50) for i in range(30)] + tail()

    def shape(ctx):
        one_task(ctx)
        assert len(big) > wm.WIN  # longer than a window: never whole in LDS
        wi, off, idx, kind, wins = where(ctx, 2)
        assert kind == "emit" and is_direct(ctx, 2) and wi == 0 and off + len(big) > wm.WIN and len(wins) >= 2  # listed in window 0, read from memory; the next window starts behind it
    return Case("win_long_record", recs, TB_FETCH, shape)


def _exact_windows(n):
    def build():
        recs = [read(1955 + k // 8, 50, name=b"x%04d" % k) for k in range(60 * n)]
        stop = read(STOP_POS, 40)
        pad_to(recs, n * wm.WIN - len(stop), 2990)
        recs.append(stop)

        def shape(ctx):
            one_task(ctx)
            sc = ctx["plan"]["span"].reshape(-1, 6)[0]
            assert sc[3] - sc[2] == n * wm.WIN  # the task's bytes: exactly n windows
            assert kinds(ctx)[len(recs) - 1] == "stop"
        return Case("bytes_exactly_%d_windows" % n, recs, TB_FETCH, shape)
    build.__name__ = "bytes_exactly_%d_windows" % n
    return case(build)


_exact_windows(1)
_exact_windows(2)


# ---- lanes
def _stop_lane(j):
    def build():
        recs = [read(1955 + k // 4, 50, name=b"l%03d" % k) for k in range(j)]
        if j == 0:  # lane 0 of the SECOND window: the first record window 0 does not list
            recs = [read(1990, 50)]
            pad_to(recs, wm.WIN - 2, 1991)
        k = len(recs)
        recs += [read(5000, 50)] + [read(5001 + i, 50) for i in range(10)] + tail()

        def shape(ctx):
            one_task(ctx)
            wi, off, idx, kind, wins = where(ctx, k)
            assert kind == "stop" and idx == j and wi == (1 if j == 0 else 0)  # lane idx % 64 of batch idx / 64
            assert len(ctx["model"]["desc"]) == (2 if j == 0 else j)
        return Case("stop_in_lane_%d" % j, recs, TB_FETCH, shape)
    build.__name__ = "stop_in_lane_%d" % j
    return case(build)


for _j in (0, 1, 63, 64):
    _stop_lane(_j)

MSG_NAME = "alignment record overruns its block"
MSG_SIZE = "bad alignment record at virtual offset"
MSG_LSEQ = "record too long for the 16-bit length columns"


@case
def stop_then_malformed_same_batch():
    sound = [read(1960 + k, 50) for k in range(5)] + [read(5000, 50), read(5001, 50)] + [read(5002 + i, 50) for i in range(5)] + tail()
    recs = list(sound)
    recs[6] = patch(sound[6], 8, "<i", 1970)  # (in reach and fetched, had the walk come to it)
    recs[6] = patch(recs[6], 12, "<B", 0)     # l_name 0

    def shape(ctx):
        one_task(ctx)
        a, b = where(ctx, 5), where(ctx, 6)
        assert a[3] == "stop" and b[3] is None and a[0] == b[0] and a[2] // 64 == b[2] // 64 and b[2] == a[2] + 1
    return Case("stop_then_malformed_same_batch", recs, TB_FETCH, shape, twin=sound)


@case
def stop_then_bad_size_in_a_later_batch():
    sound = [read(1960 + k, 50) for k in range(3)] + [read(5000, 50)] + [read(5001 + i, 50) for i in range(80)] + tail()
    recs = list(sound)
    recs[74] = patch(sound[74], 0, "<i", 31)  # the chain of window 0 ends here in state "not a record" -- behind a stop in batch 0

    def shape(ctx):
        one_task(ctx)
        a = where(ctx, 3)
        assert a[3] == "stop" and a[2] == 3 and a[0] == 0
        assert rec_buf(ctx, 74) + 4 <= wm.WIN and 74 // 64 == 1  # in window 0, second batch
    return Case("stop_then_bad_size_in_a_later_batch", recs, TB_FETCH, shape, twin=sound)


@case
def malformed_then_stop_same_batch():
    sound = [read(1960 + k, 50) for k in range(5)] + [read(1970, 50), read(5000, 50)] + [read(5002 + i, 50) for i in range(5)] + tail()
    recs = list(sound)
    recs[5] = patch(sound[5], 12, "<B", 0)

    def shape(ctx):
        one_task(ctx)
        assert kinds(ctx)[5] == "bad" and 6 not in kinds(ctx)
    return Case("malformed_then_stop_same_batch", recs, TB_FETCH, shape, twin=sound, flags={0: wm.BAD}, raises=MSG_NAME)


@case
def break_then_a_further_span():
    # slack 100, one fetch at 18000: reach [17900, 18101) in the 16 kb bin 4682.  The first record starts at 100 and ends at 20050 (bin 585: it overlaps the
    # reach); the 700 records behind it lie in bin 4681, which the reach does not touch: the index gives the task two chunks with 86 KB between them
    long_n = rec(pos=100, name=b"long_n", cigar=cig((50, "M"), (19850, "N"), (50, "M")), l_seq=100)
    recs = [long_n] + [read(200 + 20 * k, 50) for k in range(700)] + [read(17000 + 10 * k, 50) for k in range(200)] + tail(pos=21000)

    def shape(ctx):
        task = ctx["plan"]["task"].reshape(-1, 10)
        assert task.shape[0] == 1 and task[0, 3] - task[0, 2] == 2, "two spans in one walk task"
        trace = []
        wm.walk_task(ctx["pb"], 0, trace)
        assert [k for _, k in trace][:2] == ["emit", "break"] and trace[-1][1] == "stop"  # voff == span_end behind the first record, then the second span
        assert len(ctx["model"]["desc"]) > 20 and ctx["model"]["desc"][0]["direct"] == 1
    return Case("break_then_a_further_span", recs, one_base(0, [18000]), shape, slack=100)


# ---- blocks
@case
def empty_block_mid_span():
    recs = [read(1955 + k // 4, 50, name=b"b%07d" % k) for k in range(100)] + tail()
    cut_a, cut_b = 30 * READ50, 60 * READ50 + 50  # an empty block where record 30 starts, another inside record 60

    def shape(ctx):
        one_task(ctx)
        at = ctx["pb"].blk_at
        empties = [k for k in range(len(at) - 1) if at[k] == at[k + 1] and k + 2 < len(at)]
        assert len(empties) >= 2 and rec_buf(ctx, 30) == at[empties[0]] and at[empties[1]] == rec_buf(ctx, 60) + 50
        d = [x for x in ctx["model"]["desc"] if x["src"] - 4 == rec_buf(ctx, 30)][0]
        assert d["voff"] & 0xFFFF == 0 and (d["voff"] >> 16) == ctx["pb"].blk_coff[empties[0] + 1]  # the block BEHIND the empty one holds it
    return Case("empty_block_mid_span", recs, TB_FETCH, shape, ends=[-(cut_a + 1), -(cut_b + 1)], empty_at=[-(cut_a + 1), -(cut_b + 1)])


@case
def record_on_a_blocks_first_byte_and_size_field_straddling():
    recs = [read(1955 + k // 4, 50, name=b"b%07d" % k) for k in range(100)] + tail()
    ends = [10 * READ50, 20 * READ50 + 1, 30 * READ50 + 2, 40 * READ50 + 3, 50 * READ50 + 100, 50 * READ50 + 110]  # record 50 lies in three blocks

    def shape(ctx):
        one_task(ctx)
        at = set(ctx["pb"].blk_at.tolist())
        assert rec_buf(ctx, 10) in at
        for k, o in ((20, 1), (30, 2), (40, 3)):
            assert rec_buf(ctx, k) + o in at  # its size field lies in two blocks
        assert rec_buf(ctx, 50) + 100 in at and rec_buf(ctx, 50) + 110 in at
        assert sorted(kinds(ctx).values()).count("emit") == 100
    return Case("record_on_a_blocks_first_byte_and_size_field_straddling", recs, TB_FETCH, shape, ends=[-(e + 1) for e in ends])


@case
def the_files_last_record_fetched():
    recs = [read(1955 + k // 4, 50, name=b"e%07d" % k) for k in range(100)]

    def shape(ctx):
        one_task(ctx)
        sc = ctx["plan"]["span"].reshape(-1, 6)[0]
        assert sc[3] == size_of(recs)  # the gathered bytes end behind the last record: the walk cannot know that nothing follows
    return Case("the_files_last_record_fetched", recs, TB_FETCH, shape, flags={0: wm.INCOMPLETE},
                note="INCOMPLETE: the gathered bytes end where the next size field would stand; the host walks the task (its stream sees the end of the file)")


# ---- the rules at equality (UZ_STAGE_SLACK=100: a reach interval is [lo - 100, hi + 100))
def short(pos, L, name=None, **kw):
    return read(pos, L, name=name if name is not None else b"s%06d" % pos, **kw)


def edge(pos, L):
    """the records of a rule's edge carry ONE name: those no fetch returns share it with one that a fetch does return, so the filter hands them over
    and the device's answer for them is compared"""
    return read(pos, L, name=b"edge")


@case
def pos_at_tb():
    recs = [edge(1960, 50), edge(2100, 10), edge(2101, 10), edge(2102, 10)] + tail()

    def shape(ctx):
        one_task(ctx)
        assert task_of(ctx)[1] == 2101  # tb
        assert [kinds(ctx).get(k) for k in range(4)] == ["emit", "emit", "stop", None]  # pos == tb - 1, pos == tb
    return Case("pos_at_tb", recs, TB_FETCH, shape, slack=100)


@case
def gaps_between_reach_intervals():
    recs = [edge(1950, 60), edge(2100, 10), edge(2101, 10), edge(2500, 400), edge(2501, 400), edge(2950, 60)] + tail()

    def shape(ctx):
        one_task(ctx)
        assert ctx["plan"]["reach"].reshape(-1, 2).tolist() == [[1900, 2101], [2900, 3101]]
        # pos == r_b - 1: in the interval; pos == r_b: behind it; end == r_a: in front of the next; end == r_a + 1: inside it
        assert [kinds(ctx).get(k) for k in range(6)] == ["emit", "emit", "gap", "gap", "emit", "emit"]
    return Case("gaps_between_reach_intervals", recs, one_base(0, [2000, 3000]), shape, slack=100)


@case
def fetch_edges():
    recs = [edge(1990, 10), edge(1991, 10), edge(2009, 10), edge(2010, 10)] + tail()

    def shape(ctx):
        one_task(ctx)
        assert ctx["plan"]["fetch"].reshape(-1, 3)[:, :2].tolist() == [[2000, 2010]]
        # lo == end, lo == end - 1, hi == pos + 1, hi == pos
        assert [d["direct"] for d in ctx["model"]["desc"]] == [0, 1, 1, 0]
    return Case("fetch_edges", recs, [(0, 2000, 2010, 0)], shape, slack=100)


@case
def wide_fetch_among_one_base_fetches():
    pts = [3000 + 20 * k for k in range(50)]
    recs = [edge(1500 + 25 * k, 30) for k in range(240)] + tail()

    def shape(ctx):
        one_task(ctx)
        assert task_of(ctx)[8] == 5000  # max_len: the search for the first fetch that can return a record starts at pos - max_len
        far = [d for d in ctx["model"]["desc"] if d["pos"] > pts[-1] + 1 and d["pos"] < 7000]
        assert len(far) > 50 and all(d["direct"] for d in far)  # returned by the wide fetch alone, whose lo lies up to 5000 in front of them
        assert any(not d["direct"] for d in ctx["model"]["desc"])
    return Case("wide_fetch_among_one_base_fetches", recs, [(0, 2000, 7000, 0)] + one_base(0, pts), shape)


@case
def unmapped_with_its_mate_and_cigar_ops():
    every_op = cig((5, "M"), (2, "I"), (3, "D"), (100, "N"), (4, "S"), (1, "H"), (1, "P"), (6, "="), (7, "X"))  # reference length 5 + 3 + 100 + 6 + 7
    recs = [rec(pos=1880, name=b"skipN", cigar=cig((5, "M"), (115, "N"), (5, "M")), l_seq=10),
            read(1995, 50, name=b"pair", flag=0x1 | 0x8 | 0x40, mref=0, mpos=1995),
            rec(pos=1995, name=b"pair", flag=0x1 | 0x4 | 0x80, l_seq=50, mref=0, mpos=1995),  # unmapped, placed with its mate
            rec(pos=1996, name=b"ops", cigar=every_op, l_seq=24),
            rec(pos=2000, name=b"clip", cigar=cig((10, "S")), l_seq=10),  # a CIGAR whose reference length is 0
            rec(pos=2000, name=b"ins", cigar=cig((5, "I")), l_seq=5)] + tail()

    def shape(ctx):
        one_task(ctx)
        by = {d["pos"]: d for d in ctx["model"]["desc"]}
        d = ctx["model"]["desc"]
        assert [(x["pos"], x["end"]) for x in d] == [(1880, 2005), (1995, 2045), (1995, 1996), (1996, 2117), (2000, 2001), (2000, 2001)]
        assert d[0]["direct"] == 1  # only through its N: end == 2005 > 2000 (and in reach only through it: 1880 + 10 < 1900)
        assert d[2]["flag"] & 4 and by[1996]["n_cigar"] == 9
    return Case("unmapped_with_its_mate_and_cigar_ops", recs, TB_FETCH, shape, slack=100)


@case
def unplaced_record_mid_file():
    recs = [short(1960 + k, 50) for k in range(5)] + [rec(ref=-1, pos=-1, name=b"lost", flag=4, l_seq=20)] + [short(1970 + k, 50) for k in range(5)] + tail()

    def shape(ctx):
        one_task(ctx)
        assert kinds(ctx)[5] == "stop" and len(ctx["model"]["desc"]) == 5  # refID < 0 ends the walk: the records behind it lie in reach and are not met
    return Case("unplaced_record_mid_file", recs, TB_FETCH, shape)


# ---- caps
def _fetch_cap(n):
    def build():
        pts = [2000 + 20 * k for k in range(n)]
        recs = [short(1000 + 15 * k, 30) for k in range((20 * n + 2900) // 15)] + tail(pos=2000 + 20 * n + 5000)

        def shape(ctx):
            one_task(ctx)
            t = task_of(ctx)
            assert t[7] - t[6] == n  # FCAP = 1024: at most that many fetches are searched in LDS
            assert 0 < sum(d["direct"] for d in ctx["model"]["desc"]) < len(ctx["model"]["desc"])
        return Case("fetches_%d" % n, recs, one_base(0, pts), shape)
    build.__name__ = "fetches_%d" % n
    return case(build)


for _n in (wm.FCAP, wm.FCAP + 1, 1100):
    _fetch_cap(_n)


def _reach_cap(n):
    def build():
        pts = [2000 + 100 * k for k in range(n)]
        recs = [short(1900 + 37 * k, 30) for k in range((100 * n + 300) // 37)] + tail(pos=2000 + 100 * n + 500)

        def shape(ctx):
            one_task(ctx)
            t = task_of(ctx)
            assert t[5] - t[4] == n and 100 * n < wm.SUB_EXTENT  # RCAP = 256: at most that many reach intervals are searched in LDS
            k = kinds(ctx)
            assert list(k.values()).count("gap") > 100 and list(k.values()).count("emit") > 100
        return Case("reach_intervals_%d" % n, recs, one_base(0, pts), shape, slack=0)
    build.__name__ = "reach_intervals_%d" % n
    return case(build)


for _n in (wm.RCAP, wm.RCAP + 1, 300):
    _reach_cap(_n)


# ---- the filter
@case
def no_direct_record_and_every_record_direct():
    # contig c0: nothing overlaps the fetched base (all in reach: walked, none kept); contig c1: every record does
    recs = [short(1500 + 5 * k, 40) for k in range(80)] + [short(2100 + 5 * k, 40) for k in range(80)] + tail() + \
           [short(1990 + k // 4, 50, ref=1, name=b"d%04d" % k) for k in range(40)] + tail(ref=1)

    def shape(ctx):
        m = ctx["model"]
        assert len(m["first"]) == 3
        a, b = m["desc"][m["first"][0]: m["first"][1]], m["desc"][m["first"][1]: m["first"][2]]
        assert len(a) == 160 and not any(d["direct"] for d in a) and not any(m["keep"][: len(a)])
        assert len(b) == 40 and all(d["direct"] for d in b)
    return Case("no_direct_record_and_every_record_direct", recs, [(0, 2050, 2051, 0), (1, 2020, 2021, 0)], shape)


# ---- the extract
def _rng_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def sized_read(pos, L, size, name, **kw):
    """a read of exactly `size` bytes with its size field: the room goes to an aux Z field"""
    base = len(read(pos, L, name=name, **kw))
    return read(pos, L, name=name, aux=b"XZZ" + b"y" * (size - base - 4) + b"\0", **kw)


@case
def extract_lengths_pads_and_qualities():
    quals = [0, 6, 7, 8, 19, 20, 21, 40, 93, 254]  # thresholds 20 and 7: thr - 1, thr, thr + 1 of both
    recs = []
    for n, L in enumerate((0, 1, 2, 31, 32, 33, 63, 64, 65)):
        seq = bytearray(_rng_bytes(100 + L, (L + 1) // 2))
        if L & 1:
            seq[-1] |= 0x0B  # the pad nibble of an odd length, not zero in the file
        q = bytes(np.random.default_rng(L).choice(quals, L).astype(np.uint8))
        recs.append(rec(pos=1990, name=b"len%02d" % L, cigar=cig((max(L, 20), "M")), l_seq=L, seq=bytes(seq), qual=q, mref=0, mpos=1990))
    recs.append(rec(pos=2000, name=b"nocigar", l_seq=0))
    recs.append(rec(pos=2000, name=b"noqual", cigar=cig((40, "M")), l_seq=40, seq=_rng_bytes(7, 20), qual=b"\xff" + _rng_bytes(8, 39)))
    recs.append(rec(pos=2000, name=b"noqual_all", cigar=cig((33, "M")), l_seq=33, seq=_rng_bytes(9, 17), qual=b"\xff" * 33))
    recs.append(rec(pos=2000, name=b"n", cigar=cig((20, "M")), l_seq=20, mref=1, mpos=5))           # a name of one byte; the mate on another reference
    recs.append(rec(pos=2000, name=b"N" * 254, cigar=cig((20, "M")), l_seq=20, mref=-1, mpos=-1))  # the longest name (l_name 255); no mate reference
    recs.append(rec(pos=2000, name=b"long", cigar=cig((wm.LSEQ_MAX, "M")), l_seq=wm.LSEQ_MAX, seq=_rng_bytes(11, 32768), qual=_rng_bytes(12, 65535).replace(b"\xff", b"\x14")))
    recs += tail(pos=70000)

    def shape(ctx):
        one_task(ctx)
        d = ctx["model"]["desc"]
        assert [x["l_seq"] for x in d] == [0, 1, 2, 31, 32, 33, 63, 64, 65, 0, 40, 33, 20, 20, 65535] and all(x["direct"] for x in d)
        assert [x["l_name"] for x in d][12:14] == [1, 254]
        pads = [wm.parse_record(ctx["pb"].buf, x["src"] - 4)["seq"][-1] & 15 for x in d if x["l_seq"] & 1]
        assert all(pads[:5])  # (every odd length above carries a pad nibble that is not zero)
    return Case("extract_lengths_pads_and_qualities", recs, [(0, 2000, 2001, 0)], shape, thr=(20, 7))


@case
def extract_stage_cap():
    # EX_CAP = 768 bytes of LDS per record, counted from the 16-byte-aligned address in front of its size field: d + 4 + block_size of 767, 768 and 769
    # at d = 0 and d = 5
    recs, want = [], []
    for d in (0, 5):
        for tot in (wm.EX_CAP - 1, wm.EX_CAP, wm.EX_CAP + 1):
            at = (size_of(recs) + 42 + 15) // 16 * 16 + d
            pad_to(recs, at, 1990, name=b"f")
            want.append((len(recs), d, tot))
            recs.append(sized_read(1990, 100, tot - d, b"cap%d_%d" % (d, tot), mref=0, mpos=3))
    recs += tail()

    def shape(ctx):
        one_task(ctx)
        got = [((rec_buf(ctx, k) + int(ctx["pb"].blk_at[0])) & 15, ((rec_buf(ctx, k)) & 15) + len(recs[k])) for k, _, _ in want]
        assert got == [(d, tot) for _, d, tot in want]
    return Case("extract_stage_cap", recs, [(0, 2000, 2001, 0)], shape)


SA = b"SAZc1,5,+,10M,30,0;\0"
AUX_FORMS = [
    ("sa_first", SA, True),
    ("after_A", b"XAAx" + SA, True), ("after_c", b"XcC\x81" + SA, True), ("after_C", b"XCC\x01" + SA, True), ("after_s", b"Xss\x01\x02" + SA, True),
    ("after_S", b"XSS\x01\x02" + SA, True), ("after_i", b"Xii\x01\x02\x03\x04" + SA, True), ("after_I", b"XII\x01\x02\x03\x04" + SA, True),
    ("after_f", b"Xff\x00\x00\x80\x3f" + SA, True), ("after_Z", b"XZZtext\0" + SA, True), ("after_H", b"XHH1AE3\0" + SA, True),
] + [("after_B%s_%d" % (t, n), b"XBB" + t.encode() + struct.pack("<i", n) + b"\x07" * (n * w) + SA, True)
     for t, w in (("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4)) for n in (0, 3)] + [
    ("sa_inside_Z", b"XZZxSAZy\0", False), ("unknown_type", b"XQ?" + SA, False), ("Z_cut_off", b"XZZabc", False), ("i_cut_off", b"Xii\x01\x02", False),
    ("B_cut_off", b"XBBc\x01", False), ("B_negative", b"XBBc" + struct.pack("<i", -1) + SA, False), ("B_unknown_element", b"XBBZ" + struct.pack("<i", 0) + SA, False),
    ("no_tags", b"", False), ("SA_cut_to_two_bytes", b"SA", False),
]


@case
def extract_aux_forms():
    recs = [read(1990, 20, name=n.encode(), aux=a) for n, a, _ in AUX_FORMS] + tail()

    def shape(ctx):
        one_task(ctx)
        d = ctx["model"]["desc"]
        assert len(d) == len(AUX_FORMS) and all(x["direct"] for x in d)
        got = [wm.has_sa(wm.parse_record(ctx["pb"].buf, x["src"] - 4)["tags"]) for x in d]
        assert got == [w for _, _, w in AUX_FORMS]  # the model's parser against the answers written down above
    return Case("extract_aux_forms", recs, [(0, 2000, 2001, 0)], shape)


# ---- malformed records: the device flags the task BAD, the host walks it and raises
def _malformed(name, raises, fix, raises_at="walk"):
    def build():
        sound = [short(1960 + k, 50) for k in range(10)] + tail()
        recs = list(sound)
        recs[5] = fix(sound[5])

        def shape(ctx):
            one_task(ctx)
            k = kinds(ctx)
            assert all(k[i] == "emit" for i in range(5)) and 6 not in k
        return Case(name, recs, TB_FETCH, shape, twin=sound, flags={0: wm.BAD}, raises=raises, raises_at=raises_at)
    build.__name__ = name
    return case(build)


_malformed("malformed_block_size_31", MSG_SIZE, lambda r: patch(r, 0, "<i", 31))
_malformed("malformed_l_name_0", MSG_NAME, lambda r: patch(r, 12, "<B", 0))
_malformed("malformed_l_seq_65536", MSG_LSEQ, lambda r: patch(r, 20, "<i", 65536))
_malformed("malformed_l_seq_minus_1", MSG_LSEQ, lambda r: patch(r, 20, "<i", -1))
_malformed("malformed_cigar_count_overruns", MSG_NAME, lambda r: patch(r, 16, "<H", 60000))
_malformed("malformed_bases_overrun", MSG_NAME, lambda r: patch(r, 20, "<i", 200), raises_at="extract")


# ---- a set of files
@case
def reference_the_header_does_not_know():
    sound = [short(1960 + k, 50, mref=0, mpos=7) for k in range(6)] + [short(1970, 50), short(1971, 50)] + tail()
    recs = list(sound)
    recs[2] = patch(sound[2], 24, "<i", 7)  # next_refID 7 of 3: INT32_MAX in a set of files
    recs[6] = patch(sound[6], 4, "<i", 7)   # refID 7: beyond the task's reference, the walk ends

    def shape(ctx):
        one_task(ctx)
        assert kinds(ctx)[6] == "stop" and len(ctx["model"]["desc"]) == 6
        want = wm.INT32_MAX if ctx["pb"].many else 7
        assert ctx["model"]["desc"][2]["mtid"] == want
    return Case("reference_the_header_does_not_know", recs, TB_FETCH, shape, twin=sound)


def build_panel():
    cases = [fn() for fn in PANEL]
    assert len({c.name for c in cases}) == len(cases)
    return cases


# ---------------------------------------------------------------------------------------------------------------- running a case on the host
class _PlanOnly(Exception):
    pass


def _slack(case, monkeypatch):
    if case.slack is None:
        monkeypatch.delenv("UZ_STAGE_SLACK", raising=False)
    else:
        monkeypatch.setenv("UZ_STAGE_SLACK", str(case.slack))


def plan_of(src, case, thr=20) -> dict:
    """the walk plan the stage makes for the case's fetches (what select_kept hands to `walk=`), without any walk"""
    box = {}

    def grab(plan):
        box["plan"] = plan
        raise _PlanOnly()
    fc, flo, fhi, fex = case.fetch_arrays()
    try:
        src.select_kept(fc, flo, fhi, thr, walk=grab, small_tasks=True)
    except _PlanOnly:
        pass
    return box["plan"]


def context(case, w, plan, paths=None) -> dict:
    """what a case's shape assertion reads: the plan, its bytes from the file, the model's answer, the file's own block table"""
    import walkmodel
    model = walkmodel.walk_plan(plan, paths or [w["path"]])
    data, coff, at = walkmodel.inflate_file(w["path"])
    return dict(plan=plan, pb=model["pb"], model=model, info=w["info"], case=case, file_blocks=dict(off=coff), file_at=at)


def host_context(case, w, monkeypatch) -> dict:
    from unfazed_amd import io_native
    _slack(case, monkeypatch)
    src = io_native.BamSource(w["path"], threads=2, insert_size_max_sample=-1)  # (no head sample: opening reads no record)
    return context(case, w, plan_of(src, case))


def host_twin(case, w, thr=20):
    """the host's walk of the same plan (uz_stage_walk_host) and its kept list"""
    from unfazed_amd import io_native
    src = io_native.BamSource(w["path"], threads=2, insert_size_max_sample=-1)  # (no head sample: opening reads no record)
    fc, flo, fhi, fex = case.fetch_arrays()
    return src.select_kept(fc, flo, fhi, thr, small_tasks=True)


def unflagged_model(ctx, m) -> list:
    return m["desc_all"]


CODES = "=ACMGRSVTWYHKDBN"


def check_parse(path):
    """the model's parse of every record == io_native.read_bam_table's columns (the whole-file decoder keeps the placed records, in file order)"""
    import walkmodel
    from unfazed_amd import io_native
    data, coff, at = walkmodel.inflate_file(path)
    names, lens, first = walkmodel.header_of(data)
    recs = [r for r in walkmodel.records_of(data, first)]
    t = io_native.read_bam_table(path, threads=2)
    keep = [r for r in recs if r["ref"] >= 0]
    assert len(keep) == int(t.start.size), (len(keep), int(t.start.size))
    assert [int(x) for x in t.contig_off] == [sum(r["ref"] < c for r in keep) for c in range(len(names) + 1)]
    for col, key in (("start", "pos"), ("end", "end"), ("tlen", "tlen"), ("flag", "flag"), ("n_cigar", "n_cigar"), ("l_seq", "l_seq"), ("mapq", "mapq")):
        assert np.array_equal(np.asarray(getattr(t, col)).astype(np.int64), np.array([r[key] for r in keep], np.int64)), col
    for i, r in enumerate(keep):
        assert np.array_equal(t.cigar[int(t.cigar_off[i]): int(t.cigar_off[i]) + r["n_cigar"]], r["cigar"]), i
        L, o = r["l_seq"], 16 * int(t.sq_off16[i])
        want = bytes(ord(CODES[(r["seq"][b >> 1] >> (0 if b & 1 else 4)) & 15]) for b in range(L))
        assert t.seq[o: o + L].tobytes() == want, i
        if not (L and r["qual"][0] == 0xFF):
            assert t.qual[o: o + L].tobytes() == r["qual"], i
        assert t.qnames[int(t.qname[i])].encode() == r["name"], i


def check_one_pass(case, w, thr, monkeypatch):
    """the one-pass stage's table for the case's fetches (BamSource.select, every record with its bases, the quality plane as a plane) against the
    model: its kept records lie in the model's filtered set and hold every direct record; flag, l_seq, n_cigar, mapq, the aux bits and the quality
    plane of every kept record are what the model's extract writes"""
    import walkmodel
    from unfazed_amd import io_native
    _slack(case, monkeypatch)
    src = io_native.BamSource(w["path"], threads=2, insert_size_max_sample=-1)  # (no head sample: opening reads no record)
    fc, flo, fhi, fex = case.fetch_arrays()
    m = context(case, w, plan_of(src, case, thr))["model"]
    ref = src.select(fc, flo, fhi, thr, extra=fex, all_bases=True, lists=False, tup8=False)
    n = int(ref.view.n_segs)
    voff, qn, mt, bs = io_native.stage_kept_debug(src.lib, ref._stage.ptr, n)
    by_voff = {d["voff"]: (d, k) for d, k in zip(m["desc_all"], m["keep_all"])}
    assert all(int(v) in by_voff and by_voff[int(v)][1] for v in voff)
    assert {v for v, (d, k) in by_voff.items() if d["direct"]} <= {int(v) for v in voff}
    assert bs.all()
    a = ref.arrays
    tup = a["tup"][:n].astype(np.int64)
    plane = a["qlow"].view(np.uint32)
    unit = 0
    for i in range(n):
        x = walkmodel.extract(m["pb"].buf, by_voff[int(voff[i])][0]["src"], thr, True)
        got = (int(a["tup_flag"][tup[i]]), int(a["tup_l_seq"][tup[i]]), int(a["tup_n_cigar"][tup[i]]), int(a["tup_mapq"][tup[i]]), int(a["tup_aux"][tup[i]]) & 15)
        assert got == (x["flag"], x["l_seq"], x["n_cigar"], x["mapq"], x["aux"]), (i, got)
        u = (x["l_seq"] + 31) >> 5
        if u <= 255:  # (the link form counts the staged units of a record in one byte: the one-pass stage cannot say anything of a longer one)
            assert np.array_equal(plane[unit: unit + u], x["plane"]), i
        unit += u
    assert unit == int(ref.view.n_row_units)


# ---------------------------------------------------------------------------------------------------------------- the files as a set
def sets_of(cases) -> dict:
    """the cases that go through BamSource.open_many together, by the UZ_STAGE_SLACK they need (it is the process's): every case without a malformed
    record and without an expected flag -- the record whose refID its own header does not know among them"""
    out = {}
    for c in cases:
        if not c.flags and c.raises is None:
            out.setdefault(c.slack, []).append(c)
    return out


def open_set(cases, written):
    """-> (source over the cases' files, their paths, the fetches of all of them in the set's reference numbering)"""
    from unfazed_amd import io_native
    paths = [written[c.name]["path"] for c in cases]
    src = io_native.BamSource.open_many(paths, threads=2)
    parts = []
    for f, c in enumerate(cases):
        fc, flo, fhi, fex = c.fetch_arrays()
        parts.append((fc + np.int32(src.ref_base[f]), flo, fhi, fex))
    fc, flo, fhi, fex = (np.concatenate([p[k] for p in parts]) for k in range(4))
    order = np.lexsort((fhi, flo, fc))
    return src, paths, (fc[order], flo[order], fhi[order], fex[order])


def filtered(model: dict, dtype) -> np.ndarray:
    """the descriptors the device hands over: the model's walk of every task that raised no flag, through the model's filter"""
    import walkmodel
    return walkmodel.desc_array([d for d, k in zip(model["desc"], model["keep"]) if k], dtype)


def longest_read(paths) -> int:
    """the largest l_seq a record of these files declares (the chain of size fields is followed as far as it is one)"""
    import walkmodel
    out = 0
    for p in paths:
        data = walkmodel.inflate_file(p)[0]
        at = walkmodel.header_of(data)[2]
        while at + 36 <= len(data):
            r = walkmodel.parse_fixed(data, at)
            if r["bs"] < 32:
                break
            out = max(out, r["l_seq"])
            at += 4 + r["bs"]
    return out
