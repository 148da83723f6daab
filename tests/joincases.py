"""BAM files built record by record for the tests of the batch-wide joins (csrc/k_bamjoin.hip on the device, plan_finish of csrc/io_stage.cpp on the
host), in the pattern of tests/walkcases.py, whose record maker, file writer and Case they use: the PANEL -- named cases, each built against ONE
rule's edge of the joins (is_mate_of, the smallest virtual offset, wants_mate, the names, the covering, dropped copies and folds, the closure's depth
and the rotation of its counters, the frontier's sizes, the per-reference totals, files as a set).  A case carries its file, its fetches, the
UZ_STAGE_SLACK it needs and `shape(ctx)`: the assertion, from the plan and the trace of the model's closure (tests/joinmodel.py), that the branch it
aims at was reached -- which task covers the mate position, whether a need was raised, how many generations and trips ran, which copy folded.
Numbers of records inside a reach and chain lengths are taken from the plan's `reach`, never written down.  Test infrastructure."""
import ctypes as C

import numpy as np

import joinmodel
import joinoracle
import walkcases as wc
import walkmodel as wm
from walkcases import Case, read, rec, cig

P, MU, R1, R2, SUPP = 0x1, 0x8, 0x40, 0x80, 0x800
SLACK = 1000  # csrc/io_stage.cpp REACH_SLACK_DEFAULT
FAR = 12000   # behind every reach interval of a small case, inside the same 16 kb bin (walkcases.STOP_POS)


class JCase(Case):
    """a case of the joins: + all_bases; refused: the batch needs more trips through the index than UZ_JOIN_MAX_TRIPS allows, every route refuses it;
    group: the rule it belongs to (one case per group also has its table built).  Every case runs on every route"""

    def __init__(self, name, records, fetches, shape, group, all_bases=False, refused=False, **kw):
        Case.__init__(self, name, records, fetches, shape, **kw)
        self.group, self.all_bases, self.refused = group, all_bases, refused


PANEL = []


def case(fn):
    PANEL.append(fn)
    return fn


def build_panel():
    cases = [fn() for fn in PANEL]
    assert len({c.name for c in cases}) == len(cases)
    return cases


def pair(pos, mpos, flag, name=b"edge", L=50, ref=0, mref=0, **kw):
    """a paired read of the panel: L bases, one M, its mate said to lie at (mref, mpos)"""
    return read(pos, L, name=name, ref=ref, flag=P | flag, mref=mref, mpos=mpos, **kw)


def tail(ref=0, pos=FAR):
    return wc.tail(2, pos=pos, ref=ref)


# ---------------------------------------------------------------------------------------------------------------- running a case on the host
def begin(src, fetches, all_bases=False):
    """a begun stage with its blocks gathered and the walk plan of the device's route (UZ_STAGE_SMALL_TASKS: sub-tasks) -> (stage handle, plan)"""
    from unfazed_amd import io_native
    lib = src.lib
    fc, flo, fhi, fex = fetches
    st = C.c_void_p()
    flags = (io_native.STAGE_ALL_BASES if all_bases else 0) | io_native.STAGE_SMALL_TASKS
    io_native._check(lib, lib.uz_bam_stage_begin(src._h.ptr, int(fc.size), fc.ctypes.data, flo.ctypes.data, fhi.ctypes.data, fex.ctypes.data, flags, 20, int(src.threads), C.byref(st)))
    sh = io_native._Handle(st.value, lib.uz_stage_free)
    plan = io_native._gather_blocks(lib, sh, lambda n: np.empty(max(16, n), np.uint8))
    z = (C.c_int64 * 8)()
    lib.uz_stage_walk_plan_sizes(sh.ptr, z)
    nt, nsp, nr, nf, nblk, n_host = (int(x) for x in z[:6])
    task = np.zeros((max(1, nt), io_native.WALK_TASK_COLS), np.int32)
    span = np.zeros((max(1, nsp), io_native.WALK_SPAN_COLS), np.int64)
    reach, fetch = np.zeros((max(1, nr), 2), np.int32), np.zeros((max(1, nf), 3), np.int32)
    blk_coff, blk_crc = np.zeros(max(1, nblk), np.int64), np.zeros(max(1, nblk), np.uint32)
    io_native._check(lib, lib.uz_stage_walk_plan(sh.ptr, task.ctypes.data, span.ctypes.data, reach.ctypes.data, fetch.ctypes.data, blk_coff.ctypes.data, blk_crc.ctypes.data))
    plan.update(task=task[:nt], span=span[:nsp], reach=reach[:nr], fetch=fetch[:nf], blk_coff=blk_coff[:nblk], blk_crc=blk_crc[:nblk], n_ref=len(src.contigs))
    src._plan_files(plan)
    return sh, plan


def model_walk(plan, paths):
    """the descriptors of the plan's SUB-tasks as the device hands them to its joins: tests/walkmodel.py's walk of every sub-task, through the filter
    of its task of the stage -> (descriptors, d_first [n_sub + 1])"""
    from unfazed_amd import io_native
    pb = wm.PlanBytes(plan, paths)
    task = plan["task"].reshape(-1, 10)
    per = []
    for t in range(task.shape[0]):
        d, flag = wm.walk_task(pb, t)
        assert flag == 0, "a case of the joins raises no walk flag"
        per.append(d)
    keys = {}
    for t, d in enumerate(per):
        keys.setdefault(int(task[t, 9]), set()).update(x["h1"] | 1 for x in d if x["direct"])
    per = [[x for x in d if x["direct"] or (x["h1"] | 1) in keys[int(task[t, 9])]] for t, d in enumerate(per)]
    d_first = np.cumsum([0] + [len(d) for d in per]).astype(np.int64)
    return wm.desc_array([x for d in per for x in d], io_native.WALK_DESC), d_first, pb


def host_routes(case, paths, src, fetches):
    """every host route's answer for a case -> ctx: plan, trace, model, one_pass, twin, twin_sub (each dict(voff, qname, mate, bases, n_qnames))"""
    from unfazed_amd import io_native
    lib = src.lib
    fc, flo, fhi, fex = fetches

    def debug(stage, n, n_qnames):
        voff, qn, mt, bs = io_native.stage_kept_debug(lib, stage.ptr, n)
        return dict(voff=voff, qname=qn, mate=mt, bases=bs.astype(bool), n_qnames=int(n_qnames))

    out = dict(case=case)
    sh, plan = begin(src, fetches, case.all_bases)
    desc, d_first, pb = model_walk(plan, paths)
    nt = plan["task"].shape[0]
    out.update(plan=plan, pb=pb, desc=desc, d_first=d_first, trace={})
    routes = dict(
        model=lambda: joinmodel.run(lib, sh.ptr, desc, d_first, np.zeros(max(1, nt), np.int32), plan, len(src.contigs), case.all_bases, out["trace"]),
        one_pass=lambda: (lambda r: debug(r._stage, int(r.view.n_segs), r.view.n_qnames))(src.select(fc, flo, fhi, 20, extra=fex, all_bases=case.all_bases)),
        twin=lambda: (lambda k: debug(k._stage, k.n, k.n_qnames))(src.select_kept(fc, flo, fhi, 20, all_bases=case.all_bases, small_tasks=True)),
        twin_sub=lambda: (lambda k: debug(k._stage, k.n, k.n_qnames))(
            src.select_kept(fc, flo, fhi, 20, all_bases=case.all_bases, walk=lambda p: (desc, d_first, np.zeros(max(1, nt), np.int32), np.diff(d_first), None))),
    )
    out["refusals"] = {}
    for name, fn in routes.items():
        try:
            out[name] = fn()
        except (io_native.IoError, joinmodel.ClosureRefused) as e:
            out["refusals"][name] = str(e)
    return out


EQUAL = ("voff", "qname", "mate", "bases", "n_qnames")


def same(a, b):
    return [k for k in EQUAL if not np.array_equal(a[k], b[k])]


# ---------------------------------------------------------------------------------------------------------------- what a shape assertion reads
def idx(ctx, k):
    """the model's descriptor indices (trace D) of record k of the file, in the order the descriptors came"""
    v = ctx["recs"][k]["voff"]
    return [int(i) for i in np.flatnonzero(ctx["trace"]["D"]["voff"] == np.uint64(v))]


def rec_of(ctx, i):
    """the file's record number of the model's descriptor i"""
    return ctx["by_voff"][int(ctx["trace"]["D"]["voff"][i])]


def kept_recs(ctx):
    return ctx["oracle"]["rec"]


def mate_rec(ctx, k):
    """the file's record the ORACLE gives as mate of record k (None: none, or k is no member)"""
    o = ctx["oracle"]
    if k not in o["rec"]:
        return None
    m = int(o["mate"][o["rec"].index(k)])
    return None if m < 0 else o["rec"][m]


def reach_of(ctx):
    return ctx["plan"]["reach"].reshape(-1, 2).tolist()


def stage_tasks(ctx):
    return sorted(set(int(x) for x in ctx["plan"]["task"].reshape(-1, 10)[:, 9]))


def asked(ctx, k):
    """was a need raised for (a copy of) record k, in which trip (1-based; None: never)"""
    for t, need in enumerate(ctx["trace"]["needs"]):
        if any(i in need for i in idx(ctx, k)):
            return t + 1
    return None


def covering_of(ctx, k):
    """the join task the model found to cover the mate position of record k's first asking copy (-1: none; None: it never asked)"""
    for i in idx(ctx, k):
        if i in ctx["trace"]["tc"]:
            return ctx["trace"]["tc"][i]
    return None


def simple(ctx, trips=0):
    assert len(ctx["trace"]["needs"]) == trips, ctx["trace"]["needs"]


# ================================================================================================================ the panel
FETCH = [(0, 2000, 2001, 0)]  # default slack: reach [1000, 3001)


# ---------------------------------------------------------------------------------------------------------------- is_mate_of
def _mate_edge(name, cand_pos, cand_L, mpos, inside, cand_flag=R2, asker_flag=R1, cigar=True, note=""):
    def build():
        asker = pair(1990, mpos, asker_flag)
        if cigar:
            cand = pair(cand_pos, 1990, cand_flag, L=cand_L)
        else:
            cand = rec(pos=cand_pos, name=b"edge", flag=P | cand_flag, l_seq=cand_L, mref=0, mpos=1990)
        recs = sorted([cand, asker], key=lambda r: wm.parse_fixed(r, 0)["pos"]) + tail()
        ki = recs.index(asker)
        kc = recs.index(cand)

        def shape(ctx):
            simple(ctx)
            a, b = reach_of(ctx)[0]
            assert a <= mpos < b and covering_of(ctx, ki) == 0 and asked(ctx, ki) is None  # answered inside the task: no need
            c = ctx["recs"][kc]
            assert not (c["pos"] < 2001 and c["end"] > 2000), "the candidate is no fetched record"
            assert (mate_rec(ctx, ki) == kc) == inside and (kc in kept_recs(ctx)) == inside
        return JCase(name, recs, FETCH, shape, "is_mate_of", note=note)
    build.__name__ = name
    return case(build)


_mate_edge("mate_pos_at_mpos", 1500, 50, 1500, True)
_mate_edge("mate_pos_at_mpos_plus_1", 1501, 50, 1500, False)
_mate_edge("mate_end_at_mpos", 1450, 50, 1500, False)
_mate_edge("mate_end_at_mpos_plus_1", 1451, 50, 1500, True)
_mate_edge("mate_without_cigar_at_mpos", 1500, 30, 1500, True, cigar=False, note="no CIGAR: end = pos + 1 (bam_endpos)")
_mate_edge("mate_without_cigar_one_before_mpos", 1499, 30, 1500, False, cigar=False)
_mate_edge("mate_same_read_of_pair_flag", 1500, 50, 1500, False, cand_flag=R1)
_mate_edge("asker_both_flags", 1500, 50, 1500, False, asker_flag=R1 | R2, note="wants nobody: the name is seen, the mate is -1, no need")
_mate_edge("asker_neither_flag_candidate_read1", 1500, 50, 1500, True, asker_flag=0, cand_flag=R1)
_mate_edge("asker_neither_flag_candidate_read2", 1500, 50, 1500, True, asker_flag=0, cand_flag=R2)
_mate_edge("candidate_both_flags", 1500, 50, 1500, True, cand_flag=R1 | R2)


# ---------------------------------------------------------------------------------------------------------------- the smallest virtual offset wins
def _first_in_file(name, cands, ends=(), index=False, note=""):
    """cands: (pos, flag) of the candidates, all of which qualify; the first in the file must win"""
    def build():
        mpos = 6020 if index else 1520
        asker = pair(1990, mpos, R1)
        cs = [pair(p, 1990, f, L=60) for p, f in cands]
        recs = ([asker] + tail(pos=3500) + cs + tail()) if index else (cs + [asker] + tail())
        k0 = recs.index(cs[0])
        ki = recs.index(asker)

        def shape(ctx):
            simple(ctx, 1 if index else 0)
            r = ctx["recs"]
            assert all(r[k0 + j]["pos"] <= mpos < r[k0 + j]["end"] and r[k0 + j]["flag"] & R2 for j in range(len(cs)))  # every one of them qualifies
            assert mate_rec(ctx, ki) == k0 and not any(k0 + j in kept_recs(ctx) for j in range(1, len(cs)))
            v = [r[k0 + j]["voff"] for j in range(len(cs))]
            if ends:
                assert v[0] >> 16 != v[1] >> 16  # two BGZF blocks: the block's offset decides
            else:
                assert v[0] >> 16 == v[1] >> 16 and v[0] < v[1]  # one block: the offset inside it decides
            if index:
                from unfazed_amd import io_native
                D = ctx["trace"]["D"]
                assert all(int(D["src"][i]) & io_native.WALK_SRC_AUX for j in range(len(cs)) for i in idx(ctx, k0 + j))  # copies from the index, both of them
                assert asked(ctx, ki) == 1
        return JCase(name, recs, FETCH, shape, "first_in_file", ends=ends, slack=100 if index else None, note=note)
    build.__name__ = name
    return case(build)


_first_in_file("two_candidates", [(1480, R2), (1490, R2)])
_first_in_file("three_candidates", [(1470, R2), (1480, R2), (1490, R2)])
_first_in_file("supplementary_ahead_of_the_primary", [(1480, R2 | SUPP), (1495, R2)])
_first_in_file("candidates_in_two_blocks", [(1480, R2), (1490, R2)], ends=[-(len(pair(1480, 1990, R2, L=60)) + 1)])
_first_in_file("candidates_from_the_index", [(5990, R2), (6000, R2)], index=True, note="slack 100: the mate position lies outside the reach, both candidates are copies from the index")


# ---------------------------------------------------------------------------------------------------------------- wants_mate
def _wants(name, flag, mref, wants, note=""):
    def build():
        asker = read(1990, 50, name=b"edge", flag=flag, mref=mref, mpos=1500)
        cand = {r: read(1500, 50, name=b"edge", ref=r, flag=P | R2, mref=0, mpos=1990) for r in range(3)}
        recs = [cand[0], asker] + tail() + [cand[1]] + tail(1) + [cand[2]] + tail(2)

        def shape(ctx):
            n_ref = len(ctx["case"].contigs)
            assert n_ref == 3
            if not wants:
                simple(ctx)
                assert mate_rec(ctx, 1) is None and kept_recs(ctx) == [1] and covering_of(ctx, 1) is None  # nobody was asked: the candidate is there and stays out
            else:
                k = recs.index(cand[mref])
                assert mate_rec(ctx, 1) == k and (asked(ctx, 1) == 1) == (mref != 0)
        return JCase(name, recs, FETCH, shape, "wants_mate", note=note)
    build.__name__ = name
    return case(build)


_wants("wants_unpaired", R1, 0, False)
_wants("wants_mate_unmapped", P | MU | R1, 0, False)
_wants("wants_mtid_minus_1", P | R1, -1, False)
_wants("wants_mtid_0", P | R1, 0, True)
_wants("wants_mtid_last_reference", P | R1, 2, True, note="mtid == n_ref - 1: asked, through the index (no fetch on that reference)")
_wants("wants_mtid_n_ref", P | R1, 3, False, note="mtid == n_ref: in a set of files the walk makes it INT32_MAX (test_files_as_a_set)")
_wants("wants_mtid_unknown_to_the_header", P | R1, 7, False)


# ---------------------------------------------------------------------------------------------------------------- names
def _two_names(name, na, nb, note=""):
    def build():
        # the candidates of both names overlap both mate positions, the OTHER name's first: a name compared wrongly picks it
        recs = [pair(1500, 1990, R2, name=nb), pair(1500, 1990, R2, name=na), pair(1990, 1500, R1, name=na), pair(1990, 1500, R1, name=nb)] + tail()

        def shape(ctx):
            simple(ctx)
            assert [mate_rec(ctx, k) for k in range(4)] == [3, 2, 1, 0] and ctx["oracle"]["names"] == [nb, na]
            assert ctx["oracle"]["qname"].tolist()[:4] == [0, 1, 1, 0]
        return JCase(name, recs, FETCH, shape, "names", note=note)
    build.__name__ = name
    return case(build)


_two_names("names_same_length", b"nameA", b"nameB")
_two_names("names_prefix", b"nm", b"nmx")
_two_names("names_prefix_reversed", b"nmx", b"nm")
_two_names("names_1_and_254_bytes", b"n", b"N" * 254)


@case
def name_with_four_records():
    recs = [pair(1480, 1990, R2 | SUPP), pair(1500, 1990, R2), pair(1985, 1480, R1 | SUPP), pair(1990, 1500, R1)] + tail()

    def shape(ctx):
        simple(ctx)
        assert [mate_rec(ctx, k) for k in range(4)] == [2, None, 0, 0] and ctx["oracle"]["n_qnames"] == 1  # (1500 lies inside the supplementary R2 as well: it is the first)
        assert kept_recs(ctx) == [0, 2, 3]
    return JCase("name_with_four_records", recs, FETCH, shape, "names")


@case
def name_first_met_as_a_mate_only_copy():
    recs = [pair(1400, 1990, R2, name=b"yy"), read(1985, 50, name=b"xx"), pair(1990, 1400, R1, name=b"yy")] + tail()

    def shape(ctx):
        simple(ctx)
        o = ctx["oracle"]
        assert o["qname"].tolist() == [0, 1, 0] and o["bases"].tolist() == [False, True, True] and o["names"] == [b"yy", b"xx"]  # ids by output order, not by who was fetched
    return JCase("name_first_met_as_a_mate_only_copy", recs, FETCH, shape, "names")


@case
def name_on_two_contigs():
    recs = [pair(1990, 1995, R1, mref=1), read(1991, 50, name=b"other")] + tail() + [pair(1995, 1990, R2, ref=1, mref=0), read(1996, 50, ref=1, name=b"other")] + tail(1)
    k1 = len(recs) - 4

    def shape(ctx):
        simple(ctx)
        assert len(stage_tasks(ctx)) == 2 and covering_of(ctx, 0) == 1 and covering_of(ctx, k1) == 0  # each asks the OTHER task of the stage
        assert mate_rec(ctx, 0) == k1 and mate_rec(ctx, k1) == 0
        assert ctx["oracle"]["qname"].tolist() == [0, 1, 0, 1]  # "other" is one name on both contigs, though nobody is anybody's mate
    return JCase("name_on_two_contigs", recs, FETCH + [(1, 2000, 2001, 0)], shape, "names")


NAME_LENGTHS = (1, 7, 8, 9, 254)


@case
def names_of_every_length():
    recs = [read(1990, 30, name=bytes(97 + (n + j) % 26 for j in range(n))) for n in NAME_LENGTHS] + tail()

    def shape(ctx):
        simple(ctx)
        assert [len(n) for n in ctx["oracle"]["names"]] == list(NAME_LENGTHS)  # k_name_gather: eight lanes per name -- below, at and above one trip of them
    return JCase("names_of_every_length", recs, FETCH, shape, "names")


# ---------------------------------------------------------------------------------------------------------------- covering (UZ_STAGE_SLACK 100)
def _covering(name, mpos_of, inside, fetches=None, mref=0, note=""):
    """the asker's mate position against the reach intervals of the plan: mpos_of(reach) -> the position; the candidate starts on it"""
    def build():
        f = fetches or FETCH
        a0, b0 = 1900, 2101
        mpos = mpos_of(a0, b0)
        asker = pair(1990, mpos, R1, mref=mref)
        cand = pair(mpos, 1990, R2, ref=mref, L=40)
        c0 = sorted([asker, cand], key=lambda r: wm.parse_fixed(r, 0)["pos"]) if mref == 0 else [asker]
        extra0 = [read(2990, 40, name=b"far0")] if any(t == 0 and lo > 2500 for t, lo, hi, _ in f) else []
        recs = c0 + extra0 + tail() + ([cand] if mref == 1 else []) + tail(1) + [read(1990, 40, ref=2, name=b"far2")] + tail(2)
        ki, kc = recs.index(asker), recs.index(cand)

        def shape(ctx):
            rr = reach_of(ctx)
            assert rr[0] == [a0, b0] and mpos == mpos_of(*rr[0])
            assert mate_rec(ctx, ki) == kc  # in or out: the answer is the same record -- from the task or from the index
            if inside:
                simple(ctx)
                assert covering_of(ctx, ki) == 0 and asked(ctx, ki) is None
            else:
                assert covering_of(ctx, ki) == -1 and asked(ctx, ki) == 1
        return JCase(name, recs, f, shape, "covering", slack=100, note=note)
    build.__name__ = name
    return case(build)


_covering("covering_first_base", lambda a, b: a, True)
_covering("covering_one_before_the_first_base", lambda a, b: a - 1, False)
_covering("covering_last_base", lambda a, b: b - 1, True)
_covering("covering_at_the_end", lambda a, b: b, False)
_covering("covering_gap_between_two_intervals", lambda a, b: 2500, False, fetches=FETCH + [(0, 3000, 3001, 0)])
_covering("covering_reference_without_interval", lambda a, b: 1950, False, mref=1, fetches=FETCH + [(2, 2000, 2001, 0)],
          note="the search ends on an interval of the reference BEHIND the mate's")
_covering("covering_behind_the_last_interval_of_its_reference", lambda a, b: 5000, False, fetches=FETCH + [(2, 2000, 2001, 0)],
          note="the search ends on another reference's first interval")
_covering("covering_behind_the_last_interval_of_all", lambda a, b: 5000, False, note="the search ends behind the table")


@case
def covered_but_the_name_filter_dropped_the_record():
    # the mate lies in the reach of the task on c1, which walked it -- and did not keep it: it shares no name with a record a fetch of c1 returns
    recs = [pair(1990, 1950, R1, mref=1)] + tail() + [pair(1950, 1990, R2, ref=1, mref=0, L=30), read(1990, 40, ref=1, name=b"other")] + tail(1)
    kc = 3

    def shape(ctx):
        assert covering_of(ctx, 0) == 1 and asked(ctx, 0) == 1 and len(ctx["trace"]["needs"]) == 1  # covered, the name unseen there: a need all the same
        d = ctx["desc"]
        assert not (d["voff"] == np.uint64(ctx["recs"][kc]["voff"])).any()  # (the first walk handed no copy of it over)
        assert mate_rec(ctx, 0) == kc
    return JCase("covered_but_the_name_filter_dropped_the_record", recs, FETCH + [(1, 2000, 2001, 0)], shape, "covering", slack=100)


# ---------------------------------------------------------------------------------------------------------------- dropped copies and folds
def _long(pos, end, flag=0, mpos=-1, name=b"edge"):
    return rec(pos=pos, name=name, cigar=cig((50, "M"), (end - pos - 100, "N"), (50, "M")), l_seq=100, flag=(P | flag) if mpos >= 0 else 0, mref=0 if mpos >= 0 else -1, mpos=mpos)


def _sub_task_copy(name, at_stop):
    def build():
        # one task of the stage, two reach intervals further apart than a sub-task spans: two walk sub-tasks, and a record that reaches from the first
        # interval's last base (or the first base behind it) into the second -- which the fetch of the second interval returns
        stop = 2000 + 1 + SLACK
        pos = stop if at_stop else stop - 1
        recs = [read(1990, 50, name=b"a")] + [_long(pos, 40100)] + [read(39990, 50, name=b"b")] + tail(pos=60000)

        def shape(ctx):
            simple(ctx)
            task = ctx["plan"]["task"].reshape(-1, 10)
            assert task.shape[0] == 2 and task[:, 9].tolist() == [0, 0] and int(task[0, 1]) == stop  # two sub-tasks of one stage task
            d, first = ctx["desc"], ctx["d_first"]
            copies = np.flatnonzero(d["voff"] == np.uint64(ctx["recs"][1]["voff"])).tolist()
            if at_stop:
                assert len(copies) == 1 and copies[0] >= first[1]  # the sub-task before stopped AT it: the second one's copy is the record
            else:
                assert len(copies) == 2 and copies[0] < first[1] <= copies[1] and d["direct"][copies].tolist() == [1, 1]  # met twice: the later copy is dropped
            assert kept_recs(ctx) == [0, 1, 2]
        return JCase(name, recs, FETCH + [(0, 40000, 40001, 0)], shape, "copies")
    build.__name__ = name
    return case(build)


_sub_task_copy("sub_task_copy_at_stop_minus_1", False)
_sub_task_copy("sub_task_copy_at_stop", True)

BIG = 65000


def _neighbours(name, fetch_a, asker=None, second_asker=False, all_bases=False, note=""):
    """two tasks of the stage on one reference -- 13 stored blocks of filler between them, more than a task may gather -- and a 2.5 kb record X that
    both walk: A's reach ends on X's first base + 1, B's fetch returns X (or, with second_asker, does not: B holds an asker of its own)"""
    def build():
        x = rec(pos=16000, name=b"edge", cigar=cig((2500, "M")), l_seq=2500, flag=(P | R2) if asker is not None else 0, mref=0 if asker is not None else -1,
                mpos=14990 if asker is not None else -1)
        recs = []
        if asker is not None:
            recs.append(pair(14990, asker, R1))
        recs += [read(15000, 30, name=b"a"), x]
        kx = len(recs) - 1
        recs.append(read(17000, 30, name=b"stop"))  # (behind A's reach and inside the block A gathers: A's walk ends at a record, not at the end of its bytes)
        recs += [wc.filler(17000, BIG, name=b"f%02d" % k) for k in range(13)]
        if second_asker:
            recs.append(pair(19000, 18450, R1 | SUPP))
        recs += [read(19010, 30, name=b"b")] + tail(pos=30000)
        fetches = [fetch_a, (0, 19020, 19021, 0) if second_asker else (0, 18400, 18401, 0)]

        def shape(ctx):
            simple(ctx)
            assert len(stage_tasks(ctx)) == 2 and len(reach_of(ctx)) == 2
            ra, rb = reach_of(ctx)
            X = ctx["recs"][kx]
            assert X["pos"] < ra[1] and X["end"] > ra[0] and X["pos"] < rb[1] and X["end"] > rb[0]  # inside both reaches
            copies = idx(ctx, kx)
            tr = ctx["trace"]
            assert len(copies) == 2 and tr["jt"][copies].tolist() == [0, 1]
            keep = tr["keep"][copies].tolist()
            if second_asker:
                assert keep == [1, 1] and copies[1] in tr["folded"]  # reached in ONE generation through two tasks: the earlier copy survives, the later asks nothing
                assert tr["mate"][copies[0]] >= 0 and tr["mate"][copies[1]] == -1
            elif asker is not None:
                assert keep == [1, 2] and int(tr["surv"][kept_recs(ctx).index(kx)]) == copies[1]  # only a mate in A, fetched in B: B's copy survives
                assert bool(ctx["oracle"]["bases"][kept_recs(ctx).index(kx)])
            else:
                assert keep == [2, 2] and int(tr["surv"][kept_recs(ctx).index(kx)]) == copies[0] and copies[1] in tr["folded"]
            assert kept_recs(ctx).count(kx) == 1
        return JCase(name, recs, fetches, shape, "copies", level=0, all_bases=all_bases, note=note)
    build.__name__ = name
    return case(build)


_neighbours("fetched_by_two_neighbouring_tasks", (0, 16100, 16101, 0))
_neighbours("fetched_in_b_only_a_mate_in_a", (0, 15000, 15001, 0), asker=16000)
_neighbours("fetched_in_b_only_a_mate_in_a_all_bases", (0, 15000, 15001, 0), asker=16000, all_bases=True)
_neighbours("reached_in_one_generation_through_two_tasks", (0, 15000, 15001, 0), asker=16000, second_asker=True)


@case
def two_mates_outside_every_reach():
    recs = [pair(1990, 5000, R1), pair(5000, 1990, R2)] + tail()

    def shape(ctx):
        assert reach_of(ctx) == [[2000, 2001]]
        tr = ctx["trace"]
        assert len(tr["needs"]) == 2 and asked(ctx, 0) == 1 and asked(ctx, 1) == 2  # the record asks, its mate's copy asks -- and the copy of the record that comes back folds
        a = idx(ctx, 0)
        assert len(a) == 2 and a[1] in tr["folded"] and tr["keep"][a].tolist() == [2, 1]
        assert kept_recs(ctx) == [0, 1] and ctx["oracle"]["mate"].tolist()[:2] == [1, 0]
    return JCase("two_mates_outside_every_reach", recs, FETCH, shape, "copies", slack=0)


# ---------------------------------------------------------------------------------------------------------------- the closure's depth
CHAIN_FETCH = [(0, 1000, 1001, 0)]  # default slack: reach [0, 2001)


def chain_links(positions, L=2):
    """one name, read 1 and read 2 in turn, every record's mate position the next record's first base; the last one asks for nobody"""
    out = []
    for k, p in enumerate(positions):
        last = k + 1 == len(positions)
        out.append(read(p, L, name=b"chain", flag=(P if not last else 0) | (R1 if k % 2 == 0 else R2), mref=-1 if last else 0, mpos=-1 if last else positions[k + 1]))
    return out


def _chain_in_reach(n, name=None):
    def build():
        b = 1001 + SLACK
        count = min(n, (b - 1000) // 3)
        pos = [1000 + 3 * k for k in range(count)]
        recs = chain_links(pos) + tail()

        def shape(ctx):
            simple(ctx)
            assert reach_of(ctx) == [[0, b]] and pos[-1] < b and count == n
            assert ctx["trace"]["gens"] == [count] and kept_recs(ctx) == list(range(count))  # a generation per record, every one in memory
            assert ctx["oracle"]["bases"].tolist()[:2] == [True, False]
        return JCase(name or "chain_of_%d_generations" % n, recs, CHAIN_FETCH, shape, "closure")
    build.__name__ = name or "chain_of_%d_generations" % n
    return case(build)


for _n in (2, 3, 4, 5, 8, 9):  # uz_join_run looks at its counters every four generations
    _chain_in_reach(_n)
_chain_in_reach(300, "chain_of_300_in_one_reach")
_chain_in_reach(258, "chain_of_258_in_one_reach")  # one more than 64 looks of four generations


def _chain_of_trips(t):
    def build():
        pos = [1000 + 5000 * k for k in range(t + 1)]
        recs = chain_links(pos, L=30) + tail(pos=pos[-1] + 5000)

        def shape(ctx):
            tr = ctx["trace"]
            if t > joinmodel.MAX_TRIPS:
                assert len(tr["needs"]) == joinmodel.MAX_TRIPS  # (the trips the model made before it refused)
                return
            assert len(tr["needs"]) == t and all(len(n) == 1 for n in tr["needs"]) and kept_recs(ctx) == list(range(t + 1))
            assert [asked(ctx, k) for k in range(t)] == list(range(1, t + 1))
        return JCase("chain_of_%d_trips" % t, recs, CHAIN_FETCH, shape, "closure", refused=t > joinmodel.MAX_TRIPS)
    build.__name__ = "chain_of_%d_trips" % t
    return case(build)


for _t in (1, 2, 3, 4, joinmodel.MAX_TRIPS, joinmodel.MAX_TRIPS + 1):  # k_set_targets refills the frontier at J.round % 3 == 1, 2, 0, 1
    _chain_of_trips(_t)


@case
def chain_of_generations_and_trips():
    pos = [1000, 1003, 1006, 9000, 1009, 1012, 1015, 1018, 1021, 14000, 1024, 1027]
    links = chain_links(pos, L=2)
    recs = sorted(links, key=lambda r: wm.parse_fixed(r, 0)["pos"])
    recs = recs[:-2] + tail(pos=5000) + [recs[-2]] + tail(pos=12000) + [recs[-1]] + tail(pos=20000)

    def shape(ctx):
        tr = ctx["trace"]
        # three generations in memory and a need; the asker again, the copy from the index, five more in memory and a need; the asker, the copy, two more
        assert tr["gens"] == [3, 2 + 5, 2 + 2] and len(tr["needs"]) == 2
        assert len(kept_recs(ctx)) == len(pos)
    return JCase("chain_of_generations_and_trips", recs, CHAIN_FETCH, shape, "closure")


# ---------------------------------------------------------------------------------------------------------------- the frontier's sizes
def _frontier(n):
    def build():
        recs = [pair(1500, 1990, R2, name=b"p%04d" % k) for k in range(n)] + [pair(1990, 1500, R1, name=b"p%04d" % k) for k in range(n)] + tail()

        def shape(ctx):
            simple(ctx)
            assert ctx["trace"]["gens"] == [2] and len(kept_recs(ctx)) == 2 * n  # n fetched records ask, n mates join at once -- and ask in their turn
            assert int(ctx["oracle"]["bases"].sum()) == n
        return JCase("frontier_of_%d" % n, recs, FETCH, shape, "frontier")
    build.__name__ = "frontier_of_%d" % n
    return case(build)


for _n in (1, 63, 64, 65, 256, 257):  # wave_slot: a partial ballot, a full one, one lane of the next; a block's edge
    _frontier(_n)


@case
def needs_65_in_one_round():
    n = 65
    recs = [pair(1990, 6000 + 100 * k, R1, name=b"p%04d" % k) for k in range(n)] + tail(pos=4000) + [pair(6000 + 100 * k, 1990, R2, name=b"p%04d" % k) for k in range(n)] + tail(pos=20000)

    def shape(ctx):
        tr = ctx["trace"]
        assert [len(x) for x in tr["needs"]] == [n] and len(kept_recs(ctx)) == 2 * n
    return JCase("needs_65_in_one_round", recs, FETCH, shape, "frontier")


# ---------------------------------------------------------------------------------------------------------------- per-reference totals
def _totals(name, per_ref, note=""):
    def build():
        recs = []
        for r, n in enumerate(per_ref):
            recs += [read(1990, 30 + (7 * k + 11 * r) % 40, ref=r, name=b"t%d_%03d" % (r, k)) for k in range(n)] + tail(r)
        fetches = [(r, 2000, 2001, 0) for r, n in enumerate(per_ref) if n]

        def shape(ctx):
            simple(ctx)
            got = [sum(1 for k in kept_recs(ctx) if ctx["recs"][k]["ref"] == r) for r in range(3)]
            assert got == list(per_ref) and (sum(per_ref) <= 64 or max(per_ref) >= 128)
        return JCase(name, recs, fetches, shape, "totals", note=note)
    build.__name__ = name
    return case(build)


_totals("totals_three_contigs_in_one_wavefront", (5, 7, 3), note="k_final_out: the wavefront's records lie on three references")
_totals("totals_one_contig_whole_wavefronts", (0, 130, 0), note="k_final_out: one atomic per wavefront")
_totals("totals_an_empty_contig_between_two", (9, 0, 4))
_totals("totals_a_wavefront_across_two_contigs", (150, 0, 140))


def groups_of(cases):
    out = {}
    for c in cases:
        out.setdefault(c.group, []).append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------- files as a set
SET_CASES = ("mate_pos_at_mpos", "wants_mtid_n_ref", "names_same_length", "chain_of_2_trips", "name_on_two_contigs", "two_candidates")


def open_twice(cases, first, second):
    """every case's file twice -- byte-identical records and names -- as ONE source (BamSource.open_many) -> (source, paths, fetches in the set's
    reference numbering, sorted)"""
    from unfazed_amd import io_native
    paths = [w[c.name]["path"] for c in cases for w in (first, second)]
    src = io_native.BamSource.open_many(paths, threads=2)
    parts = []
    for f in range(len(paths)):
        fc, flo, fhi, fex = cases[f // 2].fetch_arrays()
        parts.append((fc + np.int32(src.ref_base[f]), flo, fhi, fex))
    fc, flo, fhi, fex = (np.concatenate([p[k] for p in parts]) for k in range(4))
    order = np.lexsort((fhi, flo, fc))
    return src, paths, (fc[order], flo[order], fhi[order], fex[order])


# ---------------------------------------------------------------------------------------------------------------- descriptor level
def rows_of(path, fetches, rename=None):
    """the records of a file as descriptors the HOST hands to the joins (uz_walk_desc with UZ_WALK_TASK_JOIN, all of join task 0), as a walk with
    no task of its own would meet them: every asker raises a need, and the answer is join task 0.  rename: {name: (h1, h2, l_name) of another name}
    -- what no file can hold: two names that agree in a hash"""
    from unfazed_amd import io_native
    recs, n_ref = joinoracle.records(path)
    rows = np.zeros(len(recs), io_native.WALK_DESC)
    for k, r in enumerate(recs):
        h1, h2, ln = wm.hash1(r["name"]), wm.hash2(r["name"]), len(r["name"])
        if rename and r["name"] in rename:
            h1, h2, ln = rename[r["name"]](h1, h2, ln)
        direct = any(r["ref"] == t and r["pos"] < hi and r["end"] > lo for t, lo, hi, _ in fetches)
        rows[k] = (r["voff"], io_native.WALK_SRC_AUX | r["at"], h1, r["pos"], r["end"], r["tlen"], r["mpos"], r["mref"], h2, io_native.WALK_TASK_JOIN | 0, r["flag"], r["l_seq"],
                   r["n_cigar"], r["mapq"], ln, int(direct), 0, 0)
    return rows, recs, n_ref


def join_rows(rows, n_ref, trace=None):
    """the pure model over such rows: nothing is covered, every need is answered by join task 0, the index brings nothing new"""
    from unfazed_amd import io_native
    return joinmodel.join(rows, np.zeros(rows.size, np.int64), np.zeros(rows.size, bool), lambda tid, pos: -1, n_ref,
                          lambda D, need: (np.zeros(0, io_native.WALK_DESC), np.zeros(len(need), np.int32)), trace=trace)


def desc_level_cases(folder):
    """-> [(name, rows, n_ref, the oracle's answer)]: the two names of names_same_length / names_prefix made to agree in h1, in h1 and h2 (they then
    differ in the length alone), and in all three -- which the joins hold to be ONE name: the oracle's answer for the file with one name"""
    A, B, C2 = b"nameA", b"nameB", b"nmx"
    hA = (wm.hash1(A), wm.hash2(A), len(A))

    def recs_with(na, nb):
        return [pair(1500, 1990, R2, name=nb), pair(1500, 1990, R2, name=na), pair(1990, 1500, R1, name=na), pair(1990, 1500, R1, name=nb)] + tail()

    out = []
    for name, other, rename, one_name in (
            ("equal_h1_different_h2", B, lambda h1, h2, ln: (hA[0], h2, ln), False),
            ("equal_h1_and_h2_different_length", C2, lambda h1, h2, ln: (hA[0], hA[1], ln), False),
            ("all_three_equal", B, lambda h1, h2, ln: hA, True)):
        c = Case(name, recs_with(A, other), FETCH, None)
        w = c.write(folder)
        rows, recs, n_ref = rows_of(w["path"], FETCH, {other: rename})
        if one_name:  # the same layout under ONE name: same offsets (the names are as long as each other), and the first candidate in the file answers both askers
            c1 = Case(name + "_one_name", recs_with(A, A), FETCH, None)
            recs1, _ = joinoracle.records(c1.write(folder)["path"])
            assert [r["voff"] for r in recs1] == [r["voff"] for r in recs]
            recs = recs1
        out.append((name, rows, n_ref, joinoracle.join(recs, FETCH, 0, n_ref)))
    return out
