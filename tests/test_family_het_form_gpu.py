"""The het form of a trio's genotype columns on the device (uz_types.h: uz_family_view.het9 ...; k_sites_expand): the SNV / breakpoint
class bytes and the window lists of a family staged in the het form equal those of the same family staged with all nine columns, and the
C oracle's, on the edge tables of tests/hetcases.py; a broken het_span_off raises the upload error; what needs the other sites' columns
is refused; a staged pass in the het form (the default of BenchLoad.stage) gives the results of one in the plain forms.
Every comparison is np.array_equal."""
import numpy as np
import pytest

import hetcases
import sitecases
from unfazed_amd import abi, io_native, pipeline
from unfazed_amd.engine import UnfazedHipError

pytestmark = pytest.mark.gpu

MODE = abi.FIND_SECOND_WINDOW
SNV_BITS = 0x07  # UZ_CL_HET | UZ_CL_CAND | UZ_CL_ALT_DAD: what a het-form family classifies
LISTS = ("cand_off", "cand_idx", "cand_flags", "het_off", "het_idx")


def _compact(t):
    plain = abi.sites_view(t)
    cv, block, _ = io_native.pack_sites(plain.view)
    return abi.Held(cv, dict(block=block, plain=plain))


def _stage(engine, t, het, hoff_edit=None):
    """-> (sites id, family id, what must stay alive)"""
    c8 = hetcases.columns8(t)
    held = _compact(t)
    if not het:
        sid, fid = engine.upload_sites_family_async(held, c8[0], c8[1], c8[2], c8[3], c8[4])
        return sid, fid, (held, c8)
    h9, hoff, _ = io_native.pack_family_het(*c8[:4])
    if hoff_edit is not None:
        hoff_edit(hoff)
    sid, fid = engine.upload_sites_family_async(held, c8[0], None, None, None, c8[4], het=(h9, hoff))
    return sid, fid, (held, c8, h9, hoff)


def _dnms(t):
    """point DNMs at the table's start, across every span boundary and at its end, and one whose window holds the whole table"""
    n = t.n_sites
    at = sorted({0, n - 1, n // 2} | {s for b in range(1024, n, 1024) for s in (b - 1, b)})
    st = np.array([int(t.pos[i]) for i in at] + [int(t.pos[n // 2])], np.int32)
    return dict(contig=np.zeros(st.size, np.int32), start=st, end=st + 1, vartype=np.zeros(st.size, np.uint8), mult=np.ones(st.size, np.uint8),
                tags=["s%d" % i for i in at] + ["mid"])


@pytest.mark.parametrize("t", hetcases.edge_tables(), ids=lambda t: t.name)
def test_classes_and_find_equal_the_full_form_and_the_oracle(engine, t):
    from oracle import oracle as orc
    sv, fv = t.sites_view(), t.family_view()
    dv = sitecases.dnms_view(_dnms(t))
    for sd in (250, 10 * t.n_sites + 10):  # windows of some fifty sites, and windows that hold the whole table
        P = abi.make_params(search_dist=sd)
        want_cls, want = orc.classify(P, sv, fv) & SNV_BITS, orc.find(P, sv, fv, dv, MODE)
        assert t.n_sites < 64 or sd == 250 or (want[0][-1] > 100 and want[3][-1] > 100)  # (the lists are not empty)
        for het in (False, True):
            sid, fid, keep = _stage(engine, t, het)
            got = engine.find(fid, dv, P, MODE)
            cls = engine.classify(fid, P, t.n_sites)
            engine.free_sites(sid)
            for name, a, b in zip(LISTS, want, got):
                assert np.array_equal(a, np.asarray(b)), (name, "het form" if het else "full form", sd)
            assert np.array_equal(cls & SNV_BITS, want_cls), ("classes", het, np.nonzero((cls & SNV_BITS) != want_cls)[0][:5])
            if het:
                assert not (cls & ~np.uint8(SNV_BITS)).any()  # (no DEL / DUP codes from a het-form family)


def test_broken_het_span_off_raises_the_upload_error(engine):
    t = hetcases.table(3 * 1024 + 5, seed=3)
    dv, P = sitecases.dnms_view(_dnms(t)), abi.make_params(search_dist=250)

    def one_more_in_span_0(hoff):
        hoff[1] += 1  # (ascending, ends at n_het: the host's check passes, the device's count of span 0 and span 1 does not)

    sid, fid, keep = _stage(engine, t, True, hoff_edit=one_more_in_span_0)
    with pytest.raises(UnfazedHipError, match="het_span_off"):
        engine.find(fid, dv, P, MODE)
    engine.free_sites(sid)

    def not_ascending(hoff):
        hoff[1], hoff[2] = hoff[2], hoff[1]

    def short_of_n_het(hoff):
        hoff[-1] -= 1

    for edit in (not_ascending, short_of_n_het):  # what the host checks: refused at the upload
        with pytest.raises(UnfazedHipError, match="het_span_off"):
            _stage(engine, t, True, hoff_edit=edit)
    # and the table itself, unbroken, still works
    sid, fid, keep = _stage(engine, t, True)
    from oracle import oracle as orc
    want = orc.find(P, t.sites_view(), t.family_view(), dv, MODE)
    for a, b in zip(want, engine.find(fid, dv, P, MODE)):
        assert np.array_equal(a, np.asarray(b))
    engine.free_sites(sid)


def test_het_form_needs_the_compact_site_form(engine):
    t = hetcases.table(100)
    c8 = hetcases.columns8(t)
    h9, hoff, _ = io_native.pack_family_het(*c8[:4])
    with pytest.raises(UnfazedHipError, match="compact"):
        engine.upload_sites_family_async(abi.sites_view(t), c8[0], None, None, None, c8[4], het=(h9, hoff))


def test_what_needs_every_sites_columns_is_refused(engine):
    E_STATE = -4
    t = hetcases.table(1025, seed=1)
    P = abi.make_params(search_dist=250)
    dn = _dnms(t)
    dn["vartype"][:] = abi.VT_DEL
    dv = sitecases.dnms_view(dn)
    sid, fid, keep = _stage(engine, t, True)
    engine.set_params(P)
    n = dv.view.n
    co, ho = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    assert engine.L.uz_find(engine.h, fid, dv.ref(), abi.FIND_WHOLE_REGION, co.ctypes.data, ho.ctypes.data) == E_STATE
    cnt, a, b, c = np.zeros(2 * n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert engine.L.uz_phase_cnv(engine.h, fid, dv.ref(), None, cnt.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data) == E_STATE
    groups = engine._groups([(fid, 0, n)])
    assert engine.L.uz_phase_cnv_cohort(engine.h, groups, 1, dv.ref(), None, cnt.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data) == E_STATE
    gt, cols = np.zeros(t.n_sites, np.uint8), np.zeros((9, t.n_sites), np.uint16)
    assert engine.L.uz_family_fetch(engine.h, fid, gt.ctypes.data, cols.ctypes.data) == E_STATE
    with pytest.raises(UnfazedHipError, match="het form"):
        engine.family_fetch(fid, t.n_sites)
    # the family still serves what it was staged for
    from oracle import oracle as orc
    dv = sitecases.dnms_view(_dnms(t))
    for a_, b_ in zip(orc.find(P, t.sites_view(), t.family_view(), dv, MODE), engine.find(fid, dv, P, MODE)):
        assert np.array_equal(a_, np.asarray(b_))
    engine.free_sites(sid)


def test_staged_pass_in_the_het_form_equals_the_plain_forms(engine):
    """run_pipelined over 3 chunks of a small bench load: the het form (BenchLoad.stage's default) against compact_sites=False"""
    from synth.benchload import BenchLoad
    from unfazed_amd.engine import PinnedPool
    ld = BenchLoad(6000, 400000, workload="snv")
    P = abi.make_params()
    engine.set_params(P)
    sid, fid, rid = ld.adopt(engine, P)
    try:
        res, st_ = [], []
        for kw in (dict(), dict(het_sites=False), dict(compact_sites=False)):
            pool = PinnedPool()
            try:
                chunks, st = ld.stage(engine, P, MODE, fid, pool, chunks=3, **kw)
                assert (chunks[0]["sites"][2].get("het") is not None) == (not kw)
                if not kw:
                    n_het, n_chunks = sum(c["sites"][2]["het"][0].size // 9 for c in chunks), len(chunks)
                res.append(pipeline.run_pipelined(engine, P, MODE, ld.n, chunks, cnv=False))
                engine.sync()
                st_.append(st)
            finally:
                pool.free_all()
        for other in res[1:]:
            for k in ("status", "counts", "origin", "evidence"):
                assert np.array_equal(np.asarray(res[0][k]), np.asarray(other[k])), k
        assert (np.asarray(res[0]["status"]) != 0).any() or (np.asarray(res[0]["counts"]) != 0).any()
        ns = st_[0]["sites"]
        print("site bytes per site: het form %.2f, all nine columns %.2f, plain site columns %.2f" % tuple(x["site_bytes"] / ns for x in st_))
        # nine bytes less for every site whose kid is not het; per chunk two columns rounded up to 256 bytes (het9, and het_span_off: a few spans)
        # (this sparse table has ~1.4 window sites per DNM, the DNM's own het site among them: the share of het sites is far above make_sites' 22 %)
        print("kid-het sites: %d of %d" % (n_het, ns))
        assert 0 < n_het < ns
        assert st_[0]["site_bytes"] <= st_[1]["site_bytes"] - 9 * (ns - n_het) + 512 * n_chunks
        assert st_[0]["site_bytes"] >= st_[1]["site_bytes"] - 9 * (ns - n_het)
    finally:
        engine.free_reads(rid)
        engine.free_sites(sid)
        ld.free()
