"""The link forms of a site window on the device, held to the model of tests/siteformmodel.py (written from uz_types.h) on the hand-built
tables of tests/siteformcases.py: what k_sites_expand, k_widen8 and k_fold_complex write is read back (uz_sites_fetch, uz_family_fetch) and
compared cell by cell, in every order of first use of a table and its family; the classes and window lists of the tables whose positions
ascend are the C oracle's; what the upload must refuse is refused, and the same view unbroken then works on the same engine.
tests/test_site_form_model.py holds the model and the tables themselves, on the CPU.  Every comparison is np.array_equal; the only cells
left out are the 16-bit depth cells the header leaves open (depth byte 255: the site's depths stand in the wide list)."""
import time
from types import SimpleNamespace

import numpy as np
import pytest

import siteformcases as sfc
import siteformmodel as sfm
import sitecases
from siteformmodel import SPAN
from unfazed_amd import abi, io_native
from unfazed_amd.engine import UnfazedHipError

pytestmark = pytest.mark.gpu

CASES = sfc.cases()
BY = {c.name: c for c in CASES}
COLS = ("pos", "sflags", "ref_base", "alt_base")
LISTS = ("cand_off", "cand_idx", "cand_flags", "het_off", "het_idx")
MODE = abi.FIND_SECOND_WINDOW
SNV_BITS = 0x07  # UZ_CL_HET | UZ_CL_CAND | UZ_CL_ALT_DAD: what a het-form family classifies
E_ARG = r"\(-1\)"  # UZ_E_ARG in the engine's error text
_T0 = time.time()


def check_sites(engine, sid, c, what):
    got = engine.sites_fetch(sid, c.n)
    for name, g, w in zip(COLS, got, c.model()):
        assert g.dtype == w.dtype and np.array_equal(g, w), (c.name, what, name, np.nonzero(g != w)[0][:5])


def check_family(engine, fid, c, what):
    gt, cols = engine.family_fetch(fid, c.n)
    want, open_ = sfm.widen8(c.cols8())
    assert np.array_equal(gt, sfm.folded_gt(c.c8[0], c.model()[1])), (c.name, what, "gt")
    assert np.array_equal(np.where(open_, 0, cols), np.where(open_, 0, want)), (c.name, what, np.argwhere(np.where(open_, 0, cols) != np.where(open_, 0, want))[:5])


def stage8(engine, c, held=None):
    gt, rd8, ad8, gq8, wide = c.c8
    return engine.upload_sites_family_async(held or c.held, gt, rd8, ad8, gq8, wide)


def stage_het(engine, c):
    gt, rd8, ad8, gq8, wide = c.c8
    h9, hoff, _ = io_native.pack_family_het(gt, rd8, ad8, gq8)
    sid, fid = engine.upload_sites_family_async(c.held, gt, None, None, None, wide, het=(h9, hoff))
    return sid, fid, (h9, hoff)


def columns16(c):
    """the trio in the 16-bit columns (an open cell holds the byte itself: the wide list overrides it)"""
    w, _ = sfm.widen8(c.cols8())
    return c.c8[0], w[0:3], w[3:6], w[6:9], c.c8[4]


_ORACLE = {}


def oracle_of(c, sd):
    """-> (params, DNM view or None, classes, find lists or None) of the C oracle on the model's plain columns; computed once per case"""
    if (c.name, sd) not in _ORACLE:
        from oracle import oracle as orc
        pos, sf, rb, ab = c.model()
        contigs = ["c%d" % k for k in range(c.parts["contig_off"].size - 1)]
        sv = abi.sites_view(SimpleNamespace(contig_off=c.parts["contig_off"], pos=pos, sflags=sf, ref_base=rb, alt_base=ab, n_sites=c.n, contigs=contigs))
        fv = abi.family_view(*columns16(c))
        P = abi.make_params(search_dist=sd)
        dv = sitecases.dnms_view(sfc.dnms_of(c)) if c.ascends() else None
        _ORACLE[(c.name, sd)] = (P, dv, orc.classify(P, sv, fv), orc.find(P, sv, fv, dv, MODE) if dv is not None else None)
    return _ORACLE[(c.name, sd)]


def check_classes_and_find(engine, fid, c, sd, bits, what):
    P, dv, want_cls, want = oracle_of(c, sd)
    if dv is not None:  # (find reads positions that ascend within a contig; the classes are a site's own)
        got = engine.find(fid, dv, P, MODE)
        for name, a, b in zip(LISTS, want, got):
            assert np.array_equal(a, np.asarray(b)), (c.name, what, sd, name)
    cls = engine.classify(fid, P, c.n)
    assert np.array_equal(cls & bits, want_cls & bits), (c.name, what, sd, np.nonzero((cls & bits) != (want_cls & bits))[0][:5])


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_family_first(engine, c):
    """compact sites + eight-bit columns; the family's first use expands both in one launch"""
    sid, fid = stage8(engine, c)
    check_family(engine, fid, c, "family first")
    check_sites(engine, sid, c, "family first")
    engine.free_sites(sid)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_sites_first_then_the_staged_family(engine, c):
    """(a) the sites are fetched before the family's first use: expanded without it, the family then takes k_widen8 + k_fold_complex"""
    sid, fid = stage8(engine, c)
    check_sites(engine, sid, c, "sites first")
    check_family(engine, fid, c, "sites first")
    check_sites(engine, sid, c, "sites first, after the family")
    engine.free_sites(sid)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_another_family_first_then_the_staged_family(engine, c):
    """(b) a second family of the table, uploaded in 16-bit columns, is used before the staged one"""
    sid, fid = stage8(engine, c)
    f16 = engine.add_family(sid, *columns16(c))
    check_family(engine, f16, c, "16-bit family")
    check_classes_and_find(engine, f16, c, 250, 0xFF, "16-bit family")
    check_family(engine, fid, c, "staged family behind a 16-bit one")
    check_classes_and_find(engine, fid, c, 250, 0xFF, "staged family behind a 16-bit one")
    check_sites(engine, sid, c, "behind both families")
    engine.free_sites(sid)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_sites_first_then_the_het_form(engine, c):
    """(c) the het form behind a first use of the sites alone: the table is expanded a second time, now with the het columns"""
    sid, fid, keep = stage_het(engine, c)
    check_sites(engine, sid, c, "sites first, het form pending")
    check_classes_and_find(engine, fid, c, 250, SNV_BITS, "het form behind the sites")
    check_sites(engine, sid, c, "after the het form's expansion")
    assert not (engine.classify(fid, oracle_of(c, 250)[0], c.n) & ~np.uint8(SNV_BITS)).any()
    engine.free_sites(sid)


PLAIN8 = [c for c in CASES if c.name.startswith(("family_", "bases_")) or c.name in ("size_1", "size_255", "size_256", "size_257", "size_1027")]


@pytest.mark.parametrize("c", PLAIN8, ids=repr)
def test_plain_sites_with_eight_bit_columns(engine, c):
    """the async route without the compact form: k_widen8 and k_fold_complex alone"""
    assert c.want is not None
    plain = abi.sites_view(SimpleNamespace(contig_off=c.parts["contig_off"], pos=c.want[0], sflags=c.want[1], ref_base=c.want[2], alt_base=c.want[3],
                                           n_sites=c.n, contigs=[""] * (c.parts["contig_off"].size - 1)))
    sid, fid = stage8(engine, c, held=plain)
    check_family(engine, fid, c, "plain sites, eight-bit columns")
    check_sites(engine, sid, c, "plain sites")
    engine.free_sites(sid)


def test_plain_eight_bit_cases_hold_the_sizes():
    assert {1, 255, 256, 257} <= {c.n for c in PLAIN8} and len(PLAIN8) == 12


@pytest.mark.parametrize("c", sfc.world_cases(), ids=repr)
def test_world_tables_against_the_oracle(engine, c):
    """compact + eight-bit and compact + het form, a search distance of 250 and one that covers the table, both orders of first use"""
    cover = int(c.table.pos.max()) + 10
    for sd in (250, cover):
        P, dv, _, want = oracle_of(c, sd)
        assert dv is not None and want[0][-1] > 0 and want[3][-1] > 0 and (sd == 250 or want[3][-1] > 100)  # (the lists are not empty)
        for het in (False, True):
            for sites_first in (False, True):
                sid, fid = (stage_het(engine, c)[:2] if het else stage8(engine, c))
                if sites_first:
                    check_sites(engine, sid, c, "world, sites first")
                check_classes_and_find(engine, fid, c, sd, SNV_BITS if het else 0xFF, "world het=%d sites_first=%d" % (het, sites_first))
                check_sites(engine, sid, c, "world")
                engine.free_sites(sid)


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def _refused_then_accepted(engine, src, match=E_ARG, plain_too=False, **edit):
    """the edited view is refused with UZ_E_ARG; the same view unbroken then expands to the model's columns on the same engine"""
    flags = {k: edit.pop(k) for k in ("null_span", "n_pos_esc") if k in edit}
    bad = sfc.hand_view(**dict(src.parts, **edit), **flags)
    if plain_too:
        bad.view.pos = src.want[0].ctypes.data
    with pytest.raises(UnfazedHipError, match=match):
        stage8(engine, src, held=bad)
    sid, fid = stage8(engine, src, held=sfc.hand_view(**src.parts))
    check_sites(engine, sid, src, "unbroken")
    check_family(engine, fid, src, "unbroken")
    engine.free_sites(sid)


def test_refusals(engine):
    src = BY["contig_starts_l0_l1_l1023"]
    S, n = SPAN, src.n
    idx, val, off = [int(e) for e in src.parts["eidx"]], [int(v) for v in src.parts["eval"]], [int(o) for o in src.parts["eoff"]]
    assert idx == [S + 1, 2 * S + 1023] and off == [0, 0, 1, 2, 2] and n == 3 * S + 5
    bad = lambda **e: _refused_then_accepted(engine, src, **e)  # noqa: E731
    bad(eidx=[S + 1, 2 * S - 1])  # an escape below its span
    bad(eidx=[2 * S + 5, 2 * S + 1023])  # ... above its span
    for beyond in (n, n + 100):  # ... at or beyond n in the partial last span
        bad(eidx=idx + [beyond], eval=val + [7], eoff=[0, 0, 1, 2, 3])
    bad(eidx=idx + [2 * S + 1023], eval=val + [7], eoff=[0, 0, 1, 3, 3])  # two escapes with equal indices
    bad(eidx=[S + 1, 2 * S + 1023, 2 * S + 7], eval=val + [7], eoff=[0, 0, 1, 3, 3])  # ... that descend
    bad(eoff=[0, 2, 1, 2, 2])  # pos_esc_off that descends
    bad(eoff=[1, 1, 1, 2, 2], match="pos_esc_off")  # ... that starts at 1
    bad(eoff=[0, 0, 1, 1, 1], match="pos_esc_off")  # ... that ends short of n_pos_esc
    bad(null_span=True, match="span_pos")  # a missing span_pos
    bad(plain_too=True, match="compact sites view")  # plain and compact pointers both set
    bad(eidx=[S, 2 * S + 1023], match="first site")  # an escape at its span's first site: the kernel takes span_pos there
    bad(eidx=[S + 1, 2 * S], match="first site")
    with pytest.raises(UnfazedHipError, match="compact site form"):  # the compact form given to uz_sites_upload
        engine.upload_sites_view(src.held)


def test_no_sites(engine):
    c = sfc.packed("no_sites", np.zeros(0, np.int64), [0, 0, 0])
    assert c.n == 0 and c.parts["eoff"].tolist() == [0]
    sid, fid = stage8(engine, c)
    assert all(x.size == 0 for x in engine.sites_fetch(sid, 0))
    gt, cols = engine.family_fetch(fid, 0)
    assert gt.size == 0 and cols.shape == (9, 0)
    engine.free_sites(sid)


def test_table_freed_before_its_first_use(engine):
    c = BY["world_a"]
    for stage in (stage8, lambda e, c: stage_het(e, c)[:2]):
        sid, fid = stage(engine, c)
        engine.free_sites(sid)  # (the copies are queued: the free waits for them; the expansion never runs)
        with pytest.raises(UnfazedHipError, match=E_ARG):
            engine.sites_fetch(sid, c.n)
    sid, fid = stage8(engine, c)  # and the engine goes on
    check_family(engine, fid, c, "after a free")
    check_sites(engine, sid, c, "after a free")
    engine.free_sites(sid)


def test_wall_time_of_this_file(engine):
    """reported, not asserted: the file is meant to run in seconds"""
    print("tests/test_site_forms_gpu.py: %.1f s from import to here, %d cases" % (time.time() - _T0, len(CASES)))
