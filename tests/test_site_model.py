"""The numpy model of the site stage (tests/sitemodel.py: the reference's Python restated with float64 quotients and np.searchsorted)
against the C oracle on every hand-built case of tests/sitecases.py, and the proof -- from the model alone -- that the cases reach the
edges they are named for.  No GPU.  tests/test_site_edges_gpu.py holds the device to the oracle on the same cases; this file must pass
before that one is trusted.  No case is skipped or filtered: every table, parameter set and batch the GPU file runs is compared here.

A shape the issue names that cannot occur: summarize_record's AMBIGUOUS_BOTH (unfazed.py:241-248, :267-276).  It needs origin_parent to be
one parent without "READBACKED" among the evidence types, and the read-backed branches set a single parent only together with
"READBACKED"; the model agrees with k_cnv_count's comment, and test_every_decision_label_occurs asserts that it never comes out."""
import itertools

import numpy as np
import pytest

import sitecases
import sitemodel
from oracle import oracle as orc
from unfazed_amd import abi

LISTS = ("cand_off", "cand_idx", "cand_flags", "het_off", "het_idx")


def _classes_equal(t, kw, what):
    P = abi.make_params(**kw)
    want, got = orc.classify(P, t.sites_view(), t.family_view()), t.model_classes(P)
    if not np.array_equal(want, got):
        i = np.nonzero(want != got)[0]
        raise AssertionError("%s: %d sites differ, first %s: oracle %s model %s" % (what, i.size, i[:5].tolist(), want[i[:5]].tolist(), got[i[:5]].tolist()))


# ------------------------------------------------------------------------------------------------------------------------ model = oracle
def test_classes_of_the_threshold_table():
    t = sitecases.threshold_table()
    for name, kw in sitecases.k1_param_sets():
        _classes_equal(t, kw, name)


def test_classes_of_the_shape_and_wide_tables():
    for t in sitecases.shape_tables() + [sitecases.big_table()]:
        for name, kw in sitecases.SHAPE_PARAMS:
            _classes_equal(t, kw, "%s, %s" % (t.name, name))
    for t in sitecases.wide_tables():
        for name, kw in sitecases.WIDE_PARAMS:
            _classes_equal(t, kw, "%s, %s" % (t.name, name))


def test_classes_of_the_batch_families():
    fams = sitecases.batch_tables()
    assert len({int(t.idx[0]) for t in fams}) == len(fams)  # every family another walk
    for k, t in enumerate(fams):
        for name, kw in (sitecases.SHAPE_PARAMS[0], sitecases.SHAPE_PARAMS[2]):
            _classes_equal(t, kw, "family %d, %s" % (k, name))


def _lists_equal(t, P, mode, dn, what):
    want = orc.find(P, t.sites_view(), t.family_view(), sitecases.dnms_view(dn), mode)
    got = sitemodel.find(P, mode, t.model_classes(P), t.pos, t.contig_off, dn)
    for name, a, b in zip(LISTS, want, got):
        assert np.array_equal(a, b), "%s: %s differs" % (what, name)
    return got


@pytest.mark.parametrize("sd,mode", sitecases.WINDOW_RUNS)
def test_window_lists(sd, mode):
    t = sitecases.window_table(bool(mode & abi.FIND_WHOLE_REGION))
    got = _lists_equal(t, abi.make_params(search_dist=sd), mode, sitecases.window_dnms(mode), "sd %d mode %d" % (sd, mode))
    assert got[0][-1] > 100 and got[3][-1] > 100


def test_window_lists_of_the_batches():
    t = sitecases.window_table(False)
    for size in sitecases.BATCH_SIZES:
        dn = sitecases.batch_dnms(size)
        co = _lists_equal(t, abi.make_params(search_dist=5), abi.FIND_SECOND_WINDOW, dn, "batch of %d" % size)[0]
        cnt = np.diff(co)
        for edge in range(4096, size, 4096):  # zero counts on both sides of every tile edge, counts beside them
            assert cnt[edge - 1] == 0 and cnt[edge] == 0 and cnt[edge - 2] > 0 and (edge + 1 >= size or cnt[edge + 1] > 0)


@pytest.fixture(scope="module")
def cnv_results():
    t, _ = sitecases.cnv_world()
    out = {}
    for ratio in sitecases.RATIOS:
        P = abi.make_params(evidence_min_ratio=ratio)
        cls = t.model_classes(P)
        for name, dn, rb in sitecases.cnv_cases():
            want = orc.phase_cnv(P, t.sites_view(), t.family_view(), sitecases.dnms_view(dn), rb)
            out[ratio, name] = (want, sitemodel.phase_cnv(P, cls, t.pos, t.contig_off, dn, rb), dn)
    return out


def test_cnv_counts_lists_and_decisions(cnv_results):
    for (ratio, name), (want, got, dn) in cnv_results.items():
        for k in ("cnv_counts", "origin", "evidence", "etype"):
            assert np.array_equal(want[k], got[k]), (ratio, name, k)
        for d in range(len(dn["start"])):
            for j in range(2):
                assert np.array_equal(want["lists"][d][j], got["lists"][d][j]), (ratio, name, d, j)


# ----------------------------------------------------------------------------------------------------- the cases reach what they claim
def _dad_block():
    """the rows that vary dad (good GQ): his genotype, total, alt depth and the full columns"""
    t = sitecases.threshold_table()
    gt, rd, ad, gq = (x[:, : t.n_threshold_rows] for x in t.true)
    third = t.n_threshold_rows // 3
    sel = np.zeros(t.n_threshold_rows, bool)
    sel[third: 2 * third] = True
    sel &= gq[1] == sitecases.GOOD_GQ
    return gt[1][sel], rd[1][sel], ad[1][sel], gq[1][sel]


@pytest.mark.parametrize("pname", ["default", "ulp_up", "ulp_down"])
def test_every_threshold_has_both_neighbours_and_a_tie_in_both_ranges(pname):
    """for each genotype's lo and hi, below total 510 (LDS copy of the interval table) and from 510 (global table): two alt depths next to
    each other at one total, one passing and one failing at that bound; under the default set an allele balance exactly on the bound"""
    P = abi.make_params(**dict(sitecases.threshold_sets())[pname])
    g, rd, ad, gq = _dad_block()
    ok = sitemodel.is_high_quality(P, g, rd, ad, gq)
    ab = sitemodel.allele_balance(rd, ad)
    t = rd + ad
    for code, w in ((sitemodel.HOM_REF, P.ab_homref), (sitemodel.HOM_ALT, P.ab_homalt), (sitemodel.HET, P.ab_het)):
        for rng_name, in_rng in (("lds", (t >= P.min_depth) & (t < 510)), ("global", t >= 510)):
            m = (g == code) & in_rng
            state = {(int(tt), int(aa)): bool(o) for tt, aa, o in zip(t[m], ad[m], ok[m])}
            # (the balance rises with the alt depth: a failing depth below a passing one lies under lo, a failing one above it over hi)
            rising = [(tt, aa) for (tt, aa), o in state.items() if o and state.get((tt, aa - 1)) is False]
            falling = [(tt, aa) for (tt, aa), o in state.items() if o and state.get((tt, aa + 1)) is False]
            assert rising and falling, (pname, code, rng_name)
            if pname == "default":
                assert np.any(m & (ab == w[0]) & ok) and np.any(m & (ab == w[1]) & ok), (code, rng_name)
    assert 509 in t and 510 in t and 65534 in t and -2 in t


def test_both_t0_outcomes_occur():
    """infinite thresholds on one genotype, min_depth 0: total 0 passes with a missing depth (+-inf) and fails with rd = ad = 0 (nan)"""
    P = abi.make_params(**sitecases.SHAPE_PARAMS[2][1])
    assert np.isinf(P.ab_het[0]) and np.isinf(P.ab_het[1]) and P.min_depth <= 0
    g, rd, ad, gq = _dad_block()
    ok = sitemodel.is_high_quality(P, g, rd, ad, gq)
    het0 = (g == sitemodel.HET) & (rd + ad == 0)
    assert np.any(het0 & (rd == 0) & (ad == 0) & ~ok) and not np.any(het0 & (rd == 0) & ok)
    assert np.any(het0 & (rd == -1) & (ad == 1) & ok) and np.any(het0 & (rd == 1) & (ad == -1) & ok)
    for t in sitecases.wide_tables()[2:]:  # ... and in the wide list
        ws, wr, wa = t.wide
        assert np.any((wr == 0) & (wa == 0)) and np.any((wr + wa == 0) & (wa == 1))
        assert {int(x) for x in sitecases.WIDE_DEPTHS} <= {int(x) for x in np.concatenate([wr.ravel(), wa.ravel()])}
        assert t.complex[ws].any() and (t.true[0][:, ws] == sitemodel.UNKNOWN).any() and ws[0] == 0 and ws[-1] == t.n_sites - 1
    assert [t.wide[0].size for t in sitecases.wide_tables()] == [1, 1, 256, 257]


def test_grids_stride():
    chunks = lambda n: (n + sitecases.CHUNK - 1) // sitecases.CHUNK  # noqa: E731
    assert chunks(sitecases.BIG_N) > 4096 + 1 and sitecases.BIG_N % sitecases.CHUNK % 8 != 0
    per_family = max((4096 + sitecases.BATCH_FAMS - 1) // sitecases.BATCH_FAMS, 16)
    assert chunks(sitecases.BATCH_N) > per_family and sitecases.BATCH_N % 8 != 0
    # no smaller family count strides on fewer sites in all: below 256 families a family gets 4096 / n_fam workgroups
    assert all(nf * (max(-(-4096 // nf), 16) * sitecases.CHUNK + 1) >= 4096 * sitecases.CHUNK for nf in range(2, 257))


def test_window_sizes_and_two_window_forms_occur():
    t = sitecases.window_table(False)
    sizes = {"wave": set(), "region": set()}
    forms = set()
    for sd, mode in sitecases.WINDOW_RUNS:
        dn = sitecases.window_dnms(mode)
        for d in range(len(dn["start"])):
            st, en, mult = int(dn["start"][d]), int(dn["end"][d]), int(dn["mult"][d])
            r = sitemodel.window_ranges(sd, mode, t.pos, t.contig_off, int(dn["contig"][d]), st, en)
            sizes["region" if mode & abi.FIND_WHOLE_REGION else "wave"] |= {b - a for a, b in r}
            w = sitemodel.windows(sd, mode, st, en)
            if len(w) == 2 and sd > 0:
                form = "overlap" if w[1][0] <= w[0][1] else ("adjacent" if w[1][0] == w[0][1] + 1 else "apart")
                forms.add((sd, form, mult > 1, en - st < 20))
            elif sd > 0 and (mode & abi.FIND_SECOND_WINDOW):
                forms.add((sd, "one", mult > 1, en - st < 20))
    for kind in ("wave", "region"):
        assert set(sitecases.WINDOW_SITES) <= sizes[kind], (kind, sorted(set(sitecases.WINDOW_SITES) - sizes[kind]))
    for sd in (5, 5000):
        for form in ("one", "overlap", "adjacent", "apart"):
            assert any(f[:3] == (sd, form, True) for f in forms), (sd, form)
    assert (5, "overlap", False, True) in forms and (5, "apart", False, True) in forms  # two windows with small-event exclusion (en - st of 6 and 19)
    assert (5, "apart", False, False) in forms
    # the contigs, and none of them starts on a multiple of 64
    sz = np.diff(t.contig_off).tolist()
    assert all(n in sz for n in sitecases.CONTIG_SIZES) and all(int(o) % 64 for o in t.contig_off[1:-1])
    # an equal run lies across every first-round probe of the 64-ary search
    for c, n in enumerate(sz):
        if n in sitecases.CONTIG_SIZES and n > 64:
            p = t.pos[t.contig_off[c]: t.contig_off[c + 1]]
            assert all(p[q - 1] == p[q] for q in sitecases.probe_indices(n))


def test_every_decision_label_occurs(cnv_results):
    labels, flagged, totals = set(), set(), set()
    ties = {r: False for r in sitecases.RATIOS}
    for (ratio, name), (want, got, dn) in cnv_results.items():
        labels |= set(got["labels"])
        flagged |= {int(e) for e in got["etype"]}
        c = got["cnv_counts"].astype(np.int64)
        totals |= set(c.sum(axis=1).tolist())
        ties[ratio] |= bool(np.any((c[:, 1] > 0) & (c[:, 0] == ratio * c[:, 1])) and np.any((c[:, 0] > 0) & (c[:, 1] == ratio * c[:, 0])))
    assert labels == {"NONE", "READBACKED", "ALLELE-BALANCE", "READBACKED+ALLELE-BALANCE", "AMBIGUOUS_READBACKED", "AMBIGUOUS_ALLELE-BALANCE",
                      "AMBIGUOUS_READBACKED+AMBIGUOUS_ALLELE-BALANCE"}
    assert (abi.ET_ALLELE_BALANCE | abi.ET_AMBIG_FLAG) in flagged and abi.ET_ALLELE_BALANCE in flagged  # mom's branch keeps `ambig`, dad's clears it
    assert {64, 65, 128, 130, 260} <= totals and all(ties.values())
    # AMBIGUOUS_BOTH cannot come out of summarize_record's branches: no counts give it
    for ratio in sitecases.RATIOS:
        for dr, mr, cd, cm in itertools.product(range(0, 13), repeat=4):
            assert "AMBIGUOUS_BOTH" not in sitemodel.summarize(dr, mr, 1, 1, cd, cm, ratio)[2]
