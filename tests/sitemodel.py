"""The site stage in plain numpy, restated from the reference's Python text: get_position (informative_site_finder.py:10-43),
is_high_quality_site (:46-73), get_kid_allele (:76-134), the per-variant body of find (:239-343) and the decision of summarize_record
(unfazed.py:193-298).  Written for tests/test_site_model.py (held to the C oracle on the CPU) and tests/test_site_edges_gpu.py.

Everything is evaluated the way the reference evaluates it: the allele balance is a float64 quotient (nan and +-inf as numpy gives
them), a window is np.searchsorted on the contig's slice of `pos`, the emitted order is a stable sort of the concatenated windows by
position.  No threshold tables, no ballots, no packed genotype bytes: genotypes, depths and qualities come in as one integer array per
member (kid, dad, mom), a missing depth or quality as -1 (what cyvcf2 hands the reference)."""
import numpy as np

from unfazed_amd import abi

HOM_REF, HET, UNKNOWN, HOM_ALT = 0, 1, 2, 3  # cyvcf2's gt_types codes
KA_NONE, KA_REF_PARENT, KA_ALT_PARENT = 0, 1, 2


def allele_balance(ref, alt):
    """alt / float(ref + alt) (:69, :98-106)"""
    with np.errstate(all="ignore"):
        return np.asarray(alt).astype(np.float64) / (np.asarray(ref) + np.asarray(alt)).astype(np.float64)


def ab_window(P, gt):
    """(min_ab, max_ab) of every site's genotype (:56-61); nan where the genotype is unknown"""
    lo = np.full(gt.shape, np.nan)
    hi = np.full(gt.shape, np.nan)
    for code, w in ((HOM_REF, P.ab_homref), (HOM_ALT, P.ab_homalt), (HET, P.ab_het)):
        lo[gt == code] = w[0]
        hi[gt == code] = w[1]
    return lo, hi


def is_high_quality(P, gt, ref, alt, gq):
    lo, hi = ab_window(P, gt)
    ab = allele_balance(ref, alt)
    with np.errstate(invalid="ignore"):
        inside = (lo <= ab) & (ab <= hi)
    return (gt != UNKNOWN) & (gq >= P.min_gt_qual) & ((ref + alt) >= P.min_depth) & inside


def kid_allele(P, vartype, gt, ref, alt):
    """get_kid_allele for one vartype on every site; gt / ref / alt: [3][n] in kid, dad, mom order -> KA_* codes"""
    n = gt.shape[1]
    out = np.zeros(n, np.int64)
    kt = ref[0] + alt[0]
    if vartype == abi.VT_DEL:
        deep = kt > 4  # :80
        out[deep & (gt[0] == HOM_ALT)] = KA_REF_PARENT
        out[deep & (gt[0] == HOM_REF)] = KA_ALT_PARENT
    elif vartype == abi.VT_DUP:
        ok = (ref[0] > 2) & (alt[0] > 2) & (kt > P.min_depth) & (gt[0] == HET)  # :89-97
        k, d, m = (allele_balance(ref[i], alt[i]) for i in range(3))
        with np.errstate(invalid="ignore"):
            s = d + m
            shared = ((s < 1) & (k > 0.5)) | ((s > 1) & (k < 0.5))  # :110-116
            out[ok & ~shared & (k >= 0.67)] = KA_ALT_PARENT
            out[ok & ~shared & ~(k >= 0.67) & (k <= 0.33)] = KA_REF_PARENT
    return out


def site_facts(P, complex_, gt, ref, alt, gq):
    """what the per-variant body (:239-339) decides about a site before it knows the DNM -> dict of bool / code arrays"""
    hq = [is_high_quality(P, gt[i], ref[i], alt[i], gq[i]) for i in range(3)]
    kid, dad, mom = gt
    alt_dad = (np.isin(dad, (HET, HOM_ALT)) & (mom == HOM_REF)) | ((mom == HET) & (dad == HOM_ALT))  # :307-309, :313-315
    alt_mom = ~alt_dad & ((np.isin(mom, (HET, HOM_ALT)) & (dad == HOM_REF)) | ((dad == HET) & (mom == HOM_ALT)))
    usable = ~complex_
    parents = hq[1] & hq[2]
    het = usable & (kid == HET) & parents  # :268-284
    informative = usable & parents & (alt_dad | alt_mom)
    cand = informative & (kid == HET) & hq[0]  # :292-295
    # :324-337
    hemi = np.isin(kid, (HOM_ALT, HOM_REF))
    het_in = (dad == HET) | (mom == HET)
    hom_in = np.isin(dad, (HOM_ALT, HOM_REF)) | np.isin(mom, (HOM_ALT, HOM_REF))
    clash = (np.isin(dad, (HOM_ALT, HOM_REF)) & (kid == dad)) | (np.isin(mom, (HOM_ALT, HOM_REF)) & (kid == mom))
    unique = ~(hemi & het_in & hom_in & clash)
    ka_del = np.where(informative & unique, kid_allele(P, abi.VT_DEL, gt, ref, alt), 0)
    ka_dup = np.where(informative & unique, kid_allele(P, abi.VT_DUP, gt, ref, alt), 0)
    return dict(hq=hq, het=het, cand=cand, alt_dad=usable & alt_dad, ka_del=ka_del, ka_dup=ka_dup)


def classes(P, complex_, gt, ref, alt, gq):
    """the facts as the class byte the library hands out (include/uz_types.h UZ_CL_*)"""
    f = site_facts(P, complex_, gt, ref, alt, gq)
    c = f["het"] * abi.CL_HET + f["cand"] * abi.CL_CAND + f["alt_dad"] * abi.CL_ALT_DAD
    c = c + (f["ka_del"] << abi.CL_DEL_SHIFT) + (f["ka_dup"] << abi.CL_DUP_SHIFT)
    return c.astype(np.uint8)


def windows(sd, mode, st, en):
    """get_position: 1-based inclusive POS windows (a region start below 1 is 1)"""
    if mode & abi.FIND_WHOLE_REGION:
        w = [(st - sd, en + sd)]
    else:
        w = [(st - sd, st + sd)]
        if (mode & abi.FIND_SECOND_WINDOW) and (en - st) > sd:
            w.append((en - sd, en + sd))
    return [(max(a, 1), b) for a, b in w]


def window_ranges(sd, mode, pos, contig_off, contig, st, en):
    """index range [i0, i1) of each window in the whole table; [] for a contig the table does not have"""
    n_contigs = len(contig_off) - 1
    if contig < 0 or contig >= n_contigs:
        return []
    clo, chi = int(contig_off[contig]), int(contig_off[contig + 1])
    p = pos[clo:chi]
    out = []
    for a, b in windows(sd, mode, st, en):
        i0 = int(np.searchsorted(p, a - 1, "left"))  # POS = pos + 1 >= a
        i1 = int(np.searchsorted(p, b - 1, "right"))  # POS <= b
        out.append((clo + i0, clo + max(i0, i1)))
    return out


def find(P, mode, cls, pos, contig_off, dn):
    """cls: classes() of the table.  dn: dict of contig, start, end, vartype, mult.
    -> cand_off, cand_idx, cand_flags, het_off, het_idx, and the window index ranges of every DNM"""
    sd = int(P.search_dist)
    whole = bool(mode & abi.FIND_WHOLE_REGION)
    is_het = (cls & abi.CL_HET) != 0
    alt_dad = (cls & abi.CL_ALT_DAD) != 0
    ka_of = {abi.VT_DEL: (cls >> abi.CL_DEL_SHIFT) & 3, abi.VT_DUP: (cls >> abi.CL_DUP_SHIFT) & 3}
    zero = np.zeros(len(cls), np.uint8)
    cand_simple = (cls & abi.CL_CAND) != 0
    n = len(dn["start"])
    ci, cf, hi, rng = [], [], [], []
    co, ho = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    seen = {}
    for d in range(n):
        key = (int(dn["contig"][d]), int(dn["start"][d]), int(dn["end"][d]), int(dn["vartype"][d]), int(dn["mult"][d]))
        if key not in seen:
            c, st, en, vt, mult = key
            r = window_ranges(sd, mode, pos, contig_off, c, st, en)
            idx = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in r] + [np.zeros(0, np.int64)])
            idx = idx[np.argsort(pos[idx], kind="stable")]  # :341-342
            if en - st < 20:  # :253-256
                idx = idx[~((pos[idx] >= st) & (pos[idx] < en))]
            ka = ka_of.get(vt, zero) if whole else zero
            is_c = (ka[idx] != 0) if whole else cand_simple[idx]
            c_idx, h_idx = np.repeat(idx[is_c], mult), np.repeat(idx[is_het[idx]], mult)
            fl = (alt_dad[c_idx] * abi.CF_ALT_DAD + (ka[c_idx].astype(np.int64) << abi.CF_KA_SHIFT)).astype(np.uint8)
            seen[key] = (c_idx.astype(np.int32), fl, h_idx.astype(np.int32), r)
        a, b, c2, r = seen[key]
        ci.append(a); cf.append(b); hi.append(c2); rng.append(r)
        co[d + 1], ho[d + 1] = co[d] + len(a), ho[d] + len(c2)
    cat = lambda xs, dt: np.concatenate(xs + [np.zeros(0, dt)]).astype(dt)  # noqa: E731
    return co, cat(ci, np.int32), cat(cf, np.uint8), ho, cat(hi, np.int32), rng


def summarize(dad_reads, mom_reads, dad_sites, mom_sites, cnv_dad, cnv_mom, ratio):
    """summarize_record's decision on counts -> (origin code, evidence count, evidence types as a list, ambig)"""
    origin, evidence, types, ambig = None, 0, [], False
    if dad_reads > 0 and dad_reads >= ratio * mom_reads:
        origin, evidence = "dad", dad_sites
        types.append("READBACKED")
    elif mom_reads > 0 and mom_reads >= ratio * dad_reads:
        origin, evidence = "mom", mom_sites
        types.append("READBACKED")
    elif dad_reads > 0 and mom_reads > 0:
        origin, evidence = "dad|mom", dad_reads + mom_reads
        types.append("AMBIGUOUS_READBACKED")
        ambig = True
    if cnv_dad > 0 and cnv_dad >= ratio * cnv_mom:
        if origin == "mom" and "READBACKED" not in types:
            origin, types, ambig = None, ["AMBIGUOUS_BOTH"], True
            evidence += cnv_dad + cnv_mom
        else:
            origin, evidence = "dad", cnv_dad
            if "AMBIGUOUS_READBACKED" in types:
                types.remove("AMBIGUOUS_READBACKED")
                ambig = False
            types.append("ALLELE-BALANCE")
    elif cnv_mom > 0 and cnv_mom >= ratio * cnv_dad:
        if origin == "dad" and "READBACKED" not in types:
            origin, types, ambig = None, ["AMBIGUOUS_BOTH"], True
            evidence += cnv_dad + cnv_mom
        else:
            origin, evidence = "mom", cnv_mom
            if "AMBIGUOUS_READBACKED" in types:
                types.remove("AMBIGUOUS_READBACKED")  # (`ambig` stays as it is, :286-287)
            types.append("ALLELE-BALANCE")
    elif cnv_dad + cnv_mom > 0 and "READBACKED" not in types:
        origin = None
        evidence += cnv_dad + cnv_mom
        types.append("AMBIGUOUS_ALLELE-BALANCE")
        ambig = True
    return origin, evidence, types, ambig


ORIGIN_CODE = {None: abi.OR_NONE, "dad": abi.OR_DAD, "mom": abi.OR_MOM, "dad|mom": abi.OR_AMBIGUOUS}
TYPE_BIT = {name: bit for bit, name in abi.ET_NAMES}


def phase_cnv(P, cls, pos, contig_off, dn, rb_counts=None):
    """run_cnv_phasing's find(search_dist=0, whole_region=True), phase_by_snvs' vote (sv_phaser.py:71-85: a candidate names the parent
    its kid_allele points at) and summarize's decision -> the dict of oracle.phase_cnv plus the branch labels"""
    import copy
    p0 = copy.copy(P)
    p0.search_dist = 0
    co, ci, cf, ho, hi, _ = find(p0, abi.FIND_WHOLE_REGION, cls, pos, contig_off, dn)
    n = len(dn["start"])
    cnt = np.zeros((n, 2), np.int32)
    origin, evidence, etype = (np.zeros(n, np.int32) for _ in range(3))
    lists, labels = [], []
    for d in range(n):
        dad_pos = mom_pos = np.zeros(0, np.int32)
        if int(dn["vartype"][d]) in (abi.VT_DEL, abi.VT_DUP):  # sv_phaser.py:401
            idx, fl = ci[co[d]:co[d + 1]], cf[co[d]:co[d + 1]]
            names_alt = ((fl >> abi.CF_KA_SHIFT) & 3) == KA_ALT_PARENT
            is_dad = names_alt == ((fl & abi.CF_ALT_DAD) != 0)
            dad_pos, mom_pos = pos[idx[is_dad]], pos[idx[~is_dad]]
        rb = [int(x) for x in rb_counts[d]] if rb_counts is not None else [0, 0, 0, 0]
        o, ev, types, ambig = summarize(rb[0], rb[1], rb[2], rb[3], len(dad_pos), len(mom_pos), int(P.evidence_min_ratio))
        cnt[d] = len(dad_pos), len(mom_pos)
        origin[d], evidence[d] = ORIGIN_CODE[o], ev
        etype[d] = sum(TYPE_BIT[t] for t in types) | (abi.ET_AMBIG_FLAG if ambig else 0)
        lists.append((dad_pos, mom_pos))
        labels.append("+".join(types) if types else "NONE")
    return dict(cnv_counts=cnt, origin=origin, evidence=evidence, etype=etype, lists=lists, labels=labels)
