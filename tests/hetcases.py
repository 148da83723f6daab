"""Edge tables for the het form of a trio's genotype columns (uz_types.h: uz_family_view.het9 ...), shared by tests/test_family_het_form.py
(packer and host twin, no GPU) and tests/test_family_het_form_gpu.py (the device's expansion against the full form and the oracle).
Pure numpy on top of tests/sitecases.py."""
import numpy as np

import sitecases
from sitemodel import HET, HOM_ALT, HOM_REF

SPAN = 1024
SIZES = (1, 1023, 1024, 1025, 2049)


def table(n, seed=0, no_het_span=None, all_het_span=None, deep_het=(), name=None):
    """n sites whose genotype bytes walk through all 64 values (site i: byte (i + seed) % 64, so every span holds each of them when n >= 64);
    depths 0 .. 60 with a missing value now and then, GQ 15 .. 99 or missing.  no_het_span / all_het_span: the kid of every site of that
    span is made hom-ref / het.  deep_het: sites made kid-het with a kid depth the eight-bit columns cannot hold (the wide list)."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    b = (np.arange(n) + seed) % 64
    gt = np.stack([b & 3, b >> 2 & 3, b >> 4 & 3]).astype(np.int64)
    lo, hi = lambda s: s * SPAN, lambda s: min(n, (s + 1) * SPAN)  # noqa: E731
    if no_het_span is not None:
        k = gt[0, lo(no_het_span): hi(no_het_span)]
        k[k == HET] = HOM_REF
    if all_het_span is not None:
        gt[0, lo(all_het_span): hi(all_het_span)] = HET
    # depths that mostly fit the genotype (so that candidates and usable het sites exist), a fifth of them drawn blind
    rd = np.where(gt == HET, rng.integers(10, 41, (3, n)), np.where(gt == HOM_REF, rng.integers(20, 61, (3, n)), rng.integers(0, 4, (3, n))))
    ad = np.where(gt == HET, rng.integers(10, 41, (3, n)), np.where(gt == HOM_REF, rng.integers(0, 4, (3, n)), rng.integers(20, 61, (3, n))))
    gq = rng.integers(15, 100, (3, n))
    blind = rng.random((3, n)) < 0.2
    rd, ad = np.where(blind, rng.integers(0, 61, (3, n)), rd), np.where(blind, rng.integers(0, 61, (3, n)), ad)
    for x in (rd, ad, gq):
        x[rng.random((3, n)) < 0.03] = -1
    for i in deep_het:
        gt[0, i] = HET
        rd[0, i], ad[0, i] = 40000, 39000  # (beyond 16 bits as well: the class comes from the wide list's exact depths)
        gt[1, i], gt[2, i] = HOM_REF, HOM_ALT  # (a candidate: its class bits come from the wide list alone)
        rd[1, i], ad[1, i], rd[2, i], ad[2, i], gq[:, i] = 30, 1, 1, 30, 99
    return sitecases.Table(name or "het_n%d_s%d" % (n, seed), gt, rd, ad, gq, complex_=rng.random(n) < 0.05)


def edge_tables():
    out = [table(n) for n in SIZES]
    out.append(table(3 * SPAN + 5, seed=3, no_het_span=1, name="span_without_het"))
    out.append(table(2 * SPAN + 77, seed=5, all_het_span=1, name="span_of_het_only"))
    out.append(table(SPAN + 300, seed=9, deep_het=(0, 1023, 1024, SPAN + 299), name="wide_het_sites"))
    return out


def columns8(t):
    """-> (gt, rd8, ad8, gq8, wide) of a sitecases.Table: the eight-bit link form (abi.family_columns8)"""
    from unfazed_amd import abi
    r8, a8, g8, wide = abi.family_columns8(t.rd, t.ad, t.gq, t.wide)
    return t.gt, list(r8), list(a8), list(g8), wide


def widened(c8):
    """what k_widen8 writes for the eight-bit columns: u16 [9][n]"""
    _, r8, a8, g8, _ = c8
    wid = lambda x, miss: np.where(x == miss, np.uint16(0xFFFF), x.astype(np.uint16))  # noqa: E731
    return np.stack([wid(x, 254) for x in r8] + [wid(x, 254) for x in a8] + [wid(x, 255) for x in g8])
