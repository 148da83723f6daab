"""The host path's two routes through the site stage: a batch that names two or more kids makes ONE device call for its find
(uz_find_cohort) and one for its allele-balance stage (uz_phase_cnv_cohort); UZ_FIND_ROUTE=kid, or a single kid, makes one per kid as
before.  Both routes leave the same records and the same annotated DNMs, the reference's two-kid golden among them."""
import contextlib
import copy
import io
import json
import os

import numpy as np
import pytest

from helpers import RUN_DEFAULTS, norm_records, params_from, tables
from oracle_backend import OracleBackend
from synth.small import SmallConfig, make_small
from test_oracle_golden import GOLD, load_snv
from unfazed_amd import abi
from unfazed_amd.hostpath import PhasingHost

pytestmark = pytest.mark.gpu


def _snvs(backend, ds, **runkw):
    """helpers.run_host, with the host's counters -> (records, annotated dnms, stderr text, stats)"""
    a = dict(RUN_DEFAULTS)
    a.update(runkw)
    sites, reads = tables(ds)
    host = PhasingHost(backend, sites, reads)
    dn = copy.deepcopy(ds.dnms)
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        recs = host.run_read_phasing(dn, ds.pedigrees, a["threads"], a["build"], a["no_extended"], a["multithread_proc_min"], a["quiet_mode"],
                                     params_from(a), a["search_dist"], a["insert_size_max_sample"], a["stdevs"], a["readlen"])
    return recs, dn, err.getvalue(), host.stats


def _cnvs(backend, ds):
    sites, reads = tables(ds)
    host = PhasingHost(backend, sites, reads)
    dn = copy.deepcopy(ds.dnms)
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        recs = host.run_cnv_phasing(dn, ds.pedigrees, 1, "38", 1000, False, abi.make_params())
    return recs, dn, err.getvalue(), host.stats


def _sites_of(dn):
    return [(d["chrom"], d["start"], d["end"], d["kid"], d.get("candidate_sites"), d.get("het_sites")) for d in dn]


def _both_routes(run, monkeypatch):
    monkeypatch.delenv("UZ_FIND_ROUTE", raising=False)
    cohort = run()
    monkeypatch.setenv("UZ_FIND_ROUTE", "kid")
    kid = run()
    monkeypatch.delenv("UZ_FIND_ROUTE")
    assert list(cohort[0].keys()) == list(kid[0].keys())
    assert json.dumps(norm_records(cohort[0]), sort_keys=True) == json.dumps(norm_records(kid[0]), sort_keys=True)
    assert _sites_of(cohort[1]) == _sites_of(kid[1])
    assert cohort[2] == kid[2]
    return cohort, kid


def test_two_kid_golden_by_both_routes(engine, monkeypatch):
    g, ds = load_snv(os.path.join(GOLD, "snv_find_many_two_kids_noext.json"))
    cohort, kid = _both_routes(lambda: _snvs(engine, ds, **g["run"]), monkeypatch)
    assert cohort[3]["find_cohort_calls"] == 1 and cohort[3]["find_kid_calls"] == 0
    assert kid[3]["find_cohort_calls"] == 0 and kid[3]["find_kid_calls"] == 2
    recs, dn = cohort[0], cohort[1]
    assert list(recs.keys()) == g["record_order"] and json.loads(json.dumps(norm_records(recs))) == g["records"]
    ref = {(d["chrom"], d["start"], d["end"], d["kid"]): d for d in g["dnms"]}
    for d in dn:
        r = ref[(d["chrom"], d["start"], d["end"], d["kid"])]
        assert d.get("candidate_sites") == r.get("candidate_sites") and d.get("het_sites") == r.get("het_sites")


def _three_kids():
    return make_small(SmallConfig(seed=909, n_dnms=21, kids=["kidA", "kidB", "kidC"], cluster_prob=0.6, odd_read_prob=0.05))


def test_three_kids_by_both_routes(engine, monkeypatch):
    ds = _three_kids()
    cohort, kid = _both_routes(lambda: _snvs(engine, ds), monkeypatch)
    assert len(cohort[0]) >= 3
    assert cohort[3]["find_cohort_calls"] == 1 and cohort[3]["find_kid_calls"] == 0
    assert kid[3]["find_cohort_calls"] == 0 and kid[3]["find_kid_calls"] == 3


def _three_kids_cnv():
    """DEL / DUP / INV events over the site-rich windows of three kids' DNMs, the kid's genotypes inside re-drawn as a hemizygous deletion or
    a 2 : 1 duplication (as tests/golden/make_golden.py lays them over one kid)"""
    rng = np.random.RandomState(5)
    ds = _three_kids()
    col = {s: i for i, s in enumerate(ds.samples)}
    svs = []
    for i, d in enumerate(ds.dnms[:12]):
        vt = ["DEL", "DUP", "DEL", "DUP", "INV"][i % 5]
        k = col[d["kid"]]
        st, en = d["start"] - int(rng.randint(500, 4000)), d["start"] + int(rng.randint(500, 4000))
        svs.append({"chrom": d["chrom"], "start": st, "end": en, "kid": d["kid"], "vartype": vt, "bam": "", "cram_ref": None})
        for r in ds.sites:
            if r.chrom != d["chrom"] or not (st <= r.start <= en) or rng.rand() >= 0.7:
                continue
            if vt == "DEL":
                depth = int(rng.randint(12, 25))
                r.gt_types[k], r.ref_depths[k], r.alt_depths[k] = (0, depth, 0) if rng.rand() < 0.5 else (3, 0, depth)
            elif vt == "DUP":
                a, b = [(20, 10), (10, 20), (30, 14), (14, 30), (22, 11), (67, 33)][rng.randint(6)]
                r.gt_types[k], r.ref_depths[k], r.alt_depths[k] = 1, a, b
    ds.dnms = svs
    return ds


def test_cnv_phasing_of_three_kids_by_both_routes(engine, monkeypatch):
    ds = _three_kids_cnv()
    assert len({d["kid"] for d in ds.dnms if d["vartype"] in ("DEL", "DUP")}) == 3
    cohort, kid = _both_routes(lambda: _cnvs(engine, ds), monkeypatch)
    assert cohort[3]["cnv_cohort_calls"] == 1 and cohort[3]["cnv_kid_calls"] == 0 and cohort[3]["find_cohort_calls"] == 1
    assert kid[3]["cnv_cohort_calls"] == 0 and kid[3]["cnv_kid_calls"] == 3 and kid[3]["find_kid_calls"] == 3
    assert sum(1 for r in cohort[0].values() if r["cnv_evidence_type"] == "ALLELE-BALANCE") >= 3
    want = _cnvs(OracleBackend(), ds)  # (a backend without the cohort calls: kid by kid, on the CPU)
    assert want[3]["cnv_cohort_calls"] == 0 and want[3]["find_cohort_calls"] == 0
    assert json.dumps(cohort[0], sort_keys=True) == json.dumps(want[0], sort_keys=True) and _sites_of(cohort[1]) == _sites_of(want[1])


def test_one_kid_takes_the_per_kid_path(engine, monkeypatch):
    monkeypatch.delenv("UZ_FIND_ROUTE", raising=False)
    ds = make_small(SmallConfig(seed=12, n_dnms=6))
    recs, dn, err, stats = _snvs(engine, ds)
    assert stats["find_cohort_calls"] == 0 and stats["find_kid_calls"] == 1 and stats["cnv_cohort_calls"] == 0
