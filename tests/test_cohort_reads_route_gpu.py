"""The read side of a cohort call by the cohort route (hostpath.PhasingHost._joined_run, UZ_READS_ROUTE=cohort): 12 kids from files -- one BAM + BAI
per kid -- in ONE phase_snvs call, the kids' files presented to the BAM stage as one (io_native.BamSource.open_many), walked and joined as one
batch, the read stage on the table that comes out (uz_phase_cohort_joined).  The records, name lists included, and the messages must be those of
the per-kid route and of the CPU oracle backend through the same host code; the counters say which route ran.  A parity test, not a truth test."""
import contextlib
import io
import os

import pytest

from helpers import norm_records
from synth.small import SmallConfig, make_small
from test_cohort_files_gpu import _indexed_files, _stats

pytestmark = pytest.mark.gpu

KIDS = ["kid%02d" % i for i in range(12)]
BASE = {"UZ_HOST_CHUNKS": "0"}


def _run(paths, dnms, pedigrees, env, sv=False, backend=None):
    """one product call -> (records, sorted stderr lines, the call's PhasingHost objects, the runs the cohort route cut)"""
    from unfazed_amd import hostpath, session
    from unfazed_amd.snv_phaser import phase_snvs
    from unfazed_amd.sv_phaser import phase_svs
    env = dict(BASE, **env)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    own = session._BACKEND
    if backend is not None:
        session.set_backend(backend)
    session._READS.clear()
    session._HOSTS.clear()
    for k in [k for k in session._SITES if "@" in k]:
        del session._SITES[k]
    runs = []
    orig = hostpath.PhasingHost._cohort_runs

    def spy(self, items):
        r = orig(self, items)
        runs.append([[len(idxs) for _, idxs in run] for run in r])
        return r
    hostpath.PhasingHost._cohort_runs = spy
    try:
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            recs = (phase_svs if sv else phase_snvs)([dict(d) for d in dnms], list(pedigrees), pedigrees, paths["sites"], 2, "38", False, 10 ** 9, False, [0.0, 0.2],
                                                    [0.8, 1.0], [0.2, 0.8], 20, 10, 5000, 1000000, 3, 1, 151, 5)
        return norm_records(recs), sorted(err.getvalue().splitlines()), list(session._HOSTS.values()), runs
    finally:
        hostpath.PhasingHost._cohort_runs = orig
        if backend is not None:
            session.set_backend(own)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    ds = make_small(SmallConfig(seed=2031, n_dnms=48, kids=KIDS, cluster_prob=0.5, coverage_per_hap=9.0))
    paths = _indexed_files(ds, tmp_path_factory.mktemp("cohort"))
    dnms = [dict(chrom=d["chrom"], start=d["start"], end=d["end"], kid=d["kid"], vartype="POINT", bam=paths["bams"][d["kid"]], cram_ref=None) for d in ds.dnms]
    return ds, paths, dnms


@pytest.fixture(scope="module")
def oracle(cohort, hip_lib):
    from oracle_backend import OracleBackend
    ds, paths, dnms = cohort
    want, err_w, _, _ = _run(paths, dnms, ds.pedigrees, {}, backend=OracleBackend())
    # conditions on the inputs, not measurements: an empty result cannot pass
    assert len(dnms) == 48 and len({r["kid"] for r in want.values()}) >= 10 and len(want) >= len(dnms) // 10
    assert any(r.get("dad_reads") or r.get("mom_reads") for r in want.values())
    return want, err_w


def test_cohort_route_equals_the_kid_route_and_the_oracle(cohort, oracle):
    ds, paths, dnms = cohort
    want, err_w = oracle
    kid, err_k, hosts_k, runs_k = _run(paths, dnms, ds.pedigrees, {"UZ_READS_ROUTE": "kid"})
    got, err_g, hosts_g, runs_g = _run(paths, dnms, ds.pedigrees, {"UZ_READS_ROUTE": "cohort"})
    assert kid == want and err_k == err_w
    assert got == want and err_g == err_w
    for k in KIDS:  # kid by kid, name lists included
        assert {x: r for x, r in got.items() if r["kid"] == k} == {x: r for x, r in want.items() if r["kid"] == k}, k
    sk, sg = _stats(hosts_k), _stats(hosts_g)
    assert (sg["bam_walks"], sg["read_tables"], sg["phase_cohort_calls"]) == (1, 1, 1), sg
    assert len(runs_g) == 1 and len(runs_g[0]) == 1 and not runs_k
    n_groups = len(runs_g[0][0])  # the kids whose DNMs reached the device
    assert 10 <= n_groups <= len(KIDS)
    assert (sk["bam_walks"], sk["read_tables"], sk["phase_cohort_calls"]) == (n_groups, n_groups, 1), sk


@pytest.mark.parametrize("limit", [5, 9])
def test_several_runs(cohort, oracle, limit):
    """four DNMs per kid: at most five per run puts every kid in a run of its own, at most nine puts two kids in a run"""
    ds, paths, dnms = cohort
    want, err_w = oracle
    got, err_g, hosts, runs = _run(paths, dnms, ds.pedigrees, {"UZ_READS_ROUTE": "cohort", "UZ_COHORT_RUN_DNMS": str(limit)})
    assert got == want and err_g == err_w
    s = _stats(hosts)
    assert len(runs) == 1 and len(runs[0]) > 1
    assert s["bam_walks"] == s["read_tables"] == s["phase_cohort_calls"] == len(runs[0])
    for run in runs[0]:  # a kid is never split; a run holds at most `limit` DNMs unless it is one kid
        assert sum(run) <= limit or len(run) == 1, run
    assert any(len(run) > 1 for run in runs[0]) == (limit == 9)


def test_a_run_the_walk_does_not_take_goes_kid_by_kid(cohort, oracle):
    ds, paths, dnms = cohort
    want, err_w = oracle
    got, err_g, hosts, runs = _run(paths, dnms, ds.pedigrees, {"UZ_READS_ROUTE": "cohort", "UZ_WALK_MAX_BYTES": "1"})
    assert got == want and err_g == err_w
    s = _stats(hosts)
    n_groups = len(runs[0][0])
    assert s["phase_cohort_calls"] == 1 and s["read_tables"] == n_groups and s["bam_walks"] == n_groups, s  # (the kids' own batches took the link form)


def test_other_switches_keep_the_kid_route(cohort, oracle):
    ds, paths, dnms = cohort
    want, err_w = oracle
    got, err_g, hosts, runs = _run(paths, dnms, ds.pedigrees, {"UZ_READS_ROUTE": "cohort", "UZ_JOINS": "host"})
    assert got == want and err_g == err_w and not runs
    one = [d for d in dnms if d["kid"] == KIDS[0]]
    got1, _, hosts1, runs1 = _run(paths, one, ds.pedigrees, {"UZ_READS_ROUTE": "cohort"})  # a call naming one kid is untouched
    assert got1 == {x: r for x, r in want.items() if r["kid"] == KIDS[0]} and not runs1 and _stats(hosts1).get("phase_cohort_calls", 0) == 0


def test_phase_svs_by_the_cohort_route(tmp_path_factory, hip_lib):
    """a few SV DNMs of four kids: +-cutoff fetches around both breakpoints, per kid its own cutoff"""
    import copy
    import gzip
    from filesio import dump_dataset, vcf_text, write_bai, write_bgzf_text, write_tbi
    from oracle_backend import OracleBackend
    from synth.small_sv import SvConfig, make_small_sv
    root = tmp_path_factory.mktemp("svs")
    kids = ["svkid%d" % i for i in range(4)]
    sets = []
    for i, k in enumerate(kids):
        ds = make_small_sv(SvConfig(seed=700 + i, n_svs=3, kid=k, coverage_per_hap=10.0))
        # every kid has parents and sites of its own: the samples renamed, the kids' site records side by side in one file
        ren = {"dad1": "dad_" + k, "mom1": "mom_" + k, k: k}
        ds.samples = [ren[s] for s in ds.samples]
        ds.pedigrees = {k: dict(ds.pedigrees[k], dad=ren["dad1"], mom=ren["mom1"])}
        sets.append(ds)
    samples = [s for ds in sets for s in ds.samples]
    recs = []
    for i, ds in enumerate(sets):  # a kid's records carry its trio's genotypes; the other samples are unknown there
        for r in ds.sites:
            r = copy.copy(r)
            pad = lambda col, fill: [fill] * (3 * i) + list(col) + [fill] * (3 * (len(sets) - 1 - i))  # noqa: E731
            r.gt_types, r.ref_depths, r.alt_depths, r.gt_quals = pad(r.gt_types, 2), pad(r.ref_depths, -1), pad(r.alt_depths, -1), pad(r.gt_quals, -1.0)
            r.genotypes = r.raw = None
            recs.append(r)
    order = {c: j for j, c in enumerate(sets[0].contigs)}
    recs.sort(key=lambda r: (order[r.chrom], r.start))
    paths = dict(bams={}, sites=str(root / "sites.vcf.gz"))
    for ds in sets:
        p = dump_dataset(ds, str(root / ds.dnms[0]["kid"]))
        write_bai(p["bams"][ds.dnms[0]["kid"]])
        paths["bams"].update(p["bams"])
    write_bgzf_text(paths["sites"], vcf_text(samples, recs, sets[0].contigs))
    write_tbi(paths["sites"])
    assert gzip.open(paths["sites"], "rt").readline().startswith("##")
    pedigrees = {k: ds.pedigrees[k] for k, ds in zip(kids, sets)}
    dnms = []
    for ds in sets:
        for d in copy.deepcopy(ds.dnms):
            d["bam"], d["cram_ref"] = paths["bams"][d["kid"]], None
            dnms.append(d)
    want, err_w, _, _ = _run(paths, dnms, pedigrees, {}, sv=True, backend=OracleBackend())
    assert len(dnms) == 12 and len(want) >= 4 and len({r["kid"] for r in want.values()}) >= 3
    kid, err_k, _, _ = _run(paths, dnms, pedigrees, {"UZ_READS_ROUTE": "kid"}, sv=True)
    got, err_g, hosts, runs = _run(paths, dnms, pedigrees, {"UZ_READS_ROUTE": "cohort"}, sv=True)
    assert kid == want and err_k == err_w
    assert got == want and err_g == err_w
    s = _stats(hosts)
    assert (s["bam_walks"], s["read_tables"], s["phase_cohort_calls"]) == (1, 1, 1) and len(runs) == 1
