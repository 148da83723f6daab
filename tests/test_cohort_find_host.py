"""The host path's cohort route without a device: a backend that answers find_cohort / phase_cnv_cohort from the CPU oracle, group by group,
shows that PhasingHost lays the kids' DNMs back to back, makes one call, and cuts every kid's slice of the lists out again -- records,
annotated DNMs and messages are those of the per-kid route.  (tests/test_cohort_find_host_gpu.py runs the same on the device's calls.)"""
import numpy as np

from oracle_backend import OracleBackend
from test_cohort_find_host_gpu import _both_routes, _cnvs, _snvs, _three_kids, _three_kids_cnv
from unfazed_amd import abi


class CohortOracle(OracleBackend):
    """OracleBackend plus the two cohort calls, each answered by one oracle call per group"""

    def _sub(self, dv, first, count):
        a = dv.arrays
        sl = slice(first, first + count)
        return abi.dnms_view(a["contig"][sl], a["rcontig"][sl], a["start"][sl], a["end"][sl], a["vartype"][sl], [b""] * count, [b""] * count, 0.0,
                             dflags=a["dflags"][sl], mult=a["mult"][sl])

    def find_cohort(self, groups, dv, params, mode, fetch=True):
        assert [f for _, f, _ in groups] == list(np.cumsum([0] + [n for _, _, n in groups])[:-1])  # back to back, in order
        parts = [self.find(fam, self._sub(dv, first, count), params, mode) for fam, first, count in groups]
        co, ho = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)]
        for p in parts:
            co.append(p[0][1:] + co[-1][-1])
            ho.append(p[3][1:] + ho[-1][-1])
        cat = lambda k: np.concatenate([p[k] for p in parts])  # noqa: E731
        return np.concatenate(co), cat(1), cat(2), np.concatenate(ho), cat(4)

    def phase_cnv_cohort(self, groups, dv, params, rb_counts=None, want_lists=True):
        parts = [self.phase_cnv(fam, self._sub(dv, first, count), params) for fam, first, count in groups]
        out = {k: np.concatenate([p[k] for p in parts]) for k in ("cnv_counts", "origin", "evidence", "etype")}
        out["lists"] = [x for p in parts for x in p["lists"]]
        return out


def test_three_kids_by_both_routes_on_the_oracle(monkeypatch):
    ds = _three_kids()
    cohort, kid = _both_routes(lambda: _snvs(CohortOracle(), ds), monkeypatch)
    assert len(cohort[0]) >= 3
    assert cohort[3]["find_cohort_calls"] == 1 and cohort[3]["find_kid_calls"] == 0
    assert kid[3]["find_cohort_calls"] == 0 and kid[3]["find_kid_calls"] == 3
    plain = _snvs(OracleBackend(), ds)  # no cohort calls: the per-kid path whatever the switch says
    assert plain[3]["find_cohort_calls"] == 0 and plain[3]["find_kid_calls"] == 3 and list(plain[0]) == list(cohort[0])


def test_cnv_phasing_of_three_kids_by_both_routes_on_the_oracle(monkeypatch):
    ds = _three_kids_cnv()
    cohort, kid = _both_routes(lambda: _cnvs(CohortOracle(), ds), monkeypatch)
    assert cohort[3]["cnv_cohort_calls"] == 1 and cohort[3]["cnv_kid_calls"] == 0 and cohort[3]["find_cohort_calls"] == 1
    assert kid[3]["cnv_cohort_calls"] == 0 and kid[3]["cnv_kid_calls"] == 3 and kid[3]["find_kid_calls"] == 3
    assert sum(1 for r in cohort[0].values() if r["cnv_evidence_type"] == "ALLELE-BALANCE") >= 3


def test_group_tuples_of_both_forms():
    """HipEngine._groups: the find side's (fam, first, count) and the read stage's (fam, reads, first, count, cutoff) give the same array type;
    the short form carries reads_id -1 and cutoff 0.0, which the find-side calls do not read."""
    from unfazed_amd.engine import HipEngine
    fields = lambda arr, n: [(g.fam_id, g.reads_id, g.dnm_first, g.dnm_count, g.cutoff) for g in arr[:n]]  # noqa: E731
    short = HipEngine._groups([(7, 0, 3), (9, 3, 0), (7, 3, 5)])
    assert isinstance(short[0], abi.CohortGroup)
    assert fields(short, 3) == [(7, -1, 0, 3, 0.0), (9, -1, 3, 0, 0.0), (7, -1, 3, 5, 0.0)]
    long = HipEngine._groups([(7, 2, 0, 3, 412.5), (9, 4, 3, 5, 388.25)])
    assert isinstance(long[0], abi.CohortGroup)
    assert fields(long, 2) == [(7, 2, 0, 3, 412.5), (9, 4, 3, 5, 388.25)]
    mixed = HipEngine._groups([(1, 0, 2), (2, 5, 2, 1, 100.0)])
    assert fields(mixed, 2) == [(1, -1, 0, 2, 0.0), (2, 5, 2, 1, 100.0)]
    assert len(HipEngine._groups([])) == 1  # (never a zero-length array: the call refuses n_groups = 0 itself)
