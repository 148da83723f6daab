"""The panel of tests/joincases.py on the CPU.  For every case four statements of the batch-wide joins must agree bit for bit -- the plain oracle
(tests/joinoracle.py: file order, first match, a fixed point; no tasks, no reach, no hashes, no index), the device's order-free formulation
(tests/joinmodel.py over the descriptors of the plan's sub-tasks), the one-pass stage (plan_finish over its own walk) and the host twin of the device
route (select_kept: plan_finish over descriptors, per task of the stage and per sub-task) -- and the case's `shape` must hold: the branch it aims at
was reached.  A batch whose closure needs more trips through the index than include/uz_bamwalk.h allows is refused by every one of them.
tests/test_join_cases_gpu.py then holds the kernels of csrc/k_bamjoin.hip to the same panel."""
import numpy as np
import pytest

import joincases as jc
import joinmodel
import joinoracle
import walkcases as wc
from unfazed_amd import io_native

CASES = jc.build_panel()
HOST_ROUTES = ("model", "one_pass", "twin", "twin_sub")


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    folder = tmp_path_factory.mktemp("joincases")
    return {c.name: c.write(folder) for c in CASES}


def test_the_cap_is_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uz_bamwalk.h")).read()
    assert int(re.search(r"#define UZ_JOIN_MAX_TRIPS (\d+)", text).group(1)) == joinmodel.MAX_TRIPS == io_native.JOIN_MAX_TRIPS == 64


def context(case, w, monkeypatch):
    wc._slack(case, monkeypatch)
    src = io_native.BamSource(w["path"], threads=2, insert_size_max_sample=-1)
    ctx = jc.host_routes(case, [w["path"]], src, case.fetch_arrays())
    recs, n_ref = joinoracle.records(w["path"])
    ctx.update(recs=recs, by_voff={r["voff"]: k for k, r in enumerate(recs)}, info=w["info"], oracle=joinoracle.join(recs, case.fetches, 0, n_ref, case.all_bases))
    return ctx


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_model_one_pass_stage_and_host_twin_agree(case, written, monkeypatch):
    ctx = context(case, written[case.name], monkeypatch)
    if case.refused:
        assert sorted(ctx["refusals"]) == sorted(HOST_ROUTES), ctx["refusals"]
        assert all(joinmodel.REFUSED in msg for msg in ctx["refusals"].values()), ctx["refusals"]
        case.shape(ctx)
        return
    assert not ctx["refusals"], ctx["refusals"]
    want = ctx["oracle"]
    assert want["voff"].size > 0
    for route in HOST_ROUTES:
        assert jc.same(ctx[route], want) == [], route
    case.shape(ctx)


@pytest.mark.parametrize("case", [c for c in CASES if not c.refused], ids=[c.name for c in CASES if not c.refused])
def test_the_oracles_parse_equals_the_whole_file_decoder(case, written):
    wc.check_parse(written[case.name]["path"])


def test_files_as_a_set(tmp_path_factory, written, monkeypatch):
    """two files with byte-identical records and names, of six cases: every mate stays inside its file, every file has name ids of its own, and a
    next_refID the file's header does not know is nobody's reference (the walk's INT32_MAX), though the set has such a reference"""
    import walkmodel as wm
    from types import SimpleNamespace
    monkeypatch.delenv("UZ_STAGE_SLACK", raising=False)
    cases = [c for c in CASES if c.name in jc.SET_CASES]
    assert len(cases) == len(jc.SET_CASES)
    folder = tmp_path_factory.mktemp("joincases_twice")
    second = {c.name: c.write(folder) for c in cases}
    src, paths, fetches = jc.open_twice(cases, written, second)
    ctx = jc.host_routes(SimpleNamespace(all_bases=False), paths, src, fetches)
    assert not ctx["refusals"], ctx["refusals"]
    want = joinoracle.run_set(paths, src.file_base, src.ref_base, list(zip(*(a.tolist() for a in fetches))))
    for route in HOST_ROUTES:
        assert jc.same(ctx[route], want) == [], route
    assert (ctx["desc"]["mtid"] == wm.INT32_MAX).sum() == 2 and len(src.contigs) > 3  # (in its own file the same record says mtid 3 of 3)
    first_rec, first_name = want["first_rec"], want["first_name"]
    assert (np.diff(first_rec)[0::2] == np.diff(first_rec)[1::2]).all() and (np.diff(first_name) > 0).all()  # the twins keep the same records, under ids of their own
    for f in range(len(paths)):
        m = want["mate"][first_rec[f]: first_rec[f + 1]]
        q = want["qname"][first_rec[f]: first_rec[f + 1]]
        assert ((m == -1) | ((m >= first_rec[f]) & (m < first_rec[f + 1]))).all() and (m >= 0).any() == (cases[f // 2].name != "wants_mtid_n_ref")
        assert q.min() == first_name[f] and q.max() == first_name[f + 1] - 1


@pytest.fixture(scope="module")
def desc_level(tmp_path_factory):
    return jc.desc_level_cases(tmp_path_factory.mktemp("joincases_rows"))


@pytest.mark.parametrize("k", range(3), ids=["equal_h1_different_h2", "equal_h1_and_h2_different_length", "all_three_equal"])
def test_names_that_agree_in_a_hash(desc_level, k):
    """no file holds two names with one h1 (64 bits): descriptors written by hand do.  The model's pure function over them against the oracle's answer
    for the names as they are -- two names, or, where h1, h2 and the length agree, one (tests/test_join_cases_gpu.py hands the same rows to the kernels)"""
    name, rows, n_ref, want = desc_level[k]
    trace = {}
    got = jc.join_rows(rows, n_ref, trace)
    assert jc.same(got, want) == [] and len(trace["needs"]) == 2  # the fetched records ask and are answered, then their mates
    assert np.unique(rows["h1"][:4]).size == 1 and want["n_qnames"] == (1 if name == "all_three_equal" else 2)
