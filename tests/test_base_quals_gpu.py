"""The quality bits of listed bases on the device (uz_types.h bl_qlow), by both header builds -- k_pack_link, and k_pack_rec with
UZ_BUILD_FROM_MEMORY=1 (read once per process: every build runs in a child, as tests/test_header_build_gpu.py's do):
 * the point-variant edge panel (tests/readcases.py) through the chunked staged route -- pipeline.run_pipelined over three chunks of its DNMs,
   every chunk's records selected for the chunk's own fetches with base_quals on -- gives, for every run of the panel, the status, counts,
   origin, evidence and the four vote lists of the oracle's read stage on the whole table, bit for bit, and no UnfazedHipError (a quality bit
   or base the form did not stage fails the call); the oracle's records of the same runs are the reference's recorded answers
   (tests/golden/read_edges.json), held here once more; every chunk's table is built by the kernel the run is named for (the build's log);
 * the table of tests/qualcases.py (quality bytes written for every rule of the form; large enough that k_pack_link takes it) uploaded in
   the old form and the new one, by both builds: the same record headers four ways, and the same read-stage results for its DNMs;
 * a flipped bit -- a record's set bits are no longer the number its count names -- is refused by both builds with the same error code, and
   a view with the column but without bl_code, with bl_n in the place of tup_n_bl, without either, or beside the quality plane with UZ_E_ARG."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
KEYS = ("status", "counts", "origin", "evidence")

_HEAD = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from oracle import oracle as orc
from unfazed_amd import abi, io_native, pipeline
from unfazed_amd.engine import HipEngine, PinnedPool, UnfazedHipError
from unfazed_amd.staging import fetch_points
MODE = abi.FIND_SECOND_WINDOW
out = sys.argv[3]
"""

_PANEL_CHILD = _HEAD + r"""
import readcases
from test_read_edges import batch_views, panel, panel_tables
pn = panel("point")
sites, reads = panel_tables("point")
dn = pn.dataset.dnms
ped = pn.dataset.pedigrees[readcases.KID]
refs, alts = [c.ref.encode() for c in pn.cases], [c.alt.encode() for c in pn.cases]
starts, ends = [d["start"] for d in dn], [d["end"] for d in dn]
eng = HipEngine(0)
sid = eng.upload_sites(sites)
fid = eng.add_family(sid, *sites.family_columns(readcases.KID, ped["dad"], ped["mom"]))
res = {}
for run in pn.runs:
    P, sv, rv, dv, found, alen, vt, rt = batch_views("point", run)
    n = dv.view.n
    want = orc.phase(P, sv, rv, dv, found, keep_lists=True)
    assert int((want["status"] == abi.ST_OK).sum()) == n
    src = io_native.ReadsSource(io_native.pack_reads(rv, P.min_gt_qual, with_end=True))
    cuts = [0, n // 3, 2 * n // 3, n]
    pool = PinnedPool()
    parts, lists = {}, {}

    def view(a, b):
        return abi.dnms_view([0] * (b - a), [0] * (b - a), starts[a:b], ends[a:b], vt[a:b], refs[a:b], alts[a:b], readcases.CUTOFF)

    def records(k, het_off, het_idx):  # the chunk's records for the chunk's own fetches (its find has just returned), in the new form
        a, b = cuts[k], cuts[k + 1]
        fc, flo, fhi, fex = fetch_points([0] * (b - a), starts[a:b], np.zeros(b - a, np.uint8), sites.pos, het_off, het_idx, P,
                                         vartype=np.array(vt[a:b]), end=ends[a:b], cutoff=readcases.CUTOFF, allele_len=alen[a:b])
        pool.new_slab(8 << 20)
        parts[k] = src.select(fc, flo, fhi, alloc=pool.alloc, all_bases=bool(P.no_extended), extra=fex, base_quals=True)
        pool.end_slab()
        return parts[k]

    def done(k, rr):
        vo, vv = eng.votes(cuts[k + 1] - cuts[k])
        lists[k] = (vo.copy(), vv.copy())

    try:
        chunks = [dict(a=cuts[k], b=cuts[k + 1], dnms=view(cuts[k], cuts[k + 1]), records=records, sites=None) for k in range(3)]
        got = pipeline.run_pipelined(eng, P, MODE, n, chunks, fid=fid, on_done=done)
        eng.sync()
        bits = [abi.base_qual_bits(p) for p in parts.values()]  # (the columns lie in the pool's page-locked blocks: read before they go back)
        bits = [None if b is None else b.copy() for b in bits]
    finally:
        pool.free_all()
    for key in ("status", "counts", "origin", "evidence"):
        assert np.array_equal(np.asarray(got[key]).reshape(np.asarray(want[key]).shape), want[key]), (run, key)
    wo, wv = want["vote_off"], want["vote_val"]
    for k in range(3):
        vo, vv = lists[k]
        qmap = parts[k].qname_map  # (the pair form numbers the names of a selection by first appearance: back to the table's ids)
        for d in range(cuts[k + 1] - cuts[k]):
            for j in range(4):  # dad reads, mom reads (name ids), dad sites, mom sites (positions)
                g = 4 * (cuts[k] + d) + j
                mine = vv[vo[4 * d + j]: vo[4 * d + j + 1]]
                if j < 2 and qmap is not None:
                    mine = qmap[mine]
                assert np.array_equal(mine, wv[wo[g]: wo[g + 1]]), (run, k, d, j)
    res[run] = dict(n=int(n), listed_bases=int(sum(0 if b is None else b.size for b in bits)), low_listed=int(sum(0 if b is None else int(b.sum()) for b in bits)),
                    qlow_pos=int(sum(int(p.view.n_qlow_pos) for p in parts.values())), votes=int(wo[-1]))
eng.free_sites(sid)
eng.close()
print("RESULT " + json.dumps(res))
"""

_TABLE_CHILD = _HEAD + r"""
import qualcases
t = qualcases.table()
src = qualcases.source()
eng = HipEngine(0)
eng.set_params(t.P)
sid = eng.upload_sites_view(t.sh)
fid = eng.add_family(sid, t.sc.gt, t.sc.rd, t.sc.ad, t.sc.gq)
res, save = {"error": {}}, {}
forms = {}
for name, bq in (("old", False), ("new", True)):
    part, idx = qualcases.select(src, bq)
    forms[name] = part
    N = int(part.view.n_segs)
    rid = eng.upload_reads_packed(part)
    eng.wait_reads(rid)
    for k, v in eng.reads_headers(rid, N).items():
        save["%s_%s" % (name, k)] = v
    eng.find(fid, t.dv, t.P, MODE)
    for k, v in eng.phase_raw(fid, rid, t.dv, t.P, MODE).items():
        save["%s_%s" % (name, k)] = np.asarray(v)
    eng.free_reads(rid)
    res["n"] = N
new = forms["new"]
res["has_bits"] = bool(new.view.bl_qlow) and not forms["old"].view.bl_qlow


def refused(part):
    try:
        rid = eng.upload_reads_packed(part)
        eng.wait_reads(rid)
        eng.free_reads(rid)
    except UnfazedHipError as e:
        return str(e)
    return None


# a flipped bit: the first record with a base list and at most UZ_QLOW_LIST_MAX low bases gets one set bit more (or less) than its count names
off, pos, code = abi.base_lists(new)
nl = abi.small_columns(new)["n_low"][:N]
k = int(np.nonzero((np.diff(off) > 0) & (nl <= abi.QLOW_LIST_MAX))[0][100])
e = int(off[k])
new.arrays["bl_qlow"][e >> 3] ^= np.uint8(1 << (e & 7))
res["error"]["flipped_bit"] = refused(new)
new.arrays["bl_qlow"][e >> 3] ^= np.uint8(1 << (e & 7))
keep = new.view.bl_code
new.view.bl_code = None
res["error"]["no_bl_code"] = refused(new)
new.view.bl_code = keep
# the column beside the plain count column (bl_n) where the form has the dictionary's (tup_n_bl); without any count of listed bases; beside the
# quality plane
spare = np.zeros(max(N, int(new.view.n_row_units) * abi.QLOW_UNIT_BYTES) + 8, np.uint8)
keep = new.view.tup_n_bl
new.view.tup_n_bl, new.view.bl_n = None, spare.ctypes.data
res["error"]["with_bl_n"] = refused(new)
new.view.bl_n = None
counts = int(new.view.n_bl), int(new.view.n_bl_units)
new.view.n_bl = new.view.n_bl_units = 0
res["error"]["no_tup_n_bl"] = refused(new)
new.view.tup_n_bl, (new.view.n_bl, new.view.n_bl_units) = keep, counts
new.view.qlow = spare.ctypes.data
res["error"]["with_plane"] = refused(new)
new.view.qlow = None
res["error"]["restored"] = refused(new)  # ... and the honest table is still taken
eng.free_sites(sid)
eng.close()
np.savez(out, **save)
print("RESULT " + json.dumps(res))
"""


def _child(tmp_path, script, tag, from_memory):
    out = str(tmp_path / ("%s_%s.npz" % (tag, "rec" if from_memory else "link")))
    env = dict(os.environ, UZ_BUILD_LOG="1")
    env.pop("UZ_BUILD_FROM_MEMORY", None)
    env.pop("UZ_BUILD_LAZY", None)
    if from_memory:
        env["UZ_BUILD_FROM_MEMORY"] = "1"
    r = subprocess.run([sys.executable, "-c", script, ROOT, TESTS, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads([x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1][len("RESULT "):])
    builds = [x for x in r.stderr.splitlines() if x.startswith("[uz_build_records]")]
    lds = [x.endswith("from_lds 1") for x in builds]
    link_form = [" link_form 1 " in x for x in builds]
    # every table of the run by the build the run is named for (k_pack_link takes the link form only: a --no-extended batch, staged with all
    # its bases and no unit masks, is not in it and has no listed bases either)
    assert builds and (not any(lds) if from_memory else lds == link_form), builds
    res["builds"], res["builds_from_lds"] = len(builds), int(sum(lds))
    return res, (dict(np.load(out)) if os.path.exists(out) else None)


@pytest.mark.parametrize("from_memory", [False, True], ids=["k_pack_link", "k_pack_rec"])
def test_edge_panel_through_the_chunked_staged_route(tmp_path, from_memory):
    from test_read_edges import assert_same_as_golden, oracle_run, panel
    # (every chunk's table -- a few hundred records, up to ~50 combinations of small columns -- is built by the kernel the run is named for:
    # _child holds the build's own log to it; three chunks for each of the panel's runs with base lists)
    res, _ = _child(tmp_path, _PANEL_CHILD, "panel", from_memory)
    print(res)
    runs = panel("point").runs
    assert res.pop("builds") >= 3 * len(runs)
    assert res.pop("builds_from_lds") >= (0 if from_memory else 3 * sum(1 for r in runs.values() if not r.get("no_extended")))
    assert sorted(res) == sorted(panel("point").runs)
    for run, r in res.items():
        assert r["n"] == len(panel("point").cases) and r["votes"] > 0
        if not panel("point").runs[run].get("no_extended"):  # (a --no-extended batch is staged with all its bases: nothing is listed)
            assert r["listed_bases"] > 50 and r["low_listed"] > 0
        assert_same_as_golden("point", run, oracle_run("point", run))  # the oracle the device was held to gives the reference's records


@pytest.fixture(scope="module")
def table_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("base_quals")
    return _child(d, _TABLE_CHILD, "table", False), _child(d, _TABLE_CHILD, "table", True)


def test_both_forms_and_both_builds_agree(table_runs):
    (link, a), (rec, b) = table_runs
    assert link["n"] == rec["n"] > 2048 and link["has_bits"] and rec["has_bits"]
    assert link["builds_from_lds"] == link["builds"] > 0 and rec["builds_from_lds"] == 0
    for k in ("start", "end", "tlen", "mate", "qname"):  # eng.reads_headers, four ways
        for other in (a["new_" + k], b["old_" + k], b["new_" + k]):
            assert np.array_equal(a["old_" + k], other), k
    for k in KEYS:  # the read stage over the table's DNMs: the old form against the new one, by either build
        for other in (a["new_" + k], b["old_" + k], b["new_" + k]):
            assert np.array_equal(a["old_" + k], other), k
    assert (a["old_status"] == 0).sum() > 5 and (a["old_counts"] != 0).any()


def test_a_wrong_bit_and_a_missing_column_are_refused(table_runs):
    (link, _), (rec, _) = table_runs
    for r in (link, rec):
        assert all(r["error"][k] is not None for k in ("flipped_bit", "no_bl_code", "with_bl_n", "no_tup_n_bl", "with_plane")) and r["error"]["restored"] is None, r["error"]
    code = [re.search(r"failed \((-?\d+)\)", r["error"]["flipped_bit"]).group(1) for r in (link, rec)]
    assert code[0] == code[1], (link["error"], rec["error"])
    for r in (link, rec):
        for k in ("no_bl_code", "with_bl_n", "no_tup_n_bl", "with_plane"):
            assert re.search(r"failed \((-?\d+)\)", r["error"][k]).group(1) == "-1", r["error"]  # UZ_E_ARG
        # ... the two views with the column and the wrong count column by the checks of the column itself
        assert "bl_qlow needs" in r["error"]["with_bl_n"] and "bl_qlow without" in r["error"]["no_tup_n_bl"], r["error"]
