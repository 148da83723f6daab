"""The header build from LDS (k_pack_link) against the build that reads every part from memory (k_pack_rec, UZ_BUILD_FROM_MEMORY=1): the
same table, uploaded in a fresh process each way, must come back with the same record headers -- start, end, template length, mate and name
id -- and a pair form that contradicts itself must be refused by both.  The tables are the pair form of test_upload_forms_gpu.py: FIRST /
SECOND pairs that straddle the 256-record rounds and the 1024-record spans of the build, SECONDs that bring their own template length, and
records spelled out in the escape list.  The one-byte dictionary index with a forced escape list is expanded at both of its places, k_pack_link's
LDS and memory (UZ_TUP8_IN_HBM=1, UZ_BUILD_FROM_MEMORY=1), to the same headers, and a span that contradicts its offsets is refused alike."""
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

_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from test_upload_forms_gpu import _odd_table, _tup8_table
from unfazed_amd import io_native
from unfazed_amd.engine import HipEngine, UnfazedHipError
n_dnms, breakage, out = int(sys.argv[3]), sys.argv[4], sys.argv[5]
rh, arrs, N = _odd_table(n_dnms)
src = io_native.ReadsSource(io_native.pack_reads(rh, 20))
contig_of = np.searchsorted(arrs["contig_off"], np.arange(N), side="right") - 1
fc = np.unique(contig_of).astype(np.int32)
# the form the staged pass sends: `end` derived, two-bit rows, quality lists and unit masks (the fetches' units: the whole contig here)
fetches = (fc, np.zeros(fc.size, np.int32), np.full(fc.size, 2 ** 31 - 1, np.int32))
n_tup_esc = None
if breakage.startswith("hot3"):  # ... with the hot table of the one-byte dictionary index cut to three entries: most records escape
    part = _tup8_table(src, fetches, 3, extra=np.ones(fc.size, np.uint16))
    n_tup_esc = int(part.view.n_tup_esc)
    if breakage == "hot3_moved_escape":  # the offsets still ascend to the total, but the spans do not hold what they say
        assert part.arrays["tup_esc_off"].size >= 3 and part.arrays["tup_esc_off"][1] > 0
        part.arrays["tup_esc_off"][1] -= 1
else:
    part = src.select(*fetches, extra=np.ones(fc.size, np.uint16))
p = part.arrays["pair_d8"]
f = np.nonzero((p[:N] >= 1) & (p[:N] <= 252))[0]
if breakage == "second_named_twice":
    i, j = int(f[5]), int(f[5]) + int(p[f[5]])
    k = next(int(x) for x in f if x != i and 0 < j - int(x) <= 252)
    p[k] = j - k
elif breakage == "orphan_second":
    p[int(f[7])] = 0
elif breakage == "first_names_a_first":
    i = int(f[9])
    k = next(int(x) for x in f if 0 < int(x) - i <= 252 and int(x) != i + int(p[i]))
    p[i] = k - i
codes = np.unique(p[:N]).tolist()
eng = HipEngine(0)
res = {"n": int(N), "codes": codes, "error": None, "n_tup_esc": n_tup_esc}
try:
    rid = eng.upload_reads_packed(part)
    eng.wait_reads(rid)
    got = eng.reads_headers(rid, N)
    eng.free_reads(rid)
    np.savez(out, **got)
except UnfazedHipError as e:
    res["error"] = str(e)
eng.close()
print("RESULT " + json.dumps(res))
"""


def _build(tmp_path, from_memory, n_dnms, breakage="none", lazy=False, tup8_in_hbm=False):
    out = str(tmp_path / ("%s%s%s_%d_%s.npz" % ("rec" if from_memory else "link", "_lazy" if lazy else "", "_hbm" if tup8_in_hbm else "", n_dnms, breakage)))
    env = dict(os.environ, UZ_BUILD_LOG="1")
    env.pop("UZ_BUILD_FROM_MEMORY", None)
    env.pop("UZ_BUILD_LAZY", None)
    env.pop("UZ_TUP8_IN_HBM", None)
    if from_memory:
        env["UZ_BUILD_FROM_MEMORY"] = "1"
    if tup8_in_hbm:  # the one-byte dictionary index rebuilt in memory in front of the LDS build too
        env["UZ_TUP8_IN_HBM"] = "1"
    if lazy:  # the header build at the table's first use, on the compute stream (read once per process: hence the child)
        env["UZ_BUILD_LAZY"] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, TESTS, str(n_dnms), breakage, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1][len("RESULT "):])
    builds = [x for x in r.stderr.splitlines() if x.startswith("[uz_build_records]")]
    assert builds and all(x.endswith("from_lds %d" % (0 if from_memory else 1)) for x in builds), builds
    res["builds"] = builds
    return res, (dict(np.load(out)) if res["error"] is None else None)


@pytest.mark.parametrize("n_dnms", [40, 260])
def test_link_headers_equal_the_memory_build(tmp_path, n_dnms):
    link, got = _build(tmp_path, False, n_dnms)
    rec, want = _build(tmp_path, True, n_dnms)
    assert link["error"] is None and rec["error"] is None
    assert link["n"] > 2048  # several spans of 1024 records, every one of its four rounds
    # SECONDs, FIRSTs, SECONDs with their own template length and spelled-out records all occur
    codes = set(link["codes"])
    assert 0 in codes and any(1 <= c <= 252 for c in codes) and {253, 254} <= codes, sorted(codes)
    for k in ("start", "end", "tlen", "mate", "qname"):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("breakage", ["second_named_twice", "orphan_second", "first_names_a_first"])
def test_a_contradicting_pair_form_is_refused_by_both_builds(tmp_path, breakage):
    link, _ = _build(tmp_path, False, 20, breakage)
    rec, _ = _build(tmp_path, True, 20, breakage)
    assert link["error"] is not None and rec["error"] is not None
    rc = [re.search(r"failed \((-?\d+)\)", e["error"]).group(1) for e in (link, rec)]
    assert rc[0] == rc[1], (link["error"], rec["error"])


def _three_builds(tmp_path, breakage):
    """default (tup8 rebuilt in k_pack_link's LDS), UZ_TUP8_IN_HBM=1 (k_tup_expand in front of k_pack_link), UZ_BUILD_FROM_MEMORY=1 (k_tup_expand
    in front of k_pack_rec); _build holds each log line to its from_lds"""
    runs = [_build(tmp_path, False, 40, breakage), _build(tmp_path, False, 40, breakage, tup8_in_hbm=True), _build(tmp_path, True, 40, breakage)]
    for (res, _), where in zip(runs, ("lds", "hbm", "hbm")):
        assert all(" tup8 %s -> " % where in x for x in res["builds"]), res["builds"]
        assert res["n"] > 2048 and res["n_tup_esc"] > 100  # several spans of 1024 records, escapes in all four rounds of each
    return runs


def test_a_forced_escape_list_expands_alike_in_lds_and_in_memory(tmp_path):
    """The one shared expansion of the one-byte dictionary index (pk_tup8_expand) at both of its places: into k_pack_link's LDS and, by
    k_tup_expand, into memory -- with a hot table of three entries, so that most records of every span go through the escape list."""
    (_, lds), (_, hbm), (_, rec) = runs = _three_builds(tmp_path, "hot3")
    assert all(res["error"] is None for res, _ in runs), [res["error"] for res, _ in runs]
    for k in ("start", "end", "tlen", "mate", "qname"):
        assert np.array_equal(lds[k], rec[k]) and np.array_equal(hbm[k], rec[k]), k
    # an escape moved from one span to the next: refused by all three, alike
    runs = _three_builds(tmp_path, "hot3_moved_escape")
    assert all(res["error"] is not None for res, _ in runs)
    rc = [re.search(r"failed \((-?\d+)\)", res["error"]).group(1) for res, _ in runs]
    assert rc[0] == rc[1] == rc[2], [res["error"] for res, _ in runs]


def test_the_build_at_first_use_gives_the_same_headers(tmp_path):
    """The header build that no upload queued (UZ_BUILD_LAZY=1): the table's first use runs it on the compute stream from the columns the
    upload left with the table -- the same headers as from the build queued behind the copies, in the link form."""
    queued, want = _build(tmp_path, False, 40)
    lazy, got = _build(tmp_path, False, 40, lazy=True)
    assert queued["error"] is None and lazy["error"] is None
    assert lazy["n"] == queued["n"] > 2048  # several spans of 1024 records
    for k in ("start", "end", "tlen", "mate", "qname"):
        assert np.array_equal(got[k], want[k]), k


def test_the_build_at_first_use_refuses_a_contradicting_pair_form(tmp_path):
    queued, _ = _build(tmp_path, False, 40, "orphan_second")
    lazy, _ = _build(tmp_path, False, 40, "orphan_second", lazy=True)
    assert queued["error"] is not None and lazy["error"] is not None
    rc = [re.search(r"failed \((-?\d+)\)", e["error"]).group(1) for e in (queued, lazy)]
    assert rc[0] == rc[1], (queued["error"], lazy["error"])
