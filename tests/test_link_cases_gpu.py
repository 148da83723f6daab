"""Every build of the device's header build (k_records.hip) held to the plain decoder of the link form (tests/linkmodel.py) on the hand-built panel
of tests/linkcases.py: every table, in every form the packer emits of it, is uploaded, read back (uz_reads_headers, uz_reads_columns,
uz_reads_marks) and compared with np.array_equal -- the five header columns, fm, l_seq, n_cigar, nlow, the stored unit mask, the CIGAR words at
cigar_off, every base below l_seq of every staged unit (found as uz_unit_of finds it: sq_off + the unit's rank in the mask) and the whole
quality word of every staged unit of a record the model gives a quality row.  No tolerances.

tests/test_link_model.py holds the model (and the host packer) to the source tables on the CPU and asserts what the panel reaches; it must pass
before this file is trusted.

The switches of uz_build_records are read once per process, so every build is one child process (tests/linkchild.py) that runs the whole panel and
writes one .npz; the parent holds the child's log lines to the build each table was meant to take.  Every build's outcome is recorded once: a child
that ends with any status but 0 -- a signal, an abort, an error of the device that came back as an exception -- or runs into its time limit fails
its test, the tests that share it fail with the same message without a new process, and no further child is started: the remaining build tests
fail without running.  Nothing retries a child."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import linkcases as lc
import linkmodel as lm
import linkrefusals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "linkchild.py")
SWITCHES = ("UZ_BUILD_FROM_MEMORY", "UZ_TUP8_IN_HBM", "UZ_BUILD_OWN_SUMS", "UZ_BUILD_SCAN_KERNEL", "UZ_BUILD_GENERIC", "UZ_BUILD_LAZY", "UZ_BASE_LISTS")
BUILDS = {"default": {}, "from_memory": {"UZ_BUILD_FROM_MEMORY": "1"}, "tup8_in_hbm": {"UZ_TUP8_IN_HBM": "1"}, "own_sums": {"UZ_BUILD_OWN_SUMS": "1"},
          "own_sums_scan_kernel": {"UZ_BUILD_OWN_SUMS": "1", "UZ_BUILD_SCAN_KERNEL": "1"}, "generic": {"UZ_BUILD_GENERIC": "1"}, "lazy": {"UZ_BUILD_LAZY": "1"}}
EXTRAS = {"default": ["ascii", "refusals"], "from_memory": ["refusals"]}
_trouble = []   # a child that died: no further child is started
_models = {}    # decode() of every table of the panel, computed once and shared by the builds
_runs = {}


def models():
    if not _models:
        for case in lc.panel():
            for form in lc.form_list(case):
                part, idx = lc.select(case, form)
                _models["%s|%s" % (case.name, form[0])] = lm.decode(part)
    return _models


def _failed(build, why):
    _trouble.append("%s: %s" % (build, why.splitlines()[0][:200]))
    _runs[build] = "the child of build %r failed: %s" % (build, why)
    raise AssertionError(_runs[build])


def run_build(tmp_path_factory, build):
    if build in _runs:
        if isinstance(_runs[build], str):  # it failed once: the same failure, no new process
            raise AssertionError(_runs[build])
        return _runs[build]
    assert not _trouble, "not started: an earlier child failed (%s)" % _trouble[0]
    out = str(tmp_path_factory.mktemp("link") / (build + ".npz"))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(BUILDS[build], UZ_BUILD_LOG="1")
    try:
        r = subprocess.run([sys.executable, CHILD, out] + EXTRAS.get(build, []), env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        _failed(build, "time limit")
    if r.returncode != 0:
        _failed(build, "status %d\n%s" % (r.returncode, r.stderr[-3000:]))
    lines = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    if not lines:
        _failed(build, "no result line\n%s" % r.stderr[-3000:])
    res = json.loads(lines[-1][len("RESULT "):])
    log, key = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("[table] "):
            key = line[len("[table] "):]
            log[key] = []
        elif line.startswith("[uz_build_records]") and key is not None:
            log[key].append(line)
    _runs[build] = (res, dict(np.load(out)), log)
    return _runs[build]


def meant(build, f):
    """the log line's fields a table must show under a build (uz_build_records: which kernels the table's form and the switches select)"""
    cols = set(f["cols"])
    link = ({"tup_umask", "tup_n_low", "start_d8", "pair_d8"} <= cols and bool(cols & {"tup", "tup8"}) and f["cigar_compact"] == 1 and "end" not in cols
            and "qlow" not in cols and build != "generic")
    host_sums = "pk_sums" in cols and f["n_pk_spans"] > 0 and not build.startswith("own_sums")
    # (uz_rec_scratch_bytes: (spans + 2) rows of UZ_PK_SUMS + 1 eight-byte sums, at least UZ_PL_DICT_MIN packed combinations of 16 bytes; a
    # table below 16.7 M records has pk_shift UZ_PK_SHIFT_SMALL; a view with tup_n_bl has bl_pos, or the upload refuses it)
    scratch = max(((f["n"] + 1023) // 1024 + 2) * (lm.PK_SUMS + 1) * 8, 256 * 16)
    from_lds = (link and host_sums and lm.pk_shift(f["n"]) == lm.PK_SHIFT_SMALL and 1 <= f["n_tup"] and 16 * f["n_tup"] <= scratch and not f["qpos_wide"]
                and not f["bl_wide"] and ("tup_n_bl" not in cols or "bl_pos" in cols) and build != "from_memory")
    tup8 = "none" if "tup8" not in cols else ("lds" if from_lds and build != "tup8_in_hbm" else "hbm")
    return dict(link_form=int(link), host_sums=int(host_sums), from_lds=int(from_lds), tup8=tup8)


@pytest.mark.parametrize("build", list(BUILDS))
def test_every_table_of_the_panel_equals_the_model(tmp_path_factory, build):
    res, got, log = run_build(tmp_path_factory, build)
    want = models()
    assert [t["key"] for t in res["tables"]] == list(want), "the child ran another panel"
    wrong, seen = [], dict(from_lds=set(), tup8=set(), link_form=set(), host_sums=set())
    for k, f in enumerate(res["tables"]):
        key = f["key"]
        rb = {name[len("%d/" % k):]: a for name, a in got.items() if name.startswith("%d/" % k)}
        bad = lm.readback_differences(want[key], rb, rb, rb)
        if bad:
            wrong.append((key, bad))
        lines = log.get(key, [])
        assert len(lines) == 1, (key, lines)
        m = re.search(r"link_form (\d) host_sums (\d) .* tup8 (\w+) -> from_lds (\d)", lines[0])
        took = dict(link_form=int(m.group(1)), host_sums=int(m.group(2)), tup8=m.group(3), from_lds=int(m.group(4)))
        assert took == meant(build, f), (key, lines[0], meant(build, f))
        for name, v in took.items():
            seen[name].add(v)
    assert not wrong, wrong[:20]
    by_key = {f["key"]: meant(build, f) for f in res["tables"]}
    if build in ("default", "lazy", "tup8_in_hbm"):
        # the build from LDS for every room-edge table and every residue; the build from memory for two-byte positions and a dictionary
        # beyond UZ_PL_DICT_MIN in a small table
        for key in ("room_cigar|" + LINK, "room_esc|" + LINK, "room_qpos|pair8/everything/tup8=1/bl=0/bq=0", "room_bl|" + POINTS, "dict_256|" + LINK,
                    "dict_edges|" + LINK, "edges|" + LINK, "edges|" + POINTS) + tuple("b0_%d|%s" % (r, POINTS) for r in range(8)):
            assert by_key[key]["from_lds"] == 1, key
        for key in ("wide|" + POINTS, "dict_257|" + LINK, "dict_300|" + LINK):
            assert by_key[key]["from_lds"] == 0, key
        assert seen["tup8"] == ({"none", "lds", "hbm"} if build != "tup8_in_hbm" else {"none", "hbm"})
    else:
        assert seen["from_lds"] == {0}
        assert seen["link_form"] == ({0} if build == "generic" else {0, 1})
        assert seen["host_sums"] == ({0} if build.startswith("own_sums") else {1})  # (every selection brings the packer's span sums)


LINK = "pair8/everything/tup8=1/bl=1/bq=1"
POINTS = "pair8/points/tup8=1/bl=1/bq=1"


def test_the_ascii_route_gives_the_source_rows_and_plane(tmp_path_factory):
    """the same source tables through uz_reads_upload (k_pack_ascii, k_build_qlow): headers, flags, every CIGAR word, every base and -- at thresholds
    0, 20, 255 and 300 (the clamp: every quality lies below it) -- every word of the quality plane and every count against the source"""
    res, got, log = run_build(tmp_path_factory, "default")
    cases = {c.name: c for c in lc.panel()}
    assert sorted(res["ascii"]) == sorted(cases)
    k32 = np.arange(32)
    for name, case in cases.items():
        T, n = case.table, case.n
        rb = {k[len("ascii/%s/" % name):]: a for k, a in got.items() if k.startswith("ascii/%s/" % name)}
        for k in ("start", "end", "tlen", "mate", "qname", "l_seq", "n_cigar"):
            assert np.array_equal(rb[k], getattr(T, k)), (name, k)
        assert np.array_equal(rb["fm"], T.flag.astype(np.uint32) | (T.mapq.astype(np.uint32) << 16) | (T.aux.astype(np.uint32) << 24)), name
        assert np.all(rb["umask"] == lm.UMASK_ALL), name
        nc = T.n_cigar.astype(np.int64)
        rel = np.arange(int(nc.sum())) - np.repeat(np.concatenate([[0], np.cumsum(nc)])[:-1], nc)
        assert np.array_equal(rb["cigar"][np.repeat(rb["cigar_off"].astype(np.int64), nc) + rel], T.cigar[np.repeat(T.cigar_off.astype(np.int64), nc) + rel] if rel.size else []), name
        units = lm.row_units(T.l_seq)
        rec = np.repeat(np.arange(n), units)
        unit = np.arange(int(units.sum())) - np.repeat(np.concatenate([[0], np.cumsum(units)])[:-1], units)
        by = rb["seq4"].reshape(-1, 16)[rb["sq_off"].astype(np.int64)[rec] + unit]
        codes = (by[:, k32 >> 1] >> np.where(k32 & 1, 0, 4)) & 15
        valid = (32 * unit[:, None] + k32[None, :]) < T.l_seq[rec][:, None]
        assert np.array_equal(codes[valid], case.code_mat[rec[:, None], 32 * unit[:, None] + k32[None, :]][valid]), name
        qrow = rb["qoff"].astype(np.int64)[rec] + unit
        assert np.unique(qrow).size == qrow.size and (qrow.size == 0 or qrow.max() < int(units.sum())), name
        for thr in lc.ASCII_THRESHOLDS:
            low = (case.qual_mat[rec[:, None], 32 * unit[:, None] + k32[None, :]] < min(thr, 256)) & valid
            want = (low.astype(np.uint64) << k32.astype(np.uint64)[None, :]).sum(1).astype(np.uint32)
            assert rb["q%d/qlow" % thr].size == int(units.sum()), (name, thr, "the plane was not built")
            assert np.array_equal(rb["q%d/qlow" % thr][qrow], want), (name, thr, "plane")
            count = np.bincount(rec, weights=low.sum(1), minlength=n).astype(np.int64)
            assert np.array_equal(rb["q%d/nlow" % thr], np.minimum(count, 255)), (name, thr, "nlow")


@pytest.mark.parametrize("name", [name for name, _ in linkrefusals.REFUSALS])
def test_a_hand_edited_view_is_refused_alike_by_both_builds(tmp_path_factory, name):
    """uz_check_upload_flag's code and sentence from the build from LDS and the build from memory; the honest view then goes through on the same context"""
    errs = []
    for build in ("default", "from_memory"):
        res, _, log = run_build(tmp_path_factory, build)
        r = {x["name"]: x for x in res["refusals"]}[name]
        # which kernel met the view: k_pack_link in the default child, but for the table with two-byte positions (a 481-base read) and the view
        # without the packer's span sums (their totals row would be refused before the build), which only k_pack_rec takes
        for which in ("edited", "honest"):
            lines = log.get("refusal|%s|%s" % (name, which), [])
            assert len(lines) == 1, (build, which, lines)
            want_lds = meant(build, r[which])["from_lds"]
            assert lines[0].endswith("from_lds %d" % want_lds), (build, which, lines[0])
            assert want_lds == int(build == "default" and name not in ("mask_on_a_481_base_read", "cigar_total_off_by_one")), (build, name)
        assert r["error"] is not None, (build, "not refused")
        assert r["honest_error"] is None, (build, r["honest_error"])
        assert linkrefusals.SENTENCE[linkrefusals.FLAG_OF[name]] in r["error"], (build, r["error"])
        errs.append(r["error"])
    codes = [re.search(r"failed \((-?\d+)\)", e).group(1) for e in errs]
    assert codes[0] == codes[1] and errs[0] == errs[1], errs
