"""One build of the device's header build over the whole panel of tests/linkcases.py, in a process of its own (uz_build_records reads its switches
once per process): every table of every form is uploaded, read back (uz_reads_headers, uz_reads_columns, uz_reads_marks) and written to one .npz;
the ASCII route and the refusals of hand-edited views ride along where asked.  Started by tests/test_link_cases_gpu.py -- not a test module."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import linkcases as lc  # noqa: E402
from unfazed_amd.engine import HipEngine, UnfazedHipError  # noqa: E402


def read_back(eng, rid, n):
    got = {}
    got.update(eng.reads_headers(rid, n))
    got.update(eng.reads_columns(rid, n))
    got.update(eng.reads_marks(rid, n))
    return got


def facts(part):
    v = part.view
    return dict(cols=sorted(k for k in part.arrays if getattr(v, k, None)), n=int(v.n_segs), n_tup=int(v.n_tup), qpos_wide=int(v.qlow_pos_wide),
                bl_wide=int(v.bl_wide), cigar_compact=int(v.cigar_compact), n_pk_spans=int(v.n_pk_spans))


def main(out, extras):
    eng = HipEngine(0)
    store, index = {}, []
    for case in lc.panel():
        for form in lc.form_list(case):
            part, idx = lc.select(case, form)
            key = "%s|%s" % (case.name, form[0])
            sys.stderr.write("[table] %s\n" % key)
            sys.stderr.flush()
            rid = eng.upload_reads_packed(part)
            eng.wait_reads(rid)
            got = read_back(eng, rid, idx.size)
            eng.free_reads(rid)
            for k, a in got.items():
                store["%d/%s" % (len(index), k)] = a
            index.append(dict(key=key, **facts(part)))
    res = dict(tables=index, ascii=[], refusals=[])
    if "ascii" in extras:
        # the same source tables through uz_reads_upload (k_pack_ascii); the quality plane of such a table is built for the threshold of the
        # parameters at a phase call (k_build_qlow): one DNM on a two-site table, once per threshold
        import sizingcases
        from unfazed_amd import abi
        sites = sizingcases.make_sites([[6000, 6050]])
        sid = eng.upload_sites(sites)
        fid = eng.add_family(sid, *sites.family_columns("kid", "dad", "mom"))
        dv = abi.dnms_view([0], [0], [6010], [6011], [abi.VT_POINT], [b"A"], [b"C"], 800.5)
        for case in lc.panel():
            sys.stderr.write("[table] ascii|%s\n" % case.name)
            sys.stderr.flush()
            rid = eng.upload_reads(case.table)
            for thr in lc.ASCII_THRESHOLDS:
                eng.phase_raw(fid, rid, dv, abi.make_params(min_gt_qual=thr, search_dist=100), abi.FIND_SECOND_WINDOW)
                got = read_back(eng, rid, case.n)
                store["ascii/%s/q%d/qlow" % (case.name, thr)] = got["qlow"]
                store["ascii/%s/q%d/nlow" % (case.name, thr)] = got["nlow"]
            for k, a in got.items():
                store["ascii/%s/%s" % (case.name, k)] = a
            eng.free_reads(rid)
            res["ascii"].append(case.name)
        eng.free_sites(sid)
    if "refusals" in extras:
        import linkrefusals
        cases = {c.name: c for c in lc.panel()}
        for name, make in linkrefusals.REFUSALS:
            honest, broken = make(cases, False), make(cases, True)
            sys.stderr.write("[table] refusal|%s|edited\n" % name)
            sys.stderr.flush()
            err = None
            try:
                rid = eng.upload_reads_packed(broken)
                eng.wait_reads(rid)
                eng.free_reads(rid)
            except UnfazedHipError as e:
                err = str(e)
                if not any(x in err for x in linkrefusals.SENTENCE.values()):  # not a refusal of the header build: nothing more on this device
                    raise
            sys.stderr.write("[table] refusal|%s|honest\n" % name)
            sys.stderr.flush()
            again = None
            try:  # the honest view still goes through on the same context
                rid = eng.upload_reads_packed(honest)
                eng.wait_reads(rid)
                eng.free_reads(rid)
            except UnfazedHipError as e:
                again = str(e)
            res["refusals"].append(dict(name=name, error=err, honest_error=again, edited=facts(broken), honest=facts(honest)))
    eng.close()
    np.savez(out, **store)
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
