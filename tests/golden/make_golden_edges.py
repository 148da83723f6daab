"""The reference's own answers on the hand-built read-stage edge panels (tests/readcases.py), in the manner of make_golden.py:
runs the REFERENCE (through tests/refrun.py and the tests/refshim stand-ins) on both panels for every run parameter set and writes
tests/golden/read_edges.json -- per panel the dataset digest, the annotated DNM site lists and the cutoff, per run its parameters, the
records, their order and the stderr lines.  Recorded results only.

Run in the authoring container only:   python tests/golden/make_golden_edges.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import readcases  # noqa: E402
import refrun  # noqa: E402
from make_golden import dataset_digest, norm_records  # noqa: E402

OUT = os.path.join(HERE, "read_edges.json")


def site_lists(dnms):
    return [dict(chrom=d["chrom"], start=d["start"], end=d["end"], kid=d["kid"], candidate_sites=d.get("candidate_sites"),
                 het_sites=d.get("het_sites")) for d in dnms]


def gen_panel(name, panel, runner):
    ds = panel.dataset
    out = dict(digest=dataset_digest(ds), runs={})
    for run, kw in panel.runs.items():
        recs, dnms, err, cutoffs = runner(ds, tag="edges_%s_%s" % (name, run), **kw)
        lists = site_lists(dnms)
        if "dnms" not in out:  # (the site lists do not depend on the read-stage parameters that the runs vary: kept once)
            out["dnms"] = lists
            out["cutoff"] = {k: float(v) for k, v in cutoffs.items()}
        assert lists == out["dnms"] and {k: float(v) for k, v in cutoffs.items()} == out["cutoff"], run
        out["runs"][run] = dict(run=kw, record_order=list(recs.keys()), records=norm_records(recs), stderr=err.splitlines())
        print(name, run, len(recs), "records")
    return out


def main():
    assert refrun.available(), "the reference is required to generate golden vectors"
    out = dict(point=gen_panel("point", readcases.point_panel(), refrun.run_phase_snvs),
               sv=gen_panel("sv", readcases.sv_panel(), refrun.run_phase_svs))
    with open(OUT, "w") as fh:
        json.dump(out, fh, sort_keys=True, separators=(",", ":"))
        fh.write("\n")


if __name__ == "__main__":
    main()
