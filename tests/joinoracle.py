"""The batch-wide joins of the BAM stage stated the PLAIN way -- the independent reference of tests/test_join_cases.py and
tests/test_join_cases_gpu.py.  Test infrastructure.

What the reference program does per DNM (read_collector.py:400, :185: the mate of every fetched read and of every mate; :226-234: tables keyed by the
read's name), said over a whole file read front to back:

  * the records are the file's, in file order (every one with its virtual offset);
  * mate(x): none unless x is paired, its mate is not flagged unmapped and its mate reference is one of the header's; else the FIRST record in file
    order that carries x's name and the other read-of-pair flag, lies on x's mate reference and overlaps x's mate position (pos <= mpos < end, end
    as htslib's bam_endpos says: pos + 1 without a CIGAR);
  * members: the records the fetches return (on the fetch's reference, pos < hi and end > lo), closed under mate() -- a plain fixed point;
  * output: the members in file order; name ids by first appearance of the name's BYTES; a record's mate is the output index of mate(x);
  * bases travel with the records a fetch returned -- with every record under all_bases.

No tasks, no reach, no hashes, no index: where the stage is limited by one of those, this is what it has to equal all the same.

"The other read-of-pair flag" is the project's statement of it (csrc/io_stage.cpp is_mate_of): the wanted flags are x's two read-of-pair bits
inverted -- a record with both bits wants nobody (its name is seen, its mate is none), a record with neither wants either bit, and a candidate that
carries both bits answers every asker that wants one.  Real files set exactly one bit on a paired record, and there the statements agree."""
import numpy as np

import walkmodel as wm

FPAIRED, FMUNMAP, FREAD1, FREAD2 = 0x1, 0x8, 0x40, 0x80


def records(path, coff_base=0, ref_base=0):
    """the placed records of a file in file order, each with its virtual offset -> (records, number of references)"""
    data, coff, at = wm.inflate_file(path)
    names, lens, first = wm.header_of(data)
    out = []
    for r in wm.records_of(data, first):
        if not 0 <= r["ref"] < len(names):
            break  # (the unplaced tail; a refID the header does not know ends every walk as well)
        k = int(np.searchsorted(at, r["at"], side="right")) - 1  # the last block that starts at or in front of the record: an empty block holds nothing
        r["voff"] = ((int(coff[k]) + coff_base) << 16) | (r["at"] - int(at[k]))
        r["ref"] += ref_base
        r["mref"] = r["mref"] + ref_base if 0 <= r["mref"] < len(names) else (-1 if r["mref"] < 0 else 1 << 40)
        out.append(r)
    return out, len(names)


def mate(recs, x, ref_lo, ref_hi):
    fl = x["flag"]
    if not (fl & FPAIRED) or (fl & FMUNMAP) or not ref_lo <= x["mref"] < ref_hi:
        return None
    want = (fl ^ (FREAD1 | FREAD2)) & (FREAD1 | FREAD2)
    for k, y in enumerate(recs):
        if y["name"] == x["name"] and (y["flag"] & want) and y["ref"] == x["mref"] and y["pos"] <= x["mpos"] < y["end"]:
            return k
    return None


def join(recs, fetches, ref_lo, ref_hi, all_bases=False):
    """-> dict(voff, qname, mate, bases, names: the name of every id, rec: the file's record number of every kept record)"""
    fetched = [any(r["ref"] == t and r["pos"] < hi and r["end"] > lo for t, lo, hi, _ in fetches) for r in recs]
    member = list(fetched)
    mates = {}
    grew = True
    while grew:  # the fixed point, the plain way
        grew = False
        for k, r in enumerate(recs):
            if member[k] and k not in mates:
                mates[k] = mate(recs, r, ref_lo, ref_hi)
                if mates[k] is not None and not member[mates[k]]:
                    member[mates[k]] = grew = True
    kept = [k for k in range(len(recs)) if member[k]]
    at = {k: i for i, k in enumerate(kept)}
    ids, names = {}, []
    for k in kept:
        if recs[k]["name"] not in ids:
            ids[recs[k]["name"]] = len(names)
            names.append(recs[k]["name"])
    return dict(voff=np.array([recs[k]["voff"] for k in kept], np.uint64), qname=np.array([ids[recs[k]["name"]] for k in kept], np.uint32),
                mate=np.array([-1 if mates[k] is None else at[mates[k]] for k in kept], np.int32),
                bases=np.array([fetched[k] or bool(all_bases) for k in kept], bool), names=names, rec=kept, n_qnames=len(names))


def run(path, fetches, all_bases=False):
    recs, n_ref = records(path)
    return join(recs, fetches, 0, n_ref, all_bases)


def run_set(paths, file_base, ref_base, fetches, all_bases=False):
    """files as a set (BamSource.open_many): every file joined on its own -- a mate stays inside its file, a name is its file's -- and the answers laid
    end to end: virtual offsets behind the files in front, references shifted, name ids and record indices counted on"""
    parts, n_recs, n_names = [], 0, 0
    for f, p in enumerate(paths):
        recs, n_ref = records(p, int(file_base[f]), int(ref_base[f]))
        x = join(recs, fetches, int(ref_base[f]), int(ref_base[f]) + n_ref, all_bases)
        x["mate"] = np.where(x["mate"] >= 0, x["mate"] + n_recs, -1).astype(np.int32)
        x["qname"] = (x["qname"] + n_names).astype(np.uint32)
        n_recs += len(x["rec"]); n_names += len(x["names"])
        parts.append(x)
    out = {k: np.concatenate([x[k] for x in parts]) for k in ("voff", "qname", "mate", "bases")}
    out.update(names=[n for x in parts for n in x["names"]], n_qnames=n_names, first_name=np.cumsum([0] + [len(x["names"]) for x in parts]),
               first_rec=np.cumsum([0] + [len(x["rec"]) for x in parts]))
    return out
