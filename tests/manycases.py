"""Sets of small BAM + BAI files for the source over many files (io_native.BamSource.open_many: uz_bamsrc_open_many), shared by
tests/test_bamsrc_many.py (host) and tests/test_cohort_walk_gpu.py (device).  A case is a list of files with the fetches of each, in the file's own
contig numbers; the same fetches through the set's source carry ref_base[f] on their contigs.  What a set must give is what its files give one by
one, laid end to end: `ends` says where each file's records and names start there, `shifted` moves a column of indices."""
import os
import shutil
from collections import namedtuple

import numpy as np

from unfazed_amd import io_native

Case = namedtuple("Case", "paths fetches env min_kept")  # env: switches the case runs under; min_kept: per file, the least records it must keep

CASES = ("copies", "same_path", "other_header", "empty_middle", "file_end", "index_and_host")


_FILES = {}


def _file(tmp, name, seed, n_dnms=4, contigs=("1", "2"), chr_prefix="", **kw):
    """one kid's BAM + BAI written by the Python writers -> (path, dataset, whole-file table); written once per directory: the cases share files"""
    key = (str(tmp), name)
    if key not in _FILES:
        _FILES[key] = _write(tmp, name, seed, n_dnms, contigs, chr_prefix, **kw)
    return _FILES[key]


def _write(tmp, name, seed, n_dnms, contigs, chr_prefix, **kw):
    from filesio import dump_dataset, write_bai
    from synth.small import SmallConfig, make_small
    ds = make_small(SmallConfig(seed=seed, n_dnms=n_dnms, contigs=list(contigs), chr_prefix=chr_prefix, cluster_prob=0.5, **kw))
    d = os.path.join(str(tmp), name)
    bam = list(dump_dataset(ds, d)["bams"].values())[0]
    write_bai(bam)
    return bam, ds, io_native.read_bam_table(bam, threads=2)


def _fetches(ds, full, seed, n_het=4):
    """the DNMs' fetches and a few one-base fetches around each (as tests/test_bamjoin_gpu.py: _small_fetches)"""
    rng = np.random.default_rng(seed)
    c, lo, hi, ex = [], [], [], []
    for d in ds.dnms:
        tid = full.contig_index[d["chrom"]]
        c.append(tid); lo.append(d["start"] - 1); hi.append(d["start"] + 1); ex.append(max(1, d["end"] - d["start"]))
        for p in np.sort(rng.integers(d["start"] - 5000, d["start"] + 5000, n_het)):
            c.append(tid); lo.append(int(p)); hi.append(int(p) + 1); ex.append(0)
    return np.array(c, np.int32), np.array(lo, np.int32), np.array(hi, np.int32), np.array(ex, np.uint16)


def _copy(bam, to):
    os.makedirs(os.path.dirname(to), exist_ok=True)
    shutil.copyfile(bam, to)
    shutil.copyfile(bam + ".bai", to + ".bai")
    return to


def build(name, tmp) -> Case:
    a, ds_a, full_a = _file(tmp, "a", 301)
    b, ds_b, full_b = _file(tmp, "b", 302, n_dnms=3)
    fa, fb = _fetches(ds_a, full_a, 1), _fetches(ds_b, full_b, 2)
    if name == "copies":  # two byte-identical files: every read name collides
        return Case([a, b, _copy(a, os.path.join(str(tmp), "a2", "copy.bam"))], [fa, fb, fa], {}, [1, 1, 1])
    if name == "same_path":
        return Case([a, b, a], [fa, fb, fa], {}, [1, 1, 1])
    if name == "other_header":  # another contig set, `chr` names: the files' references are not each other's
        c, ds_c, full_c = _file(tmp, "c", 303, n_dnms=5, contigs=("1", "2", "3"), chr_prefix="chr")
        assert full_c.contigs == ["chr1", "chr2", "chr3"] and full_a.contigs == ["1", "2"]
        return Case([a, c, b], [fa, _fetches(ds_c, full_c, 3), fb], {}, [1, 1, 1])
    if name == "empty_middle":  # the middle file's fetches meet no record
        none = (np.array([0, 1], np.int32), np.array([9_000_000, 9_500_000], np.int32), np.array([9_000_001, 9_500_001], np.int32), np.array([0, 0], np.uint16))
        return Case([a, b, a], [fa, none, fa], {}, [1, 0, 1])
    if name == "file_end":  # file 0's walk runs into the end of the file, behind which file 1 lies in the virtual file
        last = int(np.nonzero(np.diff(full_a.contig_off))[0][-1])
        p = int(full_a.start[-1])
        assert last == len(full_a.contigs) - 1 and int(full_a.contig_off[last + 1]) == full_a.n_segs
        f0 = (np.array([last, last], np.int32), np.array([p, p - 300], np.int32), np.array([p + 1, p - 299], np.int32), np.array([0, 0], np.uint16))
        return Case([a, b, a], [f0, fb, fa], {}, [1, 1, 1])
    if name == "index_and_host":  # odd records, a small reach slack: mates only the index can answer; (device) walk tasks handed back to the host
        # (every look-up through the index is a walk of its own on the host: few DNMs, a thin pile-up)
        o1, ds_1, full_1 = _file(tmp, "o1", 31, n_dnms=2, odd_read_prob=0.25, lowq_prob=0.08, softclip_prob=0.05, indel_prob=0.03, coverage_per_hap=5.0)
        o2, ds_2, full_2 = _file(tmp, "o2", 32, n_dnms=2, odd_read_prob=0.25, readlen=100, coverage_per_hap=5.0)
        return Case([o1, o2], [_fetches(ds_1, full_1, 31, 3), _fetches(ds_2, full_2, 32, 3)], {"UZ_STAGE_SLACK": "30", "UZ_TEST_FLAG_EVERY": "2"}, [1, 1])
    raise KeyError(name)


def joined_fetches(src, case):
    """the case's fetches through the set's source: file after file, ref_base[f] added to the contigs"""
    parts = [(f[0] + src.ref_base[k], f[1], f[2], f[3]) for k, f in enumerate(case.fetches)]
    return tuple(np.concatenate([p[i] for p in parts]).astype(parts[0][i].dtype) for i in range(4))


def ends(counts):
    """[n + 1]: where each file's items start when the files' are laid end to end"""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def shifted(col, by, none=-1):
    """a column of record / name indices moved by `by`, `none` kept"""
    col = np.asarray(col).astype(np.int64)
    return np.where(col == none, none, col + by)
