"""Driver and I/O surface -- host glue mirroring reference unfazed/unfazed.py
(DNM readers :18-90, get_bam_names :93-126, parse_ped :129-159, write_vcf_output :337-441,
unfazed :518-667).  Tiny data, no acceleration target; kept so that the command line and
the BED / annotated-VCF outputs drop in."""
from __future__ import annotations

import gzip
import os
import sys

import numpy as np
from glob import glob

from . import __reference_version__
from .hostpath import SNV_TYPES, SV_TYPES
from .io_vcf import read_vcf
from .model import HET, HOM_ALT
from .outfile import write_output
from .snv_phaser import phase_snvs, phase_snvs_bed
from .summarize import summarize_record, write_bed_output
from .sv_phaser import phase_svs

VCF_TYPES = ["vcf", "vcf.gz", "bcf"]  # reference utils.py:7
LABELS = ["chrom", "start", "end", "kid", "vartype"]
QUIET_MODE = False


def _bed_rows(lines):
    for line in lines:
        if line[0] == "#":
            continue
        fields = line.strip().split()
        if not len(fields) == 5:
            sys.exit("dnms bed file must contain the following columns exactly: " + ", ".join(LABELS))
        vartype = fields[4]
        if vartype not in SV_TYPES:
            vartype = SNV_TYPES[0]  # anything else becomes POINT (quirk Q20)
        yield {"chrom": fields[0], "start": int(fields[1]), "end": int(fields[2]), "kid": fields[3],
               "vartype": vartype, "bam": ""}


def read_vars_bed(bedname):
    with open(bedname, "r") as fh:
        yield from _bed_rows(fh)


def read_vars_bedzip(bedzipname):
    # the reference opens in binary mode and compares bytes to str (:44-48), which fails on
    # Python 3; a text-mode reader is the evident intent.
    with gzip.open(bedzipname, "rt") as fh:
        yield from _bed_rows(fh)


def _is_bcf(name):
    import gzip
    try:
        with gzip.open(name, "rb") as fh:
            return fh.read(4) == b"BCF\x02"
    except OSError:
        return False


def read_vars_vcf(vcfname):
    if vcfname.endswith("bcf") or _is_bcf(vcfname):
        # binary form: through the native decoder (io_native); same fields as the text path below
        from .io_native import read_vcf_table
        t = read_vcf_table(vcfname)
        chrom_of = np.repeat(np.arange(len(t.contigs)), np.diff(t.contig_off))
        # the HET / HOM_ALT cells by one selection over the [samples, records] codes: record-major, samples ascending, as the loops over both gave
        gt = np.asarray(t.gt).reshape(len(t.samples), t.n_sites)
        js, cols = np.nonzero(((gt == HET) | (gt == HOM_ALT)).T)
        last, vartype = -1, None
        for j, i in zip(js.tolist(), cols.tolist()):
            if j != last:
                last, vartype = j, t.info(j, "SVTYPE")
                if vartype is None:
                    vartype = SNV_TYPES[0]
            yield {"chrom": t.contigs[int(chrom_of[j])], "start": int(t.pos[j]), "end": int(t.end[j]),
                   "kid": t.samples[i], "vartype": vartype, "bam": ""}
        return
    samples, records, _ = read_vcf(vcfname)
    for r in records:
        vartype = r.info.get("SVTYPE")
        if vartype is None:
            vartype = SNV_TYPES[0]
        for i, gt in enumerate(r.gt_types):
            if gt in [HET, HOM_ALT]:
                yield {"chrom": r.chrom, "start": r.start, "end": r.end, "kid": samples[i], "vartype": vartype, "bam": ""}


class AlignmentFiles:
    """sample id -> alignment file(s): the directory scan (`{sample_id}.bam` / `.cram`) overlaid by explicit
    `id:path` pairs, which win.  Same outcomes and messages as reference unfazed.py:93-126."""

    def __init__(self):
        self.by_sample = {}
        self.saw_cram = False

    def scan_dir(self, directory):
        for path in sorted(glob(os.path.join(directory, "*.bam"))) + sorted(glob(os.path.join(directory, "*.cram"))):
            stem, ext = os.path.splitext(os.path.basename(path))
            self.by_sample.setdefault(stem, set()).add(path)
            self.saw_cram |= ext == ".cram"

    def pin(self, sample_id, path):
        if not os.path.isfile(path):
            sys.exit("invalid filename " + path)
        self.by_sample[sample_id] = {path}
        self.saw_cram |= path.endswith("cram")

    def check_cram_reference(self, cram_ref):
        if not self.saw_cram:
            return
        if cram_ref is None:
            sys.exit("Missing reference file for CRAM")
        if not os.path.isfile(cram_ref):
            sys.exit("Reference file is not valid")

    def lookup(self, sample):
        """-> (path, None) or (None, why) with why in {"missing", "multiple"}"""
        files = self.by_sample.get(sample)
        if files is None:
            return None, "missing"
        if len(files) != 1:
            return None, "multiple"
        return next(iter(files)), None


def get_bam_names(bam_dir, bam_pairs, cram_ref):
    files = AlignmentFiles()
    if bam_dir is not None:
        files.scan_dir(bam_dir)
    for sample_id, path in (bam_pairs or []):
        files.pin(sample_id, path)
    files.check_cram_reference(cram_ref)
    return files.by_sample


def parse_ped(ped, kids):
    """kid id -> {kid, dad, mom, sex} (strings) for the kids that have DNMs; kids with a parent coded `0`
    and kids absent from the file are reported and skipped (reference unfazed.py:129-159)."""
    wanted = set(kids)
    entries, parentless = {}, set()
    with open(ped, "r") as fh:
        rows = [ln.split() for ln in fh]
    for row in rows:
        sample = row[1]
        if sample not in wanted:
            continue
        dad, mom = row[2], row[3]
        if "0" in (dad, mom):
            _say("Parent of sample {} missing from pedigree file, will be skipped".format(sample))
            parentless.add(sample)
        else:
            entries[sample] = {"kid": sample, "dad": dad, "mom": mom, "sex": row[4]}
    for sample in kids:
        if sample not in entries and sample not in parentless:
            _say("{} missing from pedigree file, will be skipped".format(sample))
    return entries


def _say(*words):
    if not QUIET_MODE:
        print(*words, file=sys.stderr)


UOPS_HEADER = ('##FORMAT=<ID=UOPS,Number=1,Type=Float,Description="Count of pieces of evidence supporting the '
               'unfazed-identified origin parent or `-1` if missing">')
UET_HEADER = ('##FORMAT=<ID=UET,Number=1,Type=Float,Description="Unfazed evidence type: `0` (readbacked), '
              '`1` (allele-balance, for CNVs only), `2` (both), `3` (ambiguous readbacked), '
              '`4` (ambiguous allele-balance), `5` (ambiguous both), '
              '`6` (auto-phased sex-chromosome variant in male), or `-1` (missing)">')


BCF_OUTPUT_MESSAGE = ("annotated VCF output needs a text VCF as --dnms (BCF input carries no text records): "
                      "rerun with `--output-type bed`")


def uet_code(evidence_types):
    """reference unfazed.py:415-433"""
    if "AMBIGUOUS_READBACKED" in evidence_types:
        return 3
    if "AMBIGUOUS_ALLELE-BALANCE" in evidence_types:
        return 4
    if "AMBIGUOUS_BOTH" in evidence_types:
        return 5
    if "SEX-CHROM" in evidence_types:
        return 6
    if "READBACKED" in evidence_types and "ALLELE-BALANCE" in evidence_types:
        return 2
    if "READBACKED" in evidence_types:
        return 0
    if "ALLELE-BALANCE" in evidence_types:
        return 1
    return -1


def write_vcf_output(in_vcf_name, read_records, include_ambiguous, verbose, outfile, evidence_min_ratio):
    """reference unfazed.py:337-441: GT of a phased sample becomes 1|0 (paternal) / 0|1 (maternal),
    every sample gets UOPS and UET appended."""
    if in_vcf_name.endswith("bcf") or _is_bcf(in_vcf_name):
        if bcf_route() is None:
            sys.exit(BCF_OUTPUT_MESSAGE)
        return _write_vcf_from_bcf(in_vcf_name, read_records, include_ambiguous, verbose, outfile, evidence_min_ratio)
    if vcf_route() == "device" and int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        from . import session
        # asked for by name, the route makes its backend (and fails loudly without a device); as the default it serves a call that has one --
        # the driver's always has, from the phasing behind it
        backend = session.get_backend() if "UZ_VCF_ROUTE" in os.environ else session.current_backend()
        if hasattr(backend, "vcf_rows") and _write_vcf_device(in_vcf_name, read_records, include_ambiguous, verbose, outfile,
                                                              evidence_min_ratio, backend):
            return
    samples, records, header = read_vcf(in_vcf_name)
    out = _annotated_header(header)
    for r in records:
        out.append(_annotated_line(r, samples, read_records, include_ambiguous, verbose, evidence_min_ratio))
    VCF_STATS["vcf_host_rows"] += len(records)
    write_output(outfile, ["\n".join(out) + "\n"])


def _annotated_header(header):
    out = []
    out.extend(header[:-1])
    out.append("##unfazed=" + __reference_version__
               + ". Phase info in pipe-separated GT field order -> 1|0 is paternal, 0|1 is maternal")
    out.append(UOPS_HEADER)
    out.append(UET_HEADER)
    out.append(header[-1])
    return out


def _annotated_line(r, samples, read_records, include_ambiguous, verbose, evidence_min_ratio):
    """one record of the annotated VCF: the per-record part of write_vcf_output, shared by the host writer and by the device route's
    handed-back records"""
    f = list(r.raw)
    fmt = f[8].split(":")
    gt_i = fmt.index("GT") if "GT" in fmt else None
    f[8] = f[8] + ":UOPS:UET"
    for i, gt in enumerate(r.gt_types):
        uops, uet = -1, -1
        col = f[9 + i].split(":")
        # VCF lets a sample drop trailing FORMAT fields (`./.`): pad, so UOPS / UET land in their own columns
        col += ["."] * (len(fmt) - len(col))
        if gt in [HET, HOM_ALT]:
            vartype = r.info.get("SVTYPE")
            if vartype is None:
                vartype = SNV_TYPES[0]
            key = "{}_{}_{}_{}_{}".format(r.chrom, r.start, r.end, samples[i], vartype)
            if key in read_records:
                s = summarize_record(read_records[key], include_ambiguous, verbose, evidence_min_ratio)
                if s is not None:
                    if gt_i is not None:
                        if s["origin_parent"] == read_records[key]["dad"]:
                            col[gt_i] = "1|0"
                        elif s["origin_parent"] == read_records[key]["mom"]:
                            col[gt_i] = "0|1"
                    uops = s["evidence_count"]
                    uet = uet_code(s["evidence_types"])
        f[9 + i] = ":".join(col) + ":%g:%g" % (uops, uet)
    return "\t".join(f)


VCF_ROUTE_DEFAULT = "device"  # UZ_VCF_ROUTE not set.  profiles/vcf_route_ab.json: every device run ahead of every host run at both shapes (the rule bed_route() states)
VCF_STATS = {"vcf_device_rows": 0, "vcf_host_rows": 0, "vcf_calls": 0}  # records whose line the device wrote / the per-record host code wrote, uz_vcf_rows calls
UOPS_DEVICE_MAX = 999999  # the largest count the device prints ("%g" turns to an exponent at 10^6)


def vcf_route() -> str:
    """UZ_VCF_ROUTE: "device" -- a single-rank call that writes the annotated VCF gets its record lines from the device (uz_vcf_rows) -- or
    "host" (write_vcf_output's loop over the cells).  Not set: "device" where the call already has a backend with vcf_rows, else "host"."""
    return "device" if os.environ.get("UZ_VCF_ROUTE", VCF_ROUTE_DEFAULT).lower() == "device" else "host"


def vcf_annotations(sites, samples, read_records, include_ambiguous, verbose, evidence_min_ratio):
    """The annotations of the device route, one loop over RECORDS.  sites: per record the tuple (chrom, start, end, vartype) the host writer
    forms its key from, or None for a record without one.  -> (ann_off [n + 1], ann_col, ann_gt, ann_uops, ann_uet, host_rows): per record the
    sample columns that have a summarised record, ascending, with the gt code (0 none, 1 "1|0", 2 "0|1"), the evidence count and uet_code;
    host_rows: the records the caller writes with the per-record code whatever the device makes of them (a count the device does not print,
    a key whose summary raises).  None: read_records does not index by its own fields (the caller takes the host route)."""
    by_site = {}
    for key, rec in read_records.items():
        try:
            site = tuple(str(rec["region"][k]) for k in ("chrom", "start", "end")) + (str(rec["vartype"]),)
            kid = rec["kid"]
            if "{}_{}_{}_{}_{}".format(site[0], site[1], site[2], kid, site[3]) != key:
                return None
        except (KeyError, TypeError):
            return None
        by_site.setdefault(site, []).append((kid, key))
    columns = {}
    for i, name in enumerate(samples):
        columns.setdefault(name, []).append(i)
    ann_off, col, gtc, uops, uet, host_rows = [0], [], [], [], [], []
    for k, site in enumerate(sites):
        rows = []
        for kid, key in by_site.get(tuple(str(x) for x in site), ()) if site is not None else ():
            if kid not in columns:
                continue
            rec = read_records[key]
            try:
                s = summarize_record(rec, include_ambiguous, verbose, evidence_min_ratio)
            except Exception:  # (the host writer meets it only at a cell that passes the gate: the per-record code decides)
                rows = None
                break
            if s is None:
                continue
            n, e = s["evidence_count"], uet_code(s["evidence_types"])
            if not isinstance(n, int) or isinstance(n, bool) or not -1 <= n <= UOPS_DEVICE_MAX:
                rows = None
                break
            code = 1 if s["origin_parent"] == rec["dad"] else (2 if s["origin_parent"] == rec["mom"] else 0)
            rows.extend((c, code, n, e) for c in columns[kid])
        if rows is None:
            host_rows.append(k)
            rows = []
        rows.sort()
        for c, code, n, e in rows:
            col.append(c); gtc.append(code); uops.append(n); uet.append(e)
        ann_off.append(len(col))
    return (np.asarray(ann_off, np.int64), np.asarray(col, np.int32), np.asarray(gtc, np.uint8), np.asarray(uops, np.int32),
            np.asarray(uet, np.int8), host_rows)


def _write_vcf_device(in_vcf_name, read_records, include_ambiguous, verbose, outfile, evidence_min_ratio, backend):
    """The annotated VCF with its record lines rewritten on the device (backend.vcf_rows -> uz_vcf_rows; csrc/vcf_row.hpp states the rules).
    The header is written here; a record the device hands back, and one vcf_annotations names, is written by _annotated_line.  -> False, nothing
    written: the file takes the host route whole -- the native decoder refuses it, it holds a byte outside ASCII or a '\r' (text mode reads
    those differently), its header is not one `#CHROM` line behind `##` lines, or its records are not the lines read_vcf would see."""
    import ctypes as C
    from . import io_native
    from .io_vcf import site_of
    try:
        table = io_native.read_vcf_table(in_vcf_name)
        view = io_native.vcf_samples_text(table)
    except (io_native.IoError, OSError):
        return False
    n = int(view.n_records)
    raw = C.string_at(view.text, int(view.text_bytes))
    header, samples = list(table.header), list(table.samples)
    if not raw.isascii() or b"\r" in raw or not header or [h[:2] != "##" for h in header] != [False] * (len(header) - 1) + [True]:
        return False
    if header[-1].split("\t")[9:] != samples or n != sum(1 for ln in raw.split(b"\n") if ln and ln[:1] != b"#"):
        return False
    samp_at = np.ctypeslib.as_array(C.cast(view.samp_at, C.POINTER(C.c_uint64)), (n,)) if n else np.zeros(0, np.uint64)
    line_end = np.ctypeslib.as_array(C.cast(view.line_end, C.POINTER(C.c_uint64)), (n,)) if n else np.zeros(0, np.uint64)
    line_at = np.zeros(n, np.int64)
    sites = []
    for k in range(n):
        s, e = int(samp_at[k]), int(line_end[k])
        a = line_at[k] = raw.rfind(b"\n", 0, s) + 1
        if raw[a:a + 1] == b"#":
            return False
        if s >= e:
            sites.append(None)  # (no sample column: the device hands it back)
            continue
        chrom, start, _, _, end, info = site_of(raw[a:s - 1].decode().split("\t"))
        vartype = info.get("SVTYPE")
        sites.append((chrom, start, end, SNV_TYPES[0] if vartype is None else vartype))
    return _annotate_and_write(raw, header, samples, samp_at, line_end, line_at, sites, view, read_records, include_ambiguous, verbose, outfile,
                               evidence_min_ratio, backend)


def _annotate_and_write(raw, header, samples, samp_at, line_end, line_at, sites, view, read_records, include_ambiguous, verbose, outfile, evidence_min_ratio,
                        backend, keys_from_sites=False):
    """The annotate-and-write half of the device route, over record text from either source -- a text DNM file's own (_write_vcf_device) or a
    BCF's converted one (_write_vcf_from_bcf): raw bytes, the header lines, per record line_at / samp_at / line_end in raw and the site its key is
    formed from; view: the uz_vcf_text_view over them.  keys_from_sites: a record written by the per-record host code takes its key from
    `sites`, not from its text (a BCF's keys come from its table, as read_vars_vcf forms them).  -> False, nothing written: read_records does
    not index by its own fields."""
    from .io_vcf import parse_record
    n = len(sites)
    ann = vcf_annotations(sites, samples, read_records, include_ambiguous, verbose, evidence_min_ratio)
    if ann is None:
        return False
    ann_off, ann_col, ann_gt, ann_uops, ann_uet, host_rows = ann
    text, off, handed_back = backend.vcf_rows(view, line_at, ann_off, ann_col, ann_gt, ann_uops, ann_uet)
    VCF_STATS["vcf_calls"] += 1
    by_host = sorted(set(host_rows) | set(np.flatnonzero(handed_back).tolist()))
    # read_vcf parses every record before the writer meets the first: so do the records that come back
    parsed = [parse_record(raw[int(line_at[k]):int(line_end[k])].decode(), samples) for k in by_host]
    if keys_from_sites:
        parsed = [_with_site(r, sites[k]) for k, r in zip(by_host, parsed)]
    parts = [("\n".join(_annotated_header(header)) + "\n").encode()]
    body, at = memoryview(text), 0
    for k, r in zip(by_host, parsed):
        parts.append(body[at:int(off[k])])
        parts.append((_annotated_line(r, samples, read_records, include_ambiguous, verbose, evidence_min_ratio) + "\n").encode())
        at = int(off[k + 1])
    parts.append(body[at:int(off[n])])
    VCF_STATS["vcf_device_rows"] += n - len(by_host)
    VCF_STATS["vcf_host_rows"] += len(by_host)
    write_output(outfile, parts)
    return True


BCF_STATS = {"bcf_device_rows": 0, "bcf_host_rows": 0, "bcf_calls": 0}  # records whose text the device wrote / bcf_text.line wrote, uz_bcf_rows calls


def bcf_route():
    """UZ_BCF_ROUTE: "device" -- a BCF of DNMs becomes record text on the device (uz_bcf_rows; csrc/bcf_row.hpp states the rules), which the
    annotated-VCF writer then takes -- or "host" (unfazed_amd/bcf_text.py converts every record).  Not set, or any other value: None, and the
    annotated VCF of a BCF is refused with BCF_OUTPUT_MESSAGE as before."""
    v = os.environ.get("UZ_BCF_ROUTE", "").lower()
    return v if v in ("device", "host") else None


def _with_site(r, site):
    """a parsed record with the key fields of `site` (chrom, start, end, vartype): what _annotated_line forms its key from"""
    chrom, start, end, vartype = site
    r.chrom, r.start, r.end = chrom, start, end
    r.info = dict(r.info)
    r.info["SVTYPE"] = vartype
    return r


def _write_vcf_from_bcf(in_vcf_name, read_records, include_ambiguous, verbose, outfile, evidence_min_ratio):
    """The annotated VCF of a BCF of DNMs (UZ_BCF_ROUTE; reference unfazed.py:530 takes such a file and writes text from it).  The records become
    VCF lines -- on the device (backend.bcf_rows), the handed-back ones by bcf_text.line, or all of them by bcf_text.line -- the header lines are
    the table's, and the lines then go the way a text file's go: _annotate_and_write on the device route, parse_record + _annotated_line on the
    host route (and for more than one rank).  The keys come from the table (pos, end, INFO SVTYPE), exactly as read_vars_vcf forms them."""
    from . import abi, bcf_text, io_native
    from .io_vcf import parse_record
    table = io_native.read_vcf_table(in_vcf_name)
    view = io_native.vcf_bcf_lines(table)
    n = int(view.n_records)
    header, samples = list(table.header), list(table.samples)
    chrom_of = np.repeat(np.arange(len(table.contigs)), np.diff(table.contig_off))
    sites = []
    for j in range(n):
        vartype = table.info(j, "SVTYPE")
        sites.append((table.contigs[int(chrom_of[j])], int(table.pos[j]), int(table.end[j]), SNV_TYPES[0] if vartype is None else vartype))
    device = bcf_route() == "device" and int(os.environ.get("WORLD_SIZE", "1")) <= 1
    arrays = None

    def converted(only=None):
        nonlocal arrays
        if arrays is None:
            arrays = abi.bcf_lines_arrays(view)
        return bcf_text.lines(arrays[0], arrays[1], arrays[2], arrays[3], len(samples), only=only)
    if device:
        from . import session
        backend = session.get_backend()  # asked for by name: the route makes its backend, and fails loudly without a device
        text, off, samp_at, handed_back = backend.bcf_rows(view)
        BCF_STATS["bcf_calls"] += 1
        by_host = np.flatnonzero(handed_back).tolist()
        line_at, line_end, samp_at = off[:-1].astype(np.int64), off[1:].astype(np.int64) - 1, samp_at.astype(np.int64)
        if by_host:  # the handed-back records' lines spliced in where they belong: every later offset moves by their bytes
            lines = [ln.encode() + b"\n" for ln in converted(by_host)]
            parts, at, grow = [], 0, np.zeros(n + 1, np.int64)
            for k, ln in zip(by_host, lines):
                parts += [text[at:int(off[k])], ln]
                at = int(off[k])
                grow[k + 1] = len(ln)
            parts.append(text[at:])
            text = b"".join(parts)
            shift = np.cumsum(grow)
            line_at, line_end = line_at + shift[:-1], off[1:].astype(np.int64) + shift[1:] - 1
            samp_at = samp_at + shift[:-1]
            for k, ln in zip(by_host, lines):
                cols = ln[:-1].split(b"\t")
                samp_at[k] = line_at[k] + (len(b"\t".join(cols[:9])) + 1 if len(cols) > 9 else len(ln) - 1)
        BCF_STATS["bcf_device_rows"] += n - len(by_host)
        BCF_STATS["bcf_host_rows"] += len(by_host)
        tview = abi.vcf_text_view(np.frombuffer(text, np.uint8), samp_at.astype(np.uint64), line_end.astype(np.uint64), len(samples))
        if hasattr(backend, "vcf_rows") and _annotate_and_write(text, header, samples, samp_at, line_end, line_at, sites, tview, read_records, include_ambiguous,
                                                                verbose, outfile, evidence_min_ratio, backend, keys_from_sites=True):
            return
        lines = [text[int(a):int(e)].decode() for a, e in zip(line_at, line_end)]
    else:
        lines = converted()
        BCF_STATS["bcf_host_rows"] += n
    records = [_with_site(parse_record(ln, samples), site) for ln, site in zip(lines, sites)]
    out = _annotated_header(header)
    for r in records:
        out.append(_annotated_line(r, samples, read_records, include_ambiguous, verbose, evidence_min_ratio))
    VCF_STATS["vcf_host_rows"] += n
    write_output(outfile, ["\n".join(out) + "\n"])


def _dnm_reader(path):
    if path.endswith(".bed"):
        return read_vars_bed, "bed"
    if path.endswith(".bed.gz"):
        return read_vars_bedzip, "bed"
    if any(path.endswith(t) for t in VCF_TYPES):
        return read_vars_vcf, "vcf"
    sys.exit("dnms file type is unrecognized. Must be bed, bed.gz, vcf, vcf.gz, or bcf")


def _route_variants(variants, bam_names, cram_ref):
    """Attach the kid's alignment file to every DNM and split the list into point variants and SVs.  A kid
    without exactly one alignment file is reported once and its DNMs are dropped."""
    snvs, svs, kids, reported = [], [], set(), set()
    for var in variants:
        sample = var["kid"]
        files = bam_names.get(sample)
        if files is None or len(files) != 1:
            if sample not in reported:
                reported.add(sample)
                if files is None:
                    _say("missing alignment file for", sample)
                else:
                    _say("multiple alignment files for", sample + ".",
                         "Please specify correct alignment file using --bam-pairs")
            continue
        kids.add(sample)
        var["bam"] = next(iter(files))
        var["cram_ref"] = cram_ref
        kind = var["vartype"].upper()
        if kind in SV_TYPES:
            svs.append(var)
        elif kind in SNV_TYPES:
            snvs.append(var)
    return snvs, svs, kids


def _ranks(args):
    """(rank, world, torch.distributed or None): more than one rank when a launcher (torchrun, or `--gpus N` which starts the ranks
    itself, __main__.spawn_ranks) put RANK / WORLD_SIZE into the environment.  The only communication is the gather of the per-shard
    records (host objects) on rank 0: gloo, whatever the ranks compute on."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 0, 1, None
    import datetime
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(hours=12))
    return rank, world, dist


BED_ROUTE_DEFAULT = "host"  # UZ_BED_ROUTE not set: "device" is admitted only once profiles/bed_route_ab.json shows every device run ahead of every host run


def bed_route() -> str:
    """UZ_BED_ROUTE: "device" -- a single-rank call that writes BED gets its point variants' lines from the device (phase_snvs_bed) -- or
    "host" (the records dict and summarize.bed_lines).  Annotated-VCF output and calls of more than one rank always take the dict route."""
    return "device" if os.environ.get("UZ_BED_ROUTE", BED_ROUTE_DEFAULT).lower() == "device" else "host"


def unfazed(args):
    """reference unfazed.py:518-667: read the DNMs, find each kid's alignment file and pedigree entry, phase
    SVs and point variants through the two phasers, write BED or annotated VCF."""
    global QUIET_MODE
    bam_names = get_bam_names(args.bam_dir, args.bam_pairs, args.reference)
    reader, input_type = _dnm_reader(args.dnms)
    QUIET_MODE = args.quiet
    output_type = args.output_type or input_type
    if output_type == "vcf" and input_type != "vcf":
        print("Invalid option: --output-type is vcf, but input is not a vcf type. "
              + "Rerun with `--output-type bed` or input dnms as one of the following:", ", ".join(VCF_TYPES),
              file=sys.stderr)
        sys.exit(1)
    if output_type == "vcf" and bcf_route() is None and (args.dnms.endswith("bcf") or _is_bcf(args.dnms)):
        sys.exit(BCF_OUTPUT_MESSAGE)  # known before any phasing is done
    snvs, svs, kids = _route_variants(reader(args.dnms), bam_names, args.reference)
    pedigrees = parse_ped(args.ped, kids)
    kids = list(pedigrees)
    snvs = [v for v in snvs if v["kid"] in pedigrees]
    svs = [v for v in svs if v["kid"] in pedigrees]
    if not snvs and not svs:
        sys.exit("No phaseable variants")
    thresholds = (args.threads, args.build, args.no_extended, args.multiread_proc_min, args.quiet, args.ab_homref,
                  args.ab_homalt, args.ab_het, args.min_gt_qual, args.min_depth, args.search_dist,
                  args.insert_size_max_sample, args.stdevs, args.min_map_qual, args.readlen, args.split_error_margin)
    # SVs first, as the reference does (:601-646): the order of the per-variant messages on stderr is part of
    # the surface; on a key collision the SV record wins (its final merge, :648-649)
    sv_records, snv_records = {}, {}
    rank, world, dist = _ranks(args)
    if world > 1:
        # one process per GPU, contiguous DNM shards, no collective on the data path: the reference's task pool
        # over DNMs (snv_phaser.py:244-298) as shards; the records are gathered on rank 0, which writes the output.  A batch that
        # takes the many-variant path as a whole (--multiread-proc-min) takes it in every shard.
        from . import session, shard
        session.set_device(int(os.environ.get("LOCAL_RANK", rank)))
        mpm = args.multiread_proc_min

        def shard_thresholds(batch):
            return (args.threads, args.build, args.no_extended, 0 if len(batch) >= mpm else 1 << 60) + thresholds[4:]
        if svs:
            sv_records = shard.phase_sharded(phase_svs, svs, kids, pedigrees, args.sites, *shard_thresholds(svs), rank=rank, world=world, dist=dist,
                                             evidence_min_ratio=args.evidence_min_ratio,
                                             allele_balance_only=getattr(args, "sv_allele_balance_only", False))
        if snvs:
            snv_records = shard.phase_sharded(phase_snvs, snvs, kids, pedigrees, args.sites, *shard_thresholds(snvs), rank=rank, world=world, dist=dist,
                                              evidence_min_ratio=args.evidence_min_ratio)
        dist.barrier()
        dist.destroy_process_group()
        if rank != 0:
            return
        sv_records, snv_records = sv_records or {}, snv_records or {}
    else:
        if svs:
            sv_records = phase_svs(svs, kids, pedigrees, args.sites, *thresholds, evidence_min_ratio=args.evidence_min_ratio,
                                   allele_balance_only=getattr(args, "sv_allele_balance_only", False))
        if snvs and output_type == "bed" and bed_route() == "device":
            # the point variants' lines are written on the device (snv_phaser.phase_snvs_bed); the SVs keep their records, whose lines are
            # merged into the sort behind the point variants' -- the order `dict(snv_records); update(sv_records)` gives
            rows = phase_snvs_bed(snvs, kids, pedigrees, args.sites, *thresholds, evidence_min_ratio=args.evidence_min_ratio,
                                  include_ambiguous=args.include_ambiguous, verbose=args.verbose)
            rows.write(args.outfile, extra_records=sv_records)
            return
        if snvs:
            snv_records = phase_snvs(snvs, kids, pedigrees, args.sites, *thresholds, evidence_min_ratio=args.evidence_min_ratio)
    records = dict(snv_records)
    records.update(sv_records)
    if output_type == "vcf":
        write_vcf_output(args.dnms, records, args.include_ambiguous, args.verbose, args.outfile, args.evidence_min_ratio)
    else:
        write_bed_output(records, args.include_ambiguous, args.verbose, args.outfile, args.evidence_min_ratio)
