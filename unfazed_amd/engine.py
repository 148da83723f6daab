"""ctypes binding of libunfazed_hip.so (include/unfazed_hip.h) and the backend
object the host path drives.  There is no CPU fallback: if the library or a
gfx950 device is missing, construction raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UZ_HIP_LIB", os.path.join(_HERE, "libunfazed_hip.so"))

SIZING_REDUCED_WORDS = 263  # unfazed_hip.h UZ_SIZING_REDUCED_WORDS
K_SITE_SCAN, K_WINDOW_COUNT, K_WINDOW_FILL, K_PHASE, K_SIZING, K_CNV, K_FAMILY_PACK, K_CNV_DENSE = 0, 1, 2, 3, 4, 5, 6, 7
K_VCF_TABS, K_VCF_CELLS, K_VCF_COPY = 8, 9, 10  # uz_samples_from_text: the two kernels and (not a kernel) the chunks' copies
K_BCF_CELLS, K_BCF_COPY = 11, 12  # uz_samples_from_bcf: its kernel and (not a kernel) its chunks' copies
K_HEAD_INFLATE, K_HEAD_WALK, K_HEAD_RANK = 13, 14, 15  # uz_head_walk: inflate + CRC-32 of a group's heads, k_head_walk; uz_head_rank: k_head_rank
K_BED_SIZE, K_BED_FILL = 16, 17  # uz_bed_rows: k_bed_size + the scan of the lengths, k_bed_fill
K_VCFOUT_SIZE, K_VCFOUT_FILL = 18, 19  # uz_vcf_rows: k_vcfout_size + the scan of the lengths, k_vcfout_fill (per chunk)
K_BCFOUT_SIZE, K_BCFOUT_FILL = 20, 21  # uz_bcf_rows: k_bcfout_size + the scan of the lengths, k_bcfout_fill (per chunk)
K_DEFLATE, K_DEFLATE_FRAME = 22, 23  # uz_bgzf_deflate: k_bgzf_deflate (or k_bgzf_deflate_dyn) + k_bgzf_crc32_out + the scan of the sizes, k_bgzf_frame (per chunk)
K_TBX_KEYS, K_TBX_TABLE = 24, 25  # uz_bgzf_deflate_indexed: k_tbx_mark + scan + k_tbx_starts + k_tbx_keys (per chunk), the table passes behind the last chunk
DEFLATE_CODES = {"fixed": 0, "dynamic": 1}  # unfazed_hip.h UZ_DF_CODE_*
TBX_PRESETS = {"vcf": 0, "bed": 1}  # unfazed_hip.h UZ_TBX_PRESET_*
HEAD_NONE, HEAD_DONE, HEAD_END, HEAD_BAD = 0, 1, 2, 3  # unfazed_hip.h UZ_HEAD_*
HEAD_MAX_BYTES = 8 << 30  # inflated bytes of one uz_head_walk launch unless UZ_HEAD_MAX_BYTES says otherwise: a choice, not a measurement
HEAD_MAX_ROUNDS = 8       # walks of one file before it is handed back to the host route

EXPORTS = [
    "uz_create", "uz_destroy", "uz_last_error", "uz_sync", "uz_set_params",
    "uz_sites_upload", "uz_family_upload", "uz_sites_family_upload_async", "uz_samples_upload", "uz_samples_from_text", "uz_samples_from_bcf", "uz_samples_unsettled", "uz_samples_settle", "uz_families_from_samples", "uz_family_fetch", "uz_sites_fetch", "uz_samples_free", "uz_reads_upload", "uz_reads_upload_packed", "uz_reads_wait", "uz_reads_headers", "uz_reads_columns", "uz_reads_marks", "uz_bgzf_inflate", "uz_bgzf_inflate_to_host", "uz_bam_walk", "uz_bam_walk_many", "uz_reads_files", "uz_crc32_blocks", "uz_bam_walk_fetch", "uz_bam_walk_release", "uz_reads_from_bam",
    "uz_bam_walk_flags", "uz_bam_join", "uz_bam_join_needs", "uz_bam_join_fetch", "uz_reads_from_walk", "uz_reads_names", "uz_walk_slot_stats", "uz_walk_reserve",
    "uz_pinned_alloc", "uz_pinned_free",
    "uz_sites_adopt_device", "uz_family_adopt_device", "uz_reads_adopt_device",
    "uz_sites_free", "uz_reads_free", "uz_drop_derived",
    "uz_site_scan", "uz_site_scan_many", "uz_site_classes", "uz_find", "uz_find_fetch", "uz_find_answer", "uz_find_stats", "uz_find_cohort",
    "uz_phase", "uz_phase_begin", "uz_phase_end", "uz_phase_cohort", "uz_phase_cohort_joined", "uz_phase_votes", "uz_phase_groups", "uz_phase_sizing_fetch", "uz_phase_cnv", "uz_phase_cnv_cohort", "uz_phase_cnv_sites",
    "uz_bed_rows", "uz_bed_rows_lists", "uz_vcf_rows", "uz_bcf_rows", "uz_bgzf_deflate", "uz_bgzf_deflate_coded", "uz_bgzf_deflate_indexed",
    "uz_prof_enable", "uz_prof_reset", "uz_prof_get", "uz_prof_units",
    "uz_head_walk", "uz_head_rank", "uz_head_fetch", "uz_head_free",
]

_lib = None


class UnfazedHipError(RuntimeError):
    pass


def load_library(path: Optional[str] = None):
    """dlopen the HIP library and declare the prototypes.  Fails loudly."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise UnfazedHipError(
            "%s not found: build it with `python -m unfazed_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the phasing path." % p
        )
    L = C.CDLL(p)
    vp, i32, i64p = C.c_void_p, C.c_int, C.c_void_p
    L.uz_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.uz_destroy.argtypes = [vp]
    L.uz_destroy.restype = None
    L.uz_last_error.argtypes = [vp]
    L.uz_last_error.restype = C.c_char_p
    L.uz_sync.argtypes = [vp]
    L.uz_set_params.argtypes = [vp, vp]
    L.uz_reads_wait.argtypes = [vp, C.c_int]
    L.uz_reads_headers.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    L.uz_reads_columns.argtypes = [vp, C.c_int] + [vp] * 10
    L.uz_reads_marks.argtypes = [vp, C.c_int, vp, vp]
    L.uz_bgzf_inflate.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp, vp, C.c_int, C.POINTER(C.c_double)]
    L.uz_bgzf_inflate_to_host.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp, vp]
    L.uz_crc32_blocks.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
    L.uz_bam_walk.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, vp, vp, vp]
    L.uz_bam_walk_many.argtypes = L.uz_bam_walk.argtypes[:-2] + [C.c_int32, vp, vp, vp, vp, vp, vp]
    L.uz_reads_files.argtypes = [vp, C.c_int, C.c_int32, vp, vp, vp]
    L.uz_bam_walk_fetch.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.uz_bam_walk_release.argtypes = [vp, C.c_int]
    L.uz_reads_from_bam.argtypes = [vp, C.c_int, vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, C.c_int32, vp, C.c_int64, vp]
    L.uz_bam_walk_flags.argtypes = [vp, C.c_int, vp, vp]
    L.uz_bam_join.argtypes = [vp, C.c_int, C.c_int32, vp, C.c_int32, C.c_int, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, vp, vp, vp]
    L.uz_bam_join_needs.argtypes = [vp, C.c_int, vp]
    L.uz_bam_join_fetch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.uz_reads_from_walk.argtypes = [vp, C.c_int, C.c_int32, C.c_int, vp, vp]
    L.uz_reads_names.argtypes = [vp, C.c_int, vp, C.c_int64, vp, vp]
    L.uz_walk_slot_stats.argtypes = [vp, vp]
    L.uz_walk_reserve.argtypes = [vp, C.c_int]
    L.uz_pinned_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.uz_pinned_free.argtypes = [vp]
    L.uz_pinned_free.restype = None
    for f in ("uz_sites_upload", "uz_reads_upload", "uz_reads_upload_packed", "uz_sites_adopt_device", "uz_reads_adopt_device"):
        getattr(L, f).argtypes = [vp, vp, C.POINTER(C.c_int)]
    for f in ("uz_family_upload", "uz_family_adopt_device"):
        getattr(L, f).argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int)]
    L.uz_sites_family_upload_async.argtypes = [vp, vp, vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.uz_samples_upload.argtypes = [vp, C.c_int, vp, C.POINTER(C.c_int)]
    L.uz_families_from_samples.argtypes = [vp, C.c_int, C.c_int32, vp, vp, vp, vp]
    L.uz_samples_from_text.argtypes = [vp, C.c_int, vp, C.c_int32, vp, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.uz_samples_from_bcf.argtypes = L.uz_samples_from_text.argtypes
    L.uz_samples_unsettled.argtypes = [vp, C.c_int, vp]
    L.uz_samples_settle.argtypes = [vp, C.c_int, C.c_int64, vp, vp]
    L.uz_family_fetch.argtypes = [vp, C.c_int, vp, vp]
    L.uz_sites_fetch.argtypes = [vp, C.c_int, vp, vp, vp, vp]
    L.uz_samples_free.argtypes = [vp, C.c_int]
    L.uz_drop_derived.argtypes = [vp]
    L.uz_sites_free.argtypes = [vp, C.c_int]
    L.uz_reads_free.argtypes = [vp, C.c_int]
    L.uz_site_scan.argtypes = [vp, C.c_int]
    L.uz_site_scan_many.argtypes = [vp, vp, C.c_int32]
    L.uz_site_classes.argtypes = [vp, C.c_int, vp]
    L.uz_find.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    L.uz_find_fetch.argtypes = [vp, vp, vp, vp]
    L.uz_find_answer.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_size_t, vp]
    L.uz_find_stats.argtypes = [vp, vp]
    L.uz_find_cohort.argtypes = [vp, vp, C.c_int32, vp, C.c_int, vp, vp]
    L.uz_phase.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.uz_phase_begin.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int]
    L.uz_phase_end.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.uz_phase_cohort.argtypes = [vp, vp, C.c_int32, vp, C.c_int, vp, vp, vp, vp]
    L.uz_phase_cohort_joined.argtypes = [vp, C.c_int, vp, C.c_int32, vp, vp, C.c_int, vp, vp, vp, vp]
    L.uz_phase_cnv.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.uz_phase_cnv_cohort.argtypes = [vp, vp, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.uz_phase_cnv_sites.argtypes = [vp, vp, vp]
    L.uz_phase_votes.argtypes = [vp, vp, vp]
    L.uz_phase_groups.argtypes = [vp, vp, vp]
    L.uz_phase_sizing_fetch.argtypes = [vp, vp, vp, vp, vp, vp]
    L.uz_bed_rows.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
    L.uz_bed_rows_lists.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int32, vp, vp, vp, C.c_uint32, vp, vp, C.c_int32, vp, vp]
    L.uz_vcf_rows.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.uz_bgzf_deflate.argtypes = [vp, vp, C.c_int64, vp, vp, vp, C.c_int, C.POINTER(C.c_double)]
    L.uz_bgzf_deflate_coded.argtypes = [vp, vp, C.c_int64, C.c_int, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_double)]
    L.uz_bgzf_deflate_indexed.argtypes = [vp, vp, C.c_int64, C.c_int, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_double), C.c_int, vp]
    L.uz_bcf_rows.argtypes = [vp, vp, vp, vp, vp, vp]
    L.uz_head_walk.argtypes = [vp, C.POINTER(C.c_int), C.c_int32, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.uz_head_rank.argtypes = [vp, C.c_int, C.c_int32, vp, vp, vp]
    L.uz_head_fetch.argtypes = [vp, C.c_int, C.c_int32, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.uz_head_free.argtypes = [vp, C.c_int]
    L.uz_prof_enable.argtypes = [vp, C.c_int]
    L.uz_prof_reset.argtypes = [vp]
    L.uz_prof_get.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.uz_prof_units.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    for name in EXPORTS:
        fn = getattr(L, name)
        if name not in ("uz_destroy", "uz_last_error", "uz_pinned_free"):
            fn.restype = C.c_int
    if path is None:
        _lib = L
    return L


class HipEngine:
    """One context on one GPU.  Backend interface used by hostpath.PhasingHost."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.uz_create(int(device), C.byref(h))
        if rc != 0:
            raise UnfazedHipError(
                "uz_create(device=%d) failed with %d: a gfx950 (MI355X) device is required; "
                "there is no CPU fallback" % (device, rc)
            )
        self.h = h
        self.device = device
        self._keep: List[object] = []
        self._staged = {}
        self._staged_sites = {}
        self._params = None
        import threading
        self._inflate_lock = threading.Lock()
        self._walked = 0  # tables built from joined batches (reads_from_bam, from whichever thread): the slots are reserved after the 1st, 2nd and 4th
        self._walked_lock = threading.Lock()
        # walked batches on the device at once, each on its slot's own streams.  Round 5 (the host's joins the bound): two measured 10 % slower than
        # one; with the joins on the device the device's chain is the bound and a batch's walk -- a latency-bound kernel of ~1 900 wavefronts -- leaves
        # the chip to the next batch's inflate: 1 / 2 / 3 at once = 117 / 130 / 128 k DNMs/s in bench.py's feed pass
        self._walk_sem = threading.BoundedSemaphore(int(os.environ.get("UZ_WALKS_AT_ONCE", "2")))
        self._slots = {}  # stage_reads: slot -> (PinnedPool of the staged columns, PinnedPair of the gathered / inflated blocks)

    def close(self):
        for pool, pair in getattr(self, "_slots", {}).values():
            pool.free_all()
            pair.free_all()
        self._slots = {}
        if getattr(self, "_head_pin", None) is not None:
            self._head_pin[0].free_all()
            self._head_pin = None
        if getattr(self, "h", None):
            self.L.uz_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            msg = self.L.uz_last_error(self.h)
            raise UnfazedHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    # -------------------------------------------------------------- staging
    def set_params(self, params: abi.Params):
        self._ck(self.L.uz_set_params(self.h, C.byref(params)), "uz_set_params")
        self._params = params

    def upload_sites(self, sites) -> int:
        v = abi.sites_view(sites)
        sid = C.c_int(-1)
        self._ck(self.L.uz_sites_upload(self.h, v.ref(), C.byref(sid)), "uz_sites_upload")
        return sid.value

    def upload_sites_view(self, held: abi.Held) -> int:
        """the same from a prepared view (e.g. columns in pinned memory)"""
        sid = C.c_int(-1)
        self._ck(self.L.uz_sites_upload(self.h, held.ref(), C.byref(sid)), "uz_sites_upload")
        return sid.value

    def add_family(self, sites_h: int, gt, rd, ad, gq, wide=None) -> int:
        v = abi.family_view(gt, rd, ad, gq, wide)
        fid = C.c_int(-1)
        self._ck(self.L.uz_family_upload(self.h, int(sites_h), v.ref(), C.byref(fid)), "uz_family_upload")
        return fid.value

    # ---- the cohort form: the samples' columns in HBM once, trios made from them on the device
    def upload_samples(self, sites_h: int, cols) -> int:
        """model.SampleColumns (SitesTable.sample_columns; rows in pinned memory -- alloc=PinnedPool.alloc -- for link speed) -> a sample
        table of the sites table (uz_samples_upload: queued on the copy stream).  The arrays are kept until the table is freed."""
        v = abi.samples_view(cols)
        mid = C.c_int(-1)
        self._ck(self.L.uz_samples_upload(self.h, int(sites_h), v.ref(), C.byref(mid)), "uz_samples_upload")
        self._samples = getattr(self, "_samples", {})
        self._samples[mid.value] = (int(sites_h), v)
        return mid.value

    def samples_from_text(self, sites_h: int, table, pick, settle: bool = True):
        """The sample table of a natively decoded text VCF without the host parsing its sample cells: the table's record text goes to the
        device in chunks and two kernels read GT, AD (or RO / AO) and GQ of the sample columns `pick` (indices into table.samples) into the
        rows (uz_samples_from_text).  The records the device will not vouch for come back (uz_samples_unsettled) and are read by the host's
        own reader -- io_native.vcf_record_samples, then pack_samples: errors are the eager decode's -- and settled (uz_samples_settle).
            -> (handle, number of sites handed back).  settle=False leaves the round trip to the caller (settle_samples)."""
        from . import io_native
        return self._samples_from(self.L.uz_samples_from_text, "uz_samples_from_text", io_native.vcf_samples_text(table), sites_h, table, pick, settle)

    def samples_from_bcf(self, sites_h: int, table, pick, settle: bool = True):
        """The same from a natively decoded BCF (uz_samples_from_bcf): only the value arrays of GT, AD, RO, AO and GQ go to the device, in chunks,
        and one kernel reads the samples `pick` into the rows.  Handed back and settled like the text's: records with a depth the 16-bit rows
        cannot hold or a field in a type the kernel does not take.  -> (handle, number of sites handed back)"""
        from . import io_native
        return self._samples_from(self.L.uz_samples_from_bcf, "uz_samples_from_bcf", io_native.vcf_samples_bcf(table), sites_h, table, pick, settle)

    def _samples_from(self, call, name, view, sites_h, table, pick, settle):
        pick = np.ascontiguousarray(pick, np.int32)
        mid, nu = C.c_int(-1), C.c_int64(0)
        self._ck(call(self.h, int(sites_h), C.byref(view), int(pick.size), pick.ctypes.data, C.byref(mid), C.byref(nu)), name)
        self._samples = getattr(self, "_samples", {})
        self._samples[mid.value] = (int(sites_h), None)
        if settle and nu.value:
            try:
                self.settle_samples(mid.value, table, pick, nu.value)
            except Exception:
                self.free_samples(mid.value)
                raise
        return mid.value, int(nu.value)

    def unsettled_sites(self, samples_h: int, n: int):
        """the n sites a table made by samples_from_text / samples_from_bcf handed back, ascending"""
        site = np.zeros(max(1, int(n)), np.int64)
        self._ck(self.L.uz_samples_unsettled(self.h, int(samples_h), site.ctypes.data), "uz_samples_unsettled")
        return site[: int(n)]

    def settle_samples(self, samples_h: int, table, pick, n: int) -> None:
        """the n handed-back sites of a table made by samples_from_text / samples_from_bcf, read by the host's reader and written over the device's rows"""
        from . import io_native
        from .model import SampleColumns, SitesTable
        pick = np.ascontiguousarray(pick, np.int32)
        site = self.unsettled_sites(samples_h, n)
        sub = SitesTable(["row%d" % r for r in range(pick.size)], [])  # the decoder's columns of those sites alone, rows in pick order
        sub.pos = np.zeros(site.size, np.int32)
        sub.gt, sub.ref_depth, sub.alt_depth, sub.gq = io_native.vcf_record_samples(table, site, pick)
        cols = SampleColumns(list(sub.samples), *io_native.pack_samples(sub, np.arange(pick.size)))
        v = abi.samples_view(cols)
        self._ck(self.L.uz_samples_settle(self.h, int(samples_h), int(site.size), site.ctypes.data, v.ref()), "uz_samples_settle")

    def families_from_samples(self, samples_h: int, kid, dad, mom) -> list:
        """the trios (kid[t], dad[t], mom[t]) -- sample indices of the table -- as families, one launch sequence (uz_families_from_samples)"""
        k, d, m = (np.ascontiguousarray(x, np.int32) for x in (kid, dad, mom))
        if not (k.size == d.size == m.size):
            raise ValueError("kid / dad / mom lists of different lengths")
        out = np.full(max(1, k.size), -1, np.int32)
        self._ck(self.L.uz_families_from_samples(self.h, int(samples_h), int(k.size), k.ctypes.data, d.ctypes.data, m.ctypes.data, out.ctypes.data),
                 "uz_families_from_samples")
        return [int(x) for x in out[: k.size]]

    def family_fetch(self, fam: int, n_sites: int):
        """a family's device columns, whatever route made it -> (gt u8 [S] with the complex bit, cols u16 [9][S]: rd k d m, ad k d m, gq k d m)"""
        gt, cols = np.zeros(max(1, n_sites), np.uint8), np.zeros((9, max(1, n_sites)), np.uint16)
        self._ck(self.L.uz_family_fetch(self.h, int(fam), gt.ctypes.data, cols.ctypes.data), "uz_family_fetch")
        return gt[:n_sites], cols[:, :n_sites] if n_sites else cols[:, :0]

    def sites_fetch(self, sid: int, n_sites: int):
        """a sites table's device columns (uz_sites_fetch; a test aid): a pending compact table is expanded first, without its family
        -> (pos i32 [S], sflags u8 [S], ref_base u8 [S], alt_base u8 [S])"""
        n = max(1, int(n_sites))
        pos, sf, rb, ab = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self._ck(self.L.uz_sites_fetch(self.h, int(sid), pos.ctypes.data, sf.ctypes.data, rb.ctypes.data, ab.ctypes.data), "uz_sites_fetch")
        return pos[:n_sites], sf[:n_sites], rb[:n_sites], ab[:n_sites]

    def free_samples(self, samples_h: int):
        self._ck(self.L.uz_samples_free(self.h, int(samples_h)), "uz_samples_free")
        getattr(self, "_samples", {}).pop(int(samples_h), None)

    def upload_sites_family_async(self, held: abi.Held, gt, rd, ad, gq, wide=None, het=None):
        """sites + one trio's genotype columns queued on the copy stream (uz_sites_family_upload_async) -> (sites id, family id);
        the arrays (pinned) must stay alive until a call using the family has returned: the engine keeps them.
        rd / ad / gq as uint8 arrays = the eight-bit link form (abi.family_columns8, which also extends `wide`).
        het = (het9, het_span_off) of io_native.pack_family_het = the het form (rd / ad / gq None; with compact sites only): such a family
        serves the SNV / breakpoint classes, finds and read stages -- CNV classes, whole-region finds and family_fetch raise UZ_E_STATE."""
        v = abi.family_view(gt, rd, ad, gq, wide, het=het)
        sid, fid = C.c_int(-1), C.c_int(-1)
        self._ck(self.L.uz_sites_family_upload_async(self.h, held.ref(), v.ref(), C.byref(sid), C.byref(fid)), "uz_sites_family_upload_async")
        self._staged_sites[sid.value] = (held, v)
        return sid.value, fid.value

    def upload_reads(self, reads, min_base_qual=None, point_only=False, fetches=None, all_bases=False, wide_no_units=False) -> int:
        """A decoded table -> HBM.  With the base-quality threshold of the run (min_base_qual = --min-gt-qual) the table
        goes over the link in the staged form (packed on the host into pinned memory, several times fewer bytes); without it
        in the ASCII form, which the device packs and which then serves any threshold.
        point_only: the table will only serve batches of point variants (SNV / indel) -- the qualities then travel as
        per-record counts + short position lists instead of the one-bit plane (uz_types.h: the list form is exact for "good"
        records, and a point-variant batch never looks at the bits of any other; an SV batch does).
        fetches = (contig, lo, hi, extra) of staging.fetch_points for the ONE batch the table will serve (point_only): records no
        fetch returns travel without bases, of the others' rows only the 32-base units that hold a fetched position (all_bases:
        --no-extended batches read mates at candidate sites nobody fetched -- every record keeps its rows).
        wide_no_units: the batch holds SVs -- their +-cutoff fetches stage no base unit (collect_reads_sv reads none); the list form of
        the qualities serves them too: the read stage asks for quality bits of records that pass goodread only (uz_types.h)."""
        v = abi.reads_view(reads)
        if min_base_qual is not None:
            from . import io_native
            pool = PinnedPool()
            rid = None
            try:
                # the staged columns back to back in one pinned block (they cross the link as one copy); the packed form is at most
                # half the size of the ASCII table, usually a small fraction
                pool.new_slab(sum(int(getattr(x, "nbytes", 0)) for x in v.arrays.values()) // 2 + (1 << 20))
                if fetches is not None and point_only:
                    full = io_native.pack_reads(v, int(min_base_qual), lists=True, with_end=True)
                    fc, flo, fhi, fex = fetches
                    packed, idx = io_native.ReadsSource(full).select(fc, flo, fhi, alloc=pool.alloc, want_index=True, all_bases=bool(all_bases),
                                                                     extra=fex, wide_no_units=bool(wide_no_units))
                    if idx.size != int(v.view.n_segs):  # record numbers are the caller's: the table must be the fetches' own reach
                        raise UnfazedHipError("upload_reads(fetches=...): the table holds records the fetches cannot reach")
                    if packed.qname_map is not None and not np.array_equal(packed.qname_map, np.arange(packed.qname_map.size, dtype=np.uint32)):
                        # name ids are the caller's too: the pair form renumbers them unless they already count first appearances
                        pool.rewind(0)
                        packed, idx = io_native.ReadsSource(full).select(fc, flo, fhi, alloc=pool.alloc, want_index=True, all_bases=bool(all_bases),
                                                                         extra=fex, wide_no_units=bool(wide_no_units), pair8=False)
                else:
                    packed = io_native.pack_reads(v, int(min_base_qual), alloc=pool.alloc, lists=bool(point_only), with_end=None, cigar_compact=True)
                rid = self.upload_reads_packed(packed)
                self.wait_reads(rid)  # the pinned buffers go back right away: the caller may drop the table
                self._staged.pop(rid, None)
            except BaseException:
                if rid is not None:  # the copy may still be reading the pinned block: let it finish before the block goes back
                    try:
                        self.wait_reads(rid)
                    except UnfazedHipError:
                        pass
                    self._staged.pop(rid, None)
                raise
            finally:
                pool.free_all()
            return rid
        rid = C.c_int(-1)
        self._ck(self.L.uz_reads_upload(self.h, v.ref(), C.byref(rid)), "uz_reads_upload")
        return rid.value

    def upload_reads_staged(self, src, fc, flo, fhi, fex, min_base_qual: int, all_bases: bool = False, wide_no_units: bool = False, walk_only: bool = False):
        """One batch straight from an indexed BAM (io_native.BamSource) uploaded as one table: stage_reads on a slot of its own, then
        upload_reads_packed.  -> (reads id, the staged view: `.qnames` maps the name ids of the result lists back to strings -- names of the
        caller's own, valid after the table is freed and after later batches are staged on any route)"""
        staged = self.stage_reads(src, fc, flo, fhi, fex, min_base_qual, all_bases=all_bases, wide_no_units=wide_no_units, slot="single", walk_only=walk_only)
        if staged is None:  # walk_only: the batch is not one for the device's walk (stage_reads) -- nothing was staged
            return None, None
        rid = None
        try:
            rid = self.upload_reads_packed(staged)
            if self._staged.get(rid) is staged:  # the link form: the pinned columns go back right away (a walked batch's table was built from HBM)
                self.wait_reads(rid)
                self._staged.pop(rid)
        except BaseException:
            if self._staged.get(rid) is staged:  # the copy may still be reading the pinned block: let it finish before the block goes back
                try:
                    self.wait_reads(rid)
                except UnfazedHipError:
                    pass
                self._staged.pop(rid, None)
            raise
        if hasattr(staged.qnames, "frozen"):  # names in the table or in the slot's buffers (a walked batch): copied out, all of them
            staged.qnames = staged.qnames.frozen()
        return rid, staged

    def stage_reads(self, src, fc, flo, fhi, fex, min_base_qual: int, all_bases: bool = False, wide_no_units: bool = False, slot=0, walk_only: bool = False):
        """One batch of an indexed BAM (io_native.BamSource) -- the records its fetches return + their mates -- made ready for
        upload_reads_packed, by the route the switches choose (read here, on every call):
          default          the blocks go up and are inflated, checked and walked in HBM (include/uz_bamwalk.h), the joins run there too
                           (csrc/k_bamjoin.hip) -> io_native.KeptBatch, whose table is built where the records lie;
          UZ_JOINS=host    ... the walk's descriptors come down and the host joins them (round 5's route);
          UZ_WALK=host     the link form, built in page-locked memory by one pass over the blocks (uz_bam_stage_*), the blocks inflated by the
                           device (inflate_blocks) -> the packed view;
          UZ_INFLATE=host  ... the blocks inflated by the host's cores.
        A walked batch keeps its compressed blocks, the inflated bytes and worst-case descriptor slices (64 B per 36 B of inflated data) in HBM
        until its table is built, in one of four slots: a batch whose blocks inflate to more than UZ_WALK_MAX_BYTES takes the link form instead
        of failing in hipMalloc.
        slot: the set of page-locked buffers to use, made when first asked for and kept from batch to batch (pinning a gigabyte takes about a
        second: round 3's product route spent 1.2 s of its 2.4 s per 20 k DNMs there).  The next stage_reads on a slot re-uses them: the table
        staged there must have landed on the device by then, and names that lie there (host joins) answer for the later batch.  May be called
        from a worker thread (hostpath._chunked_batch stages chunk k + 1 beside the device work of chunk k).
        walk_only: a batch that does not take the device's walk (the switches, or its blocks exceed UZ_WALK_MAX_BYTES) is not staged at all -> None
        (hostpath's cohort route over many files then stages its kids one by one).
        `.qnames`, `.io_stats`, `.timing` ride on the result."""
        if slot not in self._slots:
            pool = PinnedPool()
            pool.keep = True
            self._slots[slot] = (pool, PinnedPair())
        pool, pair = self._slots[slot]
        inflate = os.environ.get("UZ_INFLATE", "device") == "device"
        if inflate and os.environ.get("UZ_WALK", "device") == "device":
            pair.start()
            host_joins = os.environ.get("UZ_JOINS", "device") != "device"
            kb = src.select_kept(fc, flo, fhi, int(min_base_qual), walk=(lambda plan: self.bam_walk(plan, alloc=pair.alloc)) if host_joins else None,
                                 join=None if host_joins else self, all_bases=bool(all_bases), alloc=pair.alloc, extra=fex, release=self.bam_walk_release,
                                 walk_max_bytes=int(os.environ.get("UZ_WALK_MAX_BYTES", 16 << 30)))
            if kb is not None:
                kb._alloc = pair.alloc  # (host joins: the names of its records come back into the slot's page-locked memory: reads_from_bam)
                return kb
        if walk_only:
            return None
        pair.start()
        packed = src.select(fc, flo, fhi, int(min_base_qual), pool=pool, all_bases=bool(all_bases), extra=fex, wide_no_units=bool(wide_no_units),
                            inflate=self.inflate_blocks if inflate else None, inflate_alloc=pair.alloc if inflate else None)
        pool.end_slab()
        return packed

    def upload_reads_packed(self, packed: abi.Held) -> int:
        """Staged form, asynchronous: the arrays of `packed` must stay alive and untouched until wait_reads() or
        a phase on the table has returned (they are kept referenced here until the table is freed)."""
        if getattr(packed, "token", None) is not None and hasattr(packed, "kept"):  # a batch walked on the device (stage_reads): its table is built from HBM
            return self.reads_from_bam(packed, names=True)
        rid = C.c_int(-1)
        self._ck(self.L.uz_reads_upload_packed(self.h, packed.ref(), C.byref(rid)), "uz_reads_upload_packed")
        self._staged[rid.value] = packed
        return rid.value

    def wait_reads(self, rid: int):
        self._ck(self.L.uz_reads_wait(self.h, int(rid)), "uz_reads_wait")

    def reads_headers(self, rid: int, n: int) -> dict:
        """start / end / tlen / mate / qname of a table as the device holds them (uz_reads_headers)"""
        out = {k: np.zeros(max(1, int(n)), np.uint32 if k == "qname" else np.int32) for k in ("start", "end", "tlen", "mate", "qname")}
        self._ck(self.L.uz_reads_headers(self.h, int(rid), *(out[k].ctypes.data for k in ("start", "end", "tlen", "mate", "qname"))), "uz_reads_headers")
        return {k: v[: int(n)] for k, v in out.items()}

    def reads_columns(self, rid: int, n: int) -> dict:
        """the other columns of a table as the device holds them (uz_reads_columns; a debug read-back like reads_headers): fm (flag | mapq << 16 |
        aux << 24), l_seq, n_cigar, cigar_off, sq_off, qoff per record; the CIGAR store, the four-bit base rows (16 bytes a unit) and the low-quality
        plane (a 32-bit word a unit)"""
        sizes = (C.c_int64 * 4)()
        self._ck(self.L.uz_reads_columns(self.h, int(rid), sizes, *([None] * 9)), "uz_reads_columns")
        assert int(sizes[0]) == int(n), "the table holds %d records" % int(sizes[0])
        m = max(1, int(n))
        out = dict(fm=np.zeros(m, np.uint32), l_seq=np.zeros(m, np.uint16), n_cigar=np.zeros(m, np.uint16), cigar_off=np.zeros(m, np.uint32),
                   sq_off=np.zeros(m, np.uint32), qoff=np.zeros(m, np.uint32), cigar=np.zeros(max(1, int(sizes[1])), np.uint32),
                   seq4=np.zeros(max(1, int(sizes[2])) * 16, np.uint8), qlow=np.zeros(max(1, int(sizes[3])), np.uint32))
        self._ck(self.L.uz_reads_columns(self.h, int(rid), sizes, *(out[k].ctypes.data for k in ("fm", "l_seq", "n_cigar", "cigar_off", "sq_off", "qoff", "cigar", "seq4", "qlow"))),
                 "uz_reads_columns")
        cut = dict(cigar=int(sizes[1]), seq4=16 * int(sizes[2]), qlow=int(sizes[3]))
        return {k: v[: cut.get(k, int(n))] for k, v in out.items()}

    def reads_marks(self, rid: int, n: int) -> dict:
        """the two per-record columns reads_columns leaves out, as the device holds them (uz_reads_marks; a debug read-back): umask (the staged
        32-base units, UZ_UMASK_LISTED set for a record whose bases came as a list) and nlow (the low-quality count that travelled)"""
        m = max(1, int(n))
        out = dict(umask=np.zeros(m, np.uint16), nlow=np.zeros(m, np.uint8))
        self._ck(self.L.uz_reads_marks(self.h, int(rid), out["umask"].ctypes.data, out["nlow"].ctypes.data), "uz_reads_marks")
        return {k: v[: int(n)] for k, v in out.items()}

    def bgzf_inflate(self, data, repeat: int = 0):
        """Every BGZF block of `data` (bytes / uint8 array: a BGZF file or a run of its blocks) inflated on the device (uz_bgzf_inflate).
        -> (uint8 array of the inflated bytes, block count, mean kernel ms over `repeat` extra runs or None)"""
        buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        n, at, ins, sizes = buf.size, 0, [], []
        while at + 18 <= n:
            if not (buf[at] == 0x1F and buf[at + 1] == 0x8B and buf[at + 2] == 8 and (buf[at + 3] & 4)):
                raise UnfazedHipError("not a BGZF block at byte %d" % at)
            xlen = int(buf[at + 10]) | (int(buf[at + 11]) << 8)
            bsize, p = None, at + 12
            while p + 4 <= at + 12 + xlen:
                slen = int(buf[p + 2]) | (int(buf[p + 3]) << 8)
                if buf[p] == 66 and buf[p + 1] == 67 and slen == 2:
                    bsize = (int(buf[p + 4]) | (int(buf[p + 5]) << 8)) + 1
                p += 4 + slen
            if bsize is None or at + bsize > n:
                raise UnfazedHipError("BGZF block at byte %d: no BC field, or the block overruns the data" % at)
            ins.append(at + 12 + xlen)
            sizes.append(int(buf[at + bsize - 4]) | (int(buf[at + bsize - 3]) << 8) | (int(buf[at + bsize - 2]) << 16) | (int(buf[at + bsize - 1]) << 24))
            at += bsize
        nb = len(ins)
        in_off = np.asarray(ins, np.int64)
        out_off = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)
        out = np.zeros(max(1, int(out_off[-1])), np.uint8)
        ms = C.c_double(0.0)
        self._ck(self.L.uz_bgzf_inflate(self.h, buf.ctypes.data, int(n), nb, in_off.ctypes.data if nb else None, out_off.ctypes.data, out.ctypes.data,
                                        int(repeat), C.byref(ms)) if nb else 0, "uz_bgzf_inflate")
        return out[: int(out_off[-1])], nb, (ms.value if repeat > 0 else None)

    def bgzf_deflate(self, data, repeat: int = 0, code: str = "fixed", kinds: bool = False, index=None):
        """`data` (bytes-like / uint8 array) as BGZF blocks written on the device (uz_bgzf_deflate_coded; csrc/deflate_body.hpp and deflate_dyn.hpp
        state the rules): one block per 65 280 bytes, without the end-of-file marker.  code: "fixed" (one fixed-Huffman block per slice, or a
        stored one) or "dynamic" (per slice the shortest of a dynamic, the fixed and a stored block).  -> (bytes of the blocks, block count, mean
        kernel ms of the code's kernel over `repeat` extra passes or None), and with kinds=True a fourth item: the blocks that came out
        (stored, fixed, dynamic).
        index: None, or "vcf" / "bed": the same blocks from uz_bgzf_deflate_indexed (csrc/k_tbx.hip; csrc/tbx_key.hpp states a line's rules),
        and as the last item the tables of the text's tabix index as numpy arrays (copies): status (0, or abi.TBX_S_* bits: no tables), refs
        (abi.TBX_REF, file order), runs (abi.TBX_RUN) grouped by (tid, bin) -- a stable sort here, of a table the index's own size: within a bin
        the runs keep the file's order -- linear, n_rows, host_rows.  unfazed_amd/tabix_index.py turns them into the file."""
        if code not in DEFLATE_CODES:
            raise ValueError("bgzf_deflate: code %r (one of %s)" % (code, ", ".join(sorted(DEFLATE_CODES))))
        if index is not None and index not in TBX_PRESETS:
            raise ValueError("bgzf_deflate: index %r (None or one of %s)" % (index, ", ".join(sorted(TBX_PRESETS))))
        buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        nb, size, ptr, ms = C.c_int64(0), C.c_int64(0), C.c_void_p(), C.c_double(0.0)
        split = (C.c_int64 * 3)()
        args = (self.h, buf.ctypes.data if buf.size else None, int(buf.size), DEFLATE_CODES[code], split, C.byref(nb), C.byref(ptr), C.byref(size), int(repeat),
                C.byref(ms))
        tables = None
        if index is None:
            self._ck(self.L.uz_bgzf_deflate_coded(*args), "uz_bgzf_deflate_coded")
        else:
            view = abi.TbxView()
            self._ck(self.L.uz_bgzf_deflate_indexed(*args, TBX_PRESETS[index], C.byref(view)), "uz_bgzf_deflate_indexed")
            tables = abi.tbx_arrays(view)  # (copies: the view is the next call's)
            runs = tables["runs"]
            tables["runs"] = runs[np.lexsort((runs["bin"], runs["tid"]))]  # (lexsort is stable: a bin's chunks stay in file order)
        out = C.string_at(ptr.value, size.value) if size.value else b""  # (a copy: the context's block is the next call's)
        res = (out, int(nb.value), (ms.value if repeat > 0 else None))
        if kinds:
            res += (tuple(int(v) for v in split),)
        return res + (tables,) if index is not None else res

    def inflate_blocks(self, comp: np.ndarray, comp_bytes: int, in_off: np.ndarray, out_off: np.ndarray, out: np.ndarray):
        """The gathered BGZF blocks of a staged batch (io_native.BamSource.select(inflate=engine.inflate_blocks)) inflated on the device:
        comp[:comp_bytes] -> out[:out_off[-1]] (both best in pinned memory: PinnedPair).  May be called from a decoder's worker thread
        beside the main thread's calls (its own stream and buffers; one call at a time)."""
        with self._inflate_lock:
            rc = self.L.uz_bgzf_inflate_to_host(self.h, comp.ctypes.data, int(comp_bytes), int(in_off.size), in_off.ctypes.data, out_off.ctypes.data,
                                                out.ctypes.data)
            if rc != 0:
                raise UnfazedHipError("uz_bgzf_inflate_to_host: %s" % (self.L.uz_last_error(self.h) or b"").decode(errors="replace"))

    # ---- the record walk on the device (include/uz_bamwalk.h)
    def _walk_start(self, plan: dict):
        """uz_bam_walk (the caller holds _walk_sem: UZ_WALKS_AT_ONCE batches at a time): the plan's blocks up, inflated, checked against their
        CRC-32 and walked in HBM -> (walk id, descriptors)"""
        wid, nd = C.c_int(-1), C.c_int64(0)
        args = [self.h, plan["comp"].ctypes.data, int(plan["comp_bytes"]), int(plan["n_blocks"]), plan["in_off"].ctypes.data,
                plan["out_off"].ctypes.data, plan["blk_coff"].ctypes.data, plan["blk_crc"].ctypes.data if plan.get("blk_crc") is not None else None,
                int(plan["task"].shape[0]), plan["task"].ctypes.data, int(plan["span"].shape[0]), plan["span"].ctypes.data,
                int(plan["reach"].shape[0]), plan["reach"].ctypes.data, int(plan["fetch"].shape[0]), plan["fetch"].ctypes.data]
        files = plan.get("files")  # a source over many files (io_native.BamSource.open_many): the walk shifts references and salts names per file
        if files is not None:
            name = "uz_bam_walk_many"
            args += [int(files["salt1"].size), files["file_base"].ctypes.data, files["ref_base"].ctypes.data, files["salt1"].ctypes.data, files["salt2"].ctypes.data]
        else:
            name = "uz_bam_walk"
        rc = getattr(self.L, name)(*args, C.byref(wid), C.byref(nd))
        if rc != 0:
            raise UnfazedHipError("%s: %s" % (name, (self.L.uz_last_error(self.h) or b"").decode(errors="replace")))
        return wid.value, int(nd.value)

    def bam_walk(self, plan: dict, alloc=None):
        """io_native.BamSource.select_kept(walk=engine.bam_walk): the batch's gathered BGZF blocks inflated in HBM and walked there
        (uz_bam_walk + uz_bam_walk_fetch).  -> (descriptors, d_first, d_flags, d_walked, walk id); the inflated bytes wait on the device for
        reads_from_bam (or bam_walk_release).  May be called from a decoder's worker thread."""
        from . import io_native
        nt = int(plan["task"].shape[0])
        with self._walk_sem:  # (held across the descriptors' fetch)
            wid, n = self._walk_start(plan)
            desc = (alloc(max(1, n) * 64).view(io_native.WALK_DESC) if alloc else np.zeros(max(1, n), io_native.WALK_DESC))[: max(1, n)]
            d_first, d_flags, d_walked = np.zeros(nt + 1, np.int64), np.zeros(max(1, nt), np.int32), np.zeros(max(1, nt), np.int64)
            rc = self.L.uz_bam_walk_fetch(self.h, wid, desc.ctypes.data, d_first.ctypes.data, d_flags.ctypes.data, d_walked.ctypes.data)
            if rc != 0:
                self.L.uz_bam_walk_release(self.h, wid)
                raise UnfazedHipError("uz_bam_walk_fetch: %s" % (self.L.uz_last_error(self.h) or b"").decode(errors="replace"))
        return desc[:n], d_first, d_flags[:nt], d_walked[:nt], wid

    # ---- the joins of a walked batch on the device (csrc/k_bamjoin.hip): the primitives io_native.BamSource.select_kept(join=engine) drives
    def walk(self, plan: dict):
        """uz_bam_walk alone: blocks up, inflated, checked and walked in HBM -> (walk id, descriptors the joins can need).  Nothing comes down."""
        with self._walk_sem:
            return self._walk_start(plan)

    def walk_flags(self, token: int, nt: int):
        d_flags, d_walked = np.zeros(max(1, nt), np.int32), np.zeros(max(1, nt), np.int64)
        self._ck(self.L.uz_bam_walk_flags(self.h, int(token), d_flags.ctypes.data, d_walked.ctypes.data), "uz_bam_walk_flags")
        return d_flags[:nt], d_walked[:nt]

    def join(self, token: int, n_host: int, h_flags, n_ref: int, all_bases: bool, xdesc=None, xaux=None, look_tid=None, need_jtask=None):
        """one call of uz_bam_join -> (needs, totals [8])"""
        nn, tot = C.c_int64(0), np.zeros(8, np.int64)
        nx = 0 if xdesc is None else int(xdesc.size)
        na = 0 if xaux is None else int(xaux.size)
        nl = 0 if look_tid is None else int(look_tid.size)
        self._ck(self.L.uz_bam_join(self.h, int(token), int(n_host), h_flags.ctypes.data if h_flags is not None else None, int(n_ref), 1 if all_bases else 0,
                                      xdesc.ctypes.data if nx else None, nx, xaux.ctypes.data if na else None, na, look_tid.ctypes.data if nl else None, nl,
                                      need_jtask.ctypes.data if need_jtask is not None else None, C.byref(nn), tot.ctypes.data), "uz_bam_join")
        return int(nn.value), tot

    def join_needs(self, token: int, n: int):
        from . import io_native
        need = np.zeros(max(1, n), io_native.NEED_REC)
        self._ck(self.L.uz_bam_join_needs(self.h, int(token), need.ctypes.data), "uz_bam_join_needs")
        return need[:n]

    def join_fetch(self, token: int, n: int, n_ref: int):
        """parity / debug: the kept records of a finished join in output order -> dict(voff, qname, mate, bases, kept, contig_off, max_span)"""
        from . import io_native
        out = dict(voff=np.zeros(max(1, n), np.uint64), qname=np.zeros(max(1, n), np.uint32), mate=np.zeros(max(1, n), np.int32), bases=np.zeros(max(1, n), np.uint8),
                   kept=np.zeros(max(1, n), io_native.KEPT_REC), contig_off=np.zeros(n_ref + 1, np.int64), max_span=np.zeros(max(1, n_ref), np.int32))
        self._ck(self.L.uz_bam_join_fetch(self.h, int(token), *(out[k].ctypes.data for k in ("voff", "qname", "mate", "bases", "kept", "contig_off", "max_span"))), "uz_bam_join_fetch")
        return {k: (v[:n] if k in ("voff", "qname", "mate", "bases", "kept") else v) for k, v in out.items()}

    def reads_names_raw(self, rid: int, ids):
        """the read names of name ids of a table built from a batch joined on the device (uz_reads_names) -> (bytes back to back, off [n + 1])"""
        ids = np.ascontiguousarray(ids, np.uint32)
        n = int(ids.size)
        off, ptr = np.zeros(n + 1, np.int64), C.c_void_p()
        if n == 0:
            return np.zeros(1, np.uint8), off
        self._ck(self.L.uz_reads_names(self.h, int(rid), ids.ctypes.data, n, off.ctypes.data, C.byref(ptr)), "uz_reads_names")
        total = int(off[-1])
        buf = np.frombuffer(C.string_at(ptr.value, total), np.uint8) if total else np.zeros(1, np.uint8)  # (a copy: the context's block is the next call's)
        return buf, off

    def reads_names(self, rid: int, ids) -> list:
        from .io_native import names_of_buffer
        return names_of_buffer(*self.reads_names_raw(rid, ids))

    def reads_files(self, rid: int, ref_base):
        """a table over many files (io_native.BamSource.open_many): per file its first record and its first name id (uz_reads_files)
        -> (rec_first [n + 1], name_first [n + 1]); refused when a file's name ids are not one range"""
        ref_base = np.ascontiguousarray(ref_base, np.int32)
        n = int(ref_base.size) - 1
        rec_first, name_first = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        self._ck(self.L.uz_reads_files(self.h, int(rid), n, ref_base.ctypes.data, rec_first.ctypes.data, name_first.ctypes.data), "uz_reads_files")
        return rec_first, name_first

    def walk_slot_stats(self) -> dict:
        z = np.zeros(8, np.int64)
        self._ck(self.L.uz_walk_slot_stats(self.h, z.ctypes.data), "uz_walk_slot_stats")
        return dict(allocations=int(z[0]), parked_blocks=int(z[1]), parked_bytes=int(z[2]), slot_room=[int(x) for x in z[4:8]])

    def crc32_blocks(self, data: np.ndarray, off: np.ndarray, want: np.ndarray) -> int:
        """k_bgzf_crc32 on blocks data[off[k]:off[k+1]] (<= 64 KiB each) against want[k] -> -1, or a block whose CRC-32 differs (uz_crc32_blocks)"""
        data = np.ascontiguousarray(data, np.uint8)
        off = np.ascontiguousarray(off, np.int64)
        want = np.ascontiguousarray(want, np.uint32)
        bad = C.c_int64(-1)
        self._ck(self.L.uz_crc32_blocks(self.h, data.ctypes.data, int(off.size) - 1, off.ctypes.data, want.ctypes.data, C.byref(bad)), "uz_crc32_blocks")
        return int(bad.value)

    def bam_walk_release(self, walk_id: int):
        self._ck(self.L.uz_bam_walk_release(self.h, int(walk_id)), "uz_bam_walk_release")

    def reads_from_bam(self, kb, names: bool = False) -> int:
        """The table of a batch walked on the device (kb: io_native.KeptBatch of select_kept(walk=self.bam_walk)): unpacked from the bytes in HBM.
        names: the read names of the kept records come back too (kb.qnames then maps the name ids of the result lists to strings)."""
        rid = C.c_int(-1)
        if getattr(kb, "joined", False):  # the joins ran on the device: the kept list lies in the batch's slot (uz_reads_from_walk)
            from . import io_native
            tot = np.zeros(8, np.int64)
            self._ck(self.L.uz_reads_from_walk(self.h, int(kb.token), int(kb.min_base_qual), 1 if names else 0, C.byref(rid), tot.ctypes.data), "uz_reads_from_walk")
            kb.token = None
            # a batch is through and its sizes are known: the other slots a pipeline will use grow to them now, not inside a later batch's walk
            # (a no-op once they have)
            with self._walked_lock:
                self._walked += 1
                walked = self._walked
            if walked in (1, 2, 4):
                self._ck(self.L.uz_walk_reserve(self.h, 4), "uz_walk_reserve")
            if names:
                kb.qnames = io_native.DeviceNames(self, rid.value, int(kb.n_qnames))
            return rid.value
        nb = int(kb.n_name_bytes) if names else 0
        alloc = getattr(kb, "_alloc", None)
        buf = (alloc(max(1, nb)) if alloc is not None else np.empty(max(1, nb), np.uint8)) if names else None
        self._ck(self.L.uz_reads_from_bam(self.h, int(kb.token), kb.kept.ctypes.data, int(kb.n), kb.aux.ctypes.data, int(kb.n_aux), kb.contig_off.ctypes.data,
                                          kb.max_span.ctypes.data, int(kb.n_contigs), int(kb.n_cigar_total), int(kb.n_row_units), int(kb.n_seq_units),
                                          int(kb.n_qnames), int(kb.min_base_qual), buf.ctypes.data if names else None, nb, C.byref(rid)), "uz_reads_from_bam")
        kb.token = None
        if names:
            kb.set_names(buf[:nb])
        return rid.value

    def adopt_sites(self, view: abi.SitesView) -> int:
        sid = C.c_int(-1)
        self._ck(self.L.uz_sites_adopt_device(self.h, C.byref(view), C.byref(sid)), "uz_sites_adopt_device")
        return sid.value

    def adopt_family(self, sites_h: int, view: abi.FamilyView) -> int:
        fid = C.c_int(-1)
        self._ck(self.L.uz_family_adopt_device(self.h, int(sites_h), C.byref(view), C.byref(fid)), "uz_family_adopt_device")
        return fid.value

    def adopt_reads(self, view: abi.ReadsPackedView) -> int:
        rid = C.c_int(-1)
        self._ck(self.L.uz_reads_adopt_device(self.h, C.byref(view), C.byref(rid)), "uz_reads_adopt_device")
        return rid.value

    def free_sites(self, sid: int):
        self._ck(self.L.uz_sites_free(self.h, int(sid)), "uz_sites_free")
        self._samples = {k: x for k, x in getattr(self, "_samples", {}).items() if x[0] != int(sid)}  # (its sample tables went with it)
        self._staged_sites.pop(int(sid), None)

    def free_reads(self, rid: int):
        self._ck(self.L.uz_reads_free(self.h, int(rid)), "uz_reads_free")
        self._staged.pop(int(rid), None)

    def drop_derived(self):
        self._ck(self.L.uz_drop_derived(self.h), "uz_drop_derived")

    def sync(self):
        self._ck(self.L.uz_sync(self.h), "uz_sync")

    # ----------------------------------------------------------- site stage
    def site_scan(self, fam: int):
        self._ck(self.L.uz_site_scan(self.h, int(fam)), "uz_site_scan")

    def site_scan_many(self, fams):
        """cohort form: all the families (of one sites table) in one launch"""
        ids = np.ascontiguousarray(np.asarray(list(fams), dtype=np.int32))
        self._ck(self.L.uz_site_scan_many(self.h, ids.ctypes.data, int(ids.size)), "uz_site_scan_many")

    def classify(self, fam: int, params: abi.Params, n_sites: int) -> np.ndarray:
        self.set_params(params)
        out = np.zeros(max(1, n_sites), dtype=np.uint8)
        self._ck(self.L.uz_site_classes(self.h, int(fam), out.ctypes.data), "uz_site_classes")
        return out[:n_sites]

    def find(self, fam: int, dv: abi.Held, params: abi.Params, mode: int, fetch: bool = True, transient: bool = False):
        """-> cand_off, cand_idx, cand_flags, het_off, het_idx.  transient: all five come back as views of ONE page-locked block this engine
        re-uses (three in turn: valid until the find after next), filled by uz_find_answer behind one wait of the host -- what a pipeline that
        reads them at once wants (pipeline.run_pipelined).  Without it: arrays of the caller's own (uz_find + uz_find_fetch)."""
        self.set_params(params)
        if transient and fetch:
            return self._find_answer(int(fam), dv, int(mode))
        return self._find_out(dv.view.n, fetch,
                              lambda co, ho: self._ck(self.L.uz_find(self.h, int(fam), dv.ref(), int(mode), co, ho), "uz_find"))

    @staticmethod
    def find_answer_layout(n: int, nc: int, nh: int):
        """(offsets of the six parts, total bytes) of a uz_find_answer block (unfazed_hip.h; csrc/find_answer.hpp)"""
        sizes = (64, 8 * (n + 1), 8 * (n + 1), 4 * nc, nc, 4 * nh)
        off, at = [], 0
        for b in sizes:
            off.append(at)
            at += (b + 255) & ~255
        return off, at

    def _find_answer(self, fam: int, dv: abi.Held, mode: int, block_bytes: Optional[int] = None):
        """find() through uz_find_answer: offsets and lists come back as views of ONE page-locked block (three in turn: the lists of a find are
        read before the find after next returns), written by one kernel behind the fill pass -- one wait of the host per find.  A block sized
        from the finds before (with head room) usually fits; one that does not is grown to what the call reports and the call made again.
        block_bytes: test hook, the size of the block handed to the first call."""
        n = dv.view.n
        if not hasattr(self, "_answer_pins"):
            self._answer_pins, self._answer_turn, self._answer_hint = [None, None, None], 0, 0
        self._answer_turn = (self._answer_turn + 1) % 3

        def block(need):
            pin = self._answer_pins[self._answer_turn]
            if pin is None or pin[1].size < need:
                if pin is not None:
                    pin[0].free_all()
                pool = PinnedPool()
                pin = self._answer_pins[self._answer_turn] = (pool, pool.alloc(need + need // 4 + (1 << 16)))
            return pin[1]

        out = np.zeros(4, dtype=np.int64)
        first = self.find_answer_layout(n, 0, 0)[1] if block_bytes is None else int(block_bytes)
        buf = block(max(first, self._answer_hint if block_bytes is None else 0, 256))
        size = buf.size if block_bytes is None else int(block_bytes)
        self._ck(self.L.uz_find_answer(self.h, fam, dv.ref(), mode, buf.ctypes.data, size, out.ctypes.data), "uz_find_answer")
        if out[0] != 0:  # the batch outgrew the lists' room or the block: once more, on a block of the size it needs
            buf = block(int(out[1]))
            self._ck(self.L.uz_find_answer(self.h, fam, dv.ref(), mode, buf.ctypes.data, buf.size, out.ctypes.data), "uz_find_answer")
            if out[0] != 0:
                raise UnfazedHipError("uz_find_answer: no answer on a block of the size it asked for (%d bytes, code %d)" % (int(out[1]), int(out[0])))
        self._answer_hint = max(self._answer_hint, int(out[1]) + int(out[1]) // 4)
        nc, nh = int(out[2]), int(out[3])
        off, _ = self.find_answer_layout(n, nc, nh)
        co = buf[off[1]: off[1] + 8 * (n + 1)].view(np.int64)
        ho = buf[off[2]: off[2] + 8 * (n + 1)].view(np.int64)
        return co, buf[off[3]: off[3] + 4 * nc].view(np.int32), buf[off[4]: off[4] + nc], ho, buf[off[5]: off[5] + 4 * nh].view(np.int32)

    def find_stats(self):
        """(host waits, kernel launches, fall-back bits, bytes of the answer) of the last find of this engine (uz_find_stats)"""
        out = np.zeros(4, dtype=np.int64)
        self._ck(self.L.uz_find_stats(self.h, out.ctypes.data), "uz_find_stats")
        return tuple(int(x) for x in out)

    def _find_out(self, n, fetch, run):
        """The outputs of a find over n DNMs: run(cand_off, het_off) makes the call on the two offset arrays' addresses; the index lists behind
        them are fetched when asked for."""
        co = np.zeros(n + 1, dtype=np.int64)
        ho = np.zeros(n + 1, dtype=np.int64)
        run(co.ctypes.data, ho.ctypes.data)
        if not fetch:
            return co, None, None, ho, None
        ci, cf, hi = self._fetch(int(co[n]), int(ho[n]))
        return co, ci, cf, ho, hi

    @staticmethod
    def _groups(groups):
        """[(fam, first, count)] or [(fam, reads_h, first, count, cutoff)] -> uz_cohort_group array.  The short form is the find side's, whose
        calls read neither the reads handle nor the cutoff: -1 and 0.0."""
        arr = (abi.CohortGroup * max(1, len(groups)))()
        for k, g in enumerate(groups):
            fam, rh, first, count, cutoff = g if len(g) == 5 else (g[0], -1, g[1], g[2], 0.0)
            arr[k].fam_id, arr[k].reads_id, arr[k].dnm_first, arr[k].dnm_count, arr[k].cutoff = int(fam), int(rh), int(first), int(count), float(cutoff)
        return arr

    def find_cohort(self, groups, dv: abi.Held, params: abi.Params, mode: int, fetch: bool = True):
        """Cohort form of find(): groups = [(fam, first, count)] covering the DNMs of `dv` exactly once (several kids, each with its own
        family columns), one launch sequence (uz_find_cohort).  Same result layout as find(), in DNM order."""
        self.set_params(params)
        arr = self._groups(groups)
        return self._find_out(dv.view.n, fetch,
                              lambda co, ho: self._ck(self.L.uz_find_cohort(self.h, arr, len(groups), dv.ref(), int(mode), co, ho), "uz_find_cohort"))

    def _fetch(self, nc: int, nh: int):
        ci = np.zeros(max(1, nc), dtype=np.int32)
        cf = np.zeros(max(1, nc), dtype=np.uint8)
        hi = np.zeros(max(1, nh), dtype=np.int32)
        self._ck(self.L.uz_find_fetch(self.h, ci.ctypes.data, cf.ctypes.data, hi.ctypes.data), "uz_find_fetch")
        return ci[:nc], cf[:nc], hi[:nh]

    # ----------------------------------------------------------- read stage
    def _phase_out(self, n, run):
        """The results of a read stage over n DNMs: run(status, counts, origin, evidence) makes the call on the four arrays' addresses."""
        status = np.empty(max(1, n), dtype=np.int32)  # (the call writes all n entries of each, or raises)
        counts = np.empty(max(1, 4 * n), dtype=np.int32)
        origin = np.empty(max(1, n), dtype=np.int32)
        evidence = np.empty(max(1, n), dtype=np.int32)
        run(status.ctypes.data, counts.ctypes.data, origin.ctypes.data, evidence.ctypes.data)
        return dict(status=status[:n], counts=counts[: 4 * n].reshape(n, 4), origin=origin[:n], evidence=evidence[:n])

    def _with_lists(self, r, n, want_lists):
        """the vote lists of the read stage that made `r`, four per DNM -- or None -- as r["lists"]"""
        r["lists"] = None
        if want_lists:
            vo, vv = self.votes(n)
            r["lists"] = [tuple(vv[vo[4 * k + j]: vo[4 * k + j + 1]] for j in range(4)) for k in range(n)]
        return r

    def phase_raw(self, fam: int, reads_h: int, dv: abi.Held, params: abi.Params, find_mode: int):
        self.set_params(params)
        return self._phase_out(dv.view.n, lambda *out: self._ck(self.L.uz_phase(self.h, int(fam), int(reads_h), dv.ref(), int(find_mode), *out), "uz_phase"))

    def phase_begin(self, fam: int, reads_h: int, dv: abi.Held, params: abi.Params, find_mode: int):
        """first half of phase_raw (uz_phase_begin): queues the batch and returns; phase_end -- same arguments -- hands out the results.
        Uploads and find() of OTHER batches may run in between: they queue up behind this batch's kernels."""
        self.set_params(params)
        self._ck(self.L.uz_phase_begin(self.h, int(fam), int(reads_h), dv.ref(), int(find_mode)), "uz_phase_begin")

    def phase_end(self, fam: int, reads_h: int, dv: abi.Held, params: abi.Params, find_mode: int):
        return self._phase_out(dv.view.n, lambda *out: self._ck(self.L.uz_phase_end(self.h, int(fam), int(reads_h), dv.ref(), int(find_mode), *out), "uz_phase_end"))

    def phase_cohort(self, groups, dv: abi.Held, params: abi.Params, found_list=None, want_lists: bool = True,
                     find_mode: int = abi.FIND_SECOND_WINDOW, joined=None):
        """Cohort form of phase(): groups = [(fam, reads_h, first, count, cutoff)] over the DNMs of `dv` (several kids, each
        with its own family columns / alignment records / insert cutoff), one launch sequence.  Same result layout as
        phase(); the query-name ids of the lists are those of each group's own table."""
        self.set_params(params)
        n = dv.view.n
        arr = self._groups(groups)
        if joined is None:
            r = self._phase_out(n, lambda *out: self._ck(self.L.uz_phase_cohort(self.h, arr, len(groups), dv.ref(), int(find_mode), *out), "uz_phase_cohort"))
        else:  # ONE table over the groups' files (uz_phase_cohort_joined): the lists carry that table's name ids
            rid, base = joined
            base = np.ascontiguousarray(base, np.int32)
            assert base.size == len(groups)
            r = self._phase_out(n, lambda *out: self._ck(self.L.uz_phase_cohort_joined(self.h, int(rid), arr, len(groups), base.ctypes.data, dv.ref(),
                                                                                       int(find_mode), *out), "uz_phase_cohort_joined"))
        return self._with_lists(r, n, want_lists)

    def phase_cohort_joined(self, rid: int, groups, group_ref_base, dv: abi.Held, params: abi.Params, found_list=None, want_lists: bool = True,
                            find_mode: int = abi.FIND_SECOND_WINDOW):
        """phase_cohort on ONE reads table built over the groups' alignment files presented as one (io_native.BamSource.open_many): no table is
        concatenated.  groups as phase_cohort's (their reads handle is not looked at); group_ref_base[g]: the first contig of group g's file in the
        table.  The query-name ids of the lists are the table's own."""
        return self.phase_cohort(groups, dv, params, found_list, want_lists, find_mode, joined=(rid, group_ref_base))

    def votes(self, n: int):
        vo = np.zeros(4 * n + 1, dtype=np.int64)
        self._ck(self.L.uz_phase_votes(self.h, vo.ctypes.data, None), "uz_phase_votes")
        vv = np.zeros(max(1, int(vo[-1])), dtype=np.int32)
        self._ck(self.L.uz_phase_votes(self.h, vo.ctypes.data, vv.ctypes.data), "uz_phase_votes")
        return vo, vv[: int(vo[-1])]

    def groups(self, n: int):
        go = np.zeros(2 * n + 1, dtype=np.int64)
        self._ck(self.L.uz_phase_groups(self.h, go.ctypes.data, None), "uz_phase_groups")
        gq = np.zeros(max(1, int(go[-1])), dtype=np.int32)
        self._ck(self.L.uz_phase_groups(self.h, go.ctypes.data, gq.ctypes.data), "uz_phase_groups")
        return go, gq[: int(go[-1])]

    def _bed_text(self, n: int, off, ptr):
        total = int(off[n])
        return (C.string_at(ptr.value, total) if total else b""), off  # (a copy: the context's block is the next call's)

    def bed_rows(self, rows, str_off, str_bytes, verbose: bool, include_ambiguous: bool):
        """The BED lines of rows of the LAST finished batch (uz_bed_rows), written on the device from the batch's result where it lies.
        rows: abi.BED_ROW records; -> (bytes, off [n + 1]): row k is bytes[off[k]: off[k + 1]], empty when the row is dropped."""
        v = abi.bed_view(rows, str_off, str_bytes)
        n = int(v.view.n_rows)
        off, ptr = np.zeros(n + 1, np.int64), C.c_void_p()
        self._ck(self.L.uz_bed_rows(self.h, v.ref(), int(bool(verbose)), int(bool(include_ambiguous)), off.ctypes.data, C.byref(ptr)), "uz_bed_rows")
        return self._bed_text(n, off, ptr)

    def bed_rows_lists(self, rows, str_off, str_bytes, verbose: bool, include_ambiguous: bool, status, list_off, list_val, name_off, name_bytes, ratio: int):
        """Test hook (uz_bed_rows_lists): the same kernels over the caller's lists -- uz_phase_votes' layout -- and a plain name store
        (name_off None: no names); no read stage is run."""
        v = abi.bed_view(rows, str_off, str_bytes)
        n = int(v.view.n_rows)
        status = np.ascontiguousarray(status, np.int32)
        list_off = np.ascontiguousarray(list_off, np.int64)
        list_val = np.ascontiguousarray(list_val, np.int32)
        off, ptr = np.zeros(n + 1, np.int64), C.c_void_p()
        if name_off is not None:
            name_off, name_bytes = np.ascontiguousarray(name_off, np.uint32), np.ascontiguousarray(name_bytes, np.uint8)
            nq, p_no, p_nb = int(name_off.size) - 1, name_off.ctypes.data, name_bytes.ctypes.data if name_bytes.size else None
        else:
            nq, p_no, p_nb = 0, None, None
        self._ck(self.L.uz_bed_rows_lists(self.h, v.ref(), int(bool(verbose)), int(bool(include_ambiguous)), int(status.size), status.ctypes.data,
                                          list_off.ctypes.data, list_val.ctypes.data if list_val.size else None, nq, p_no, p_nb, int(ratio),
                                          off.ctypes.data, C.byref(ptr)), "uz_bed_rows_lists")
        return self._bed_text(n, off, ptr)

    def vcf_rows(self, text: "abi.VcfTextView", line_at, ann_off, ann_col, ann_gt, ann_uops, ann_uet):
        """The record lines of the annotated VCF (uz_vcf_rows), rewritten on the device from the DNM file's text.  text: io_native.vcf_samples_text's
        view; line_at [n]: every record's line start; the annotations as a sparse table over the records (ann_off [n + 1]; column, gt code 0 / 1 / 2,
        uops, uet).  -> (bytes, off [n + 1], handed_back bool [n]): record k is bytes[off[k]: off[k + 1]], empty when the record is handed back."""
        n = int(text.n_records)
        line_at, ann_off = np.ascontiguousarray(line_at, np.int64), np.ascontiguousarray(ann_off, np.int64)
        ann_col, ann_uops = np.ascontiguousarray(ann_col, np.int32), np.ascontiguousarray(ann_uops, np.int32)
        ann_gt, ann_uet = np.ascontiguousarray(ann_gt, np.uint8), np.ascontiguousarray(ann_uet, np.int8)
        if line_at.size != n or ann_off.size != n + 1 or not (ann_col.size == ann_gt.size == ann_uops.size == ann_uet.size):
            raise UnfazedHipError("vcf_rows: the arrays do not fit the records")
        ptr_or_none = lambda a: a.ctypes.data if a.size else None
        off, hb, ptr = np.zeros(n + 1, np.int64), np.zeros(max(1, n), np.uint8), C.c_void_p()
        self._ck(self.L.uz_vcf_rows(self.h, C.addressof(text), line_at.ctypes.data if n else None, ann_off.ctypes.data, ptr_or_none(ann_col), ptr_or_none(ann_gt),
                                    ptr_or_none(ann_uops), ptr_or_none(ann_uet), off.ctypes.data, C.byref(ptr), hb.ctypes.data), "uz_vcf_rows")
        total = int(off[n])
        return (C.string_at(ptr.value, total) if total else b""), off, hb[:n].astype(bool)  # (a copy: the context's block is the next call's)

    def bcf_rows(self, view: "abi.BcfLinesView"):
        """The records of a BCF as VCF text lines (uz_bcf_rows), written on the device.  view: io_native.vcf_bcf_lines's, or abi.bcf_lines_view over
        the caller's arrays.  -> (bytes, off [n + 1], samp_at uint64 [n], handed_back bool [n]): record k's line, its '\n' included, is
        bytes[off[k]: off[k + 1]], empty when the record is handed back; samp_at[k]: where its column 10 starts in bytes (its '\n' without one)."""
        n = int(view.n_records)
        off, samp_at, hb, ptr = np.zeros(n + 1, np.int64), np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint8), C.c_void_p()
        self._ck(self.L.uz_bcf_rows(self.h, C.addressof(view), off.ctypes.data, samp_at.ctypes.data, C.byref(ptr), hb.ctypes.data), "uz_bcf_rows")
        total = int(off[n])
        return (C.string_at(ptr.value, total) if total else b""), off, samp_at[:n], hb[:n].astype(bool)  # (a copy: the context's block is the next call's)

    def phase_sizing(self, n: int, n_het: int) -> dict:
        """Test hook (uz_phase_sizing_fetch): the sizing pass's output for the last phase_raw / phase_end -- n DNMs, n_het = het_off[n] of the
        batch's window lists.  -> bounds [n, 5], pre_win [n, 4], pre_ha [n_het], pre_hl [n_het] and the batch's reduction: mA, mT, mH, mC,
        active, mM, sumP as ints, hist int64 [256]."""
        n, n_het = int(n), int(n_het)
        bounds = np.zeros(max(1, 5 * n), np.int32)
        pre_win = np.zeros(max(1, 4 * n), np.int32)
        pre_ha = np.zeros(max(1, n_het), np.int32)
        pre_hl = np.zeros(max(1, n_het), np.int32)
        red = np.zeros(SIZING_REDUCED_WORDS, np.int64)
        self._ck(self.L.uz_phase_sizing_fetch(self.h, bounds.ctypes.data, pre_win.ctypes.data, pre_ha.ctypes.data, pre_hl.ctypes.data,
                                              red.ctypes.data), "uz_phase_sizing_fetch")
        out = dict(bounds=bounds[: 5 * n].reshape(n, 5), pre_win=pre_win[: 4 * n].reshape(n, 4), pre_ha=pre_ha[:n_het], pre_hl=pre_hl[:n_het])
        out.update({k: int(red[j]) for j, k in enumerate(("mA", "mT", "mH", "mC", "active", "mM", "sumP"))})
        out["hist"] = red[7:].copy()
        return out

    def phase(self, fam: int, reads_h: int, dv: abi.Held, params: abi.Params, found_list, want_lists: bool = True,
              find_mode: int = abi.FIND_SECOND_WINDOW):
        """Backend entry used by PhasingHost.run_read_phasing (found_list is ignored:
        the window lists are recomputed on the device for the batch)."""
        return self._with_lists(self.phase_raw(fam, reads_h, dv, params, find_mode), dv.view.n, want_lists)

    # ------------------------------------------------------------ CNV stage
    def phase_cnv(self, fam: int, dv: abi.Held, params: abi.Params, rb_counts=None, want_lists: bool = True):
        """K6: allele-balance phasing of the DEL / DUP of the batch + summarize_record's decision (merged with the
        read-backed counts when given).  -> dict(cnv_counts [n,2], origin, evidence, etype[, lists: (dad, mom) positions])"""
        self.set_params(params)
        return self._cnv_out(dv.view.n, rb_counts, want_lists, lambda *io: self._ck(self.L.uz_phase_cnv(self.h, int(fam), dv.ref(), *io), "uz_phase_cnv"))

    def phase_cnv_cohort(self, groups, dv: abi.Held, params: abi.Params, rb_counts=None, want_lists: bool = True):
        """Cohort form of phase_cnv(): groups = [(fam, first, count)] covering the DNMs of `dv` exactly once, one whole-region find with a
        family per DNM and one K6 launch (uz_phase_cnv_cohort).  Same result layout as phase_cnv(), in DNM order."""
        self.set_params(params)
        arr = self._groups(groups)
        return self._cnv_out(dv.view.n, rb_counts, want_lists,
                             lambda *io: self._ck(self.L.uz_phase_cnv_cohort(self.h, arr, len(groups), dv.ref(), *io), "uz_phase_cnv_cohort"))

    def _cnv_out(self, n, rb_counts, want_lists, run):
        """The outputs of an allele-balance stage over n DNMs: run(rb_counts or None, cnv_counts, origin, evidence, etype) makes the call on the
        arrays' addresses; the site lists behind the counts are fetched when asked for."""
        cnt = np.zeros(max(1, 2 * n), np.int32)
        origin = np.zeros(max(1, n), np.int32)
        evidence = np.zeros(max(1, n), np.int32)
        etype = np.zeros(max(1, n), np.int32)
        rb = None
        if rb_counts is not None:
            rb = np.ascontiguousarray(rb_counts, np.int32).reshape(-1)
            assert rb.size == 4 * n
        run(rb.ctypes.data if rb is not None else None, cnt.ctypes.data, origin.ctypes.data, evidence.ctypes.data, etype.ctypes.data)
        r = dict(cnv_counts=cnt[: 2 * n].reshape(n, 2), origin=origin[:n], evidence=evidence[:n], etype=etype[:n], lists=None)
        if want_lists:
            off = np.zeros(2 * n + 1, np.int64)
            self._ck(self.L.uz_phase_cnv_sites(self.h, off.ctypes.data, None), "uz_phase_cnv_sites")
            pos = np.zeros(max(1, int(off[-1])), np.int32)
            self._ck(self.L.uz_phase_cnv_sites(self.h, off.ctypes.data, pos.ctypes.data), "uz_phase_cnv_sites")
            r["lists"] = [(pos[off[2 * k]: off[2 * k + 1]], pos[off[2 * k + 1]: off[2 * k + 2]]) for k in range(n)]
        return r

    # ---------------------------------------------------------- the heads of a cohort's alignment files (read_collector.py:11-25)
    def head_walk(self, head: int, comp: np.ndarray, comp_bytes: int, in_off, isize, crc, blk_first, start, want, have):
        """uz_head_walk: one round over the blocks given (head = -1 opens a head) -> (head id, taken, cursor, state) per file"""
        i64 = lambda a: np.ascontiguousarray(a, np.int64)
        in_off, blk_first, start, want, have = i64(in_off), i64(blk_first), i64(start), i64(want), i64(have)
        isize, crc = np.ascontiguousarray(isize, np.int32), np.ascontiguousarray(crc, np.uint32)
        nf = int(want.size)
        taken, cursor, state = np.zeros(nf, np.int64), np.zeros(nf, np.int64), np.zeros(nf, np.int32)
        hid = C.c_int(int(head))
        self._ck(self.L.uz_head_walk(self.h, C.byref(hid), nf, comp.ctypes.data, int(comp_bytes), int(in_off.size), in_off.ctypes.data, isize.ctypes.data,
                                     crc.ctypes.data, blk_first.ctypes.data, start.ctypes.data, want.ctypes.data, have.ctypes.data, taken.ctypes.data,
                                     cursor.ctypes.data, state.ctypes.data), "uz_head_walk")
        return int(hid.value), taken, cursor, state

    def head_rank(self, head: int, readlen: int, k):
        """uz_head_rank: per file the keys |tlen - 2 readlen| at ranks k[f] and min(k[f] + 1, n - 1); k[f] < 0 skips the file -> (a, b) uint32"""
        k = np.ascontiguousarray(k, np.int64)
        a, b = np.zeros(k.size, np.uint32), np.zeros(k.size, np.uint32)
        self._ck(self.L.uz_head_rank(self.h, int(head), int(readlen), k.ctypes.data, a.ctypes.data, b.ctypes.data), "uz_head_rank")
        return a, b

    def head_fetch(self, head: int, file: int, cap: int) -> np.ndarray:
        out = np.zeros(max(1, int(cap)), np.int32)
        n = C.c_int64(0)
        self._ck(self.L.uz_head_fetch(self.h, int(head), int(file), out.ctypes.data, int(cap), C.byref(n)), "uz_head_fetch")
        return out[: int(n.value)].copy()

    def head_free(self, head: int):
        self._ck(self.L.uz_head_free(self.h, int(head)), "uz_head_free")

    def _head_pinned(self, nbytes: int) -> np.ndarray:
        """page-locked memory for the gathered heads of a group, kept and grown from call to call"""
        pin = getattr(self, "_head_pin", None)
        if pin is None or pin[1].size < nbytes:
            if pin is not None:
                pin[0].free_all()
            pool = PinnedPool()
            self._head_pin = pin = (pool, pool.alloc(int(nbytes) + int(nbytes) // 4 + (1 << 20)))
        return pin[1]

    @staticmethod
    def _head_first_estimate(src, coff: int, start: int, want: int) -> int:
        """Round 1's byte estimate of one file: the host inflates the file's first data block itself, takes the mean record size there and asks
        for `want` times that plus a margin (UZ_HEAD_FIRST_BYTES overrides it).  A block that holds no whole record: 512 bytes a record."""
        env = os.environ.get("UZ_HEAD_FIRST_BYTES")
        if env:
            return max(1, int(env))
        import zlib
        b = src.list_blocks(coff, 1, cap=1)
        mean = 512.0
        if b["off"].size:
            with open(src.path, "rb") as fh:
                fh.seek(int(b["data"][0]))
                raw = fh.read(int(b["off"][0]) + int(b["csize"][0]) - 8 - int(b["data"][0]))
            data = zlib.decompressobj(-15).decompress(raw)
            c, n = int(start), 0
            while c + 4 <= len(data):
                bs = int.from_bytes(data[c: c + 4], "little", signed=True)
                if bs < 32 or c + 4 + bs > len(data):
                    break
                c, n = c + 4 + bs, n + 1
            if n:
                mean = (c - int(start)) / n
        return int(want * mean) + int(want * mean) // 16 + (1 << 17)

    def head_ranks(self, files, want: int, readlen: int, stats=None, fetch: bool = False):
        """The two order statistics behind the insert cutoff of every file (read_collector.py:11-25), from the first `want` records of each:
        -> per file (n, a, b) -- n records read (the whole file when it holds fewer), a / b the keys |tlen - 2 readlen| at ranks
        floor((n - 1) 0.995) and the next (hostpath.cutoff_from_ranks makes the cutoff of them) -- or None: the file is handed back to the
        host route (a record or a block the device refuses, a file the lister refuses, no record at all, more than HEAD_MAX_ROUNDS walks).
        files: paths of indexed BAMs, or io_native.BamSource objects (opened without a head).  Rounds: every file asks for an estimate of the
        bytes its `want` records take; a file whose bytes ended before its count goes on in the next round from where the cursor fell.
        Groups: one uz_head_walk holds at most UZ_HEAD_MAX_BYTES inflated bytes (a larger file is a group of its own, cut by rounds).
        stats: a dict whose "cutoff_walk_calls" counts the walks.  fetch: -> (the list, the tlen column of every file or None)."""
        import zlib
        from .hostpath import head_rank_index
        from .io_native import BamSource, IoError
        nf = len(files)
        out = [None] * nf
        cols = [None] * nf
        want = int(want)
        if nf == 0 or want <= 0 or want > 0x7FFFFFFF or not (0 <= int(readlen) < (1 << 30)):
            return (out, cols) if fetch else out
        max_bytes = max(1, int(os.environ.get("UZ_HEAD_MAX_BYTES", HEAD_MAX_BYTES)))
        srcs, st = [None] * nf, [None] * nf  # st: per file [coff, start, est bytes, rounds] while it is walked
        for f, x in enumerate(files):
            try:
                srcs[f] = x if isinstance(x, BamSource) else BamSource(x, insert_size_max_sample=-1)
                v = int(srcs[f].first_voff[0])
                st[f] = [v >> 16, v & 0xFFFF, self._head_first_estimate(srcs[f], v >> 16, v & 0xFFFF, want), 0]
            except (IoError, OSError, zlib.error):
                st[f] = None  # the host route answers or raises for it
        wants = np.full(nf, want, np.int64)
        have = np.zeros(nf, np.int64)
        finished = np.zeros(nf, bool)
        head = -1
        try:
            while any(s is not None for s in st):
                # this round's blocks, file by file
                listed = {}
                for f in range(nf):
                    if st[f] is None:
                        continue
                    try:
                        listed[f] = srcs[f].list_blocks(st[f][0], min(st[f][2], max_bytes))
                    except IoError:
                        st[f] = None
                groups, cur, cur_bytes = [], [], 0
                for f, b in listed.items():
                    nb = int(b["isize"].sum())
                    if cur and cur_bytes + nb > max_bytes:
                        groups.append(cur)
                        cur, cur_bytes = [], 0
                    cur.append(f)
                    cur_bytes += nb
                if cur:
                    groups.append(cur)
                for grp in groups:
                    src_off = [int(listed[f]["off"][0]) if listed[f]["off"].size else 0 for f in grp]
                    nbytes = [int(listed[f]["off"][-1] + listed[f]["csize"][-1]) - so if listed[f]["off"].size else 0 for f, so in zip(grp, src_off)]
                    dst_off = np.concatenate([[0], np.cumsum(nbytes)]).astype(np.int64)
                    comp = self._head_pinned(int(dst_off[-1]) + 64)
                    BamSource.gather_ranges([srcs[f] for f in grp], src_off, nbytes, dst_off[:-1], comp)
                    blk_first = np.zeros(nf + 1, np.int64)
                    start = np.zeros(nf, np.int64)
                    for f in grp:
                        blk_first[f + 1] = listed[f]["off"].size
                        start[f] = st[f][1]
                    blk_first = np.cumsum(blk_first)
                    in_off = np.concatenate([listed[f]["data"] - so + d for f, so, d in zip(grp, src_off, dst_off[:-1])] + [np.zeros(0, np.int64)])
                    isize = np.concatenate([listed[f]["isize"] for f in grp] + [np.zeros(0, np.int32)])
                    crc = np.concatenate([listed[f]["crc"] for f in grp] + [np.zeros(0, np.uint32)])
                    head, taken, cursor, state = self.head_walk(head, comp, int(dst_off[-1]), in_off, isize, crc, blk_first, start, wants, have)
                    if stats is not None:
                        stats["cutoff_walk_calls"] = (stats["cutoff_walk_calls"] if "cutoff_walk_calls" in stats else 0) + 1
                    have += taken
                    for f in grp:
                        b, s = listed[f], st[f]
                        cum = np.cumsum(b["isize"].astype(np.int64))
                        total = int(cum[-1]) if cum.size else 0
                        cu = int(cursor[f])
                        if state[f] == HEAD_DONE:
                            finished[f], st[f] = True, None
                        elif state[f] == HEAD_END and b["at_end"]:
                            finished[f], st[f] = cu == total, None  # (a record cut off by the file's end: the host route raises for it)
                        elif state[f] == HEAD_END and s[3] + 1 < HEAD_MAX_ROUNDS:
                            if cu >= total:
                                s[0], s[1] = int(b["off"][-1]) + int(b["csize"][-1]), 0
                            else:
                                k = int(np.searchsorted(cum, cu, side="right"))
                                s[0], s[1] = int(b["off"][k]), cu - (int(cum[k - 1]) if k else 0)
                            left = want - int(have[f])
                            used = cu - int(start[f])
                            s[2] = (int(left * used / int(taken[f])) * 17 // 16 + (1 << 17)) if taken[f] > 0 else 2 * max(s[2], total)
                            s[3] += 1
                        else:
                            st[f] = None  # HEAD_BAD, no block listed, or too many rounds: handed back
            if head >= 0:
                ks = np.array([head_rank_index(int(have[f])) if finished[f] and have[f] > 0 else -1 for f in range(nf)], np.int64)
                if (ks >= 0).any():
                    a, b = self.head_rank(head, int(readlen), ks)
                    for f in range(nf):
                        if ks[f] >= 0:
                            out[f] = (int(have[f]), int(a[f]), int(b[f]))
                            if fetch:
                                cols[f] = self.head_fetch(head, f, int(have[f]))
        finally:
            if head >= 0:
                self.head_free(head)
        return (out, cols) if fetch else out

    # ---------------------------------------------------------- measurement
    def prof_enable(self, on=True):
        """on: False / True, or the kernel ids (abi.K_*) to time -- an empty list is False"""
        v = (1 if on else 0) if isinstance(on, (bool, int)) else sum(1 << (int(k) + 1) for k in set(on))
        self._ck(self.L.uz_prof_enable(self.h, int(v)), "uz_prof_enable")

    def prof_reset(self):
        self._ck(self.L.uz_prof_reset(self.h), "uz_prof_reset")

    def prof_get(self, kernel: int):
        ms = C.c_double(0)
        n = C.c_int64(0)
        self._ck(self.L.uz_prof_get(self.h, int(kernel), C.byref(ms), C.byref(n)), "uz_prof_get")
        return ms.value, n.value

    def prof_units(self, kernel: int) -> int:
        u = C.c_int64(0)
        self._ck(self.L.uz_prof_units(self.h, int(kernel), C.byref(u)), "uz_prof_units")
        return int(u.value)


class PinnedPair:
    """The two page-locked buffers a staged batch needs when the device inflates its blocks (gathered bytes, inflated bytes), kept and
    grown from batch to batch: `alloc` is BamSource.select's inflate_alloc (called twice per batch, after start())."""

    def __init__(self):
        self.pool = PinnedPool()
        self.bufs = []
        self.k = 0

    def start(self):
        self.k = 0

    def alloc(self, nbytes: int) -> np.ndarray:
        i, self.k = self.k, self.k + 1
        while len(self.bufs) <= i:
            self.bufs.append(None)
        if self.bufs[i] is None or self.bufs[i].size < nbytes:
            self.bufs[i] = self.pool.alloc(int(nbytes) + int(nbytes) // 4 + (1 << 20))  # (the block it outgrew stays until free_all)
        return self.bufs[i][: max(64, int(nbytes))]

    def free_all(self):
        self.bufs = []
        self.pool.free_all()


class PinnedPool:
    """Page-locked host memory for the staged columns (uz_pinned_alloc), handed out as numpy uint8 arrays.
    alloc() is the `alloc` callback of abi.packed_view_alloc / io_native.pack_reads / ReadsSource.select."""

    def __init__(self):
        self.L = load_library()
        self._blocks = []
        self._slab = None  # [base address, capacity, used]: alloc() carves from it while it lasts
        self._ended = None  # the slab end_slab() closed (rewind() takes it up again)
        self.keep = False   # kept from batch to batch by its owner (io_native.BamSource.select rewinds it instead of pinning a new block)
        self.last_slab_used = 0

    def new_slab(self, nbytes: int):
        """The allocations that follow come back to back (256-byte aligned) out of ONE page-locked block of `nbytes`: the
        columns of a table staged this way cross the link as one copy (uz_stage.hpp: SlabPlan).  What does not fit any more gets
        a block of its own, as without a slab."""
        nbytes = max(1 << 20, int(nbytes))
        p = C.c_void_p()
        if self.L.uz_pinned_alloc(nbytes, C.byref(p)) != 0 or not p.value:
            raise MemoryError("uz_pinned_alloc(%d) failed" % nbytes)
        self._blocks.append(p.value)
        self.last_slab_used = self._slab[2] if self._slab else 0
        self._slab = [p.value, nbytes, 0]

    def rewind(self, nbytes: int) -> bool:
        """Start over in the current slab when it holds at least `nbytes` (a staging loop re-uses its page-locked block chunk after
        chunk instead of pinning a new one); the overflow blocks of the last use are freed.  False: no slab of that size."""
        if self._slab is None and getattr(self, "_ended", None) is not None:
            self._slab = self._ended  # (end_slab() closed it: the block is still there)
        if self._slab is None or self._slab[1] < int(nbytes):
            return False
        keep = self._slab[0]
        for p in self._blocks:
            if p != keep:
                self.L.uz_pinned_free(C.c_void_p(p))
        self._blocks = [keep]
        self._slab[2] = 0
        return True

    def slab_used(self) -> int:
        return self._slab[2] if self._slab else 0

    def end_slab(self) -> int:
        used = self._slab[2] if self._slab else 0
        self._ended = self._slab
        self._slab = None
        return used

    def alloc(self, nbytes: int) -> np.ndarray:
        nbytes = max(64, int(nbytes))
        if self._slab is not None:
            at = (self._slab[2] + 255) & ~255
            if at + nbytes <= self._slab[1]:
                self._slab[2] = at + nbytes
                buf = (C.c_uint8 * nbytes).from_address(self._slab[0] + at)
                return np.frombuffer(buf, dtype=np.uint8, count=nbytes)
        p = C.c_void_p()
        if self.L.uz_pinned_alloc(nbytes, C.byref(p)) != 0 or not p.value:
            raise MemoryError("uz_pinned_alloc(%d) failed" % nbytes)
        self._blocks.append(p.value)
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype=np.uint8, count=nbytes)

    def free_all(self):
        for p in self._blocks:
            self.L.uz_pinned_free(C.c_void_p(p))
        self._blocks = []
        self._slab = None
        self._ended = None
