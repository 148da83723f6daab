"""The one place the driver writes its output file: write_output(outfile, parts), called from every writer of unfazed.py and summarize.py.

UZ_OUT_BGZF decides what an outfile whose name ends in ".gz" holds:
  not set, or any other value   plain text, whatever the file is called (as before)
  "host"    BGZF: one block per 65 280 bytes (htslib's slice), zlib's raw DEFLATE at UZ_OUT_BGZF_LEVEL (6), the 28-byte end-of-file marker
  "device"  the same blocks from backend.bgzf_deflate (uz_bgzf_deflate; csrc/deflate_body.hpp states its rules).  Asked for by name, the
            route makes its backend and fails loudly without a device, as UZ_BCF_ROUTE=device does.  UZ_OUT_BGZF_CODE=dynamic (read on this
            route alone; any case) asks for the dynamic coder (csrc/deflate_dyn.hpp): per block the shortest of a dynamic-Huffman, the fixed and
            a stored block; not set, or any other value: the fixed code, as before
UZ_OUT_INDEX=tbi (any case; read only where the outfile is written as BGZF) writes the file's tabix index to outfile + ".tbi", itself BGZF by the
same route, end-of-file marker included.  The preset comes from the text (tabix_index.preset_of: "##fileformat=VCF" at byte 0, or BED).  "device":
the tables come out of the deflate call (uz_bgzf_deflate_indexed: csrc/k_tbx.hip); "host": tabix_index.build_host.  A text that cannot be
indexed (tabix_index.py lists the reasons: the annotated VCF keeps the DNM file's order, which nobody sorted for us) gets no index and loses
the one an earlier run left; the data file is written as ever, one line on stderr names the reason, nothing is raised.  Not set, or any other
value: no index file, as before.
An outfile without ".gz", and /dev/stdout, stay plain on every setting.  The two routes' files differ in their compressed bytes (the
compressors differ) and in nothing else: the inflated text, every ISIZE, every CRC-32 and the end-of-file marker are the same."""
import os
import struct
import sys
import zlib

SLICE = 0xFF00  # bytes of text per BGZF block: htslib's BGZF_BLOCK_SIZE
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# Blocks the device / zlib wrote, files written as BGZF.  The first outfile written under UZ_OUT_INDEX adds three counters (a run without the
# switch has the keys it always had): "index_files" index files written, "index_refused" texts that got none, "index_host_rows" rows the
# host settled on the device route
OUT_STATS = {"bgzf_device_blocks": 0, "bgzf_host_blocks": 0, "bgzf_calls": 0}
INDEX_KEYS = ("index_files", "index_refused", "index_host_rows")
OUT_KINDS = {"stored": 0, "fixed": 0, "dynamic": 0}  # the device's blocks by their form


def out_route():
    """UZ_OUT_BGZF: "device", "host", or None (not set, or any other value: every outfile is plain text)"""
    v = os.environ.get("UZ_OUT_BGZF", "").lower()
    return v if v in ("device", "host") else None


def out_code():
    """UZ_OUT_BGZF_CODE on the device route: "dynamic", or "fixed" (not set, or any other value)"""
    return "dynamic" if os.environ.get("UZ_OUT_BGZF_CODE", "").lower() == "dynamic" else "fixed"


def out_index():
    """UZ_OUT_INDEX: "tbi", or None (not set, or any other value: no index file)"""
    return "tbi" if os.environ.get("UZ_OUT_INDEX", "").lower() == "tbi" else None


def bgzf_block(stream: bytes, payload) -> bytes:
    """one BGZF block around a raw DEFLATE stream of `payload`"""
    size = 18 + len(stream) + 8
    if size > 65536:
        raise ValueError("a BGZF block of %d bytes" % size)
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", size - 1) + stream
            + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def host_blocks(data, level=None):
    """`data` as BGZF blocks by zlib, one per SLICE bytes, without the end-of-file marker -> (bytes, block count)"""
    if level is None:
        level = int(os.environ.get("UZ_OUT_BGZF_LEVEL", "6"))
    view, out = memoryview(data), []
    for at in range(0, len(view), SLICE):
        piece = view[at:at + SLICE]
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        stream = z.compress(piece) + z.flush()
        if len(stream) > 5 + len(piece):  # bytes that do not compress: one stored block, as the device writes it
            stream = b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + bytes(piece)
        out.append(bgzf_block(stream, piece))
    return b"".join(out), len(out)


def _as_bytes(parts):
    return b"".join(p.encode() if isinstance(p, str) else bytes(p) for p in parts)


def write_output(outfile, parts):
    """parts: the output's pieces in order, str or bytes-like.  Plain: text through sys.stdout for /dev/stdout, the same bytes to a file
    otherwise.  BGZF (see the module's head): the blocks, then the end-of-file marker."""
    if outfile == "/dev/stdout":
        for p in parts:
            sys.stdout.write(p if isinstance(p, str) else bytes(p).decode())
        return
    route = out_route() if outfile.endswith(".gz") else None
    if route is None:
        if all(isinstance(p, str) for p in parts):
            with open(outfile, "w") as fh:
                for p in parts:
                    fh.write(p)
        else:
            with open(outfile, "wb") as fh:
                for p in parts:
                    fh.write(p.encode() if isinstance(p, str) else p)
        return
    data = _as_bytes(parts)  # (with --gpus N > 1 only rank 0 gets here: unfazed.unfazed returns on the others before it writes)
    index = out_index()
    if index:
        from . import tabix_index
        preset = tabix_index.preset_of(data)
        for key in INDEX_KEYS:
            OUT_STATS.setdefault(key, 0)
    if route == "device":
        from . import session
        backend = session.get_backend()  # asked for by name: the route makes its backend, and fails loudly without a device
        blocks, n, _, kinds, *dev = backend.bgzf_deflate(data, code=out_code(), kinds=True, **({"index": preset} if index else {}))
        OUT_STATS["bgzf_device_blocks"] += n
        for key, k in zip(("stored", "fixed", "dynamic"), kinds):
            OUT_KINDS[key] += k
        if index:
            OUT_STATS["index_host_rows"] += dev[0]["host_rows"]
            tables, reason = tabix_index.from_device(data, dev[0])
    else:
        blocks, n = host_blocks(data)
        OUT_STATS["bgzf_host_blocks"] += n
        if index:
            tables, reason = tabix_index.build_host(data, tabix_index.block_sizes(blocks), preset)
    OUT_STATS["bgzf_calls"] += 1
    with open(outfile, "wb") as fh:
        fh.write(blocks)
        fh.write(BGZF_EOF)
    if not index:
        return
    if tables is None:  # no index, and none of an earlier run's beside the new file
        if os.path.exists(outfile + ".tbi"):
            os.remove(outfile + ".tbi")
        OUT_STATS["index_refused"] += 1
        sys.stderr.write("unfazed: no index written for %s: %s\n" % (outfile, reason))
        return
    tbi = tabix_index.serialize(preset, tables)
    tbi_blocks = backend.bgzf_deflate(tbi, code=out_code())[0] if route == "device" else host_blocks(tbi)[0]
    with open(outfile + ".tbi", "wb") as fh:
        fh.write(tbi_blocks)
        fh.write(BGZF_EOF)
    OUT_STATS["index_files"] += 1
