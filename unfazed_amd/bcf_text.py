"""One BCF2 record into its VCF text line, in plain Python: the rules csrc/bcf_row.hpp states for the device, stated again without it.  Three
uses: the host route of UZ_BCF_ROUTE, the writer of the records the device hands back, and the statement the hand-built panel
(tests/bcfrowcases.py) checks first.  The text form is pinned by the BCF2 / VCF specifications and by C's "%g", which Python's "%g" equals.

Where the device prints, this prints the same characters.  Where the device hands a record back, this either writes the line (a float that
"%g" prints in exponent form, an infinity, a NaN) or raises ValueError: the rules have no line for the record."""
import struct

FLOAT_MISSING, FLOAT_EOV = 0x7F800001, 0x7F800002
_SIZE = {0: 0, 1: 1, 2: 2, 3: 4, 5: 4, 7: 1}
_INT = {1: ("<b", -128), 2: ("<h", -32768), 3: ("<i", -2147483648)}


class _Bad(ValueError):
    pass


def _int(data, type_, at, k):
    """entry k of an integer vector -> a value, None (the missing marker) or "eov" """
    fmt, lowest = _INT[type_]
    x = struct.unpack_from(fmt, data, at + k * _SIZE[type_])[0]
    return None if x == lowest else "eov" if x == lowest + 1 else x


def _desc(data, at, end):
    """a typed value's descriptor -> (type, n, at behind it)"""
    if at >= end:
        raise _Bad("a descriptor outside its block")
    b = data[at]
    at += 1
    type_, n = b & 15, b >> 4
    if n == 15:
        if at >= end:
            raise _Bad("a length outside its block")
        b2 = data[at]
        at += 1
        if (b2 & 15) not in _INT or b2 >> 4 != 1 or end - at < _SIZE[b2 & 15]:
            raise _Bad("a length that is no typed scalar integer inside its block")
        n = _int(data, b2 & 15, at, 0)
        if not isinstance(n, int) or n < 0:
            raise _Bad("a negative length")
        at += _SIZE[b2 & 15]
    if type_ not in _SIZE:
        raise _Bad("type %d" % type_)
    return type_, n, at


def _typed(data, at, end):
    """-> (type, n, where the entries start, at behind them)"""
    type_, n, at = _desc(data, at, end)
    if end - at < n * _SIZE[type_]:
        raise _Bad("a value outside its block")
    return type_, n, at, at + n * _SIZE[type_]


def _key(data, at, end):
    type_, n, p, at = _typed(data, at, end)
    if type_ not in _INT or n != 1 or not isinstance(_int(data, type_, p, 0), int):
        raise _Bad("a key that is no scalar integer")
    return _int(data, type_, p, 0), at


def _name(names, i, what):
    if not 0 <= i < len(names) or not names[i]:
        raise _Bad("%s id %d without a name" % (what, i))
    return _text(names[i].encode() if isinstance(names[i], str) else bytes(names[i]))


def _text(b):
    if any(c < 0x20 or c > 0x7E for c in b):
        raise _Bad("a byte outside 0x20 .. 0x7E in a string")
    return b.decode("ascii")


def _float(bits):
    return "%g" % struct.unpack("<f", struct.pack("<I", bits))[0]


def _vector(data, type_, at, n):
    out = []
    if type_ == 7:
        b = bytes(data[at:at + n]).split(b"\0", 1)[0]
        return _text(b) or "."
    if type_ == 5:
        for k in range(n):
            bits = struct.unpack_from("<I", data, at + 4 * k)[0]
            if bits == FLOAT_EOV:
                break
            out.append("." if bits == FLOAT_MISSING else _float(bits))
    elif type_ in _INT:
        for k in range(n):
            x = _int(data, type_, at, k)
            if x == "eov":
                break
            out.append("." if x is None else str(x))
    return ",".join(out) or "."


def _gt(data, type_, at, n):
    out = ""
    k = 0
    for k in range(n):
        x = _int(data, type_, at, k)
        if x == "eov":
            break
        x = 0 if x is None else x
        if x < 0:
            raise _Bad("a negative GT entry")
        out += ("|" if x & 1 else "/") if out else ""
        out += "." if x >> 1 == 0 else str((x >> 1) - 1)
    return out or "."


def line(data, rec_at, dict_names, contig_names, n_samples, index=None):
    """The VCF line (no line end) of the record whose l_shared word lies at data[rec_at].  dict_names: the FILTER / INFO / FORMAT dictionary by
    id, contig_names: the header's contigs by id (an undefined id: an empty name); n_samples: the header's sample count.  ValueError, naming
    `index`, where the rules have no line."""
    try:
        return _line(data, int(rec_at), dict_names, contig_names, int(n_samples))
    except _Bad as e:
        raise ValueError("BCF record %s: %s" % ("?" if index is None else index, e)) from None


def _line(data, rec_at, dict_names, contig_names, n_samples):
    size = len(data)
    if rec_at < 0 or size - rec_at < 8:
        raise _Bad("a record outside the data")
    ls, li = struct.unpack_from("<II", data, rec_at)
    if ls < 24 or ls > size - rec_at - 8 or li > size - rec_at - 8 - ls:
        raise _Bad("a block outside the data")
    at = rec_at + 8
    send, iend = at + ls, at + ls + li
    chrom, pos, _, qual, nai, nfs = struct.unpack_from("<iiiIII", data, at)
    n_allele, n_info, n_fmt, n_smp = nai >> 16, nai & 0xFFFF, nfs >> 24, nfs & 0xFFFFFF
    at += 24
    if n_allele == 0:
        raise _Bad("no allele")
    if n_fmt and n_smp != n_samples:
        raise _Bad("%d samples, the header has %d" % (n_smp, n_samples))
    cols = [_name(contig_names, chrom, "contig"), str(pos + 1)]
    alleles = []
    for k in range(1 + n_allele):  # ID, then the alleles
        type_, n, p, at = _typed(data, at, send)
        if type_ != 7 and n:
            raise _Bad("an ID or allele that is no string")
        s = _text(bytes(data[p:p + n]))
        if k == 0:
            cols.append(s or ".")
        else:
            alleles.append(s)
    cols += [alleles[0], ",".join(alleles[1:]) if n_allele > 1 else "."]
    cols.append("." if qual == FLOAT_MISSING else _float(qual))
    type_, n, p, at = _typed(data, at, send)
    if type_ not in _INT and n:
        raise _Bad("a FILTER that is no integer vector")
    names = []
    for k in range(n):
        x = _int(data, type_, p, k)
        if x == "eov":
            break
        if x is None:
            raise _Bad("a missing FILTER id")
        names.append(_name(dict_names, x, "dictionary"))
    cols.append(";".join(names) or ".")
    info = []
    for _k in range(n_info):
        key, at = _key(data, at, send)
        name = _name(dict_names, key, "dictionary")
        type_, n, p, at = _typed(data, at, send)
        info.append(name if type_ == 0 or n == 0 else name + "=" + _vector(data, type_, p, n))
    cols.append(";".join(info) or ".")
    if n_fmt and n_smp:
        fields, f = [], send
        for _k in range(n_fmt):
            key, f = _key(data, f, iend)
            name = _name(dict_names, key, "dictionary")
            type_, n, f = _desc(data, f, iend)
            per = n * _SIZE[type_]
            if iend - f < per * n_smp:
                raise _Bad("a FORMAT array outside its block")
            fields.append((name, type_, n, f, per))
            f += per * n_smp
        cols.append(":".join(x[0] for x in fields))
        for s in range(n_smp):
            cols.append(":".join(_gt(data, t, p + s * per, n) if name == "GT" and t in _INT else _vector(data, t, p + s * per, n)
                                 for name, t, n, p, per in fields))
    return "\t".join(cols)


def lines(data, rec_at, dict_names, contig_names, n_samples, only=None):
    """line() of every record (or of the records `only` names) -> list of str"""
    ks = range(len(rec_at)) if only is None else only
    return [line(data, rec_at[k], dict_names, contig_names, n_samples, index=k) for k in ks]
