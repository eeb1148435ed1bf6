"""An independent LIME / ILDG / SciDAC-ETMC writer and reader in pure Python (struct + numpy), built from the public format
description alone (the "format facts" in include/ddamg_hip_io.h); it does not go through the library.  The c-lime library that
the reference links is not available to produce fixtures, so this module is the second implementation the library is held against
(tests/test_lime_formats.py, tests/test_gpu_ildg.py)."""
import re, struct
import numpy as np

MAGIC = bytes([0x45, 0x67, 0x89, 0xAB])
HEADER = 144


def pad8(n):
    return (n + 7) // 8 * 8


def header(rtype, length, flags=0xC0):
    """magic, version 1, flags (0x80 message begin | 0x40 message end), reserved 0, length, type: all big endian"""
    assert len(rtype) < 128
    head = MAGIC + struct.pack(">HBBQ", 1, flags, 0, length) + rtype.encode().ljust(128, b"\0")
    assert len(head) == HEADER
    return head


def record(rtype, data, flags=0xC0):
    """header + data + zero padding of one record"""
    return header(rtype, len(data), flags) + bytes(data) + b"\0" * (pad8(len(data)) - len(data))


def parse(path, keep=1 << 16):
    """[(type, flags, version, offset of the data, length, data or None if longer than `keep`, padding bytes)] and the offset
    behind the last record; asserts the magic number, the reserved byte and the NUL fill of the type field"""
    out = []
    with open(path, "rb") as f:
        f.seek(0, 2); size = f.tell(); off = 0
        while off < size:
            f.seek(off); h = f.read(HEADER)
            assert len(h) == HEADER, "file ends inside a record header"
            assert h[:4] == MAGIC, "bad magic"
            version, flags, reserved, length = struct.unpack(">HBBQ", h[4:16])
            assert reserved == 0
            name = h[16:]
            end = name.index(b"\0")
            assert name[end:] == b"\0" * (128 - end)
            data = pad = None
            if length <= keep:
                data = f.read(length); pad = f.read(pad8(length) - length)
                assert len(data) == length and len(pad) == pad8(length) - length
            out.append((name[:end].decode(), flags, version, off + HEADER, length, data, pad))
            off += HEADER + pad8(length)
    return out, off


def tag(text, name):
    return int(re.search(r"<%s>\s*(-?\d+)" % name, text).group(1))


def ildg_format_xml(L, precision):
    """L = [T,Z,Y,X]"""
    return ('<?xml version="1.0" encoding="UTF-8"?><ildgFormat xmlns="http://www.lqcd.org/ildg"><version>1.0</version><field>su3gauge</field>'
            "<precision>%d</precision><lx>%d</lx><ly>%d</ly><lz>%d</lz><lt>%d</lt></ildgFormat>" % (precision, L[3], L[2], L[1], L[0]))


def ildg_bytes(U, precision):
    """links [V][4(T,Z,Y,X)][9][2] -> the bytes of ildg-binary-data: directions X,Y,Z,T, big endian"""
    a = np.asarray(U, dtype=np.float64).reshape(-1, 4, 18)[:, ::-1, :]
    return np.ascontiguousarray(a).astype(">f8" if precision == 64 else ">f4").tobytes()


def ildg_links(raw, precision):
    """the inverse: bytes -> [V][4(T,Z,Y,X)][9][2] float64"""
    a = np.frombuffer(raw, dtype=">f8" if precision == 64 else ">f4").reshape(-1, 4, 18)[:, ::-1, :]
    return np.ascontiguousarray(a).astype(np.float64).reshape(-1, 4, 9, 2)


def write_ildg(path, L, U, precision=64, plaquette=None, xlf_text=None, extra_first=()):
    """plaquette: the number that goes into the file (average plaquette in [0,1]); None: no xlf-info record"""
    with open(path, "wb") as f:
        for r in extra_first:
            f.write(record(*r))
        f.write(record("ildg-format", ildg_format_xml(L, precision).encode()))
        if plaquette is not None or xlf_text is not None:
            f.write(record("xlf-info", (xlf_text if xlf_text is not None else "plaquette = %.17g\n trajectory nr = 7\n" % plaquette).encode()))
        f.write(record("ildg-binary-data", ildg_bytes(U, precision)))


def read_ildg(path):
    """(L [T,Z,Y,X], precision, links [V][4][9][2], the file's plaquette or None)"""
    recs, _ = parse(path, keep=1 << 40)
    by = {r[0]: r for r in recs}
    text = by["ildg-format"][5].decode()
    L = [tag(text, n) for n in ("lt", "lz", "ly", "lx")]; precision = tag(text, "precision")
    plaq = None
    if "xlf-info" in by:
        m = re.search(r"plaquette =\s*([-+0-9.eE]+)", by["xlf-info"][5].decode())
        plaq = float(m.group(1)) if m else None
    raw = by["ildg-binary-data"][5]
    assert len(raw) == int(np.prod(L)) * 72 * precision // 8
    return L, precision, ildg_links(raw, precision), plaq


def etmc_format_xml(L, precision, flavours=1, spin=4, colour=3):
    return ("<?xml version=\"1.0\" encoding=\"UTF-8\"?>\n<etmcFormat>\n<field>diracFermion</field>\n<precision>%d</precision>\n<flavours>%d</flavours>\n"
            "<lx>%d</lx>\n<ly>%d</ly>\n<lz>%d</lz>\n<lt>%d</lt>\n<spin>%d</spin>\n<colour>%d</colour>\n</etmcFormat>"
            % (precision, flavours, L[3], L[2], L[1], L[0], spin, colour))


def write_vector(path, L, v, precision=64, format_record="etmc-propagator-format", **fmt):
    with open(path, "wb") as f:
        f.write(record(format_record, etmc_format_xml(L, precision, **fmt).encode()))
        f.write(record("scidac-binary-data", np.asarray(v, dtype=np.float64).astype(">f8" if precision == 64 else ">f4").tobytes()))
