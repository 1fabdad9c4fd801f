"""Test-only sequential DCT JPEG encoder from GIVEN quantised coefficients to a stream (ITU T.81 F.1.2, one component, Huffman):
no forward DCT, so a test chooses the very codewords the decoder meets (ZRL chains, a non-zero 64th coefficient, large SSSS,
16-bit codes).  P = 8 (SOF0 or SOF1) or 12 (SOF1), quantisation tables of 8 or 16 bits, any restart interval, the Huffman
tables given, read out of a committed fixture's DHT segments (libjpeg's, = T.81 Annex K at P = 8), or optimal for the symbols
coded (tests/ljpeg_writer.optimal_table).  Also the DICOM slice / series writers over dicom_writer.  The streams are pinned
against libjpeg-turbo's decode in tests/test_dicom_jpeg_dct_cpu.py."""
import os
import struct

import numpy as np

import jpeg_dct_model as M
import ljpeg_writer as LW

JPEG_BASELINE = "1.2.840.10008.1.2.4.50"
JPEG_EXTENDED = "1.2.840.10008.1.2.4.51"
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_dct")
_CACHE = {}


def fixtures(which):
    """{name: (stream bytes, libjpeg's pixels)} of golden/jpeg_dct/<which>.npz ("p8", "p12")."""
    if which not in _CACHE:
        g = np.load(os.path.join(FIXTURES, which + ".npz"))
        _CACHE[which] = {str(n): (g["stream_" + str(n)].tobytes(), g["decoded_" + str(n)]) for n in g["names"]}
    return _CACHE[which]


def fixture_tables():
    """(dc, ac) Huffman tables, each (counts, values), read out of a committed libjpeg stream: the tables of T.81 Annex K, which
    hold DC SSSS up to 11 and AC SSSS up to 10 (libjpeg's 12-bit streams carry tables made for their image only)."""
    p = M.parse(fixtures("p8")["64x64_q75"][0])
    return p["dc"], p["ac"]


def block_symbols(coef_zz, pred):
    """One block's coefficients in zig-zag order -> [(class, symbol, extra bits value, extra bits count)]."""
    out = []
    d = int(coef_zz[0]) - pred
    s = abs(d).bit_length()
    out.append((0, s, d if d >= 0 else d + (1 << s) - 1, s))
    nz = np.flatnonzero(coef_zz[1:]) + 1
    k = 1
    for z in nz:
        run = int(z) - k
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        v = int(coef_zz[z])
        s = abs(v).bit_length()
        out.append((1, (run << 4) | s, v if v >= 0 else v + (1 << s) - 1, s))
        k = int(z) + 1
    if k < 64:
        out.append((1, 0x00, 0, 0))
    return out


def encode(coef, *, rows, cols, P=8, qt=None, qbits=8, dc=None, ac=None, optimal=False, ri=0, sof=None, dc_id=0, ac_id=0,
           q_id=0):
    """coef: int [blocks, 64] quantised coefficients in natural order (blocks = the padded image's, raster order) -> one frame
    (SOI .. EOI).  qt: [64] natural order (default all ones); dc / ac: (counts, values), default `fixture_tables()`, or with
    optimal=True the optimal tables of the symbols coded."""
    coef = np.asarray(coef, dtype=np.int64)
    nb = -(-rows // 8) * -(-cols // 8)
    assert coef.shape == (nb, 64) and P in (8, 12) and qbits in (8, 16)
    qt = np.ones(64, dtype=np.int64) if qt is None else np.asarray(qt, dtype=np.int64)
    assert qt.min() >= 1 and qt.max() < (1 << qbits)
    zz = coef[:, M.ZIGZAG]
    R = ri or nb
    syms, pred = [], 0
    for b in range(nb):
        if b % R == 0:
            pred = 0
        syms.append(block_symbols(zz[b], pred))
        pred = int(zz[b, 0])
    if optimal:
        freq = [np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)]
        for blk in syms:
            for c, s, _, _ in blk:
                freq[c][s] += 1
        dc, ac = LW.optimal_table(freq[0]), LW.optimal_table(freq[1])
    elif dc is None or ac is None:
        fdc, fac = fixture_tables()
        dc, ac = dc or fdc, ac or fac
    books = [LW.canonical_codes(*dc), LW.canonical_codes(*ac)]
    ecs = b""
    for k, b0 in enumerate(range(0, nb, R)):
        if k:
            ecs += bytes([0xFF, 0xD0 + (k - 1) % 8])
        lengths, vals = [], []
        for blk in syms[b0:b0 + R]:
            for c, s, extra, n in blk:
                code, ln = books[c][s]
                lengths.append(ln + n)
                vals.append((code << n) | extra)
        ecs += LW._pack(lengths, vals)
    seg = lambda m, body: bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body   # noqa: E731
    qzz = np.zeros(64, dtype=np.int64)
    qzz[:] = qt[M.ZIGZAG]
    out = b"\xFF\xD8" + seg(0xDB, bytes([((qbits == 16) << 4) | q_id]) + qzz.astype(">u2" if qbits == 16 else np.uint8).tobytes())
    sof = (0xC0 if P == 8 else 0xC1) if sof is None else sof
    out += seg(sof, struct.pack(">BHHB", P, rows, cols, 1) + bytes([1, 0x11, q_id]))
    out += seg(0xC4, bytes([dc_id]) + bytes(dc[0]) + bytes(dc[1]) + bytes([0x10 | ac_id]) + bytes(ac[0]) + bytes(ac[1]))
    if ri:
        out += seg(0xDD, struct.pack(">H", ri))
    out += seg(0xDA, bytes([1, 1, (dc_id << 4) | ac_id, 0, 63, 0]))
    return out + ecs + b"\xFF\xD9"


def random_coefficients(rng, nb, P, *, density=0.3, amp=None, dc_amp=None):
    """Plausible quantised coefficients: sparse ACs of decaying magnitude, DCs within the sample range."""
    amp = amp or (1 << (P - 3))
    dc_amp = dc_amp or (1 << (P - 1))
    scale = np.maximum(1, amp / (1 + np.arange(64)))[M.ZIGZAG.argsort()]
    c = np.rint(rng.normal(0, 1, (nb, 64)) * scale * (rng.random((nb, 64)) < density)).astype(np.int64)
    c[:, 0] = rng.integers(-dc_amp // 2, dc_amp // 2, nb)
    return c


def write_compressed_series(folder, streams, decoded, *, transfer_syntax=JPEG_EXTENDED, origin=(-100.0, -120.0, 50.0),
                            iop=(1, 0, 0, 0, 1, 0), dz=1.5, name="IM%04d.dcm", **kw):
    """One DICOM slice per stream (decoded[z]: the stored values it decodes to; only their shape is used), slice z at
    origin + z * dz * normal."""
    os.makedirs(folder, exist_ok=True)
    iop_a = np.asarray(iop, dtype=float)
    normal = np.cross(iop_a[:3], iop_a[3:])
    paths = []
    for z, st in enumerate(streams):
        p = os.path.join(folder, name % z)
        LW.write_compressed_slice(p, decoded[z], st, transfer_syntax=transfer_syntax,
                                  ipp=np.asarray(origin, dtype=float) + z * dz * normal, iop=iop, instance=z + 1, **kw)
        paths.append(p)
    return paths
