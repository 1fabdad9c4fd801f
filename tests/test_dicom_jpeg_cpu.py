"""JPEG Lossless DICOM input, host side (no device): encapsulated PixelData, the marker parser's acceptance and refusals, and
the compressed syntaxes that stay refused."""
import struct

import numpy as np
import pytest

import ljpeg_writer as W
from dicom_writer import write_series, write_slice
from boa_hip import dicom, jpeg_lossless as J
from boa_hip.dicom import DicomError


def _img(h=20, w=24, P=12, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << P, (h, w))


def _parse(stream, h=20, w=24, alloc=16, stored=12):
    return J.parse_frame(stream, rows=h, cols=w, bits_allocated=alloc, bits_stored=stored, name="f.dcm")


def _seg(m, body):
    return bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body


def _replace(stream, marker, new):
    """Replace the marker segment `marker` of a stream by the bytes `new`."""
    i = stream.index(bytes([0xFF, marker]))
    ln = struct.unpack(">H", stream[i + 2:i + 4])[0]
    return stream[:i] + new + stream[i + 2 + ln:]


def test_parser_accepts_and_locates_intervals():
    x = _img()
    s = W.encode(x, precision=12, predictor=4, pt=1, restart_rows=3, table_id=2)
    s = s[:2] + _seg(0xE0, b"JFIF\0" + bytes(9)) + _seg(0xFE, b"comment") + s[2:]     # APP0 and COM are skipped
    fr = _parse(s)
    assert (fr.precision, fr.pt, fr.predictor, fr.restart_rows) == (12, 1, 4, 3)
    assert len(fr.seg_bounds) == 8 and fr.seg_bounds[0] == 0 and fr.seg_bounds[-1] == len(fr.data)
    assert (np.diff(fr.seg_bounds) > 0).all()
    # un-stuffed data holds no RST marker and every stuffed FF once
    ecs = s[s.index(b"\xFF\xDA") + 10:-2]
    assert len(fr.data) == len(ecs) - ecs.count(b"\xFF\x00") - 2 * 6
    # several DHT segments / tables: the scan's table is the one taken
    t1 = W.optimal_table(np.ones(17))
    s2 = W.encode(x, precision=12, table_id=1, extra_tables=[(0, *t1), (3, *t1)])
    assert _parse(s2).counts == W.optimal_table(np.bincount(W.categories(W.differences(x, precision=12))[0].ravel(),
                                                            minlength=17))[0]
    # fill bytes ahead of markers
    s3 = W.encode(x, precision=12)
    s3 = s3[:-2] + b"\xFF\xFF\xFF\xD9"
    assert len(_parse(s3).data) == len(_parse(W.encode(x, precision=12)).data)


def test_table_expansion_matches_canonical_codes():
    counts, values = W.optimal_table(np.array([5, 50, 400, 900, 700, 300, 90, 30, 9, 4, 2, 1, 1, 1, 1, 1, 1]))
    T = J.expand_table(counts, values)
    look = T[:256].view(np.uint16)
    maxcode, valoff = T[256:274].view(np.int32), T[274:292].view(np.int32)
    hv = T[292:356].view(np.uint8)
    for v, (code, ln) in W.canonical_codes(counts, values).items():
        if ln <= J.LOOKUP_BITS:
            sh = J.LOOKUP_BITS - ln
            assert (look[code << sh:(code + 1) << sh] == (ln << 8) | v).all()
        else:
            assert code <= maxcode[ln] and hv[valoff[ln] + code] == v
    assert max(ln for _, ln in W.canonical_codes(counts, values).values()) > J.LOOKUP_BITS


@pytest.mark.parametrize("marker,process", [(0xC0, "baseline"), (0xC1, "extended sequential"), (0xC2, "progressive"),
                                            (0xC7, "differential lossless"), (0xCB, "lossless \\(arithmetic\\)"),
                                            (0xF7, "JPEG-LS")])
def test_other_processes_raise_not_implemented(marker, process):
    s = W.encode(_img(), precision=12)
    i = s.index(b"\xFF\xC3")
    s = s[:i + 1] + bytes([marker]) + s[i + 2:]
    with pytest.raises(NotImplementedError, match=process):
        _parse(s)


def test_refusals_name_what_was_found():
    x = _img()
    s = W.encode(x, precision=12)
    sof = lambda p=12, y=20, xx=24, nf=1: _seg(0xC3, struct.pack(">BHHB", p, y, xx, nf) + bytes([1, 0x11, 0]) * nf)  # noqa: E731
    with pytest.raises(DicomError, match="0 lines"):
        _parse(_replace(s, 0xC3, sof(y=0)))
    with pytest.raises(DicomError, match="differs from Rows x Columns"):
        _parse(_replace(s, 0xC3, sof(y=21)))
    with pytest.raises(DicomError, match="components"):
        _parse(_replace(s, 0xC3, sof(nf=3)))
    with pytest.raises(DicomError, match="precision 12 outside"):
        _parse(s, alloc=8, stored=8)
    with pytest.raises(DicomError, match="precision 12 outside"):
        _parse(s, stored=16)
    with pytest.raises(DicomError, match="no DHT defined"):
        _parse(_replace(s, 0xC4, b""))
    with pytest.raises(DicomError, match="table 1, which no DHT defined"):
        t = W.optimal_table(np.bincount(W.categories(W.differences(x, precision=12))[0].ravel(), minlength=17))
        _parse(W.encode(x, precision=12, table=t, table_id=1)[:2] + W.encode(x, precision=12, table=t, table_id=0)[2:]
               .replace(bytes([0xFF, 0xDA, 0, 8, 1, 1, 0x00]), bytes([0xFF, 0xDA, 0, 8, 1, 1, 0x10])))
    with pytest.raises(DicomError, match="DNL"):
        _parse(s[:-2] + _seg(0xDC, struct.pack(">H", 20)) + b"\xFF\xD9")
    with pytest.raises(DicomError, match="more than one scan"):
        sos = s.index(b"\xFF\xDA")
        _parse(s[:-2] + s[sos:])
    with pytest.raises(DicomError, match="EOI missing"):
        _parse(s[:-2])
    with pytest.raises(DicomError, match="restart intervals"):
        _parse(W.encode(x, precision=12, restart_rows=5).replace(b"\xFF\xD2", b""))
    with pytest.raises(NotImplementedError, match="whole number"):
        _parse(_replace(W.encode(x, precision=12), 0xC4, _seg(0xDD, struct.pack(">H", 30)) +
                        s[s.index(b"\xFF\xC4"):s.index(b"\xFF\xC3")]))
    with pytest.raises(DicomError, match="SOI"):
        _parse(s[2:])


def _file_bytes(tmp_path, name, **kw):
    x = _img(P=16, seed=4)
    stream = W.encode(x, precision=16)
    p = tmp_path / name
    W.write_compressed_slice(p, x, stream, ipp=(0, 0, 0), **kw)
    return p, stream


@pytest.mark.parametrize("fragments,bot", [(1, False), (1, True), (3, False), (3, True)])
def test_encapsulated_fragments(tmp_path, fragments, bot):
    p, stream = _file_bytes(tmp_path, "a.dcm", fragments=fragments, bot=bot)
    ds = dicom.read_file(p)
    px = ds["PixelData"]
    assert isinstance(px, J.CompressedFrame) and px.transfer_syntax == W.JPEG_LOSSLESS_SV1
    assert bytes(px).rstrip(b"\0") == stream and len(px) == len(stream) + len(stream) % 2   # odd frame: one pad byte
    fr = J.parse_frame(px, rows=20, cols=24, name=str(p))
    assert fr.predictor == 1
    assert dicom.read_file(p, stop_before_pixels=True).get("PixelData") is None


def test_encapsulated_errors(tmp_path):
    p, _ = _file_bytes(tmp_path, "a.dcm")
    buf = p.read_bytes()
    with pytest.raises(DicomError, match="sequence delimiter"):
        (tmp_path / "b.dcm").write_bytes(buf[:-8])
        dicom.read_file(tmp_path / "b.dcm")
    i = buf.index(struct.pack("<HH2sHI", 0x7FE0, 0x0010, b"OB", 0, 0xFFFFFFFF)) + 12
    two_frames = buf[:i] + struct.pack("<HHI", 0xFFFE, 0xE000, 8) + bytes(8) + buf[i + 8:]
    (tmp_path / "c.dcm").write_bytes(two_frames)
    with pytest.raises(NotImplementedError, match="multi-frame"):
        dicom.read_file(tmp_path / "c.dcm")


def test_native_pixel_data_under_jpeg_syntax_refused_before_the_device(tmp_path):
    vol = np.zeros((10, 8, 8), dtype=np.int64)
    write_series(tmp_path / "s", vol, transfer_syntax=W.JPEG_LOSSLESS_SV1)
    with pytest.raises(NotImplementedError, match="transfer syntax"):
        dicom.load_series(tmp_path / "s", ctx=object())    # (a context that would fail if it were used)


def test_refusal_precedes_device_in_load_series(tmp_path):
    """A frame the parser refuses raises from load_series before the context is touched."""
    x = _img(P=16, seed=1)
    s = W.encode(x, precision=16)
    i = s.index(b"\xFF\xC3")
    for z in range(3):
        W.write_compressed_slice(tmp_path / f"IM{z}.dcm", x, s[:i + 1] + b"\xC1" + s[i + 2:] if z == 1 else s,
                                 ipp=(0, 0, 1.5 * z), instance=z + 1)
    with pytest.raises(NotImplementedError, match="extended sequential"):
        dicom.load_series(tmp_path, ctx=object())


@pytest.mark.parametrize("ts", ["1.2.840.10008.1.2.2", "1.2.840.10008.1.2.1.99", "1.2.840.10008.1.2.4.50",
                                "1.2.840.10008.1.2.4.51", "1.2.840.10008.1.2.4.80", "1.2.840.10008.1.2.4.81",
                                "1.2.840.10008.1.2.4.90", "1.2.840.10008.1.2.4.91", "1.2.840.10008.1.2.5"])
def test_other_syntaxes_still_refused(tmp_path, ts):
    write_slice(tmp_path / "a.dcm", np.zeros((4, 4)), ipp=(0, 0, 0), transfer_syntax=ts)
    with pytest.raises(NotImplementedError, match="transfer syntax"):
        dicom.read_file(tmp_path / "a.dcm")
