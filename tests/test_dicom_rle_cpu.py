"""CPU: the RLE Lossless (PS3.5 Annex G) host side -- tests/rle_writer.py's encoder styles and decoder model against each other
and against libtiff's PackBits strips (tests/golden/rle), `dicom.read_file` on RLE files, the refusals of
`rle_lossless.parse_frame`, and that a refusal raises from `load_series` before the device is touched."""
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN
import rle_writer as R
from boa_hip import dicom, rle_lossless as RL
from boa_hip.dicom import DicomError
from boa_hip.jpeg_lossless import CompressedFrame


def _img(rows=21, cols=301, seed=0):
    rng = np.random.default_rng(seed)
    x = np.full((rows, cols), 24, dtype=np.int64)
    x[:, cols // 4:3 * cols // 4] = 1064 + rng.integers(-30, 31, (rows, 3 * cols // 4 - cols // 4))
    x[rows // 2] = 700                                   # a whole constant row, and constant row ends that meet the next row's start
    return x


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "rle", "packbits_libtiff.npz"))


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("mode", R.MODES)
def test_model_round_trip(mode, bits):
    for shape in ((1, 1), (1, 300), (300, 1), (21, 301)):
        x = _img(*shape, seed=bits) & ((1 << bits) - 1)
        frame = R.encode_frame(x, bits, mode)
        assert len(frame) % 2 == 0 and struct.unpack_from("<II", frame) == (bits // 8, 64)
        px, st = R.decode_frame(frame, *shape)
        assert st == 0
        np.testing.assert_array_equal(px, x)
        for seg in R.segments_of(frame):
            assert (0x80 in [t[0] for t in _controls(seg)]) == (mode == "noops")
            assert R.chunked_decode(seg, 256, x.size) == R.decode_segment(seg, x.size)


def _controls(seg):
    p, out = 0, []
    while p < len(seg):
        adv, _ = R.step(seg[p])
        if p + adv > len(seg):
            break
        out.append(seg[p:p + adv])
        p += adv
    return out


def test_encoder_styles_are_what_they_say():
    x = _img()
    hi, lo = R.planes_of(x, 16)
    rows = R.tokens(lo, "rows")
    per_row = [sum(R.step(t[0])[1] for t in R.tokens(lo[r:r + 1], "rows")) for r in range(lo.shape[0])]
    assert per_row == [lo.shape[1]] * lo.shape[0] and b"".join(rows) == b"".join(b"".join(R.tokens(lo[r:r + 1], "rows"))
                                                                                 for r in range(lo.shape[0]))
    ends = set(np.cumsum([R.step(t[0])[1] for t in R.tokens(hi, "crossing")]).tolist())
    assert not set(range(hi.shape[1], hi.size, hi.shape[1])) <= ends             # runs that cross the row ends
    assert {t[0] for t in R.tokens(lo, "literal")[:-1]} == {127}
    assert {t[0] for t in R.tokens(lo, "dense")} == {0, 255}
    assert R.encode_segment(lo, "noops", k=700, at=(5,)).count(b"\x80" * 700) == 1


def test_libtiff_golden_decodes_with_the_model(golden):
    for i in range(2):
        src = golden[f"source_{i}"]
        strips = [golden[f"strip_{i}_{k}"].tobytes() for k in range(2)]
        assert all(0x80 not in [t[0] for t in _controls(s)] for s in strips)
        px, st = R.decode_frame(R.frame_of(strips), *src.shape)
        assert st == 0
        np.testing.assert_array_equal(px, src)
        # libtiff encodes every row on its own, as the writer's conforming style does: the same number of bytes per row
        for k, plane in enumerate(R.planes_of(src, 16)):
            p = 0
            for r in range(src.shape[0]):
                got, st = R.decode_segment(strips[k][p:], src.shape[1])
                assert st == 0 and got == plane[r].tobytes()
                n = 0
                while n < src.shape[1]:
                    adv, out = R.step(strips[k][p])
                    p, n = p + adv, n + out
                assert n == src.shape[1], "a libtiff run crosses a row end"
            assert p == len(strips[k])


@pytest.mark.parametrize("fragments,bot", [(1, False), (1, True), (3, False), (3, True)])
def test_read_file_returns_a_tagged_frame(tmp_path, fragments, bot):
    x = _img()
    frame = R.encode_frame(x, 16)
    R.write_slice(tmp_path / "a.dcm", x, frame, ipp=(0, 0, 0), fragments=fragments, bot=bot)
    ds = dicom.read_file(tmp_path / "a.dcm")
    assert isinstance(ds["PixelData"], CompressedFrame) and ds["PixelData"].transfer_syntax == RL.RLE_LOSSLESS
    assert bytes(ds["PixelData"]) == frame and ds["BitsAllocated"] == 16 and ds["Rows"] == x.shape[0]
    fr = RL.parse_frame(ds["PixelData"], rows=x.shape[0], cols=x.shape[1], bits_allocated=16, name="a.dcm")
    assert [bytes(fr.data[a:b]) for a, b in fr.bounds] == R.segments_of(frame)
    assert "PixelData" not in dicom.read_file(tmp_path / "a.dcm", stop_before_pixels=True)


def test_read_file_8_bit_and_header_plausibility(tmp_path):
    x = _img() & 0xFF
    R.write_slice(tmp_path / "b.dcm", x, bits_allocated=8, ipp=(0, 0, 0))
    ds = dicom.read_file(tmp_path / "b.dcm")
    assert ds["BitsAllocated"] == 8 and ds["BitsStored"] == 8
    fr = RL.parse_frame(ds["PixelData"], rows=x.shape[0], cols=x.shape[1], bits_allocated=8, name="b.dcm")
    assert len(fr.bounds) == 1 and fr.bounds[0] == (64, len(ds["PixelData"]))
    # what does not start like an RLE header is an unsupported file, by the syntax's name
    good = R.encode_frame(x, 8)
    for k, bad in enumerate((good[:40], struct.pack("<I", 0) + good[4:], struct.pack("<I", 16) + good[4:],
                             good[:4] + struct.pack("<I", 66) + good[8:], b"\xFF\x4F\xFF\x51" + good[4:])):
        R.write_slice(tmp_path / f"bad{k}.dcm", x, bad, bits_allocated=8, ipp=(0, 0, 0))
        with pytest.raises(NotImplementedError, match="transfer syntax 1.2.840.10008.1.2.5: PixelData does not start with an RLE header"):
            dicom.read_file(tmp_path / f"bad{k}.dcm")


def _header(count, offsets, body=bytes(200)):
    return struct.pack("<16I", count, *(list(offsets) + [0] * (15 - len(offsets)))) + body


def test_parse_frame_refusals():
    kw = dict(rows=4, cols=5, name="x.dcm")
    ok = RL.parse_frame(_header(2, [64, 100]), bits_allocated=16, **kw)
    assert ok.bounds == [(64, 100), (100, 264)]
    # unused offsets are not looked at
    assert RL.parse_frame(_header(2, [64, 100, 7, 0xFFFFFFFF]), bits_allocated=16, **kw).bounds == ok.bounds
    for count, alloc in ((3, 8), (4, 16), (1, 16), (2, 8), (3, 16), (15, 16)):
        with pytest.raises(NotImplementedError, match=f"x.dcm: RLE frame of {count} segments with BitsAllocated {alloc}"):
            RL.parse_frame(_header(count, [64 + 2 * k for k in range(count)]), bits_allocated=alloc, **kw)
    with pytest.raises(NotImplementedError, match="BitsAllocated 32"):
        RL.parse_frame(_header(4, [64, 70, 80, 90]), bits_allocated=32, **kw)
    with pytest.raises(DicomError, match="x.dcm: first RLE segment at offset 68, 64 expected"):
        RL.parse_frame(_header(2, [68, 100]), bits_allocated=16, **kw)
    for second in (64, 63, 0):
        with pytest.raises(DicomError, match="x.dcm: RLE segment offsets are not increasing"):
            RL.parse_frame(_header(2, [64, second]), bits_allocated=16, **kw)
    for second in (264, 265, 0x7FFFFFFF):
        with pytest.raises(DicomError, match=f"x.dcm: RLE segment offset {second} is outside the 264-byte frame"):
            RL.parse_frame(_header(2, [64, second]), bits_allocated=16, **kw)
    with pytest.raises(DicomError, match="x.dcm: RLE segment offset 64 is outside the 64-byte frame"):
        RL.parse_frame(_header(1, [64], b""), bits_allocated=8, **kw)
    for n in (0, 10, 63):
        with pytest.raises(DicomError, match=f"x.dcm: RLE frame of {n} bytes is shorter than its 64-byte header"):
            RL.parse_frame(_header(2, [64, 100])[:n], bits_allocated=16, **kw)
    for count in (0, 16, 0xFFFFFFFF):
        with pytest.raises(DicomError, match=f"x.dcm: RLE header with {count} segments"):
            RL.parse_frame(_header(count, [64, 100]), bits_allocated=16, **kw)


def test_build_batch_tables():
    x = _img()
    frames = [RL.parse_frame(R.encode_frame(x, 16, m), rows=x.shape[0], cols=x.shape[1], name=m) for m in ("rows", "literal")]
    frames.append(RL.parse_frame(R.encode_frame(x & 0xFF, 8), rows=x.shape[0], cols=x.shape[1], bits_allocated=8, name="8"))
    data, ftab = RL.build_batch(frames)
    assert ftab.shape == (3, RL.FRAME_WORDS) and ftab.dtype == np.int32 and len(data) == sum(len(f.data) for f in frames)
    off = 0
    for f, row in zip(frames, ftab):
        assert list(row[:4]) == [off, 0, len(f.data), len(f.bounds)]
        assert list(row[4:4 + 2 * len(f.bounds)]) == [v for b in f.bounds for v in b] and not row[4 + 2 * len(f.bounds):].any()
        assert bytes(data[off:off + len(f.data)]) == bytes(f.data)
        off += len(f.data)


def test_refusal_precedes_device_in_load_series(tmp_path):
    """A frame the header parser refuses raises from load_series before the context is touched."""
    x = _img(rows=8, cols=8)
    good = R.encode_frame(x, 16)
    three = struct.pack("<I", 3) + good[4:]                      # an RGB-like header on a 16-bit slice
    for z in range(3):
        R.write_slice(tmp_path / f"IM{z}.dcm", x, three if z == 1 else good,
                      ipp=(0, 0, 1.5 * z), instance=z + 1)
    with pytest.raises(NotImplementedError, match="IM1.dcm: RLE frame of 3 segments"):
        dicom.load_series(tmp_path, ctx=object())                # (a context that would fail if it were used)
    backwards = good[:8] + struct.pack("<I", 64) + good[12:]
    R.write_slice(tmp_path / "IM1.dcm", x, backwards, ipp=(0, 0, 1.5), instance=2)
    with pytest.raises(DicomError, match="IM1.dcm: RLE segment offsets are not increasing"):
        dicom.load_series(tmp_path, ctx=object())
