"""CPU: the JPEG-LS (ITU-T T.87) host side -- tests/jls_model.py and tests/jls_writer.py against CharLS's streams
(tests/golden/jls) and against each other, `dicom.read_file` on JPEG-LS files, the refusals of `jpeg_ls.parse_frame`, and that a
refusal raises from `load_series` before the device is touched."""
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN
import jls_model as M
import jls_writer as W
from boa_hip import dicom, jpeg_ls as JL
from boa_hip.dicom import DicomError
from boa_hip.jpeg_lossless import CompressedFrame

GPU_SHAPES = ((1, 1), (1, 300), (300, 1), (5, 63), (5, 64), (5, 65), (97, 129))


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "jls", "charls.npz"))
    return {k[7:]: dict(stream=g["stream_" + k[7:]].tobytes(), source=g["source_" + k[7:]], decoded=g["decoded_" + k[7:]],
                        params=g["params_" + k[7:]].tolist()) for k in g.files if k.startswith("stream_")}


@pytest.fixture(scope="module")
def phantom():
    generate = W.golden_generator()
    vol = generate.phantom_slices()
    return [(np.load(os.path.join(GOLDEN, "jls", f"charls_phantom{i}.npz"))["stream_phantom"].tobytes(), vol[z])
            for i, z in enumerate(generate.PHANTOM_Z)]


def _ct_like(shape, bits, seed):
    rng = np.random.default_rng(seed)
    rows, cols = shape
    yy, xx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    body = ((yy - rows / 2) ** 2 / max(rows * 0.4, 1) ** 2 + (xx - cols / 2) ** 2 / max(cols * 0.4, 1) ** 2) < 1
    v = np.where(body, 1064 + rng.integers(-200, 201, shape), 24)
    return (v << (bits - 12) if bits >= 12 else v >> (12 - bits)).astype(np.int64)


def test_golden_set_is_what_the_tests_need(golden):
    assert set(golden) == {"h3", "lse", "noise16"} | {f"ct{b}_{r}x{c}_near{n}" for r, c, b in ((40, 48, 12), (33, 301, 16), (40, 48, 8))
                                                      for n in (0, 2)}
    h3 = golden["h3"]["stream"]
    assert h3[h3.index(b"\xFF\xF7"):].hex().startswith("fff7000b0800040004010111" + "00" + "ffda00080101000000" + "00"
                                                          + "c000006c80208e01c00000574000006ee6000001bc18000005d800009160ffd9")
    assert golden["lse"]["params"] == [12, 0, 4095, 9, 30, 100, 31] and b"\xFF\xF8" in golden["lse"]["stream"]
    for name, g in golden.items():
        near = g["params"][1]
        assert int(np.abs(g["decoded"].astype(int) - g["source"].astype(int)).max()) <= near
        assert (near == 0) == (g["decoded"] == g["source"]).all() or name == "h3"


def test_model_decodes_charls_streams(golden, phantom):
    for name, g in golden.items():
        px, st, _ = M.decode_stream(g["stream"])
        assert st == M.OK, name
        np.testing.assert_array_equal(px, g["decoded"], err_msg=name)
    for stream, source in phantom:
        px, st, stats = M.decode_stream(stream)
        assert st == M.OK and stats["runs"] > 100
        np.testing.assert_array_equal(px, source)


def test_writer_scan_bytes_equal_charls(golden, phantom):
    """JPEG-LS encoding is deterministic: the same source and parameters give the same scan bytes."""
    for name, g in golden.items():
        scan, rows, cols, p = M.scan_of(g["stream"])
        mine, rec = W.encode_scan(g["source"], p)
        assert mine == scan, name
        np.testing.assert_array_equal(rec, g["decoded"], err_msg=name)
        bits, near, *lse = g["params"]
        if bits > 12:
            continue                                               # (CharLS spells the defaults out in an LSE there)
        whole = W.encode(g["source"], bits, near, lse if any(lse) else None)
        assert whole[whole.index(b"\xFF\xF7"):] == g["stream"][g["stream"].index(b"\xFF\xF7"):], name
    stream, source = phantom[0]
    scan, rows, cols, p = M.scan_of(stream)
    assert W.encode_scan(source, p)[0] == scan


@pytest.mark.parametrize("bits,near", [(8, 0), (12, 0), (16, 0), (8, 3), (12, 3), (16, 3)])
def test_model_inverts_writer(bits, near):
    rng = np.random.default_rng(bits + near)
    p = M.Params((1 << bits) - 1, near)
    for shape in GPU_SHAPES:
        for img in (_ct_like(shape, bits, 5), rng.integers(0, 1 << bits, shape)):
            scan, rec = W.encode_scan(img, p)
            px, st, _ = M.decode_scan(scan, shape[0], shape[1], p)
            assert st == M.OK
            np.testing.assert_array_equal(px, rec)
            assert int(np.abs(rec.astype(int) - img).max()) <= near


def test_parse_frame_accepts_charls_spiff_streams(golden):
    for name, g in golden.items():
        bits, near, *lse = g["params"]
        assert g["stream"][2:4] == b"\xFF\xE8"                     # SPIFF in APP8
        rows, cols = g["source"].shape
        fr = JL.parse_frame(g["stream"], rows=rows, cols=cols, bits_allocated=8 if bits == 8 else 16, bits_stored=bits, name=name)
        scan, _, _, p = M.scan_of(g["stream"])
        assert bytes(fr.data) == scan and fr.precision == bits
        assert [fr.maxval, fr.near, fr.t1, fr.t2, fr.t3, fr.reset] == p.words()
        assert JL.plausible_stream(g["stream"])
    assert JL.default_thresholds(4095, 0) == (18, 67, 276) == JL.default_thresholds(65535, 0) and JL.default_thresholds(255, 0) == (3, 7, 21)


def test_build_batch_tables(golden):
    names = ["h3", "lse", "ct16_33x301_near2"]
    frames = [JL.parse_frame(golden[n]["stream"], rows=golden[n]["source"].shape[0], cols=golden[n]["source"].shape[1],
                             bits_allocated=16, bits_stored=golden[n]["params"][0], name=n) for n in names]
    data, ftab = JL.build_batch(frames)
    assert ftab.shape == (3, JL.FRAME_WORDS) and ftab.dtype == np.int32
    for f, row in zip(frames, ftab):
        assert row[0] % 4 == 0 and row[1] == 0 and row[2] == len(f.data) and row[0] + ((row[2] + 3) & ~3) <= len(data)
        assert list(row[3:9]) == [f.maxval, f.near, f.t1, f.t2, f.t3, f.reset] and not row[9:].any()
        assert bytes(data[row[0]:row[0] + row[2]]) == bytes(f.data) and not data[row[0] + row[2]:row[0] + ((row[2] + 3) & ~3)].any()


IMG = _ct_like((8, 12), 12, 1)
KW = dict(rows=8, cols=12, bits_allocated=16, bits_stored=12, name="x.dcm")


def _with(segment, before=b"\xFF\xDA", stream=None):
    s = W.encode(IMG, 12) if stream is None else stream
    i = s.index(before)
    return s[:i] + segment + s[i:]


def _refusals():
    """(stream, exception, message pattern)"""
    good = W.encode(IMG, 12)
    scan_at = good.index(b"\xFF\xDA") + 10
    lse = lambda *v: b"\xFF\xF8" + struct.pack(">HB5H", 13, 1, *v)   # noqa: E731
    N, D = NotImplementedError, DicomError
    return [
        (W.markers(8, 12, 12, components=3) + good[scan_at:], N, "x.dcm: JPEG-LS frame of 3 components"),
        (W.markers(8, 12, 12, ilv=1) + good[scan_at:], N, "x.dcm: JPEG-LS scan of 1 components, interleave mode 1"),
        (_with(b"\xFF\xF8" + struct.pack(">HB", 3 + 5, 2) + bytes(5)), N, "x.dcm: JPEG-LS LSE id 2 .mapping table specification."),
        (_with(b"\xFF\xF8" + struct.pack(">HB", 3 + 5, 3) + bytes(5)), N, "x.dcm: JPEG-LS LSE id 3 .mapping table continuation."),
        (_with(b"\xFF\xF8" + struct.pack(">HBBHH", 8, 4, 2, 8, 12)), N, "x.dcm: JPEG-LS LSE id 4 .oversize image dimensions."),
        (W.markers(8, 12, 12, table=1) + good[scan_at:], N, "x.dcm: JPEG-LS mapping table 1 selected in SOS"),
        (_with(b"\xFF\xDD" + struct.pack(">HH", 4, 4)), N, "x.dcm: JPEG-LS restart interval of 4 lines"),
        (W.markers(8, 12, 12, pt=2) + good[scan_at:], N, "x.dcm: JPEG-LS point transform 2"),
        (b"\x00\x00" + good[2:], D, "x.dcm: JPEG-LS frame does not start with SOI"),
        (good[:2] + good[good.index(b"\xFF\xDA"):], D, "x.dcm: scan before the frame header .no SOF55."),
        (good[:good.index(b"\xFF\xDA")] + b"\x00" + good[scan_at:], D, "x.dcm: expected a marker at byte .* .no SOS."),
        (good[:good.index(b"\xFF\xDA")] + b"\xFF\xD9", D, "x.dcm: EOI before any scan .no SOS."),
        (good[:-2], D, "x.dcm: JPEG-LS scan not terminated by a marker .EOI missing."),
        (good[:-2] + b"\xFF\xDA" + good[scan_at - 8:], D, "x.dcm: more than one scan"),
        (good[:-2] + b"\xFF\xDC\x00\x04\x00\x08\xFF\xD9", D, "x.dcm: DNL marker"),
        (_with(b"\xFF\xDC\x00\x04\x00\x08"), D, "x.dcm: DNL marker"),
        (good[:-2] + b"\xFF\xD0" + good[-8:], D, "x.dcm: marker FFD0 after the scan .EOI expected."),
        (good[:4] + b"\xFF\xFF", D, "x.dcm: marker segment of length 65535 overruns the frame"),
        (_with(b"\xFF\xE8\x40\x00abc"), D, "x.dcm: marker segment of length 16384 overruns the frame"),
        (W.markers(8, 13, 12) + good[scan_at:], D, "x.dcm: SOF55 size 8 x 13 differs from Rows x Columns 8 x 12"),
        (W.markers(8, 12, 11) + good[scan_at:], D, "x.dcm: SOF55 precision 11 outside BitsStored 12 .. BitsAllocated 16"),
        (W.markers(8, 12, 17) + good[scan_at:], D, "x.dcm: SOF55 precision 17"),
        (_with(b"\xFF\xC3" + good[good.index(b"\xFF\xF7") + 2:good.index(b"\xFF\xDA")], b"\xFF\xF7"), D, "x.dcm: SOF marker C3 in a JPEG-LS frame"),
        (_with(good[good.index(b"\xFF\xF7"):good.index(b"\xFF\xDA")]), D, "x.dcm: more than one frame header"),
        (W.markers(8, 12, 12)[:-5] + b"\x02" + W.markers(8, 12, 12)[-4:] + good[scan_at:], D, "x.dcm: scan component 2 is not the frame's component 1"),
        (_with(lse(4096, 0, 0, 0, 0)), D, "x.dcm: LSE MAXVAL 4096 above the 12-bit precision"),
        (W.markers(8, 12, 4, near=8) + good[scan_at:], D, "x.dcm: SOF55 precision 4 outside"),
        (_with(lse(100, 0, 0, 0, 0), stream=W.markers(8, 12, 12, near=51) + good[scan_at:]), D, "x.dcm: NEAR 51 above min.255, MAXVAL / 2. = 50"),
        (_with(lse(0, 70, 67, 0, 0)), D, "x.dcm: LSE thresholds T1 70, T2 67, T3 276 out of order"),
        (_with(lse(0, 0, 0, 5000, 0)), D, "x.dcm: LSE thresholds T1 18, T2 67, T3 5000 out of order or range"),
        (_with(lse(0, 0, 0, 0, 2)), D, "x.dcm: LSE RESET 2 outside 3 .. 4095"),
        (_with(lse(0, 0, 0, 0, 4096)), D, "x.dcm: LSE RESET 4096 outside 3 .. 4095"),
        (_with(b"\xFF\xF8" + struct.pack(">HB", 3 + 4, 1) + bytes(4)), D, "x.dcm: LSE segment id 1 of 5 bytes"),
        (_with(b"\xFF\xF8" + struct.pack(">HB", 3, 9)), D, "x.dcm: LSE segment id 9 of 1 bytes"),
        (_with(b"\xFF\xC4\x00\x02"), D, "x.dcm: unexpected marker FFC4 ahead of the scan"),
    ]


REFUSALS = _refusals()


def test_parse_frame_accepts_variants():
    good = W.encode(IMG, 12)
    ok = JL.parse_frame(good, **KW)
    assert (ok.maxval, ok.near, ok.t1, ok.t2, ok.t3, ok.reset) == (4095, 0, 18, 67, 276, 64)
    for s in (_with(b"\xFF\xFE\x00\x05abc"), _with(b"\xFF\xDD\x00\x04\x00\x00"), _with(b"\xFF\xDD\x00\x06\x00\x00\x00\x00"),
              _with(b"\xFF"), good + b"\x00", good + b"\xFF\xD9junk", _with(b"\xFF\xF8" + struct.pack(">HB5H", 13, 1, 0, 0, 0, 0, 0))):
        fr = JL.parse_frame(s, **KW)
        assert bytes(fr.data) == bytes(ok.data) and fr.t1 == 18
    lse = W.encode(IMG, 12, 0, (0, 9, 0, 100, 31))
    fr = JL.parse_frame(lse, **KW)
    assert (fr.maxval, fr.t1, fr.t2, fr.t3, fr.reset) == (4095, 9, 67, 100, 31)
    np.testing.assert_array_equal(M.decode_scan(bytes(fr.data), 8, 12, M.Params(4095, 0, 9, 67, 100, 31))[0], IMG)
    near = JL.parse_frame(W.encode(IMG, 12, 3), **KW)
    assert (near.near, near.t1, near.t2, near.t3) == (3, 27, 82, 297)


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_parse_frame_refusals(k):
    stream, exc, pattern = REFUSALS[k]
    with pytest.raises(exc, match=pattern) as info:
        JL.parse_frame(stream, **KW)
    assert (exc is DicomError) == isinstance(info.value, DicomError)


def test_refusal_precedes_device_in_load_series(tmp_path):
    """Every frame the marker parser refuses raises from load_series before the context is touched."""
    good = W.encode(IMG, 12)
    for z in (0, 2):
        W.write_slice(tmp_path / f"IM{z}.dcm", IMG, good, bits_stored=12, ipp=(0, 0, 1.5 * z), instance=z + 1)
    for stream, exc, pattern in REFUSALS:
        if not JL.plausible_stream(stream):
            continue                                               # (refused by read_file already, by the syntax's name: below)
        W.write_slice(tmp_path / "IM1.dcm", IMG, stream + b"\0" * (len(stream) % 2), bits_stored=12, ipp=(0, 0, 1.5), instance=2)
        with pytest.raises(exc, match=pattern.replace("x.dcm", "IM1.dcm")):
            dicom.load_series(tmp_path, ctx=object())              # (a context that would fail if it were used)
    assert sum(JL.plausible_stream(s) for s, _, _ in REFUSALS) >= len(REFUSALS) - 4


@pytest.mark.parametrize("fragments,bot", [(1, False), (1, True), (2, False), (3, False), (3, True)])
@pytest.mark.parametrize("near", [0, 2])
def test_read_file_returns_a_tagged_frame(tmp_path, fragments, bot, near):
    stream = W.encode(IMG, 12, near)
    stream += b"\0" * (len(stream) % 2)
    W.write_slice(tmp_path / "a.dcm", IMG, stream, bits_stored=12, near=near, ipp=(0, 0, 0), fragments=fragments, bot=bot)
    ds = dicom.read_file(tmp_path / "a.dcm")
    ts = JL.JPEG_LS_NEAR if near else JL.JPEG_LS_LOSSLESS
    assert ds["TransferSyntaxUID"] == ts
    assert isinstance(ds["PixelData"], CompressedFrame) and ds["PixelData"].transfer_syntax == ts
    assert bytes(ds["PixelData"]) == stream and ds["BitsStored"] == 12 and ds["Rows"] == 8
    fr = JL.parse_frame(ds["PixelData"], rows=8, cols=12, bits_allocated=16, bits_stored=12, name="a.dcm")
    assert fr.near == near
    assert "PixelData" not in dicom.read_file(tmp_path / "a.dcm", stop_before_pixels=True)


@pytest.mark.parametrize("ts", JL.SYNTAXES)
def test_read_file_refuses_what_does_not_start_like_jpeg_ls(tmp_path, ts):
    from ljpeg_writer import encode as encode_sof3
    good = W.encode(IMG, 12)
    sof3_first = encode_sof3(IMG, precision=12)
    for k, bad in enumerate((b"\xFF\x4F\xFF\x51" + good[4:], good[1:] + b"\0", sof3_first, b"\xFF\xD8" + good[good.index(b"\xFF\xDA"):],
                             b"\xFF\xD8")):
        W.write_slice(tmp_path / f"bad{k}.dcm", IMG, bad + b"\0" * (len(bad) % 2), bits_stored=12, ipp=(0, 0, 0), transfer_syntax=ts)
        with pytest.raises(NotImplementedError, match=f"transfer syntax {ts}: PixelData does not start like a JPEG-LS stream"):
            dicom.read_file(tmp_path / f"bad{k}.dcm")
