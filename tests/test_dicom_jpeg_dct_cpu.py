"""Sequential DCT JPEG (transfer syntaxes .50 / .51), host side: the numpy model of tests/jpeg_dct_model.py against libjpeg-turbo's
pixels at P = 8 and P = 12 (the committed fixtures of tests/golden/jpeg_dct, and, where Pillow's bundled libjpeg-turbo imports,
fresh streams), the test encoder of tests/jpeg_dct_writer.py against libjpeg-turbo's decode, and boa_hip.jpeg_dct's parser: what it
accepts, every refusal by name, and the tables it builds for the device."""
import hashlib
import importlib.util
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import jpeg_dct_model as M
import jpeg_dct_writer as W
import ljpeg_writer as LW
from boa_hip import dicom, jpeg_dct as J
from boa_hip.dicom import DicomError
from dicom_writer import write_slice


def _fixture_tools():
    spec = importlib.util.spec_from_file_location("jpeg_dct_make_fixtures", os.path.join(W.FIXTURES, "make_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FX = _fixture_tools()


def _have_libjpeg12():
    """The library is probed in a child process: on a layout other than the one make_fixtures.py assumes, libjpeg's error exit
    ends the process that called it."""
    try:
        import PIL.Image  # noqa: F401
    except Exception:
        return False
    if FX.lib12() is None:
        return False
    return subprocess.run([sys.executable, os.path.join(W.FIXTURES, "make_fixtures.py"), "--probe"], capture_output=True).returncode == 0


needs_libjpeg = pytest.mark.skipif(not _have_libjpeg12(), reason="Pillow with libjpeg-turbo 3.x (12-bit entry points) not importable")


def test_model_equals_libjpeg_on_every_fixture():
    seen = set()
    for which in ("p8", "p12"):
        for name, (stream, want) in W.fixtures(which).items():
            p = M.parse(stream)
            px, st = M.decode(stream)
            assert st == M.OK, name
            np.testing.assert_array_equal(px, want, err_msg=f"{which} {name}")
            seen.add((p["sof"], p["P"], int(p["qt"].max()) > 255))
    assert seen >= {(0xC0, 8, False), (0xC1, 12, False), (0xC1, 12, True)}
    assert W.fixtures("p8")["optimize_q85"][0] != W.fixtures("p8")["64x64_q75"][0]
    assert M.parse(W.fixtures("p8")["optimize_q85"][0])["ac"] != W.fixture_tables()[1]     # custom Huffman tables
    for name, (stream, want) in list(W.fixtures("p8").items()) + list(W.fixtures("p12").items()):
        if name.startswith("noise"):                                                        # both ends of the range limit
            assert want.min() == 0 and want.max() == (1 << M.parse(stream)["P"]) - 1


def test_model_equals_libjpeg_on_the_phantom_slices():
    g = np.load(os.path.join(W.FIXTURES, "phantom12.npz"))
    for name in g["names"]:
        px, st = M.decode(g["stream_" + str(name)].tobytes())
        assert st == M.OK and px.shape == (512, 512)
        assert hashlib.sha256(px.astype("<u2").tobytes()).hexdigest() == str(g["sha256_" + str(name)])


@needs_libjpeg
@pytest.mark.parametrize("P", [8, 12])
def test_model_equals_libjpeg_fresh_sweep(P):
    rng = np.random.default_rng(P)
    for shape in ((8, 8), (1, 1), (17, 9), (40, 64)):
        for q in (10, 50, 75, 95, 100):
            for x in (FX.smooth(shape, P, q), rng.integers(0, 1 << P, shape), rng.integers(0, 2, shape) * ((1 << P) - 1)):
                if P == 8:
                    stream = FX.encode8(x, quality=q)
                    want = FX.decode8(stream)
                else:
                    stream = FX.encode12(x.astype(np.uint16), q)
                    want = FX.decode12(stream, *shape)
                px, st = M.decode(stream)
                assert st == M.OK
                np.testing.assert_array_equal(px, want, err_msg=f"P {P} {shape} q {q}")


def _libjpeg(stream, P, shape):
    return FX.decode8(stream) if P == 8 else FX.decode12(stream, *shape)


@needs_libjpeg
@pytest.mark.parametrize("P", [8, 12])
def test_libjpeg_decodes_the_writers_streams_to_the_models_pixels(P):
    rng = np.random.default_rng(40 + P)
    rows, cols = 21, 43                                  # 3 x 6 blocks
    nb = 18
    qt = rng.integers(1, 40, 64)
    for ri in (0, 1, 7, 6, 100):                         # none, every block, odd, one block row, more than all blocks
        coef = W.random_coefficients(rng, nb, P)
        stream = W.encode(coef, rows=rows, cols=cols, P=P, qt=qt, ri=ri, optimal=(P == 12))
        got_coef, st = M.decode_coefficients(M.parse(stream))
        assert st == M.OK
        np.testing.assert_array_equal(got_coef, coef)
        want = M.pixels(coef, qt, P, rows, cols)
        np.testing.assert_array_equal(_libjpeg(stream, P, (rows, cols)), want, err_msg=f"Ri {ri}")
    # 16-bit quantisation table, the fixture's own Huffman tables, a non-zero 64th coefficient, ZRL chains
    coef = np.zeros((nb, 64), dtype=np.int64)
    coef[:, 0] = rng.integers(-20, 20, nb)
    coef[::2, 63] = 1
    coef[1::3, 40] = -2
    qt16 = np.full(64, 300)
    qt16[0] = 16
    stream = W.encode(coef, rows=rows, cols=cols, P=P, qt=qt16, qbits=16, sof=0xC1)
    np.testing.assert_array_equal(_libjpeg(stream, P, (rows, cols)), M.pixels(coef, qt16, P, rows, cols))


def _good(P=12, rows=16, cols=24, **kw):
    rng = np.random.default_rng(1)
    nb = -(-rows // 8) * -(-cols // 8)
    kw.setdefault("optimal", True)
    return W.encode(W.random_coefficients(rng, nb, P), rows=rows, cols=cols, P=P, **kw)


def _parse(stream, rows=16, cols=24, bits_stored=12, **kw):
    return J.parse_frame(stream, rows=rows, cols=cols, name="x.dcm", bits_stored=bits_stored, **kw)


def _with_sof(stream, marker):
    i = stream.index(b"\xFF\xC1")
    return stream[:i + 1] + bytes([marker]) + stream[i + 2:]


def test_parse_frame_accepts():
    fr = _parse(_good(), bits_stored=12)
    assert (fr.rows, fr.cols, fr.precision, fr.restart, fr.n_blocks) == (16, 24, 12, 0, 6)
    assert _parse(_good(ri=4)).restart == 4 and len(_parse(_good(ri=4)).seg_bounds) == 3
    assert _parse(_good(ri=6)).restart == 0 and _parse(_good(ri=1)).restart == 1
    assert _parse(_good(P=8), bits_stored=8).precision == 8
    assert _parse(_good(P=8, sof=0xC1), bits_stored=8).precision == 8
    s = _good()
    i = s.index(b"\xFF\xDB")
    _parse(s[:i] + b"\xFF\xFE\x00\x05abc" + b"\xFF\xE1\x00\x04hi" + s[i:])        # COM and APPn ahead of the tables
    for name, (stream, want) in W.fixtures("p12").items():
        fr = J.parse_frame(stream, rows=want.shape[0], cols=want.shape[1], bits_stored=12, name=name)
        np.testing.assert_array_equal(np.frombuffer(fr.qtable, dtype="<u2"), M.parse(stream)["qt"])


@pytest.mark.parametrize("marker,what", [(0xC2, "progressive DCT"), (0xC3, "lossless"), (0xC5, "differential sequential"),
                                         (0xC9, "arithmetic"), (0xCA, "progressive DCT \\(arithmetic"), (0xF7, "JPEG-LS")])
def test_parse_frame_refuses_other_processes_by_name(marker, what):
    with pytest.raises(NotImplementedError, match=what):
        _parse(_with_sof(_good(), marker))


def test_parse_frame_refuses_components_and_scans_by_name():
    s = _good()
    i = s.index(b"\xFF\xC1")
    three = s[:i] + b"\xFF\xC1" + struct.pack(">HBHHB", 17, 12, 16, 24, 3) + bytes([1, 0x11, 0, 2, 0x11, 0, 3, 0x11, 0]) + s[i + 13:]
    with pytest.raises(NotImplementedError, match="3 components"):
        _parse(three)
    j = s.index(b"\xFF\xDA")
    two = s[:-2] + s[j:]                                                          # a second SOS where EOI is expected
    with pytest.raises(NotImplementedError, match="more than one scan"):
        _parse(two)


def test_parse_frame_malformed_names_the_file():
    s = _good()
    i, j = s.index(b"\xFF\xC1"), s.index(b"\xFF\xDA")
    cases = {
        "no SOI": b"\x00\x00" + s[2:],
        "DNL": s[:-2] + b"\xFF\xDC\x00\x04\x00\x10\xFF\xD9",
        "DNL ahead": s[:j] + b"\xFF\xDC\x00\x04\x00\x10" + s[j:],
        "size": s[:i + 5] + struct.pack(">HH", 16, 32) + s[i + 9:],
        "zero lines": s[:i + 5] + struct.pack(">HH", 0, 24) + s[i + 9:],
        "precision": s[:i + 4] + b"\x10" + s[i + 5:],
        "sampling": s[:i + 11] + b"\x22" + s[i + 12:],
        "progressive scan": s[:j + 7] + bytes([0, 5, 0]) + s[j + 10:],
        "successive approximation": s[:j + 9] + b"\x01" + s[j + 10:],
        "no quantisation table": s[:2] + s[i:],
        "no EOI": s[:-2],
        "undefined table": s[:j + 6] + b"\x33" + s[j + 7:],
        "cut header": s[:i + 6],
        "no frame header": s[:i] + s[i + 13:],
    }
    for what, bad in cases.items():
        with pytest.raises(DicomError, match="x.dcm"):
            _parse(bad)
        assert not isinstance(_try(bad), NotImplementedError), what
    with pytest.raises(DicomError, match="precision 12 outside BitsStored 16"):
        _parse(s, bits_stored=16)
    with pytest.raises(DicomError, match="precision 12"):
        _parse(_with_sof(s, 0xC0))                                               # baseline is 8-bit
    with pytest.raises(DicomError, match="restart intervals"):
        _parse(_good(ri=2).replace(b"\xFF\xDD\x00\x04\x00\x02", b"\xFF\xDD\x00\x04\x00\x03"))
    # an AC table with an EOBn symbol, a DC table with SSSS 16
    dc, ac = W.fixture_tables()
    s8 = _good(P=8, optimal=False)
    assert bytes(ac[0]) + ac[1] in s8 and bytes(dc[0]) + dc[1] in s8
    with pytest.raises(DicomError, match="EOBn"):
        _parse(s8.replace(bytes(ac[0]) + ac[1], bytes(ac[0]) + ac[1].replace(b"\x11", b"\x20")), bits_stored=8)
    with pytest.raises(DicomError, match="SSSS values above 15"):
        _parse(s8.replace(bytes(dc[0]) + dc[1], bytes(dc[0]) + dc[1].replace(b"\x0B", b"\x10")), bits_stored=8)


def _try(stream):
    try:
        _parse(stream)
    except Exception as e:          # noqa: BLE001
        return e
    return None


def test_read_file_accepts_both_syntaxes_and_still_refuses_what_is_not_dct(tmp_path):
    x = np.zeros((16, 24))
    for ts, P in ((W.JPEG_BASELINE, 8), (W.JPEG_EXTENDED, 12), (W.JPEG_EXTENDED, 8)):
        stream = _good(P=P)
        LW.write_compressed_slice(tmp_path / "a.dcm", x, stream, transfer_syntax=ts, ipp=(0, 0, 0), bits_stored=P)
        ds = dicom.read_file(tmp_path / "a.dcm")
        assert ds["TransferSyntaxUID"] == ts and ds["PixelData"].transfer_syntax == ts
        assert bytes(ds["PixelData"]).startswith(stream)
        assert dicom._CODECS[ts] is J
    for ts in J.SYNTAXES:
        write_slice(tmp_path / "n.dcm", x, ipp=(0, 0, 0), transfer_syntax=ts)                     # native PixelData
        with pytest.raises(NotImplementedError, match=f"transfer syntax {ts}"):
            dicom.read_file(tmp_path / "n.dcm")
        for other in (LW.encode(np.zeros((16, 24), dtype=np.int64), precision=12), _with_sof(_good(), 0xC2), b"\xFF\x4F\xFF\x51" + bytes(40)):
            LW.write_compressed_slice(tmp_path / "o.dcm", x, other, transfer_syntax=ts, ipp=(0, 0, 0))
            with pytest.raises(NotImplementedError, match=f"transfer syntax {ts}"):
                dicom.read_file(tmp_path / "o.dcm")
    assert J.plausible_stream(_good()) and not J.plausible_stream(b"") and not J.plausible_stream(b"\xFF\xD8\xFF")


def test_load_series_refusal_precedes_any_touch_of_the_context(tmp_path):
    x = np.zeros((16, 24))
    good = _good()
    j = good.index(b"\xFF\xDA")
    two_scans = good[:-2] + good[j:]
    for z in range(3):
        LW.write_compressed_slice(tmp_path / f"IM{z}.dcm", x, two_scans if z == 2 else good, transfer_syntax=W.JPEG_EXTENDED,
                                  ipp=(0, 0, 1.5 * z), instance=z + 1, bits_stored=12)
    with pytest.raises(NotImplementedError, match="more than one scan"):
        dicom.load_series(tmp_path, ctx=object())


def test_build_batch_tables_are_self_consistent():
    f8 = W.fixtures("p8")
    frames = [J.parse_frame(s, rows=w.shape[0], cols=w.shape[1], bits_stored=8, name=n) for n, (s, w) in f8.items()
              if w.shape == (40, 48)]
    frames += [_parse(_good(rows=40, cols=48, ri=ri), rows=40, cols=48) for ri in (0, 1, 7, 6)]
    data, ftab, segs, subs, tabs, qt = J.build_batch(frames, subseq_bytes=16)
    assert ftab.shape == (len(frames), J.FRAME_WORDS) and tabs.shape[1] == 384 and qt.shape[1] == 64 and qt.dtype == np.uint16
    assert len(data) % 4 == 0
    for f, fr in enumerate(frames):
        off, ln, P, ri, dc, ac, q, s0, ns, b0, nb = (int(v) for v in ftab[f, [0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]])
        assert off % 4 == 0 and bytes(data[off:off + ln]) == fr.data.tobytes() and (P, ri) == (fr.precision, fr.restart)
        np.testing.assert_array_equal(tabs[dc], J.expand_table(*fr.dc))
        np.testing.assert_array_equal(tabs[ac], J.expand_table(*fr.ac))
        np.testing.assert_array_equal(qt[q], np.frombuffer(fr.qtable, dtype="<u2"))
        R = ri or fr.n_blocks
        assert ns == -(-fr.n_blocks // R) == len(fr.seg_bounds) - 1
        i = b0
        for k in range(ns):
            lo, hi, first_block, first_sub = (int(v) for v in segs[s0 + k])
            assert (lo, hi, first_block, first_sub) == (fr.seg_bounds[k], fr.seg_bounds[k + 1], k * R, i)
            starts = []
            while i < b0 + nb and subs[i, 1] == s0 + k:
                starts.append(int(subs[i, 0]))
                i += 1
            assert starts == list(range(lo, max(hi, lo + 1), 16))
        assert i == b0 + nb
    with pytest.raises(ValueError):
        J.build_batch(frames, subseq_bytes=2)
