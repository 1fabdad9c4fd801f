"""JPEG 2000 DICOM input, host side (no device): the codestream parser and tier-2 of boa_hip/jpeg2000.py proven through the
numpy reference tier-1 / inverse 5/3 (tests/j2k_reference.py) on the committed OpenJPEG fixtures and fresh streams (lossless,
and truncated reversible ones against OpenJPEG's own decode), the midpoint rule at every pass count, tile-parts and COC / QCC, every refusal by name, malformed streams, and the transfer syntaxes read_file accepts."""
import struct

import numpy as np
import pytest

import j2k_reference as R
import j2k_writer as JW
from boa_hip import dicom, jpeg2000 as J
from boa_hip.dicom import DicomError

FIXTURES = JW.load_fixtures()


def _parse(stream, rows, cols, alloc=16, name="f.dcm"):
    return J.parse_frame(stream, rows=rows, cols=cols, bits_allocated=alloc, name=name)


def _small(name="129x97_u16_rpcl_precincts"):
    return next(f for f in FIXTURES if f["name"] == name)


def _roundtrip(stream, want, name="f.dcm"):
    fr = _parse(stream, *want.shape, name=name)
    px, ok = R.decode_frame(fr)
    assert ok, name
    np.testing.assert_array_equal(px, (np.asarray(want).astype(np.int64) & 0xFFFF).astype(np.uint16), err_msg=name)
    return fr


def _segment(marker, body):
    return struct.pack(">HH", marker, len(body) + 2) + body


def _main_header_end(stream):
    return stream.index(b"\xFF\x90")            # the first SOT


@pytest.mark.parametrize("fx", FIXTURES, ids=[f["name"] for f in FIXTURES])
def test_fixture_through_host_tier2_and_reference(fx):
    fr = _roundtrip(fx["stream"], JW.expected(fx), fx["name"])
    assert (fr.precision, fr.signed) == (fx["bits"], fx["signed"])
    assert fr.blocks[:, 6].sum() > 0
    nbp, passes = fr.blocks[:, 5], fr.blocks[:, 6]
    early = (passes > 0) & (passes < 3 * nbp - 2)
    assert early.any() == ("decoded" in fx), fx["name"]   # a truncated fixture stops blocks early, a lossless one never
    if "decoded" in fx:
        assert not np.array_equal(fx["decoded"], fx["source"]) and fx["openjpeg"]
    if "30db" in fx["name"]:
        assert (passes == 0).any()


def test_fixture_coverage():
    names = " ".join(f["name"] for f in FIXTURES)
    for want in ("lrcp", "rlcp", "rpcl", "pcrl", "cprl", "2layers", "3layers", "1res", "8res", "cb4x4", "cb16x64", "cb32",
                 "precincts", "plt_com", "jp2", "1x1", "1x37", "41x1", "40x33", "129x97", "256x256", "512x512", "_s8", "_s16",
                 "fullrange_noise", "ct_trunc_rate10", "ct_trunc_2layers_cb16", "u8_trunc_30db_3res", "s16_1res_trunc",
                 "s8_random_trunc", "trunc_rpcl_cb4x4_3layers", "1x37_u16_trunc", "41x1_u8_trunc", "u8_saturated_trunc",
                 "u16_saturated_trunc", "s16_saturated_trunc", "256x256_ct_phantom_crop_trunc_rate8"):
        assert want in names, want


def test_fresh_pillow_streams():
    if not JW.have_pillow_j2k():
        pytest.skip("Pillow with OpenJPEG does not import here")
    rng = np.random.default_rng(7)
    for k, (shape, bits, signed, kw) in enumerate([
            ((23, 58), 16, False, dict(progression="PCRL", codeblock_size=(8, 32))),
            ((64, 5), 8, True, dict(quality_layers=[30, 0], quality_mode="rates")),
            ((77, 70), 16, True, dict(progression="LRCP", num_resolutions=4, precinct_size=(16, 16), codeblock_size=(4, 16))),
            ((3, 200), 16, False, dict(progression="CPRL"))]):
        lo, hi = (-(1 << (bits - 1)), 1 << (bits - 1)) if signed else (0, 1 << bits)
        x = rng.integers(lo, hi, shape)
        s = JW.stream_of(x, bits, signed, **kw)
        np.testing.assert_array_equal(JW.openjpeg_decode(s), x)
        _roundtrip(s, x, f"fresh{k}")
    # truncated reversible streams (rate- or quality-limited layers): bit-equal to OpenJPEG's own decode
    yy, xx = np.meshgrid(np.arange(129), np.arange(129), indexing="ij")
    layer_options = [dict(quality_layers=[10], quality_mode="rates"),
                     dict(quality_layers=[40, 10], quality_mode="rates", codeblock_size=(16, 16)),
                     dict(quality_layers=[30], quality_mode="dB", num_resolutions=3),
                     dict(quality_layers=[20, 8, 4], quality_mode="rates", codeblock_size=(4, 4), progression="RPCL"),
                     dict(quality_layers=[45, 35], quality_mode="dB", codeblock_size=(64, 64)),
                     dict(quality_layers=[5], quality_mode="rates", progression="PCRL", num_resolutions=3)]
    tried = refused = lossy = 0
    for shape in ((5, 7), (23, 58), (40, 33), (97, 129)):
        for bits in (8, 16):
            full = (1 << bits) - 1
            body = np.hypot(yy[:shape[0], :shape[1]] - shape[0] / 2, xx[:shape[0], :shape[1]] - shape[1] / 2) < 0.4 * max(shape)
            contents = [np.clip(np.round(full / 64 + body * (full / 60 + rng.normal(0, full / 4000 + 1, shape))), 0, full),
                        rng.integers(0, full + 1, shape), rng.integers(0, 2, shape) * full]      # CT-like, noise, saturated
            for signed in (False, True):
                for c, u in enumerate(contents):
                    x = u.astype(np.int64) - ((1 << (bits - 1)) if signed else 0)
                    for o, kw in enumerate(layer_options):
                        name = f"trunc {shape} {bits} bits signed {signed} content {c} options {o}"
                        tried += 1
                        try:
                            s = JW.stream_of(x, bits, signed, **kw)
                        except OSError:                 # Pillow itself refuses some option sets on tiny images
                            refused += 1
                            continue
                        want = JW.openjpeg_decode(s)
                        lossy += not np.array_equal(want, x)
                        _roundtrip(s, want, name)
    print(f"truncated sweep: {tried} tried, {refused} refused by Pillow, {lossy} not lossless")
    assert tried == 288 and refused * 8 <= tried, (tried, refused)
    assert lossy * 8 >= 7 * (tried - refused), (lossy, tried, refused)     # the sweep is about truncation: most are lossy


def test_every_pass_count_keeps_the_decoded_bits_and_holds_the_midpoint():
    """No OpenJPEG here: every block of a lossless fixture decoded with its first P passes, P = 0 .. its own count.  Where a
    coefficient was coded down to plane b_last, the bits at and above b_last are those of the full decode, and the bits below
    are the midpoint 2^(b_last - 1) (nothing for b_last = 0); the full count gives the full decode."""
    fx = _small("40x33_u8_lrcp_2layers")
    fr = _parse(fx["stream"], *fx["source"].shape)
    off = 0
    seen = set()
    for o, x0, y0, w, h, nbp, own, ln in fr.blocks.tolist():
        assert own == 3 * nbp - 2 or own == 0
        full, last_full, ok = R.decode_block(fr.data, off, ln, w, h, o, nbp, own, with_last=True)
        assert ok and ((last_full == 0) == (full != 0)).all() and ((last_full == -1) == (full == 0)).all()
        for P in range(own + 1):
            v, last, ok = R.decode_block(fr.data, off, ln, w, h, o, nbp, P, with_last=True)
            assert ok
            if P == own:
                np.testing.assert_array_equal(v, full)
                continue
            if P == 0:
                assert not v.any()
                continue
            kind, bf = (2 if P == 1 else (P - 2) % 3), nbp - 1 - (P + 1) // 3
            seen.add((kind, bf >= 1))
            sig = last >= 0
            assert not v[~sig].any()
            assert sig[np.abs(full) >> (bf + 1) != 0].all()            # significant above plane bf: coded by now
            assert ((last[sig] == bf) | ((last[sig] == bf + 1) & (kind == 0))).all()
            b, m, mf = last[sig], np.abs(v[sig]), np.abs(full[sig])
            np.testing.assert_array_equal(np.sign(v[sig]), np.sign(full[sig]))
            np.testing.assert_array_equal(m >> b, mf >> b)
            np.testing.assert_array_equal(m & ((1 << b) - 1), np.where(b >= 1, 1 << np.maximum(b - 1, 0), 0))
        off += ln
    assert seen == {(k, hi) for k in (0, 1, 2) for hi in (False, True)} - {(2, False)}


def _split_tile_parts(stream, cut, last_psot_zero=False):
    """The one tile-part of `stream` as two: data [0, cut) and [cut, end); the second with Psot = 0 if asked."""
    sot = stream.index(b"\xFF\x90")
    psot = struct.unpack(">I", stream[sot + 6:sot + 10])[0]
    sod = stream.index(b"\xFF\x93", sot) + 2
    head, data = stream[sot:sod], stream[sod:sot + psot]
    a, b = data[:cut], data[cut:]
    tp0 = bytearray(head)
    tp0[6:10] = struct.pack(">I", len(head) + len(a))
    tp0[11] = 2
    tp1 = bytearray(_segment(0xFF90, struct.pack(">HIBB", 0, 0, 1, 2)) + b"\xFF\x93")
    tp1[6:10] = struct.pack(">I", 0 if last_psot_zero else len(tp1) + len(b))
    return stream[:sot] + bytes(tp0) + a + bytes(tp1) + b + stream[sot + psot:]


def test_tile_parts_concatenated():
    fx = _small()
    for cut in (0, 1, 100, 5000):
        for zero in (False, True):
            _roundtrip(_split_tile_parts(fx["stream"], cut, zero), fx["source"])


def test_coc_and_qcc_override_cod_and_qcd():
    fx = _small()
    s = fx["stream"]
    i = s.index(b"\xFF\x52")
    ln = struct.unpack(">H", s[i + 2:i + 4])[0]
    cod = s[i + 4:i + 2 + ln]
    sp = cod[5:]                                        # SPcod: levels, code-block size, style, transform, precincts
    wrong = bytearray(cod)
    wrong[6] = wrong[7] = 0                             # 4 x 4 code blocks in COD: only COC's sizes decode the stream
    q = s.index(b"\xFF\x5C")
    qln = struct.unpack(">H", s[q + 2:q + 4])[0]
    qcd = s[q + 4:q + 2 + qln]
    s2 = s[:i + 4] + bytes(wrong) + s[i + 2 + ln:]
    s2 = JW.patch_exponents(s2, 20)
    end = _main_header_end(s2)
    _roundtrip(s2[:end] + _segment(0xFF53, bytes([0, cod[0] & 1]) + sp) + _segment(0xFF5D, bytes([0]) + qcd) + s2[end:],
               fx["source"])
    try:                                                # without the COC / QCC the stream does not decode to its source
        px, ok = R.decode_frame(_parse(s2, *fx["source"].shape))
        assert not (ok and np.array_equal(px, JW.expected(fx)))
    except DicomError:
        pass


def _cod_offset(s):
    return s.index(b"\xFF\x52") + 4


REFUSALS = [  # (what, patch(stream) -> stream, exception, message)
    ("9/7", lambda s: _setb(s, _cod_offset(s) + 9, 0), NotImplementedError, "lossy JPEG 2000 is not read"),
    ("quant derived", lambda s: _setb(s, s.index(b"\xFF\x5C") + 4, (2 << 5) | 1), NotImplementedError, "scalar quantisation"),
    ("quant expounded", lambda s: _setb(s, s.index(b"\xFF\x5C") + 4, (2 << 5) | 2), NotImplementedError, "scalar quantisation"),
    ("tiles", lambda s: _set32(s, s.index(b"\xFF\x51") + 4 + 18, 32), NotImplementedError, "several tiles"),
    ("origin", lambda s: _set32(s, s.index(b"\xFF\x51") + 4 + 10, 1), NotImplementedError, "origin"),
    ("tile origin", lambda s: _set32(s, s.index(b"\xFF\x51") + 4 + 26, 1), NotImplementedError, "origin"),
    ("sub-sampling", lambda s: _setb(s, s.index(b"\xFF\x51") + 4 + 37, 2), NotImplementedError, "sub-sampling"),
    ("components", lambda s: _setb(s, s.index(b"\xFF\x51") + 4 + 35, 3), NotImplementedError, "3 image components"),
    ("mct", lambda s: _setb(s, _cod_offset(s) + 4, 1), NotImplementedError, "MCT"),
    ("sop", lambda s: _setb(s, _cod_offset(s), s[_cod_offset(s)] | 2), NotImplementedError, "SOP"),
    ("eph", lambda s: _setb(s, _cod_offset(s), s[_cod_offset(s)] | 4), NotImplementedError, "EPH"),
    ("poc", lambda s: _insert_main(s, _segment(0xFF5F, bytes([0, 0, 0, 1, 6, 0, 1]))), NotImplementedError, "POC"),
    ("ppm", lambda s: _insert_main(s, _segment(0xFF60, bytes(5))), NotImplementedError, "PPM"),
    ("rgn", lambda s: _insert_main(s, _segment(0xFF5E, bytes([0, 0, 3]))), NotImplementedError, "RGN"),
    ("ppt", lambda s: _insert_tile(s, _segment(0xFF61, bytes(5))), NotImplementedError, "PPT"),
] + [(name, (lambda bit: lambda s: _setb(s, _cod_offset(s) + 8, bit))(bit), NotImplementedError, name)
     for bit, name in ((1, "BYPASS"), (2, "RESET"), (4, "TERMALL"), (8, "VCAUSAL"), (16, "PTERM"), (32, "SEGSYM"))]


def _setb(s, i, v):
    return s[:i] + bytes([v]) + s[i + 1:]


def _set32(s, i, v):
    return s[:i] + struct.pack(">I", v) + s[i + 4:]


def _insert_main(s, seg):
    e = _main_header_end(s)
    return s[:e] + seg + s[e:]


def _insert_tile(s, seg):
    sot = s.index(b"\xFF\x90")
    psot = struct.unpack(">I", s[sot + 6:sot + 10])[0]
    s = _set32(s, sot + 6, psot + len(seg))
    return s[:sot + 12] + seg + s[sot + 12:]


@pytest.mark.parametrize("what,patch,exc,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_by_name(what, patch, exc, msg):
    fx = _small()
    with pytest.raises(exc, match=msg):
        _parse(patch(fx["stream"]), *fx["source"].shape, name="refused.dcm")


def test_refusal_precedes_device_in_load_series(tmp_path):
    fx = _small()
    bad = REFUSALS[0][1](fx["stream"])
    stored = np.stack([fx["source"]] * 3)
    JW.write_series(tmp_path, stored, [fx["stream"], bad, fx["stream"]])
    with pytest.raises(NotImplementedError, match="lossy JPEG 2000"):
        dicom.load_series(tmp_path, ctx=object())       # (a context that would fail if it were used)


def test_inconsistent_headers_are_dicom_errors():
    fx = _small()
    s, (h, w) = fx["stream"], fx["source"].shape
    with pytest.raises(DicomError, match="differs from Rows x Columns"):
        _parse(s, h + 1, w)
    with pytest.raises(DicomError, match="above BitsAllocated 8"):
        _parse(s, h, w, alloc=8)
    with pytest.raises(DicomError, match="SOC"):
        _parse(b"\xFF\xD8" + s[2:], h, w)


def test_truncated_and_corrupted_streams_name_the_file():
    rng = np.random.default_rng(3)
    for fx in (_small(), _small("40x33_u16_rlcp_cb4x4"), _small("40x33_u16_jp2")):
        s, shape = fx["stream"], fx["source"].shape
        cuts = sorted(set(rng.integers(0, len(s), 60).tolist()) | set(range(0, 200, 3)))
        for n in cuts:
            try:
                _parse(s[:n], *shape, name="trunc.dcm")
            except DicomError as e:
                assert "trunc.dcm" in str(e)
        for k in range(150):
            b = bytearray(s)
            for i in rng.integers(0, min(len(s), 400 if k % 2 else len(s)), 1 + k % 4):
                b[i] = int(rng.integers(0, 256))
            try:
                fr = _parse(bytes(b), *shape, name="corrupt.dcm")
            except (DicomError, NotImplementedError) as e:
                assert "corrupt.dcm" in str(e)
            else:                                       # the table stays inside the frame and its data
                bl = fr.blocks
                assert (bl[:, 1] + bl[:, 3] <= shape[1]).all() and (bl[:, 2] + bl[:, 4] <= shape[0]).all()
                assert bl[:, 7].sum() == len(fr.data)


def test_build_batch_tables():
    fx = [_small(), _small("1x1_u8")]
    frames = [_parse(f["stream"], *f["source"].shape) for f in fx]
    data, ftab, btab = J.build_batch(frames)
    assert ftab.shape == (2, J.FRAME_WORDS) and btab.shape == (sum(len(f.blocks) for f in frames), J.BLOCK_WORDS)
    assert ftab[1, 0] == 129 * 97 and ftab[1, 7] == len(frames[0].blocks) and ftab[1, 8] == 1
    assert btab[:, 8].max() + btab[btab[:, 8].argmax(), 10] <= len(data)
    np.testing.assert_array_equal(btab[:, 0], np.repeat([0, 1], [len(f.blocks) for f in frames]))


@pytest.mark.parametrize("ts", [JW.J2K_LOSSLESS, JW.J2K])
def test_read_file_accepts_j2k(tmp_path, ts):
    fx = _small()
    JW.write_slice(tmp_path / "a.dcm", fx["source"], fx["stream"], transfer_syntax=ts, ipp=(0, 0, 0), fragments=3, bot=True)
    ds = dicom.read_file(tmp_path / "a.dcm")
    assert ds["TransferSyntaxUID"] == ts and ds["PixelData"].transfer_syntax == ts
    assert bytes(ds["PixelData"]).startswith(fx["stream"])
    _roundtrip(ds["PixelData"], fx["source"])


@pytest.mark.parametrize("ts", ["1.2.840.10008.1.2.4.80", "1.2.840.10008.1.2.4.81", "1.2.840.10008.1.2.4.50",
                                "1.2.840.10008.1.2.5", "1.2.840.10008.1.2.4.92"])
def test_other_compressed_syntaxes_still_refused(tmp_path, ts):
    fx = _small()
    JW.write_slice(tmp_path / "a.dcm", fx["source"], fx["stream"], transfer_syntax=ts, ipp=(0, 0, 0))
    with pytest.raises(NotImplementedError, match=f"transfer syntax {ts}"):
        dicom.read_file(tmp_path / "a.dcm")
