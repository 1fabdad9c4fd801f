"""Irreversible (9/7) JPEG 2000 DICOM input, host side (no device): the parser's quantisation tables and the pairing of transform
and quantisation style of boa_hip/jpeg2000.py, and the numpy float32 model of the decoder's arithmetic (tests/j2k97_reference.py)
against OpenJPEG's own decode, bit for bit: on the committed fixtures of tests/golden/j2k97 and, where Pillow imports, on a fresh
sweep of rates, dB layers, progressions, block sizes and resolutions."""
import struct

import numpy as np
import pytest

import j2k97_fixtures as FX
import j2k97_reference as M
import j2k_writer as JW
from boa_hip import dicom, jpeg2000 as J
from boa_hip.dicom import DicomError

FIXTURES = FX.load_fixtures()
REVERSIBLE = {f["name"]: f for f in JW.load_fixtures()}


def _fx(name):
    return next(f for f in FIXTURES if f["name"] == name)


def _qcd(stream):
    """(position of the QCD marker, Sqcd, the bytes after Sqcd)"""
    i = stream.index(b"\xFF\x5C")
    ln = struct.unpack(">H", stream[i + 2:i + 4])[0]
    return i, stream[i + 4], stream[i + 5:i + 2 + ln]


def _with_qcd(stream, sqcd, body):
    i, _, old = _qcd(stream)
    return stream[:i] + struct.pack(">HHB", 0xFF5C, 3 + len(body), sqcd) + body + stream[i + 5 + len(old):]


def _setb(s, i, v):
    return s[:i] + bytes([v]) + s[i + 1:]


def _transform_pos(s):
    return s.index(b"\xFF\x52") + 4 + 9


def test_fixture_coverage():
    names = " ".join(f["name"] for f in FIXTURES)
    for want in ("2x2_u16_1level", "40x33_u8_lrcp_2layers", "40x33_s8", "61x75_u16_noise", "rate10_rpcl_precincts_cb32",
                 "rate10_3res_cb16", "_1res", "checkerboard_rate20", "512x512_ct_phantom_z0", "512x512_ct_phantom_z1"):
        assert want in names, want
    for f in FIXTURES:
        assert f["openjpeg"] and f["decoded"].shape == (f["rows"], f["cols"])
    cb = _fx("40x33_u16_checkerboard_rate20")
    assert cb["decoded"].min() == 0 and cb["decoded"].max() == 65535


@pytest.mark.parametrize("fx", FIXTURES, ids=[f["name"] for f in FIXTURES])
def test_model_equals_openjpeg_on_fixture(fx):
    fr = FX.parse(fx)
    assert (fr.transform, fr.precision, fr.signed) == (0, fx["bits"], fx["signed"])
    assert fr.levels == fx["options"].get("num_resolutions", 6) - 1
    px, _ = FX.model(fx)
    np.testing.assert_array_equal(px, FX.expected(fx), err_msg=fx["name"])


def test_model_equals_openjpeg_on_a_fresh_sweep():
    if not JW.have_pillow_j2k():
        pytest.skip("Pillow with OpenJPEG does not import here")
    rng = np.random.default_rng(5)
    options = [{}, dict(quality_layers=[10], quality_mode="rates"), dict(quality_layers=[45, 35], quality_mode="dB"),
               dict(quality_layers=[40, 8], quality_mode="rates", progression="RLCP", codeblock_size=(16, 16)),
               dict(num_resolutions=2, progression="PCRL", codeblock_size=(4, 64)), dict(num_resolutions=1),
               dict(progression="RPCL", precinct_size=(32, 32), codeblock_size=(8, 8), quality_layers=[20], quality_mode="rates"),
               dict(progression="CPRL", num_resolutions=4, quality_layers=[30], quality_mode="dB")]
    tried = refused = 0
    for shape in ((2, 2), (5, 7), (23, 58), (64, 37)):
        yy, xx = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        for bits in (8, 16):
            full = (1 << bits) - 1
            contents = [np.round(full * (0.5 + 0.4 * np.sin(xx / 5.0) * np.cos(yy / 7.0))), rng.integers(0, full + 1, shape),
                        ((yy // 2 + xx // 2) & 1) * full]
            for c, u in enumerate(contents):
                for signed in (False, True):
                    x = u.astype(np.int64) - ((1 << (bits - 1)) if signed else 0)
                    for o, kw in enumerate(options):
                        name = f"{shape} {bits} bits signed {signed} content {c} options {o}"
                        tried += 1
                        try:
                            s = FX.stream_of(x, bits, signed, **kw)
                        except OSError:                 # Pillow itself refuses some option sets on tiny images
                            refused += 1
                            continue
                        fr = J.parse_frame(s, rows=shape[0], cols=shape[1], name=name)
                        assert fr.transform == 0 and fr.signed == signed
                        px, ok = M.decode_frame(fr)
                        assert ok, name
                        np.testing.assert_array_equal(px, (JW.openjpeg_decode(s) & 0xFFFF).astype(np.uint16), err_msg=name)
    print(f"9/7 sweep: {tried} tried, {refused} refused by Pillow")
    assert tried == 384 and refused * 8 <= tried, (tried, refused)


@pytest.mark.parametrize("name", ["61x75_u16_noise", "40x33_s8_random", "129x97_u16_ct_rate10_3res_cb16", "40x33_u16_1res"])
def test_expounded_step_table(name):
    """Sqcd style 2: one 16-bit eps << 11 | mu per subband; step_b = (1 + mu / 2048) 2^(P - eps) and M_b = G + eps - 1."""
    fx = _fx(name)
    fr = FX.parse(fx)
    _, sqcd, body = _qcd(fx["stream"])
    assert sqcd & 31 == 2 and len(body) == 2 * (3 * fr.levels + 1)
    vals = struct.unpack(f">{len(body) // 2}H", body)
    assert fr.steps.dtype == np.float32 and len(fr.steps) == len(fr.band_mb) == 3 * fr.levels + 1
    for b, v in enumerate(vals):
        eps, mu = v >> 11, v & 0x7FF
        assert fr.band_mb[b] == (sqcd >> 5) + eps - 1
        assert float(fr.steps[b]) == (2048 + mu) * 2.0 ** (fx["bits"] - eps - 11)     # (exact in float32 and in float64)
    # every block knows its subband: orientation and resolution agree with the table's order
    for (o, x0, y0, *_), sb in zip(fr.blocks.tolist(), fr.band.tolist()):
        assert (sb == 0) == (o == 0) and (o == 0 or (sb - 1) % 3 + 1 == o)
    data, ftab, btab = J.build_batch([fr])
    assert ftab[0, 9] == 0
    np.testing.assert_array_equal(btab[:, 11].view(np.float32), np.float32(0.5) * fr.steps[fr.band])


def test_derived_step_table():
    """Sqcd style 1 (T.800 E-5): eps_b = eps_0 for LL and resolution 1, eps_0 - (r - 1) from resolution 2 on; mu_b = mu_0."""
    fx = _fx("129x97_u16_ct_rate10_3res_cb16")
    sqcd = _qcd(fx["stream"])[1]
    eps0, mu0 = 14, 0x2A5
    s = _with_qcd(fx["stream"], (sqcd & 0xE0) | 1, struct.pack(">H", eps0 << 11 | mu0))
    fr = J.parse_frame(s, rows=fx["rows"], cols=fx["cols"], name="derived.dcm")
    eps = [eps0, eps0, eps0, eps0, eps0 - 1, eps0 - 1, eps0 - 1]
    np.testing.assert_array_equal(fr.band_mb, (sqcd >> 5) + np.array(eps) - 1)
    np.testing.assert_array_equal(fr.steps, np.array([(1 + mu0 / 2048) * 2.0 ** (16 - e) for e in eps], dtype=np.float32))
    # an exponent that would fall below 0 stays 0
    exps, steps = J._band_table(3, 1, [1 << 11 | mu0], 16, "derived.dcm")
    assert exps == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0] and len(steps) == 10


def test_reversible_frames_keep_their_tables():
    fx = REVERSIBLE["129x97_u16_rpcl_precincts"]
    fr = J.parse_frame(fx["stream"], rows=fx["rows"], cols=fx["cols"])
    guard, exps = JW.quant_header(fx["stream"])
    assert fr.transform == 1 and fr.steps is None
    np.testing.assert_array_equal(fr.band_mb, guard + np.array(exps) - 1)
    _, ftab, btab = J.build_batch([fr])
    assert ftab[0, 9] == 1 and not btab[:, 11].any()


def test_one_resolution_stream_patched_to_derived_decodes_to_the_same_pixels():
    fx = _fx("40x33_u16_1res")
    i, sqcd, body = _qcd(fx["stream"])
    assert sqcd & 31 == 2 and len(body) == 2                # one subband: the derived form carries the same one value
    s = _setb(fx["stream"], i + 4, (sqcd & 0xE0) | 1)
    fr = J.parse_frame(s, rows=fx["rows"], cols=fx["cols"], name="derived.dcm")
    px, ok = M.decode_frame(fr)
    assert ok
    np.testing.assert_array_equal(px, FX.expected(fx))
    if JW.have_pillow_j2k():
        np.testing.assert_array_equal(JW.openjpeg_decode(s), fx["decoded"])


def test_transform_and_quantisation_style_have_to_belong_together():
    lossy, lossless = _fx("129x97_u16_ct_rate10_3res_cb16"), REVERSIBLE["129x97_u16_rpcl_precincts"]
    i, sqcd, _ = _qcd(lossy["stream"])
    with pytest.raises(NotImplementedError, match="scalar quantisation"):           # 5/3 with style 2
        J.parse_frame(_setb(lossy["stream"], _transform_pos(lossy["stream"]), 1), rows=129, cols=97, name="mixed.dcm")
    with pytest.raises(NotImplementedError, match="lossy JPEG 2000 is not read"):   # 9/7 with style 0
        J.parse_frame(_setb(lossy["stream"], i + 4, sqcd & 0xE0), rows=129, cols=97, name="mixed.dcm")
    s = lossless["stream"]
    with pytest.raises(NotImplementedError, match="mixed.dcm.*lossy JPEG 2000 is not read"):
        J.parse_frame(_setb(s, _transform_pos(s), 0), rows=129, cols=97, name="mixed.dcm")
    assert J.parse_frame(lossy["stream"], rows=129, cols=97).transform == 0
    assert J.parse_frame(s, rows=129, cols=97).transform == 1


def test_qcc_and_coc_of_component_0_decide():
    """A QCD of style 0 and a COD with 5/3, overridden by the QCC / COC that hold the stream's real values: the effective pair
    is consistent, and the frame decodes as before."""
    fx = _fx("40x33_u16_1res")
    s = fx["stream"]
    i, sqcd, body = _qcd(s)
    c = s.index(b"\xFF\x52")
    cln = struct.unpack(">H", s[c + 2:c + 4])[0]
    cod = s[c + 4:c + 2 + cln]
    coc = struct.pack(">HHBB", 0xFF53, 4 + len(cod) - 5, 0, cod[0] & 1) + cod[5:]
    qcc = struct.pack(">HHBB", 0xFF5D, 4 + len(body), 0, sqcd) + body
    s2 = _with_qcd(_setb(s, _transform_pos(s), 1), sqcd & 0xE0, bytes([10 << 3]))
    with pytest.raises(NotImplementedError):
        J.parse_frame(_setb(s2, _transform_pos(s2), 0), rows=40, cols=33)
    end = s2.index(b"\xFF\x90")
    fr = J.parse_frame(s2[:end] + coc + qcc + s2[end:], rows=40, cols=33)
    px, ok = M.decode_frame(fr)
    assert ok and fr.transform == 0
    np.testing.assert_array_equal(px, FX.expected(fx))


def test_malformed_quantisation_names_the_file():
    fx = _fx("129x97_u16_ct_rate10_3res_cb16")
    s = fx["stream"]
    _, sqcd, body = _qcd(s)
    assert len(body) == 14
    with pytest.raises(DicomError, match="bad.dcm.*QCD marker segment truncated"):      # half a step value
        J.parse_frame(_with_qcd(s, sqcd, body[:-1]), rows=129, cols=97, name="bad.dcm")
    with pytest.raises(DicomError, match="bad.dcm.*QCD marker segment truncated"):      # derived, with one byte
        J.parse_frame(_with_qcd(s, (sqcd & 0xE0) | 1, body[:1]), rows=129, cols=97, name="bad.dcm")
    with pytest.raises(DicomError, match="bad.dcm.*holds 6 step sizes, 7 subbands"):    # too few for 3 NL + 1 bands
        J.parse_frame(_with_qcd(s, sqcd, body[:-2]), rows=129, cols=97, name="bad.dcm")


@pytest.mark.parametrize("ts", [JW.J2K_LOSSLESS, JW.J2K])
def test_the_stream_decides_not_the_transfer_syntax(tmp_path, ts):
    fx = _fx("40x33_u16_1res")
    JW.write_slice(tmp_path / "a.dcm", fx["decoded"], fx["stream"], transfer_syntax=ts, ipp=(0, 0, 0))
    ds = dicom.read_file(tmp_path / "a.dcm")
    fr = J.parse_frame(ds["PixelData"], rows=40, cols=33, name="a.dcm")
    assert fr.transform == 0
    np.testing.assert_array_equal(M.decode_frame(fr)[0], FX.expected(fx))
