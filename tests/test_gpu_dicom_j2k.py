"""JPEG 2000 DICOM series decoded on the device (csrc/j2k.hip): the committed OpenJPEG fixtures (tests/golden/j2k) decoded
bit-exactly, alone and in one mixed batch (lossless ones to their sources, truncated reversible ones to OpenJPEG's own decode),
blocks cut at every pass count against the numpy model, the clamp at both range ends, per-frame errors, get_image_info on J2K series against the uncompressed
series of the same pixels, a series mixing JPEG Lossless and JPEG 2000 slices, and a 512 x 512 x 600 series.  No Pillow here:
only the committed fixtures are read."""
import dataclasses
import os

import numpy as np
import pytest

import j2k_reference as R
import j2k_writer as JW
import ljpeg_writer as LW
from dicom_writer import write_series

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


@pytest.fixture(scope="module")
def fixtures():
    return JW.load_fixtures()


def _frame(fx, name=None, alloc=16):
    from boa_hip import jpeg2000 as J
    return J.parse_frame(fx["stream"], rows=fx["rows"], cols=fx["cols"], bits_allocated=alloc, name=name or fx["name"])


def _by_name(fixtures, name):
    return next(f for f in fixtures if f["name"] == name)


def test_every_fixture_alone(ctx, fixtures):
    from boa_hip import jpeg2000 as J
    assert len(fixtures) >= 20
    for fx in fixtures:
        px, st = J.decode_frames(ctx, [_frame(fx)])
        assert st[0] == 0, fx["name"]
        np.testing.assert_array_equal(px[0], JW.expected(fx), err_msg=fx["name"])


def test_all_geometries_in_one_call(ctx, fixtures):
    """Every fixture (1x1 to 512x512, 8 and 16 bits, signed, 1-8 resolutions, lossless and truncated) in one boa_j2k_decode
    call, twice over in a shuffled order."""
    from boa_hip import jpeg2000 as J
    order = np.random.default_rng(0).permutation(2 * len(fixtures)) % len(fixtures)
    frames = [_frame(fixtures[i], name=f"{fixtures[i]['name']}#{k}") for k, i in enumerate(order)]
    px, st = J.decode_frames(ctx, frames)
    assert (st == 0).all(), st
    for i, got in zip(order, px):
        np.testing.assert_array_equal(got, JW.expected(fixtures[i]), err_msg=fixtures[i]["name"])


@pytest.mark.parametrize("name", ["40x33_u8_lrcp_2layers", "40x33_s8_random"])
def test_every_pass_count_equals_the_model(ctx, fixtures, name):
    """One frame per P = 0 .. the most passes of a block, every block cut to its first min(P, own) passes, all in one call:
    every kind of last pass at every plane.  The numpy model keeps each coefficient's lowest coded plane; the kernel infers it
    from the last pass."""
    from boa_hip import jpeg2000 as J
    fr = _frame(_by_name(fixtures, name))
    own = fr.blocks[:, 6]
    assert (own[own > 0] == 3 * fr.blocks[own > 0, 5] - 2).all()         # a lossless fixture: every block complete
    frames = []
    for P in range(int(own.max()) + 1):
        b = fr.blocks.copy()
        b[:, 6] = np.minimum(P, own)
        frames.append(dataclasses.replace(fr, blocks=b, name=f"{name}#P{P}"))
    px, st = J.decode_frames(ctx, frames)
    assert (st == 0).all(), st
    want = [R.decode_frame(f) for f in frames]
    assert all(ok for _, ok in want)
    for P, (got, (w, _)) in enumerate(zip(px, want)):
        np.testing.assert_array_equal(got, w, err_msg=f"{name}: {P} passes")
    np.testing.assert_array_equal(px[-1], JW.expected(_by_name(fixtures, name)))
    assert len({w.tobytes() for w, _ in want}) > len(want) // 2         # (the cut frames really differ from one another)


def test_saturated_truncated_frames_clamp_at_both_ends(ctx, fixtures):
    from boa_hip import jpeg2000 as J
    sat = [f for f in fixtures if "saturated" in f["name"]]
    assert sorted((f["bits"], f["signed"]) for f in sat) == [(8, False), (16, False), (16, True)]
    px, st = J.decode_frames(ctx, [_frame(f) for f in sat])
    assert (st == 0).all(), st
    for fx, got in zip(sat, px):
        P = fx["bits"]
        lo, hi = (-(1 << (P - 1)), (1 << (P - 1)) - 1) if fx["signed"] else (0, (1 << P) - 1)
        assert fx["decoded"].min() == lo and fx["decoded"].max() == hi, fx["name"]
        np.testing.assert_array_equal(got, JW.expected(fx), err_msg=fx["name"])


def test_malformed_frame_reports_and_next_batch_decodes(ctx, fixtures):
    from boa_hip import jpeg2000 as J
    from boa_hip.dicom import DicomError
    fx = _by_name(fixtures, "129x97_u8_pcrl_3layers_cb16x64")
    good = fx["stream"]
    # every exponent raised to 31: Mb = G + 30, and a block without zero bit-planes has more than the 30 the decoder accepts
    deep = JW.patch_exponents(good, 31)
    # the LL exponent lowered until the LL block with the most zero bit-planes keeps one: it carries more passes than that
    g = J.parse_frame(good, rows=fx["rows"], cols=fx["cols"])
    guard, eps = JW.quant_header(good)
    ll = g.blocks[g.blocks[:, 0] == 0]
    zbp = int((guard + eps[0] - 1 - ll[:, 5]).max())
    shallow = JW.patch_marker(good, 0xFF5C, 1, (zbp + 2 - guard) << 3)
    # garbage in the code-block data: decodes to something, without a fault
    sod = good.index(b"\xFF\x93") + 2
    noise = bytes(np.random.default_rng(1).integers(0, 256, 400, dtype=np.uint8))
    garbage = good[:sod] + good[sod:sod + 40] + bytes(b & 0x7F for b in noise) + good[sod + 440:]
    names = ["good.dcm", "deep.dcm", "shallow.dcm", "good2.dcm"]
    frames = [J.parse_frame(s, rows=fx["rows"], cols=fx["cols"], name=n) for s, n in zip([good, deep, shallow, good], names)]
    px, st = J.decode_frames(ctx, frames)
    assert list(st) == [0, 1, 1, 0], st
    np.testing.assert_array_equal(px[0], JW.expected(fx))
    np.testing.assert_array_equal(px[3], JW.expected(fx))
    for bad in frames[1:3]:
        with pytest.raises(DicomError, match=bad.name):
            J.decode(ctx, [frames[0], bad])
    try:
        g = J.parse_frame(garbage, rows=fx["rows"], cols=fx["cols"], name="garbage.dcm")
    except Exception as e:                              # (tier-2 may already refuse it on the host)
        assert isinstance(e, DicomError) and "garbage.dcm" in str(e)
    else:
        J.decode_frames(ctx, [frames[0], g, frames[0]])
    px = J.decode(ctx, [frames[0]] * 3)
    np.testing.assert_array_equal(px, np.stack([JW.expected(fx)] * 3))


@pytest.mark.parametrize("name,syntax,signed_pr", [("129x97_u16_rpcl_precincts", JW.J2K_LOSSLESS, False),
                                                   ("129x97_s16_rpcl_3layers", JW.J2K, True),
                                                   ("129x97_s16_rpcl_3layers", JW.J2K_LOSSLESS, False),
                                                   ("129x97_u16_cprl_plt_com_cb32", JW.J2K, True)])
def test_get_image_info_j2k_equals_uncompressed(ctx, fixtures, tmp_path, name, syntax, signed_pr):
    """The codestream's samples, then the DICOM PixelRepresentation: a signed stream read as unsigned pixels and the reverse
    follow the existing BitsStored / sign rules, as for the uncompressed twin holding the same 16-bit patterns."""
    from boa_hip import nifti
    from boa_hip.compute.io import get_image_info
    fx = _by_name(fixtures, name)
    n = 12
    pattern = JW.expected(fx).astype(np.int64)
    stored = np.stack([pattern.astype(np.uint16).view(np.int16) if signed_pr else pattern] * n).astype(np.int64)
    kw = dict(signed=signed_pr, intercept=0 if signed_pr else -1024)
    write_series(tmp_path / "raw", stored, **kw)
    JW.write_series(tmp_path / "j2k", stored, [fx["stream"]] * n, transfer_syntax=syntax, **kw)
    p_raw, info_raw = get_image_info(tmp_path / "raw", tmp_path / "o_raw")
    p_j2k, info_j2k = get_image_info(tmp_path / "j2k", tmp_path / "o_j2k")
    d_raw, a_raw, _ = nifti.load(p_raw)
    d_j2k, a_j2k, _ = nifti.load(p_j2k)
    assert d_raw.dtype == d_j2k.dtype
    np.testing.assert_array_equal(d_j2k, d_raw)
    np.testing.assert_array_equal(a_j2k, a_raw)
    np.testing.assert_array_equal(d_raw.transpose(2, 1, 0), stored + (0 if signed_pr else -1024))
    assert info_raw == info_j2k


@pytest.mark.parametrize("names,signed_pr", [(("129x97_u16_ct_trunc_rate10", "129x97_u16_ct_trunc_2layers_cb16"), False),
                                             (("64x64_s16_1res_trunc",), True)])
def test_get_image_info_truncated_j2k_equals_openjpeg_pixels(ctx, fixtures, tmp_path, names, signed_pr):
    """A .91 series of truncated reversible streams reads as the uncompressed series that holds OpenJPEG's decoded pixels."""
    from boa_hip import nifti
    from boa_hip.compute.io import get_image_info
    fxs = [_by_name(fixtures, n) for n in names]
    assert all(f["signed"] == signed_pr and "decoded" in f for f in fxs)
    n = 12
    stored = np.stack([fxs[z % len(fxs)]["decoded"] for z in range(n)]).astype(np.int64)
    assert any(not np.array_equal(f["decoded"], f["source"]) for f in fxs)
    kw = dict(signed=signed_pr, intercept=0 if signed_pr else -1024)
    write_series(tmp_path / "raw", stored, **kw)
    JW.write_series(tmp_path / "j2k", stored, [fxs[z % len(fxs)]["stream"] for z in range(n)], transfer_syntax=JW.J2K, **kw)
    p_raw, info_raw = get_image_info(tmp_path / "raw", tmp_path / "o_raw")
    p_j2k, info_j2k = get_image_info(tmp_path / "j2k", tmp_path / "o_j2k")
    d_raw, a_raw, _ = nifti.load(p_raw)
    d_j2k, a_j2k, _ = nifti.load(p_j2k)
    assert d_raw.dtype == d_j2k.dtype
    np.testing.assert_array_equal(d_j2k, d_raw)
    np.testing.assert_array_equal(a_j2k, a_raw)
    np.testing.assert_array_equal(d_raw.transpose(2, 1, 0), stored + (0 if signed_pr else -1024))
    assert info_raw == info_j2k


def test_load_series_mixing_jpeg_lossless_and_j2k(ctx, fixtures, tmp_path):
    from boa_hip import dicom
    from dicom_writer import write_slice
    fx = _by_name(fixtures, "129x97_u16_cprl_plt_com_cb32")
    src = fx["source"]
    os.makedirs(tmp_path / "mix")
    for z in range(10):
        p = str(tmp_path / "mix" / f"IM{z:04d}.dcm")
        ipp = (-100.0, -120.0, 50.0 + 1.5 * z)
        if z % 3 == 0:
            LW.write_compressed_slice(p, src, LW.encode(src, precision=16), ipp=ipp, instance=z + 1, fragments=2)
        elif z % 3 == 1:
            JW.write_slice(p, src, fx["stream"], transfer_syntax=(JW.J2K, JW.J2K_LOSSLESS)[z % 2], ipp=ipp, instance=z + 1,
                           fragments=1 + z % 3, bot=bool(z % 2))
        else:
            write_slice(p, src, ipp=ipp, instance=z + 1)
    data, geom, files = dicom.load_series(tmp_path / "mix", ctx=ctx)
    np.testing.assert_array_equal(data.transpose(2, 1, 0), np.stack([src] * 10) - 1024)


def test_600_slice_series(ctx, fixtures):
    from boa_hip import jpeg2000 as J
    ph = [f for f in fixtures if f["name"].startswith("512x512_ct_phantom")]
    assert len(ph) == 2
    base = [_frame(f) for f in ph]
    frames = [base[z % 2] for z in range(600)]
    px = J.decode(ctx, frames)
    assert px.shape == (600, 512, 512)
    for k in range(2):
        np.testing.assert_array_equal(px[k::2], np.broadcast_to(JW.expected(ph[k]), (300, 512, 512)))
