"""JPEG-LS (ITU-T T.87) DICOM series decoded on the device (csrc/jls.hip): CharLS's streams (tests/golden/jls), the writer's at
sizes around the lane count and at every precision, with and without NEAR, images built to reach the escape code, the longest
runs, the clamps of C and the halving at RESET; the one-wave decoder against the one-lane decoder and the Python model, bit for
bit; per-frame errors; and get_image_info on JPEG-LS series against the uncompressed series of the same volume."""
import dataclasses
import os

import numpy as np
import pytest

from conftest import GOLDEN
from dicom_writer import write_slice as write_native_slice
import jls_model as M
import jls_writer as W

pytestmark = pytest.mark.gpu
SHAPES = ((1, 1), (1, 300), (300, 1), (5, 63), (5, 64), (5, 65), (97, 129))


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


def _frame(stream, shape, bits=16, name="frame"):
    from boa_hip import jpeg_ls as JL
    return JL.parse_frame(stream, rows=shape[0], cols=shape[1], bits_allocated=16, bits_stored=bits, name=name)


def _model(frame):
    return M.decode_scan(bytes(frame.data), frame.rows, frame.cols,
                         M.Params(frame.maxval, frame.near, frame.t1, frame.t2, frame.t3, frame.reset))


def _decode_all(ctx, frames, want_px, want_status):
    """The one-lane decoder and the one-wave one: the expected status, and for the frames that decode the expected samples (the
    samples of a failed frame are unspecified)."""
    from boa_hip import jpeg_ls as JL
    ok = np.asarray(want_status) == 0
    for kw in (dict(serial=True), dict()):
        px, st = JL.decode_frames(ctx, frames, **kw)
        assert px.dtype == np.uint16 and px.shape == (len(frames), frames[0].rows, frames[0].cols)
        np.testing.assert_array_equal(st, want_status, err_msg=str(kw))
        for i in np.flatnonzero(ok):
            np.testing.assert_array_equal(px[i], want_px[i], err_msg=f"{kw} frame {i} ({frames[i].name})")


def _ct_like(shape, bits, seed):
    rng = np.random.default_rng(seed)
    rows, cols = shape
    yy, xx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    body = ((yy - rows / 2) ** 2 / max(rows * 0.4, 1) ** 2 + (xx - cols / 2) ** 2 / max(cols * 0.4, 1) ** 2) < 1
    v = np.where(body, 1064 + rng.integers(-200, 201, shape), 24)
    return (v << (bits - 12) if bits >= 12 else v >> (12 - bits)).astype(np.int64)


def test_golden_charls_streams(ctx):
    generate = W.golden_generator()
    g = np.load(os.path.join(GOLDEN, "jls", "charls.npz"))
    for name in [k[7:] for k in g.files if k.startswith("stream_")]:
        want = g["decoded_" + name]
        fr = _frame(g["stream_" + name].tobytes(), want.shape, int(g["params_" + name][0]), name)
        px, st, _ = _model(fr)
        assert st == M.OK and (px == want).all(), name
        _decode_all(ctx, [fr], [want], [0])
    source = generate.phantom_slices()[generate.PHANTOM_Z[0]]
    fr = _frame(np.load(os.path.join(GOLDEN, "jls", "charls_phantom0.npz"))["stream_phantom"].tobytes(), (512, 512), 12, "phantom")
    px, st, _ = _model(fr)
    assert st == M.OK and (px == source).all()
    _decode_all(ctx, [fr], [source], [0])


@pytest.mark.parametrize("bits", [8, 12, 16])
def test_sizes_precisions_near(ctx, bits):
    """CT-like, uniform noise and quiet-with-spikes images, NEAR 0 and 3, every shape in one batch per shape: wave == serial ==
    model; the noise reaches the escape code and byte stuffing, the spikes the escape code under NEAR too."""
    rng = np.random.default_rng(bits)
    for shape in SHAPES:
        frames, want = [], []
        for near in (0, 3):
            spiky = np.where(rng.random(shape) < 0.03, rng.integers(0, 1 << bits, shape), (1 << (bits - 1)) + rng.integers(-8, 9, shape))
            for kind, img in (("ct", _ct_like(shape, bits, sum(shape))), ("noise", rng.integers(0, 1 << bits, shape)), ("spiky", spiky)):
                fr = _frame(W.encode(img, bits, near), shape, bits, f"{kind}_near{near}")
                px, st, stats = _model(fr)
                assert st == M.OK and int(np.abs(px.astype(int) - img).max()) <= near
                if shape == (97, 129) and kind != "ct":
                    # (uniform noise under NEAR 3 adapts k before a code can reach the escape: the quiet image with spikes does)
                    assert stats["escapes"] > 0 or (kind, near) == ("noise", 3)
                    assert 0xFF in fr.data or kind == "spiky"
                frames.append(fr)
                want.append(px)
        _decode_all(ctx, frames, want, [0] * len(frames))


def test_constant_wide_rows_reach_the_longest_runs(ctx):
    """2 x 65535 samples of one value: RUNindex climbs to 31; the rows are wider than the one-wave kernel's LDS rows."""
    shape = (2, 65535)
    fr = _frame(W.encode(np.full(shape, 200), 8), shape, 8, "constant")
    px, st, stats = _model(fr)
    assert st == M.OK and (px == 200).all() and stats["max_runindex"] == 31
    _decode_all(ctx, [fr], [px], [0])


def test_steep_ramp_reaches_the_clamps(ctx):
    """A 64 x 64 ramp falling by 300 per column and 500 per row: one context, a constant prediction error, so C runs into its
    clamp and N into RESET; the same with an LSE RESET of 3 and at 4096 columns (the widest rows of the one-wave kernel)."""
    yy, xx = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    img = 65000 - 300 * xx - 500 * yy
    frames = [_frame(W.encode(img, 16), (64, 64), 16, "ramp"), _frame(W.encode(img, 16, 0, (0, 0, 0, 0, 3)), (64, 64), 16, "ramp_reset3")]
    model = [_model(f) for f in frames]
    for px, st, stats in model:
        assert st == M.OK and (px == img).all() and stats["c_clamped"] and stats["n_reset"]
    _decode_all(ctx, frames, [img, img], [0, 0])
    wide = (np.arange(4096)[None, :] * 13 % 4096 + np.arange(3)[:, None]) % 4096
    fr = _frame(W.encode(wide, 12), (3, 4096), 12, "wide")
    assert _model(fr)[1] == M.OK
    _decode_all(ctx, [fr], [wide], [0])


def _unlike_frames(shape=(64, 80)):
    rng = np.random.default_rng(4)
    specs = [(np.full(shape, 1024), 16, 0, None), (_ct_like(shape, 12, 1), 12, 0, None), (rng.integers(0, 1 << 16, shape), 16, 0, None),
             (_ct_like(shape, 8, 2), 8, 0, None), (_ct_like(shape, 16, 3), 16, 2, None), (rng.integers(0, 256, shape), 8, 2, None),
             (_ct_like(shape, 12, 5), 12, 0, (4095, 9, 30, 100, 31))]
    frames = [_frame(W.encode(x, b, near, lse), shape, b, f"f{i}") for i, (x, b, near, lse) in enumerate(specs)]
    return frames, [_model(f) for f in frames]


def test_one_batch_of_unlike_frames_keeps_order(ctx):
    """Constant, CT-like and noise frames, 8-, 12- and 16-bit, NEAR 0 and 2, one with LSE, 280 frames in one batch (several
    waves share a compute unit); a table that points outside the data or holds parameters out of range is refused before
    anything is launched."""
    from boa_hip import jpeg_ls as JL
    frames, model = _unlike_frames()
    assert all(st == M.OK for _, st, _ in model)
    sizes = [len(f.data) for f in frames]
    assert max(sizes) > 50 * min(sizes)
    want = [px for px, _, _ in model]
    _decode_all(ctx, frames * 40, want * 40, [0] * 280)
    data, ftab = JL.build_batch(frames)
    for f, word, value in ((2, 2, len(data)), (0, 0, len(data)), (6, 2, sizes[6] + 16), (1, 2, -1), (3, 0, ftab[3, 0] + 2), (4, 1, 1),
                           (5, 3, 0), (5, 3, 65536), (5, 4, 128), (1, 5, 0), (1, 6, 17), (1, 7, 4096), (2, 8, 2), (2, 8, 65536)):
        bad = ftab.copy()
        bad[f, word] = value
        for serial in (False, True):
            with pytest.raises(ValueError, match="boa_jls_decode: frame"):
                JL._decode_tables(ctx, data, bad, frames[0].rows, frames[0].cols, serial=serial)
    with pytest.raises(ValueError, match="one size"):
        JL.decode_frames(ctx, [frames[0], dataclasses.replace(frames[1], rows=frames[1].rows + 1)])
    _decode_all(ctx, frames, want, [0] * len(frames))


def test_malformed_frames_report_and_next_batch_decodes(ctx):
    from boa_hip import jpeg_ls as JL
    from boa_hip.dicom import DicomError
    shape = (48, 50)
    x = _ct_like(shape, 12, 8)
    stream = W.encode(x, 12)
    good = _frame(stream, shape, 12, "good.dcm")
    scan = bytes(good.data)
    assert len(scan) > 400

    def damaged(name, data):
        return dataclasses.replace(good, name=name, data=np.frombuffer(data, dtype=np.uint8))

    at = stream.index(scan)
    frames = [good, damaged("half.dcm", scan[:len(scan) // 2]), damaged("last_byte.dcm", scan[:-1]),
              damaged("marker.dcm", scan[:300] + b"\xFF\xC3" + scan[302:]), damaged("zeros.dcm", bytes(len(scan))),
              # the marker as the host meets it: EOI in the middle of the scan, the rest of the stream behind it
              _frame(stream[:at + 300] + b"\xFF\xD9" + stream[at + 302:], shape, 12, "early_eoi.dcm"),
              dataclasses.replace(good, name="good2.dcm")]
    model = [_model(f) for f in frames]
    status = [st for _, st, _ in model]
    assert status == [0, M.TRUNCATED, M.TRUNCATED, M.TRUNCATED, M.INVALID, M.TRUNCATED, 0]
    assert len(frames[5].data) == 300
    _decode_all(ctx, frames, [px for px, _, _ in model], status)
    for kw in (dict(serial=True), dict()):
        for bad, why in zip(frames[1:6], ("scan truncated", "scan truncated", "scan truncated", "invalid code in the scan", "scan truncated")):
            with pytest.raises(DicomError, match=f"{bad.name}: JPEG-LS decode failed: {why}"):
                JL.decode(ctx, [frames[0], bad, frames[6]], **kw)
        np.testing.assert_array_equal(JL.decode(ctx, [frames[0], frames[6], frames[0]], **kw), np.stack([x] * 3).astype(np.uint16))


def _ct_volume(n=12, rows=40, cols=48, seed=0):
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.arange(n), np.arange(rows), np.arange(cols), indexing="ij")
    body = ((yy - rows / 2) ** 2 / (rows * 0.4) ** 2 + (xx - cols / 2) ** 2 / (cols * 0.4) ** 2) < 1
    hu = np.where(body, 40 + 10 * np.sin(zz / 3.0), -1000) + rng.normal(0, 15, body.shape)
    return np.clip(np.round(hu), -1024, 3071).astype(np.int64)


@pytest.mark.parametrize("signed,alloc,stored", [(False, 16, 16), (True, 16, 12), (False, 8, 8)])
def test_get_image_info_jls_equals_uncompressed(ctx, tmp_path, signed, alloc, stored):
    from boa_hip import nifti
    from boa_hip.compute.io import get_image_info
    hu = _ct_volume(seed=alloc + stored)
    if alloc == 8:
        values = (hu + 1024) >> 4                   # 0 .. 255, slope 1 intercept 0
        kw = dict(signed=False, intercept=0, bits_stored=8)
    else:
        values = np.clip(hu, -1024, 2047) if signed else hu + 1024
        kw = dict(signed=signed, intercept=0 if signed else -1024, bits_stored=stored)
    W.write_series(tmp_path / "raw", values, compressed=False, bits_allocated=alloc, **kw)
    W.write_series(tmp_path / "jls", values, bits_allocated=alloc, **kw)
    p_raw, info_raw = get_image_info(tmp_path / "raw", tmp_path / "o_raw")
    p_jls, info_jls = get_image_info(tmp_path / "jls", tmp_path / "o_jls")
    d_raw, a_raw, _ = nifti.load(p_raw)
    d_jls, a_jls, _ = nifti.load(p_jls)
    assert d_raw.dtype == d_jls.dtype
    np.testing.assert_array_equal(d_jls, d_raw)
    np.testing.assert_array_equal(a_jls, a_raw)
    np.testing.assert_array_equal(d_raw.transpose(2, 1, 0), values + kw["intercept"])
    assert info_raw == info_jls


def test_load_series_mixed_jls_and_native(ctx, tmp_path):
    """JPEG-LS slices in one to three fragments, with and without an offset table, beside native slices."""
    from boa_hip import dicom
    hu = _ct_volume(n=10, seed=9) + 1024
    os.makedirs(tmp_path / "mix")
    for z in range(10):
        p = str(tmp_path / "mix" / f"IM{z:04d}.dcm")
        ipp = (-100.0, -120.0, 50.0 + 1.5 * z)
        if z % 4 == 3:
            write_native_slice(p, hu[z], ipp=ipp, instance=z + 1)
        else:
            W.write_slice(p, hu[z], ipp=ipp, instance=z + 1, fragments=1 + z % 3, bot=bool(z % 2))
    data, geom, files = dicom.load_series(tmp_path / "mix", ctx=ctx)
    np.testing.assert_array_equal(data.transpose(2, 1, 0), hu - 1024)


def test_near_lossless_series_equals_the_model(ctx, tmp_path):
    """A NEAR-2 series (syntax .81): what the model decodes from the same streams, through the rescale."""
    from boa_hip import dicom
    hu = _ct_volume(n=10, seed=3) + 1024
    want = []
    for z in range(10):
        stream = W.encode(hu[z], 16, 2)
        px, st, _ = M.decode_stream(stream)
        assert st == M.OK and 0 < int(np.abs(px.astype(int) - hu[z]).max()) <= 2
        want.append(px.astype(np.int64) - 1024)
        W.write_slice(tmp_path / f"IM{z:04d}.dcm", hu[z], stream, near=2, ipp=(-100.0, -120.0, 50.0 + 1.5 * z), instance=z + 1)
    assert dicom.read_file(tmp_path / "IM0000.dcm")["TransferSyntaxUID"] == "1.2.840.10008.1.2.4.81"
    data, geom, files = dicom.load_series(tmp_path, ctx=ctx)
    np.testing.assert_array_equal(data.transpose(2, 1, 0), np.stack(want))
