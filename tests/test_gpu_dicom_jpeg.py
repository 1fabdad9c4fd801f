"""JPEG Lossless (Process 14) DICOM series decoded on the device (csrc/jpeg_ll.hip): bit-identity with libjpeg-turbo at P = 8
(tests/golden/ljpeg), round trips of tests/ljpeg_writer.py streams at P = 12 / 16, the parallel decoder against the serial one,
per-frame errors, and get_image_info on compressed series against the uncompressed series of the same volume."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from dicom_writer import write_series
import ljpeg_writer as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


def _frame(stream, shape, P, name="frame", bits_allocated=16):
    from boa_hip import jpeg_lossless as J
    return J.parse_frame(stream, rows=shape[0], cols=shape[1], bits_allocated=bits_allocated, bits_stored=P, name=name)


def _decode_all(ctx, frames, **kw):
    """Both decoders (and the parallel one at a tiny subsequence size): identical output and status."""
    from boa_hip import jpeg_lossless as J
    px, st = J.decode_frames(ctx, frames, **kw)
    ps, ss = J.decode_frames(ctx, frames, serial=True)
    pt, stt = J.decode_frames(ctx, frames, subseq_bytes=4)
    np.testing.assert_array_equal(st, ss)
    np.testing.assert_array_equal(st, stt)
    np.testing.assert_array_equal(px, ps)
    np.testing.assert_array_equal(px, pt)
    return px, st


def _roundtrip(ctx, images, P, **enc):
    frames = [_frame(W.encode(x, precision=P, **enc), x.shape, P, name=f"img{i}") for i, x in enumerate(images)]
    px, st = _decode_all(ctx, frames)
    assert (st == 0).all(), st
    pt = enc.get("pt", 0)
    for x, got in zip(images, px):
        np.testing.assert_array_equal(got, ((np.asarray(x) >> pt) << pt).astype(np.uint16))


def test_golden_p8_libjpeg_turbo(ctx):
    g = np.load(os.path.join(GOLDEN, "ljpeg", "p8_libjpeg_turbo.npz"))
    for i, (h, w, pred, pt, rr) in enumerate(g["params"]):
        fr = _frame(g[f"stream_{i}"].tobytes(), (h, w), 8, name=f"golden{i}", bits_allocated=8)
        assert (fr.predictor, fr.pt, fr.restart_rows) == (pred, pt, rr if rr < h else 0)
        px, st = _decode_all(ctx, [fr])
        assert st[0] == 0
        np.testing.assert_array_equal(px[0], g[f"decoded_{i}"].astype(np.uint16), err_msg=f"golden stream {i}")


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (511, 509), (512, 512)])
def test_sizes_every_predictor_p16(ctx, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    noise = rng.integers(0, 1 << 16, shape)
    smooth = (np.cumsum(rng.integers(-40, 41, shape), axis=1) + 30000) % (1 << 16)
    for pred in range(1, 8):
        _roundtrip(ctx, [noise, smooth], 16, predictor=pred)


def test_p12_constant_noise_pt_restarts(ctx):
    rng = np.random.default_rng(3)
    imgs = [np.full((64, 70), 2049), np.zeros((64, 70), dtype=np.int64), rng.integers(0, 4096, (64, 70))]
    for pred in range(1, 8):
        for pt in (0, 3):
            for rr in (0, 1, 5, 64):
                _roundtrip(ctx, imgs, 12, predictor=pred, pt=pt, restart_rows=rr)


def test_ssss16_differences(ctx):
    x = np.zeros((9, 40), dtype=np.int64)
    x[:, 1::2] = 32768                                  # every difference along a row is +-32768: SSSS 16, no extra bits
    d = W.differences(x, precision=16)
    assert (W.categories(d)[0][:, 1:] == 16).all()
    for pred in (1, 2, 7):
        _roundtrip(ctx, [x, 65535 - x], 16, predictor=pred)


def test_16_bit_codes_and_several_tables_in_one_batch(ctx):
    rng = np.random.default_rng(5)
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    s = np.repeat(np.arange(17), fib[::-1])            # category frequencies Fibonacci: code lengths pushed to 16
    rng.shuffle(s)
    s = np.concatenate([s, np.zeros(64 * 66 - len(s), dtype=np.int64)])[:64 * 66].reshape(64, 66)
    lo = 1 << np.maximum(s - 1, 0)
    mag = np.where(s >= 16, 32768, lo + rng.integers(0, lo))    # a magnitude of category s: [2^(s-1), 2^s)
    d = np.where(s == 0, 0, np.where(rng.random(s.shape) < 0.5, mag, -mag)) & 0xFFFF
    x = ((1 << 15) + np.cumsum(d[:, :1], axis=0)) % 65536          # predictor 1 reconstruction of those differences
    x = (x + np.concatenate([np.zeros((64, 1), dtype=np.int64), np.cumsum(d[:, 1:], axis=1)], axis=1)) % 65536
    np.testing.assert_array_equal(W.differences(x, precision=16), d)
    counts, _ = W.optimal_table(np.bincount(W.categories(d)[0].ravel(), minlength=17))
    assert counts[15] > 0, "no 16-bit code"
    noise = rng.integers(0, 1 << 16, (64, 66))
    const = np.full((64, 66), 1234)
    # different optimal tables per frame, table ids 0-3, unused extra DHT entries
    streams = [W.encode(x, precision=16), W.encode(noise, precision=16, table_id=2),
               W.encode(const, precision=16, table_id=3, extra_tables=[(0, *W.optimal_table(np.ones(17)))]),
               W.encode(noise, precision=16, predictor=5, restart_rows=7, table_id=1)]
    frames = [_frame(st, (64, 66), 16, name=f"t{i}") for i, st in enumerate(streams)]
    px, st = _decode_all(ctx, frames)
    assert (st == 0).all()
    for got, want in zip(px, [x, noise, const, noise]):
        np.testing.assert_array_equal(got, want.astype(np.uint16))


def test_parallel_equals_serial_noisy_batch(ctx):
    from boa_hip import jpeg_lossless as J
    rng = np.random.default_rng(11)
    vol = rng.integers(0, 1 << 16, (64, 512, 512))
    frames = [_frame(W.encode(v, precision=16, predictor=1 + i % 7, restart_rows=(0, 8, 1)[i % 3]), v.shape, 16, name=f"n{i}")
              for i, v in enumerate(vol)]
    pp, sp = J.decode_frames(ctx, frames, subseq_bytes=16)
    ps, ss = J.decode_frames(ctx, frames, serial=True)
    assert (sp == 0).all() and (ss == 0).all()
    np.testing.assert_array_equal(pp, ps)
    np.testing.assert_array_equal(pp, vol.astype(np.uint16))


def test_malformed_frames_report_and_next_batch_decodes(ctx):
    from boa_hip import jpeg_lossless as J
    from boa_hip.dicom import DicomError
    rng = np.random.default_rng(2)
    x = rng.integers(0, 4096, (48, 50))
    good = W.encode(x, precision=12)
    head = good.index(b"\xFF\xDA") + 10                 # SOS segment: marker + length 8
    ecs = good[head:-2]
    truncated = good[:head] + ecs[:len(ecs) // 2] + b"\xFF\xD9"
    mid = len(ecs) // 2 - (len(ecs) // 2) % 2
    invalid = good[:head] + ecs[:mid] + b"\xFF\x00" * 8 + ecs[mid:] + b"\xFF\xD9"   # sixteen 1-bytes: no code is all 1 bits
    garbage = good[:head] + ecs + bytes(rng.integers(0, 255, 64, dtype=np.uint8)) + b"\xFF\xD9"
    frames = [_frame(s, x.shape, 12, name=n) for s, n in
              [(good, "good.dcm"), (truncated, "truncated.dcm"), (invalid, "invalid.dcm"), (garbage, "garbage.dcm")]]
    for serial in (False, True):
        _, st = J.decode_frames(ctx, frames, serial=serial)
        assert st[0] == 0 and st[1] == 1 and st[2] == 2 and st[3] == 3, (serial, st)
        for bad in frames[1:]:
            with pytest.raises(DicomError, match=bad.name):
                J.decode(ctx, [frames[0], bad], serial=serial)
    px = J.decode(ctx, [frames[0]] * 3)
    np.testing.assert_array_equal(px, np.stack([x] * 3).astype(np.uint16))


def _ct_volume(n=12, rows=40, cols=48, seed=0):
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.arange(n), np.arange(rows), np.arange(cols), indexing="ij")
    body = ((yy - rows / 2) ** 2 / (rows * 0.4) ** 2 + (xx - cols / 2) ** 2 / (cols * 0.4) ** 2) < 1
    hu = np.where(body, 40 + 10 * np.sin(zz / 3.0), -1000) + rng.normal(0, 15, body.shape)
    return np.clip(np.round(hu), -1024, 3071).astype(np.int64)


@pytest.mark.parametrize("syntax,pred,signed,bits", [(W.JPEG_LOSSLESS_SV1, 1, False, 16), (W.JPEG_LOSSLESS, 6, True, 16),
                                                     (W.JPEG_LOSSLESS_SV1, 1, True, 12), (W.JPEG_LOSSLESS, 3, False, 12)])
def test_get_image_info_compressed_equals_uncompressed(ctx, tmp_path, syntax, pred, signed, bits):
    from boa_hip import nifti
    from boa_hip.compute.io import get_image_info
    hu = _ct_volume(seed=pred)
    stored = hu if signed else hu + 1024            # signed: slope 1 intercept 0; unsigned: intercept -1024
    kw = dict(signed=signed, intercept=0 if signed else -1024, bits_stored=bits)
    write_series(tmp_path / "raw", stored, **kw)
    W.write_compressed_series(tmp_path / "jpg", stored, transfer_syntax=syntax, predictor=pred,
                              restart_rows=4 if pred == 3 else 0, **kw)
    p_raw, info_raw = get_image_info(tmp_path / "raw", tmp_path / "o_raw")
    p_jpg, info_jpg = get_image_info(tmp_path / "jpg", tmp_path / "o_jpg")
    d_raw, a_raw, _ = nifti.load(p_raw)
    d_jpg, a_jpg, _ = nifti.load(p_jpg)
    assert d_raw.dtype == d_jpg.dtype
    np.testing.assert_array_equal(d_jpg, d_raw)
    np.testing.assert_array_equal(a_jpg, a_raw)
    np.testing.assert_array_equal(d_raw.transpose(2, 1, 0), hu)
    assert info_raw == info_jpg


def test_load_series_mixed_fragments(ctx, tmp_path):
    """Compressed slices as one to three fragments, with and without an offset table, beside native slices of the series."""
    from boa_hip import dicom
    from dicom_writer import write_slice
    hu = _ct_volume(n=10, seed=9) + 1024
    os.makedirs(tmp_path / "mix")
    for z in range(10):
        p = str(tmp_path / "mix" / f"IM{z:04d}.dcm")
        ipp = (-100.0, -120.0, 50.0 + 1.5 * z)
        if z % 4 == 3:
            write_slice(p, hu[z], ipp=ipp, instance=z + 1)
        else:
            W.write_compressed_slice(p, hu[z], W.encode(hu[z], precision=16), ipp=ipp, instance=z + 1, fragments=1 + z % 3,
                                     bot=bool(z % 2))
    data, geom, files = dicom.load_series(tmp_path / "mix", ctx=ctx)
    np.testing.assert_array_equal(data.transpose(2, 1, 0), hu - 1024)
