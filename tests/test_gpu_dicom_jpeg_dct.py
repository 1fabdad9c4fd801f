"""Sequential DCT JPEG DICOM series (transfer syntaxes .50 / .51) decoded on the device (csrc/jpeg_dct.hip): bit-identity with
libjpeg-turbo's default decode at P = 8 and P = 12 (tests/golden/jpeg_dct), tests/jpeg_dct_writer.py streams against the numpy
model of tests/jpeg_dct_model.py (itself pinned to libjpeg on the CPU), the parallel entropy decoder against the serial one,
per-frame errors, the chunked workspace, and get_image_info on compressed series against the uncompressed series that holds
libjpeg's pixels."""
import os

import numpy as np
import pytest

from dicom_writer import write_series, write_slice
import jpeg_dct_model as M
import jpeg_dct_writer as W
import ljpeg_writer as LW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.compute.inference import get_context
    return get_context("gpu")


def _frame(stream, shape, P, name="frame"):
    from boa_hip import jpeg_dct as J
    return J.parse_frame(stream, rows=shape[0], cols=shape[1], bits_allocated=16, bits_stored=P, name=name)


def _decode_all(ctx, frames):
    """Both entropy decoders, the parallel one also at tiny subsequence sizes: identical output and status."""
    from boa_hip import jpeg_dct as J
    px, st = J.decode_frames(ctx, frames)
    ps, ss = J.decode_frames(ctx, frames, serial=True)
    for sub in (4, 16):
        pt, stt = J.decode_frames(ctx, frames, subseq_bytes=sub)
        np.testing.assert_array_equal(st, stt)
        np.testing.assert_array_equal(px, pt)
    np.testing.assert_array_equal(st, ss)
    np.testing.assert_array_equal(px, ps)
    return px, st


def _check(ctx, items):
    """items: [(coef, kwargs of W.encode)] of one size -> decoded by every path to the model's pixels."""
    frames, want = [], []
    for i, (coef, kw) in enumerate(items):
        stream = W.encode(coef, **kw)
        p = M.parse(stream)
        frames.append(_frame(stream, (p["rows"], p["cols"]), p["P"], name=f"f{i}"))
        want.append(M.pixels(coef, p["qt"], p["P"], p["rows"], p["cols"]))
    px, st = _decode_all(ctx, frames)
    assert (st == 0).all(), st
    for i, (got, w) in enumerate(zip(px, want)):
        np.testing.assert_array_equal(got, w, err_msg=f"frame {i}")


def _all_fixtures():
    return [(which, n, s, px) for which in ("p8", "p12") for n, (s, px) in W.fixtures(which).items()]


@pytest.mark.parametrize("which,name", [(w, n) for w, n, _, _ in _all_fixtures()])
def test_fixture_alone_decodes_to_libjpegs_pixels(ctx, which, name):
    stream, want = W.fixtures(which)[name]
    px, st = _decode_all(ctx, [_frame(stream, want.shape, 8 if which == "p8" else 12, name=name)])
    assert st[0] == 0
    np.testing.assert_array_equal(px[0], want)


def test_fixtures_of_both_depths_and_several_table_sets_in_one_call(ctx):
    sel = [(w, n, s, px) for w, n, s, px in _all_fixtures() if px.shape in ((40, 48), (37, 51))]
    for shape in ((40, 48), (37, 51)):
        grp = [t for t in sel if t[3].shape == shape]
        assert {t[0] for t in grp} == {"p8", "p12"}
        frames = [_frame(s, shape, 8 if w == "p8" else 12, name=n) for w, n, s, _ in grp] * 2
        assert len({(f.dc, f.ac) for f in frames}) >= 2 and len({f.precision for f in frames}) == 2
        px, st = _decode_all(ctx, frames)
        assert (st == 0).all()
        for got, (_, n, _, want) in zip(px, grp * 2):
            np.testing.assert_array_equal(got, want, err_msg=n)


@pytest.mark.parametrize("shape", [(1, 1), (8, 8), (9, 17), (64, 8), (511, 509)])
def test_sizes_from_the_writer_against_the_model(ctx, shape):
    rng = np.random.default_rng(shape[0] * 3 + shape[1])
    nb = -(-shape[0] // 8) * -(-shape[1] // 8)
    items = []
    for P in (8, 12):
        qt = rng.integers(1, 30, 64)
        items.append((W.random_coefficients(rng, nb, P), dict(rows=shape[0], cols=shape[1], P=P, qt=qt, optimal=True)))
        items.append((W.random_coefficients(rng, nb, P, density=0.05), dict(rows=shape[0], cols=shape[1], P=P, qt=qt, optimal=True,
                                                                            ri=max(1, -(-shape[1] // 8)))))
    _check(ctx, items)


def test_parallel_equals_serial_on_dense_noisy_coefficients(ctx):
    """Dense coefficients of large magnitude: long codewords, so that subsequences of 4 and 16 bytes begin inside extra bits and
    inside blocks, and resynchronisation takes many subsequences."""
    rng = np.random.default_rng(21)
    rows, cols, nb = 64, 72, 72
    items = []
    for P in (8, 12):
        for ri in (0, 5):
            coef = W.random_coefficients(rng, nb, P, density=0.95, amp=1 << (P - 1), dc_amp=1 << (P + 2))
            items.append((coef, dict(rows=rows, cols=cols, P=P, optimal=True, ri=ri)))
    _check(ctx, items)


def test_named_coding_cases(ctx):
    rng = np.random.default_rng(4)
    rows, cols, nb = 24, 40, 15
    kw = dict(rows=rows, cols=cols)
    items = []
    for P, smax in ((8, 11), (12, 15)):
        last = W.random_coefficients(rng, nb, P, density=0.2)
        last[:, 63] = rng.integers(1, 5, nb)                           # the 64th coefficient non-zero: no EOB
        items.append((last, dict(kw, P=P, optimal=True)))
        zrl = np.zeros((nb, 64), dtype=np.int64)
        zrl[:, 0] = rng.integers(-50, 50, nb)
        zrl[::3, M.ZIGZAG[63]] = -1                                    # ZRL ZRL ZRL then run 14
        zrl[1::3, M.ZIGZAG[17]] = 2                                    # one ZRL, run 0
        zrl[2::3, M.ZIGZAG[33]] = 1
        zrl[2::3, M.ZIGZAG[49]] = -3                                   # ZRL chains twice in a block (run 15 coded as run/size)
        items.append((zrl, dict(kw, P=P)))
        items.append((np.zeros((nb, 64), dtype=np.int64), dict(kw, P=P)))               # all-EOB frame, DC differences 0
        items.append((np.zeros((nb, 64), dtype=np.int64), dict(kw, P=P, ri=1)))
        big = np.zeros((nb, 64), dtype=np.int64)
        top = (1 << (smax - 1)) - 1
        big[::2, 0], big[1::2, 0] = top, -top - 1                      # DC differences of SSSS smax, both signs
        big[:, 1] = np.where(np.arange(nb) % 2, (1 << (smax - 1)) - 1, -(1 << (smax - 2)))   # AC of SSSS smax - 1, smax - 1
        assert max(abs(int(d)).bit_length() for d in np.diff(big[:, 0])) == smax
        items.append((big, dict(kw, P=P, optimal=True)))
        for ri in (1, 7, 5, 100):                                      # every block, odd, one block row, more than all blocks
            items.append((W.random_coefficients(rng, nb, P), dict(kw, P=P, optimal=True, ri=ri)))
    _check(ctx, items)


def test_16_bit_codes(ctx):
    """AC symbol frequencies growing a little faster than Fibonacci numbers (f[n] = f[n-1] + f[n-2] + 1: no ties, so the Huffman
    tree is one long chain) push the optimal code lengths to the 16-bit limit.  287 blocks, so that the EOB of every block takes
    the place of the number 287 among the sixteen other symbols' frequencies."""
    rng = np.random.default_rng(6)
    f = [1, 1]
    while len(f) < 17:
        f.append(f[-1] + f[-2] + 1)
    nb = 287
    counts = [v for v in f[::-1] if v != nb]
    assert len(counts) == 16 and sum(counts) <= 29 * nb
    seq = np.repeat(np.arange(16), counts)                             # symbol index i -> (run i % 2, size 1 + i // 2)
    rng.shuffle(seq)
    coef = np.zeros((nb, 64), dtype=np.int64)
    coef[:, 0] = rng.integers(-100, 100, nb)
    for b in range(nb):
        k = 1
        for i in seq[b::nb]:                                           # 28 or 29 symbols a block: at most 58 positions
            k += int(i) % 2
            coef[b, M.ZIGZAG[k]] = (1 << (int(i) // 2)) * (1 if (b + k) % 2 else -1)
            k += 1
    kw = dict(rows=56, cols=328, P=8, optimal=True)
    assert M.parse(W.encode(coef, **kw))["ac"][0][15] > 0, "no 16-bit code"
    _check(ctx, [(coef, kw), (coef, dict(kw, ri=41))])


def test_every_branch_of_the_range_limit(ctx):
    nb = 16
    for P in (8, 12):
        mx = (1 << P) - 1
        qt = np.ones(64, dtype=np.int64)
        qt[0] = 64                                                     # a DC of d moves every sample by 8 d
        coef = np.zeros((nb, 64), dtype=np.int64)
        coef[:, 0] = [0, 3, -3, mx // 16, -(mx // 16) - 1, mx // 8, -(mx // 8), mx // 4, -(mx // 4), 3 * mx // 8 + 5, -(3 * mx // 8),
                      mx // 2, -(mx // 2), 1, -1, 7][:nb]
        coef[:, 1] = 2
        coef[:, 8] = -1
        want = M.pixels(coef, qt, P, 32, 32)
        x = M._pass(M._pass((coef * qt).reshape(-1, 8, 8).transpose(0, 2, 1), 13 - M.pass1_bits(P)).transpose(0, 2, 1), 16 + M.pass1_bits(P))
        centre = (mx + 1) // 2
        idx = x & (4 * mx + 3)
        assert (idx < centre).any() and ((idx >= centre) & (idx < 2 * (mx + 1))).any() and (idx >= 4 * (mx + 1) - centre).any()
        assert ((idx >= 2 * (mx + 1)) & (idx < 4 * (mx + 1) - centre)).any() and want.min() == 0 and want.max() == mx
        _check(ctx, [(coef, dict(rows=32, cols=32, P=P, qt=qt, optimal=True))])


def _damaged(P=12):
    """(name, stream, expected status) of one good frame and frames damaged in the entropy-coded data."""
    rng = np.random.default_rng(2)
    rows, cols, nb = 48, 56, 42
    coef = W.random_coefficients(rng, nb, P, density=0.5)
    good = W.encode(coef, rows=rows, cols=cols, P=P)                    # the Annex K tables: no code is all 1 bits
    head = good.index(b"\xFF\xDA") + 10
    ecs = good[head:-2]
    mid = len(ecs) // 2
    out = [("good.dcm", good), ("truncated.dcm", good[:head] + ecs[:mid] + b"\xFF\xD9"),
           ("invalid.dcm", good[:head] + ecs[:mid] + b"\xFF\x00" * 8 + ecs[mid:] + b"\xFF\xD9"),
           ("trailing.dcm", good[:head] + ecs + bytes(rng.integers(0, 255, 64, dtype=np.uint8)) + b"\xFF\xD9")]
    # a run past 63: in a block whose last coefficient sits at zig-zag index 62, the EOB behind it (k = 63) is replaced by the
    # codeword of (run 3, size 1)
    past = np.zeros((nb, 64), dtype=np.int64)
    past[:, 0] = 3
    past[5, M.ZIGZAG[62]] = 1
    s = W.encode(past, rows=rows, cols=cols, P=P)
    p = M.parse(s)
    steps = []
    M.decode_coefficients(p, steps)
    k = next(i for i, t in enumerate(steps) if t[5] == 62)
    at, eob_len = steps[k + 1][1], steps[k + 1][3]
    assert steps[k + 1][2] == 63 and steps[k + 1][5] == -1
    code, ln = LW.canonical_codes(*p["ac"])[0x31]
    bits = "".join(f"{b:08b}" for b in p["segments"][0])
    new = bits[:at] + f"{code:0{ln}b}" + "1" + bits[at + eob_len:]
    new += "1" * (-len(new) % 8)
    seg = bytes(int(new[i:i + 8], 2) for i in range(0, len(new), 8)).replace(b"\xFF", b"\xFF\x00")
    out.append(("run_past.dcm", s[:s.index(b"\xFF\xDA") + 10] + seg + b"\xFF\xD9"))
    # an oversized SSSS: a P = 12 stream with DC differences of SSSS 12 relabelled as P = 8 (SOF1 allows both)
    wide = np.zeros((nb, 64), dtype=np.int64)
    wide[::2, 0] = 2500
    s = W.encode(wide, rows=rows, cols=cols, P=12, optimal=True)
    i = s.index(b"\xFF\xC1")
    out.append(("ssss.dcm", s[:i + 4] + b"\x08" + s[i + 5:]))
    want = [0, M.TRUNCATED, M.INVALID_CODE, M.TRAILING, M.RUN_PAST_BLOCK, M.BAD_SSSS]
    return (rows, cols), coef, [(n, st, w) for (n, st), w in zip(out, want)]


def test_malformed_frames_report_and_next_batch_decodes(ctx):
    from boa_hip import jpeg_dct as J
    from boa_hip.dicom import DicomError
    shape, coef, cases = _damaged()
    for name, stream, want in cases:
        assert M.decode(stream)[1] == want, name                        # the model agrees on what is wrong with each
    frames = [_frame(s, shape, 8 if n == "ssss.dcm" else 12, name=n) for n, s, _ in cases]
    for kw in (dict(), dict(serial=True), dict(subseq_bytes=4), dict(subseq_bytes=16)):
        px, st = J.decode_frames(ctx, frames, **kw)
        assert list(st) == [w for _, _, w in cases], (kw, st)
        np.testing.assert_array_equal(px[0], M.pixels(coef, np.ones(64), 12, *shape))
        for bad in frames[1:]:
            with pytest.raises(DicomError, match=bad.name):
                J.decode(ctx, [frames[0], bad], **kw)
    px = J.decode(ctx, [frames[0]] * 3)
    np.testing.assert_array_equal(px, np.stack([M.pixels(coef, np.ones(64), 12, *shape)] * 3))


def test_host_entry_rejects_inconsistent_tables(ctx):
    """boa_jdct_decode validates every table field on the host: BOA_EINVAL before the device is touched."""
    import ctypes as C
    from boa_hip import jpeg_dct as J
    shape, coef, cases = _damaged()
    fr = _frame(cases[0][1], shape, 12)
    data, ftab, segs, subs, tabs, qt = J.build_batch([fr, fr], 16)
    d_data = ctx.from_numpy(data)
    out = ctx.alloc(2 * shape[0] * shape[1] * 2)
    ip = C.POINTER(C.c_int)

    def call(ftab=ftab, segs=segs, subs=subs, tabs=tabs, nbytes=data.nbytes, n_tabs=None, n_q=None):
        status = np.zeros(2, dtype=np.int32)
        arrs = [np.ascontiguousarray(a) for a in (ftab, segs, subs, tabs, qt)]
        return ctx.lib.boa_jdct_decode(
            ctx.h, d_data.vp, nbytes, 2, arrs[0].ctypes.data_as(ip), shape[0], shape[1], len(arrs[1]), arrs[1].ctypes.data_as(ip),
            len(arrs[2]), arrs[2].ctypes.data_as(ip), len(arrs[3]) if n_tabs is None else n_tabs,
            arrs[3].ctypes.data_as(C.POINTER(C.c_uint32)), len(arrs[4]) if n_q is None else n_q,
            arrs[4].ctypes.data_as(C.POINTER(C.c_uint16)), out.vp, status.ctypes.data_as(ip), 0)

    def edited(a, idx, v):
        b = a.copy()
        b[idx] = v
        return b

    assert call() == 0
    bad = [dict(ftab=edited(ftab, (1, 0), ftab[1, 0] + 2)), dict(ftab=edited(ftab, (1, 2), data.nbytes)), dict(nbytes=len(fr.data)),
           dict(ftab=edited(ftab, (0, 3), 10)), dict(ftab=edited(ftab, (0, 5), 9)), dict(ftab=edited(ftab, (0, 7), 3)),
           dict(ftab=edited(ftab, (1, 9), 2)), dict(ftab=edited(ftab, (1, 10), len(subs))), dict(ftab=edited(ftab, (0, 4), 5)),
           dict(segs=edited(segs, (0, 1), len(fr.data) + 4)), dict(segs=edited(segs, (1, 2), 1)), dict(segs=edited(segs, (1, 3), 0)),
           dict(subs=edited(subs, (1, 0), 0)), dict(subs=edited(subs, (2, 1), 1)), dict(subs=edited(subs, (len(subs) - 1, 0), len(fr.data))),
           dict(tabs=edited(tabs, (0, 0), 0x0A00)), dict(tabs=edited(tabs, (1, 256 + 12), 1 << 12)), dict(n_tabs=1), dict(n_q=0)]
    for kw in bad:
        assert call(**kw) != 0, kw
    assert call() == 0
    d_data.free()
    out.free()


def test_chunked_workspace(ctx, monkeypatch):
    """A dozen 64 x 64 frames (8 KiB of coefficients each) under a workspace cap of 20 KiB: six chunks of two frames."""
    from boa_hip import jpeg_dct as J
    rng = np.random.default_rng(9)
    items = [(W.random_coefficients(rng, 64, 8 + 4 * (i % 2)), dict(rows=64, cols=64, P=8 + 4 * (i % 2), optimal=True, ri=(0, 3)[i % 2]))
             for i in range(12)]
    frames = [_frame(W.encode(c, **kw), (64, 64), kw["P"], name=f"c{i}") for i, (c, kw) in enumerate(items)]
    want = np.stack([M.pixels(c, np.ones(64), kw["P"], 64, 64) for c, kw in items])
    whole, st = J.decode_frames(ctx, frames)
    assert (st == 0).all()
    np.testing.assert_array_equal(whole, want)
    for cap in ("20", "1"):                                             # two frames per chunk; below one frame: one per chunk
        monkeypatch.setenv("BOA_JDCT_WS_KB", cap)
        for kw in (dict(), dict(serial=True), dict(subseq_bytes=8)):
            got, st = J.decode_frames(ctx, frames, **kw)
            assert (st == 0).all()
            np.testing.assert_array_equal(got, want)


def _series(P, signed, n=12):
    """n streams of one size at precision P and the stored values libjpeg decodes them to."""
    rng = np.random.default_rng(P + signed)
    rows, cols, nb = 40, 48, 30
    streams, stored = [], []
    for z in range(n):
        coef = W.random_coefficients(rng, nb, P, density=0.2, amp=1 << (P - 5), dc_amp=1 << (P - 2))
        coef[:, 0] += (-(1 << (P - 3)) if not signed else (1 << (P - 3)) * (1 if z % 2 else -3))
        qt = rng.integers(1, 12, 64)
        streams.append(W.encode(coef, rows=rows, cols=cols, P=P, qt=qt, optimal=True, ri=(0, 6)[z % 2]))
        px = M.pixels(coef, qt, P, rows, cols).astype(np.int64)
        stored.append(np.where(px >= (1 << (P - 1)), px - (1 << P), px) if signed else px)
    return streams, np.stack(stored)


@pytest.mark.parametrize("syntax,P,signed", [(W.JPEG_EXTENDED, 12, False), (W.JPEG_EXTENDED, 12, True), (W.JPEG_BASELINE, 8, False)])
def test_get_image_info_compressed_equals_uncompressed(ctx, tmp_path, syntax, P, signed):
    from boa_hip import nifti
    from boa_hip.compute.io import get_image_info
    streams, stored = _series(P, signed)
    if signed:
        assert stored.min() < 0 < stored.max()
    kw = dict(signed=signed, intercept=0 if signed else -1024, bits_stored=P)
    write_series(tmp_path / "raw", stored, **kw)
    W.write_compressed_series(tmp_path / "jpg", streams, stored, transfer_syntax=syntax, **kw)
    p_raw, info_raw = get_image_info(tmp_path / "raw", tmp_path / "o_raw")
    p_jpg, info_jpg = get_image_info(tmp_path / "jpg", tmp_path / "o_jpg")
    d_raw, a_raw, _ = nifti.load(p_raw)
    d_jpg, a_jpg, _ = nifti.load(p_jpg)
    assert d_raw.dtype == d_jpg.dtype
    np.testing.assert_array_equal(d_jpg, d_raw)
    np.testing.assert_array_equal(a_jpg, a_raw)
    np.testing.assert_array_equal(d_raw.transpose(2, 1, 0), stored + (0 if signed else -1024))
    assert info_raw == info_jpg


def test_fixture_series_through_get_image_info(ctx, tmp_path):
    """libjpeg's own stream and pixels (P = 12) as a .51 series."""
    from boa_hip import nifti
    from boa_hip.compute.io import get_image_info
    stream, px = next(v for k, v in W.fixtures("p12").items() if k.startswith("37x51"))
    stored = np.stack([px.astype(np.int64)] * 10)
    kw = dict(intercept=-1024, bits_stored=12)
    write_series(tmp_path / "raw", stored, **kw)
    W.write_compressed_series(tmp_path / "jpg", [stream] * 10, stored, **kw)
    d_raw = nifti.load(get_image_info(tmp_path / "raw", tmp_path / "o_raw")[0])[0]
    d_jpg = nifti.load(get_image_info(tmp_path / "jpg", tmp_path / "o_jpg")[0])[0]
    np.testing.assert_array_equal(d_jpg, d_raw)
    np.testing.assert_array_equal(d_jpg.transpose(2, 1, 0), stored - 1024)


def test_series_mixing_lossless_and_dct_slices(ctx, tmp_path):
    from boa_hip import dicom
    streams, stored = _series(12, False, n=10)
    os.makedirs(tmp_path / "mix")
    for z in range(10):
        p = str(tmp_path / "mix" / f"IM{z:04d}.dcm")
        ipp = (-100.0, -120.0, 50.0 + 1.5 * z)
        if z % 3 == 0:
            LW.write_compressed_slice(p, stored[z], LW.encode(stored[z], precision=12), transfer_syntax=LW.JPEG_LOSSLESS_SV1, ipp=ipp,
                                      instance=z + 1, bits_stored=12)
        elif z % 3 == 1:
            LW.write_compressed_slice(p, stored[z], streams[z], transfer_syntax=W.JPEG_EXTENDED, ipp=ipp, instance=z + 1,
                                      bits_stored=12, fragments=1 + z % 2)
        else:
            write_slice(p, stored[z], ipp=ipp, instance=z + 1, bits_stored=12)
    data, geom, files = dicom.load_series(tmp_path / "mix", ctx=ctx)
    np.testing.assert_array_equal(data.transpose(2, 1, 0), stored - 1024)
