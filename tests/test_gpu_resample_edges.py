"""Edge cases of the resampling kernels (csrc/resample.hip) and of `boa_ct_normalize`, every call through the C ABI, every
comparison on raw bits (fp64 as uint64, fp32 as uint32, labels equal): no tolerance anywhere.  References: scipy.ndimage.zoom
for `boa_resample_cubic` / `boa_resample_nearest_u8`, oracle.nnunet_resample.resample_data_or_seg (+ oracle.labels.argmax_labels)
for `boa_resize_skimage_f32` / `boa_resize_logits_argmax`, numpy float32 for `boa_ct_normalize`.  The cases come from
tests/resample_cases.py, which tests/test_resample_cases_cpu.py pins without a device (shape identities, the once / twice rounded
halves, the one-ulp-past-the-extent list, the residues of the contiguous axis).

  A  contiguous-axis prefilter (`k_spline_filter_contig`): last axis of every length 2 .. 33 = every residue mod 8 of the padded
     length at four lengths, down and up, leading dims kept and resized, noise and a +-30000 step (clip active)
  B  cubic geometry: output axes of length 1 and 2, input axes of length 2, x8, identity, every (n_in, n_out) whose last
     coordinate lies one ulp past the extent on every axis, four input dtypes, int32 truncation around zero, EINVAL for n_in = 1
  C  nearest: n_in 1 .. 39 x n_out 1 .. 59 on one axis against the index formula and scipy
  D  per-slice clip groups: every slice with its own value range, slice axis 0 / 1 / 2 kept and resized, single slices, < 8 voxels
  E  logits resize + argmax: the double -> half pairs that round differently through float32, slice axes 1 and 2, C = 1 / 255,
     crops flush with the far corner, one-voxel crops, merge over a lut that maps a class to 0, ties between classes 2 and 7
  F  CTNormalization from float32 and int32, the sd clamp, n = 0, a second trip of the grid-stride loop

Logits stay finite: the reference raises on inf logits and the task checks the inf flag before `boa_resize_logits_argmax` runs;
NaN / inf semantics of that kernel are not part of this file."""
import ctypes as C

import numpy as np
import pytest

import resample_cases as R
from test_gpu_nnunet_resample import _i3, _resize

pytestmark = pytest.mark.gpu

_RES = R.contig_residue_table()
assert sorted(_RES) == list(range(8)) and min(len(v) for v in _RES.values()) >= 4, _RES     # every scalar-tail length, >= 4 times

IN_DTYPES = {np.dtype(np.int16): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2, np.dtype(np.int32): 3}


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def _cubic(ctx, x, out_shape, out_dtype=np.float64):
    from boa_hip._lib import check
    x = np.ascontiguousarray(x)
    d_in = ctx.from_numpy(x)
    d_out = ctx.alloc(int(np.prod(out_shape)) * np.dtype(out_dtype).itemsize)
    try:
        check(ctx.lib.boa_resample_cubic(ctx.h, d_in.vp, IN_DTYPES[x.dtype], _i3(x.shape), d_out.vp,
                                         0 if np.dtype(out_dtype) == np.int32 else 1, _i3(out_shape)))
        return d_out.download(tuple(out_shape), out_dtype)
    finally:
        d_in.free()
        d_out.free()


def _zoom3(x, out_shape):
    from scipy import ndimage
    ref = ndimage.zoom(np.asarray(x, np.float64), R.zoom_tuple(x.shape, out_shape), order=3, mode="nearest")
    assert ref.shape == tuple(out_shape), (x.shape, out_shape, ref.shape)
    return ref


def _oracle_resize(x, out_shape, axis):
    from oracle import nnunet_resample as nnr
    want = nnr.resample_data_or_seg(x[None], out_shape, axis if axis >= 0 else None, 3, axis >= 0, 0)[0]
    assert want.dtype == np.float32 and want.shape == tuple(out_shape)
    return want


def _bits_equal(got, want, msg):
    u = {8: np.uint64, 4: np.uint32}[got.dtype.itemsize]
    assert got.dtype == want.dtype and got.shape == want.shape, msg
    np.testing.assert_array_equal(got.view(u), want.view(u), err_msg=msg)


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["noise", "step"])
@pytest.mark.parametrize("z", R.CONTIG_LENGTHS)
def test_contig_prefilter_cubic(ctx, z, regime):
    assert z in _RES[(z + 24) % 8]
    for k, (i, o) in enumerate(R.contig_cases(z)):
        x = R.amplitude_volume(i, regime, 100 * z + k)
        _bits_equal(_cubic(ctx, x, o), _zoom3(x, o), f"{i} -> {o}, padded length {z + 24} = {(z + 24) % 8} mod 8")


@pytest.mark.parametrize("regime", ["noise", "step"])
@pytest.mark.parametrize("z", R.CONTIG_LENGTHS)
def test_contig_prefilter_skimage(ctx, z, regime):
    assert z in _RES[(z + 24) % 8]
    clipped = 0
    for k, (i, o) in enumerate(R.contig_cases(z)):
        x = R.amplitude_volume(i, regime, 100 * z + k).astype(np.float32)
        for axis in (-1, 0):
            want = _oracle_resize(x, o, axis)
            _bits_equal(_resize(ctx, x, o, axis), want, f"{i} -> {o}, slice axis {axis}, padded length {z + 24} = {(z + 24) % 8} mod 8")
            clipped += int((np.abs(want) == 30000).sum())
    if regime == "step" and z >= 8:
        assert clipped > 50                               # the overshoot was there to be clipped


# ---- B ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dtype", [np.int16, np.float32, np.float64, np.int32])
@pytest.mark.parametrize("name", sorted(R.CUBIC_GEOMETRY))
def test_cubic_geometry(ctx, name, in_dtype):
    i, o = R.CUBIC_GEOMETRY[name]
    x = (np.random.default_rng(len(name)).normal(size=i) * 400).astype(in_dtype)
    ref = _zoom3(x, o)
    _bits_equal(_cubic(ctx, x, o), ref, f"{name} {i} -> {o}")
    np.testing.assert_array_equal(_cubic(ctx, x, o, np.int32), ref.astype(np.int32), err_msg=name)


_PAST = R.past_extent_cases()


@pytest.mark.parametrize("part", range(12))
def test_cubic_last_coordinate_past_the_extent(ctx, part):
    """(n_out - 1) * fl((n_in - 1) / (n_out - 1)) = n_in - 1 + one ulp: scipy evaluates the spline there, inside its padding"""
    assert len(_PAST) >= 3 and any(i[1] == 47 and o[1] == 43 for i, o in _PAST)
    dtypes = [np.float64, np.int16, np.float32, np.int32]
    for k, (i, o) in list(enumerate(_PAST))[part::12]:
        x = (np.random.default_rng(k).normal(size=i) * 400).astype(dtypes[k % 4])
        _bits_equal(_cubic(ctx, x, o), _zoom3(x, o), f"{i} -> {o}")


@pytest.mark.parametrize("in_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["up8", "identity", "out1_axis1", "in2_all"])
def test_cubic_int32_truncates_toward_zero(ctx, name, in_dtype):
    """values on both sides of zero with |t| < 1: `.astype(np.int32)` gives 0 where floor gives -1 and rounding gives +-1"""
    i, o = R.CUBIC_GEOMETRY[name]
    x = (np.random.default_rng(7).normal(size=i) * 0.6).astype(in_dtype)
    ref = _zoom3(x, o)
    if ref.size > 100:
        assert ((ref > -1) & (ref < 0)).any() and ((ref > 0.5) & (ref < 1)).any() and ((ref < -0.5) & (ref > -1)).any()
    np.testing.assert_array_equal(_cubic(ctx, x, o, np.int32), ref.astype(np.int32))


def test_cubic_refuses_an_input_axis_of_one_sample(ctx):
    from boa_hip._lib import BOA_EINVAL
    d_in, d_out = ctx.zeros(16 * 8), ctx.zeros(64 * 8)
    for ax in range(3):
        i = [4, 4, 4]
        i[ax] = 1
        rc = ctx.lib.boa_resample_cubic(ctx.h, d_in.vp, 2, _i3(i), d_out.vp, 1, _i3((4, 4, 4)))
        assert rc == BOA_EINVAL
        assert b"boa_resample_cubic" in ctx.lib.boa_last_error()
    d_in.free()
    d_out.free()


# ---- C ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_in", R.NEAREST_IN)
def test_nearest_sweep(ctx, n_in):
    from boa_hip._lib import check
    from scipy import ndimage
    for n_out in R.NEAREST_OUT:
        ax = (n_in + n_out) % 3
        i, o = [2, 2], [2, 2]
        i.insert(ax, n_in)
        o.insert(ax, n_out)
        x = (np.arange(4 * n_in) % 251).astype(np.uint8).reshape(i)
        d_in, d_out = ctx.from_numpy(x), ctx.alloc(4 * n_out)
        check(ctx.lib.boa_resample_nearest_u8(ctx.h, d_in.vp, _i3(i), d_out.vp, _i3(o)))
        got = d_out.download(tuple(o), np.uint8)
        d_in.free()
        d_out.free()
        idx = [np.arange(2)] * 2
        idx.insert(ax, R.nearest_index(n_in, n_out))
        np.testing.assert_array_equal(got, x[np.ix_(*idx)], err_msg=f"{n_in} -> {n_out} on axis {ax}: index formula")
        ref = ndimage.zoom(x, R.zoom_tuple(i, o), order=0, mode="nearest")
        assert ref.shape == tuple(o)
        np.testing.assert_array_equal(got, ref, err_msg=f"{n_in} -> {n_out} on axis {ax}: scipy")


# ---- D ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SLICE_CLIP_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + "x".join(map(str, c[1])) + f"-ax{c[2]}")
def test_per_slice_clip(ctx, case):
    i, o, axis = case
    x = R.slice_range_volume(i, axis, sum(i) + axis)
    _bits_equal(_resize(ctx, x, o, axis), _oracle_resize(x, o, axis), str(case))


# ---- E ------------------------------------------------------------------------------------------------------------------
def _argmax(ctx, lg, off, crop, out, axis, lut, merge=0, prefill=0):
    from boa_hip._lib import check
    d_lg = ctx.from_numpy(np.ascontiguousarray(lg).view(np.uint16))
    n = int(np.prod(out))
    d_lab = ctx.alloc(n)
    try:
        check(ctx.lib.boa_memset(ctx.h, d_lab.vp, prefill, n))
        check(ctx.lib.boa_resize_logits_argmax(ctx.h, d_lg.vp, lg.shape[0], _i3(lg.shape[1:]), _i3(off), _i3(crop), _i3(out), axis,
                                               lut.ctypes.data_as(C.c_void_p) if lut is not None else None, merge, d_lab.vp))
        return d_lab.download(tuple(out), np.uint8)
    finally:
        d_lg.free()
        d_lab.free()


def _oracle_labels(lg, off, crop, out, axis):
    from oracle import labels as olab
    from oracle import nnunet_resample as nnr
    box = np.ascontiguousarray(lg[:, off[0]:off[0] + crop[0], off[1]:off[1] + crop[1], off[2]:off[2] + crop[2]])
    want_lg = nnr.resample_data_or_seg(box, out, axis if axis >= 0 else None, 1, axis >= 0, 0)
    assert want_lg.dtype == np.float16 and want_lg.shape == (lg.shape[0], *out)
    return olab.argmax_labels(want_lg), want_lg


@pytest.mark.parametrize("pair", R.HALF_PAIRS, ids=lambda p: f"{p[0]:g}")
def test_logits_double_to_half_rounds_once(ctx, pair):
    """0.75 a + 0.25 b rounds to a different half through float32; class 1 sits on the larger of the two candidates, so the label
    at output plane 1 says which rounding ran (tests/test_resample_cases_cpu.py shows the oracle's labels and the twice-rounded
    ones differ for every pair)."""
    for arr in R.half_rounding_case(pair):
        lg = arr["logits"]
        want, _ = _oracle_labels(lg, (0, 0, 0), lg.shape[1:], arr["out"], arr["axis"])
        assert set(np.unique(want)) == {0, 1}
        got = _argmax(ctx, lg, (0, 0, 0), lg.shape[1:], arr["out"], arr["axis"], None)
        np.testing.assert_array_equal(got, want, err_msg=f"pair {pair}, slice axis {arr['axis']}")


LOGIT_CASES = {
    "axis1_same": dict(grid=(9, 7, 11), off=(1, 0, 2), crop=(7, 7, 8), out=(10, 7, 13), axis=1, C=9),
    "axis1_new": dict(grid=(9, 7, 11), off=(1, 2, 2), crop=(7, 4, 8), out=(10, 9, 13), axis=1, C=9),
    "axis2_same": dict(grid=(9, 7, 11), off=(0, 1, 3), crop=(8, 5, 6), out=(11, 9, 6), axis=2, C=9),
    "axis2_new": dict(grid=(9, 7, 11), off=(0, 1, 3), crop=(8, 5, 6), out=(6, 8, 10), axis=2, C=9),
    "C1_3d": dict(grid=(5, 6, 7), off=(0, 0, 0), crop=(5, 6, 7), out=(7, 5, 9), axis=-1, C=1),
    "C1_axis0": dict(grid=(5, 6, 7), off=(1, 0, 0), crop=(3, 6, 7), out=(4, 8, 5), axis=0, C=1),
    "C255_3d": dict(grid=(4, 5, 6), off=(0, 0, 0), crop=(4, 5, 6), out=(6, 5, 8), axis=-1, C=255),
    "C255_axis1": dict(grid=(4, 5, 6), off=(0, 1, 0), crop=(4, 3, 6), out=(5, 4, 9), axis=1, C=255),
    "far_corner_3d": dict(grid=(10, 9, 8), off=(4, 3, 2), crop=(6, 6, 6), out=(9, 8, 11), axis=-1, C=9),
    "far_corner_axis0": dict(grid=(10, 9, 8), off=(4, 3, 2), crop=(6, 6, 6), out=(5, 8, 11), axis=0, C=9),
    "far_corner_axis2": dict(grid=(10, 9, 8), off=(4, 3, 2), crop=(6, 6, 6), out=(7, 4, 6), axis=2, C=9),
    "one_voxel_axis0": dict(grid=(6, 7, 8), off=(5, 2, 1), crop=(1, 4, 6), out=(3, 6, 5), axis=-1, C=9),
    "one_voxel_axis2": dict(grid=(6, 7, 8), off=(1, 2, 7), crop=(4, 4, 1), out=(5, 3, 4), axis=-1, C=9),
    "one_voxel_inplane": dict(grid=(6, 7, 8), off=(0, 6, 1), crop=(6, 1, 6), out=(6, 2, 9), axis=0, C=9),
}


@pytest.mark.parametrize("name", sorted(LOGIT_CASES))
def test_logits_resize_argmax_edges(ctx, name):
    """Labels against the oracle (order 1, float16 result, numpy argmax: first maximum wins), written through a lut; then merge
    mode over a volume pre-filled with 9.  The merge rule looks at the CLASS INDEX, not at the mapped value: class 0 never
    writes, although lut[0] = 5, and class 3 writes lut[3] = 0 over the 9."""
    case = LOGIT_CASES[name]
    Cn, grid, off, crop, out, axis = (case[k] for k in ("C", "grid", "off", "crop", "out", "axis"))
    assert all(o + c <= g for o, c, g in zip(off, crop, grid))
    if name.startswith("far_corner"):
        assert all(o + c == g and o > 0 for o, c, g in zip(off, crop, grid))
    rng = np.random.default_rng(len(name) + Cn)
    lg = (rng.standard_normal((Cn, *grid)) * 4).astype(np.float16)
    if Cn > 1:
        lg[1, ::3] = lg[0, ::3]                                              # ties between neighbouring classes
    if Cn > 7:
        h = grid[2] // 2                                                     # upper half of the last axis: classes 2 and 7 tie on top
        lg[2, :, :, h:] = (lg[2, :, :, h:].astype(np.float32) + 30).astype(np.float16)
        lg[7, :, :, h:] = lg[2, :, :, h:]
    assert np.isfinite(lg).all()
    want, want_lg = _oracle_labels(lg, off, crop, out, axis)
    if Cn > 7 and off[2] + crop[2] > grid[2] // 2 + 1:
        tie = (want_lg[2] == want_lg[7]) & (want == 2)
        assert tie.sum() > 20                                                # ... and the oracle gives them to class 2
    if Cn == 1:
        assert (want == 0).all()
    if Cn == 255:
        assert want.max() > 128
    lut = (np.arange(256) * 7 % 251).astype(np.uint8)
    lut[0], lut[3] = 5, 0
    np.testing.assert_array_equal(_argmax(ctx, lg, off, crop, out, axis, lut), lut[want], err_msg=name)
    np.testing.assert_array_equal(_argmax(ctx, lg, off, crop, out, axis, None), want, err_msg=name + " (identity lut)")
    got = _argmax(ctx, lg, off, crop, out, axis, lut, merge=1, prefill=9)
    np.testing.assert_array_equal(got, np.where(want != 0, lut[want], 9), err_msg=name + " (merge)")
    assert (got[want == 0] == 9).all() and (got[want == 3] == 0).all()
    if name in ("axis1_new", "far_corner_3d"):
        assert (want == 0).any() and (want == 3).any()


# ---- F ------------------------------------------------------------------------------------------------------------------
def _normalize(ctx, x, code, mean, sd, lo, hi, n=None, prefill=None):
    from boa_hip._lib import check
    n = x.size if n is None else n
    d_in = ctx.from_numpy(x)
    d_out = ctx.alloc(max(x.size, 1) * 4)
    try:
        if prefill is not None:
            d_out.upload(prefill)
        check(ctx.lib.boa_ct_normalize(ctx.h, d_in.vp, code, d_out.vp, n, mean, sd, lo, hi))
        return d_out.download(x.shape, np.float32)
    finally:
        d_in.free()
        d_out.free()


F32 = np.float32
NORM_ARGS = [(40.25, 310.5, -900.0, 1200.0), (-103.7, 0.0, -1000.5, 250.25), (12.0, 1e-9, -1000.5, 250.25)]


@pytest.mark.parametrize("mean,sd,lo,hi", NORM_ARGS)
def test_ct_normalize_float32(ctx, mean, sd, lo, hi):
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(5003) * 700).astype(F32)
    edge = [F32(lo), F32(hi), np.nextafter(F32(lo), F32(np.inf)), np.nextafter(F32(lo), F32(-np.inf)),
            np.nextafter(F32(hi), F32(np.inf)), np.nextafter(F32(hi), F32(-np.inf)), F32(mean), F32(0.1), F32(-0.1), F32(1e-30)]
    x[:len(edge)] = edge
    want = R.ct_normalize_ref(x, mean, sd, lo, hi)
    assert np.isfinite(want).all() and (x == F32(lo)).any() and (x == F32(hi)).any() and (x != np.rint(x)).any()
    _bits_equal(_normalize(ctx, x, 1, mean, sd, lo, hi), want, f"sd {sd}")


@pytest.mark.parametrize("mean,sd,lo,hi", NORM_ARGS + [(123.456, 1000.5, -2.0 ** 30, 2.0 ** 30)])
def test_ct_normalize_int32(ctx, mean, sd, lo, hi):
    rng = np.random.default_rng(12)
    x = np.concatenate([rng.integers(-2 ** 31, 2 ** 31 - 1, size=3000), rng.integers(-2000, 2000, size=2001),
                        [2 ** 24 + 1, -(2 ** 24) - 1, 2 ** 30, -(2 ** 30), 2 ** 30 + 1, 2 ** 30 - 1, 2 ** 31 - 1, -(2 ** 31), int(lo), int(hi)]]).astype(np.int32)
    assert (x.astype(F32).astype(np.float64) != x).sum() > 1000          # int -> float rounds above 2^24
    want = R.ct_normalize_ref(x, mean, sd, lo, hi)
    assert np.isfinite(want).all()
    _bits_equal(_normalize(ctx, x, 2, mean, sd, lo, hi), want, f"sd {sd}")


def test_ct_normalize_clamps_sd(ctx):
    """sd = 0 and 1e-9 divide by 1e-8f, as 1e-8 itself does; 2e-8 does not"""
    x = np.arange(-50, 50, dtype=np.int32)
    outs = [_normalize(ctx, x, 2, 1.5, sd, -40.0, 40.0) for sd in (0.0, 1e-9, 1e-8, 2e-8)]
    assert np.isfinite(outs[0]).all()
    _bits_equal(outs[0], R.ct_normalize_ref(x, 1.5, 0.0, -40.0, 40.0), "sd 0")
    _bits_equal(outs[1], outs[0], "sd 1e-9")
    _bits_equal(outs[2], outs[0], "sd 1e-8")
    _bits_equal(outs[3], R.ct_normalize_ref(x, 1.5, 2e-8, -40.0, 40.0), "sd 2e-8")
    assert (outs[3] != outs[0]).any()


def test_ct_normalize_n0_writes_nothing(ctx):
    x = np.arange(64, dtype=np.int32)
    keep = np.full(64, 7.5, F32)
    for code, arr in ((0, x.astype(np.int16)), (1, x.astype(F32)), (2, x)):
        got = _normalize(ctx, arr, code, 1.0, 2.0, -5.0, 5.0, n=0, prefill=keep)
        _bits_equal(got, keep, f"in_dtype {code}")


@pytest.mark.parametrize("code,dtype", [(2, np.int32), (1, np.float32), (0, np.int16)])
def test_ct_normalize_grid_stride_second_trip(ctx, code, dtype):
    """more elements than the launch has threads (cu_count * 16 blocks of 256), and a ragged end"""
    threads = ctx.info()["cu_count"] * 16 * 256
    n = 2 * threads + 333
    assert n > threads and n % 256 != 0
    rng = np.random.default_rng(13)
    x = rng.integers(-3000, 3000, size=n).astype(dtype)
    if dtype == np.int32:
        x[::7] = rng.integers(-2 ** 31, 2 ** 31 - 1, size=x[::7].size)
    x[-1] = 17
    want = R.ct_normalize_ref(x, 40.25, 310.5, -900.0, 1200.0)
    _bits_equal(_normalize(ctx, x, code, 40.25, 310.5, -900.0, 1200.0), want, f"n {n}")
