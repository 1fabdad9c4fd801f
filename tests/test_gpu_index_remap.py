"""boa_copy3 (k_copy3_t, k_copy3) and boa_nonzero_bbox (vector loop, per-element loop) against numpy on the same views, case by case
(tests/remap_cases.py; tests/test_remap_cases_cpu.py proves what each case is built to have).  Every comparison is bit-exact and over
the WHOLE destination buffer, which starts as 0xAA; the source is downloaded again and has to be unchanged; and every case asserts
through the launch counters `copy_t` / `bbox_vec` that the kernel it is named for ran -- a case that falls back proves nothing."""
import ctypes as C

import numpy as np
import pytest

import remap_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from boa_hip.device import Context
    c = Context(0)
    yield c
    c.close()


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(RC.bits(got) != RC.bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} elements differ, first at {bad[:8]}: got {got[bad[:8]]}, want {want[bad[:8]]}"


def dev_view(ctx, buf, base_shape, dtype, ops):
    from boa_hip.devarray import DevArray
    v = DevArray(ctx, buf, base_shape, dtype)
    for op in ops:
        v = getattr(v, op[0])(*op[1:])
    return v


def run_copy(ctx, c):
    """one boa_copy3 call through DevArray.copy_to; returns the counter so that callers can tally"""
    from boa_hip.devarray import DevArray
    src, dst = ctx.from_numpy(c["src"]), ctx.from_numpy(c["dst"])
    try:
        if c["src_ops"] is not None:           # the views as DevArray builds them
            sv = dev_view(ctx, src, c["src_base_shape"], c["src"].dtype, c["src_ops"])
            dv = dev_view(ctx, dst, c["dst_base_shape"], c["dst"].dtype, c["dst_ops"])
            assert (sv.offset, sv.strides, sv.shape) == (c["in_off"], c["in_strides"], c["shape"])
            assert (dv.offset, dv.strides, dv.shape) == (c["out_off"], c["out_strides"], c["shape"])
        else:                                  # overlapping rows, broadcasts, a strided destination: explicit strides
            sv = DevArray(ctx, src, c["shape"], c["src"].dtype, c["in_strides"], c["in_off"])
            dv = DevArray(ctx, dst, c["shape"], c["dst"].dtype, c["out_strides"], c["out_off"])
        predicted = RC.copy3_transposed(c["shape"], c["in_strides"], c["out_strides"])
        assert predicted == (c["axis"] is not None)
        ctx.counters(reset=True)
        sv.copy_to(dv)
        cnt = ctx.counters()
        got = dst.download(c["dst"].shape, c["dst"].dtype)
        after = src.download(c["src"].shape, c["src"].dtype)
    finally:
        src.free()
        dst.free()
    assert cnt["copy_t"] == (1 if predicted else 0), (c["name"], cnt["copy_t"], predicted)
    assert_same_bits(got, RC.expected_dst(c), c["name"] + " destination")
    assert_same_bits(after, c["src"], c["name"] + " source after the call")
    return cnt["copy_t"]


# ---- boa_copy3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.COPY_NAMES)
def test_copy3_views(ctx, name):
    """tiles (full, partial, single), signs of the unit and of the outer strides, boxes inside larger buffers, priority between the two
    candidate axes, broadcasts, and the four ways to miss the rule by one condition"""
    run_copy(ctx, RC.copy_cases()[name])


@pytest.mark.parametrize("n", RC.GRID_BATCHES + RC.GRID_TILE_ROWS)
def test_copy3_grid_limits(ctx, n):
    """batch extent 65 535 runs k_copy3_t with gridDim.z = 65 535, 65 536 has to fall back to k_copy3 (16 MiB of uint8 each way);
    the same for gridDim.y: 65 535 tiles of 64 along axis 2, and one element more (64 MiB each way)"""
    run_copy(ctx, RC.grid_limit_case(n))


@pytest.mark.parametrize("o", RC.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("i", RC.DTYPES, ids=lambda d: d.name)
@pytest.mark.parametrize("kernel", ["t", "e"])
def test_copy3_dtype_matrix(ctx, kernel, i, o):
    """all 25 (in, out) pairs through k_copy3_t on (3, 17, 33) and through k_copy3 on (3, 5, 7): wraparound of narrowing integer
    conversions, round-to-nearest-even of int32 -> float32 and float64 -> float32 (ties, subnormal results, overflow to inf, signed
    zeros), truncation toward zero of in-range float -> int, and every bit pattern (NaN payloads) through same-dtype copies"""
    assert run_copy(ctx, RC.matrix_case(kernel, i, o)) == (1 if kernel == "t" else 0)


# ---- boa_nonzero_bbox ------------------------------------------------------------------------------------------------------------
def run_bbox(ctx, vol, lead):
    """the box of `vol`, which sits `lead` elements into its buffer (0: through DevArray; otherwise through the C ABI with the
    advanced pointer); returns (box, whether the vector loop ran)"""
    from boa_hip._lib import check
    from boa_hip.devarray import DevArray
    flat, off = RC.bbox_embed(vol, lead)
    buf = ctx.from_numpy(flat)
    try:
        isz = vol.dtype.itemsize
        predicted = RC.bbox_vectorised(vol.shape, isz, (buf.ptr + off * isz) % 16)
        ctx.counters(reset=True)
        if off == 0:
            got = DevArray(ctx, buf, vol.shape, vol.dtype).nonzero_bbox()
        else:
            bb = (C.c_int * 6)()
            check(ctx.lib.boa_nonzero_bbox(ctx.h, C.c_void_p(buf.ptr + off * isz), RC.DTYPES.index(vol.dtype), (C.c_int * 3)(*vol.shape), bb),
                  "boa_nonzero_bbox")
            got = [[bb[0], bb[1]], [bb[2], bb[3]], [bb[4], bb[5]]]
        cnt = ctx.counters()
        after = buf.download(flat.shape, flat.dtype)
    finally:
        buf.free()
    assert cnt["bbox_vec"] == (1 if predicted else 0), (vol.shape, vol.dtype, lead, cnt["bbox_vec"], predicted)
    assert_same_bits(after, flat, "source after the call")
    return got, predicted


def check_bbox_patterns(ctx, shape, dtype, vec_when_aligned):
    from boa_hip.task import nonzero_bbox
    for name, vol in RC.bbox_patterns(shape, dtype).items():
        want = nonzero_bbox(vol)
        got, vec = run_bbox(ctx, vol, 0)
        assert vec == vec_when_aligned and got == want, (name, "aligned", got, want)
        if vec_when_aligned:                   # the same volume at a misaligned address: the per-element loop on a vectorisable shape
            got, vec = run_bbox(ctx, vol, RC.BBOX_LEAD[dtype.itemsize])
            assert not vec and got == want, (name, "misaligned", got, want)


@pytest.mark.parametrize("k", range(8))
@pytest.mark.parametrize("dtype", RC.BBOX_DTYPES, ids=lambda d: d.name)
def test_bbox_row_lengths(ctx, dtype, k):
    """rows of 16, 32, 48 and 1040 bytes (vector loop; and the per-element loop at a misaligned base) and of 16 k +- one element
    (per-element loop), each with a single voxel in every corner, on the first and the last element of a 16-byte chunk, in the last
    chunk of a row, pairs that alone decide one axis, nothing, only negative values, and for float32 -0.0, NaN and a subnormal"""
    d2, vec = RC.bbox_row_lengths(dtype)[k]
    check_bbox_patterns(ctx, (RC.D0, RC.D1, d2), dtype, vec)


@pytest.mark.parametrize("dtype", RC.BBOX_DTYPES, ids=lambda d: d.name)
def test_bbox_degenerate_row_split(ctx, dtype):
    """d1 = 1, d0 = 1 and both: the row number is the axis-0 index, the axis-1 index, or 0"""
    for shape in RC.bbox_degenerate_shapes(dtype):
        check_bbox_patterns(ctx, shape, dtype, True)


@pytest.mark.parametrize("dtype", RC.BBOX_DTYPES, ids=lambda d: d.name)
def test_bbox_more_rows_than_one_sweep(ctx, dtype):
    """more than two sweeps of the grid (32 rows per CU and sweep, the CU count read from the device): the first and the last row
    and two rows of the second sweep decide the box; with both loops"""
    vol, facts = RC.bbox_sweep_case(dtype, ctx.info()["cu_count"])
    assert facts["rows"] > 2 * facts["sweep"]
    got, vec = run_bbox(ctx, vol, 0)
    assert vec and got == facts["bbox"]
    got, vec = run_bbox(ctx, vol, RC.BBOX_LEAD[dtype.itemsize])
    assert not vec and got == facts["bbox"]


def test_bbox_float64_is_refused_and_the_context_survives(ctx):
    from boa_hip import _lib
    from boa_hip.devarray import DevArray
    from boa_hip.task import nonzero_bbox
    vol = RC.bbox_patterns((RC.D0, RC.D1, 8), np.dtype(np.float32))["lo_hi_axis2"].astype(np.float64)
    d = DevArray.from_numpy(ctx, vol)
    ctx.counters(reset=True)
    bb = (C.c_int * 6)(*([-7] * 6))
    rc = ctx.lib.boa_nonzero_bbox(ctx.h, d.buf.vp, 4, (C.c_int * 3)(*vol.shape), bb)
    assert rc == _lib.BOA_EINVAL
    msg = ctx.lib.boa_last_error().decode()
    assert "boa_nonzero_bbox" in msg and "dtype 4" in msg
    assert list(bb) == [-7] * 6 and ctx.counters()["bbox_vec"] == 0
    with pytest.raises(ValueError, match="dtype 4"):
        d.nonzero_bbox()
    # the context is still usable: the same values as float32 give their box
    v32 = vol.astype(np.float32)
    got, vec = run_bbox(ctx, v32, 0)
    assert vec and got == nonzero_bbox(v32) != [[0, n] for n in vol.shape]
    np.testing.assert_array_equal(d.download(), vol)
