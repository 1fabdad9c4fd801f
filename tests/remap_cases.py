"""Cases of tests/test_gpu_index_remap.py: the strided copy `boa_copy3` (csrc/morph.hip: the LDS-tiled transpose `k_copy3_t` and the
element-wise `k_copy3`) and the bounding box `boa_nonzero_bbox` (`k_nonzero_bbox`: a 16-byte vector loop and a per-element loop).
numpy only, no device: every generator returns its buffers together with the facts the case is built to have (which kernel has to run,
that every address lies inside the buffers, that numpy's conversion of its values is defined), and tests/test_remap_cases_cpu.py proves
those facts before a case reaches a GPU.

A copy case is a dict: `src` (the whole source buffer, 1-D), `in_off` / `in_strides` (elements) and `shape` of the view that is read;
`dst` (the whole destination buffer, 1-D, every byte 0xAA), `out_off` / `out_strides` of the view that is written; `axis` = the output
axis A along which `k_copy3_t` reads contiguously, or None where `k_copy3` has to run; `src_ops` / `dst_ops` = the same views as calls of
DevArray.transpose / flip / slice on a contiguous 3-D array of `src_base_shape` / `dst_base_shape`, or None where only explicit strides
can express the view.  The reference is numpy on the same views: `expected_dst`."""
import functools
import zlib

import numpy as np
from numpy.lib.stride_tricks import as_strided

DTYPES = (np.dtype(np.uint8), np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float32), np.dtype(np.float64))   # dtype codes 0 .. 4
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
TILE = 64                        # k_copy3_t moves 64 x 64 tiles of the (A, 2) plane
T_MIN = 16                       # smallest extent on A and on axis 2 for which copy3_out picks k_copy3_t
GRID_MAX = 65535                 # grid limit of blockIdx.y / blockIdx.z


def bits(a):
    """the array's bit patterns as unsigned integers: NaN payloads and the sign of zero count in a comparison"""
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype.itemsize])


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- the two path rules, mirrored from csrc/morph.hip ----------------------------------------------------------------------------
def copy3_axis(shape, in_strides, out_strides):
    """copy3_out: the output axis A (1 before 0) that k_copy3_t reads contiguously, or None where k_copy3 runs (or nothing, for an
    empty shape)"""
    d, s, t = shape, in_strides, out_strides
    if d[0] * d[1] * d[2] == 0:
        return None
    A = None
    if abs(t[2]) == 1 and abs(s[2]) != 1 and d[2] >= T_MIN:
        if abs(s[1]) == 1 and d[1] >= T_MIN:
            A = 1
        elif abs(s[0]) == 1 and d[0] >= T_MIN:
            A = 0
    if A is None or d[1 - A] > GRID_MAX or (d[2] + TILE - 1) // TILE > GRID_MAX:
        return None
    return A


def copy3_transposed(shape, in_strides, out_strides):
    return copy3_axis(shape, in_strides, out_strides) is not None


def bbox_vectorised(shape, itemsize, base_misalignment):
    """boa_nonzero_bbox: the 16-byte loop needs rows that start on 16-byte boundaries; `base_misalignment` = address of the first
    voxel modulo 16"""
    if shape[0] * shape[1] * shape[2] == 0:
        return False
    return base_misalignment % 16 == 0 and (shape[2] * itemsize) % 16 == 0


# ---- views -----------------------------------------------------------------------------------------------------------------------
def geometry(base, view):
    """(offset, strides) in elements of a numpy view of `base`"""
    isz = base.itemsize
    delta = view.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    assert delta % isz == 0 and all(s % isz == 0 for s in view.strides)
    return delta // isz, tuple(s // isz for s in view.strides)


def view_of(flat, off, shape, strides):
    """the (offset, strides) view of a 1-D buffer, the way k_copy3 addresses it"""
    isz = flat.itemsize
    return as_strided(flat[off:], shape, tuple(s * isz for s in strides))


def address_range(off, shape, strides):
    """(lowest, highest) element a view addresses"""
    lo = off + sum(min(0, (d - 1) * s) for d, s in zip(shape, strides))
    hi = off + sum(max(0, (d - 1) * s) for d, s in zip(shape, strides))
    return lo, hi


def apply_ops(v, ops):
    """the view ops on a numpy array; the GPU test applies the same list to a DevArray"""
    for op in ops:
        if op[0] == "transpose":
            v = v.transpose(op[1])
        elif op[0] == "flip":
            v = np.flip(v, op[1])
        elif op[0] == "slice":
            sl = [slice(None)] * 3
            sl[op[1]] = slice(op[2], op[3])
            v = v[tuple(sl)]
        else:
            raise ValueError(op)
    return v


def distinct(n, dtype, rng):
    """n values of which no two are equal (uint8: seeded noise), in seeded order: a misplaced element cannot go unnoticed"""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    assert dtype != np.int16 or n <= 65536
    return (rng.permutation(n) - n // 2).astype(dtype)


def aa(n, dtype):
    """n elements with every byte 0xAA"""
    return np.full(n * np.dtype(dtype).itemsize, 0xAA, np.uint8).view(dtype)


def expected_dst(case):
    """the whole destination buffer after the copy, by numpy: dst[view] = src[view].astype(out dtype)"""
    want = case["dst"].copy()
    src = view_of(case["src"], case["in_off"], case["shape"], case["in_strides"])
    with np.errstate(all="ignore"):          # float64 -> float32 overflows to inf on purpose
        view_of(want, case["out_off"], case["shape"], case["out_strides"])[...] = src.astype(want.dtype)
    return want


def _case(name, src_base, src_view, dst_base, dst_view, axis, src_ops=None, dst_ops=None, **facts):
    assert src_view.shape == dst_view.shape
    in_off, in_strides = geometry(src_base, src_view)
    out_off, out_strides = geometry(dst_base, dst_view)
    return dict(name=name, src=src_base.reshape(-1), in_off=in_off, in_strides=in_strides, shape=tuple(src_view.shape),
                dst=dst_base.reshape(-1), out_off=out_off, out_strides=out_strides, axis=axis,
                src_ops=src_ops, dst_ops=dst_ops, src_base_shape=src_base.shape, dst_base_shape=dst_base.shape, **facts)


# ---- boa_copy3: views built from transposes, boxes and flips ---------------------------------------------------------------------
PERM = {1: (0, 2, 1), 0: (2, 1, 0)}      # the source is a contiguous array seen through this transpose: its last axis is output axis A
NOPAD = ((0, 0),) * 3


def out_shape(A, dA, d2, dC):
    return (dC, dA, d2) if A == 1 else (dA, dC, d2)


def permuted_case(name, A, shape, dtype=np.int16, out_dtype=None, src_pad=NOPAD, dst_pad=NOPAD, src_flips=(), dst_flips=(), axis="A"):
    """output `shape` read from a contiguous array transposed by PERM[A] (its last axis becomes output axis A), boxed by `src_pad`
    = (before, after) per OUTPUT axis and flipped along `src_flips`; written into a box of a contiguous array (`dst_pad`), through
    a view flipped along `dst_flips`"""
    rng = _rng(name)
    dtype = np.dtype(dtype)
    out_dtype = dtype if out_dtype is None else np.dtype(out_dtype)
    perm = PERM[A]
    padded = [n + a + b for n, (a, b) in zip(shape, src_pad)]
    base_shape = [0, 0, 0]
    for i, p in enumerate(perm):
        base_shape[p] = padded[i]
    src_base = distinct(int(np.prod(base_shape)), dtype, rng).reshape(base_shape)
    src_ops = [("transpose", perm)] + [("slice", i, a, a + n) for i, (n, (a, b)) in enumerate(zip(shape, src_pad)) if a or b]
    src_ops += [("flip", ax) for ax in src_flips]
    dst_shape = [n + a + b for n, (a, b) in zip(shape, dst_pad)]
    dst_base = aa(int(np.prod(dst_shape)), out_dtype).reshape(dst_shape)
    dst_ops = [("slice", i, a, a + n) for i, (n, (a, b)) in enumerate(zip(shape, dst_pad)) if a or b] + [("flip", ax) for ax in dst_flips]
    return _case(name, src_base, apply_ops(src_base, src_ops), dst_base, apply_ops(dst_base, dst_ops), A if axis == "A" else axis,
                 src_ops=src_ops, dst_ops=dst_ops)


# (extent on A, extent on axis 2, third extent): a single 16 x 16 tile; one full tile; partial tiles on A, on axis 2, on both, next to
# full ones (65 = 64 + 1, 130 = 2 * 64 + 2, 63 and 17 = one partial tile)
T_PAIRS = ((16, 16, 3), (64, 64, 1), (17, 130, 3), (130, 17, 1), (65, 63, 3), (63, 65, 1))
SIGN_EXTENTS = (65, 17, 3)       # two tiles on A (one of them a single row), a partial tile on axis 2


def _strided_case(name, n_src, in_off, shape, in_strides, axis):
    """a source view that only explicit strides express (overlapping rows, broadcast axes), copied into a contiguous destination"""
    src_base = distinct(n_src, np.int16, _rng(name))
    dst_base = aa(shape[0] * shape[1] * shape[2], np.int16).reshape(shape)
    return _case(name, src_base, view_of(src_base, in_off, shape, in_strides), dst_base, dst_base, axis)


@functools.lru_cache(maxsize=None)
def copy_cases():
    """{name: case} of every view case of boa_copy3 but the grid-limit cases and the dtype matrix (built once per process)"""
    out = {}

    def add(c):
        assert c["name"] not in out
        out[c["name"]] = c

    for A in (1, 0):
        # tiles: full, partial on either side, a single 16 x 16 one
        for dA, d2, dC in T_PAIRS:
            add(permuted_case(f"tiles_A{A}_{dA}x{d2}x{dC}", A, out_shape(A, dA, d2, dC)))
        shape = out_shape(A, *SIGN_EXTENTS)
        C = 1 - A
        # sign of the unit strides; negative non-unit strides on the other axes
        add(permuted_case(f"flipped_source_A{A}", A, shape, src_flips=(A,)))                      # in stride -1 on A
        add(permuted_case(f"flipped_destination_A{A}", A, shape, dst_flips=(2,)))                 # out stride -1 on axis 2
        add(permuted_case(f"negative_outer_strides_A{A}", A, shape, src_flips=(2, C), dst_flips=(A, C)))
        add(permuted_case(f"all_flipped_A{A}", A, shape, src_flips=(0, 1, 2), dst_flips=(0, 1, 2)))
        # boxes inside larger buffers: offsets and pitches; the last element of both buffers; element 0 of both buffers (through
        # flipped views, so that the offsets are still not 0)
        add(permuted_case(f"box_inner_A{A}", A, shape, out_dtype=np.int32, src_pad=((1, 2), (3, 1), (2, 5)), dst_pad=((2, 1), (1, 3), (4, 2))))
        add(permuted_case(f"box_last_A{A}", A, shape, src_pad=((2, 0), (3, 0), (1, 0)), dst_pad=((1, 0), (2, 0), (5, 0))))
        add(permuted_case(f"box_first_A{A}", A, shape, src_pad=((0, 1), (0, 2), (0, 3)), dst_pad=((0, 2), (0, 1), (0, 4)),
                          src_flips=(A,), dst_flips=(2,)))
        # just outside the rule: k_copy3 has to run
        add(permuted_case(f"outside_15_on_A_A{A}", A, out_shape(A, 15, 33, 3), axis=None))
        add(permuted_case(f"outside_15_on_axis2_A{A}", A, out_shape(A, 17, 15, 3), axis=None))
        shape = out_shape(A, 17, 33, 3)
        rng = _rng(f"outside_out_stride_2_A{A}")
        src_base = distinct(17 * 33 * 3, np.int16, rng).reshape([shape[p] for p in PERM[A]])
        dst_base = aa(17 * 33 * 3 * 2, np.int16).reshape(shape[0], shape[1], 2 * shape[2])
        add(_case(f"outside_out_stride_2_A{A}", src_base, src_base.transpose(PERM[A]), dst_base, dst_base[:, :, ::2], None))
    # a plain copy: input stride 1 on axis 2
    src_base = distinct(3 * 17 * 33, np.int16, _rng("outside_plain_copy")).reshape(3, 17, 33)
    dst_base = aa(3 * 17 * 33, np.int16).reshape(3, 17, 33)
    add(_case("outside_plain_copy", src_base, src_base, dst_base, dst_base, None, src_ops=[], dst_ops=[]))
    # priority: both input axes 0 and 1 have stride +-1 and extents >= 16 (overlapping rows): axis 1 is taken; one launch either way
    add(_strided_case("priority_both_unit", 16 + 17 + 32 * 40 + 1, 0, (17, 18, 33), (1, 1, 40), 1))
    add(_strided_case("priority_unit_and_minus_unit", 16 + 17 + 32 * 40 + 1, 17, (17, 18, 33), (1, -1, 40), 1))
    # broadcasts: stride 0 on the batch axis; stride 0 on axis 1 of 16 with axis 0 contiguous: axis 1 does not qualify, axis 0 does
    add(_strided_case("broadcast_batch_A1", 17 * 33, 0, (3, 17, 33), (0, 1, 17), 1))
    add(_strided_case("broadcast_batch_A0", 17 * 33, 0, (17, 3, 33), (1, 0, 17), 0))
    add(_strided_case("broadcast_axis1_of_16_A0", 17 * 33, 0, (17, 16, 33), (1, 0, 17), 0))
    return out


def _copy_names():
    out = []
    for A in (1, 0):
        out += [f"tiles_A{A}_{a}x{b}x{c}" for a, b, c in T_PAIRS]
        out += [f"{k}_A{A}" for k in ("flipped_source", "flipped_destination", "negative_outer_strides", "all_flipped", "box_inner",
                                      "box_last", "box_first", "outside_15_on_A", "outside_15_on_axis2", "outside_out_stride_2")]
    return tuple(out) + ("outside_plain_copy", "priority_both_unit", "priority_unit_and_minus_unit", "broadcast_batch_A1",
                         "broadcast_batch_A0", "broadcast_axis1_of_16_A0")


COPY_NAMES = _copy_names()

GRID_BATCHES = (65535, 65536)    # blockIdx.z = the batch axis: the last extent k_copy3_t takes, the first it does not
GRID_TILE_ROWS = (64 * 65535, 64 * 65535 + 1)    # blockIdx.y = 64-wide tiles along axis 2: the same for the second limit (64 MiB buffers)


def grid_limit_case(n):
    """uint8, read along output axis 0 (the whole-volume (x,y,z) -> (z,y,x) view change): (16, n, 16) for the batch limit, 16 MiB per
    buffer; (16, 1, n) for the limit on the tiles along axis 2"""
    name = f"grid_{n}"
    shape = (16, n, 16) if n in GRID_BATCHES else (16, 1, n)
    size = shape[0] * shape[1] * shape[2]
    src_base = distinct(size, np.uint8, _rng(name)).reshape(shape[::-1])
    dst_base = aa(size, np.uint8).reshape(shape)
    ops = [("transpose", PERM[0])]
    axis = 0 if shape[1] <= GRID_MAX and -(-shape[2] // TILE) <= GRID_MAX else None
    return _case(name, src_base, apply_ops(src_base, ops), dst_base, dst_base, axis, src_ops=ops, dst_ops=[])


# ---- boa_copy3: the dtype matrix -------------------------------------------------------------------------------------------------
MATRIX_SHAPES = {"t": (3, 17, 33), "e": (3, 5, 7)}     # k_copy3_t (A = 1) and k_copy3, both through the PERM[1] transpose
F32_MAX = float(np.finfo(np.float32).max)


def _specials(i, o):
    """values of dtype i whose conversion to dtype o says something (and is defined)"""
    i, o = np.dtype(i), np.dtype(o)
    if i.kind in "iu":
        ii = np.iinfo(i)
        v = [0, 1, ii.max, ii.min, ii.max - 1, ii.min + 1]
        if i == np.int16:
            v += [-1, 255, 256, 128, 127, -128, -129, -256, -255, 0x0100, 0x7F00]
        if i == np.int32:
            v += [-1, 255, 256, 128, -129, 70000, -70000, 32767, 32768, -32768, -32769, 65535, 65536, 0x00010000, 0x7FFF0000,
                  2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, -(2 ** 24 + 1), -(2 ** 24 + 3), 2 ** 25 + 2, 2 ** 25 + 6,
                  2 ** 31 - 1, 2 ** 31 - 64, 2 ** 31 - 65, 2 ** 31 - 128, -(2 ** 31) + 1, 123456789]
        if i == np.uint8:
            v += [127, 128, 129, 254]
        return np.array(v, np.int64).astype(i)
    if o.kind in "iu":
        # float -> int: fractions of both signs, strictly inside the target range (uint8: none below 0, and no -0.0 either)
        oi = np.iinfo(o)
        v = [0.0, 0.25, 0.5, 0.75, 0.999, 1.0, 1.5, 2.5, 3.5, 126.5, 127.5, 128.5, 254.5, 254.999]
        if oi.min < 0:
            v += [-x for x in v] + [-0.0]
        if o == np.int16 or o == np.int32:
            v += [255.5, 256.5, -255.5, -256.5, 32766.5, -32767.5, 32766.998, -32767.998, 1e-30, -1e-30]
        if o == np.int32:
            v += [32767.5, 32768.5, -32768.5, 65535.5, 8388607.5, -8388607.5, 16777215.0, -16777216.0, 2147483520.0, -2147483520.0]
            if i == np.float64:
                v += [2147483646.999, -2147483647.999, 2147483646.5, 16777216.5, -16777217.5, 4294967.296]
        return np.array(v, i)
    if i == np.float64 and o == np.float32:
        u = 2.0 ** -24                   # half an ulp of float32 at 1.0
        v = [1.0 + u, 1.0 + 3 * u, 1.0 + 5 * u, 1.0 + u + 2.0 ** -50, 1.0 + u - 2.0 ** -50, -(1.0 + u), -(1.0 + 3 * u),      # ties, and next to them
             1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -150, 0.75 * 2.0 ** -149, 2.0 ** -126 * (1 - 2.0 ** -25), 1e-50, -1e-50,   # subnormal, or 0
             3.5e38, -3.5e38, 1e300, -1e300, F32_MAX, -F32_MAX, F32_MAX * (1 + 2.0 ** -25), (2 - 2.0 ** -24) * 2.0 ** 127,          # overflow: inf
             (2 - 2.0 ** -24) * 2.0 ** 127 * (1 - 2.0 ** -53),
             0.0, -0.0, np.inf, -np.inf, np.nan, 0.1, -0.1, 1 / 3, np.pi, 65504.0, 1e-5]
        return np.array(v, np.float64)
    if i == np.float32 and o == np.float64:
        v = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, 2.0 ** -126, F32_MAX, -F32_MAX, 0.1, 1 / 3, np.pi, 1.0 + 2.0 ** -23]
        return np.array(v, np.float32)
    # the same float type: every bit pattern passes
    if i == np.float32:
        return np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FC12345,
                         0x7FA55AA5, 0xFFFFFFFF, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x3F800000], np.uint32).view(np.float32)
    return np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000,
                     0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FF8000012345678, 0x7FF4AAAA5555AAAA,
                     0xFFFFFFFFFFFFFFFF, 0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x0010000000000000,
                     0x7FEFFFFFFFFFFFFF, 0x3FF0000000000000], np.uint64).view(np.float64)


def _filler(i, o, n, rng):
    """seeded values for the rest of the volume, with the same guarantees"""
    i, o = np.dtype(i), np.dtype(o)
    if i.kind in "iu":
        ii = np.iinfo(i)
        return rng.integers(ii.min, ii.max, n, dtype=np.int64, endpoint=True).astype(i)
    if o.kind in "iu":
        oi = np.iinfo(o)
        lo, hi = (0.0, 254.0) if oi.min == 0 else (max(oi.min, -2.0 ** 30) + 1.0, min(oi.max, 2.0 ** 30) - 1.0)
        scale = rng.choice(np.array([1.0, 1e-2, 1e-4]), n)         # small and large magnitudes, all with fractions
        v = (rng.uniform(lo, hi, n) * scale).astype(i)
        return v
    if i == o:
        return rng.integers(0, 2 ** (8 * i.itemsize), n, dtype=BITS[i.itemsize], endpoint=False).view(i)
    return (rng.standard_normal(n) * 10.0 ** rng.integers(-42, 39, n)).astype(i) if i == np.float64 else \
        (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32)


def matrix_values(i, o, n):
    """n values of dtype i for the conversion to o: the special values first, seeded filler after them"""
    sp = _specials(i, o)
    assert len(sp) <= n, (i, o, len(sp))
    return np.concatenate([sp, _filler(i, o, n - len(sp), _rng(f"matrix_{np.dtype(i)}_{np.dtype(o)}"))]).astype(i, copy=False)


def conversion_defined(values, o):
    """numpy's (and C++'s) conversion of these values to dtype o is defined: anything but a float -> int conversion, or finite
    values strictly inside the integer range (uint8: from +0.0 on, no negative sign at all)"""
    o = np.dtype(o)
    if values.dtype.kind != "f" or o.kind == "f":
        return True
    oi = np.iinfo(o)
    v = values.astype(np.float64)
    if not np.isfinite(v).all() or not (v < oi.max).all():
        return False
    return bool((v > oi.min).all()) if oi.min < 0 else not np.signbit(v).any()


def matrix_case(kernel, i, o):
    """dtype i -> o through k_copy3_t (kernel "t") or k_copy3 ("e")"""
    i, o = np.dtype(i), np.dtype(o)
    shape = MATRIX_SHAPES[kernel]
    n = shape[0] * shape[1] * shape[2]
    src_base = matrix_values(i, o, n).reshape([shape[p] for p in PERM[1]])
    dst_base = aa(n, o).reshape(shape)
    ops = [("transpose", PERM[1])]
    return _case(f"matrix_{kernel}_{i}_{o}", src_base, apply_ops(src_base, ops), dst_base, dst_base, 1 if kernel == "t" else None,
                 src_ops=ops, dst_ops=[])


# ---- boa_nonzero_bbox ------------------------------------------------------------------------------------------------------------
BBOX_DTYPES = DTYPES[:4]
BBOX_LEAD = {1: 5, 2: 3, 4: 1}     # elements in front of a misaligned volume: 5, 6 and 4 bytes
BBOX_GUARD = 32                    # non-zero elements after every volume: a read past the end would widen the box
D0, D1 = 4, 5


def bbox_row_lengths(dtype):
    """[(d2, the 16-byte loop applies to an aligned volume)]: rows of 16, 32 and 48 bytes and one of 65 chunks (a lane takes two);
    rows of 16 k +- one element for k = 1 and 65"""
    isz = np.dtype(dtype).itemsize
    E = 16 // isz
    return [(E, True), (2 * E, True), (3 * E, True), (65 * E, True), (E - 1, False), (E + 1, False), (65 * E - 1, False), (65 * E + 1, False)]


def _nonzero_values(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return [1, 255, 128, 16]
    if dtype == np.int16:
        return [1, -1, 0x0100, -32768, 0x7F00]
    if dtype == np.int32:
        return [1, -1, 0x00010000, -2 ** 31, 0x01000000, 0x0000FF00]
    return [1.0, -1.0, np.inf, -2.5, 1e-30, -np.inf]


def bbox_patterns(shape, dtype):
    """{name: volume}: what decides a box on this shape.  Each volume's box follows from `boa_hip.task.nonzero_bbox`; the CPU test
    pins the ones that are known by construction."""
    dtype = np.dtype(dtype)
    d0, d1, d2 = shape
    E = 16 // dtype.itemsize
    vals = _nonzero_values(dtype)
    out = {"zeros": np.zeros(shape, dtype)}

    def single(name, pos, k=0):
        v = np.zeros(shape, dtype)
        v[pos] = vals[k % len(vals)]
        out[name] = v

    for k, (z, y, x) in enumerate([(z, y, x) for z in (0, d0 - 1) for y in (0, d1 - 1) for x in (0, d2 - 1)]):
        single(f"corner_{int(z > 0)}{int(y > 0)}{int(x > 0)}", (z, y, x), k)
    cm = (d2 // E) // 2                                   # a chunk in the middle of the row (chunk 0 of a one-chunk row)
    single("chunk_first_element", (d0 // 2, d1 // 2, min(cm * E, d2 - 1)), 1)
    single("chunk_last_element", (d0 // 2, d1 // 2, min(cm * E + E - 1, d2 - 1)), 2)
    single("last_chunk_of_row", (d0 - 1, 1 % d1, max(d2 - E, 0)), 3)
    # two voxels that alone set lo and hi of one axis
    mid = [d0 // 2, d1 // 2, d2 // 2]
    for ax, n in enumerate(shape):
        a, b = (1, n - 2) if n > 3 else (0, n - 1)
        v = np.zeros(shape, dtype)
        for q, c in enumerate((a, b)):
            p = list(mid)
            p[ax] = c
            v[tuple(p)] = vals[(ax + q) % len(vals)]
        out[f"lo_hi_axis{ax}"] = v
    # only "negative" values: the sign bit and nothing else decides nothing (uint8: the high bit)
    v = np.zeros(shape, dtype)
    blk = v[d0 // 4:d0 - d0 // 4, 1 % d1:max(d1 - 1, 1 % d1 + 1), 2:max(d2 - 1, 3)]
    ramp = np.arange(blk.size).reshape(blk.shape) % 100 + 1
    blk[...] = (ramp + 128 if dtype == np.uint8 else -ramp).astype(dtype)
    out["only_negative"] = v
    if dtype == np.float32:
        out["all_negative_zero"] = np.full(shape, -0.0, np.float32)
        v = np.full(shape, -0.0, np.float32)
        v[d0 // 2, d1 // 2, min(cm * E + 1, d2 - 1)] = 1.5      # -0.0 on both sides in the same chunk
        out["negative_zero_around_a_value"] = v
        v = np.zeros(shape, np.float32)
        v[::2] = -0.0
        v[1 % d0, d1 // 2, d2 // 3] = np.nan
        out["nan_is_nonzero"] = v
        v = np.zeros(shape, np.float32)
        v[d0 - 1, 0, d2 - 1] = np.float32(1e-45)                # the smallest subnormal: != 0 in numpy
        out["subnormal_is_nonzero"] = v
    return out


def bbox_embed(vol, lead):
    """(buffer, element offset of the volume): `lead` non-zero elements, the volume, BBOX_GUARD non-zero elements"""
    one = np.ones(1, vol.dtype)
    return np.concatenate([np.repeat(one, lead), vol.reshape(-1), np.repeat(one, BBOX_GUARD)]), lead


def bbox_sweep_case(dtype, cu_count):
    """more rows than one sweep of the grid covers: the grid is min(rows / 4, 8 * CUs) blocks of four waves, one row per wave, so a
    sweep is 32 * CUs rows.  Rows of 16 elements.  Returns (volume, facts): the first and the last row decide axes 0 and 1,
    two rows of the second sweep decide axis 2 (the box is not the whole volume, which is also the answer for "nothing found")."""
    dtype = np.dtype(dtype)
    sweep = 32 * cu_count
    d1, d2 = 33, 16
    d0 = -(-(2 * sweep + 40) // d1)
    rows = d0 * d1
    vol = np.zeros((d0, d1, d2), dtype)
    vals = _nonzero_values(dtype)
    r_lo, r_hi = sweep + 7, 2 * sweep - 3                 # rows of the second sweep
    vox = {"first_row": (0, 0, 5), "last_row": (d0 - 1, d1 - 1, 9), "second_sweep_lo2": (*divmod(r_lo, d1), 3),
           "second_sweep_hi2": (*divmod(r_hi, d1), 13)}
    for k, p in enumerate(vox.values()):
        vol[p] = vals[k % len(vals)]
    return vol, dict(rows=rows, sweep=sweep, voxels=vox, bbox=[[0, d0], [0, d1], [3, 14]])


def bbox_degenerate_shapes(dtype):
    """d1 = 1 and d0 = 1 (the row -> (axis 0, axis 1) split degenerates), rows of 48 bytes; both at once"""
    E = 16 // np.dtype(dtype).itemsize
    return [(37, 1, 3 * E), (1, 37, 3 * E), (1, 1, 3 * E)]
