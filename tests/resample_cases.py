"""Case generators and reference one-liners of tests/test_gpu_resample_edges.py (the edge cases of csrc/resample.hip and of
`boa_ct_normalize`).  No device here: tests/test_resample_cases_cpu.py pins every generator against the property it states and
every reference against scipy / the oracle, so a GPU case can neither be skipped for a shape mismatch nor lose its bite."""
import numpy as np

F64, F32, F16 = np.float64, np.float32, np.float16


# ---- shapes -----------------------------------------------------------------------------------------------------------
def zoom_of(n_in, n_out):
    """The zoom handed to scipy.ndimage.zoom for n_in -> n_out samples; scipy's output length is round(n_in * zoom)."""
    return n_out / n_in


def zoomed_len(n_in, n_out):
    return int(round(n_in * zoom_of(n_in, n_out)))


def zoom_tuple(in_shape, out_shape):
    return tuple(zoom_of(i, o) for i, o in zip(in_shape, out_shape))


def nearest_index(n_in, n_out):
    """Source index of every output sample of `ndimage.zoom(order=0, mode="nearest")` (grid_mode False): the coordinate
    k * (n_in - 1) / (n_out - 1) (scipy's `where=zoom_div != 0` rule: factor 1.0 for a single output sample) rounded as
    floor(c + 0.5), clamped."""
    f = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
    return np.clip(np.floor(np.arange(n_out, dtype=F64) * f + 0.5), 0, n_in - 1).astype(np.int64)


def past_extent_pairs(max_in=64, max_out=96):
    """(n_in, n_out) whose last cubic coordinate (n_out - 1) * fl((n_in - 1) / (n_out - 1)) lands above n_in - 1 in fp64."""
    out = []
    for n_in in range(2, max_in + 1):
        for n_out in range(2, max_out + 1):
            if F64(n_out - 1) * (F64(n_in - 1) / F64(n_out - 1)) > F64(n_in - 1):
                out.append((n_in, n_out))
    return out


# A: the contiguous axis takes every length of CONTIG_LENGTHS; its padded length is Z + 24, so Z % 8 is the scalar tail
CONTIG_LENGTHS = tuple(range(2, 34))
LEAD = (3, 5)


def contig_residue_table(lengths=CONTIG_LENGTHS):
    """{(Z + 24) % 8: [Z, ...]} of the contiguous-axis lengths."""
    t = {}
    for z in lengths:
        t.setdefault((z + 24) % 8, []).append(z)
    return t


def contig_cases(z):
    """(in_shape, out_shape) of section A for one contiguous length: down and up on the last axis, leading dims untouched
    and resized."""
    down, up = max(1, 2 * z // 3), 2 * z + 1
    return [((*LEAD, z), (*LEAD, down)), ((*LEAD, z), (*LEAD, up)), ((*LEAD, z), (4, 4, down)), ((*LEAD, z), (2, 7, up))]


def amplitude_volume(shape, regime, seed):
    """fp64 volume: `noise` = Gaussian * 400; `step` = a +-30000 edge across the last axis (its position varies with the
    line, 15 % of the voxels flipped): the cubic overshoot leaves [-30000, 30000] by thousands."""
    rng = np.random.default_rng(seed)
    if regime == "noise":
        return rng.normal(size=shape) * 400
    assert regime == "step"
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    edge = np.where(z + (x + y) % 3 > shape[2] // 2, 30000.0, -30000.0)
    edge[rng.random(shape) < 0.15] *= -1
    return edge


# B: cubic geometry edges (in_shape, out_shape)
CUBIC_GEOMETRY = {
    "out1_axis0": ((6, 5, 7), (1, 5, 7)),
    "out1_axis1": ((6, 5, 7), (6, 1, 9)),
    "out1_axis2": ((6, 5, 7), (4, 5, 1)),
    "out1_all": ((6, 5, 7), (1, 1, 1)),
    "out2": ((6, 5, 7), (2, 2, 2)),
    "in2_all": ((2, 2, 2), (5, 3, 2)),
    "in2_axis2": ((5, 4, 2), (5, 4, 9)),
    "in2_to1": ((2, 2, 2), (1, 2, 1)),
    "up8": ((5, 4, 3), (40, 32, 24)),
    "identity": ((7, 6, 9), (7, 6, 9)),
}


def past_extent_cases():
    """every pair of past_extent_pairs() on each axis in turn; the other two axes 3 -> 3 and 4 -> 5"""
    out = []
    for n_in, n_out in past_extent_pairs():
        for ax in range(3):
            i, o = [3, 4], [3, 5]
            i.insert(ax, n_in)
            o.insert(ax, n_out)
            out.append((tuple(i), tuple(o)))
    return out


# C: nearest sweep
NEAREST_IN = range(1, 40)
NEAREST_OUT = range(1, 60)


def all_zoom_shape_pairs():
    """every (n_in, n_out) an `ndimage.zoom(x, n_out / n_in)` reference of the GPU test is asked for"""
    pairs = set()
    for z in CONTIG_LENGTHS:
        for i, o in contig_cases(z):
            pairs.update(zip(i, o))
    for i, o in list(CUBIC_GEOMETRY.values()) + past_extent_cases():
        pairs.update(zip(i, o))
    pairs.update((a, b) for a in NEAREST_IN for b in NEAREST_OUT)
    return sorted(pairs)


# ---- E: double -> half, one rounding against two ------------------------------------------------------------------------
def _pair(a, b):
    """plane values (a, b) of class 0 and the constant of class 1 = the larger of the once- and the twice-rounded value: the
    smaller one loses to class 1, the larger one ties with it and wins as the first maximum"""
    t = F64(0.75) * F64(a) + F64(0.25) * F64(b)
    once, twice = t.astype(F16), t.astype(F32).astype(F16)
    return float(a), float(b), float(max(once, twice))


# 0.75 a is the half-way point of two neighbouring halves and 0.25 b a nudge off it that fp64 keeps and float32 drops (b = a
# tiny half, mostly the smallest subnormal): rounded once the nudge decides, rounded twice the exact tie goes to the even
# neighbour, which lies on the other side.  a = 1366 * 2^s: even half below the tie, 1370 * 2^s: even half above it.
HALF_PAIRS = tuple(_pair(a, b) for a, b in [
    (1366.0, 2.0 ** -24),            # the issue's case: 1024.5 + 2^-26 -> 1025 once, 1024 twice
    (1370.0, -2.0 ** -24),           # mirrored: 1027.5 - 2^-26 -> 1027 once, 1028 twice
    (-1366.0, -2.0 ** -24),          # negative sign
    (-1370.0, 2.0 ** -24),
    (1366.0 / 1024, 2.0 ** -24),     # binade [1, 2)
    (1370.0 / 1024, -2.0 ** -24),
    (1366.0 * 16, 2.0 ** -24),       # binade [2^14, 2^15)
    (-1370.0 * 16, 2.0 ** -24),
    (1366.0 * 2, 2.0 ** -14),        # b = the smallest normal half
    (1366.0 / 256, 3 * 2.0 ** -24),
])


def half_rounding_case(pair=HALF_PAIRS[0]):
    """fp16 logits [2][2][3][3]: class 0 plane 0 = a, plane 1 = b, class 1 constant; resized 2 -> 4 along axis 0 (order 1).  At
    output plane 1 class 0 is 0.75 a + 0.25 b.  Returns three arrangements of the same numbers as dicts {logits, out, axis}:
    3-D, and separate-z (the resized axis in-plane) with the slice axis before / after the resized axis."""
    a, b, c1 = pair
    lg = np.empty((2, 2, 3, 3), F16)
    lg[0, 0], lg[0, 1], lg[1] = a, b, c1
    assert float(lg[0, 0, 0, 0]) == a and float(lg[0, 1, 0, 0]) == b and float(lg[1, 0, 0, 0]) == c1   # exact in half
    t = np.ascontiguousarray(lg.transpose(0, 2, 1, 3))                      # [2][3][2][3]: resized axis is axis 1
    return [dict(logits=lg, out=(4, 3, 3), axis=-1, resized=0),
            dict(logits=t, out=(3, 4, 3), axis=0, resized=1),
            dict(logits=t, out=(3, 4, 3), axis=2, resized=1)]


def oracle_logits(arr, dtype=F16):
    """the oracle's resized logits of one arrangement, in `dtype` (float64: before any rounding)"""
    from oracle import nnunet_resample as nnr
    ax = arr["axis"]
    return nnr.resample_data_or_seg(np.ascontiguousarray(arr["logits"].astype(dtype)), arr["out"], ax if ax >= 0 else None, 1,
                                    ax >= 0, 0)


# ---- D: per-slice value ranges ------------------------------------------------------------------------------------------
def slice_range_volume(shape, axis, seed):
    """float32: slice s along `axis` = Gaussian * 10^(s % 5) + (-1)^s * 3 * 10^(s % 5)"""
    rng = np.random.default_rng(seed)
    s = np.arange(shape[axis])
    sh = [1, 1, 1]
    sh[axis] = -1
    scale = (10.0 ** (s % 5)).reshape(sh)
    sign = np.where(s % 2 == 0, 1.0, -1.0).reshape(sh)
    return (rng.standard_normal(shape) * scale + sign * 3 * scale).astype(F32)


# (in_shape, out_shape, slice_axis): no in-plane size is a multiple of 8, so the 8-voxel runs of the min/max kernel cross slices
SLICE_CLIP_CASES = [
    ((11, 9, 13), (11, 13, 10), 0), ((11, 9, 13), (17, 7, 19), 0), ((11, 9, 13), (5, 12, 9), 0),
    ((9, 12, 7), (13, 12, 10), 1), ((9, 12, 7), (6, 17, 11), 1), ((9, 12, 7), (11, 5, 5), 1),
    ((7, 6, 13), (9, 5, 13), 2), ((7, 6, 13), (10, 9, 21), 2), ((7, 6, 13), (5, 8, 6), 2),
    ((1, 9, 7), (1, 12, 5), 0), ((1, 9, 7), (3, 12, 5), 0), ((5, 1, 7), (7, 2, 9), 1), ((5, 6, 1), (4, 9, 1), 2),
    ((1, 2, 3), (1, 3, 5), 0), ((3, 1, 2), (4, 2, 3), 1), ((3, 3, 3), (4, 3, 5), 2), ((2, 2, 1), (3, 3, 2), 2),
]


# ---- F: CTNormalization ---------------------------------------------------------------------------------------------------
def ct_normalize_ref(x, mean, sd, lo, hi):
    """float32 throughout, the scalars as float32: clip, subtract, divide by max(sd, 1e-8)"""
    v = np.clip(x.astype(F32), F32(lo), F32(hi))
    v = v - F32(mean)
    return v / F32(max(sd, 1e-8))
