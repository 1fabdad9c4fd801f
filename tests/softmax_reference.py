"""float64 model and the derived error bound of the class-probability arithmetic (csrc/softmax_codes.h), and the logit families
the host program (test_softmax_codes_host_cpu.py) and the kernels (test_gpu_probabilities.py) are fed with.  numpy only.

The bound, for fp16 logits and p64 = their float64 softmax:
    |p - p64| <= (C + 110) 2^-24 p64   where p64 > 2^-100,        |p - p64| <= 2^-99   elsewhere
(the rounded difference x - m inside exp: <= 104 2^-24 for a class that does not underflow; expf <= 2 ulp; C - 1 additions; one
division).  It comes from the number formats, not from any implementation's measured error."""
import numpy as np

F16 = np.float16
FLOOR_P = 2.0 ** -100
FLOOR_ABS = 2.0 ** -99


def rel_bound(C):
    return (C + 110) * 2.0 ** -24


def softmax64(h):
    """float64 softmax over axis 0 of fp16 logits (NaN columns come out NaN)."""
    x = np.asarray(h, dtype=F16).astype(np.float64)
    with np.errstate(invalid="ignore", under="ignore"):
        m = np.max(x, axis=0, keepdims=True)
        e = np.exp(x - m)
        return e / e.sum(axis=0, keepdims=True)


def bound_violations(p, p64, C):
    """-> (boolean array of violations, worst relative error in units of 2^-24, worst absolute error below the floor).  Columns
    with a NaN in p64 are not judged here."""
    p = np.asarray(p, dtype=np.float64)
    ok = ~np.isnan(p64).any(axis=0, keepdims=True) & np.ones(p64.shape, bool)
    big = ok & (p64 > FLOOR_P)
    small = ok & ~big
    err = np.abs(p - p64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(big, err / np.where(big, p64, 1.0), 0.0)
    bad = (big & ~(rel <= rel_bound(C))) | (small & ~(err <= FLOOR_ABS))
    return bad, float(rel.max(initial=0.0)) * 2.0 ** 24, float(np.where(small, err, 0.0).max(initial=0.0))


def assert_within_bound(p, p64, C, what=""):
    bad, rel, small = bound_violations(p, p64, C)
    print(f"{what}: C {C} worst relative error {rel:.2f} x 2^-24 (bound {C + 110}), worst error below the floor {small:.3g}")
    assert not bad.any(), f"{what}: {int(bad.sum())} probabilities outside the bound, worst relative error {rel:.2f} x 2^-24"
    return rel


def first_max(p):
    """The label rule: the first class whose p equals the maximum p; a NaN column gives 0 (no comparison with a NaN holds)."""
    p = np.asarray(p)
    lab = np.zeros(p.shape[1:], dtype=np.int64)
    best = p[0].copy()
    for c in range(1, p.shape[0]):
        up = p[c] > best
        lab[up] = c
        best = np.where(up, p[c], best)
    return lab


def assert_labels(labels, p, p64, C, what=""):
    """labels are exactly the first maximum of the RETURNED probabilities, and differ from the float64 argmax only where the float64
    top-two relative gap is within the bound."""
    labels = np.asarray(labels).astype(np.int64)
    np.testing.assert_array_equal(labels, first_max(p), err_msg=f"{what}: labels are not the first maximum of the probabilities")
    nan = np.isnan(p64).any(axis=0)
    want = np.where(nan, 0, np.argmax(np.where(np.isnan(p64), -1.0, p64), axis=0))
    diff = (labels != want) & ~nan
    if diff.any():
        top = np.take_along_axis(p64, want[None], 0)[0]
        mine = np.take_along_axis(p64, labels[None], 0)[0]
        gap = (top - mine) / top
        assert (gap[diff] <= rel_bound(C)).all(), f"{what}: {int((gap[diff] > rel_bound(C)).sum())} labels differ from float64 beyond a near-tie"
    return int(diff.sum())


def _next16(h, k=1):
    """The fp16 value k steps above a non-negative fp16 value."""
    return (np.asarray(h, dtype=F16).view(np.uint16) + np.uint16(k)).view(F16)


def families(C, n_random=48, seed=0):
    """fp16 logit columns [C, n]: noise at scales 0.5 / 8 / 60, all-equal columns, +-65504, subnormals, a top pair of adjacent
    fp16 values at 0 / 1 / 1024, exact ties of the maximum (the first must win).  No NaN (nan_columns has those)."""
    rng = np.random.default_rng(1000 * C + seed)
    cols = []
    for scale in (0.5, 8.0, 60.0):
        cols.append((rng.standard_normal((C, n_random)) * scale).astype(F16))
    eq = np.array([0.0, -0.0, 1.0, -3.5, 65504.0, -65504.0, 6e-8, 1024.0], dtype=F16)
    cols.append(np.broadcast_to(eq, (C, eq.size)).copy())
    ext = np.zeros((C, 6), dtype=F16)                       # +-65504 among ordinary values
    ext[:, 0] = -65504.0
    ext[C - 1, 0] = 65504.0
    ext[:, 1] = 65504.0
    ext[0, 1] = -65504.0
    ext[:, 2] = (rng.standard_normal(C) * 3).astype(F16)
    ext[C // 2, 2] = 65504.0
    ext[:, 3] = (rng.standard_normal(C) * 3).astype(F16)
    ext[C // 2, 3] = -65504.0
    ext[:, 4] = 65504.0
    ext[C - 1, 4] = 65472.0                                 # the fp16 value below the largest
    ext[:, 5] = -65504.0
    ext[0, 5] = -65472.0
    cols.append(ext)
    sub = rng.integers(0, 0x400, size=(C, 8)).astype(np.uint16)          # subnormals of both signs, and +-0
    sub |= (rng.integers(0, 2, size=(C, 8)).astype(np.uint16) << 15)
    cols.append(sub.view(F16))
    for base in (0.0, 1.0, 1024.0):                         # the two largest logits one fp16 step apart, at every pair of positions
        pair = np.full((C, 2 * min(C, 4)), -2.0, dtype=F16) + (rng.standard_normal((C, 2 * min(C, 4))) * 0.25).astype(F16)
        pair = np.minimum(pair, F16(-0.5)).astype(F16)
        for k in range(pair.shape[1]):
            i = (k * 7) % C
            j = (i + 1 + k) % C
            pair[i, k] = F16(base)
            if j != i:
                pair[j, k] = _next16(F16(base))
        cols.append(pair)
    tie = (rng.standard_normal((C, 12)) * 2).astype(F16)    # exact ties of the maximum at two or three positions
    for k in range(12):
        top = F16(np.max(tie[:, k].astype(np.float32)) + 1.0)
        for i in rng.choice(C, size=min(C, 2 + k % 2), replace=False):
            tie[i, k] = top
    cols.append(tie)
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def nan_columns(C):
    """[C, 3]: a NaN first, last, and (C > 1) in the middle of ordinary values."""
    x = np.linspace(-2, 2, C).astype(F16)
    cols = np.stack([x, x, x], axis=1)
    cols[0, 0] = np.nan
    cols[C - 1, 1] = np.nan
    cols[C // 2, 2] = np.nan
    return cols


def fill_volume(C, shape, seed=0):
    """fp16 logits [C, *shape] whose voxels run through families(C) (every family lands at many offsets of the row)."""
    cols = families(C, seed=seed)
    n = int(np.prod(shape))
    idx = (np.arange(n) * 5 + seed) % cols.shape[1]
    return np.ascontiguousarray(cols[:, idx].reshape(C, *shape))
