"""Adversarial z-slab cuts for the sharded connected-component engine (boa_hip/agg_shard.py): an in-process communicator that drives
the protocol's collectives for every rank inside one process, explicit cut plans (every plane its own slab, more ranks than planes,
cuts on / one before / one after a 16-plane CCL tile boundary, an empty slab between two others), and masks whose components only
exist through a slab interface.  numpy only, no device: tests/test_agg_shard_cases_cpu.py proves each mask's stated facts with the
flood fill of tests/floodfill.py and runs the protocol with the numpy engine; tests/test_gpu_agg_engine.py runs the same
(mask, cut plan) pairs with the HIP engine."""
import functools

import numpy as np

import morph_cases as MC
from morph_cases import lin

ERODE_REACH = 3                  # agg_shard.ERODE_REACH (pinned in tests/test_agg_shard_cases_cpu.py)
SMALL = (7, 6, 9)                # every plane its own slab, more ranks than planes
BIG = (34, 35, 70)               # 3 x 3 x 3 tiles of 16 x 16 x 32, none of the sizes a multiple of the tile


# ---- the communicator ------------------------------------------------------------------------------------------------------------
class _Gathered(Exception):
    """ends a rank's call of pass 1 at its all_gather"""


class TwoPassComm:
    """What agg_shard's protocol needs of a communicator (rank, world, all_gather), for all ranks in one process.  Each sharded filter
    makes exactly ONE all_gather and changes nothing before it, so two passes do: in pass 1 a rank's call hands over its contribution
    and is ended there, in pass 2 the call runs again and gets every rank's contribution."""

    def __init__(self, world):
        self.world, self.rank = int(world), 0
        self.parts = [None] * self.world
        self.given = [False] * self.world
        self.second = False
        self.calls = 0

    def all_gather(self, obj):
        self.calls += 1
        if not self.second:
            self.parts[self.rank], self.given[self.rank] = obj, True
            raise _Gathered()
        return list(self.parts)


def drive(world, call):
    """One collective step of `world` ranks: call(comm, rank) runs one sharded filter for that rank.  All ranks finish the step before
    drive returns, so a chain of filters is a sequence of drive calls."""
    comm = TwoPassComm(world)
    for r in range(world):
        comm.rank = r
        try:
            call(comm, r)
        except _Gathered:
            continue
        raise AssertionError(f"rank {r}: the call returned without an all_gather")
    assert all(comm.given)
    comm.second = True
    for r in range(world):
        comm.rank, comm.calls = r, 0
        call(comm, r)
        assert comm.calls == 1, f"rank {r}: {comm.calls} all_gather calls in one filter"


def region_chain(ag, region_ids):
    """[(mode, vals)] of the filters of agg_shard.postprocess_region_segmentation_sharded in its order, recorded from the function
    itself (its filter_largest_sharded replaced by a recorder for the duration of the call)."""
    seen = []
    real = ag.filter_largest_sharded
    ag.filter_largest_sharded = lambda comm, engine, mask, seg, z0, fill_value=255: seen.append(mask + (fill_value,))
    try:
        ag.postprocess_region_segmentation_sharded(None, None, lambda seg, mode, vals: (mode, tuple(vals)), None, 0, region_ids)
    finally:
        ag.filter_largest_sharded = real
    return seen


def select_ref(seg, mode, vals):
    """boa_label_select on a host array: mode 1: seg > 0; 2: seg in vals; 0: seg == vals[0]"""
    if mode == 1:
        return seg > 0
    if mode == 2:
        return np.isin(seg, vals)
    return seg == vals[0]


# ---- cut plans -------------------------------------------------------------------------------------------------------------------
def balanced(Z, world):
    """agg_shard.slab_bounds, restated (pinned against it in tests/test_agg_shard_cases_cpu.py)"""
    q, r = divmod(Z, world)
    out, lo = [], 0
    for i in range(world):
        hi = lo + q + (1 if i < r else 0)
        out.append((lo, hi))
        lo = hi
    return out


def cut_plans(Z, every_plane=None):
    """{name: [(z0, z1)] in z order, covering [0, Z)}.  Volumes of up to 8 planes get the every-plane plans, volumes of at least 18
    planes the cuts around the CCL tile boundary z = 16."""
    plans = {"balanced2": balanced(Z, 2), "balanced3": balanced(Z, 3)}
    if every_plane is None:
        every_plane = Z <= 8
    if every_plane:
        plans["every_plane"] = balanced(Z, Z)
        plans["two_ranks_too_many"] = balanced(Z, Z + 2)                # empty slabs at the end
        plans["empty_in_the_middle"] = [(0, Z // 2), (Z // 2, Z // 2), (Z // 2, Z)]
        plans["thin"] = [(0, 2), (2, 3), (3, Z)]                        # slabs of 2 and 1 planes: thinner than ERODE_REACH
    if Z >= 18:
        plans["tile16"] = [(0, 16), (16, Z)]
        plans["cut15"] = [(0, 15), (15, Z)]
        plans["cut17"] = [(0, 17), (17, Z)]
        plans["cut15_16_17"] = [(0, 15), (15, 16), (16, 17), (17, Z)]   # two one-plane slabs, inside and on the tile boundary
    for name, p in plans.items():
        assert p[0][0] == 0 and p[-1][1] == Z and all(a[1] == b[0] for a, b in zip(p[:-1], p[1:])) and all(a <= b for a, b in p), name
    return plans


# ---- interface masks -------------------------------------------------------------------------------------------------------------
# A case is morph_cases._case: mask, n, sizes = {size: how many}, keep = first voxel of the component filter_largest keeps, thresholds.
def _bounce(start, step, n, size):
    """n positions from `start` in steps of +-1, reflected at 0 and size - 1 (never two equal neighbours)"""
    out, p, d = [], start, step
    for _ in range(n):
        out.append(p)
        if not 0 <= p + d < size:
            d = -d
        p += d
    return out


def u_shape(shape, flip=False):
    """two arms along z at opposite corners of the plane, joined ONLY in the last plane: above every cut the arms are two local
    components that become one through the slabs below (flip: joined only in plane 0).  A block that is larger than an arm and smaller
    than the U competes."""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    m[:, 0, 0] = m[:, Y - 1, X - 1] = True
    m[Z - 1, :, 0] = m[Z - 1, Y - 1, :] = True
    u = 2 * Z + (Y - 2) + (X - 1)
    bz, by, bx = (2, 2, 3) if Z < 16 else (3, 4, 4)                    # 7 < 12 < 26 and 34 < 48 < 170
    m[1:1 + bz, 2:2 + by, 3:3 + bx] = True
    block = bz * by * bx
    assert Z < block < u
    if flip:
        m = np.ascontiguousarray(m[::-1])
    return MC._case(m, n=2, sizes={u: 1, block: 1}, keep=0, thresholds=(0, Z, block, u - 1, u), arm=Z)


def corner_chain(shape):
    """one voxel per plane, consecutive ones (dz, dy, dx) = (1, +-1, +-1) apart: linked through corner diagonals only, reflected at the
    y and x borders (on the big shape: at x = 0 in plane 15 and at y = Y - 1 in plane 16, the planes of the tile-boundary cuts).  A
    bar in plane 0 that starts BEFORE the chain in raster order is smaller than the chain and larger than any piece of it."""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    if Z < 16:
        ys, xs = _bounce(Y - 1, -1, Z, Y), _bounce(X - 1, -1, Z, X)
        bar = (0, 0, slice(0, 4))
    else:
        ys, xs = _bounce(Y - 1 - 16, 1, Z, Y), _bounce(15, -1, Z, X)
        bar = (0, 2, slice(30, 50))
    for z in range(Z):
        m[z, ys[z], xs[z]] = True
    chain = [(z, ys[z], xs[z]) for z in range(Z)]
    assert all(abs(a[1] - b[1]) == 1 and abs(a[2] - b[2]) == 1 for a, b in zip(chain[:-1], chain[1:]))
    assert {0, Y - 1} & set(ys) and {0, X - 1} & set(xs)
    m[bar] = True
    nb = bar[2].stop - bar[2].start
    keep, bar_first = lin(shape, *chain[0]), lin(shape, bar[0], bar[1], bar[2].start)
    assert bar_first < keep and nb < Z
    return MC._case(m, n=2, sizes={Z: 1, nb: 1}, keep=keep, thresholds=(0, 1, nb, Z - 1, Z), chain=chain, bar_first=bar_first)


def tie_three(shape):
    """three components of the same size: a rod along z through several slabs whose first voxel is the LAST voxel of its plane, a bar
    along x in a middle plane, a bar along y in a late plane.  The rod's first voxel is the smallest: it stays."""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    if Z < 16:
        s, za, zb, zc = 5, 0, 3, 6
    else:
        s, za, zb, zc = 20, 5, 16, 30
    m[za:za + s, Y - 1, X - 1] = True
    m[zb, 0, 0:s] = True
    m[zc, 0:s, 2] = True
    return MC._case(m, n=3, sizes={s: 3}, keep=lin(shape, za, Y - 1, X - 1), thresholds=(0, s - 1, s))


def late_winner(shape):
    """the largest component starts after a smaller one, in a later slab, and every piece of it that a cut leaves is smaller than or
    equal to the loser: it wins only by its merged size"""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    if Z < 16:
        m[0:2, 0:2, 0:3] = True                  # 12
        m[3:7, 4, 2:6] = True                    # 4 planes of 4 = 16
        lose, win, first = 12, 16, lin(shape, 3, 4, 2)
    else:
        m[0:2, 0:5, 0:10] = True                 # 100
        m[14:20, 20, 10:30] = True               # 6 planes of 20 = 120: cuts at 15 / 16 / 17 leave 20 + 100, 40 + 80, 60 + 60
        lose, win, first = 100, 120, lin(shape, 14, 20, 10)
    return MC._case(m, n=2, sizes={lose: 1, win: 1}, keep=first, thresholds=(0, lose - 1, lose, win - 1, win))


def through_middle(shape):
    """a rod through every plane (it touches both interfaces of every middle slab) next to one that ends at plane zc from below and
    one that starts at zc + 1: each of those touches one side of the interface zc | zc + 1 only, one voxel column apart from the
    other (x and x + 2), so that they must NOT be linked"""
    Z, Y, X = shape
    zc = 3 if Z < 16 else 15
    m = np.zeros(shape, bool)
    m[:, 1, 1] = True
    m[0:zc + 1, 4, 4] = True
    m[zc + 1:, 4, 6] = True
    sizes = {}
    for s in (Z, zc + 1, Z - zc - 1):
        sizes[s] = sizes.get(s, 0) + 1
    return MC._case(m, n=3, sizes=sizes, keep=lin(shape, 0, 1, 1), thresholds=(0, min(zc + 1, Z - zc - 1), max(zc + 1, Z - zc - 1), Z))


def all_background(shape):
    return MC._case(np.zeros(shape, bool), n=0, sizes={}, keep=None, thresholds=(0, 1))


def all_foreground(shape):
    k = int(np.prod(shape))
    return MC._case(np.ones(shape, bool), n=1, sizes={k: 1}, keep=0, thresholds=(0, k - 1, k))


def single_component(shape):
    """exactly one component (the `len(size_by_rep) <= 1` return of filter_largest_sharded) that leaves the first and the last plane
    free: with one plane per slab the outer slabs have no foreground at all"""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    m[1:Z - 1, 2:4, 3:6] = True
    k = (Z - 2) * 6
    return MC._case(m, n=1, sizes={k: 1}, keep=lin(shape, 1, 2, 3), thresholds=(0, k - 1, k))


def background_gap(shape):
    """two blobs at the same (y, x) with background planes between them: a slab that is all background lies between two that are not
    (balanced3 on the small shape, cut15_16_17 on the big one).  The upper blob is the larger: the winner starts in a later slab."""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    if Z < 16:
        m[0:2, 2:4, 2:4] = True                  # 8
        m[5:7, 2:4, 2:5] = True                  # 12
        lo, hi, first, gap = 8, 12, lin(shape, 5, 2, 2), (2, 5)
    else:
        m[10:15, 2:4, 2:4] = True                # 20
        m[17:22, 2:4, 2:5] = True                # 30
        lo, hi, first, gap = 20, 30, lin(shape, 17, 2, 2), (15, 17)
    return MC._case(m, n=2, sizes={lo: 1, hi: 1}, keep=first, thresholds=(0, lo, hi), gap=gap)


def threshold_merge(shape):
    """a rod of s voxels along z that every cut through it leaves in pieces of at most s - 2, next to unsplit bars of s - 1, s and s + 1
    voxels in single planes: at max_size s - 1 the rod stays (its pieces alone would go), at s it goes with the bar of s"""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    if Z < 16:
        s, z0 = 5, 1                             # planes 1 .. 5: balanced2 cuts 3 + 2
    else:
        s, z0 = 10, 12                           # planes 12 .. 21: cuts at 15 / 16 / 17 leave 3 + 7, 4 + 6, 5 + 5
    m[z0:z0 + s, 0, 0] = True
    m[0, 2, 2:2 + s - 1] = True
    m[Z - 1, 2, 2:2 + s] = True
    m[Z // 2, Y - 1, 2:2 + s + 1] = True
    if X < 2 + s + 1 + 1:
        raise AssertionError("shape too narrow")
    return MC._case(m, n=4, sizes={s - 1: 1, s: 2, s + 1: 1}, keep=lin(shape, Z // 2, Y - 1, 2), thresholds=(0, s - 2, s - 1, s, s + 1), s=s)


_BUILDERS = (("u_shape", u_shape), ("n_shape", lambda s: u_shape(s, True)), ("corner_chain", corner_chain), ("tie_three", tie_three),
             ("late_winner", late_winner), ("through_middle", through_middle), ("all_background", all_background),
             ("all_foreground", all_foreground), ("single_component", single_component), ("background_gap", background_gap),
             ("threshold_merge", threshold_merge))


@functools.lru_cache(maxsize=None)
def interface_cases():
    """{name: case}: every interface mask on the small and on the big shape (built once per process)"""
    out = {}
    for tag, shape in (("small", SMALL), ("big", BIG)):
        for name, fn in _BUILDERS:
            out[f"{name}_{tag}"] = fn(shape)
    return out


INTERFACE_NAMES = tuple(f"{name}_{tag}" for tag in ("small", "big") for name, _ in _BUILDERS)


@functools.lru_cache(maxsize=None)
def all_cases():
    """the interface masks and the worst cases of tests/morph_cases.py"""
    out = dict(interface_cases())
    out.update(MC.cc_cases())
    return out


ALL_NAMES = INTERFACE_NAMES + MC.CC_NAMES


@functools.lru_cache(maxsize=None)
def pairs():
    """every (mask name, plan name) pair, in a fixed order"""
    out = []
    for name in ALL_NAMES:
        for plan in cut_plans(all_cases()[name]["mask"].shape[0]):
            out.append((name, plan))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def references(name):
    """(largest_ref, {threshold: remove_small_ref}) of a case on the WHOLE volume, computed once per process and shared (read-only)"""
    c = all_cases()[name]
    big = MC.largest_ref(c["mask"])
    big.setflags(write=False)
    small = {}
    for t in c["thresholds"]:
        small[t] = MC.remove_small_ref(c["mask"], t)
        small[t].setflags(write=False)
    return big, small


@functools.lru_cache(maxsize=None)
def flood(name):
    """(roots, sizes) of tests/floodfill.components26 for a case, computed once per process and shared (read-only)"""
    if name in MC.CC_NAMES:
        return MC.cc_flood(name)
    from floodfill import components26
    roots, sizes = components26(all_cases()[name]["mask"])
    roots.setflags(write=False)
    return roots, sizes


def seg_around(m):
    """label 3 on the mask, label 9 sprinkled around it (must stay untouched)"""
    rng = np.random.default_rng(int(m.sum()) % 1000)
    seg = m.astype(np.uint8) * 3
    seg[~m] = (rng.random(m.shape)[~m] < 0.1) * 9
    return seg


# ---- the region chain's phantom --------------------------------------------------------------------------------------------------
REGION_SHAPE = (24, 20, 33)


def region_islands(R):
    """[((slice z, slice y, slice x), label)] of the phantom's stray islands: every one of them, and nothing else, becomes 255"""
    sl = lambda z, y, x: (slice(*z), slice(*y), slice(*x))  # noqa: E731
    return [
        # outside the body (removed by the first filter): below every cut, above every cut, across the cuts at 15 .. 17
        (sl((1, 3), (0, 2), (0, 2)), R["ABDOMINAL_CAVITY"]),
        (sl((20, 23), (0, 2), (30, 33)), R["THORACIC_CAVITY"]),
        (sl((14, 19), (18, 20), (0, 2)), R["MUSCLE"]),
        # inside the body, in the muscle ring (removed by the later filters)
        (sl((2, 4), (9, 11), (6, 8)), R["PERICARDIUM"]),
        (sl((21, 23), (9, 11), (6, 8)), R["PERICARDIUM"]),
        (sl((15, 18), (9, 11), (25, 27)), R["ABDOMINAL_CAVITY"]),      # across the cuts at 16 and 17
        (sl((5, 7), (9, 11), (25, 27)), R["MEDIASTINUM"]),             # a thoracic label below every cut
    ]


def region_phantom(R):
    """uint8 body_regions labels on REGION_SHAPE: nested ellipses along z (abdominal cavity below plane 12, thoracic cavity, mediastinum
    and pericardium above) and stray islands of the filtered labels on BOTH sides of the cuts at 8, 12, 15, 16 and 17, some of them
    lying across a cut."""
    Z, Y, X = REGION_SHAPE
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    r = np.sqrt(((yy - Y / 2) / (Y * 0.40)) ** 2 + ((xx - X / 2) / (X * 0.40)) ** 2)
    seg = np.zeros(REGION_SHAPE, np.uint8)
    seg[r < 1.0] = R["SUBCUTANEOUS_TISSUE"]
    seg[r < 0.8] = R["MUSCLE"]
    seg[(r < 0.55) & (zz < 12)] = R["ABDOMINAL_CAVITY"]
    seg[(r < 0.55) & (zz >= 12)] = R["THORACIC_CAVITY"]
    seg[(r < 0.25) & (zz >= 14)] = R["MEDIASTINUM"]
    seg[(r < 0.12) & (zz >= 15) & (zz < 20)] = R["PERICARDIUM"]
    for sl, label in region_islands(R):
        seg[sl] = label
    return seg


# ---- the halo claims of the sharded measurements ---------------------------------------------------------------------------------
ERODE_SHAPES = ((7, 13, 21), (34, 35, 33))
HIST_SHAPES = ((7, 5, 7), (34, 5, 7))          # Y * X = 35 is odd: the slab views start at odd multiples of 35 (labels) and 70 (CT) bytes


def halo(Z, a, b):
    """the planes a rank cuts from its copy of the volume for the slab [a, b): ERODE_REACH more on either side, inside the volume"""
    return max(0, a - ERODE_REACH), min(Z, b + ERODE_REACH)


@functools.lru_cache(maxsize=None)
def erode_mask(shape):
    """a solid volume with one pinhole in every plane, at positions that walk through the plane, and a few seeded ones: within 3
    planes of every cut, on both sides, something decides the 6^3 erosion (reach -3 .. +2 per axis, outside counts as set)"""
    Z, Y, X = shape
    rng = np.random.default_rng(Z * 1000 + X)
    m = rng.random(shape) >= 0.15 / 216
    for z in range(Z):
        m[z, (5 * z + 1) % Y, (7 * z + 2) % X] = False
    m.setflags(write=False)
    return m


def hist_inputs(shape):
    """(int16 CT over the whole int16 range with both ends present, uint8 labels with a third background, mask with values 0 / 1 / 2)"""
    rng = np.random.default_rng(shape[0])
    ct = rng.integers(-32768, 32768, size=shape).astype(np.int16)
    ct[0, 0, 0], ct[-1, -1, -1] = -32768, 32767
    lab = rng.integers(0, 256, size=shape).astype(np.uint8)
    lab[rng.random(shape) < 0.3] = 0
    lab[0, 0, 0] = lab[-1, -1, -1] = 255
    mask = rng.choice(np.array([0, 1, 1, 2], np.uint8), size=shape)
    mask[0, 0, 0] = mask[-1, -1, -1] = 1
    return ct, lab, mask


def hist_ref(ct, lab, mask, nbins=65536, hu_min=-32768):
    """boa_label_hu_histogram from its definition: [256][nbins] counts of (label, HU - hu_min) over the voxels with label != 0 (and
    mask != 0), bins clamped"""
    l = lab.ravel().astype(np.int64)
    if mask is not None:
        l = np.where(mask.ravel() != 0, l, 0)
    b = np.clip(ct.ravel().astype(np.int64) - hu_min, 0, nbins - 1)
    h = np.zeros((256, nbins), np.uint32)
    np.add.at(h, (l[l > 0], b[l > 0]), 1)
    return h
