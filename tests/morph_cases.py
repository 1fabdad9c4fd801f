"""Worst-case masks of tests/test_gpu_morph_worstcase.py: the structures that i.i.d. noise and random balls cannot produce and that
the connected-component tables (csrc/ccl_bits.hip: 32 x 16 x 16 tiles labelled by csrc/ccl_tile.h, 1024 table entries per tile), the slice flood, the erosions
and the cross dilation are most likely to get wrong.  numpy only, no device: every generator returns its mask(s) together with the
facts the case is built to have, and tests/test_morph_cases_cpu.py proves those facts with the flood fills of tests/floodfill.py and
with scipy.ndimage before a case reaches a GPU."""
import functools

import numpy as np

TX, TY, TZ = 32, 16, 16          # CCL_TX / CCL_TY / CCL_TZ of ccl_tile.h (the tiles of ccl_bits.hip and ccl_bytes.hip)
CAP = 1024                       # CB_CAP: table entries per tile = the most 26-connected components a tile can hold
S26 = np.ones((3, 3, 3), bool)


def lin(shape, z, y, x):
    """linear (raster, C order) index of a voxel"""
    return (z * shape[1] + y) * shape[2] + x


def tile_of(shape, z, y, x):
    """index of the 32 x 16 x 16 tile that holds a voxel, in the kernels' order (tz, ty, tx)"""
    tx, ty = -(-shape[2] // TX), -(-shape[1] // TY)
    return ((z // TZ) * ty + y // TY) * tx + x // TX


def tile_slices(shape):
    """{tile index: (slice z, slice y, slice x)}"""
    out = {}
    for z0 in range(0, shape[0], TZ):
        for y0 in range(0, shape[1], TY):
            for x0 in range(0, shape[2], TX):
                out[tile_of(shape, z0, y0, x0)] = (slice(z0, z0 + TZ), slice(y0, y0 + TY), slice(x0, x0 + TX))
    return out


# ---- connected-component cases ---------------------------------------------------------------------------------------------------
# A case: dict(mask = bool [Z][Y][X], n = number of 26-connected components or None (taken from the flood fill), sizes = {size: how
# many components} or None, keep = linear index of the first voxel of the component the largest-component filter must keep,
# thresholds = max_size values for remove_small on the mask, inv_thresholds = the same on the complement, plus case-specific facts.
def _case(mask, n=None, sizes=None, keep=None, thresholds=(0, 1), inv_thresholds=None, **facts):
    if inv_thresholds is None:
        inv_thresholds = (1, int(mask.size))
    return dict(mask=mask, n=n, sizes=sizes, keep=keep, thresholds=tuple(thresholds), inv_thresholds=tuple(inv_thresholds), **facts)


def lattice(shape, parity):
    """single voxels two apart on every axis: as many components as voxels, CAP of them in every complete tile; parity 1 puts one
    on each complete tile's last voxel.  All tie: the raster-first voxel is the largest component.  The complement is ONE component."""
    m = np.zeros(shape, bool)
    m[parity::2, parity::2, parity::2] = True
    k = int(m.sum())
    return _case(m, n=k, sizes={1: k}, keep=lin(shape, parity, parity, parity), thresholds=(0, 1),
                 inv_thresholds=(1, m.size - k - 1, m.size - k, m.size), complement_n=1)


def lattice_bridged():
    """the even lattice on (32, 32, 64) = 8 tiles.  In the tiles with even tz + ty + tx, the rows with even (z / 2 + y / 2) get a
    voxel at x0 + 4 j + 1 (odd coordinate: it touches exactly the lattice voxels x0 + 4 j and x0 + 4 j + 2: a component of 3); in
    the OTHER tiles of word column 1 the same rows get a voxel at x = 63, which touches only the lattice voxel at 62 (x = 64 is
    outside): a component of 2, on the tile's last bit.  Thresholds 0, 1, 2, 3 keep four different sets."""
    shape = (32, 32, 64)
    m = lattice(shape, 0)["mask"].copy()
    n1, n2, n3 = int(m.sum()), 0, 0
    for tz in range(2):
        for ty in range(2):
            for tx in range(2):
                rows = [(z, y) for z in range(tz * TZ, tz * TZ + TZ, 2) for y in range(ty * TY, ty * TY + TY, 2) if (z // 2 + y // 2) % 2 == 0]
                if (tz + ty + tx) % 2 == 0:
                    for z, y in rows:
                        for j in range(8):
                            m[z, y, tx * TX + 4 * j + 1] = True
                            n3 += 1
                            n1 -= 2
                elif tx == 1:
                    for z, y in rows:
                        m[z, y, 63] = True
                        n2 += 1
                        n1 -= 1
    return _case(m, n=n1 + n2 + n3, sizes={1: n1, 2: n2, 3: n3}, keep=lin(shape, 0, 0, 0), thresholds=(0, 1, 2, 3))


def tie_cases():
    """{name: case}: two (or three) components of equal size whose raster order is NOT the order of their tiles / table entries.
    The one whose first voxel comes first in raster order must survive the largest-component filter."""
    shape = (20, 20, 70)
    out = {}
    m = np.zeros(shape, bool)
    m[0, 0, 40:44] = True                   # word column 1 (tile 1), raster-first
    m[0, 1, 0:4] = True                     # word column 0 (tile 0)
    out["word_columns"] = _case(m, n=2, sizes={4: 2}, keep=lin(shape, 0, 0, 40), thresholds=(3, 4))
    m = np.zeros(shape, bool)
    m[0, 0, 0:4] = True                     # mirrored: tile order and raster order agree
    m[0, 1, 40:44] = True
    out["mirrored"] = _case(m, n=2, sizes={4: 2}, keep=lin(shape, 0, 0, 0), thresholds=(3, 4))
    m = np.zeros(shape, bool)
    m[0, 16, 0:4] = True                    # tile row ty = 1, plane 0: raster-first
    m[1, 0, 40:44] = True                   # tile row ty = 0, plane 1
    out["y_tile_border"] = _case(m, n=2, sizes={4: 2}, keep=lin(shape, 0, 16, 0), thresholds=(3, 4))
    m = np.zeros(shape, bool)
    m[0, 17, 0:4] = True                    # tile (tz 0, ty 1): raster-first
    m[14:18, 0, 40] = True                  # crosses the z tile border in tile column (ty 0, tx 1): its root is in an earlier tile
    out["z_tile_border"] = _case(m, n=2, sizes={4: 2}, keep=lin(shape, 0, 17, 0), thresholds=(3, 4))
    return out


def chain_first_in_later_tile(with_larger=False):
    """the diagonal chain (i, 0, 40 - i), i = 0 .. 9: its raster-first voxel (0, 0, 40) lies in word column 1, its last voxel
    (9, 0, 31) in word column 0, so its root entry belongs to tile 0 and `first` has to be handed over from tile 1.  Against an
    equally large bar at (0, 5, 0:10) the chain stays; with_larger adds a block of 36 that beats both."""
    shape = (20, 20, 70)
    m = np.zeros(shape, bool)
    for i in range(10):
        m[i, 0, 40 - i] = True
    m[0, 5, 0:10] = True
    keep = lin(shape, 0, 0, 40)
    sizes = {10: 2}
    if with_larger:
        m[12:15, 10:13, 50:54] = True
        keep = lin(shape, 12, 10, 50)
        sizes = {10: 2, 36: 1}
    return _case(m, n=sum(sizes.values()), sizes=sizes, keep=keep, thresholds=(9, 10, 36),
                 chain_first=lin(shape, 0, 0, 40), chain_last=(9, 0, 31))


def rods_64_roots():
    """(32, 32, 64): in every tile of word column 1, 64 rods along x (x = 32 .. 63, two apart in y and z); each has one more voxel at
    x = 31 in the neighbouring tile of word column 0, which also carries the lattice x = 0, 2 .. 28: 15 * 64 + 64 = CAP local
    components.  Each rod's root is its x = 31 voxel's entry in the lower tile, so the 64 consecutive table entries of a rod tile hand
    their size and first voxel to 64 DIFFERENT roots in one wave iteration."""
    shape = (32, 32, 64)
    m = np.zeros(shape, bool)
    m[::2, ::2, 31:64] = True
    m[::2, ::2, 0:29:2] = True
    rods = 16 * 16
    return _case(m, n=rods * 16, sizes={33: rods, 1: rods * 15}, keep=lin(shape, 0, 0, 31), thresholds=(1, 32, 33),
                 rods_per_tile=64, lower_tile_components=CAP)


def full_tile_contacts():
    """(32, 32, 96): the tile (tz 0, ty 0, tx 1) is all foreground; single voxels touch it across a face, an edge and a corner, on
    the forward and on the backward side; others sit exactly two away and stay separate; a diagonal chain hangs from the corner
    voxel (16, 16, 64).  Counts and sizes come from the flood fill."""
    shape = (32, 32, 96)
    m = np.zeros(shape, bool)
    m[0:16, 0:16, 32:64] = True
    touch = [(5, 5, 64), (5, 5, 31), (16, 5, 40), (5, 16, 40),            # faces: +x, -x, +z, +y
             (16, 16, 45), (9, 16, 64), (16, 9, 31), (16, 2, 64),         # edges
             (16, 16, 64)]                                                # corner
    chain = [(16 + i, 16 + i, 64 + i) for i in range(1, 10)]
    far = [(10, 10, 65), (17, 10, 50), (10, 17, 55), (17, 17, 30), (12, 2, 30), (17, 4, 65), (1, 17, 65), (25, 5, 5)]
    for v in touch + chain + far:
        m[v] = True
    big = TX * TY * TZ + len(touch) + len(chain)
    bg = m.size - int(m.sum())
    return _case(m, keep=lin(shape, 0, 0, 32), thresholds=(1, big - 1, big), inv_thresholds=(1, bg - 1, bg),
                 touch=touch, chain=chain, far=far, big=big)


def full_tiles_corner():
    """two all-foreground tiles that meet only at a corner: one component of 2 * 8192 (one union per pair of full tiles)"""
    shape = (32, 32, 64)
    m = np.zeros(shape, bool)
    m[0:16, 0:16, 0:32] = True
    m[16:32, 16:32, 32:64] = True
    return _case(m, n=1, sizes={16384: 1}, keep=0, thresholds=(16383, 16384))


def full_empty_mixed():
    """2 x 2 x 2 tiles: one full, the opposite one empty, six mixed (seeded noise of different densities)"""
    shape = (32, 32, 64)
    rng = np.random.default_rng(2024)
    m = np.zeros(shape, bool)
    for t, sl in tile_slices(shape).items():
        m[sl] = rng.random((TZ, TY, TX)) < (0.04, 0.1, 0.2, 0.35, 0.5, 0.7, 0.85, 0.95)[t]
    m[0:16, 0:16, 0:32] = True
    m[16:32, 16:32, 32:64] = False
    return _case(m, keep=None, thresholds=(1, 5, 8192, 8193), inv_thresholds=(1, 5, 8192))


def boustrophedon(shape=(34, 35, 70)):
    """a one-voxel-wide path through every tile: along x in the rows y = 0, 2, 4 .. of the planes z = 0, 2, 4 .., consecutive rows
    joined at alternating ends, consecutive planes joined at alternating corners.  ONE component."""
    Z, Y, X = shape
    m = np.zeros(shape, bool)
    ys = list(range(0, Y, 2))
    for pi, z in enumerate(range(0, Z, 2)):
        order = ys if pi % 2 == 0 else ys[::-1]
        for ri, y in enumerate(order):
            m[z, y, :] = True
            if ri + 1 < len(order):
                right = (ri + pi * len(ys)) % 2 == 0           # the row ends alternate along the whole path
                m[z, (y + order[ri + 1]) // 2, X - 1 if right else 0] = True
        if z + 2 < Z:
            right = (len(ys) - 1 + pi * len(ys)) % 2 == 0
            m[z + 1, order[-1], X - 1 if right else 0] = True
    k = int(m.sum())
    return _case(m, n=1, sizes={k: 1}, keep=0, thresholds=(k - 1, k))


def complement_of(case):
    m = ~case["mask"]
    return _case(m, keep=None, thresholds=(1, 100), inv_thresholds=case["thresholds"])


def checkerboard(shape=(34, 35, 70)):
    """2 x 2 x 2 blocks of alternating value: the blocks of one colour touch along edges and at corners only.  ONE component, and so
    is the complement."""
    zz, yy, xx = np.meshgrid(*[np.arange(s) // 2 for s in shape], indexing="ij")
    m = (zz + yy + xx) % 2 == 0
    k = int(m.sum())
    return _case(m, n=1, sizes={k: 1}, keep=0, thresholds=(k - 1, k), inv_thresholds=(m.size - k - 1, m.size - k), complement_n=1)


@functools.lru_cache(maxsize=None)
def cc_cases():
    """{name: case} of every connected-component case (built once per process)"""
    out = {}
    for shape in ((32, 32, 64), (33, 35, 70)):
        for parity in (0, 1):
            out[f"lattice{parity}_{shape[0]}x{shape[1]}x{shape[2]}"] = lattice(shape, parity)
    out["lattice_bridged"] = lattice_bridged()
    for k, v in tie_cases().items():
        out["tie_" + k] = v
    out["chain_first_in_later_tile"] = chain_first_in_later_tile()
    out["chain_and_larger"] = chain_first_in_later_tile(True)
    out["rods_64_roots"] = rods_64_roots()
    out["full_tile_contacts"] = full_tile_contacts()
    out["full_tiles_corner"] = full_tiles_corner()
    out["full_empty_mixed"] = full_empty_mixed()
    out["boustrophedon"] = boustrophedon()
    out["boustrophedon_complement"] = complement_of(out["boustrophedon"])
    out["checkerboard"] = checkerboard()
    return out


CC_NAMES = ("lattice0_32x32x64", "lattice1_32x32x64", "lattice0_33x35x70", "lattice1_33x35x70", "lattice_bridged", "tie_word_columns",
            "tie_mirrored", "tie_y_tile_border", "tie_z_tile_border", "chain_first_in_later_tile", "chain_and_larger", "rods_64_roots",
            "full_tile_contacts", "full_tiles_corner", "full_empty_mixed", "boustrophedon", "boustrophedon_complement", "checkerboard")


@functools.lru_cache(maxsize=None)
def cc_flood(name):
    """(roots, sizes) of tests/floodfill.components26 for a case, computed once per process and shared (read-only)"""
    from floodfill import components26
    roots, sizes = components26(cc_cases()[name]["mask"])
    roots.setflags(write=False)
    return roots, sizes


def label26(mask):
    from scipy import ndimage
    return ndimage.label(mask, structure=S26)


def remove_small_ref(mask, max_size):
    """remove_small_objects(max_size, connectivity 3): components with <= max_size voxels are cleared (scipy labelling)"""
    lab, k = label26(mask)
    if k == 0:
        return mask.copy()
    small = np.bincount(lab.ravel()) <= max_size
    small[0] = False
    return mask & ~small[lab]


def largest_ref(mask):
    """voxels OUTSIDE the largest component (ties: the lowest label = the raster-first component); nothing for <= 1 component"""
    lab, k = label26(mask)
    if k <= 1:
        return np.zeros(mask.shape, bool)
    keep = int(np.argmax(np.bincount(lab.ravel())[1:])) + 1
    return mask & (lab != keep)


# ---- contour fill cases ----------------------------------------------------------------------------------------------------------
def corridor(Y, X, open_mouth=False):
    """a frame with baffles in every second row, attached alternately to the left and to the right wall: the inside is one corridor
    that turns once per baffle.  Closed, the contour fill sets the whole slice; with one mouth in the frame next to the corridor's far
    end the flood from the border walks the whole corridor (one outer iteration of the kernels' flood per turn) and nothing is filled."""
    m = np.zeros((Y, X), bool)
    m[0] = m[-1] = True
    m[:, 0] = m[:, -1] = True
    for i, y in enumerate(range(2, Y - 2, 2)):
        if i % 2 == 0:
            m[y, 1:X - 2] = True            # gap at x = X - 2
        else:
            m[y, 2:X - 1] = True            # gap at x = 1
    if open_mouth:
        m[Y - 1, 1 if len(range(2, Y - 2, 2)) % 2 == 1 else X - 2] = False      # bottom frame, at the side away from the last gap
    return m


def corridor_volume(Y, X):
    """[Z = 6][Y][X]: closed, open, blank, full, open upside down, closed mirrored"""
    c, o = corridor(Y, X), corridor(Y, X, True)
    return np.stack([c, o, np.zeros((Y, X), bool), np.ones((Y, X), bool), o[::-1], c[:, ::-1]])


CORRIDOR_SHAPES = ((300, 70), (70, 300), (300, 33), (300, 64))


def corridor_batch(Y, X):
    """two masks for one batched call: the volume above (transposed slices for Y < X, so that the corridors run along y) and the same
    slices in reverse order"""
    if Y >= X:
        v = corridor_volume(Y, X)
    else:
        v = np.ascontiguousarray(corridor_volume(X, Y).transpose(0, 2, 1))
    return [v, np.ascontiguousarray(v[::-1])]


def fill_ref(vol):
    from scipy import ndimage
    return np.stack([ndimage.binary_fill_holes(s) for s in vol])


LDS_LIMIT = 150 * 1024           # cb_lds_limit() of ccl_bits.hip on gfx950 (160 KiB opt-in LDS minus 10 KiB of headroom)


def bits_fill_supported(Y, X):
    """boa_bits_fill_supported: two [Y][W | 1] word arrays in LDS"""
    return Y * (((X + 31) // 32) | 1) * 8 <= LDS_LIMIT


def bytes_fill_in_lds(Y, X):
    """boa_fill_holes_2d keeps its LDS flood (two [Y][W] word arrays) up to the same limit; above it the union-find over bytes runs"""
    return Y * ((X + 31) // 32) * 8 <= LDS_LIMIT


BIG_SLICE = (2, 2048, 300)       # Y * 11 * 8 = 180 224 > 153 600 (bit path unsupported) and Y * 10 * 8 = 163 840 (byte flood not in LDS)


def big_slice_labels():
    """uint8 labels on BIG_SLICE: label 1 a frame around almost the whole slice (its bounding box is > 70 % of the volume: the byte
    path fills it uncropped, by union-find) with solid blocks inside; label 2 small frames (closed holes, a frame with a mouth) inside
    a small bounding box (the cropped LDS flood); label 3 specks that the small-object filter removes; label 2 frames also inside
    label 1's blocks, so that the ascending overwrite order matters."""
    Z, Y, X = BIG_SLICE
    seg = np.zeros(BIG_SLICE, np.uint8)
    for z in range(Z):
        seg[z, 10:2040, 5] = seg[z, 10:2040, 294] = 1
        seg[z, 10, 5:295] = seg[z, 2039, 5:295] = 1
        seg[z, 300:360, 100:180] = 1                       # solid block of label 1 ...
        seg[z, 310:350, 110:170] = 0                       # ... with a hole: filled by the contour fill
        seg[z, 600 + z:660, 40:44] = 1
    seg[1, 2039, 150] = 0                                  # slice 1: the big frame has a mouth, nothing of it is filled
    for z in range(Z):
        seg[z, 1000:1030, 50:90] = 2
        seg[z, 1003:1027, 53:87] = 0                       # closed frame of label 2
        seg[z, 1100:1130, 50:90] = 2
        seg[z, 1103:1127, 53:87] = 0
        seg[z, 1100:1103, 70] = 0                          # frame with a mouth
        seg[z, 1010:1014, 60:64] = 3                       # a speck inside the closed frame
    rng = np.random.default_rng(77)
    specks = (rng.random(BIG_SLICE) < 0.0005) & (seg == 0)
    seg[specks] = 3
    return seg


SMALL_VOLUME = (4, 10, 33)


def small_volume_labels():
    """fewer voxels than the default threshold of 3000: labels 2 and 5 present, 1 and 7 absent"""
    seg = np.zeros(SMALL_VOLUME, np.uint8)
    seg[1:3, 2:6, 3:20] = 2
    seg[0:2, 6:9, 25:33] = 5
    return seg


# ---- erosion cases ---------------------------------------------------------------------------------------------------------------
def erode_reach(k):
    """offsets [lo, hi] per axis of boa_binary_erode(kernel_value = k) (morph.hip): the k^3 footprint, end-padded to k + 1 for even k"""
    center = (k + 1) // 2 if k % 2 == 0 else k // 2
    return -center, k - 1 - center


def erode_on_bits(lo, hi):
    """the rule of boa_binary_erode (morph.hip): reaches below 32 run on bit masks (k_bits_erode_axis), larger ones on bytes (k_erode_axis)"""
    return lo > -32 and hi < 32


def erode_box_ref(mask, lo, hi):
    """AND over the offsets [lo, hi] on every axis, positions outside the volume count as set: shifted copies of the padded mask"""
    out = np.asarray(mask, bool)
    for ax in range(3):
        n = out.shape[ax]
        pad = [(0, 0)] * 3
        pad[ax] = (-lo, hi)
        p = np.pad(out, pad, constant_values=True)
        acc = np.ones(out.shape, bool)
        for d in range(lo, hi + 1):
            sl = [slice(None)] * 3
            sl[ax] = slice(d - lo, d - lo + n)
            acc &= p[tuple(sl)]
        out = acc
    return out


PINHOLE_X = (31, 32, 33, 64, 65, 97)
PINHOLE_K = tuple(range(1, 10))
PINHOLE_ZY = (22, 26)


def pinhole_mask(X, k):
    """a solid (22, 26, X) volume with seeded pinholes, dense enough that the k^3 erosion leaves 20 .. 80 % (a pinhole clears k^3
    voxels: the density is ln 2 / k^3 for one half, less what the forced ones clear), and pinholes forced at x = 0, 31, 32, X - 1 and
    at the first / last y and z"""
    Z, Y = PINHOLE_ZY
    rng = np.random.default_rng(1000 * X + k)
    m = rng.random((Z, Y, X)) >= 0.55 / k ** 3 if k > 1 else rng.random((Z, Y, X)) >= 0.5
    for v in ((0, 7, 0), (Z - 1, 12, X - 1), (9, 0, min(31, X - 1)), (14, Y - 1, min(32, X - 1)), (0, 0, X // 2), (Z - 1, Y - 1, 0)):
        m[v] = False
    return m


ASYM_REACHES = ((-31, 0), (0, 31), (-31, 31), (0, 0), (-1, 30))
ASYM_X = (32, 64, 100)           # rows of 1, 2 and 4 words


def asym_mask(X):
    """(40, 38, X), solid but for a pinhole near the low corner and one near the high corner: with reaches of 31 the eroded result is
    neither empty nor full (reach (0, 0) returns the mask)"""
    m = np.ones((40, 38, X), bool)
    m[2, 3, 1] = m[38, 35, X - 2] = False
    return m


BYTE_K = (63, 64, 65)             # reaches (-31, 31): the last on bits; (-32, 31) and (-32, 32): the first on bytes
BYTE_SHAPES = ((70, 5, 70), (5, 70, 33))
# scipy's binary_erosion visits the whole structure for every voxel: 65^3 * 24 500 voxels = 30 s per call on (70, 5, 70).  The oracle
# (`erode_region`) is therefore called on thin volumes with one long axis each; on BYTE_SHAPES the reference is erode_box_ref, which
# tests/test_morph_cases_cpu.py pins against the oracle on the thin volumes and for every k <= 9.
BYTE_THIN_SHAPES = ((70, 2, 5), (2, 70, 5), (2, 3, 70))


def byte_mask(shape):
    """solid, but for the plane at index 34 of every axis longer than 65.  With reaches of 31 / 32 only
    the first and last two to four planes of such an axis survive, so each of lo and hi decides one plane of the result, and on the
    short axes every offset beyond the volume has to count as set.  (Few survivors and early misses also keep scipy's erosion with a
    65^3 structure at a second or two: it visits the whole structure for every voxel that survives.)"""
    m = np.ones(shape, bool)
    for ax, n in enumerate(shape):
        if n > 65:
            sl = [slice(None)] * 3
            sl[ax] = 34
            m[tuple(sl)] = False
    return m


# ---- dilation and the assign kernels ---------------------------------------------------------------------------------------------
DILATE_ITERATIONS = (1, 2, 3, 4, 7)
DILATE_SHAPES = ((1, 1, 7), (5, 3, 100), (17, 20, 33))


def dilate_masks(shape):
    """{name: mask}: seeds on corners, edges and faces, an empty and a full mask"""
    Z, Y, X = shape
    out = {"empty": np.zeros(shape, bool), "full": np.ones(shape, bool)}
    m = np.zeros(shape, bool)
    m[0, 0, 0] = m[Z - 1, Y - 1, X - 1] = True
    out["corners"] = m
    m = np.zeros(shape, bool)
    m[0, 0, X // 2] = m[Z - 1, Y // 2, X - 1] = m[Z // 2, Y - 1, 0] = True
    out["edges"] = m
    m = np.zeros(shape, bool)
    m[0, Y // 2, X // 3] = m[Z // 2, Y // 2, X - 1] = m[Z // 2, 0, X // 2] = True
    out["faces"] = m
    return out


ASSIGN_N = (1, 255, 256, 257, 1000003)


def assign_inputs(n):
    """(mask bytes with values 0 / 1 / 2 / 255, previous content of out, part labels for the overlay)"""
    rng = np.random.default_rng(n)
    mask = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), size=n)
    prev = rng.integers(0, 256, n, dtype=np.uint8)
    part = (rng.integers(0, 256, n, dtype=np.uint8) * (rng.random(n) < 0.4)).astype(np.uint8)
    mask[-1], part[-1] = 255, 201        # the last element is written
    if n > 1:
        mask[0], part[0] = 0, 0          # the first keeps its content (invert = 0)
    return mask, prev, part
