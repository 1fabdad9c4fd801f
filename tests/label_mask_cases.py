"""The case table of the per-structure mask writer (tests/test_gpu_label_masks.py), built with numpy and zlib only, and the host
restatement of what the device computes: the presence table of `boa_label_member_presence` and the payload of a (label, member) pair
of `boa_deflate_label_pairs`.  tests/test_label_mask_cases_cpu.py pins the table: every claim a case makes about itself is checked
there, so that the GPU test cannot pass on a case that no longer holds what its name says."""
import zlib

import numpy as np

BLK = 16384                      # input bytes of a deflate block of the device encoder
VOLUME_SHAPE = (37, 29, 23)      # odd in every axis; 24 679 voxels
PRESENCE_MEMBER_BYTES = (1, 4093, 4096, 16384, 65536, 24679, 24680)      # .., n, n + 1


def n_members(n, member_bytes):
    return max(1, -(-n // member_bytes))


def member_slice(n, member_bytes, m):
    return slice(min(n, m * member_bytes), min(n, (m + 1) * member_bytes))


def presence_table(payload, member_bytes):
    """bool [members][256]: label k occurs in member m (n == 0: one all-false row)."""
    payload = np.asarray(payload, np.uint8).reshape(-1)
    out = np.zeros((n_members(payload.size, member_bytes), 256), bool)
    for m in range(out.shape[0]):
        out[m] = np.bincount(payload[member_slice(payload.size, member_bytes, m)], minlength=256) > 0
    return out


def presence_words(table):
    """The table as the device lays it out: [members][8] uint32, bit k % 32 of word k / 32."""
    return np.packbits(table, axis=1, bitorder="little").view("<u4")


def pair_payload(payload, member_bytes, label, m):
    """The bytes a pair stands for: (payload == label) over member m, as uint8 0 / 1."""
    payload = np.asarray(payload, np.uint8).reshape(-1)
    return (payload[member_slice(payload.size, member_bytes, m)] == label).astype(np.uint8).tobytes()


def pair_crc(payload, member_bytes, label, m):
    return zlib.crc32(pair_payload(payload, member_bytes, label, m))


def volume():
    """A label volume of VOLUME_SHAPE in file order (x fastest): boxes of 13 labels over a background of 0, so that labels are
    spatially coherent and every label misses most members; plus ids 255 (one voxel) and 254 (one x-row)."""
    x, y, z = np.meshgrid(*(np.arange(s) for s in VOLUME_SHAPE), indexing="ij")
    v = np.zeros(VOLUME_SHAPE, np.uint8)
    k = 0
    for z0 in (1, 9, 17):
        for y0 in (2, 15):
            for x0 in (3, 20):
                k += 1
                v[(x >= x0) & (x < x0 + 11 + k % 5) & (y >= y0) & (y < y0 + 9) & (z >= z0) & (z < z0 + 5)] = k
    v[5:30, 12, 8] = 254
    v[36, 28, 22] = 255          # the very last voxel
    v[0, 0, 0] = 13              # the very first
    out = np.asfortranarray(v).reshape(-1, order="F")
    out.setflags(write=False)
    return out


def _case(name, payload, member_bytes, present, absent, boundary=(), shift=0, note=""):
    payload = np.ascontiguousarray(payload, np.uint8)
    payload.setflags(write=False)
    return dict(name=name, payload=payload, member_bytes=int(member_bytes), present=list(present), absent=list(absent),
                boundary=list(boundary), shift=int(shift), note=note)


def _coherent(n, seed, labels=(0, 3, 9)):
    """n bytes in runs of 20 .. 400 bytes of the given labels."""
    rng = np.random.default_rng(seed)
    out = np.empty(n + 400, np.uint8)
    at = 0
    while at < n:
        run = int(rng.integers(20, 400))
        out[at:at + run] = labels[int(rng.integers(0, len(labels)))]
        at += run
    return out[:n]


def cases():
    """[case]: name, payload (uint8, file order), member_bytes, present / absent: [(label, member)] the case claims to be so, boundary:
    [(label, byte index, member, offset in member or -1 for its last byte)] of single voxels the case places, shift: bytes the source
    pointer is moved off a 16-byte boundary."""
    out = []
    # ---- n in {0, 1, 15, 17}: below, at and just above one vector; n == 0 is one empty member
    out.append(_case("n0", np.zeros(0, np.uint8), 4096, [], [(0, 0), (7, 0)]))
    out.append(_case("n1", np.array([7], np.uint8), 4096, [(7, 0)], [(0, 0)]))
    p = np.zeros(15, np.uint8)
    p[14] = 2
    out.append(_case("n15", p, 4096, [(0, 0), (2, 0)], [(1, 0)], [(2, 14, 0, -1)]))
    p = np.full(17, 4, np.uint8)
    p[16] = 5
    out.append(_case("n17_members_of_16", p, 16, [(4, 0), (5, 1)], [(5, 0), (4, 1)], [(5, 16, 1, 0)]))
    # ---- a source pointer one byte off a 16-byte boundary
    p = _coherent(2 * 4096 + 100, 1)
    out.append(_case("unaligned", p, 4096, [(3, 0), (9, 1), (int(p[-1]), 2)], [(1, 0), (200, 2)], shift=1))
    # ---- a last member of one byte
    p = _coherent(2 * 4096 + 1, 2).copy()
    p[-1] = 77
    out.append(_case("last_member_one_byte", p, 4096, [(77, 2), (3, 0)], [(77, 0), (77, 1), (3, 2)], [(77, 2 * 4096, 2, 0)]))
    # ---- the history cut: a label whose only voxel is the first byte of a member, another whose only voxel is the last byte of one;
    # members of 40 000 bytes (two full blocks and a ragged one), the neighbours across the cut carry the same label on both sides
    mb = 40_000
    p = _coherent(3 * mb, 3).copy()
    p[mb - 3:mb + 3] = 9
    p[mb] = 101                   # first byte of member 1
    p[2 * mb - 3:2 * mb + 3] = 3
    p[2 * mb - 1] = 102           # last byte of member 1
    out.append(_case("first_and_last_byte_of_a_member", p, mb, [(101, 1), (102, 1), (9, 0), (9, 1), (3, 1), (3, 2)],
                     [(101, 0), (101, 2), (102, 0), (102, 2)], [(101, mb, 1, 0), (102, 2 * mb - 1, 1, -1)]))
    # ---- a label present only in the short last member
    p = _coherent(2 * 4096 + 300, 4).copy()
    p[2 * 4096 + 100:2 * 4096 + 180] = 55
    out.append(_case("only_in_the_short_last_member", p, 4096, [(55, 2)], [(55, 0), (55, 1)]))
    # ---- one label filling the volume
    out.append(_case("one_label_fills", np.full(2 * BLK + 77, 7, np.uint8), BLK + 5, [(7, 0), (7, 1), (7, 2)], [(0, 0), (8, 1), (255, 2)]))
    # ---- per-voxel random labels 0 .. 255: the label bytes themselves would be stored blocks; a mask of them is isolated ones
    p = np.random.default_rng(5).integers(0, 256, 3 * 4096 + 11).astype(np.uint8)
    p[p == 250] = 251             # one id that is absent everywhere
    out.append(_case("random_labels", p, 4096, [(0, 0), (255, 1), (128, 2), (int(p[3 * 4096]), 3)], [(250, 0), (250, 3)],
                     note="every member holds (nearly) every id; the short last member of 11 bytes holds at most 11"))
    # ---- a random 0 / 1 volume: the mask of id 1 is as incompressible as a mask gets
    p = np.random.default_rng(6).integers(0, 2, BLK + 100).astype(np.uint8)
    out.append(_case("random_bits", p, 1 << 20, [(0, 0), (1, 0)], [(2, 0)]))
    # ---- ids 0 and 255 as structures
    p = _coherent(3 * 4096, 7, labels=(0, 255, 1)).copy()
    p[4096:2 * 4096] = 1
    out.append(_case("ids_0_and_255", p, 4096, [(0, 0), (255, 0), (1, 1), (0, 2), (255, 2)], [(0, 1), (255, 1)]))
    # ---- a member of several blocks with a tail: 3 x 16 KiB + 5 bytes in one member, and in members of the default size
    p = _coherent(3 * BLK + 5, 8, labels=(0, 3, 9, 12))
    out.append(_case("three_blocks_and_a_tail", p, 3 * BLK + 5, [(0, 0), (3, 0), (9, 0), (12, 0)], [(1, 0)]))
    out.append(_case("three_blocks_and_a_tail_4MiB", p, 4 << 20, [(0, 0), (12, 0)], [(1, 0)]))
    return out
