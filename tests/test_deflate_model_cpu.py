"""tests/deflate_model.py against zlib: the reader on streams a third party made, the model encoder's streams through zlib's inflate,
its code lengths against Huffman's algorithm and a plain package-merge, and its fixed-code sizes against the device sizes that
DESIGN 4.9 records for the three label phantoms."""
import functools
import itertools
import zlib

import numpy as np
import pytest

import deflate_model as dm


def _payloads():
    rng = np.random.default_rng(3)
    text = (b"the quick brown fox jumps over the lazy dog; " * 40 + bytes(rng.integers(0, 256, 500, dtype=np.uint8))) * 12
    return {"text": text, "regions_like": dm.CONTENTS["regions_like"](70_000).tobytes(), "prefix_image": dm.prefix_image().tobytes(),
            "random0to3": dm.CONTENTS["random0to3"](40_000).tobytes(), "empty": b"", "one": b"x"}


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_parse_blocks_reads_zlib_streams(level):
    types = set()
    for name, raw in _payloads().items():
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        body = c.compress(raw) + c.flush()
        blocks = dm.parse_blocks(body)
        assert b"".join(b["data"] for b in blocks) == raw, name
        assert blocks[-1]["final"] and not any(b["final"] for b in blocks[:-1])
        assert blocks[-1]["end_bit"] <= 8 * len(body) < blocks[-1]["end_bit"] + 8
        for b in blocks:
            assert b["end_bit"] - b["start_bit"] == b["header_bits"] + b["payload_bits"]
            if b["type"] == 2:
                assert max(b["ll_lens"]) <= 15 and max(b["cl_lens"]) <= 7
        types |= {b["type"] for b in blocks}
    assert types == ({0} if level == 0 else {1, 2}), types            # zlib writes short inputs fixed, the others dynamic


def _naive_package_merge(freqs, limit):
    """Package-merge with the symbols of every item written out (fine for small alphabets)."""
    leaves = sorted((f, (s,)) for s, f in enumerate(freqs) if f)
    n, level = len(leaves), None
    for _ in range(limit):
        packs = [] if level is None else [(level[2 * q][0] + level[2 * q + 1][0], level[2 * q][1] + level[2 * q + 1][1])
                                          for q in range(len(level) // 2)]
        level = sorted(leaves + packs, key=lambda it: it[0])
    lens = [0] * len(freqs)
    for _, syms in level[:2 * n - 2]:
        for s in syms:
            lens[s] += 1
    return lens


def _brute_force_cost(freqs, limit):
    """Least cost over every multiset of lengths <= limit with Kraft sum <= 1, the longest codes to the rarest symbols."""
    f = sorted((x for x in freqs if x), reverse=True)
    best = None
    for lens in itertools.combinations_with_replacement(range(1, limit + 1), len(f)):
        if sum(2.0 ** -ln for ln in lens) <= 1.0:
            cost = sum(a * b for a, b in zip(f, lens))
            best = cost if best is None else min(best, cost)
    return best


def test_limited_lengths_are_optimal():
    rng = np.random.default_rng(7)
    cost = lambda f, lens: sum(a * b for a, b in zip(f, lens))
    for trial in range(300):
        n = int(rng.integers(2, 20))
        f = [int(x) for x in (rng.integers(1, 6, n) if trial % 3 else 2 ** rng.integers(0, 9, n))]
        f += [0] * int(rng.integers(0, 3))
        for limit in (5, 7, 15):
            lens = dm.limited_lengths(f, limit)
            assert dm.kraft(lens) == 1 << 15 and max(lens) <= limit and all(bool(a) == bool(b) for a, b in zip(f, lens))
            assert cost(f, lens) == cost(f, _naive_package_merge(f, limit))
            opt, depth = dm.huffman_cost_and_depth(f)
            assert cost(f, lens) >= opt and (depth > limit or cost(f, lens) == opt)
    for f in ([1, 1, 2, 3, 5, 8, 13], [1, 2, 4, 8, 16, 32], [3, 3, 3, 3, 3], [1, 1, 1, 1, 50, 50]):
        for limit in (3, 4):
            assert cost(f, dm.limited_lengths(f, limit)) == _brute_force_cost(f, limit)
    # large alphabets: Huffman's cost whenever its tree fits
    for seed in range(5):
        f = [int(x) for x in np.random.default_rng(seed).geometric(0.02, 286)]
        opt, depth = dm.huffman_cost_and_depth(f)
        lens = dm.limited_lengths(f, 15)
        assert depth <= 15 and cost(f, lens) == opt and dm.kraft(lens) == 1 << 15
    assert dm.limited_lengths([0, 9, 0], 15) == [0, 1, 0] and dm.limited_lengths([0, 0], 7) == [0, 0]


def test_fibonacci_block_needs_the_limit():
    blk = dm.fibonacci_block()
    ll, d, _ = dm.histograms(list(blk.tobytes()))
    assert sorted(x for x in ll if x) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584] and not any(d)
    opt, depth = dm.huffman_cost_and_depth(ll)
    lens = dm.limited_lengths(ll, 15)
    assert depth >= 16 and max(lens) == 15 and dm.kraft(lens) == 1 << 15
    assert sum(a * b for a, b in zip(ll, lens)) > opt


def test_rle_rule():
    assert dm.rle_lengths([0] * 138) == [(18, 127)] and dm.rle_lengths([0] * 139) == [(18, 127), (0, 0)]
    assert dm.rle_lengths([0] * 141) == [(18, 127), (17, 0)] and dm.rle_lengths([0] * 10) == [(17, 7)] and dm.rle_lengths([0] * 11) == [(18, 0)]
    assert dm.rle_lengths([0, 0]) == [(0, 0), (0, 0)]
    assert dm.rle_lengths([5] * 3) == [(5, 0)] * 3 and dm.rle_lengths([5] * 4) == [(5, 0), (16, 0)]
    assert dm.rle_lengths([5] * 7) == [(5, 0), (16, 3)] and dm.rle_lengths([5] * 9) == [(5, 0), (16, 3), (5, 0), (5, 0)]
    assert dm.rle_lengths([5] * 10) == [(5, 0), (16, 3), (16, 0)]
    assert dm.rle_lengths([4, 4, 0, 0, 0, 7]) == [(4, 0), (4, 0), (17, 0), (7, 0)]


@pytest.mark.parametrize("content", ["zeros", "random", "random0to3", "prefix_image", "regions_like", "alternating"])
def test_model_streams_inflate(content):
    for n, mb, row, near in ((0, 40_000, 0, 1), (1, 40_000, 7, 1), (259, 40_000, 192, 2), (16385, 40_000, dm.IMG_W, 1),
                             (50_001, 20_000, dm.IMG_W, 2), (50_001, 20_000, 32769, 16)):
        payload = dm.CONTENTS[content](n).tobytes()
        streams, records = dm.encode_model(payload, mb, row, near)
        assert len(streams) == max(1, -(-n // mb))
        for m, body in enumerate(streams):
            d = zlib.decompressobj(-15)
            got = d.decompress(body) + d.flush()
            assert d.eof and d.unused_data == b"" and got == payload[m * mb:(m + 1) * mb], (content, n, m)
        assert sum(len(s) for s in streams) == sum(r[("stored_bytes", "fixed_bytes", "dynamic_bytes")[r["type"]]] for r in records)
        # the reader sees the blocks the model wrote (an empty stored block follows every non-final one)
        seen = [b for body in streams for b in dm.parse_blocks(body) if not (b["type"] == 0 and not b["data"] and not b["final"])]
        assert [b["type"] for b in seen] == [r["type"] for r in records]
        for b, r in zip(seen, records):
            if b["type"]:
                assert b["tokens"] == r["tokens"]
            if b["type"] == 2:
                assert b["payload_bits"] == r["payload_bits"] and b["header_bits"] == r["header_bits"]
    if content == "random":
        assert {r["type"] for r in records} == {0}
    if content in ("random0to3", "regions_like"):
        assert 2 in {r["type"] for r in records}


@functools.lru_cache(maxsize=None)
def _phantom_payload(name):
    from boa_hip import synthetic
    return np.asfortranarray(getattr(synthetic, f"label_phantom_{name}")((192, 160, 128))).reshape(-1, order="F").tobytes()


# device body sizes of the fixed-code encoder on the 192 x 160 x 128 phantoms, row_bytes = 192, 4 MiB members
DEVICE_FIXED_BYTES = {"total": 178_465, "regions": 186_301, "parts": 61_736}


@pytest.mark.parametrize("name", sorted(DEVICE_FIXED_BYTES))
def test_fixed_code_model_matches_the_recorded_device_sizes(name):
    payload = _phantom_payload(name)
    streams, records = dm.encode_model(payload, 4 << 20, 192, 1, dynamic=False)
    size = sum(len(s) for s in streams)
    print(f"{name}: model fixed {size} B, device {DEVICE_FIXED_BYTES[name]} B")
    assert abs(size - DEVICE_FIXED_BYTES[name]) <= 0.002 * DEVICE_FIXED_BYTES[name]
    assert b"".join(zlib.decompress(s, -15) for s in streams) == payload
