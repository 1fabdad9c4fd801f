"""Pins tests/label_mask_cases.py: every case holds what it claims (present and absent pairs, single voxels on member boundaries),
and the host restatement of the presence table is right -- against a plain loop that shares nothing with it."""
import zlib

import numpy as np
import pytest

import label_mask_cases as lm

CASES = {c["name"]: c for c in lm.cases()}


def _slow_presence(payload, member_bytes):
    n = len(payload)
    rows = [set() for _ in range(lm.n_members(n, member_bytes))]
    for i, v in enumerate(payload.tolist()):
        rows[i // member_bytes].add(v)
    return rows


def test_the_table_covers_what_the_gpu_test_relies_on():
    assert set(CASES) >= {"n0", "n1", "n15", "n17_members_of_16", "unaligned", "last_member_one_byte", "first_and_last_byte_of_a_member",
                          "only_in_the_short_last_member", "one_label_fills", "random_labels", "random_bits", "ids_0_and_255",
                          "three_blocks_and_a_tail", "three_blocks_and_a_tail_4MiB"}
    assert [len(CASES[k]["payload"]) for k in ("n0", "n1", "n15", "n17_members_of_16")] == [0, 1, 15, 17]
    assert CASES["unaligned"]["shift"] == 1 and all(c["shift"] == 0 for k, c in CASES.items() if k != "unaligned")
    c = CASES["last_member_one_byte"]
    assert len(c["payload"]) % c["member_bytes"] == 1
    c = CASES["three_blocks_and_a_tail"]
    assert len(c["payload"]) == 3 * lm.BLK + 5 == c["member_bytes"]
    c = CASES["one_label_fills"]
    assert len(set(c["payload"].tolist())) == 1 and c["member_bytes"] % 16 != 0 and c["member_bytes"] > lm.BLK
    c = CASES["random_labels"]
    assert len(set(c["payload"].tolist())) == 255
    c = CASES["ids_0_and_255"]
    assert {k for k, _ in c["present"]} >= {0, 255}
    c = CASES["first_and_last_byte_of_a_member"]
    assert c["member_bytes"] > 2 * lm.BLK and c["member_bytes"] % lm.BLK


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_holds_what_it_claims(name):
    c = CASES[name]
    payload, mb = c["payload"], c["member_bytes"]
    n = len(payload)
    table = lm.presence_table(payload, mb)
    assert table.shape == (lm.n_members(n, mb), 256)
    assert c["absent"], "every case lists an absent pair"
    assert c["present"] or n == 0, "every case but the empty one lists a present pair"
    for k, m in c["present"]:
        assert table[m, k], (k, m)
        assert any(lm.pair_payload(payload, mb, k, m))
    for k, m in c["absent"]:
        assert m < table.shape[0] and not table[m, k], (k, m)
        body = lm.pair_payload(payload, mb, k, m)
        assert not any(body) and len(body) == len(payload[lm.member_slice(n, mb, m)])
    for k, index, m, off in c["boundary"]:
        sl = lm.member_slice(n, mb, m)
        assert payload[index] == k and index == (sl.start + off if off >= 0 else sl.stop - 1)
        assert int((payload[sl] == k).sum()) == 1, "the label's only voxel of that member"
        assert int((payload == k).sum()) == 1, "and of the volume"


@pytest.mark.parametrize("name", sorted(CASES))
def test_presence_restatement(name):
    c = CASES[name]
    payload = c["payload"]
    for mb in {c["member_bytes"], 1, 7, 4096} if len(payload) <= 20_000 else {c["member_bytes"]}:
        table = lm.presence_table(payload, mb)
        slow = _slow_presence(payload, mb)
        assert [set(np.flatnonzero(r).tolist()) for r in table] == slow
        words = lm.presence_words(table)
        assert words.shape == (len(slow), 8) and words.dtype == np.dtype("<u4")
        for m, row in enumerate(slow):
            assert {k for k in range(256) if (int(words[m, k >> 5]) >> (k & 31)) & 1} == row


def test_volume_and_pair_payload():
    v = lm.volume()
    assert v.shape == (int(np.prod(lm.VOLUME_SHAPE)),) and lm.PRESENCE_MEMBER_BYTES[-2:] == (v.size, v.size + 1)
    ids = sorted(set(v.tolist()))
    assert ids == list(range(14)) + [254, 255]
    assert v[0] == 13 and v[-1] == 255 and int((v == 255).sum()) == 1
    # spatially coherent: most (label, member) pairs are absent at a member size of a few rows, and both kinds occur for every id but 0
    table = lm.presence_table(v, 4096)
    assert table.shape[0] == 7
    for k in ids[1:]:
        assert table[:, k].any() and not table[:, k].all(), k
    assert table[:, ids].mean() < 0.5
    # a row is 37 bytes: the x-row of 254 is one run
    at = np.flatnonzero(v == 254)
    assert len(at) == 25 and (np.diff(at) == 1).all()
    # the pair payload is the mask's member, its CRC the member's
    mask = (v == 5).astype(np.uint8).tobytes()
    for m in range(7):
        assert lm.pair_payload(v, 4096, 5, m) == mask[m * 4096:(m + 1) * 4096]
        assert lm.pair_crc(v, 4096, 5, m) == zlib.crc32(mask[m * 4096:(m + 1) * 4096])
