"""csrc/rle_codes.h on the host: the control step, the entry maps by pointer doubling, the chain walk, the marking of a chunk's
runs and the run lookup that the RLE kernels call, compiled into tools/rle_codes_host.cpp with the address and undefined-behaviour
sanitizers, run as a child process and compared with the plain walks of tests/rle_writer.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import rle_writer as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (256, 1024)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("rle_codes") / "rle_codes_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "body-and-organ-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tools", "rle_codes_host.cpp"), "-o", str(exe)])

    def ask(*requests):
        r = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        return [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    return ask


def _segments():
    """(name, segment, wanted): the libtiff strips, seeded random byte strings (any byte string is a control chain), strings
    rich in no-ops and in long literals, and the boundary cases of both chunk sizes."""
    g = np.load(os.path.join(GOLDEN, "rle", "packbits_libtiff.npz"))
    out = []
    for i in range(2):
        for k in range(2):
            out.append((f"golden_{i}_{k}", g[f"strip_{i}_{k}"].tobytes(), g[f"source_{i}"].size))
    rng = np.random.default_rng(11)
    for n in (0, 1, 2, 129, 255, 256, 257, 1023, 1024, 1153, 3000):
        out.append((f"random_{n}", rng.integers(0, 256, n, dtype=np.uint8).tobytes(), 2 * n + 7))
    out.append(("random_noops", rng.choice(np.array([0x80, 0x80, 0x80, 0, 255, 127], dtype=np.uint8), 2500).tobytes(), 4000))
    out.append(("random_long_literals", rng.integers(100, 128, 2500, dtype=np.uint8).tobytes(), 2000))
    out.append(("random_repeats", rng.integers(129, 256, 2500, dtype=np.uint8).tobytes(), 1 << 20))
    for cb in CHUNKS:
        out += [(f"{name}_{cb}", seg, wanted) for name, (seg, wanted) in R.boundary_cases(cb).items()]
    return out


SEGMENTS = _segments()


@pytest.mark.parametrize("cb", CHUNKS)
def test_entry_maps_of_every_chunk(host, cb):
    reqs, want = [], []
    for _, seg, _ in SEGMENTS:
        reqs += ["seg " + seg.hex(), f"map {cb}"]
        want += [R.chunk_map(seg, cb, k) for k in range(R.n_chunks(seg, cb))]
    assert host(*reqs) == want


@pytest.mark.parametrize("cb", CHUNKS)
def test_chain_walk(host, cb):
    """Entries, output bases and the total, for the wanted count of the case, a smaller one (the chain ends early: the chunks
    behind are not live) and a larger one (truncated)."""
    reqs, want = [], []
    for _, seg, wanted in SEGMENTS:
        tables = [R.chunk_map(seg, cb, k) for k in range(R.n_chunks(seg, cb))]
        reqs.append("seg " + seg.hex())
        for w in (wanted, max(1, wanted // 3), wanted + 1000):
            total, entries, bases = R.chain(tables, w)
            reqs.append(f"chain {cb} {w}")
            want += [[total, len(tables)], entries, bases]
    assert host(*reqs) == want


@pytest.mark.parametrize("cb", CHUNKS)
def test_run_lists_and_lookup(host, cb):
    """The run list of every live chunk, and the output assembled by looking up the run of every byte: the model's bytes and
    status, also where the wanted count clips the last run or the segment is truncated."""
    reqs, want = [], []
    for name, seg, wanted in SEGMENTS:
        tables = [R.chunk_map(seg, cb, k) for k in range(R.n_chunks(seg, cb))]
        reqs.append("seg " + seg.hex())
        for w in (wanted, max(1, wanted // 3)):
            total, entries, _ = R.chain(tables, w)
            reqs.append(f"runs {cb} {w}")
            want += [[k] + [v for run in R.chunk_runs(seg, cb, k, e) for v in run] for k, e in enumerate(entries) if e != R.NOT_LIVE]
            out, st = R.decode_segment(seg, w)
            assert R.chunked_decode(seg, cb, w) == (out, st), name
            reqs += [f"expand {cb} {w}", f"serial {w}"]
            want += [[st, len(out), R.fnv(out + bytes(w - len(out)))]] * 2
    # (the host program zero-fills its output as the model does, so a truncated segment's bytes compare too)
    assert host(*reqs) == want


def test_step_bounds():
    """What the word layouts of rle_codes.h rest on: a step advances by 1 .. 129 and produces at most 128 bytes per two
    stream bytes, so a 4096-byte chunk produces at most 2^18."""
    steps = [R.step(c) for c in range(256)]
    assert min(a for a, _ in steps) == 1 and max(a for a, _ in steps) == 129
    assert all(out <= 128 and (out == 0 or adv >= 2) for adv, out in steps)
    seg = bytes([129, 7]) * 2048
    assert R.chunk_map(seg, 4096, 0)[0] == 1 << 18
