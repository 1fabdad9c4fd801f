"""csrc/deflate_codes.h on the host: the symbol, canonical-code and run-length helpers that the deflate kernel calls, compiled into
tools/deflate_codes_host.cpp with the address and undefined-behaviour sanitizers and compared with tests/deflate_model.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import deflate_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("deflate_codes") / "deflate_codes_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "body-and-organ-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tools", "deflate_codes_host.cpp"), "-o", str(exe)])

    def ask(*requests):
        r = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    return ask


def test_length_and_distance_symbols(host):
    out = host("len", "dist", "order")
    assert out[:256] == [list(dm.len_symbol(l)) for l in range(3, 259)]
    assert out[256:256 + 32768] == [list(dm.dist_symbol(d)) for d in range(1, 32769)]
    assert [v[0] for v in out[256 + 32768:]] == dm.CL_ORDER


def _length_sets():
    rng = np.random.default_rng(4)
    sets = [dm.FIXED_LL[:286], dm.FIXED_D, [0] * 285 + [1], [1], [1, 1], [0, 3, 3, 3, 3, 3, 2, 4, 4], [2, 1, 3, 3]]
    for _ in range(40):
        n = int(rng.integers(2, 287))
        f = [int(x) for x in rng.geometric(float(rng.choice([0.5, 0.05, 0.005])), n) * (rng.random(n) < rng.choice([0.1, 0.5, 1.0]))]
        f[int(rng.integers(0, n))] += 1
        f[0] += 1
        sets.append(dm.limited_lengths(f, int(rng.choice([7, 15])) if n <= 19 else 15))
    sets.append(dm.limited_lengths(dm.histograms(list(dm.fibonacci_block().tobytes()))[0], 15))
    return sets


def test_canonical_codes(host):
    sets = _length_sets()
    out = host(*("codes %d %s" % (len(s), " ".join(map(str, s))) for s in sets))
    for s in sets:
        got, out = out[:len(s)], out[len(s):]
        codes = dm.canonical_codes(s)
        want = [[int(format(codes[k], f"0{ln}b")[::-1], 2), ln] if ln else [0, 0] for k, ln in enumerate(s)]
        assert got == want
    assert not out


def test_run_length_code_of_the_header(host):
    rng = np.random.default_rng(9)
    seqs = [[0] * n for n in (1, 2, 3, 10, 11, 138, 139, 140, 141, 276, 277, 316)] + [[7] * n for n in (1, 3, 4, 6, 7, 8, 9, 10, 11, 70)]
    seqs += [s + [0] for s in _length_sets()[:12]]
    for _ in range(60):
        vals = rng.choice([0, 0, 0, 1, 5, 8, 9, 15], int(rng.integers(1, 60)))
        runs = rng.choice([1, 1, 2, 3, 4, 7, 12, 150], len(vals))
        seqs.append([int(v) for v in np.repeat(vals, runs)[:316]])
    out = host(*("rle %d %s" % (len(s), " ".join(map(str, s))) for s in seqs))
    for s in seqs:
        k = out[0][0]
        want = dm.rle_lengths(s)
        assert k == len(want) <= len(s) and [tuple(v) for v in out[1:1 + k]] == want
        hist = [0] * 19
        for sym, _ in want:
            hist[sym] += 1
        assert [v[0] for v in out[1 + k:1 + k + 19]] == hist
        out = out[1 + k + 19:]
        # what the rule writes is what a decoder expands
        back = []
        for sym, ev in want:
            back += [sym] if sym < 16 else [back[-1]] * (3 + ev) if sym == 16 else [0] * ((3 if sym == 17 else 11) + ev)
        assert back == s
    assert not out
