"""csrc/softmax_codes.h on the host: the fp16 -> fp32 conversion, the fp32 softmax column and the first-maximum label that the
kernels of prob.hip call, compiled into tools/softmax_host.cpp with -ffp-contract=off and the address and undefined-behaviour
sanitizers, run as a child process and compared with the float64 softmax of the same fp16 logits within the derived bound
(tests/softmax_reference.py: (C + 110) 2^-24 relative where p64 > 2^-100, 2^-99 absolute elsewhere)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import softmax_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = (1, 2, 3, 25, 32, 33, 118)
F16 = np.float16


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("softmax_host") / "softmax_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "body-and-organ-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tools", "softmax_host.cpp"), "-o", str(exe)])

    def ask(*requests, status=0):
        r = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True)
        assert r.returncode == status, r.stderr[-4000:]
        return [np.array(ln.split(), dtype=np.int64) for ln in r.stdout.splitlines()]
    return ask


def _bits(h):
    return " ".join(map(str, np.ascontiguousarray(h, dtype=F16).view(np.uint16).ravel().tolist()))


def _planes(host, cols):
    """cols fp16 [C, n] through the `planes` request -> (labels [n], probabilities float32 [C, n])."""
    C, n = cols.shape
    out = host(f"planes {C} {n} {_bits(cols)}")[0]
    assert out.size == n + C * n
    return out[:n], out[n:].astype(np.uint32).view(np.float32).reshape(C, n)


def test_half_conversion_of_every_bit_pattern(host):
    h = np.arange(65536, dtype=np.uint16)
    got = host("cvt " + " ".join(map(str, h.tolist())))[0].astype(np.uint32)
    want = h.view(F16).astype(np.float32)
    nan = np.isnan(want)
    np.testing.assert_array_equal(got[~nan], want.view(np.uint32)[~nan])
    assert np.isnan(got.view(np.float32)[nan]).all()


@pytest.mark.parametrize("C", CLASSES)
def test_columns_within_the_bound_of_float64(host, C):
    """Noise at three scales, +-65504, subnormals, adjacent top pairs at 0 / 1 / 1024 and exact ties."""
    cols = S.families(C)
    labels, p = _planes(host, cols)
    p64 = S.softmax64(cols)
    assert np.isfinite(p).all()
    S.assert_within_bound(p, p64, C, "host columns")
    S.assert_labels(labels, p, p64, C, "host columns")
    # the same columns stored class-contiguous (`col`): the same bits
    got = host(f"col {C} {_bits(cols.T)}")[0].reshape(cols.shape[1], C + 1)
    np.testing.assert_array_equal(got[:, 0], labels)
    np.testing.assert_array_equal(got[:, 1:].T.astype(np.uint32), p.view(np.uint32))


@pytest.mark.parametrize("C", CLASSES)
def test_equal_columns_give_equal_probabilities_and_label_0(host, C):
    vals = np.array([0.0, -0.0, 1.0, -3.5, 65504.0, -65504.0, 6e-8, -6e-8, 1024.0, 0.333], dtype=F16)
    cols = np.broadcast_to(vals, (C, vals.size)).copy()
    labels, p = _planes(host, cols)
    assert (labels == 0).all()
    assert (p.view(np.uint32) == p.view(np.uint32)[0]).all()          # exactly equal
    np.testing.assert_array_equal(p[0], np.float32(1.0) / np.float32(C))


@pytest.mark.parametrize("C", [c for c in CLASSES if c > 1])
def test_first_maximum_wins_exact_ties(host, C):
    rng = np.random.default_rng(C)
    cols = np.minimum(rng.standard_normal((C, 4 * C)) * 2, 8.0).astype(F16)      # (below the planted maximum of 9)
    want = []
    for k in range(cols.shape[1]):
        i = k % C
        j = (i + 1 + (k // C) * 3) % C
        cols[[i, j], k] = F16(9.0)
        want.append(min(i, j))
    labels, p = _planes(host, cols)
    np.testing.assert_array_equal(labels, want)
    S.assert_labels(labels, p, S.softmax64(cols), C, "ties")


@pytest.mark.parametrize("C", CLASSES)
def test_extremes_do_not_trip_the_sanitizers(host, C):
    """-65504 against +65504 (x - m = -131008: expf underflows to 0), every probability finite, the column sums to 1."""
    cols = np.full((C, 3), -65504.0, dtype=F16)
    cols[C - 1, 0] = 65504.0
    cols[0, 1] = 65504.0
    cols[:, 2] = 65504.0
    labels, p = _planes(host, cols)
    assert np.isfinite(p).all()
    np.testing.assert_array_equal(labels[:2], [C - 1, 0])
    assert labels[2] == 0
    if C > 1:
        assert p[C - 1, 0] == 1.0 and p[0, 1] == 1.0 and (p[:C - 1, 0] == 0).all() and (p[1:, 1] == 0).all()
    S.assert_within_bound(p, S.softmax64(cols), C, "extremes")


@pytest.mark.parametrize("C", CLASSES)
def test_nan_column_gives_nan_probabilities_and_label_0(host, C):
    cols = S.nan_columns(C)
    labels, p = _planes(host, cols)
    assert np.isnan(p).all()
    assert (labels == 0).all()


def test_requests_outside_the_admitted_ranges_end_the_program(host):
    for bad in ("col 0 1", "col 256 1", "col 3 1 2", "col 2 1 65536", "col 2 1 x", "planes 2 2 1 2 3", "planes 2 0", "cvt 70000",
                "cvt -1", "what"):
        host(bad, status=2)
