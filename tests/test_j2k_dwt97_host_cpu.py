"""csrc/j2k_dwt97.h on the host: the lowest coded plane, the dequantisation, the one-dimensional 9/7 synthesis and the sample
conversion that the kernels of j2k.hip call, compiled into tools/j2k_dwt97_host.cpp with -ffp-contract=off and the address and
undefined-behaviour sanitizers, run as a child process and compared bit for bit with the numpy model (tests/j2k97_reference.py)
and with OpenJPEG's decode of the fixtures of tests/golden/j2k97."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import j2k97_fixtures as FX
import j2k97_reference as M
import j2k_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = FX.load_fixtures()
F = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("j2k_dwt97") / "j2k_dwt97_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "body-and-organ-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tools", "j2k_dwt97_host.cpp"), "-o", str(exe)])

    def ask(*requests, status=0):
        r = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True)
        assert r.returncode == status, r.stderr[-4000:]
        return [np.array(ln.split(), dtype=np.int64) for ln in r.stdout.splitlines()]
    return ask


def _bits(a):
    return " ".join(map(str, np.ascontiguousarray(a, dtype=F).view(np.uint32).ravel().tolist()))


def _floats(a):
    return a.astype(np.uint32).view(F)


def _same_bits(got, want, msg=""):
    np.testing.assert_array_equal(got.astype(np.uint32), np.ascontiguousarray(want, dtype=F).view(np.uint32).ravel(), err_msg=msg)


def test_synthesis_of_every_short_length_and_edge(host):
    """Lengths 1 .. 19 and 64 / 65 (every mirror case of the +-4 window, both parities), noise of a large range."""
    rng = np.random.default_rng(2)
    reqs, want = [], []
    for n in list(range(1, 20)) + [64, 65]:
        for scale in (1.0, 3.0e4):
            x = (rng.standard_normal(n) * scale).astype(F)
            reqs.append(f"syn {n} {_bits(x)}")
            want.append(M.idwt97_1d(x, 0))
    for got, w in zip(host(*reqs), want):
        _same_bits(got, w, f"n = {len(w)}")
    assert _floats(host(f"syn 1 {_bits([7.25])}")[0])[0] == F(7.25)          # a length-1 signal passes through unscaled


def test_lowest_coded_plane_and_dequantisation_of_cut_blocks(host):
    """Blocks of the two 40 x 33 fixtures cut at every pass count: the header's b_last rule on the decoded magnitudes equals the
    plane the model tracks per coefficient, and the dequantised coefficients equal the model's."""
    reqs, want = [], []
    for name in ("40x33_u8_lrcp_2layers", "40x33_s8_random"):
        fr = FX.parse(next(f for f in FIXTURES if f["name"] == name))
        off = 0
        for k, (o, x0, y0, w, h, nbp, own, ln) in enumerate(fr.blocks.tolist()):
            sh = F(0.5) * fr.steps[fr.band[k]]
            for P in range(1, own + 1):
                v, last, ok = R.decode_block(fr.data, off, ln, w, h, o, nbp, P, with_last=True)
                assert ok
                sig = last >= 0
                if not sig.any():
                    continue
                half = np.where(last >= 1, 1 << np.maximum(last - 1, 0), 0) if P < 3 * nbp - 2 else 0
                t = (np.sign(v) * (np.abs(v) - half))[sig]                      # the magnitude bits, without the midpoint
                kf, bf = (2 if P == 1 else (P - 2) % 3), nbp - 1 - (P + 1) // 3
                reqs.append(f"blast {kf} {bf} " + " ".join(map(str, np.abs(t).tolist())))
                want.append(last[sig])
                reqs.append(f"deq {_bits([sh])} " + " ".join(f"{a} {b}" for a, b in zip(t.tolist(), last[sig].tolist())))
                q = M.quantised(v, last)[sig]
                want.append((q.astype(np.int32).astype(F) * sh).view(np.uint32).astype(np.int64))
            off += ln
    assert len(reqs) > 200
    for got, w in zip(host(*reqs), want):
        np.testing.assert_array_equal(got, w)


def test_dequantisation_extremes(host):
    sh = F(0.5) * F(1.75)
    got = _floats(host(f"deq {_bits([sh])} 0 0 1 0 -1 0 {(1 << 30) - 1} 0 {-(1 << 30) + 1} 0 {1 << 29} 29 {3 << 28} 28 -8 3")[0])
    want = np.array([0, 3, -3, (1 << 31) - 1, -(1 << 31) + 1, (1 << 30) + (1 << 29), (3 << 29) + (1 << 28), -24],
                    dtype=np.int64).astype(np.int32).astype(F) * sh
    _same_bits(got.view(np.uint32), want)
    assert np.signbit(got[0]) == False and got[0] == 0                       # zero stays +0.0f


def test_samples_round_to_even_shift_and_clamp(host):
    vals = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, 127.5, 126.5, 32767.5, 32766.5, -32768.5, -32769.5, 1e9, -1e9,
                     3e38, -3e38, np.inf, -np.inf, np.nan, -0.0, 65535.0, 131072.5], dtype=F)
    for P, sg in ((8, 0), (8, 1), (16, 0), (16, 1), (12, 0), (1, 0)):
        got = host(f"sam {P} {sg} {_bits(vals)}")[0]
        finite = np.nan_to_num(vals, nan=-np.inf)
        np.testing.assert_array_equal(got, M.samples(finite, P, bool(sg)), err_msg=f"P {P} signed {sg}")


@pytest.mark.parametrize("fx", FIXTURES, ids=[f["name"] for f in FIXTURES])
def test_fixture_plane_to_samples(host, fx):
    """The model's dequantised plane of the fixture through the header's synthesis, strung together per level as the kernels do:
    OpenJPEG's samples."""
    fr = FX.parse(fx)
    _, plane = FX.model(fx)
    got = host(f"frame {fr.rows} {fr.cols} {fr.levels} {fr.precision} {int(fr.signed)} {_bits(plane)}")[0]
    np.testing.assert_array_equal(got.reshape(fr.rows, fr.cols), FX.expected(fx))


def test_requests_outside_the_admitted_ranges_end_the_program(host):
    for bad in ("deq 1065353216 5 1", "deq 1065353216 1 31", "blast 3 0 1", "sam 17 0 0", "syn 0", "frame 2 2 1 16 0 1 2 3", "what"):
        host(bad, status=2)
