"""csrc/jls_codes.h on the host: the parameter derivation, the stuffed bit stream, the limited Golomb code, the sample rules and the
row chain that the JPEG-LS kernels call, compiled into tools/jls_codes_host.cpp with the address and undefined-behaviour
sanitizers, run as a child process on whole scans (through the plain loop of k_jls_serial and through the row structure of
k_jls_wave) and compared, samples and status, with the Python model of tests/jls_model.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
import jls_model as M
import jls_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("jls_codes") / "jls_codes_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "body-and-organ-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tools", "jls_codes_host.cpp"), "-o", str(exe)])

    def ask(*requests):
        r = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        return [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    return ask


def fnv(px) -> int:
    h = 1469598103934665603
    for v in np.ascontiguousarray(px, dtype="<u2").tobytes():
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _ct_like(shape, bits, seed):
    rng = np.random.default_rng(seed)
    rows, cols = shape
    yy, xx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    body = ((yy - rows / 2) ** 2 / max(rows * 0.4, 1) ** 2 + (xx - cols / 2) ** 2 / max(cols * 0.4, 1) ** 2) < 1
    v = np.where(body, 1064 + rng.integers(-200, 201, shape), 24)
    return (v << (bits - 12) if bits >= 12 else v >> (12 - bits)).astype(np.int64)


def _scans():
    """(name, scan, rows, cols, Params): CharLS's scans, the writer's on shapes around the lane count and at every precision,
    with and without NEAR, and damaged ones: cut, a marker planted, zero bytes, noise."""
    out = []
    g = np.load(os.path.join(GOLDEN, "jls", "charls.npz"))
    for name in [k[7:] for k in g.files if k.startswith("stream_")]:
        out.append((name,) + M.scan_of(g["stream_" + name].tobytes()))
    rng = np.random.default_rng(3)
    for shape in ((1, 1), (1, 70), (70, 1), (5, 63), (5, 64), (5, 65), (9, 130)):
        for bits, near in ((8, 0), (12, 3), (16, 0), (2, 0), (16, 40)):
            p = M.Params((1 << bits) - 1, near)
            for kind, img in (("ct", _ct_like(shape, bits, sum(shape)) & ((1 << bits) - 1)), ("noise", rng.integers(0, 1 << bits, shape))):
                out.append((f"{kind}{bits}_{shape[0]}x{shape[1]}_near{near}", W.encode_scan(img, p)[0], shape[0], shape[1], p))
    p = M.Params(4095, 0, 9, 30, 100, 31)
    out.append(("lse", W.encode_scan(_ct_like((20, 40), 12, 1), p)[0], 20, 40, p))
    p = M.Params(255)
    out.append(("constant_wide", W.encode_scan(np.full((2, 5000), 7), p)[0], 2, 5000, p))
    name, scan, rows, cols, p = out[3]
    for tag, bad in (("half", scan[:len(scan) // 2]), ("last_byte", scan[:-1]), ("marker", scan[:200] + b"\xFF\x90" + scan[202:]),
                     ("zeros", bytes(len(scan))), ("ones", b"\xFF\x7F" * 100), ("empty", b""), ("noise", rng.integers(0, 256, 900, dtype=np.uint8).tobytes()),
                     ("noise_no_ff", rng.integers(0, 255, 900, dtype=np.uint8).tobytes())):
        out.append((f"{name}_{tag}", bad, rows, cols, p))
    return out


SCANS = _scans()


def test_whole_scans_plain_and_wave(host):
    reqs, want, names = [], [], []
    statuses = set()
    for name, scan, rows, cols, p in SCANS:
        px, st, _ = M.decode_scan(scan, rows, cols, p)
        statuses.add(st)
        args = " ".join(str(v) for v in [rows, cols] + p.words())
        reqs += ["scan " + scan.hex(), "plain " + args, "wave " + args]
        want.append((st, fnv(px)))
        names.append(name)
    assert statuses == {M.OK, M.TRUNCATED, M.INVALID}
    got = host(*reqs)
    for k, name in enumerate(names):
        st, h = want[k]
        assert got[2 * k] == [st, h], f"plain {name}"
        assert got[2 * k + 1][0] == st and (st != M.OK or got[2 * k + 1][1] == h), f"wave {name}"


def test_parameter_derivation(host):
    """Defaults and derived values for every MAXVAL a precision gives, LSE-like odd MAXVALs and a sweep of NEAR; the validity
    ranges of T.87 C.2.4.1.1."""
    cases = [((1 << b) - 1, n) for b in range(2, 17) for n in (0, 1, 2, 7, 255) if n <= min(255, ((1 << b) - 1) // 2)]
    cases += [(m, n) for m in (1, 5, 100, 127, 128, 1000, 4000, 5000, 65534) for n in (0, 3) if n <= m // 2]
    reqs, want = [], []
    for maxval, near in cases:
        p = M.Params(maxval, near)
        reqs += [f"defaults {maxval} {near}", "derive " + " ".join(str(v) for v in p.words())]
        want += [[p.t1, p.t2, p.t3], [1, p.range, p.qbpp, p.bpp, p.limit, p.a0]]
    assert host(*reqs) == want
    assert (M.Params(4095).words()[2:5], M.Params(65535).words()[2:5], M.Params(255).words()[2:5]) == ([18, 67, 276], [18, 67, 276], [3, 7, 21])
    assert (M.Params(65535).limit, M.Params(4095).limit, M.Params(255).limit, M.Params(65535).a0, M.Params(255).a0) == (64, 48, 32, 1024, 4)
    bad = ["0 0 1 1 1 64", "65536 0 18 67 276 64", "255 128 129 129 129 64", "255 0 0 7 21 64", "255 0 3 2 21 64", "255 0 3 7 6 64",
           "255 0 3 7 256 64", "255 0 3 7 21 2", "255 0 3 7 21 256", "255 3 3 7 21 64", "4095 256 300 300 300 64"]
    assert host(*["derive " + b for b in bad]) == [[0] * 6] * len(bad)
    assert host("derive 4095 0 18 67 276 4095", "derive 255 127 128 128 128 255")[0][0] == 1
