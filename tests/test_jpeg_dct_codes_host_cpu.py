"""csrc/jpeg_dct_codes.h (over csrc/jpeg_huff.h) on the host: the codeword step, the zig-zag table, libjpeg's islow passes and
range limit that the kernels of jpeg_dct.hip call, compiled into tools/jpeg_dct_host.cpp with the address and undefined-behaviour
sanitizers, run as a child process and compared with the Python model of tests/jpeg_dct_model.py: codeword by codeword, whole
restart intervals through the loop of k_jd_serial and through the phases of k_jd_parallel, and the committed fixtures' samples."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_dct_model as M
import jpeg_dct_writer as W
from boa_hip.jpeg_lossless import expand_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    out = tmp_path_factory.mktemp("jpeg_dct_codes") / "jpeg_dct_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "body-and-organ-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tools", "jpeg_dct_host.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def host(exe):
    def ask(*requests):
        r = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        return [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    return ask


def fnv(v) -> int:
    h = 1469598103934665603
    for b in np.ascontiguousarray(v).astype("<u2").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _setup(p):
    """The requests that load a parsed stream's tables."""
    return ["tab dc " + expand_table(*p["dc"]).astype("<u4").tobytes().hex(), "tab ac " + expand_table(*p["ac"]).astype("<u4").tobytes().hex(),
            "qt " + p["qt"].astype("<u2").tobytes().hex()]


def _coef_hash(coef):
    return fnv(coef.astype(np.int64) & 0xFFFF)


def _streams():
    rng = np.random.default_rng(8)
    out = [(n, s) for which in ("p8", "p12") for n, (s, _) in W.fixtures(which).items()]
    for P in (8, 12):
        dense = W.random_coefficients(rng, 12, P, density=0.9, amp=1 << (P - 1), dc_amp=1 << (P + 2))
        out.append((f"dense{P}", W.encode(dense, rows=24, cols=32, P=P, optimal=True)))
        sparse = np.zeros((12, 64), dtype=np.int64)
        sparse[::2, 63] = 3                               # no EOB, three ZRL ahead of the last coefficient
        sparse[1::2, 17] = -1
        sparse[:, 0] = rng.integers(-(1 << (P + 1)), 1 << (P + 1), 12)
        out.append((f"zrl{P}", W.encode(sparse, rows=24, cols=32, P=P, optimal=True)))
        out.append((f"eob{P}", W.encode(np.zeros((12, 64), dtype=np.int64), rows=24, cols=32, P=P)))
    return out


def test_codeword_steps_and_whole_intervals(host):
    reqs, want = [], []
    for name, stream in _streams():
        p = M.parse(stream)
        steps = []
        coef, st = M.decode_coefficients(p, steps)
        assert st == M.OK, name
        nb = len(coef)
        reqs += _setup(p) + ["seg " + p["segments"][0].hex()]
        for _, at, k, ln, knext, zz, val in steps[:400]:
            reqs.append(f"step {at} {k} {p['P']}")
            want.append((name, [0, ln, knext, zz, val]))
        for req in (f"serial {p['P']} {nb}", f"parallel {p['P']} {nb} 4", f"parallel {p['P']} {nb} 16", f"parallel {p['P']} {nb} 4096"):
            reqs.append(req)
            want.append((name + " " + req, [0, _coef_hash(coef)]))
        reqs.append(f"pixels {p['P']} {p['rows']} {p['cols']}")
        want.append((name + " pixels", [0, fnv(M.pixels(coef, p["qt"], p["P"], p["rows"], p["cols"]))]))
    got = host(*reqs)
    assert len(got) == len(want)
    for g, (what, w) in zip(got, want):
        assert g == w, what


def test_fixture_samples(host):
    reqs, want = [], []
    for which in ("p8", "p12"):
        for name, (stream, px) in W.fixtures(which).items():
            p = M.parse(stream)
            reqs += _setup(p) + ["seg " + p["segments"][0].hex(), f"pixels {p['P']} {p['rows']} {p['cols']}"]
            want.append([0, fnv(px)])
    assert host(*reqs) == want


def test_malformed_intervals_report_the_models_status(host):
    rng = np.random.default_rng(5)
    P = 12
    coef = W.random_coefficients(rng, 12, P, density=0.6)
    p = M.parse(W.encode(coef, rows=24, cols=32, P=P))            # the Annex K tables: no code of all 1 bits, SSSS 11 absent from AC
    seg = p["segments"][0]
    cases = {"cut": seg[:len(seg) // 2], "cut one byte": seg[:-1], "ones": seg[:20] + b"\xFF" * 8 + seg[20:], "empty": b"",
             "trailing": seg + bytes(9), "noise": bytes(rng.integers(0, 256, 300, dtype=np.uint8))}
    # a run past the block: fifteen zeros and a coefficient from zig-zag index 60
    bad = np.zeros((12, 64), dtype=np.int64)
    bad[:, 0] = 5
    bad[3, M.ZIGZAG[60]] = 1
    good_seg = M.parse(W.encode(bad, rows=24, cols=32, P=P))["segments"][0]
    reqs, want, seen = _setup(p), [], set()
    for what, s in cases.items():
        q = dict(p, segments=[s])
        c, st = M.decode_coefficients(q)
        seen.add(st)
        reqs += ["seg " + s.hex(), f"serial {P} 12", f"parallel {P} 12 4", f"parallel {P} 12 16"]
        want += [(what, st)] * 3
    assert {M.TRUNCATED, M.INVALID_CODE, M.TRAILING} <= seen
    got = host(*reqs)
    for g, (what, st) in zip(got, want):
        assert g[0] == st, what
    # the same interval at P = 8 holds DC differences of SSSS 12: refused there only
    wide = np.zeros((12, 64), dtype=np.int64)
    wide[::2, 0] = 2500
    pw = M.parse(W.encode(wide, rows=24, cols=32, P=12, optimal=True))
    got = host(*(_setup(pw) + ["seg " + pw["segments"][0].hex(), "serial 12 12", "serial 8 12", "parallel 8 12 4"]))
    assert [g[0] for g in got] == [M.OK, M.BAD_SSSS, M.BAD_SSSS]
    assert M.decode_coefficients(dict(pw, P=8))[1] == M.BAD_SSSS
    # a run past the block: the codewords of a valid block (three ZRL from k = 1, then run 11 to zig-zag index 60) decoded
    # from a later k than the one they were written at
    steps = []
    M.decode_coefficients(M.parse(W.encode(bad, rows=24, cols=32, P=P)), steps)
    at = next(s for s in steps if s[5] == 60)
    zrl = next(s for s in steps if s[5] == -1 and s[4] == 17)
    assert at[2] == 49
    got = host(*(_setup(p) + ["seg " + good_seg.hex(), f"step {at[1]} 49 {P}", f"step {at[1]} 53 {P}", f"step {zrl[1]} 48 {P}",
                              f"step {zrl[1]} 49 {P}"]))
    assert [g[0] for g in got] == [M.OK, M.RUN_PAST_BLOCK, M.OK, M.RUN_PAST_BLOCK] and got[2][1:] == [zrl[3], 0, -1, 0]


def test_range_limit_and_blocks(host):
    rng = np.random.default_rng(3)
    reqs, want = [], []
    for P in (8, 12):
        mx = (1 << P) - 1
        qt = np.ones(64, dtype=np.int64)
        qt[0] = 64                                           # a DC of d moves every sample by 8 d
        p = M.parse(W.fixtures("p8")["64x64_q75"][0])
        reqs += _setup(dict(p, qt=qt))
        for dc in (0, 3, -3, mx // 16, -(mx // 16) - 1, mx // 8, -(mx // 8), mx // 4, -(mx // 4), 3 * mx // 8 + 5, -(3 * mx // 8), 32767, -32768):
            c = np.zeros(64, dtype=np.int64)
            c[0] = dc
            c[1:] = rng.integers(-3, 4, 63)
            reqs.append(f"block {P} " + " ".join(str(int(v)) for v in c))
            want.append([int(v) for v in M.idct_blocks(c[None], qt, P).ravel()])
        wild = rng.integers(-32768, 32768, 64)
        reqs.append(f"block {P} " + " ".join(str(int(v)) for v in wild))
        want.append([int(v) for v in M.idct_blocks(wild[None], qt, P).ravel()])
    got = host(*reqs)
    assert got == want
    flat = np.array(want)
    assert flat.min() == 0 and flat.max() == 4095


def test_requests_outside_the_admitted_ranges_end_with_an_error(exe):
    p = M.parse(W.fixtures("p8")["64x64_q75"][0])
    seg = "seg " + p["segments"][0].hex()
    for bad in ("step 0 0 8", "\n".join(_setup(p) + [seg, "step 0 64 8"]), "\n".join(_setup(p) + [seg, f"step {8 * len(p['segments'][0])} 0 8"]),
                "\n".join(_setup(p) + [seg, "step 0 0 10"]), "\n".join(_setup(p) + [seg, "serial 8 0"]),
                "\n".join(_setup(p) + [seg, "parallel 8 4 3"]), "\n".join(_setup(p) + [seg, "pixels 8 5000 8"]),
                "tab dc 00", "\n".join(_setup(p) + ["frobnicate"])):
        r = subprocess.run([exe], input=bad + "\n", capture_output=True, text=True)
        assert r.returncode == 2, bad[:40]
