"""csrc/conv_sched.h on the host: the tile schedule k_conv_ws / k_conv_ns walk -- virtual workgroups, grid, the run table of a layer,
the descriptor row length and a workgroup's tile count -- compiled into tools/conv_sched_host.cpp with the address and
undefined-behaviour sanitizers, run as a child process over a sweep of tiles per sample, both CU counts and both tile orders, and
compared with numpy restatements of what the device-side walk (csrc/conv_ws_dev.h: decode_tile, TileSeq) expects of them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILES = list(range(1, 600)) + [1000, 1024, 2047, 2048, 4096, 4097, 8192, 32768]
CUS = (256, 104)
BATCHES = 25


def _geometry(T):
    """A layer with T tiles per sample: cout groups, spatial tiles per axis (x, y, z) and a tile's extent."""
    ncy = next(c for c in (4, 3, 2, 1) if T % c == 0)
    nsp = T // ncy
    t0 = max(d for d in range(1, 9) if nsp % d == 0)
    t2 = max(d for d in range(1, 9) if (nsp // t0) % d == 0)
    return ncy, (t0, nsp // t0 // t2, t2), ((4, 4, 8), (4, 4, 32), (1, 16, 32))[T % 3]


@pytest.fixture(scope="module")
def layers(tmp_path_factory):
    """Every (T, CUs, cy_fast) of the sweep: what the host program printed.  The batches are asked once per (T, CUs): neither the
    counts of the run table nor anything derived from them depends on the tile order (asserted in the partition test)."""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("conv_sched") / "conv_sched_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "body-and-organ-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tools", "conv_sched_host.cpp"), "-o", str(exe)])
    asked = []
    for cu in CUS:
        for T in TILES:
            ncy, t, ext = _geometry(T)
            for cy_fast in (0, 1):
                asked.append(dict(T=T, cu=cu, cy_fast=cy_fast, ncy=ncy, t=t, ext=ext, nmax=0 if cy_fast else BATCHES))
    lines = ["layer {T} {cu} {cy_fast} {t[0]} {t[1]} {t[2]} {ncy} {ext[0]} {ext[1]} {ext[2]} {nmax}".format(**a) for a in asked]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    flat = np.fromstring(r.stdout, dtype=np.int64, sep=" ")
    at = 0
    for a in asked:
        a["vw"], a["nslots"] = int(flat[at]), int(flat[at + 1])
        assert 1 <= a["vw"] <= a["cu"]
        a["tab"] = flat[at + 2:at + 2 + 8 * a["vw"]].reshape(a["vw"], 8)
        at += 2 + 8 * a["vw"]
        a["batches"] = []
        for N in range(1, a["nmax"] + 1):
            grid, row = int(flat[at]), int(flat[at + 1])
            assert 1 <= grid <= a["cu"]
            a["batches"].append((N, grid, row, flat[at + 2:at + 2 + grid]))
            at += 2 + grid
    assert at == len(flat)
    return asked


def _first_index(a):
    """The first tile index of every run, from the (cy, sp) the table stores: decode_tile's order, inverted."""
    cy, sp, nsp = a["tab"][:, 1], a["tab"][:, 2], int(np.prod(a["t"]))
    assert ((0 <= cy) & (cy < a["ncy"]) & (0 <= sp) & (sp < nsp)).all()
    return sp * a["ncy"] + cy if a["cy_fast"] else cy * nsp + sp


def test_sizes(layers):
    for a in layers:
        assert a["vw"] == min(a["T"], a["cu"]) and a["nslots"] == 4 * a["vw"]
        for N, grid, row, _ in a["batches"]:
            assert grid == min(N * a["vw"], a["cu"])
            assert row == -(-N * a["vw"] // grid) * (a["T"] // a["vw"] + 2) + 1


def test_runs_partition_a_sample_in_xcd_order(layers):
    """Virtual workgroup j belongs to XCD j % 8: the tile list is cut into 8 contiguous ranges, one per XCD, and the virtual workgroups
    of an XCD take contiguous runs of its range in the order of j (a vw that is no multiple of 8: contiguous runs in the order of j).
    Ranges and the runs of one range differ by at most one tile -- what the descriptor row length counts on."""
    xcd_layers = 0
    by_order = {}
    for a in layers:
        T, vw, count, first = a["T"], a["vw"], a["tab"][:, 0], _first_index(a)
        j = np.arange(vw)
        order = np.lexsort((j >> 3, j & 7)) if vw % 8 == 0 else j
        assert (count >= 1).all(), (T, a["cu"])
        assert first[order[0]] == 0 and (first[order][1:] == (first + count)[order][:-1]).all(), (T, a["cu"], a["cy_fast"])
        assert first[order[-1]] + count[order[-1]] == T
        if vw % 8 == 0:
            xcd_layers += 1
            per_xcd = np.array([count[j & 7 == x].sum() for x in range(8)])
            assert per_xcd.max() - per_xcd.min() <= 1 and all(np.ptp(count[j & 7 == x]) <= 1 for x in range(8))
        else:
            assert np.ptp(count) <= 1
        assert count.max() <= T // vw + 2
        assert not a["tab"][:, 6:].any()
        other = by_order.setdefault((T, a["cu"]), count)
        assert np.array_equal(other, count), "the cut depends on the tile order"
    assert xcd_layers > 100 and xcd_layers < len(layers) - 100


def test_first_tile_coordinates(layers):
    """ox0, oy0, oz0 of a run = the decode of its first tile index: x fastest, then z, then y (decode_tile)."""
    for a in layers:
        first, (t0, t1, t2), nsp = _first_index(a), a["t"], int(np.prod(a["t"]))
        sp = first // a["ncy"] % nsp if a["cy_fast"] else first % nsp
        cy = first % a["ncy"] if a["cy_fast"] else first // nsp
        tx, tz, ty = sp % t0, sp // t0 % t2, sp // t0 // t2
        assert (ty < t1).all()
        want = np.stack([cy, sp, tx * a["ext"][0], ty * a["ext"][1], tz * a["ext"][2]], 1)
        assert np.array_equal(a["tab"][:, 1:6], want), (a["T"], a["cu"], a["cy_fast"])


def test_descriptor_rows_hold_every_workgroup(layers):
    """Physical workgroup b walks the runs of the virtual workgroups b, b + grid, ... of the N vw of a launch; a descriptor row has
    one entry in front of a workgroup's tiles."""
    workgroups, fullest = 0, 0.0
    for a in layers:
        count, vw = a["tab"][:, 0], a["vw"]
        for N, grid, row, tiles in a["batches"]:
            v = np.arange(N * vw)
            want = np.bincount(v % grid, weights=count[v % vw], minlength=grid).astype(np.int64)
            assert np.array_equal(tiles, want), (a["T"], a["cu"], N)
            assert tiles.sum() == N * a["T"] and tiles.min() >= 1
            assert tiles.max() <= row - 1, (a["T"], a["cu"], N, int(tiles.max()), row)
            workgroups += grid
            fullest = max(fullest, tiles.max() / (row - 1))
    print(f"\n{workgroups} workgroups, fullest row {100 * fullest:.1f} %")
    assert workgroups > 5_000_000
