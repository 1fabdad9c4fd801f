"""csrc/tile_grid.h on the host: the tile grid test, the gather head's walk table, the stash layout and the deferral plan of a
tile-sharded call, compiled into tools/tile_grid_host.cpp with the address and undefined-behaviour sanitizers, run as a child process
and compared with numpy models of what net_stash.hip and k_gather_head expect of them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from boa_hip import sliding_window as sw
from boa_hip import tile_shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (image, patch, step): step 0.5; step 0.8 with a z extent that is no multiple of 32; a step below half a patch; one step on axis 0
GRIDS = [((70, 50, 96), (32, 32, 32), 0.5), ((44, 40, 52), (32, 32, 32), 0.8), ((40, 36, 70), (32, 32, 32), 0.3),
         ((32, 50, 70), (32, 32, 32), 0.5)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("tile_grid") / "tile_grid_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "body-and-organ-analysis_amd", "csrc"),
                           os.path.join(ROOT, "tools", "tile_grid_host.cpp"), "-o", str(exe)])

    def ask(*requests):
        r = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        return [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    return ask


def _ints(v):
    return " ".join(str(int(x)) for x in np.asarray(v).reshape(-1))


def _grid(host, origins):
    head, s0, s1, s2 = host("origins " + _ints(origins), "grid")
    return bool(head[0]), head[1:], [s0, s1, s2]


@pytest.mark.parametrize("image,patch,step", GRIDS)
def test_grid_origins_accepts_the_sliding_window_grid(host, image, patch, step):
    want = sw.compute_steps_for_sliding_window(list(image), list(patch), step)
    ok, n, steps = _grid(host, sw.get_sliding_window_origins(list(image), list(patch), step))
    assert ok and n == [len(s) for s in want] and steps == [list(s) for s in want]
    if image[0] == patch[0]:
        assert n[0] == 1


def test_grid_origins_rejects_what_is_no_canonical_grid(host):
    o = sw.get_sliding_window_origins([70, 50, 96], [32, 32, 32], 0.5)
    assert len(o) == 4 * 3 * 5 and _grid(host, o)[0]
    swapped = o.copy()
    swapped[[7, 8]] = swapped[[8, 7]]
    bad = {"swapped": swapped, "dropped": np.delete(o, 11, axis=0), "duplicated": np.insert(o, 4, o[4], axis=0)}
    for axis in range(3):   # a full cartesian grid whose steps along one axis do not ascend
        s = [[0, 19, 38], [0, 18], [0, 16, 32, 48, 64]]
        s[axis][0], s[axis][1] = s[axis][1], s[axis][0]
        bad[f"axis {axis} descends"] = np.array([(x, y, z) for x in s[0] for y in s[1] for z in s[2]])
    for name, origins in bad.items():
        assert not _grid(host, origins)[0], name
    line = lambda n, axis: np.eye(3, dtype=np.int64)[axis][None, :] * np.arange(n)[:, None]   # noqa: E731
    for axis in range(3):   # the walk table's cover words hold 8-bit tile indices
        assert _grid(host, line(255, axis))[0] and not _grid(host, line(256, axis))[0]
    assert not _grid(host, np.zeros((0, 3)))[0]


def _check_walk(host, steps, ext, PV):
    """Every x, every y and every 32-voxel z run: the tiles whose extent covers it (brute force over all tiles of the axis) are
    exactly the index range [first, first + count) of the table's cover word; the table's length is walk_table_ints."""
    (ints, length), tab = host(*[f"steps {a} " + _ints(steps[a]) for a in range(3)], "walk " + _ints(ext) + " " + _ints(PV))
    n = [len(s) for s in steps]
    assert ints == length == len(tab) == sum(n) + PV[0] + PV[1] + -(-PV[2] // 32)
    assert tab[:sum(n)] == [int(v) for s in steps for v in s]
    words = tab[sum(n):]
    spans = [(x, x) for x in range(PV[0])], [(y, y) for y in range(PV[1])], [(z, min(z + 31, PV[2] - 1)) for z in range(0, PV[2], 32)]
    assert len(words) == sum(len(s) for s in spans)
    k = 0
    for a in range(3):
        for lo, hi in spans[a]:
            cover = [i for i, s in enumerate(steps[a]) if s <= hi and s + ext[a] > lo]
            first, count = words[k] & 255, words[k] >> 8
            assert count == len(cover) and (count == 0 or cover == list(range(first, first + count))), (a, lo, hi)
            k += 1
    return words


@pytest.mark.parametrize("image,patch,step", GRIDS)
def test_walk_table_covers(host, image, patch, step):
    steps = sw.compute_steps_for_sliding_window(list(image), list(patch), step)
    words = _check_walk(host, steps, patch, image)
    assert all(w >> 8 for w in words)        # the tiles of a fold cover the whole volume
    if image[2] % 32:
        assert image[2] - 32 * (image[2] // 32) < 32 and len(words) == image[0] + image[1] + image[2] // 32 + 1


def _model_plan(org, defer, patch0):
    d = defer > 0
    if not d.any():
        return dict(x0=0, x_split=int(org[:, 0].min()), dp0=0, n_def=0, rows=[])
    ends = set(int(v) for v in (org[:, 0] + defer)[d])
    assert len(ends) == 1
    return dict(x0=int(org[d, 0].min()), x_split=ends.pop(), dp0=int(defer.max()), n_def=int(d.sum()),
                rows=sorted(set(int(v) for v in org[d, 0])))


def _defer(host, org, defer, patch0):
    (consistent, x0, x_split, x_end, dp0, n_def), rows = host("origins " + _ints(org), f"defer {patch0} " + _ints(defer))
    return bool(consistent), dict(x0=x0, x_split=x_split, dp0=dp0, n_def=n_def, rows=rows), x_end


# (image, patch, step, world): three active ranks at step 0.5; a step below half a patch, where two rows and more defer
SHARDS = [((120, 20, 40), (32, 16, 32), 0.5, 3), ((120, 20, 40), (32, 16, 32), 0.5, 2), ((88, 20, 70), (32, 16, 32), 0.3, 2),
          ((88, 20, 70), (32, 16, 32), 0.3, 3)]


def test_deferral_plans_of_the_tile_shard_planner(host):
    """Every rank's pattern of tile_shard.plan_rows is consistent, its plan is what numpy derives from the same arrays, and the walk
    table of its deferring rows (dp0 planes per tile) covers like a fold's."""
    most_rows, most_ranks = 0, 0
    for image, patch, step, world in SHARDS:
        origins = sw.get_sliding_window_origins(list(image), list(patch), step)
        plan = tile_shard.plan_rows(origins, patch[0], image[0], world)
        most_ranks = max(most_ranks, plan.active)
        for rank in range(plan.active):
            org, defer = origins[plan.tiles(rank)], plan.defer_planes(rank)
            assert (defer > 0).any() == (rank > 0)
            consistent, got, x_end = _defer(host, org, defer, patch[0])
            want = _model_plan(org, defer, patch[0])
            assert consistent and got == want and x_end == int(org[:, 0].max()) + patch[0], (image, step, world, rank)
            most_rows = max(most_rows, len(want["rows"]))
            ok, n, steps = _grid(host, org)
            assert ok and want["n_def"] == len(want["rows"]) * n[1] * n[2]
            if want["n_def"]:
                words = _check_walk(host, [want["rows"], steps[1], steps[2]], (want["dp0"], patch[1], patch[2]), image)
                # every row keeps dp0 planes: the planes [x0, x_split) that boa_net_apply_deferred visits, and valid planes behind them
                covered = [x for x in range(image[0]) if words[x] >> 8]
                assert covered == sorted(set(x for r in want["rows"] for x in range(r, r + want["dp0"])))
                assert covered[0] == want["x0"] and set(range(want["x0"], want["x_split"])) <= set(covered)
    assert most_rows >= 2 and most_ranks == 3


def test_deferral_plans_that_are_not_consistent(host):
    """One tile's count changed by one -- in the first row, in the last deferring row, in a row that defers nothing -- and a
    pattern in which a middle row alone defers."""
    untouched = 0
    for image, patch, step, world in (SHARDS[1], SHARDS[2]):
        origins = sw.get_sliding_window_origins(list(image), list(patch), step)
        plan = tile_shard.plan_rows(origins, patch[0], image[0], world)
        org, defer = origins[plan.tiles(1)], plan.defer_planes(1)
        assert _defer(host, org, defer, patch[0])[0]
        tiles = [0, int(np.nonzero(defer > 0)[0][-1])] + [int(t) for t in np.nonzero(defer == 0)[0][:1]]
        untouched += len(tiles) == 3
        for tile in tiles:
            for delta in (-1, 1):
                d = defer.copy()
                d[tile] += delta
                if 0 <= d[tile] <= patch[0]:
                    assert not _defer(host, org, d, patch[0])[0], (image, tile, delta)
        rows = sorted(set(int(v) for v in org[:, 0]))
        middle = np.where(org[:, 0] == rows[1], 5, 0)     # the first row reaches below the middle row's split plane and defers nothing
        assert len(rows) >= 3 and not _defer(host, org, middle, patch[0])[0]
        assert _defer(host, org, np.zeros(len(org), int), patch[0])[0]
    assert untouched >= 1


def test_stash_offsets_are_aligned_and_disjoint(host):
    for act, n, F, ss16, ints in [(0, 0, 32, 0, 37), (3 * 65536 + 2, 3, 32, 1, 1), (12345, 7, 32, 0, 64), (4096, 125, 32, 1, 1600)]:
        (ss, s16, ssp, tab, total), = host(f"offsets {act} {n} {F} {ss16} {ints}")
        assert all(v % 256 == 0 for v in (ss, s16, ssp, tab, total))
        assert ss >= act and s16 >= ss + n * F * 8 and ssp >= s16 + (n * F * 4 if ss16 else 0) and tab >= ssp + n * 128 and total >= tab + 4 * ints
        assert total - (tab + 4 * ints) < 256
