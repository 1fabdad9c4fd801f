"""Writes tests/golden/g17_basic_statistics.npz / .json: the reference's OWN get_basic_statistics (TS/statistics.py:91-141), executed
through the stub-import harness of make_golden.py on the calls of tests/basic_statistics_cases.py.  The .npz holds the inputs (label
volume, CT, float32 zooms per volume), the .json the returned dicts per call, key order kept; floats are written with repr, so they
read back bit for bit.

    python tests/golden/make_golden_statistics.py        (dev container only: needs the reference checkout)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_harness  # noqa: E402

_ref_harness.install()
from totalsegmentator import statistics as ts_stats  # noqa: E402
from totalsegmentator.map_to_binary import class_map  # noqa: E402

import basic_statistics_cases as cases  # noqa: E402


class _Header:
    def __init__(self, zooms):
        self._zooms = tuple(np.float32(z) for z in zooms)

    def get_zooms(self):
        return self._zooms


class _Image:
    """what get_basic_statistics needs of a nibabel image: get_fdata() (float64) and header.get_zooms() (float32)"""

    def __init__(self, data, zooms):
        self._data, self.header = data, _Header(zooms)

    def get_fdata(self):
        return np.asarray(self._data, dtype=np.float64)


def main():
    arrays, dicts = {}, {}
    for name in cases.VOLUMES:
        seg, ct, zooms = cases.volume(name)
        arrays[f"{name}.seg"], arrays[f"{name}.ct"], arrays[f"{name}.zooms"] = seg, ct, zooms
    with np.errstate(all="raise"):       # (an overflow of the reference's int16 normalisation would make the case meaningless)
        for k, (name, kw) in enumerate(cases.CALLS):
            seg, ct, zooms = cases.volume(name)
            res = ts_stats.get_basic_statistics(seg, _Image(ct, zooms), None, quiet=True, task=cases.TASK, **kw)
            dicts[cases.call_key(k)] = {"kwargs": kw, "stats": [[n, float(v["volume"]), float(v["intensity"])] for n, v in res.items()]}
    np.savez_compressed(os.path.join(HERE, "g17_basic_statistics.npz"), **arrays)
    with open(os.path.join(HERE, "g17_basic_statistics.json"), "w") as f:
        json.dump({"class_map": [[int(k), v] for k, v in class_map[cases.TASK].items()], "calls": dicts}, f, indent=0)
    for ext in ("npz", "json"):
        p = os.path.join(HERE, f"g17_basic_statistics.{ext}")
        print(p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
