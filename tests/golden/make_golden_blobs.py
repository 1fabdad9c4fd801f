"""Writes tests/golden/g16_blobs.npz: the reference's OWN keep_largest_blob_multilabel, remove_small_blobs_multilabel, keep_largest_blob
and remove_small_blobs (TS/postprocessing.py:13-98), executed through the stub-import harness of make_golden.py on the small label
volumes of tests/blob_cases.py.  Inputs and outputs are stored (uint8; the 0 / 1 arrays of the two binary functions too).

    python tests/golden/make_golden_blobs.py        (dev container only: needs the reference checkout)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_harness  # noqa: E402

_ref_harness.install()
from totalsegmentator import postprocessing as pp  # noqa: E402

import blob_cases  # noqa: E402


def main():
    out = {}
    for name, (arr, calls) in blob_cases.golden_cases().items():
        out[f"{name}.input"] = arr
        for k, (fn, kw) in enumerate(calls):
            if fn in ("keep_largest_blob_multilabel", "remove_small_blobs_multilabel"):
                res = getattr(pp, fn)(arr.copy(), blob_cases.CLASS_MAP, quiet=True, **kw)
            else:
                res = getattr(pp, fn)(arr != 0, **kw)
            res = np.asarray(res)
            assert res.shape == arr.shape and res.min() >= 0 and res.max() <= 255
            out[blob_cases.call_key(name, k, fn)] = res.astype(np.uint8)
    path = os.path.join(HERE, "g16_blobs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
