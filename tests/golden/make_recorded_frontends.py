"""Records the bits of the spectral front ends as THIS checkout's build computes them on the MI355X: one
tests/golden/frontends/<case>.npz per case of tests/test_frontend_bits_gpu.py (the cases and their seeded inputs are defined there,
once), each holding the outputs as uint32, the first 8 samples of every input and the commit that computed them.

Run by hand, on the commit whose bits are to be kept, after building it:
    python tests/golden/make_recorded_frontends.py [commit-hash]
(the hash is read from git when it is not given)."""

import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_frontend_bits_gpu as T  # noqa: E402


def main():
    commit = sys.argv[1] if len(sys.argv) > 1 else subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    os.makedirs(T.FIXTURES, exist_ok=True)
    for name in sorted(T.CASES):
        got = T.CASES[name]()
        arrays = {k: (np.ascontiguousarray(v).view(np.uint32) if v.dtype == np.float32 and k != "heads" else v) for k, v in got.items()}
        path = os.path.join(T.FIXTURES, name + ".npz")
        np.savez_compressed(path, parent_commit=np.array(commit), **arrays)
        print(f"{name}: {os.path.getsize(path)} bytes, " + ", ".join(f"{k} {v.shape}" for k, v in arrays.items()), flush=True)


if __name__ == "__main__":
    main()
