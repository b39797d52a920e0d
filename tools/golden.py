"""Fixtures under tests/golden/ that are larger than the repository's 1 MiB
limit for a committed file are stored in parts: <name>.part0, <name>.part1,
... of at most PART_BYTES each, the bytes of the one file in order.  load()
reads a fixture either way; split() turns a freshly written file into parts
(tests/golden/make_golden.py)."""
import glob
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
PART_BYTES = 1000000


def parts(name, folder=GOLDEN):
    found = glob.glob(os.path.join(glob.escape(folder), name + ".part*"))
    return sorted(found, key=lambda p: int(p.rsplit(".part", 1)[1]))


def load(name, folder=GOLDEN):
    """np.load of tests/golden/<name> (an .npz), whole or in parts."""
    path = os.path.join(folder, name)
    if os.path.exists(path):
        return np.load(path)
    ps = parts(name, folder)
    if not ps:
        raise FileNotFoundError(path)
    return np.load(io.BytesIO(b"".join(open(p, "rb").read() for p in ps)))


def split(name, folder=GOLDEN):
    """Replace tests/golden/<name> by its parts if it is over the limit (parts
    of an earlier, larger version are removed either way); returns the files
    that now hold it."""
    path = os.path.join(folder, name)
    for p in parts(name, folder):
        os.remove(p)
    data = open(path, "rb").read()
    if len(data) <= PART_BYTES:
        return [path]
    out = []
    for k in range(0, len(data), PART_BYTES):
        out.append(f"{path}.part{k // PART_BYTES}")
        with open(out[-1], "wb") as f:
            f.write(data[k:k + PART_BYTES])
    os.remove(path)
    return out
