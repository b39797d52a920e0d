"""CPU: tools/golden.py -- a fixture over the 1 MiB limit for a committed file
is stored as <name>.part0, .part1, ...; split() writes the parts and load()
reads the fixture whole or in parts."""
import os

import numpy as np
import pytest

from tools import golden


def write(folder, name, n, seed):
    a = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    np.savez(os.path.join(folder, name), data=a, tag=np.array([seed]))
    return a


def test_small_fixture_stays_whole(tmp_path):
    d = str(tmp_path)
    a = write(d, "s.npz", 1000, 1)
    assert golden.split("s.npz", d) == [os.path.join(d, "s.npz")] and os.listdir(d) == ["s.npz"]
    assert np.array_equal(golden.load("s.npz", d)["data"], a)


def test_split_and_load_round_trip(tmp_path):
    d = str(tmp_path)
    a = write(d, "big.npz", 2 * golden.PART_BYTES + 12345, 2)
    whole = open(os.path.join(d, "big.npz"), "rb").read()
    written = golden.split("big.npz", d)
    assert [os.path.basename(p) for p in written] == ["big.npz.part0", "big.npz.part1", "big.npz.part2"]
    assert sorted(os.listdir(d)) == sorted(os.path.basename(p) for p in written)  # the whole file is gone
    assert all(os.path.getsize(p) <= golden.PART_BYTES for p in written) and golden.PART_BYTES <= 1 << 20
    assert b"".join(open(p, "rb").read() for p in written) == whole
    z = golden.load("big.npz", d)
    assert sorted(z.files) == ["data", "tag"] and np.array_equal(z["data"], a) and z["tag"][0] == 2


def test_parts_are_read_in_numeric_order_and_stale_parts_removed(tmp_path, monkeypatch):
    d = str(tmp_path)
    monkeypatch.setattr(golden, "PART_BYTES", 1000)
    a = write(d, "m.npz", 11500, 3)  # 13 parts: part10 sorts after part9, not after part1
    assert len(golden.split("m.npz", d)) == 13
    assert np.array_equal(golden.load("m.npz", d)["data"], a)
    b = write(d, "m.npz", 2500, 4)  # regenerated smaller, next to the old parts
    assert len(golden.split("m.npz", d)) == 4 and len(os.listdir(d)) == 4
    assert np.array_equal(golden.load("m.npz", d)["data"], b)


def test_missing_fixture_raises(tmp_path):
    with pytest.raises(FileNotFoundError):
        golden.load("absent.npz", str(tmp_path))


@pytest.mark.parametrize("name", ["c3_4096_q75.npz", "q75_1080p.npz", "test_color_png.npz"])
def test_committed_fixtures_are_within_the_limit(name):
    ps = golden.parts(name)
    assert ps and not os.path.exists(os.path.join(golden.GOLDEN, name))
    assert all(os.path.getsize(p) <= 1 << 20 for p in ps) and golden.load(name).files
