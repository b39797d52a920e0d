"""`python bench.py --gpus 1 --steps K --warmup W`: a plain run times K steps
and prints the headline record alone; what else the benchmark measures comes
with --full; --dump-outputs writes the same files for the same arguments.

The GPU test runs the command line itself (that is what it is about), once
plain and once with --full, at a batch of 3 frames -- one of each content --
and with the smallest counts for --full's repeats, so that it stays short."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
# what a --full run on one GPU always adds to the record
FULL_1GPU = {"runs", "stage_ms_isolated", "roofline", "stage_roofline", "c2_single_frame", "c3", "c5", "cpu_baseline"}
FULL_ONLY = FULL_1GPU | {"gather", "valu"}  # N > 1 only; only where the dominant kernel has a committed SQ pass


def test_plain_record_has_the_headline_and_nothing_measured_apart():
    args = argparse.Namespace(batch=64, steps=5, warmup=2, slots=3, split=True, full=False)
    rec = bench.base_record(args, 1, 1, 0.1, {"encode": 1.0})
    assert PLAIN_KEYS <= set(rec) and not FULL_ONLY & set(rec)
    assert rec["ms_per_step"] == 20.0 and rec["steps"] == 5 and rec["unit"] == "MPixels/s"
    assert rec["value"] == round(64 * bench.W * bench.H * 5 / 0.1 / 1e6, 1) and rec["full"] is False


def test_dump_positions_are_distinct_spread_and_fixed():
    for n, m in ((bench.DUMP_RECORDS + 1, bench.DUMP_RECORDS), (64 * 8160, bench.DUMP_RECORDS),
                 (64 * 1080 * 1920 * 4, bench.DUMP_ELEMENTS)):
        p = bench.dump_positions("nrgba", n, m)
        assert p.shape == (m,) and p[0] >= 0 and p[-1] < n and (np.diff(p) > 0).all()
        edges = np.arange(m + 1) * n // m  # one position in each of m strata
        assert (p >= edges[:-1]).all() and (p < edges[1:]).all()
        assert np.array_equal(p, bench.dump_positions("nrgba", n, m))
        assert not np.array_equal(p, bench.dump_positions("dec_y", n, m))


def run_bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--batch", "3", *extra], cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_and_full_runs_and_their_dumps(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    rec = run_bench("--dump-outputs", a)
    assert PLAIN_KEYS <= set(rec) and not FULL_ONLY & set(rec)
    assert rec["steps"] == 4 and rec["warmup"] == 1 and rec["full"] is False and rec["ms_per_step"] > 0
    # value and ms_per_step are rounded to 0.1 and 0.001 in the record
    assert abs(rec["value"] - 3 * bench.W * bench.H / rec["ms_per_step"] / 1e3) <= \
        rec["value"] * 0.0005 / (rec["ms_per_step"] - 0.0005) + 0.06
    # --full: the same headline fields, and everything that moved behind it is measured and reported
    full = run_bench("--full", "--runs", "2", "--run-steps", "2", "--iso-steps", "1", "--cpu-seconds", "0.3",
                     "--dump-outputs", b)
    assert PLAIN_KEYS <= set(full) and FULL_1GPU <= set(full) and full["full"] is True
    assert all(full[k] == rec[k] for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"))
    assert full["runs"]["runs"] == 2 and set(full["runs"]) >= {"encode+decode", "encode", "decode"}
    assert set(full["stage_ms_isolated"]) == set(full["stage_ms_overlapped"]) == set(bench.BYTES_PER_PX)
    assert full["roofline"]["measured_copy_peak"]["GB/s"] > 0 and full["roofline"]["critical_path"]["mb_steps"] > 0
    assert set(full["c2_single_frame"]) == set(bench.CONTENTS) and full["c3"]["MPix/s"] > 0
    assert set(full["c5"]["stages"]) == set(bench.C5_BYTES_PER_PX) and full["cpu_baseline"]["value"] > 0
    # the same arguments to the timed path: the same outputs, from another process and with --full
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "nrgba.npy" in names and "enc_coeffs.npy" in names
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 * 1000 * 1000
    for n in names:
        x = np.load(os.path.join(a, n))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, np.load(os.path.join(b, n))), n
