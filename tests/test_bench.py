"""bench.py's own contract: a plain run measures the timed sweeps only, --full adds the converge phase and the CPU baseline,
--dump-outputs writes the state of the last timed sweep (a fixed sample of arrays above the size cap)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_a_step_count_it_cannot_time(argv):
    pr = subprocess.run([sys.executable, BENCH] + argv, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert pr.returncode == 2 and "--steps must be at least 1" in pr.stderr, pr.stderr[-2000:]


def test_dump_rows_keeps_small_arrays_and_a_fixed_sample_of_large_ones():
    from bench import DUMP_BYTES_PER_ARRAY, dump_rows
    small = np.arange(40.0).reshape(10, 4)
    assert dump_rows(small, 1) is small
    Q = 4
    n = DUMP_BYTES_PER_ARRAY // (8 * Q) + 1000
    big = np.repeat(np.arange(n, dtype=np.float64)[:, None], Q, axis=1)  # row i holds i
    a, b, c = dump_rows(big, 1), dump_rows(big, 1), dump_rows(big, 2)
    assert a.nbytes <= DUMP_BYTES_PER_ARRAY and len(a) == DUMP_BYTES_PER_ARRAY // (8 * Q)
    assert np.array_equal(a, b) and not np.array_equal(a, c)  # the seed fixes the rows
    rows = a[:, 0]
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n  # distinct rows of `big`, ascending
    assert np.array_equal(a, big[rows.astype(np.int64)])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """a plain run prints the headline fields only, its --steps are the timed sweeps, and two runs with the same arguments
    dump the same state (one GPU: marginals and messages, float64, under the size cap)"""
    lines, dumps = [], []
    for i in range(2):
        out = tmp_path / ("run%d" % i)
        cmd = [sys.executable, BENCH, "--gpus", "1", "--workload", "small", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
        pr = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert pr.returncode == 0, pr.stderr[-3000:]
        ls = [l for l in pr.stdout.splitlines() if l.startswith("{")]
        assert len(ls) == 1, pr.stdout[-2000:]
        lines.append(json.loads(ls[0]))
        dumps.append({f: np.load(out / f) for f in sorted(os.listdir(out))})
    d = lines[0]
    assert d["metric"] == "BP edge-message updates/sec" and d["unit"] == "edge-msg/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["steps"] == 3 and d["warmup"] == 1
    assert "converge" not in d and "cpu_baseline" not in d  # --full only
    assert abs(d["value"] - d["config"]["E2"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    a, b = dumps
    assert sorted(a) == ["marginals.npy", "messages.npy"] and sum(x.nbytes for x in a.values()) <= 64 << 20
    N, Q = d["config"]["N"], d["config"]["Q"]
    psi = a["marginals.npy"]
    assert psi.dtype == np.float64 and psi.shape == (N, Q) and np.abs(psi.sum(axis=1) - 1.0).max() < 1e-12
    msg = a["messages.npy"]
    assert msg.dtype == np.float64 and msg.shape[1] == Q and np.abs(msg.sum(axis=1) - 1.0).max() < 1e-12
    for f in a:
        assert a[f].shape == b[f].shape and np.abs(a[f] - b[f]).max() < 1e-12, f


@pytest.mark.gpu
def test_two_rank_dump_holds_the_one_rank_marginals(tmp_path):
    """`--gpus 2` from a bare shell (SBMBP_REHEARSAL=1: both ranks on cuda:0) dumps the marginals gathered over the ranks; the
    initial state and the sweeps are partition invariant, so they are the one-GPU run's"""
    env = dict(os.environ, SBMBP_REHEARSAL="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "SBMBP_SHARD_CHUNKS"):
        env.pop(k, None)
    psi = []
    for gpus in ("1", "2"):
        out = tmp_path / ("gpus" + gpus)
        cmd = [sys.executable, BENCH, "--gpus", gpus, "--workload", "small", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
        pr = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert pr.returncode == 0, pr.stderr[-3000:]
        psi.append(np.load(out / "marginals.npy"))
    assert sorted(os.listdir(tmp_path / "gpus2")) == ["marginals.npy"]  # messages: one GPU only
    assert psi[0].shape == psi[1].shape and np.abs(psi[0] - psi[1]).max() < 1e-12
