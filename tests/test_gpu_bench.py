"""GPU: bench.py's two kinds of run on a small cloud -- a plain one prints the headline and nothing that needs runs of
its own; --full adds roofline, config.secondary and cpu_baseline (strong_100M belongs to the 10M bench only)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
ARGS = ["--points", "200000", "--steps", "5", "--warmup", "2", "--repeats", "3"]


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_and_full():
    plain = _bench()
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["unit"] == "iterations/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["value"] > 0 and plain["steps"] == 5 and plain["repeats"] == 3
    assert "roofline" not in plain and "cpu_baseline" not in plain and "secondary" not in plain["config"]

    full = _bench("--full")
    assert full["metric"] == plain["metric"] and full["steps"] == 5
    assert full["roofline"]["kernel_ms_avg"] > 0
    assert "cold_30_iteration_call_ms" in full["config"]["secondary"]
    assert "strong_100M" not in full["config"]["secondary"]
    parity = full["cpu_baseline"]["parity_sample"]
    assert parity["hit_pattern_equal"] and parity["d2_bitexact"]
