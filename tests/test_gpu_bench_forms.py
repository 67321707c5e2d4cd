"""`bench.py` on the GPU, plain and with `--full`: a plain run prints the headline and its roofline block and measures nothing
else; `--full` adds the step-time distribution, the CPU baselines and their parity check against the C oracle.  (At 2^20 samples,
with the informational legs and the live PMC passes left out, so that the test stays short.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("step_time_distribution", "cpu_baseline", "cpu_baseline_all_cores", "cpu_baseline_numpy", "cpu_baseline_numba", "parity",
             "config3_batch", "short_signal_batches", "mid_size_signals", "many_mid_size_signals", "f_rows", "config5_audio",
             "headline_on_quantised_2p24", "headline_with_valid_flags")


def _line(extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--warm-ms", "0",
                        "--log2n", "20"] + extra, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_a_plain_run_measures_the_headline_alone():
    d = _line([])
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 3 and d["warmup"] == 1
    assert d["config"]["rows"] == 9 and d["roofline"]["avg_launch_us"] > 0
    assert d["roofline"].get("traffic_live_attempt") is None          # (no PMC passes were started)
    assert [k for k in FULL_ONLY if k in d] == []


def test_full_adds_the_step_distribution_and_the_cpu_legs():
    d = _line(["--full", "--no-extra", "--no-live-traffic"])
    assert d["value"] > 0 and d["config"]["rows"] == 9
    assert d["step_time_distribution"]["steps"] >= 8
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline_all_cores"]["value"] > 0 and d["cpu_baseline_numpy"]["value"] > 0
    assert d["parity"] == {"knot_counts_equal": True, "rows_bit_exact": True}
