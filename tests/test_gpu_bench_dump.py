"""`bench.py --dump-outputs DIR` on the GPU: what it writes is what the headline's last timed step computed — the rows at the sampled
positions are the oracle's bit for bit, the summary is the oracle's, and the whole dump stays within 64 MB."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dumped_rows_are_the_oracles(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    from oracle import cpu_oracle
    log2n = 20          # larger than what fits in the dump: the rows are sampled
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--warm-ms", "0",
                        "--log2n", str(log2n), "--no-extra", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= bench.DUMP_BYTES
    n = 1 << log2n
    ref = cpu_oracle.itd_lean(bench.sines_noise(n, seed=0), bench.MAX_ITERATION)
    nr = ref["rows"].shape[0]
    assert np.load(tmp_path / "n_rows.npy").tolist() == [nr]
    pos = np.load(tmp_path / "rows_sample_positions.npy")
    assert pos.dtype == np.float64 and 0 < len(pos) < n and pos[0] == 0 and pos[-1] == n - 1 and np.all(np.diff(pos) > 0)
    sample = np.load(tmp_path / "rows_sample.npy")
    assert sample.dtype == np.float64 and sample.shape == (1, bench.MAX_ITERATION + 2, len(pos))
    assert_bits_equal(sample[0, :nr], ref["rows"][:, pos.astype(np.int64)], "dumped rows")
    assert np.isnan(sample[0, nr:]).all()
