"""bench.py --dump-outputs: the arrays the timed path computed in its last step, written after the timed steps.

Two plain runs with the same arguments get the same inputs, so their dumps must agree: the photons (looked up
by stream id, whatever slot DefragParticles left them in) exactly, the fields to the rounding of the tally's
atomic sums.  A plain run measures only its headline: none of the --full legs appear in its line.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--particles-per-gpu", "200000", "--block-nx", "16", "--dump-outputs", str(out_dir), *extra]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_outputs_of_two_plain_runs_agree(gpu_device, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    da = _bench(a)
    _bench(b)
    assert da["steps"] == 2 and da["warmup"] == 1 and da["ms_per_step"] > 0.0
    for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert k in da
    assert "cpu_baseline" not in da and "accuracy" not in da
    assert da["arithmetic"]["other_variant"] is None
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    for want in ("tally.npy", "edelta.npy", "u.npy", "cell_index.npy", "photon_id.npy", "photon_x.npy",
                 "photon_w.npy", "photon_rng_lo.npy", "totals.npy"):
        assert want in names
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and x.size > 0, n
        if n.startswith("photon_") or n == "cell_index.npy":
            assert np.array_equal(x, y, equal_nan=True), n
        else:
            np.testing.assert_allclose(x, y, rtol=1e-12, atol=0.0, err_msg=n)
    # every photon of the deck is alive at census (pure scattering between reflecting / periodic walls): the
    # sample finds each of them
    assert not np.isnan(np.load(a / "photon_x.npy")).any()
