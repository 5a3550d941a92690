"""bench.py's plain run and --dump-outputs: a plain run times the steps and reports the headline only (the other legs are --full's), and the
last timed step's frame and counters are written as float arrays that two runs with the same arguments agree on."""
import os

import numpy as np
import pytest

from helpers import run_bench

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    runs = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        c, d, _ = run_bench(["--config", "tiny", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)], timeout=600)
        runs.append((c, d, out))
    c, d, out = runs[0]
    assert c["steps"] == 3 and c["warmup"] == 1 and c["ms_per_step"] > 0 and c["value"] > 0 and c["unit"] == "Msamples/s"
    assert not {"cpu_baseline", "extra", "with_empty_space_skipping", "without_phase_events"} & set(d) and "views" not in d["roofline"]
    assert sorted(os.listdir(out)) == ["counters.npy", "grad.npy", "rgba.npy"] and d["dumped_outputs"]["arrays"] == ["counters", "grad", "rgba"]
    rgba, grad, counters = (np.load(out / f"{k}.npy") for k in ("rgba", "grad", "counters"))
    assert rgba.dtype == np.float32 and rgba.shape == (256, 256, 4) and grad.dtype == np.float32 and grad.shape == (256, 256, 3)
    assert np.isfinite(rgba).all() and (rgba[..., 3] > 0).mean() > 0.05
    # counters: samples, shaded_samples, shadow_samples, rays, active_pixels, ... of the last step - a static camera renders the same work every step
    assert counters.dtype == np.float64 and counters[0] == d["per_frame"]["samples"] and counters[3] == 256 * 256
    # the same arguments give the same inputs: the frames agree up to the accumulation's division by a frame count the tuner's warm-up may change
    _, _, out2 = runs[1]
    assert np.array_equal(np.load(out2 / "counters.npy"), counters)
    np.testing.assert_allclose(np.load(out2 / "rgba.npy"), rgba, rtol=0, atol=1e-5)
    np.testing.assert_allclose(np.load(out2 / "grad.npy"), grad, rtol=0, atol=1e-5)
