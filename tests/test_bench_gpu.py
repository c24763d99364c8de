"""bench.py on the device, in fresh processes as the driver runs it: a plain run prints the headline line, writes
--dump-outputs and runs nothing that takes steps of its own; --full adds the dominant kernel timed alone and the
configs[1] / configs[2] side measurements to the same line."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_line(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_to_it(tmp_path):
    plain = bench_line("--gpus", "1", "--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path / "d"))
    assert (plain["metric"], plain["unit"], plain["higher_is_better"], plain["dtype"]) == \
        ("train-step images/sec", "images/s", True, "f32")
    assert (plain["steps"], plain["warmup"], plain["n_gpus"]) == (4, 2, 1)
    assert plain["ms_per_step"] > 0 and plain["value"] == pytest.approx(32e3 / plain["ms_per_step"], rel=1e-9)
    assert math.isfinite(plain["final_loss"])
    # nothing that takes runs of its own: no CPU leg, no side configurations, and no pipelined roofline (the kernel
    # alone on the chip needs one-stream steps after the timed region)
    assert not set(plain) & {"cpu_baseline", "secondary", "secondary2"}
    assert plain["roofline"] is None
    assert sorted(os.listdir(str(tmp_path / "d"))) == ["generated.npy", "losses.npy", "trained_weights.npy"]
    losses = np.load(str(tmp_path / "d" / "losses.npy"))
    assert losses[4] == pytest.approx(plain["final_loss"], rel=1e-6)

    full = bench_line("--gpus", "1", "--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline")
    assert set(plain) <= set(full) and "cpu_baseline" not in full
    # the same steps on the same inputs before anything --full adds
    assert full["final_loss"] == pytest.approx(plain["final_loss"], rel=1e-5)
    roof = full["roofline"]
    assert roof["achieved"] > 0 and roof["timed_region_event_ms"] > 0 and roof["launches_per_step"] > 0
    for key in ("secondary", "secondary2"):
        assert "error" not in full[key] and full[key]["value"] > 0, full[key]
