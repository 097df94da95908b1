"""bench.py's plain run and ``--dump-outputs`` on one GPU, at a small size (2 x 1 x 64^3).

A plain run carries the headline fields and none of the ``--full`` legs (``roofline``,
``cpu_baseline``); ``--steps`` sets the number of timed steps and ``ms_per_step`` is the time of
one of them; ``--dump-outputs DIR`` leaves ``DIR/<name>.npy`` in float32 / float64, under
64 MB in all, holding the last step's loss, logits and labels and the seeded sample of the
updated parameters and their gradients."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, BATCH = 3, 2


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench_outputs")
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
           "--batch", str(BATCH), "--size", "64", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), out


def test_plain_run_result_line(plain_run):
    res, _ = plain_run
    assert res["steps"] == STEPS and res["unit"] == "volumes/sec"
    assert res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["metric"].startswith("volumes/sec fwd+bwd")
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region
    assert res["value"] == pytest.approx(BATCH / (res["ms_per_step"] * 1e-3), rel=1e-9)
    assert "roofline" not in res and "cpu_baseline" not in res


def test_dump_outputs(plain_run):
    _, out = plain_run
    names = sorted(os.listdir(out))
    assert names == ["grads_sample.npy", "labels.npy", "loss.npy", "outputs.npy",
                     "params_sample.npy", "sample_index.npy"]
    arrays = {n[:-4]: np.load(os.path.join(out, n)) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    assert arrays["outputs"].shape == (BATCH, 2) and arrays["labels"].size == BATCH
    assert arrays["loss"].size == 1 and np.isfinite(arrays["loss"]).all()
    assert np.isfinite(arrays["outputs"]).all()
    idx = arrays["sample_index"]
    assert idx.shape == arrays["params_sample"].shape == arrays["grads_sample"].shape
    assert len(idx) > 0 and (np.diff(idx) > 0).all() and (idx == np.round(idx)).all()
    assert np.isfinite(arrays["params_sample"]).all() and np.abs(arrays["params_sample"]).max() > 0
    # (the gradients may all be zero: the reference's head ends in a ReLU on the logits, and
    # once both logits of every sample are clamped the step has no gradient left)
    assert np.isfinite(arrays["grads_sample"]).all()
