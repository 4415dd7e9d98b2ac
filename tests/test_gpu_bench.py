"""bench.py's plain run on the device: `--steps` is the number of timed steps, the
headline line carries the fields later runs are compared on, nothing of the --full
measurements runs, and --dump-outputs writes the parameters and the losses of the last
timed steps run once more from the seeded model."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(tmp_path, out, *args):
    env = dict(os.environ, NCF_BENCH_WARM_S="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args, "--dump-outputs", str(out)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_exactly_steps_and_dumps_outputs(tmp_path):
    out = tmp_path / "out"
    d = _bench(tmp_path, out, "--steps", "90", "--warmup", "3")
    assert d["steps"] == 90 and d["unit"] == "interactions/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0 and d["metric"].startswith("training interactions/sec")
    # 90 steps from the start of a 76-step epoch: 76 * 65,536-row batches short of the
    # epoch's last one, then 14 full ones
    rows = d["config"]["rows_per_epoch"] + 14 * 65536
    assert d["value"] == pytest.approx(rows / (d["ms_per_step"] * 1e-3 * 90), rel=1e-9)
    for key in ("kernel_ms", "roofline", "e2e", "cpu_baseline", "sustained", "frozen_epoch", "quality"):
        assert key not in d, key
    files = sorted(os.listdir(out))
    assert "loss.npy" in files and "embed_user_MLP.weight.npy" in files and "predict_layer.weight.npy" in files
    total = 0
    for f in files:
        a = np.load(out / f)
        total += a.nbytes
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
    assert total <= 64 * 2 ** 20
    assert np.load(out / "embed_user_MLP.weight.npy").shape == (6041, 64)
    # the dumped steps start from the seeded model (BCE near ln 2) and train it: 64 Adam
    # steps at lr 1e-3 take this model's loss below 0.55 (0.42 after one 76-step epoch)
    loss = np.load(out / "loss.npy")
    assert loss.shape == (64,) and 0.65 < float(loss[0]) < 0.75 and float(loss[-1]) < 0.55
    # no step jumps up: from batch to batch the loss moves by up to 0.008 once it has settled
    assert (np.diff(loss) < 0.02).all()


def test_dumped_outputs_agree_between_runs(tmp_path):
    """Two runs with the same arguments dump the same arrays.  The dumped parameters are
    two Adam steps of at most lr = 1e-3 per element from the same seeded state, on the
    same batches; only the order of the fp32 atomic sums varies.  Bound: a thousandth of
    one such step, 1e-6 absolute, for the losses too (measured: 1e-7 at most, the
    losses of 64 steps within two ulp)."""
    a, b = tmp_path / "a", tmp_path / "b"
    for out in (a, b):
        _bench(tmp_path, out, "--steps", "30", "--warmup", "3")
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in sorted(os.listdir(a)):
        x, y = np.load(a / f), np.load(b / f)
        print(f, float(np.abs(x.astype(np.float64) - y).max()))
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-6, err_msg=f)
