"""A plain `bench.py` run on the GPU: exactly --steps timed steps, the headline line without the --full extras, and --dump-outputs writing what the last
timed step computed (the loss it returned, samples of its logits and of the updated weights)."""
import json, os, subprocess, sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def test_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bench
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    env["PYTHONNOUSERSITE"] = "1"
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["dtype"] == "bf16" and out["unit"] == "images/sec" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and abs(out["value"] - 32 * 1e3 / out["ms_per_step"]) <= 0.01 * out["value"]
    assert not {"roofline", "kernels", "fp32", "fp32fast", "configs", "inference", "dp1", "cpu_baseline"} & set(out)       # --full only
    assert sorted(os.listdir(d)) == ["logits.npy", "loss.npy", "weights.npy"]
    loss = np.load(d / "loss.npy")
    assert loss.dtype == np.float32 and np.array_equal(loss, np.array(out["loss"], dtype=np.float32))
    for n in ("logits", "weights"):
        a = np.load(d / f"{n}.npy")
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,) and np.isfinite(a).all() and float(np.abs(a).max()) > 0
