"""bench.py contract tests: single-process and torchrun world-2 (gloo on
CPU — the same code path the driver uses with RCCL on GPUs)."""
import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent

REQUIRED_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
                 "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config"}


def _last_json(text: str) -> dict:
    for line in reversed(text.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{text[-2000:]}")


def test_bench_single_process():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--model", "tiny", "--calls", "2", "--prompt-len", "16",
         "--gen-len", "4"],
        cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    j = _last_json(out.stdout)
    assert REQUIRED_KEYS <= set(j)
    assert j["n_gpus"] == 1 and j["value"] > 0
    assert j["config"]["model"] == "tiny"
    assert j["config"]["parallelism"] == "dp1"


def _run_dump(tmp_path, name, *extra):
    import numpy as np
    d = tmp_path / name
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--model", "tiny", "--calls", "3",
         "--prompt-len", "16", "--gen-len", "4", "--device", "cpu",
         "--dump-outputs", str(d), *extra],
        cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    j = _last_json(out.stdout)
    assert j["steps"] == 2 and j["ms_per_step"] > 0
    arrays = {p.stem: np.load(p) for p in d.glob("*.npy")}
    for a in arrays.values():
        assert a.dtype == np.float32
    return arrays


def test_bench_dump_outputs_engine_only(tmp_path):
    """--dump-outputs writes the last timed step's token ids; the same
    arguments give the same inputs, so two runs agree exactly.  --full is
    accepted and leaves the headline path alone."""
    import numpy as np
    a = _run_dump(tmp_path, "a", "--engine-only")
    b = _run_dump(tmp_path, "b", "--engine-only", "--full")
    assert set(a) == {"tokens"}
    assert a["tokens"].shape == (3, 4)
    assert (a["tokens"] >= 0).all() and (a["tokens"] < 512).all()
    assert np.array_equal(a["tokens"], b["tokens"])


def test_bench_dump_outputs_rest(tmp_path):
    a = _run_dump(tmp_path, "a")
    assert set(a) == {"tokens", "text_bytes"}
    assert a["tokens"].shape == (3, 4) and (a["tokens"] >= 0).all()
    assert a["text_bytes"].shape[0] == 3


def test_bench_torchrun_world2():
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29687", "bench.py", "--gpus", "2", "--steps", "2",
         "--warmup", "0", "--model", "tiny", "--calls", "2",
         "--device", "cpu",  # gloo on CPU, also where GPUs are visible
         "--prompt-len", "16", "--gen-len", "4"],
        cwd=REPO, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    j = _last_json(out.stdout)
    assert j["n_gpus"] == 2
    assert j["config"]["parallelism"] == "dp2"
    assert j["config"]["global_batch"] == 4
