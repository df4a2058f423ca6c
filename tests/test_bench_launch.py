"""bench.py contract on the CPU: ``python bench.py --gpus N`` without a launcher starts N ranks
itself, each with its own RANK and the shared private rendezvous, exactly one
JSON line comes out (rank 0), and a failing rank fails the whole run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

_STUB = r"""
import json, os, sys
d = sys.argv[1]
r = int(os.environ["RANK"])
open(os.path.join(d, "rank%d" % r), "w").write(json.dumps({k: os.environ[k] for k in
    ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}))
if os.environ.get("STUB_FAIL_RANK") == str(r):
    sys.exit(3)
if r == 0:
    print(json.dumps({"metric": "stub", "n_gpus": int(os.environ["WORLD_SIZE"])}), flush=True)
"""


def _run(tmp_path, n, extra_env=None):
    stub = tmp_path / "stub.py"
    stub.write_text(_STUB)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "MASTER_PORT")}
    env["KFAMD_BENCH_RANK_ARGV"] = json.dumps([sys.executable, str(stub), str(tmp_path)])
    env.update(extra_env or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)


def test_bench_self_launches_n_ranks(tmp_path):
    p = _run(tmp_path, 4)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 4
    ranks = [json.loads((tmp_path / f"rank{r}").read_text()) for r in range(4)]
    assert sorted(int(x["RANK"]) for x in ranks) == [0, 1, 2, 3]
    assert all(x["WORLD_SIZE"] == "4" and x["LOCAL_RANK"] == x["RANK"] for x in ranks)
    assert len({(x["MASTER_ADDR"], x["MASTER_PORT"]) for x in ranks}) == 1


def test_bench_rank_failure_fails_the_run(tmp_path):
    p = _run(tmp_path, 2, {"STUB_FAIL_RANK": "1"})
    assert p.returncode == 3, (p.returncode, p.stderr)


def test_launch_cli_runs_program_per_rank(tmp_path):
    stub = tmp_path / "stub.py"
    stub.write_text(_STUB)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "MASTER_PORT")}
    env.update({"LOCAL_WORLD_SIZE": "3", "MASTER_ADDR": "127.0.0.9", "MASTER_PORT": "29999"})
    p = subprocess.run([sys.executable, "-m", "kubeflow_rm_amd.parallel.launch", "--", str(stub), str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    ranks = [json.loads((tmp_path / f"rank{r}").read_text()) for r in range(3)]
    # the pod's injected rendezvous is used as is
    assert all(x["MASTER_ADDR"] == "127.0.0.9" and x["MASTER_PORT"] == "29999" for x in ranks)


def test_control_plane_latencies_measured():
    """BASELINE configs 3 / 5 (bench.py extra): Profile with GPU quota, TensorBoard, PVCViewer ready."""
    from tests.conftest import _ensure_native
    _ensure_native()
    from kubeflow_rm_amd.bench_coldstart import measure_control_plane
    r = measure_control_plane(runs=2)
    for k in ("profile_ready_p50_s", "tensorboard_ready_p50_s", "pvcviewer_ready_p50_s"):
        assert r[k] is not None and 0 < r[k] < 30, r


def test_dump_outputs_whole_and_seeded_row_sample(tmp_path, monkeypatch):
    """--dump-outputs: a small result is written whole as float32; one over the byte budget as the
    same sorted sample of whole rows every time, split between the ranks when there are several."""
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import bench

    c = torch.arange(40 * 8, dtype=torch.float32).reshape(40, 8).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "whole"), c, 0, 1)
    whole = np.load(tmp_path / "whole" / "c.npy")
    assert whole.dtype == np.float32 and np.array_equal(whole, c.float().numpy())

    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * 8 * 4)  # room for 10 rows
    bench.dump_outputs(str(tmp_path / "s1"), c, 0, 1)
    bench.dump_outputs(str(tmp_path / "s2"), c, 0, 1)
    s1, s2 = np.load(tmp_path / "s1" / "c.npy"), np.load(tmp_path / "s2" / "c.npy")
    assert s1.shape == (10, 8) and np.array_equal(s1, s2)
    rows = (s1[:, 0] / 8).astype(int)  # row r starts with 8 r: exact in bf16 up to 256
    assert np.all(np.diff(rows) > 0) and np.array_equal(s1, c.float().numpy()[rows])
    bench.dump_outputs(str(tmp_path / "s1"), c, 1, 2)
    assert np.load(tmp_path / "s1" / "c_rank1.npy").shape == (5, 8)


def _bench_gpu(*argv):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--prewarm-s", "0", "--gemm-m", "520", "--gemm-n", "392", "--gemm-k", "264", *argv],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_gpu_plain_run_times_the_steps_and_dumps_the_last_result(tmp_path):
    """A plain run: the K timed steps and the result line, nothing after them; --dump-outputs writes
    the GEMM result of the operands that the arguments determine (an odd shape with edge tiles)."""
    import numpy as np
    import torch
    d = _bench_gpu("--dump-outputs", str(tmp_path / "out"))
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["dtype"] == "bf16" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["unit"].startswith("TFLOPS")
    assert "extras_status" not in d and "correct" not in d and "cold_start_p50_s" not in d
    got = np.load(tmp_path / "out" / "c.npy")
    assert got.dtype == np.float32 and got.shape == (520, 392)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    a = (torch.rand(520, 264, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    b = (torch.rand(392, 264, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    ref = (a.double() @ b.double().t()).cpu().numpy()
    # fp32 accumulation of 264 bf16 products (2^-24 each, relative to sum |a||b| <= 264), then one
    # rounding of the result to bf16 (8 significand bits: unit roundoff 2^-8)
    tol = 2.0 ** -8 * np.abs(ref) + 264 * 264 * 2.0 ** -24
    assert np.all(np.abs(got - ref) <= tol), float(np.abs(got - ref).max())


@pytest.mark.gpu
def test_gpu_full_run_keeps_the_check_and_the_extras():
    d = _bench_gpu("--full", "--coldstart-runs", "0", "--ab-blocks", "1", "--budget-s", "120")
    assert d["correct"] is True and d["check_rows"] == 3 and d["ms_per_step"] > 0
    assert d["extras_status"]["gemm_ab_vs_hipblaslt"]["status"] == "ok" and d["ab_ours_tflops_median"] > 0


_HANG_STUB = r"""
import json, os, sys, time
sys.path.insert(0, sys.argv[2])
from kubeflow_rm_amd.bench_extras import Extras, print_line
r = int(os.environ["RANK"])
line = {"metric": "stub", "n_gpus": int(os.environ["WORLD_SIZE"])}
ex = Extras(float(sys.argv[3]), rank=r, grace_s=1.0, nonzero_rank_delay_s=1.0,
            emit=lambda rep: print_line({**line, **rep}))
ex.run("quick", lambda e: {"quick_value": 1}, est_s=0.1, timeout_s=5)
ex.run("broken", lambda e: 1 / 0, est_s=0.1, timeout_s=5)
ex.run("hang", lambda e: time.sleep(3600), est_s=0.1, timeout_s=2)
ex.run("never", lambda e: {"never": 1})
line.update(ex.finish())
ex.emit_once()
"""


def test_bench_extra_that_hangs_still_yields_the_line(tmp_path):
    """one extra hangs on every rank; the self-launched job still ends well inside
    the budget with exactly one JSON line, the hung extra marked ``timeout``, the finished ones kept,
    and the exit status is 124 (not the headline's 0)."""
    import time
    stub = tmp_path / "hang.py"
    stub.write_text(_HANG_STUB)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "MASTER_PORT")}
    env["KFAMD_BENCH_RANK_ARGV"] = json.dumps([sys.executable, str(stub), str(tmp_path), str(ROOT), "60"])
    t0 = time.time()
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    took = time.time() - t0
    assert p.returncode == 124, (p.returncode, p.stderr)  # a hang fails the run
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    st = d["extras_status"]
    assert st["quick"]["status"] == "ok" and d["quick_value"] == 1
    assert st["broken"]["status"] == "error" and "ZeroDivisionError" in st["broken"]["error"]
    assert st["hang"]["status"] == "timeout"
    assert "never" not in st and "never" not in d
    assert took < 40, took


def test_bench_extras_skip_what_does_not_fit_the_budget():
    from kubeflow_rm_amd.bench_extras import Extras
    ex = Extras(5.0)
    assert ex.run("fits", lambda e: {"x": 1}, est_s=1)
    assert not ex.run("too_big", lambda e: {"y": 1}, est_s=30)
    # collective extras follow the agreement, not the local view
    ex.agree = lambda ok: False
    assert not ex.run("peer_says_no", lambda e: {"z": 1}, est_s=0, collective=True)
    rep = ex.finish()
    assert rep["x"] == 1 and "y" not in rep and "z" not in rep
    assert rep["extras_status"]["too_big"]["status"] == "skipped"
    assert rep["extras_status"]["peer_says_no"]["status"] == "skipped"


def test_cold_start_failures_keep_their_count_and_diagnostics():
    """The default path's prefix is ``cold_start``: its failure COUNT (``cold_start_failures``) must
    not collide with the per-variant pod diagnostics (``cold_start_failure_diagnostics``)."""
    sys.path.insert(0, str(ROOT))
    import bench

    cs = {"runs": [0.1, 0.2], "p50_s": 0.1, "p90_s": 0.2, "failures": [{"pod": "bench/nb-3", "reason": "timeout"}]}
    out = bench._cs_keys("cold_start", cs)
    assert out["cold_start_failures"] == 1
    assert out["cold_start_failure_diagnostics"] == {"cold_start": cs["failures"]}
    out2 = bench._cs_keys("cold_start_odh", dict(cs, failures=[]))
    assert out2["cold_start_odh_failures"] == 0 and "cold_start_failure_diagnostics" not in out2
