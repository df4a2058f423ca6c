"""Pod zygote (kubelet --pod-zygote, kubeflow_rm_amd/images/zygote.py): notebook containers fork
from a pre-imported interpreter instead of exec'ing a fresh one.

Checks the container contract survives the fork: the pod's own env, cwd, log and process session;
readiness through the gateway; the exit status of a crashing container reaches the pod status
(restartCount, terminated exit code) although the kubelet is not the process's parent; deletion
kills the process; and a zygote that is gone falls back to a fresh interpreter.
"""
import json
import os
import shutil
import signal
import tempfile
import time
import urllib.error
import urllib.request
from pathlib import Path

import pytest

from kubeflow_rm_amd.cluster import LocalCluster

NB = "kubeflow.org/v1"


def _notebook(name, ns, env=None):
    c = {"name": name, "image": "jupyter-scipy:latest", "env": env or []}
    return {"apiVersion": NB, "kind": "Notebook", "metadata": {"name": name, "namespace": ns},
            "spec": {"template": {"spec": {"containers": [c]}}}}


def _ready(o):
    return (o.get("status") or {}).get("readyReplicas") == 1


@pytest.fixture(scope="module")
def zc():
    with LocalCluster(gpus=0, zygote=True) as cl:
        cl.wait_zygotes(timeout=300)
        cl.client.create({"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": "zy"}})
        yield cl


@pytest.fixture
def zsock(tmp_path):
    """Path for a zygote's socket. An AF_UNIX address holds at most 107 bytes and the zygote binds
    ``<path>.tmp`` first: under a deep temporary root pytest's tmp_path is too long for it, and the
    socket gets a short directory of its own."""
    path = str(tmp_path / "z.sock")
    if len(os.fsencode(path + ".tmp")) <= 100:
        yield path
        return
    base = tempfile.gettempdir()
    d = tempfile.mkdtemp(prefix="zy-", dir=base if len(os.fsencode(base)) <= 70 else "/tmp")
    try:
        yield os.path.join(d, "z.sock")
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _get(url):
    deadline = time.time() + 20
    while True:
        try:
            with urllib.request.urlopen(url, timeout=5) as r:
                return json.loads(r.read())
        except (urllib.error.URLError, ConnectionError):
            if time.time() > deadline:
                raise
            time.sleep(0.1)


def _pid_of(c, pod, ns):
    st = c.get("v1", "Pod", pod, ns)["status"]["containerStatuses"][0]
    return int(st["containerID"].split("://")[1])


def test_notebook_forks_from_zygote_with_its_own_env(zc):
    c = zc.client
    c.create(_notebook("z1", "zy", env=[{"name": "KFAMD_GPU_TOPOLOGY", "value": "zygote-env-test"}]))
    c.wait_for(NB, "Notebook", "z1", "zy", _ready, timeout=60)
    logs = c.pod_logs("z1-0", "zy")
    assert "forked from zygote" in logs, logs
    ip = c.get("v1", "Pod", "z1-0", "zy")["status"]["podIP"]
    info = _get(f"http://{ip}:8888/notebook/zy/z1/api/gpu")
    # the container's env (read by the server at run time; /proc/<pid>/environ shows the zygote's
    # initial block, as for any process that changed its environment)
    assert info["topology"] == "zygote-env-test" and "cpus_allowed" in info
    assert "serving /notebook/zy/z1 on" in c.pod_logs("z1-0", "zy")
    pid = _pid_of(c, "z1-0", "zy")
    # its own session (the kubelet kills the process group) and the pod's working directory
    assert os.getsid(pid) == pid
    assert "/pods/zy_z1-0_" in os.readlink(f"/proc/{pid}/cwd")
    # torch came preloaded: the container did not import it itself
    assert "torch" in Path(f"/proc/{pid}/maps").read_text()


def test_crash_exit_code_reaches_pod_status(zc):
    c = zc.client
    c.create(_notebook("z2", "zy", env=[{"name": "NB_PORT", "value": "not-a-port"}]))

    def crashed(o):
        for cs in (o.get("status") or {}).get("containerStatuses") or []:
            last = (cs.get("lastState") or {}).get("terminated") or (cs.get("state") or {}).get("terminated")
            if cs.get("restartCount", 0) >= 1 and last and last.get("exitCode") == 1:
                return True
        return False
    c.wait_for("v1", "Pod", "z2-0", "zy", crashed, timeout=60)
    assert "ValueError" in c.pod_logs("z2-0", "zy")
    c.delete(NB, "Notebook", "z2", "zy")


def test_delete_kills_forked_process(zc):
    c = zc.client
    pid = _pid_of(c, "z1-0", "zy")
    c.delete(NB, "Notebook", "z1", "zy")
    c.wait_gone("v1", "Pod", "z1-0", "zy", timeout=60)
    deadline = time.time() + 10
    while time.time() < deadline:
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            break
        time.sleep(0.05)
    else:
        pytest.fail(f"forked container {pid} still alive after pod deletion")


def test_fresh_interpreter_when_zygote_is_gone_then_restarted(zc):
    c = zc.client
    socks = zc.wait_zygotes()
    zpid = None
    for lg in (Path(zc.data_dir) / "kubelet").glob("zygote-*.log"):
        for line in lg.read_text().splitlines():
            if "ready on" in line:
                zpid = int(line.split("pid ")[1].split()[0])
    assert zpid
    os.kill(zpid, signal.SIGKILL)  # its socket file stays behind: connect is refused
    assert socks
    c.create(_notebook("z3", "zy"))
    c.wait_for(NB, "Notebook", "z3", "zy", _ready, timeout=60)
    logs = c.pod_logs("z3-0", "zy")
    assert "forked from zygote" not in logs
    c.delete(NB, "Notebook", "z3", "zy")
    # the kubelet restarts the zygote (heartbeat-thread supervision), and containers fork from it again
    deadline = time.time() + 120
    new_pid = None
    while time.time() < deadline and new_pid is None:
        for lg in (Path(zc.data_dir) / "kubelet").glob("zygote-*.log"):
            for line in lg.read_text().splitlines():
                if "ready on" in line and int(line.split("pid ")[1].split()[0]) != zpid:
                    new_pid = int(line.split("pid ")[1].split()[0])
        time.sleep(0.2)
    assert new_pid, "zygote not restarted"
    c.wait_gone("v1", "Pod", "z3-0", "zy", timeout=60)
    c.create(_notebook("z4", "zy"))
    c.wait_for(NB, "Notebook", "z4", "zy", _ready, timeout=60)
    assert f"forked from zygote {new_pid}" in c.pod_logs("z4-0", "zy")
    with urllib.request.urlopen(zc.url + "/metrics", timeout=10) as r:
        metrics = r.read().decode()
    assert 'kubelet_container_starts_total{mode="zygote"}' in metrics
    assert 'kubelet_container_starts_total{mode="fresh"}' in metrics
    assert "kubelet_zygote_restarts_total 1" in metrics
    c.delete(NB, "Notebook", "z4", "zy")


@pytest.mark.gpu
def test_gpu_torch_ready_notebook_forked_from_zygote():
    """On the GPU: the torch-ready server forked from the zygote creates its own HIP context on the
    pod's GPU, runs the MFMA GEMM and passes the fp32 spot check; the GPU readiness sidecar passes."""
    from kubeflow_rm_amd.bench_coldstart import measure_cold_start
    r = measure_cold_start(runs=2, gpus_per_notebook=1, server="torch-ready", zygote=True, namespace="zy-gpu",
                           settle_s=0.3, timeout=120)
    assert len(r["runs"]) == 2
    for run in r["runs"]:
        w = run["server_warmup"] or {}
        assert w.get("ok") is True, run
        assert w.get("import_torch_ms", 1e9) < 50, w  # preloaded, not imported by the container
    assert (r.get("readiness") or {}).get("ok", True) is not False


@pytest.mark.gpu
def test_gpu_torch_ready_notebook_fresh_interpreter_is_reliable():
    """the fresh-interpreter torch-ready server (import torch, HIP pre-init after
    torch._C, MFMA GEMM, fp32 spot check) becomes Ready in <= 4 s in every one of 5 runs, with no
    failed run."""
    from kubeflow_rm_amd.bench_coldstart import measure_cold_start
    r = measure_cold_start(runs=5, gpus_per_notebook=1, server="torch-ready", namespace="fresh-gpu",
                           settle_s=0.3, timeout=30, max_failures=1)
    assert not r["failures"], r["failures"]
    assert len(r["runs"]) == 5
    for run in r["runs"]:
        w = run["server_warmup"] or {}
        assert w.get("ok") is True, run
        assert w.get("hip_preinit") == "after-c", w
        assert (w.get("preinit_ms") or {}).get("step") == "done", w
        assert run["cold_start_s"] <= 4.0, [x["cold_start_s"] for x in r["runs"]]


def test_zygote_protocol_thread_pool_env_argv_exit(tmp_path, zsock):
    """The protocol directly: a forked container gets its own CPU mask with a torch/OpenMP pool sized
    to it (not the zygote's), its env, argv and cwd; the exit status comes back on the connection."""
    import socket
    import subprocess
    import sys
    root = Path(__file__).resolve().parents[1]
    sock = zsock
    env = dict(os.environ, PYTHONPATH=str(root))
    env.pop("OMP_NUM_THREADS", None)
    env.pop("OPENBLAS_NUM_THREADS", None)
    z = subprocess.Popen([sys.executable, "-m", "kubeflow_rm_amd.images.zygote", "--socket", sock,
                          "--preload", "numpy,torch"], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    try:
        deadline = time.time() + 120
        while not os.path.exists(sock):
            assert z.poll() is None and time.time() < deadline
            time.sleep(0.05)
        assert oct(os.stat(sock).st_mode & 0o777) == "0o600"
        # fork-safe: numpy (OpenBLAS) and torch preloaded, yet only the main thread exists
        assert len(os.listdir(f"/proc/{z.pid}/task")) == 1
        cpus = sorted(os.sched_getaffinity(0))[:2]

        def run(extra_env, exit_code):
            log = tmp_path / f"c{exit_code}.log"
            s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
            s.connect(sock)
            req = {"argv": ["-m", "tests.zygote_probe_mod", "a1", "a2"], "cwd": str(tmp_path), "log": str(log),
                   "cpus": cpus, "env": [f"PYTHONPATH={root}", "PROBE_VAR=v", f"PROBE_EXIT={exit_code}", *extra_env]}
            s.sendall((json.dumps(req) + "\n").encode())
            f = s.makefile("r")
            pid = json.loads(f.readline())["pid"]
            st = json.loads(f.readline())
            s.close()
            probe = json.loads([ln for ln in log.read_text().splitlines() if ln.startswith("PROBE ")][0][6:])
            return pid, st, probe
        pid, st, probe = run([], 0)
        assert st == {"exit": 0, "signal": 0}
        assert probe["cpus"] == cpus and probe["threads"] == len(cpus)
        assert probe["blas_threads"] == [len(cpus)]  # grown back from the zygote's 1
        assert probe["env"] == "v" and probe["argv"] == ["a1", "a2"] and probe["cwd"] == str(tmp_path)
        pid, st, probe = run(["OMP_NUM_THREADS=1"], 3)
        assert st["exit"] == 3 and probe["threads"] == 1 and probe["blas_threads"] == [1]
        assert len(os.listdir(f"/proc/{z.pid}/task")) == 1
    finally:
        z.terminate()
        z.wait(timeout=10)


@pytest.mark.gpu
def test_gpu_exec_into_torch_ready_notebook():
    """On the GPU: kfctl-style exec into a GPU notebook (forked from the zygote) runs a torch op on the
    pod's GPU from the container's environment."""
    with LocalCluster(gpus=None, zygote=True) as cl:
        cl.wait_zygotes(timeout=300)
        c = cl.client
        c.create({"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": "zx"}})
        c.create({"apiVersion": NB, "kind": "Notebook", "metadata": {"name": "g", "namespace": "zx"},
                  "spec": {"template": {"spec": {"containers": [{
                      "name": "g", "image": "kfamd/jupyter-pytorch-rocm:latest",
                      "env": [{"name": "KFAMD_WARMUP", "value": "torch"}],
                      "resources": {"limits": {"amd.com/gpu": "1"}}}]}}}})
        c.wait_for(NB, "Notebook", "g", "zx", _ready, timeout=120)
        r = c.pod_exec("g-0", "zx", ["python3", "-c", "import torch; print(float(torch.ones(4, device='cuda').sum()), "
                                     "torch.cuda.device_count())"], timeout=120)
        assert r["exitCode"] == 0, r
        assert r["output"].strip().splitlines()[-1] == "4.0 1"
        c.delete(NB, "Notebook", "g", "zx")


def test_zygote_refuses_a_multithreaded_preload(tmp_path):
    """A preload that leaves a native thread behind makes the zygote refuse to serve (exit 4), naming
    the threads; the kubelet then starts containers as fresh interpreters."""
    import subprocess
    import sys
    root = Path(__file__).resolve().parents[1]
    sock = str(tmp_path / "z.sock")
    p = subprocess.run([sys.executable, "-m", "kubeflow_rm_amd.images.zygote", "--socket", sock,
                        "--preload", "tests.zygote_thread_mod"], env=dict(os.environ, PYTHONPATH=str(root)),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 4, p.stdout + p.stderr
    assert "refusing to serve" in p.stdout and "2 threads" in p.stdout, p.stdout
    assert not os.path.exists(sock)


def test_zygote_rejects_malformed_requests(tmp_path, zsock):
    import socket
    import subprocess
    import sys
    root = Path(__file__).resolve().parents[1]
    sock = zsock
    z = subprocess.Popen([sys.executable, "-m", "kubeflow_rm_amd.images.zygote", "--socket", sock],
                         env=dict(os.environ, PYTHONPATH=str(root)), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    try:
        deadline = time.time() + 60
        while not os.path.exists(sock):
            assert z.poll() is None and time.time() < deadline
            time.sleep(0.05)
        for bad in (b"not json\n", b'{"argv": ["python", "x.py"], "cwd": "/", "log": "/dev/null"}\n',
                    b'{"argv": ["-m", "x"], "log": "/dev/null"}\n'):
            s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
            s.connect(sock)
            s.sendall(bad)
            reply = json.loads(s.makefile("r").readline())
            s.close()
            assert "error" in reply and "pid" not in reply, reply
        assert z.poll() is None  # still serving
    finally:
        z.terminate()
        z.wait(timeout=10)


def test_operator_image_recipe_with_its_own_zygote(tmp_path):
    """--image-recipes: an operator maps an image to a command and opts it into a zygote with its own
    preload list; containers of that image fork from it."""
    recipes = tmp_path / "recipes.json"
    recipes.write_text(json.dumps([{"match": "acme/lab", "argv": ["{python}", "-m", "kubeflow_rm_amd.images.notebook_server"],
                                    "zygote": "json,kubeflow_rm_amd.images.notebook_server"}]))
    with LocalCluster(gpus=0, zygote=True, args=["--image-recipes", str(recipes)]) as cl:
        socks = cl.wait_zygotes(timeout=300)
        assert len(socks) == 2  # the built-in notebook zygote + the operator's
        c = cl.client
        c.create({"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": "op"}})
        c.create({"apiVersion": NB, "kind": "Notebook", "metadata": {"name": "a", "namespace": "op"},
                  "spec": {"template": {"spec": {"containers": [{"name": "a", "image": "acme/lab:1"}]}}}})
        c.wait_for(NB, "Notebook", "a", "op", _ready, timeout=60)
        logs = c.pod_logs("a-0", "op")
        assert "recipe:acme/lab" in logs and "preloaded json,kubeflow_rm_amd.images.notebook_server" in logs, logs


def test_cold_start_bench_zygote_path_on_cpu():
    """bench_coldstart's zygote path end to end on the CPU (synthetic GPUs, no readiness op): the
    cluster waits for its zygote, the runs complete and their phases are recorded."""
    from kubeflow_rm_amd.bench_coldstart import measure_cold_start
    r = measure_cold_start(runs=2, gpus_per_notebook=1, gpus=2, readiness=False, zygote=True, namespace="zy-cpu",
                           settle_s=0.0, timeout=60)
    assert len(r["runs"]) == 2 and r["zygote"] is True
    assert r["p50_s"] < 30 and "create_to_pod_ready_s" in r["phases_p50_s"]


@pytest.mark.gpu
def test_gpu_warm_child_takes_the_one_gpu_notebook():
    """the product's default cold start. The torch zygote keeps a warm child per GPU
    (HIP + torch's device context + the first GEMM's code object already up); each 1-GPU torch-ready
    notebook takes the warm child of its GPU, so HIP bring-up is off the cold-start path, and the
    server's own warmup (GEMM + fp32 spot check) still runs in the pod and passes."""
    from kubeflow_rm_amd.bench_coldstart import measure_cold_start
    r = measure_cold_start(runs=3, gpus_per_notebook=1, server="torch-ready", zygote=True, namespace="zy-warm",
                           settle_s=1.0, timeout=60)
    assert not r["failures"], r["failures"]
    assert r["warm_children"] >= 2, [x.get("warm_child") for x in r["runs"]]
    for run in r["runs"]:
        w = run["server_warmup"] or {}
        assert w.get("ok") is True, run
    warm = [x for x in r["runs"] if x.get("warm_child")]
    assert min(x["server_warmup"]["total_ms"] for x in warm) < 80, [x["server_warmup"] for x in warm]
    # the gpu-readiness sidecar's op ran in the node's warm op of the GPU (kfamd-readiness --warm-op)
    assert sum(x["readiness_stages"].get("warm_op", 0) for x in r["runs"]) >= 2, [x["readiness_stages"] for x in r["runs"]]


def test_warm_children_fail_soft_without_a_gpu(tmp_path, zsock):
    """On a host without a GPU a zygote asked for warm children reports each failure (at most 3 in a
    row per device) and keeps serving plain forks."""
    import socket
    import subprocess
    import sys
    root = Path(__file__).resolve().parents[1]
    sock = zsock
    log = tmp_path / "z.log"
    env = dict(os.environ, PYTHONPATH=str(root), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    with open(log, "w") as lf:
        z = subprocess.Popen([sys.executable, "-m", "kubeflow_rm_amd.images.zygote", "--socket", sock, "--preload", "torch",
                              "--warm-devices", "0"], env=env, stdout=lf, stderr=subprocess.STDOUT)
    try:
        deadline = time.time() + 120
        while not os.path.exists(sock):
            assert z.poll() is None and time.time() < deadline, log.read_text()
            time.sleep(0.05)
        if "torch" in sys.modules and __import__("torch").cuda.is_available():
            pytest.skip("a GPU is visible: warm children succeed here")
        while log.read_text().count("for device 0 failed") < 3:
            assert z.poll() is None and time.time() < deadline, log.read_text()
            time.sleep(0.1)
        s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        s.connect(sock)
        out = tmp_path / "c.log"
        s.sendall((json.dumps({"argv": ["-m", "tests.zygote_probe_mod"], "cwd": str(tmp_path), "log": str(out),
                               "env": [f"PYTHONPATH={root}", "PROBE_EXIT=0"], "warm_device": 0}) + "\n").encode())
        f = s.makefile("r")
        rep = json.loads(f.readline())
        assert "pid" in rep and not rep.get("warm")
        assert json.loads(f.readline()) == {"exit": 0, "signal": 0}
        s.close()
        time.sleep(1.5)  # no fourth warm attempt
        assert log.read_text().count("for device 0 failed") == 3
    finally:
        z.terminate()
        z.wait(timeout=10)
