"""bench.py's own multi-rank launch path (`python bench.py --gpus N` with no launcher), on the CPU with a stub step."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, env_drop=("WORLD_SIZE", "RANK", "LOCAL_RANK")):
    env = {k: v for k, v in os.environ.items() if k not in env_drop}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--steps", "3", "--warmup", "1", *extra],
                          env=env, capture_output=True, text=True, timeout=180)


def test_self_spawn_two_ranks_prints_one_line():
    r = _run("--gpus", "2")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"


def test_self_spawn_fails_when_a_rank_fails():
    r = _run("--gpus", "2", "--stub-fail-rank", "1")
    assert r.returncode != 0
    assert "rank exit codes" in r.stderr


def test_single_rank_needs_no_spawn():
    r = _run("--gpus", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip())["n_gpus"] == 1


def test_valu_roof_model():
    """The VALU roof bench.py reports: cfg3' is HBM-bound on paper, cfg3 / cfg4 are bound by the exact-order arithmetic."""
    sys.path.insert(0, ROOT)
    import bench
    roofs = {}
    for name, order in (("cfg2", 1), ("cfg3p", 1), ("cfg3", 2), ("cfg4", 0)):
        cfg = bench.WORKLOADS[name]
        valu, f32, f64 = bench.valu_roof_msamples(cfg, order)
        hbm = bench.HBM_PEAK_GBPS * 1e9 / (bench.BPS[cfg["fmt"]] + cfg["W"] * 4 / (cfg["S"] * cfg["lp"][1])) / 1e6
        roofs[name] = (valu, hbm)
        assert f32 >= 4.0 * cfg["lp"][2] / cfg["lp"][1]
    assert roofs["cfg2"][0] > roofs["cfg2"][1] and roofs["cfg3p"][0] > roofs["cfg3p"][1]     # hbm-bound
    assert roofs["cfg3"][0] < roofs["cfg3"][1] and roofs["cfg4"][0] < roofs["cfg4"][1]       # valu-bound


def test_steps_below_one_are_refused():
    r = _run("--steps", "0")
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


def test_dump_windows_are_fixed_and_bounded():
    """--dump-outputs: every window of a small output; of a large one a sample that depends on nothing but the shape, keeps the first
    and the last window and stays inside the budget (float32 norms + float64 indices)."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    assert np.array_equal(bench.dump_windows(1000, 128), np.arange(1000))
    for n, w in ((1 << 19, 128), (1 << 22, 64), (1 << 19, 1024)):
        a, b = bench.dump_windows(n, w), bench.dump_windows(n, w)
        assert np.array_equal(a, b) and a[0] == 0 and a[-1] == n - 1
        assert np.all(np.diff(a) > 0) and a.size * (w * 4 + 8) <= bench.DUMP_BUDGET < 64 * 10**6


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_dump_outputs_are_the_last_step_and_repeat(tmp_path):
    """bench.py --dump-outputs on a small cfg2 stream: every window's norms, and the same bytes whatever the number of timed steps
    (the input is a pure function of the arguments).  Child processes only: this process never touches the GPU."""
    import numpy as np
    dumps = []
    for steps in (1, 5):
        d = tmp_path / f"s{steps}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg2", "--samples-log2", "20", "--steps", str(steps),
                            "--warmup", "1", "--settle", "0", "--no-cpu-baseline", "--no-power", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == steps
        norms, windows = np.load(d / "norms.npy"), np.load(d / "windows.npy")
        assert norms.dtype == np.float32 and windows.dtype == np.float64
        assert norms.shape[1] == 128 and np.array_equal(windows, np.arange(norms.shape[0]))
        assert norms.shape[0] == (1 << 20) // (16 * 128) - 1 and np.isfinite(norms).all()
        dumps.append(norms)
    assert np.array_equal(dumps[0].view(np.uint32), dumps[1].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.spawns_gpu_ranks
def test_plain_run_is_lean_and_full_adds_the_rest():
    """A plain run prints the headline and the roofline of its own timed steps and nothing that takes runs of its own; --full adds
    the CPU baselines and the informational legs.  Child processes only: this process never touches the GPU."""
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-power", "--cpu-seconds", "0.5"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--samples-log2", "20", "--steps", "2", "--warmup", "1",
                            "--settle", "0", *extra], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[mode] = json.loads(r.stdout.strip().splitlines()[-1])
    for d in lines.values():
        assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
        assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["roofline"]["kernel_ms"] > 0
    extras = ("cpu_baseline", "cpu_allcores", "fast_mode", "write_sink")
    assert not any(k in lines["plain"] for k in extras) and "power" not in lines["plain"]["roofline"]
    assert all(k in lines["full"] for k in extras) and lines["full"]["cpu_baseline"]["value"] > 0
