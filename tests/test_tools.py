"""The measurement tools stay runnable: the microbenchmarks compile for gfx950 (CPU check), the per-rank slab cost tool runs
end to end on a small lattice (GPU)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("src", ["tile_pull_copy.hip", "march_pull_copy.hip", "march3d_pull_copy.hip", "tile_persist.hip", "tile_compact.hip"])
def test_microbenchmarks_compile(src, tmp_path):
    out = tmp_path / "a.out"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(ROOT, "tools", "microbench", src), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.exists()


def test_live_traffic_passes_stand_down_without_side_effects(monkeypatch, tmp_path):
    """bench.py counts its HBM bytes with rocprofv3 passes over a child process; it must start none when it is itself being profiled
    (rocprofv3 exports ROCPROF_* to the profiled process), when rocprofv3 is missing, and after one pass of the run has failed"""
    sys.path.insert(0, ROOT)
    import bench
    started = []
    monkeypatch.setattr(subprocess, "Popen", lambda *a, **k: started.append(a) or (_ for _ in ()).throw(AssertionError("a pass was started")))
    monkeypatch.setenv("ROCPROF_OUTPUT_PATH", str(tmp_path))
    assert bench.under_rocprof()
    bench._LIVE["ok"] = True
    assert bench.live_pmc_traffic("rk3dq_fused<false", ["--steps", "1"]) is None and not started
    # one failure ends the live passes of the run
    assert bench._LIVE["ok"] is False
    monkeypatch.delenv("ROCPROF_OUTPUT_PATH")
    assert not bench.under_rocprof()
    assert bench.live_pmc_traffic("rk3dq_fused<false", ["--steps", "1"]) is None and not started
    # no rocprofv3 on the machine
    bench._LIVE["ok"] = True
    monkeypatch.setattr(shutil, "which", lambda name: None)
    monkeypatch.setattr(os.path, "exists", lambda path: False)
    assert bench.live_pmc_traffic("rk3dq_fused<false", ["--steps", "1"]) is None and not started
    bench._LIVE["ok"] = True


@pytest.mark.gpu
def test_slab_rank_cost_runs_on_a_small_lattice():
    env = dict(os.environ, LBMPM_K3_RELAX="SRT")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "slab_rank_cost.py"), "64", "2", "4"], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("rank ")]
    assert len(lines) == 2 and "sum over ranks" in r.stdout


@pytest.mark.gpu
def test_pipelined_slab_bench_reports_a_bit_equal_run():
    """tools/slabbench_pipelined.py: k ranks of lbmpm_rk3d_step_slab on one GPU (one host thread per rank, exact exchange) -- the tool
    that showed round 3's face-message bug; its verdict line must say the run equals the single domain"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "slabbench_pipelined.py"), "96", "3", "4"], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, LBMPM_K3_RELAX="MRT"), cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "k=3 pipelined step_slab" in r.stdout and "bit for bit: True" in r.stdout, r.stdout[-1500:]


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_sample_depends_on_the_whole_lattice_alone(tmp_path):
    """bench.py --dump-outputs: float64 files of at most DUMP_CELLS values, the same seeded sample of fluid cells (ascending) on every
    call, and the same files whether rank 0 holds the whole lattice or the planes of two ranks are gathered to it (any cut)"""
    import numpy as np
    bench = _bench_module()
    rng = np.random.default_rng(5)
    dom = (rng.random((24, 128, 640)) > 0.35).astype(np.uint8)
    assert (dom == 1).sum() > bench.DUMP_CELLS
    fields = {n: rng.standard_normal(dom.shape) for n in ("rhoR", "rhoB", "vx", "vy", "vz", "phi")}
    whole = tmp_path / "whole"
    bench.dump_outputs(str(whole), {n: (lambda a=a: a) for n, a in fields.items()}, dom)
    idx = bench.dump_sample(dom)
    assert idx.size == bench.DUMP_CELLS and np.all(np.diff(idx) > 0) and np.all(dom.reshape(-1)[idx] == 1)
    assert np.array_equal(idx, bench.dump_sample(dom.copy()))
    sparse = np.zeros_like(dom); sparse[::3, ::2] = dom[::3, ::2]      # fewer fluid cells than DUMP_CELLS: every one of them
    assert np.array_equal(bench.dump_sample(sparse), np.flatnonzero(sparse == 1))
    assert sorted(p.name for p in whole.iterdir()) == sorted(n + ".npy" for n in fields)
    assert sum(p.stat().st_size for p in whole.iterdir()) <= 64 * 10 ** 6
    for n, a in fields.items():
        got = np.load(whole / (n + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a.reshape(-1)[idx])
    for cut in (5, 17):                     # two ranks: rank 1 hands its planes over, rank 0 stacks them below its own
        sent = []
        split = tmp_path / ("cut%d" % cut)
        bench.dump_outputs(str(split), {n: (lambda a=a: a[cut:]) for n, a in fields.items()}, dom, rank=1, gather=lambda a: sent.append(a))
        assert not split.exists() and len(sent) == len(fields)
        queue = iter(sent)
        bench.dump_outputs(str(split), {n: (lambda a=a: a[:cut]) for n, a in fields.items()}, dom, rank=0,
                           gather=lambda a: np.concatenate([a, next(queue)], axis=0))
        for n in fields:
            assert np.array_equal(np.load(split / (n + ".npy")), np.load(whole / (n + ".npy"))), (cut, n)
    # replicas (no gather): rank 0 writes, the others nothing; a lattice of at most DUMP_CELLS cells is written whole
    small = tmp_path / "small"
    bench.dump_outputs(str(small), {"rhoR": lambda: np.ones((40, 50))}, np.ones((40, 50), np.uint8), rank=1)
    assert not small.exists()
    bench.dump_outputs(str(small), {"rhoR": lambda: np.ones((40, 50), np.float32)}, np.ones((40, 50), np.uint8), rank=0)
    got = np.load(small / "rhoR.npy")
    assert got.dtype == np.float64 and got.shape == (2000,)
    with pytest.raises(ValueError):
        bench.dump_outputs(str(small), {"f%d" % k: (lambda: np.ones((40, 50))) for k in range(bench.DUMP_MAX_FIELDS + 1)}, np.ones((40, 50), np.uint8))


def _bench_line(args, env=None, timeout=600):
    env = {k: v for k, v in (env or os.environ).items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    import json
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_its_outputs(tmp_path):
    """a plain run times its steps and prints the headline only (no CPU baseline, secondary workloads, stream test or counter passes);
    --dump-outputs writes the same files on every run, and a two-rank run (gloo rehearsal on this GPU, slabs cut by measured cost)
    writes the one-rank run's files bit for bit"""
    import numpy as np
    bench = _bench_module()
    size = ["--size", "128", "128", "128", "--steps", "4", "--warmup", "1"]
    d = _bench_line(size + ["--dump-outputs", str(tmp_path / "a")])
    assert d["steps"] == 4 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "MLUPS" and d["dtype"] == "f64"
    assert not any(k.startswith("cpu_baseline") or k == "secondary" for k in d)
    assert d["roofline"]["measured_stream_ceiling"] is None and d["roofline"]["traffic_live"] is None
    _bench_line(size + ["--dump-outputs", str(tmp_path / "b")])
    _bench_line(["--gpus", "2"] + size + ["--dump-outputs", str(tmp_path / "n2")], env=dict(os.environ, LBMPM_DIST_BACKEND="gloo"))
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(n + ".npy" for n in ("rhoR", "rhoB", "vx", "vy", "vz", "phi"))
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= 64 * 10 ** 6
    for n in names:
        a = np.load(tmp_path / "a" / n)
        assert a.dtype == np.float64 and a.shape == (bench.DUMP_CELLS,) and np.isfinite(a).all()
        assert np.array_equal(a, np.load(tmp_path / "b" / n)), n
        assert np.array_equal(a, np.load(tmp_path / "n2" / n)), n
    assert sorted(p.name for p in (tmp_path / "n2").iterdir()) == names


@pytest.mark.gpu
def test_full_bench_line_carries_the_extras():
    """--full adds what a plain run leaves out: the CPU baselines and the measured stream ceiling (secondary workloads and counter
    passes switched off here to keep the test short)"""
    d = _bench_line(["--full", "--no-secondary", "--no-live-traffic", "--size", "128", "128", "128", "--steps", "4", "--warmup", "1"])
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline_reference_shape"]["value"] > 0
    assert d["roofline"]["measured_stream_ceiling"]["copy_GBs"] > 0 and "secondary" not in d
