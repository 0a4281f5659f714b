"""bench.py's --dump-outputs and --full: the dump's size bound and run-to-run identity (CPU), and on the GPU that a
plain run's dump is exactly what the last timed step computed -- the frames re-rendered in-process from the same seed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    rng = np.random.default_rng(3)
    arrays = {"rgb": rng.random((16, 32, 3), dtype=np.float32),          # 6144 B: over its share of 4096 / 3
              "grid_W": rng.random((1, 8, 8), dtype=np.float32),         # 256 B: under it, kept whole
              "grid_M": rng.integers(0, 2 ** 32, (1, 16, 32), dtype=np.uint32)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = 0
    for name, src in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == (np.float32 if src.dtype == np.float32 else np.float64)
        assert np.array_equal(a, b), name   # the same elements on every run
        total += a.nbytes
    assert total <= 4096
    assert np.array_equal(np.load(tmp_path / "a" / "grid_W.npy"), arrays["grid_W"])
    # a sample holds elements of its array (integers exactly, as float64), in index order
    m = np.load(tmp_path / "a" / "grid_M.npy")
    assert m.ndim == 1 and m.size == 4096 // 3 // 8 and np.isin(m, arrays["grid_M"].astype(np.float64)).all()
    # under the budget nothing is cut
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    bench.dump_outputs(str(tmp_path / "c"), arrays)
    assert np.array_equal(np.load(tmp_path / "c" / "rgb.npy"), arrays["rgb"])
    assert np.array_equal(np.load(tmp_path / "c" / "grid_M.npy"), arrays["grid_M"].astype(np.float64))


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["c2", "c3"])
def test_plain_run_dumps_the_last_timed_frame(tmp_path, config):
    """bench.py --steps 2 --warmup 1 on a 96 x 64 tile: the result line is a plain one (2 timed steps, nothing of --full)
    and the dump equals frame 2 of the same sequence rendered here, bit for bit (c3: with the grid threaded through)."""
    import bench
    from romis_amd import _abi, restir, scene
    W, H, steps, warmup = 96, 64, 2, 1
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                          str(warmup), "--config", config, "--tile-width", str(W), "--tile-height", str(H),
                          "--prewarm-gemm-ms", "0", "--dump-outputs", str(tmp_path)], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["full"] is False
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "f32" and d["higher_is_better"] is True
    # ms_per_step is the time of one timed step: value follows from it (both are rounded in the line: within 1 %)
    assert abs(d["value"] - W * H / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-2 * d["value"]
    assert d["kernels"] is None and d["cpu_baseline"] is None and d["roofline_ris"] is None
    assert "measured_read_peak" not in (d["roofline"] or {})

    cf = bench.CONFIGS[config]
    f = _abi.default_features(initial_light_samples=cf["M"], num_samples_in_reservoir=1, num_neighbours_to_sample=5,
                              spatial_resample_radius=10, spatial_resampling_passes=cf["passes"], spatial_reuse=1,
                              temporal_reuse=cf["temporal"], unbiased_combination=cf["unbiased"],
                              spatial_reuse_visibility_check=cf["vis"])
    cam = scene.camera_for(cf["scene"], W, H, None)
    tile = restir.tile_plan(W, H, 1, 1, 0, cf["passes"] * 10)
    r = restir.Renderer(0)
    try:
        r.set_scene(scene.bench_scene(cf["scene"]))
        r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
        grid = None
        for i in range(warmup + steps):
            last = i == warmup + steps - 1
            rgb, g = r.render_restir(grid if cf["temporal"] else None, cam, W, H, f, tile=tile, want_rgb=last,
                                     want_grid=bool(cf["temporal"]))
            grid = g
        want = {"rgb": rgb}
        if cf["temporal"]:
            want.update(zip(("grid_pos", "grid_color", "grid_W", "grid_M"), grid.download()))
        del grid, g
    finally:
        r.close()
    assert sorted(p for p in os.listdir(tmp_path) if p.endswith(".npy")) == sorted(k + ".npy" for k in want)
    for name, w_ in want.items():
        got = np.load(tmp_path / f"{name}.npy")
        if name == "grid_M":
            assert got.dtype == np.float64 and np.array_equal(got, w_.astype(np.float64)), name
        else:
            assert got.dtype == np.float32 and got.shape == w_.shape, name
            assert np.array_equal(got.view(np.uint32), w_.view(np.uint32)), name
