"""tests/cpp/history_gather_frames.cpp -- Renderer::historyGather and romis::HistoryGather of include/romis_amd/restir.hpp --
compiles and links (CPU), and on the GPU writes the BMP the Python binding writes for the same four frames of a yawing
camera, folded into the image history with the bilinear gather, filtered and tone mapped."""
import os
import subprocess

import pytest

from romis_amd import _abi, restir, scene
from test_cpp_wrapper import build_cpp, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "history_gather_frames.cpp")
BIN = os.path.join(ROOT, "romis_amd", "_build", "history_gather_frames")
NAME = "nightclub_128pt"
STEP = "0.0078125"   # 2^-7 in the camera's own unit: exact in float32, so the program's cameras are these


def test_example_compiles_and_links():
    assert os.path.exists(build_cpp(SRC, BIN))


@pytest.mark.gpu
def test_cpp_example_writes_the_python_bindings_file(tmp_path):
    W, H = 70, 37
    sc, cam = scene.bench_scene(NAME), scene.camera_for(NAME, W, H)
    write_scene(tmp_path / "s.bin", sc, cam)
    got = tmp_path / "cpp.bmp"
    subprocess.check_call([build_cpp(SRC, BIN), str(tmp_path / "s.bin"), str(got), str(W), str(H), STEP], timeout=120)
    f = _abi.default_features(num_samples_in_reservoir=1, initial_light_samples=32, num_neighbours_to_sample=5,
                              spatial_resample_radius=10, spatial_reuse=1, temporal_reuse=0, spatial_resampling_passes=1,
                              enable_tone_mapping=0)
    tone = _abi.default_features(enable_tone_mapping=1, exposure=1.5, gamma=2.2)

    def python_file(mode, path):
        r = restir.Renderer(0)
        try:
            assert r.history_gather() == restir.HISTORY_GATHER_NEAREST
            assert r.history_gather(mode) == mode
            r.set_scene(sc)
            r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
            r.history_begin()
            c = _abi.Camera.from_buffer_copy(cam)
            for k in range(4):
                if k:
                    c.rotation[1] = c.rotation[1] + float(STEP)   # (one float32 rounding, as the program's +=)
                r.render_restir(None, c, W, H, f, want_rgb=False, want_grid=False)
                r.history_advance(c, W, H)
            rgb = r.history_denoise(tone=tone)
            assert 0.0 < rgb.mean() < 1.0 and r.history_frames() == (4, 0)
            r.write_bmp(path)
            r.history_end()
            return path.read_bytes()
        finally:
            r.close()

    assert got.read_bytes() == python_file(restir.HISTORY_GATHER_BILINEAR, tmp_path / "py.bmp")
