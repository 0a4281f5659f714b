"""tests/cpp/denoise_lum_frames.cpp -- Renderer::denoiseLum and romis::DenoiseLumParams of include/romis_amd/restir.hpp --
compiles and links (CPU), and on the GPU checks a filtered frame against restir_denoise_lum_host and writes the BMP the
Python binding writes for the same four accumulated frames, filtered by their own variance and tone mapped."""
import os
import subprocess

import pytest

from romis_amd import _abi, restir, scene
from test_cpp_wrapper import build_cpp, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "denoise_lum_frames.cpp")
BIN = os.path.join(ROOT, "romis_amd", "_build", "denoise_lum_frames")
NAME = "nightclub_128pt"


def test_example_compiles_and_links():
    assert os.path.exists(build_cpp(SRC, BIN))


@pytest.mark.gpu
def test_cpp_example_writes_the_python_bindings_file(tmp_path):
    W, H = 70, 37
    sc, cam = scene.bench_scene(NAME), scene.camera_for(NAME, W, H)
    write_scene(tmp_path / "s.bin", sc, cam)
    got = tmp_path / "cpp.bmp"
    subprocess.check_call([build_cpp(SRC, BIN), str(tmp_path / "s.bin"), str(got), str(W), str(H)], timeout=120)
    f = _abi.default_features(num_samples_in_reservoir=1, initial_light_samples=32, num_neighbours_to_sample=5,
                              spatial_resample_radius=10, spatial_reuse=1, temporal_reuse=0, spatial_resampling_passes=1,
                              enable_tone_mapping=0)
    tone = _abi.default_features(enable_tone_mapping=1, exposure=1.5, gamma=2.2)
    r = restir.Renderer(0)
    try:
        r.set_scene(sc)
        r.set_seed(_abi.RESTIR_DEFAULT_SEED, 0)
        r.accum_begin(True)
        for _ in range(4):
            r.render_restir(None, cam, W, H, f, want_rgb=False, want_grid=False)
            r.accum_add()
        rgb = r.denoise_lum(cam, W, H, params=restir.denoise_lum_params(variance_source=_abi.RESTIR_DENOISE_VAR_ACCUM), tone=tone)
        assert 0.0 < rgb.mean() < 1.0
        want = tmp_path / "py.bmp"
        r.write_bmp(want)
        assert got.read_bytes() == want.read_bytes()
        r.accum_end()
    finally:
        r.close()
