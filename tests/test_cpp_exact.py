"""tests/cpp/exact_image.cpp -- romis::renderExact and Renderer::renderExact / referenceSet / referenceClear / error of
include/romis_amd/restir.hpp -- compiles and links (CPU), and on the GPU writes the BMP the Python binding writes for the
exact image of the same scene."""
import os
import subprocess

import pytest

from romis_amd import _abi, restir, scene
from test_cpp_wrapper import build_cpp, write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "exact_image.cpp")
BIN = os.path.join(ROOT, "romis_amd", "_build", "exact_image")
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
    f = _abi.default_features(enable_tone_mapping=1, exposure=1.5, gamma=2.2)
    r = restir.Renderer(0)
    try:
        r.set_scene(sc)
        rgb = r.render_exact(cam, W, H, f)
        assert 0.0 < rgb.mean() < 1.0
        want = tmp_path / "py.bmp"
        r.write_bmp(want)
        assert got.read_bytes() == want.read_bytes()
    finally:
        r.close()
