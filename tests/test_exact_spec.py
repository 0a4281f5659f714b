"""The CPU ground the exact image's GPU tests stand on (tests/exact_spec.py over the oracle; no GPU): the census of lit
(pixel, light) pairs by the shadow ray's answer, for the frames of tests/test_gpu_exact.py, equals the counts recorded
when those tests were written -- so a change of a scene, a camera or the oracle that would leave a ray test without
occluded pairs is seen here first -- and the specification image has the properties its definition gives it."""
import numpy as np
import pytest

from romis_amd import _abi
from test_gpu_exact import NIGHT, assert_rays_matter, bits, spec_image

CENSUS = [(NIGHT, None, 33, 17, 32420, 12180), (NIGHT, None, 70, 37, 153228, 54740),
          ("monkey16", "toml", 33, 17, 159, 54), ("monkey16", "toml", 70, 37, 828, 293)]


@pytest.mark.parametrize("name,cam,w,h,visible,occluded", CENSUS)
def test_census_counts_are_the_recorded_ones(oracle, name, cam, w, h, visible, occluded):
    assert assert_rays_matter(oracle, name, cam, w, h) == (visible, occluded)


def test_the_specification_is_a_sum_of_non_negative_terms_from_plus_zero(oracle):
    """No -0 and no NaN anywhere (the argument that lets the kernel skip a ray whose shade is +-0), light where pairs are
    visible, none without lights, and tone mapping maps +0 to +0 and everything into [0, 1]."""
    w, h = 33, 17
    lin = spec_image(oracle, NIGHT, None, w, h, _abi.default_features(enable_tone_mapping=0))
    assert not np.isnan(lin).any() and not (bits(lin) == 0x80000000).any() and (lin >= 0).all() and (lin > 0).any()
    dark = spec_image(oracle, "dark", None, w, h, _abi.default_features(enable_tone_mapping=0))
    assert not bits(dark).any()
    toned = spec_image(oracle, NIGHT, None, w, h, _abi.default_features(gamma=2.2, exposure=0.7))
    assert not bits(toned[lin == 0]).any() and (toned > 0).any() and toned.min() >= 0.0 and toned.max() <= 1.0
