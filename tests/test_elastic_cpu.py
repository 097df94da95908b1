"""Host side of the elastic deformation (multimodal_alzheimer_amd.augment): the two settings
are validated when the augmenter is built, the fold guard ``AugmentConfig.check_elastic`` is
pure Python, and the two C entries refuse bad arguments before anything is launched.  No
kernel is launched here."""
import math
import os
import re

import pytest

from multimodal_alzheimer_amd import _lib, augment


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from multimodal_alzheimer_amd import _build
        _build.build()
    return _lib.load()


# ------------------------------------------------------------------------------ 1. settings
@pytest.mark.parametrize("bad", [
    {"elastic_vox": -0.5},
    {"elastic_vox": [1.0, -1.0, 1.0]},
    {"elastic_vox": [1.0, 1.0]},
    {"elastic_grid": 1},
    {"elastic_grid": 13},
    {"elastic_grid": [7, 1, 7]},
    {"elastic_grid": [7, 7, 13]},
    {"elastic_grid": 7.5},
    {"elastic_grid": [7, 6.0, 7]},
    {"elastic_grid": [7, 7]},
])
def test_bad_elastic_settings_raise_value_error(bad):
    with pytest.raises(ValueError):
        augment.VolumeAugmenter(**bad)


def test_defaults_mean_off_and_settings_are_kept():
    assert "elastic_vox" in augment.CONFIG_KEYS and "elastic_grid" in augment.CONFIG_KEYS
    off = augment.VolumeAugmenter()
    assert off.cfg.elastic_vox == (0.0, 0.0, 0.0) and off.cfg.elastic_grid == (7, 7, 7)
    assert not off.cfg.elastic and off.lattice is None
    assert not augment.AugmentConfig(elastic_grid=[2, 5, 12]).elastic
    on = augment.VolumeAugmenter(elastic_vox=[0.0, 1.5, 0.0], elastic_grid=[2, 5, 12]).cfg
    assert on.elastic and on.elastic_vox == (0.0, 1.5, 0.0) and on.elastic_grid == (2, 5, 12)
    assert augment.AugmentConfig(elastic_vox=2).elastic_vox == (2.0, 2.0, 2.0)
    with pytest.raises(ValueError, match="gamma"):           # unknown keys keep raising
        augment.VolumeAugmenter(elastic_vox=1.0, gamma=[0.8, 1.2])


# ---------------------------------------------------------------------------- 2. fold guard
def cap_by_hand(shape, grid, scale_lo):
    """scale_lo / (2 sqrt(3 sum_j 1 / s_j^2)), s_j = size_j / (G_j - 1)"""
    inv = sum(((g - 1) / n) ** 2 for g, n in zip(grid, shape))
    return scale_lo / (2.0 * math.sqrt(3.0 * inv))


@pytest.mark.parametrize("shape, grid, scale", [
    ((91, 109, 91), 7, (1.0, 1.0)),
    ((91, 109, 91), 7, (0.8, 1.1)),
    ((24, 20, 28), (4, 3, 5), (0.8, 1.1)),
    ((24, 20, 28), (12, 2, 3), (1.0, 1.2)),
])
def test_check_elastic_passes_under_the_cap_and_raises_at_it(shape, grid, scale):
    grid3 = (grid,) * 3 if isinstance(grid, int) else grid
    cap = cap_by_hand(shape, grid3, scale[0])
    assert augment.AugmentConfig(elastic_grid=grid, scale=scale).elastic_cap(shape) == \
        pytest.approx(cap, rel=1e-14)
    augment.AugmentConfig(elastic_vox=0.999 * cap, elastic_grid=grid, scale=scale) \
        .check_elastic(shape)
    for vox in (cap, 1.001 * cap, 3.0 * cap):
        with pytest.raises(ValueError) as e:
            augment.AugmentConfig(elastic_vox=vox, elastic_grid=grid, scale=scale) \
                .check_elastic(shape)
        # the message carries the admissible value
        assert float(re.search(r"below (\d+\.\d+)", str(e.value)).group(1)) == \
            pytest.approx(cap, abs=1e-4)


def test_cap_value_scaling_and_anisotropic_bounds():
    cfg = augment.AugmentConfig(elastic_grid=7)
    assert cfg.elastic_cap((91, 109, 91)) == pytest.approx(2.67, abs=0.005)
    half = augment.AugmentConfig(elastic_grid=7, scale=(0.5, 1.0))
    assert half.elastic_cap((91, 109, 91)) == pytest.approx(0.5 * cfg.elastic_cap((91, 109, 91)),
                                                           rel=1e-14)
    # beta depends on sum m_i^2 only: one axis may take sqrt(3) times the isotropic cap
    cap = cfg.elastic_cap((91, 109, 91))
    augment.AugmentConfig(elastic_vox=[0.0, 0.0, 0.999 * math.sqrt(3.0) * cap]) \
        .check_elastic((91, 109, 91))
    with pytest.raises(ValueError):
        augment.AugmentConfig(elastic_vox=[0.0, 0.0, 1.001 * math.sqrt(3.0) * cap]) \
            .check_elastic((91, 109, 91))
    augment.AugmentConfig().check_elastic((91, 109, 91))       # off: nothing to refuse


# ----------------------------------------------------------------------------- 3. C entries
def test_bad_arguments_are_rejected_without_launching(lib):
    # the pointer values are never dereferenced here
    seed, lat, x, th, out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    assert lib.mmad_elastic_draw(2, 7, 7, 7, 1.0, 1.0, 1.0, None, lat, None) == 1003
    assert lib.mmad_elastic_draw(2, 7, 7, 7, 1.0, 1.0, 1.0, seed, None, None) == 1003
    for g in ((1, 7, 7), (7, 13, 7), (7, 7, 0), (7, 7, 13)):
        assert lib.mmad_elastic_draw(2, *g, 1.0, 1.0, 1.0, seed, lat, None) == 1001
        assert lib.mmad_deform_resample3d(2, 8, 8, 8, x, th, *g, lat, None, 0, 0, out,
                                          None) == 1001
    for m in ((-1.0, 1.0, 1.0), (1.0, -0.5, 1.0), (1.0, 1.0, float("nan"))):
        assert lib.mmad_elastic_draw(2, 7, 7, 7, *m, seed, lat, None) == 1001
    assert lib.mmad_elastic_draw(0, 7, 7, 7, 1.0, 1.0, 1.0, seed, lat, None) == 1001
    for args in ((None, th, lat, out), (x, None, lat, out), (x, th, None, out),
                 (x, th, lat, None)):
        xx, tt, ll, oo = args
        assert lib.mmad_deform_resample3d(2, 8, 8, 8, xx, tt, 7, 7, 7, ll, None, 0, 0, oo,
                                          None) == 1003
    assert lib.mmad_deform_resample3d(2, 8, 0, 8, x, th, 7, 7, 7, lat, None, 0, 0, out,
                                      None) == 1001
    assert lib.mmad_deform_resample3d(2, 8, 8, 8, x, th, 7, 7, 7, lat, None, 0, 0, x,
                                      None) == _lib.EUNSUPPORTED      # in place
    assert lib.mmad_deform_resample3d(1, 2048, 1024, 1024, x, th, 7, 7, 7, lat, None, 0, 0, out,
                                      None) == _lib.EUNSUPPORTED      # d * h * w >= 2^31
