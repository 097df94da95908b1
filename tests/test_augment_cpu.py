"""Host side of the device augmentation (multimodal_alzheimer_amd.augment): settings are
validated when the augmenter is built, there is no CPU path, and ``hparams['augment']`` is
the only thing that changes a model -- no new state-dict keys, and the key travels in the
checkpoint's hyper-parameters.  No kernel is launched here."""
import pytest
import torch

import multimodal_alzheimer_amd as M
from multimodal_alzheimer_amd import _lib, augment
from tests import _golden as G

CFG = {"flip_p": [0.5, 0.0, 0.5], "rotate_deg": [10.0, 10.0, 10.0], "scale": [0.95, 1.05],
       "translate_vox": [4.0, 4.0, 4.0], "gain": [0.9, 1.1], "bias": [-0.1, 0.1],
       "padding": "border"}


@pytest.mark.parametrize("bad", [
    {"flip_p": [-0.1, 0.0, 0.0]},
    {"flip_p": [0.0, 1.5, 0.0]},
    {"flip_p": [0.5, 0.5]},
    {"scale": [1.1, 0.9]},
    {"scale": [0.0, 1.0]},
    {"rotate_deg": [-5.0, 0.0, 0.0]},
    {"translate_vox": -1.0},
    {"gain": [1.2, 0.8]},
    {"bias": {"mri": [0.0, 0.1]}},
    {"padding": "reflection"},
])
def test_bad_settings_raise_value_error(bad):
    with pytest.raises(ValueError):
        augment.VolumeAugmenter(**bad)


def test_unknown_key_raises():
    with pytest.raises(ValueError, match="gamma"):
        augment.VolumeAugmenter(gamma=[0.8, 1.2])


def test_defaults_mean_off_and_settings_are_kept():
    off = augment.VolumeAugmenter().cfg
    assert off.flip_p == (0.0, 0.0, 0.0) and off.rotate_deg == (0.0, 0.0, 0.0)
    assert off.scale == (1.0, 1.0) and off.translate_vox == (0.0, 0.0, 0.0)
    assert off.gain == (1.0, 1.0) and off.bias == (0.0, 0.0) and not off.intensity
    assert off.padding == "zeros"
    on = augment.VolumeAugmenter(**CFG).cfg
    assert on.intensity and on.padding == "border" and on.flip_p == (0.5, 0.0, 0.5)
    c = on.struct(2)
    assert c.nmod == 2 and list(c.gain_lo)[:2] == [0.9, 0.9] and list(c.bias_hi)[:2] == [0.1, 0.1]
    assert abs(c.rot_max[0] - 0.17453292519943295) < 1e-15
    per_key = augment.AugmentConfig(gain={"mri": [0.9, 1.1], "pet1451": [1.0, 1.0]}).struct(2)
    assert list(per_key.gain_lo)[:2] == [0.9, 1.0] and list(per_key.gain_hi)[:2] == [1.1, 1.0]


def test_cpu_tensors_raise():
    x = torch.zeros((1, 4, 4, 4), dtype=torch.float64)
    theta = torch.eye(3, 4, dtype=torch.float64)[None]
    with pytest.raises(_lib.MMADError):
        augment.resample(x, theta)
    with pytest.raises(_lib.MMADError):
        augment.draw(CFG, 2, (4, 4, 4), "cpu")
    with pytest.raises(_lib.MMADError):
        augment.VolumeAugmenter(**CFG)({"mri": x, "label": torch.zeros(1, dtype=torch.long)})


def test_batch_without_volumes_passes_through():
    batch = {"label": torch.zeros(2, dtype=torch.long), "tabular": torch.zeros(2, 9)}
    assert augment.VolumeAugmenter(**CFG)(batch) is batch


def test_model_without_the_key_is_unchanged():
    plain = M.Anat_CNN(G.anat_hparams(10))
    with_key = M.Anat_CNN(G.anat_hparams(10, augment=CFG))
    assert plain.augmenter is None and "augment" not in plain.hparams
    assert isinstance(with_key.augmenter, augment.VolumeAugmenter)
    assert list(plain.state_dict()) == list(with_key.state_dict())
    batch = {"mri": torch.zeros((1, 4, 4, 4), dtype=torch.float64)}
    assert plain.augment_batch(batch, "train") is batch
    assert with_key.augment_batch(batch, "val") is batch        # only 'train' augments
    assert with_key.on_after_batch_transfer(batch) is batch     # the hook never augments


def test_key_survives_checkpoint_round_trip(tmp_path):
    m = M.Anat_CNN(G.anat_hparams(10, augment=CFG))
    assert m.hparams["augment"] == CFG
    p = str(tmp_path / "aug.ckpt")
    m.save_checkpoint(p)
    back = M.Anat_CNN.load_from_checkpoint(p)
    assert back.hparams["augment"] == CFG
    assert back.augmenter is not None and back.augmenter.cfg.padding == "border"
    assert back.augmenter.cfg.scale == (0.95, 1.05)
    assert list(back.state_dict()) == list(m.state_dict())
