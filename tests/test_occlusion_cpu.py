"""explain.occlusion without a device: the window arithmetic of ``occlusion_windows`` against a
brute-force enumeration, the replay count and every argument check (all of which run before
the model or a kernel is touched)."""
import itertools
import math

import numpy as np
import pytest
import torch

from multimodal_alzheimer_amd import classifiers, explain

GEOMS = [((9, 10, 13), (4, 4, 5), (3, 4, 4)),      # odd W, a clamped last window, overlap
         ((9, 10, 13), (9, 10, 13), None),         # patch == size: one window
         ((5, 6, 7), (3, 2, 4), (1, 1, 1)),        # stride 1
         ((8, 8, 8), (4, 4, 4), None),             # patch == stride, exact tiling
         ((16, 16, 16), 8, 8)]


def _brute_starts(s, p, t):
    """window starts of one axis: step by t until a full window no longer fits, then one last
    window that ends at the extent"""
    out, x = [], 0
    while x + p < s:
        out.append(x)
        x += t
    out.append(s - p)
    return out


@pytest.mark.parametrize("size,patch,stride", GEOMS)
def test_windows_match_a_brute_force_enumeration(size, patch, stride):
    w = explain.occlusion_windows(size, patch, stride)
    p3 = (patch,) * 3 if isinstance(patch, int) else tuple(patch)
    t3 = p3 if stride is None else ((stride,) * 3 if isinstance(stride, int) else tuple(stride))
    assert w["patch"] == p3 and w["stride"] == t3
    cover = np.zeros(size, dtype=np.int64)
    for a in range(3):
        starts = w["starts"][a]
        assert starts == _brute_starts(size[a], p3[a], t3[a])
        assert len(starts) == max(1, math.ceil((size[a] - p3[a]) / t3[a]) + 1)
        assert starts[-1] + p3[a] == size[a]                  # the last window ends at the extent
        assert all(0 <= s and s + p3[a] <= size[a] for s in starts)   # every window is full size
        assert starts == sorted(starts) and len(set(starts)) == len(starts)
    n = [len(s) for s in w["starts"]]
    assert explain.window_count(w) == n[0] * n[1] * n[2]
    # j = (iz * n_h + iy) * n_w + ix is the row-major order of the three start lists
    for j, (iz, iy, ix) in enumerate(itertools.product(*[range(k) for k in n])):
        assert j == (iz * n[1] + iy) * n[2] + ix
        z, y, x = w["starts"][0][iz], w["starts"][1][iy], w["starts"][2][ix]
        cover[z:z + p3[0], y:y + p3[1], x:x + p3[2]] += 1
    assert cover.min() >= 1                                   # every voxel is covered
    if t3 == p3 and all(s % p == 0 for s, p in zip(size, p3)):
        assert cover.max() == 1


def test_issue_geometry_has_27_windows():
    w = explain.occlusion_windows((9, 10, 13), (4, 4, 5), (3, 4, 4))
    assert [len(s) for s in w["starts"]] == [3, 3, 3]
    assert w["starts"] == ([0, 3, 5], [0, 4, 6], [0, 4, 8])


@pytest.mark.parametrize("p,m,n", [(27, 3, 9), (27, 4, 7), (27, 1, 27), (27, 64, 1), (1, 1, 1)])
def test_replay_count(p, m, n):
    assert explain.replay_count(p, m) == n == math.ceil(p / m)


def _batch(b=2, shape=(8, 8, 8), keys=("mri", "pet1451")):
    return {k: torch.zeros((b,) + shape, dtype=torch.float64) for k in keys}


@pytest.mark.parametrize("kw", [
    {"patch": 0}, {"patch": 9}, {"patch": (4, 4)}, {"patch": (4, 4, 9)}, {"patch": 2.5},
    {"patch": True}, {"patch": 4, "stride": 0}, {"patch": 4, "stride": 5},
    {"patch": 4, "stride": (4, 4, 5)}, {"patch": 4, "stride": "4"},
    {"score": "softmax"}, {"score": None},
    {"fill": "median"}, {"fill": None}, {"fill": {"mri": 0.0}}, {"fill": {"mri": 0.0,
                                                                           "pet1451": "x"}},
    {"keys": ("ct",)}, {"keys": ()}, {"keys": ("mri", "mri")},
    {"windows_per_replay": 0}, {"windows_per_replay": 1.5}, {"windows_per_replay": 40000},
    {"graph": "yes"},
])
def test_wrong_arguments_raise_before_the_model_is_touched(kw):
    kw = {"patch": 4, **kw}
    with pytest.raises(ValueError):
        explain.occlusion(None, _batch(), **kw)      # model None: nothing may reach it


def test_a_key_missing_from_the_batch_raises():
    with pytest.raises(ValueError):
        explain.occlusion(None, _batch(keys=("mri",)), patch=4, keys=("pet1451",))
    with pytest.raises(ValueError):
        explain.occlusion(None, {"label": torch.zeros(2, dtype=torch.int64)}, patch=4)
    with pytest.raises(ValueError):                  # occluded volumes of different extents
        explain.occlusion(None, {"mri": torch.zeros(2, 8, 8, 8),
                                 "pet1451": torch.zeros(2, 8, 8, 9)}, patch=4)


def test_the_plan_resolves_defaults():
    keys, w, spec, m, capture = explain._occlusion_plan(
        None, _batch(b=3), 4, None, "mean", "prob", None, None, None)
    assert keys == ["mri", "pet1451"] and m == 2 and capture
    assert spec == {"mri": "mean", "pet1451": "mean"}
    assert w["stride"] == (4, 4, 4) and explain.window_count(w) == 8
    keys, _, spec, m, capture = explain._occlusion_plan(
        None, _batch(b=16), 4, 2, {"mri": 1, "pet1451": "mean"}, "logit", "mri", 5, False)
    assert keys == ["mri"] and spec == {"mri": 1.0} and m == 5 and not capture
    assert explain._occlusion_plan(None, _batch(b=16), 4, 2, 0.0, "logit", None, None,
                                   None)[3] == 1


@pytest.mark.parametrize("cls", [classifiers.Tabular_MRT_Model, classifiers.PET_TABULAR_CNN,
                                 classifiers.All_Modalities_Fusion])
def test_graph_true_on_a_tabpfn_stage_class_raises(cls):
    m = object.__new__(cls)                          # the type decides; no TabPFN is loaded
    assert explain._host_forward(m)
    with pytest.raises(ValueError, match="captured"):
        explain.occlusion(m, _batch(), patch=4, graph=True)
    assert explain._occlusion_plan(m, _batch(), 4, None, 0.0, "logit", None, None, None)[4] is False
    assert not explain._host_forward(object.__new__(classifiers.Anat_CNN))
