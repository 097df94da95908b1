"""The gradient guard's host side (fused_optim.GradGuard, csrc/gradguard.hip): argument
validation in Python, the grid bound, and the C entry points' argument checks.  No kernel is
launched here."""
import ctypes as C
import inspect
import math
import os

import pytest
import torch

from multimodal_alzheimer_amd import _lib
from multimodal_alzheimer_amd import fused_optim as F
from multimodal_alzheimer_amd.graph_step import GraphedTrainStep


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from multimodal_alzheimer_amd import _build
        _build.build()
    return _lib.load()


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


def test_grad_guard_validates_max_norm():
    for bad in (0, 0.0, -1.0, float("nan"), "x", True, torch.tensor(1.0)):
        with pytest.raises(ValueError):
            F.GradGuard(_params(), max_norm=bad)
    g = F.GradGuard(_params())
    assert g.max_norm == math.inf and g.skip_nonfinite is True
    assert F.GradGuard(_params(), max_norm=None, skip_nonfinite=False).skip_nonfinite is False
    g = F.GradGuard(_params(), max_norm=2)
    assert g.max_norm == 2.0
    g.set_max_norm(0.5)                       # before prepare(): kept for it
    assert g.max_norm == 0.5
    g.set_max_norm(None)
    assert g.max_norm == math.inf
    for bad in (0.0, -3, float("nan")):
        with pytest.raises(ValueError):
            g.set_max_norm(bad)
    assert g.max_norm == math.inf
    with pytest.raises(ValueError):
        F.GradGuard([torch.zeros(2), "not a tensor"])


def test_grad_guard_takes_an_optimizer_a_list_or_one_tensor():
    ps = _params()
    opt = torch.optim.Adam([{"params": ps[:1]}, {"params": ps[1:]}])
    assert [id(p) for p in F.GradGuard(opt).params] == [id(p) for p in ps]
    assert [id(p) for p in F.GradGuard(iter(ps)).params] == [id(p) for p in ps]
    assert F.GradGuard(ps[0]).params[0] is ps[0]


def test_state_slot_names():
    assert (F.MAX_NORM, F.SKIP_NONFINITE, F.SUMSQ, F.NORM, F.COEF, F.SKIP, F.STEPS, F.CLIPPED,
            F.SKIPPED, F.RESERVED) == tuple(range(10))
    assert F.STATE_SLOTS == 10 and len(F.STATE_NAMES) == 10
    assert F.STATE_NAMES[F.NORM] == "norm" and F.STATE_NAMES[F.SKIPPED] == "skipped"
    assert C.sizeof(_lib.GradJob) == 24


def test_guard_settings_of_the_captured_step():
    gs = F.guard_settings
    assert gs() is None
    assert gs(None, False, None) is None and gs(None, False, "") is None
    assert gs(1.5) == (1.5, False)
    assert gs(None, True) == (math.inf, True)
    assert gs(2, True) == (2.0, True)
    # the environment switch counts only with both arguments at their defaults
    assert gs(None, False, "0.25") == (0.25, True)
    assert gs(None, False, "inf") == (math.inf, True)
    assert gs(3.0, False, "0.25") == (3.0, False)
    assert gs(None, True, "0.25") == (math.inf, True)
    for bad in (0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            gs(bad)
    for bad in ("0", "-1", "nan", "on"):
        with pytest.raises(ValueError):
            gs(None, False, bad)


def test_graphed_train_step_rejects_bad_guard_arguments_before_any_gpu_work():
    sig = inspect.signature(GraphedTrainStep.__init__).parameters
    assert sig["clip_grad_norm"].default is None and sig["skip_nonfinite"].default is False
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_norm"):
            GraphedTrainStep(None, None, {}, clip_grad_norm=bad)


def test_grid_bound(lib):
    assert lib.mmad_grad_guard_blocks(1) == 1
    assert lib.mmad_grad_guard_blocks(1024) == 1024
    assert lib.mmad_grad_guard_blocks(5000) == 1024
    assert lib.mmad_grad_guard_blocks(0) == 0


def test_null_and_empty_calls_do_not_launch(lib):
    # (the pointer values are never dereferenced on the host)
    jobs, part, state, arr = 0x1000, 0x2000, 0x3000, 0x4000
    # nothing to do: OK whatever else is passed
    assert lib.mmad_grad_sumsq(0, None, 0, 0, None, None) == 0
    assert lib.mmad_grad_sumsq(-1, None, 5, 5, None, None) == 0
    assert lib.mmad_grad_scale(0, None, 0, None, None) == 0
    assert lib.mmad_adam_repack_guarded(0, None, None, 0, None, None, None) == 0
    # null pointers
    assert lib.mmad_grad_sumsq(2, None, 3, 3, part, None) == 1003
    assert lib.mmad_grad_sumsq(2, jobs, 3, 3, None, None) == 1003
    assert lib.mmad_grad_guard_finalize(3, None, state, None) == 1003
    assert lib.mmad_grad_guard_finalize(3, part, None, None) == 1003
    assert lib.mmad_grad_scale(2, None, 3, state, None) == 1003
    assert lib.mmad_grad_scale(2, jobs, 3, None, None) == 1003
    assert lib.mmad_adam_repack_guarded(2, jobs, None, 3, arr, None, None) == 1003
    assert lib.mmad_adam_repack_guarded(2, None, None, 3, arr, state, None) == 1003
    assert lib.mmad_adam_repack_guarded(2, jobs, None, 3, None, state, None) == 1003
    # work to do and no block to do it (or more blocks than `partials` has slots)
    assert lib.mmad_grad_sumsq(2, jobs, 3, 0, part, None) == 1001
    assert lib.mmad_grad_sumsq(2, jobs, 3, -4, part, None) == 1001
    assert lib.mmad_grad_sumsq(2, jobs, 5000, 1025, part, None) == 1001
    assert lib.mmad_grad_guard_finalize(-1, part, state, None) == 1001
    assert lib.mmad_grad_guard_finalize(1025, part, state, None) == 1001
