"""The gradient guard on the MI355X (csrc/gradguard.hip, mmad_adam_repack_guarded in
csrc/adam.hip, fused_optim.GradGuard / clip_grad_norm_, GraphedTrainStep(clip_grad_norm=,
skip_nonfinite=)): the global norm in double, torch's clip coefficient, a guarded Adam that is
torch's Adam on clipped gradients bit for bit, a non-finite step skipped without a trace, and
captured steps that equal their eager twins.

Parameters: tests/test_adam_repack_gpu.py's SHAPES plus one (4099,) parameter whose gradient is
a view at storage offset 1 (4-byte aligned only: a misaligned head and tail)."""
import copy
import math

import numpy as np
import pytest
import torch

import multimodal_alzheimer_amd as M
from multimodal_alzheimer_amd import fused_optim as F
from multimodal_alzheimer_amd import layers as Lyr
from multimodal_alzheimer_amd import volume_ops as V
from multimodal_alzheimer_amd.graph_step import GraphedTrainStep
from tests import _poison
from tests.test_adam_repack_gpu import SHAPES, _batch, _hparams, _opt

pytestmark = pytest.mark.gpu

ODD = 4099
ALL_SHAPES = SHAPES + [(ODD,)]
NUMEL = sum(int(np.prod(s)) for s in ALL_SHAPES)


def _params(seed, shapes=ALL_SHAPES):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device="cuda", generator=g) * 0.1) for s in shapes]


def _grads(params, seed):
    """random gradients; the (4099,) one a view one element into its storage"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in params:
        if tuple(p.shape) == (ODD,):
            buf = torch.randn(ODD + 1, device="cuda", generator=g) * 1e-2
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        else:
            p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-2


def _ref_sumsq(params):
    return sum((p.grad.double() ** 2).sum() for p in params if p.grad is not None)


def _coef_ref(max_norm, norm):
    """clip_grad_norm_'s coefficient in float32 from the float32-rounded norm"""
    c = torch.tensor(max_norm, dtype=torch.float32) / (norm.detach().cpu().to(torch.float32) + 1e-6)
    return torch.clamp(c, max=1.0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


# ------------------------------------------------------------------ 1. norm
def test_norm_is_a_double_sum_and_reproducible():
    assert NUMEL < 10 ** 6
    params = _params(1)
    _grads(params, 2)
    guard = F.GradGuard(params)
    guard.measure()
    first = guard.state.clone()
    guard.measure()
    second = guard.state.clone()
    ref = _ref_sumsq(params).sqrt()
    rel = abs(float(first[F.NORM]) - float(ref)) / float(ref)
    print(f"norm {float(first[F.NORM])!r} ref {float(ref)!r} rel {rel:.3e}")
    assert rel <= 1e-10
    assert torch.equal(_bits(first[F.SUMSQ:F.SKIP + 1]), _bits(second[F.SUMSQ:F.SKIP + 1]))
    assert float(first[F.NORM]) == math.sqrt(float(first[F.SUMSQ]))
    assert guard.nblocks == guard.chunks == sum(-(-int(np.prod(s)) // 4096) for s in ALL_SHAPES)
    # parameters without a gradient are left out
    params[0].grad = None
    guard.measure()
    ref = _ref_sumsq(params).sqrt()
    assert abs(float(guard.norm) - float(ref)) / float(ref) <= 1e-10


def test_norm_with_more_chunks_than_blocks():
    """1026 chunks on 1024 blocks: two blocks take a second chunk (the grid-stride walk), in
    the sum and in the in-place scale.  Bound: n * 2^-53 for the sum of n non-negative doubles,
    n = 4.2e6 -> 4.7e-10 (halved by the square root)."""
    n = 1024 * 4096 + 5000
    gen = torch.Generator(device="cuda").manual_seed(7)
    p = torch.nn.Parameter(torch.zeros(n - 3000, device="cuda"))
    q = torch.nn.Parameter(torch.zeros(3000, device="cuda"))
    p.grad = torch.randn(n - 2999, device="cuda", generator=gen)[1:]
    q.grad = torch.randn(3000, device="cuda", generator=gen)
    guard = F.GradGuard([p, q], max_norm=100.0)
    before = [p.grad.clone(), q.grad.clone()]
    norm = F.clip_grad_norm_([p, q], 100.0, guard=guard)
    assert guard.chunks == 1026 and guard.nblocks == 1024
    ref = (before[0].double() ** 2).sum().add((before[1].double() ** 2).sum()).sqrt()
    rel = abs(float(norm) - float(ref)) / float(ref)
    print(f"norm {float(norm)!r} ref {float(ref)!r} rel {rel:.3e}")
    assert rel <= n * 2.0 ** -53
    coef = guard.state[F.COEF].to(torch.float32)
    assert float(coef) < 1.0
    assert torch.equal(_bits(p.grad), _bits(before[0] * coef))
    assert torch.equal(_bits(q.grad), _bits(before[1] * coef))


def test_norm_under_poisoned_allocations():
    """partials, the job table and every other torch.empty buffer hold NaN / 1 (fill A) or
    zeros (fill B) before the launches: equal results, so every partial that is read was
    written, and nothing written outside."""
    params = _params(1)
    _grads(params, 2)
    plain = F.GradGuard(params, max_norm=1.0)
    plain.measure()
    got = []
    for fill in ("A", "B"):
        with _poison.poisoned(fill) as ps:
            guard = F.GradGuard(params, max_norm=1.0)
            guard.measure()
            got.append(guard.state.clone())
            ps.check()
            assert len(ps.records) >= 2
    assert torch.equal(_bits(got[0]), _bits(got[1]))
    assert torch.equal(_bits(got[0]), _bits(plain.state))
    assert torch.isfinite(got[0]).all()


# ------------------------------------------------------------------ 2. coefficient
def test_coefficient_follows_torch_clip_grad_norm():
    params = _params(1)
    _grads(params, 3)
    guard = F.GradGuard(params)                       # max_norm=None: measure only
    guard.measure()
    st = guard.stats()
    assert st["coef"] == 1.0 and st["steps"] == 1 and st["clipped"] == 0 and st["skip"] == 0
    assert st["max_norm"] == float("inf") and st["skip_nonfinite"] == 1
    norm = st["norm"]
    for k, (factor, clips) in enumerate(((0.5, True), (2.0, False))):
        guard.set_max_norm(factor * norm)
        guard.measure()
        got = float(guard.coef)
        assert got == float(np.float32(got))          # a float32, widened
        exp = _coef_ref(factor * norm, guard.norm)
        ulp = float(np.spacing(np.float32(exp.item())))
        print(f"max_norm {factor} x norm: coef {got!r} torch {exp.item()!r}")
        assert abs(got - exp.item()) <= ulp
        assert (got < 1.0) == clips
        if not clips:
            assert got == 1.0
        st = guard.stats()
        assert st["steps"] == 2 + k and st["clipped"] == 1 and st["skipped"] == 0
    assert guard.norm.dim() == 0 and guard.norm.is_cuda and guard.coef.dim() == 0


# ------------------------------------------------------------------ 3. guarded Adam
def test_guarded_adam_is_torch_adam_on_clipped_gradients():
    """side A: g.mul_(coef), torch's fused step; side B: AdamRepack(guard=...); side C: the
    unguarded AdamRepack on A's gradients (the raw ones whenever the threshold does not clip).
    The gradient norm is ~3.7: max_norm 1.0 clips, 1000 does not."""
    pa, pb, pc = _params(1), _params(1), _params(1)
    oa, ob, oc = _opt(pa), _opt(pb), _opt(pc)
    for ps, o in ((pa, oa), (pb, ob), (pc, oc)):
        _grads(ps, 2)
        o.step()                                    # state initialised by torch
    guard = F.GradGuard(ob, skip_nonfinite=True)
    fused = F.AdamRepack(ob, guard=guard)
    plain = F.AdamRepack(oc)
    for it, max_norm in enumerate((1000.0, 1.0, 1000.0, 1.0)):
        for ps in (pa, pb, pc):
            _grads(ps, 10 + it)
        raw = [p.grad.clone() for p in pb]
        guard.set_max_norm(max_norm)
        fused.step()
        coef = guard.state[F.COEF].to(torch.float32)
        for ps in (pa, pc):
            for p in ps:
                p.grad.mul_(coef)
        oa.step()
        plain.step()
        torch.cuda.synchronize()
        assert (float(coef) < 1.0) == (max_norm == 1.0)
        if max_norm != 1.0:
            assert float(coef) == 1.0
            assert all(torch.equal(p.grad, r) for p, r in zip(pc, raw))
        for a, b, c, r in zip(pa, pb, pc, raw):
            assert torch.equal(b.grad, r)            # .grad keeps the unclipped gradient
            sa, sb, sc = oa.state[a], ob.state[b], oc.state[c]
            assert torch.equal(a, b), (it, tuple(a.shape), (a - b).abs().max().item())
            assert torch.equal(a, c), (it, tuple(a.shape))
            for f in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(sa[f], sb[f]), (it, f, tuple(a.shape))
                assert torch.equal(sa[f], sc[f]), (it, f, tuple(a.shape))
    assert float(ob.state[pb[0]]["step"]) == 5.0
    assert int(fused.arrivals.abs().sum()) == 0
    st = guard.stats()
    assert (st["steps"], st["clipped"], st["skipped"]) == (4, 2, 0)


# ------------------------------------------------------------------ 4. / 5. packed layouts
def _conv_stack(seed):
    torch.manual_seed(seed)
    convs = torch.nn.Sequential(
        Lyr.Conv3d(1, 64, 7, stride=2, padding=3, bias=False),       # the unfolded stem
        Lyr.Conv3d(64, 64, 3, padding=1, bias=False),
        Lyr.Conv3d(64, 128, 3, stride=2, padding=1, bias=False),
        Lyr.Conv3d(128, 128, 3, padding=2, dilation=2, bias=False),
        Lyr.Conv3d(128, 256, 1, stride=2, bias=False)).cuda()
    for c in convs:
        c.compute_dtype = torch.bfloat16
    V.prepack(convs)
    plan = convs._mmad_pack_plan
    assert plan.nduals >= 2 and len(plan.unfolds) == 1
    return convs, plan


def _packed(plan):
    return [tuple(None if b is None else b.clone() for b in e[2:4]) for e in plan.entries]


def _same_packed(got, ref):
    for g, r in zip(got, ref):
        for a, b in zip(g, r):
            assert (a is None) == (b is None)
            assert a is None or torch.equal(a, b)


def test_guarded_step_writes_both_packed_layouts():
    convs, plan = _conv_stack(3)
    params = list(convs.parameters())
    opt = torch.optim.Adam([{"params": params, "lr": torch.tensor(1e-2, device="cuda")}],
                           fused=True, capturable=True)
    _grads(params, 5)
    opt.step()
    guard = F.GradGuard(opt, max_norm=0.5)
    fused = F.AdamRepack(opt, [plan], guard=guard)
    before = [p.detach().clone() for p in params]
    _grads(params, 6)
    fused.step()
    torch.cuda.synchronize()
    assert float(guard.coef) < 1.0
    assert all(not torch.equal(p, b) for p, b in zip(params, before))
    got = _packed(plan)
    plan.run_duals()                                     # the same weights, packed separately
    torch.cuda.synchronize()
    _same_packed(got, _packed(plan))


BAD = {"inf_in_repacked_conv": (1, 12345, float("inf")),
       "nan_last_of_1000": (-2, 999, float("nan")),
       "neg_inf_in_misaligned_view": (-1, 1, float("-inf"))}


@pytest.mark.parametrize("case", sorted(BAD))
def test_nonfinite_step_is_skipped_fully(case):
    """One bad value anywhere in the gradients: nothing the optimizer owns changes, the next
    finite step continues as if the bad one had never been asked for, and with
    skip_nonfinite=False the same gradients raise no skip.  (Data values, not faults.)"""
    which, at, value = BAD[case]
    convs, plan = _conv_stack(3)
    extra = _params(4, [(7, 5), (1000,), (ODD,)])
    pb = list(convs.parameters()) + extra
    pa = [torch.nn.Parameter(p.detach().clone()) for p in pb]

    def opt(ps):
        return torch.optim.Adam(
            [{"params": ps[0::2], "lr": torch.tensor(1e-2, device="cuda")},
             {"params": ps[1::2], "lr": torch.tensor(3e-3, device="cuda"), "weight_decay": 0.01}],
            fused=True, capturable=True)
    oa, ob = opt(pa), opt(pb)
    guard = F.GradGuard(ob, max_norm=1.0, skip_nonfinite=True)
    fused = F.AdamRepack(ob, [plan], guard=guard)

    def both(seed):
        _grads(pa, seed)
        _grads(pb, seed)

    both(20)
    oa.step()
    ob.step()                                        # state initialised by torch in both
    both(21)
    fused.step()                                     # a first guarded step: packed copies current
    for p in pa:
        p.grad.mul_(guard.state[F.COEF].to(torch.float32))
    oa.step()
    torch.cuda.synchronize()

    def snapshot():
        out = [p.detach().clone() for p in pb]
        for p in pb:
            out += [ob.state[p][f].clone() for f in ("exp_avg", "exp_avg_sq", "step")]
        for pair in _packed(plan):
            out += [b for b in pair if b is not None]
        out.append(fused.arrivals.clone())
        return out

    snap = snapshot()
    skipped = guard.stats()["skipped"]
    _grads(pb, 22)
    assert tuple(pb[which].shape) in ((64, 64, 3, 3, 3), (1000,), (ODD,))
    pb[which].grad.view(-1)[at] = value
    guard.set_skip_nonfinite(False)
    guard.measure()                                  # measured only: nothing is applied
    assert float(guard.skip) == 0.0 and not np.isfinite(float(guard.state[F.SUMSQ]))
    guard.set_skip_nonfinite(True)
    fused.step()
    torch.cuda.synchronize()
    st = guard.stats()
    assert st["skip"] == 1 and st["skipped"] == skipped + 1
    for was, now in zip(snap, snapshot()):
        assert torch.equal(was, now)
    both(23)                                         # finite again: torch continues from the same state
    fused.step()
    coef = guard.state[F.COEF].to(torch.float32)
    for p in pa:
        p.grad.mul_(coef)
    oa.step()
    torch.cuda.synchronize()
    assert guard.stats()["skip"] == 0 and guard.stats()["skipped"] == skipped + 1
    for a, b in zip(pa, pb):
        assert torch.equal(a, b), tuple(a.shape)
        for f in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(oa.state[a][f], ob.state[b][f]), (f, tuple(a.shape))
    got = _packed(plan)
    plan.run_duals()
    torch.cuda.synchronize()
    _same_packed(got, _packed(plan))
    assert int(fused.arrivals.abs().sum()) == 0


# ------------------------------------------------------------------ 6. eager form
def test_eager_clip_grad_norm_scales_in_place():
    params = _params(1)
    _grads(params, 8)
    before = [p.grad.clone() for p in params]
    guard = F.GradGuard(params, skip_nonfinite=True)
    norm = F.clip_grad_norm_(params, 1.0, guard=guard)
    assert guard.max_norm == 1.0
    assert norm.data_ptr() == guard.state[F.NORM].data_ptr() and norm.dtype == torch.float64
    coef = guard.state[F.COEF].to(torch.float32)
    assert float(coef) < 1.0
    for p, g in zip(params, before):
        assert torch.equal(_bits(p.grad), _bits(g * coef)), tuple(p.shape)
    # the same call without a guard of one's own, against torch's (fp32 norm: close, not equal)
    for p, g in zip(params, before):
        p.grad = g.clone()
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for t, g in zip(twins, before):
        t.grad = g.clone()
    n1 = F.clip_grad_norm_(params, 1.0)
    n2 = torch.nn.utils.clip_grad_norm_(twins, 1.0)
    assert abs(float(n1) - float(n2)) <= 1e-5 * float(n2)
    for p, t in zip(params, twins):
        assert torch.allclose(p.grad, t.grad, rtol=1e-5, atol=0)
    # a skip pending: the gradients stay as they are, bad value included
    params[-2].grad[-1] = float("nan")
    held = [_bits(p.grad) for p in params]
    F.clip_grad_norm_(params, 1.0, guard=guard)
    assert float(guard.skip) == 1.0
    for p, h in zip(params, held):
        assert torch.equal(_bits(p.grad), h)


# ------------------------------------------------------------------ 7. - 10. captured steps
WARM, STEPS, SEED = 1, 4, 13


def _capturable(opt):
    for grp in opt.param_groups:
        grp["capturable"] = True
        grp["lr"] = torch.tensor(float(grp["lr"]), device="cuda")
    return opt


def _opt_state(opt):
    return {k: {f: v[f].clone() for f in ("step", "exp_avg", "exp_avg_sq")}
            for k, v in opt.state_dict()["state"].items()}


def _model_state(m):
    return {k: v.clone() for k, v in m.state_dict().items()}


class _Eager:
    """the eager twin of a guarded captured step: zero_grad, general_step, backward,
    fused_optim.clip_grad_norm_ (when a threshold is set), torch's optimizer.step()"""

    def __init__(self, model):
        self.model = model
        self.opt = _capturable(model.configure_optimizers())
        self.guard = F.GradGuard(self.opt, skip_nonfinite=False)

    def step(self, batch, clip=None, update=True):
        self.opt.zero_grad(set_to_none=True)
        out = self.model.general_step(batch, 0, "train")
        if update:
            out["loss"].backward()
            if clip is not None:
                F.clip_grad_norm_(self.guard.params, clip, guard=self.guard)
            self.opt.step()
        return out["loss"].detach().clone()


def _same_as(model, opt, ref_model_state, ref_opt_state):
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref_model_state[k]), k
    got = opt.state_dict()["state"]
    assert set(got) == set(ref_opt_state)
    for k, fields in ref_opt_state.items():
        for f, v in fields.items():
            assert torch.equal(got[k][f], v), (k, f)


@pytest.fixture(scope="module")
def twin():
    """Anat_CNN ResNet-10, bf16, batch 2 of 32^3; clip = half of the first step's norm.  The
    eager twin's WARM + STEPS clipped steps, then one unclipped step, computed once.

    The seed: this model ends in a ReLU over two logits, and from many initialisations both go
    negative for both scans within a step or two, after which every gradient is exactly zero --
    nothing left to clip or to overflow.  From seed 13 the gradient norm stays between 5.7 and
    11.3 over these steps (first norm 5.7, so half of it clips every step)."""
    torch.manual_seed(SEED)
    base = M.Anat_CNN(_hparams()).cuda()
    batches = [_batch(30 + i) for i in range(STEPS + 1)]
    probe = copy.deepcopy(base)
    probe.general_step(batches[0], 0, "train")["loss"].backward()
    g = F.GradGuard(list(probe.parameters()))
    g.measure()
    clip = 0.5 * float(g.norm)
    assert np.isfinite(clip) and clip > 0
    e = _Eager(copy.deepcopy(base))
    for _ in range(WARM):
        e.step(batches[0], clip)
    losses = [e.step(batches[i], clip) for i in range(STEPS)]
    torch.cuda.synchronize()
    st = e.guard.stats()
    assert st["clipped"] == st["steps"] == WARM + STEPS, st    # the threshold clips throughout
    out = {"base": base, "batches": batches, "clip": clip, "losses": losses,
           "model": _model_state(e.model), "opt": _opt_state(e.opt)}
    out["loss5"] = e.step(batches[STEPS])                     # unclipped
    torch.cuda.synchronize()
    out["model5"], out["opt5"] = _model_state(e.model), _opt_state(e.opt)
    return out


def test_captured_clipped_step_equals_eager_twin(twin, monkeypatch):
    monkeypatch.setattr(F, "GRAD_GUARD", None)
    b = copy.deepcopy(twin["base"])
    opt = b.configure_optimizers()
    gs = GraphedTrainStep(b, opt, twin["batches"][0], warmup=WARM, clip_grad_norm=twin["clip"])
    assert gs.guard is not None and gs.fused is not None and gs.fused.guard is gs.guard
    assert gs.guard.skip_nonfinite is False
    losses = [gs(twin["batches"][i])["loss"].clone() for i in range(STEPS)]
    torch.cuda.synchronize()
    for x, y in zip(twin["losses"], losses):
        assert torch.equal(x, y)
    _same_as(b, opt, twin["model"], twin["opt"])
    st = gs.guard.stats()
    assert st["clipped"] == st["steps"] == WARM + STEPS and st["skipped"] == 0
    # the threshold is read at replay time: no re-capture
    gs.guard.set_max_norm(float("inf"))
    loss5 = gs(twin["batches"][STEPS])["loss"].clone()
    torch.cuda.synchronize()
    assert torch.equal(loss5, twin["loss5"])
    _same_as(b, opt, twin["model5"], twin["opt5"])
    st = gs.guard.stats()
    assert st["coef"] == 1.0 and st["clipped"] == WARM + STEPS and st["steps"] == WARM + STEPS + 1


def test_captured_step_skips_an_overflowing_backward(twin, monkeypatch):
    """The static backward seed set to inf for one replay: the forward is finite, every
    gradient is not.  Weights, Adam state and step counters stay; BN running statistics move,
    as they do in an eager model that ran the same forward."""
    monkeypatch.setattr(F, "GRAD_GUARD", None)
    batches = twin["batches"]
    b = copy.deepcopy(twin["base"])
    opt = b.configure_optimizers()
    gs = GraphedTrainStep(b, opt, batches[0], warmup=WARM, skip_nonfinite=True)
    assert gs.guard.max_norm == float("inf") and gs.guard.skip_nonfinite is True
    e = _Eager(copy.deepcopy(twin["base"]))
    for _ in range(WARM):
        e.step(batches[0])
    la = [e.step(batches[0]), e.step(batches[1], update=False), e.step(batches[2])]
    lb = [gs(batches[0])["loss"].clone()]
    torch.cuda.synchronize()
    held_p = [p.detach().clone() for p in b.parameters()]
    held_o = _opt_state(opt)
    gs._one.fill_(float("inf"))
    lb.append(gs(batches[1])["loss"].clone())
    gs._one.fill_(1.0)
    torch.cuda.synchronize()
    st = gs.guard.stats()
    assert st["skip"] == 1 and st["skipped"] == 1 and not np.isfinite(st["sumsq"])
    assert any(not torch.isfinite(p.grad).all() for p in b.parameters() if p.grad is not None)
    for p, h in zip(b.parameters(), held_p):
        assert torch.equal(p, h)
    now = _opt_state(opt)
    for k, fields in held_o.items():
        for f, v in fields.items():
            assert torch.equal(now[k][f], v), (k, f)
    lb.append(gs(batches[2])["loss"].clone())
    torch.cuda.synchronize()
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    _same_as(b, opt, _model_state(e.model), _opt_state(e.opt))     # BN statistics included
    st = gs.guard.stats()
    assert st["skip"] == 0 and st["skipped"] == 1 and st["steps"] == WARM + 3


def test_off_means_off(twin, monkeypatch):
    batches = twin["batches"]
    monkeypatch.setattr(F, "GRAD_GUARD", None)
    a = copy.deepcopy(twin["base"])
    opt_a = a.configure_optimizers()
    plain = GraphedTrainStep(a, opt_a, batches[0], warmup=WARM)
    assert plain.guard is None and plain.fused is not None and plain.fused.guard is None
    # MMAD_GRAD_GUARD=inf (read at import; set here as its module value): a guard that measures
    # and would skip, and on finite gradients changes nothing
    monkeypatch.setattr(F, "GRAD_GUARD", "inf")
    b = copy.deepcopy(twin["base"])
    opt_b = b.configure_optimizers()
    guarded = GraphedTrainStep(b, opt_b, batches[0], warmup=WARM)
    assert guarded.guard is not None and guarded.guard.skip_nonfinite is True
    assert guarded.guard.max_norm == float("inf")
    for i in range(STEPS):
        la = plain(batches[i])["loss"].clone()
        lb = guarded(batches[i])["loss"].clone()
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    _same_as(b, opt_b, _model_state(a), _opt_state(opt_a))
    st = guarded.guard.stats()
    assert (st["steps"], st["clipped"], st["skipped"], st["coef"]) == (WARM + STEPS, 0, 0, 1.0)


def test_guard_needs_the_fused_optimizer_path(twin, monkeypatch):
    monkeypatch.setattr(F, "GRAD_GUARD", None)
    b = copy.deepcopy(twin["base"])
    sgd = torch.optim.SGD(b.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="fused optimizer"):
        GraphedTrainStep(b, sgd, twin["batches"][0], warmup=WARM, clip_grad_norm=1.0)
    with pytest.raises(ValueError, match="warmup"):
        GraphedTrainStep(b, b.configure_optimizers(), twin["batches"][0], warmup=0,
                         skip_nonfinite=True)


@pytest.mark.parametrize("mode", ["after", "staged"])
def test_guard_sits_in_the_optimizer_graph_under_data_parallel(twin, monkeypatch, mode):
    """world size 1 (the average is the gradient itself): guarded replays with the collectives
    "after" / "staged" equal the eager twin, the number of backward graphs is what it was, and
    the guard's launches belong to opt_graph (only its replay moves the guard's counter)."""
    import torch.distributed as dist
    from multimodal_alzheimer_amd.data_parallel import GradAllReduce
    from multimodal_alzheimer_amd.graph_step import backward_stages
    monkeypatch.setattr(F, "GRAD_GUARD", None)
    batches = twin["batches"]
    b = copy.deepcopy(twin["base"])
    port = 29573 + (mode == "after")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", torch.cuda.current_device()))
    try:
        opt = b.configure_optimizers()
        if mode == "staged":
            red = GradAllReduce(b.parameters(), bucket_mb=None, stages=backward_stages(b)[1])
        else:
            red = GradAllReduce(b.parameters(), bucket_mb=4.0)
        gs = GraphedTrainStep(b, opt, batches[0], warmup=WARM, reducer=red, collectives=mode,
                              clip_grad_norm=twin["clip"])
        assert gs.opt_graph is not None
        assert len(gs.graphs) == (4 if mode == "staged" else 1)
        losses = [gs(batches[i])["loss"].clone() for i in range(STEPS)]
        torch.cuda.synchronize()
        steps = gs.guard.stats()["steps"]
        assert steps == WARM + STEPS
        for x, y in zip(twin["losses"], losses):
            assert torch.equal(x, y)
        _same_as(b, opt, twin["model"], twin["opt"])
        gs.opt_graph.replay()                        # the guard + Adam alone, once more
        torch.cuda.synchronize()
        assert gs.guard.stats()["steps"] == steps + 1
    finally:
        dist.destroy_process_group()
