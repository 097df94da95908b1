"""The captured training step's optimizer: Adam fused with the bf16 weight repack.

``AdamRepack(optimizer, plans)`` replaces ``optimizer.step()`` inside a captured step
(graph_step.GraphedTrainStep) by ONE launch of ``mmad_adam_repack`` (csrc/adam.hip):

* every parameter of every group gets torch's fused Adam update, bit for bit (the
  reference's optimizer: ``torch.optim.Adam`` over anat_cnn.py:111-126's groups, here
  ``classifiers.MergedAdam`` with ``fused=True``), its device ``step`` counter included, so
  the optimizer state stays torch's own (``state_dict`` / resume unchanged);
* each conv weight a ``volume_ops.PackPlan`` repacks every step (the bf16 forward and
  input-gradient layouts, ``mmad_conv_pack_dual_batch``) leaves the update in both layouts
  as well, for the NEXT step's forward: the captured forward then skips that repack
  (``PackPlan.external``), so the fp32 weights are read once per step, not twice, and four
  launches (step counters, two learning-rate groups, the repack) become one.

The packed copies are then only as fresh as the last Adam step: ``refresh()`` repacks them
from the fp32 weights (GraphedTrainStep calls it before the first replay and whenever a
parameter was modified outside the graph, seen through its ``_version``).

Supported: ``torch.optim.Adam`` (and subclasses that keep its ``step``) with fused=True,
amsgrad / maximize / differentiable / decoupled weight decay off, float betas, fp32
parameters and state, no gradient scaler.  ``supported(optimizer)`` says whether it
applies; the caller keeps ``optimizer.step()`` otherwise.

Gradient guard.  ``GradGuard`` measures the global L2 norm of the gradients in one bandwidth
pass (csrc/gradguard.hip: ``mmad_grad_sumsq`` + ``mmad_grad_guard_finalize``) and leaves, in a
float64[10] device tensor ``state`` (slot names below), the norm, the clip coefficient of
``torch.nn.utils.clip_grad_norm_`` and a skip flag for a step whose gradients hold an Inf or a
NaN.  Two consumers:

* ``AdamRepack(optimizer, plans, guard=guard)``: ``step()`` measures, then launches
  ``mmad_adam_repack_guarded``, which multiplies each gradient by the coefficient on its way
  into the update (bit for bit ``g.mul_(coef)`` followed by torch's Adam) and does nothing at
  all on a skipped step (torch's fused Adam under ``found_inf``).  ``p.grad`` is NOT rewritten:
  after a guarded step it still holds the unclipped gradient, and ``state`` says what was
  applied.
* ``clip_grad_norm_(parameters, max_norm, guard=None)``: the eager form for hand-written loops,
  ``guard.measure()`` then ``guard.apply_()`` (``mmad_grad_scale`` rewrites the gradients in
  place), a drop-in for the torch function that returns the norm without a host sync.

The threshold and the skip switch live in ``state`` and are read by the kernels, so
``set_max_norm`` / ``set_skip_nonfinite`` between two replays of a captured step take effect
without a re-capture."""
import ctypes as C
import inspect
import math
import os

import torch

from . import _lib as L

# MMAD_ADAM_REPACK=0: captured steps keep torch's fused Adam and the in-forward repack (A/B)
ENABLED = os.environ.get("MMAD_ADAM_REPACK", "1") != "0"
# MMAD_GRAD_GUARD=<float>: graph_step.GraphedTrainStep built without clip_grad_norm= /
# skip_nonfinite= gets a GradGuard with this max_norm (inf: measure and skip only) and
# skip_nonfinite=True; unset: no guard
GRAD_GUARD = os.environ.get("MMAD_GRAD_GUARD") or None

# slots of GradGuard.state (float64[10]; include/mmad.h)
MAX_NORM, SKIP_NONFINITE, SUMSQ, NORM, COEF, SKIP, STEPS, CLIPPED, SKIPPED, RESERVED = range(10)
STATE_SLOTS = 10
STATE_NAMES = ("max_norm", "skip_nonfinite", "sumsq", "norm", "coef", "skip", "steps",
               "clipped", "skipped", "reserved")
GRAD_CHUNK = 4096                 # elements per chunk of a gradient job (csrc/gradguard.hip)
GRAD_MAX_BLOCKS = 1024            # slots of GradGuard.partials


def supported(optimizer):
    if not ENABLED or not isinstance(optimizer, torch.optim.Adam):
        return False
    # (torch wraps a class's step with its profiling hook on first construction, on the
    # subclass or on Adam itself: compare the functions underneath)
    if isinstance(optimizer, torch.optim.AdamW) or \
            inspect.unwrap(type(optimizer).step) is not inspect.unwrap(torch.optim.Adam.step):
        return False
    if getattr(optimizer, "grad_scale", None) is not None or \
            getattr(optimizer, "found_inf", None) is not None:
        return False
    for g in optimizer.param_groups:
        if not g.get("fused") or g.get("amsgrad") or g.get("maximize") or \
                g.get("differentiable") or g.get("decoupled_weight_decay", False):
            return False
        b1, b2 = g["betas"]
        if torch.is_tensor(b1) or torch.is_tensor(b2) or torch.is_tensor(g["eps"]) or \
                torch.is_tensor(g["weight_decay"]):
            return False
    return True


def state_ready(optimizer):
    """every parameter that will get a gradient has its Adam state (one eager step ran)"""
    return all(all(k in optimizer.state.get(p, {}) for k in ("step", "exp_avg", "exp_avg_sq"))
               for g in optimizer.param_groups for p in g["params"] if p.requires_grad)


def pack_plans(model):
    """the volume_ops.PackPlan objects under ``model`` (built by its forwards)"""
    out = []
    for m in model.modules():
        plan = getattr(m, "_mmad_pack_plan", None)
        if plan is not None and plan not in out:
            out.append(plan)
    return out


def check_max_norm(max_norm):
    """``max_norm`` as a float: None = +inf (measure only); non-positive or NaN raises"""
    if max_norm is None:
        return math.inf
    if isinstance(max_norm, bool) or torch.is_tensor(max_norm):
        raise ValueError(f"max_norm must be a positive number or None, not {max_norm!r}")
    try:
        v = float(max_norm)
    except (TypeError, ValueError):
        raise ValueError(f"max_norm must be a positive number or None, not {max_norm!r}") from None
    if math.isnan(v) or v <= 0.0:
        raise ValueError(f"max_norm must be positive (None or inf: do not clip), got {max_norm!r}")
    return v


def guard_settings(clip_grad_norm=None, skip_nonfinite=False, env=None):
    """What GraphedTrainStep's guard arguments ask for: ``None`` (no guard) or ``(max_norm,
    skip_nonfinite)``.  ``env`` (the value of MMAD_GRAD_GUARD) counts only when both arguments
    are at their defaults: that max_norm and skip_nonfinite=True."""
    if clip_grad_norm is None and not skip_nonfinite:
        if env is None or env == "":
            return None
        try:
            v = float(env)
        except ValueError:
            raise ValueError(f"MMAD_GRAD_GUARD must be a positive number or inf, got {env!r}") \
                from None
        return check_max_norm(v), True
    return check_max_norm(clip_grad_norm), bool(skip_nonfinite)


class GradGuard:
    """Global gradient norm, clip coefficient and non-finite flag of a set of parameters, on
    the device (module docstring).  ``params_or_optimizer``: an optimizer (its groups'
    parameters), an iterable of tensors or one tensor; parameters without a gradient when
    ``measure()`` runs are left out, as torch leaves them out.  ``max_norm=None`` is +inf: the
    norm is measured and nothing is clipped."""

    def __init__(self, params_or_optimizer, max_norm=None, skip_nonfinite=True):
        self._max_norm = check_max_norm(max_norm)
        self._skip_nonfinite = bool(skip_nonfinite)
        if isinstance(params_or_optimizer, torch.optim.Optimizer):
            ps = [p for g in params_or_optimizer.param_groups for p in g["params"]]
        elif torch.is_tensor(params_or_optimizer):
            ps = [params_or_optimizer]
        else:
            ps = list(params_or_optimizer)
        if any(not torch.is_tensor(p) for p in ps):
            raise ValueError("GradGuard: parameters must be tensors")
        self.params = ps
        self.state = self.partials = self.table = None
        self.njobs = self.chunks = self.nblocks = 0
        self._host = self._committed = b""

    def prepare(self, device):
        """allocate the state, the block partials and the device job table (before a capture:
        nothing may be allocated from the host inside one)"""
        self.state = torch.zeros(STATE_SLOTS, dtype=torch.float64, device=device)
        self.state[MAX_NORM].fill_(self._max_norm)
        self.state[SKIP_NONFINITE].fill_(float(self._skip_nonfinite))
        self.partials = torch.empty(GRAD_MAX_BLOCKS, dtype=torch.float64, device=device)
        self.table = torch.empty(max(len(self.params), 1) * C.sizeof(L.GradJob),
                                 dtype=torch.uint8, device=device)
        self._committed = b""

    def _device(self):
        for p in self.params:
            if p.is_cuda:
                return p.device
        raise L.MMADError("GradGuard runs on HIP devices only: no parameter is on one")

    def _jobs(self):
        jobs, chunks = [], 0
        for p in self.params:
            g = p.grad
            if g is None or g.numel() == 0:
                continue
            if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
                raise ValueError("GradGuard: gradients must be contiguous fp32 device tensors")
            j = L.GradJob()
            j.grad, j.numel, j.chunk0 = g.data_ptr(), g.numel(), chunks
            chunks += (g.numel() + GRAD_CHUNK - 1) // GRAD_CHUNK
            jobs.append(j)
        return jobs, chunks

    def measure(self):
        """launch the norm pass and its finalize on the current stream (capturable: the job
        table of the gradients present now is written by ``commit()``, outside capture)"""
        if self.state is None:
            self.prepare(self._device())
        jobs, chunks = self._jobs()
        if len(jobs) * C.sizeof(L.GradJob) > self.table.numel():
            raise ValueError("GradGuard: more jobs than prepared")
        self.njobs, self.chunks = len(jobs), chunks
        self.nblocks = L.load().mmad_grad_guard_blocks(chunks)
        self._host = bytes((L.GradJob * len(jobs))(*jobs)) if jobs else b""
        if not torch.cuda.is_current_stream_capturing():
            self.commit()
        L.call("mmad_grad_sumsq", self.njobs, L.ptr(self.table), self.chunks, self.nblocks,
               L.ptr(self.partials), L.stream())
        L.call("mmad_grad_guard_finalize", self.nblocks, L.ptr(self.partials),
               L.ptr(self.state), L.stream())

    def commit(self):
        """copy the job table built by the last ``measure()`` to the device (outside capture;
        nothing to do while the gradients stay where they were)"""
        if self._host and self._host != self._committed:
            host = torch.frombuffer(bytearray(self._host), dtype=torch.uint8)
            self.table[:host.numel()].copy_(host)
            self._committed = self._host

    def apply_(self):
        """``g *= coef`` in place over the gradients of the last ``measure()`` (nothing on a
        step to be skipped)"""
        if self.state is None:
            raise ValueError("GradGuard.apply_: call measure() first")
        L.call("mmad_grad_scale", self.njobs, L.ptr(self.table), self.chunks,
               L.ptr(self.state), L.stream())

    def set_max_norm(self, max_norm):
        """new clip threshold (None / inf: do not clip), in place: the next launch or replay
        reads it"""
        self._max_norm = check_max_norm(max_norm)
        if self.state is not None:
            self.state[MAX_NORM].fill_(self._max_norm)

    def set_skip_nonfinite(self, on):
        self._skip_nonfinite = bool(on)
        if self.state is not None:
            self.state[SKIP_NONFINITE].fill_(float(self._skip_nonfinite))

    @property
    def max_norm(self):
        return self._max_norm

    @property
    def skip_nonfinite(self):
        return self._skip_nonfinite

    # 0-d device views of the state: reading one into Python is the caller's sync
    @property
    def norm(self):
        return self.state[NORM]

    @property
    def coef(self):
        return self.state[COEF]

    @property
    def skip(self):
        return self.state[SKIP]

    def stats(self):
        """the state as a dict of Python numbers (one host sync)"""
        vals = self.state.tolist()
        out = dict(zip(STATE_NAMES, vals))
        for k in ("skip_nonfinite", "skip", "steps", "clipped", "skipped"):
            out[k] = int(out[k])
        del out["reserved"]
        return out


def clip_grad_norm_(parameters, max_norm, guard=None):
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` (L2) in three launches and no
    host sync: measure, finalize, scale in place.  Returns the total norm as a 0-d float64
    device tensor, a view of ``guard.state`` that the next call overwrites.  ``guard``: a
    GradGuard over the same parameters, kept between calls (its buffers and job table are
    reused, its ``max_norm`` follows this call's); without one a fresh guard is built, which
    never skips (a non-finite norm propagates into the gradients, as in torch)."""
    if guard is None:
        guard = GradGuard(parameters, max_norm, skip_nonfinite=False)
    elif check_max_norm(max_norm) != guard.max_norm:
        guard.set_max_norm(max_norm)
    guard.measure()
    guard.apply_()
    return guard.norm


class AdamRepack:
    def __init__(self, optimizer, plans=(), guard=None):
        """``guard``: a GradGuard over the optimizer's parameters; ``step()`` then measures
        the gradients and launches the guarded update (module docstring)"""
        if not supported(optimizer):
            raise ValueError("AdamRepack: optimizer configuration not supported")
        self.optimizer = optimizer
        self.guard = guard
        self.plans = [p for p in plans if p.nduals or p.unfolds]
        self.table = None
        self.njobs = self.tiles = 0
        self._host = None

    def _jobs(self):
        lib = L.load()
        dual, unf = {}, {}
        for plan in self.plans:
            for job in plan.duals:
                dual[job.w] = job
            for w, d, wp in plan.unfolds:
                unf[w.data_ptr()] = (d, wp)
        jobs, tiles = [], 0
        for g in self.optimizer.param_groups:
            lr = g["lr"]
            if not (torch.is_tensor(lr) and lr.is_cuda and lr.dtype == torch.float32):
                raise ValueError("AdamRepack: the group lr must be a device float32 tensor "
                                 "(graph_step installs one)")
            b1, b2 = g["betas"]
            for p in g["params"]:
                if p.grad is None:
                    continue                 # torch's Adam skips these too
                st = self.optimizer.state.get(p, {})
                need = ("step", "exp_avg", "exp_avg_sq")
                if any(k not in st for k in need):
                    raise ValueError("AdamRepack: optimizer state not initialised (run one "
                                     "eager step first)")
                ts = (p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"])
                if any(not t.is_cuda or t.dtype != torch.float32 for t in ts) or \
                        any(not t.is_contiguous() for t in ts[:4]) or st["step"].numel() != 1:
                    raise ValueError("AdamRepack: fp32 contiguous device tensors required")
                j = L.AdamJob()
                j.param, j.grad = p.data_ptr(), p.grad.data_ptr()
                j.exp_avg, j.exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                j.step, j.lr = st["step"].data_ptr(), lr.data_ptr()
                j.beta1, j.beta2 = float(b1), float(b2)
                j.eps, j.weight_decay = float(g["eps"]), float(g["weight_decay"])
                d = dual.get(p.data_ptr())
                if d is not None:
                    j.w_fwd, j.w_dgrad = d.w_fwd, d.w_dgrad
                    j.co, j.ci, j.taps, j.flip = d.co, d.ci, d.taps, d.flip
                u = unf.get(p.data_ptr())
                if u is not None:
                    desc, wp = u
                    j.w_fwd = wp.data_ptr()
                    j.co, j.ci, j.taps = desc.co, 1, desc.kd * desc.kh
                    j.unf_kw, j.kpad = desc.kw, wp.numel() // desc.co
                j.numel = p.numel()
                j.tile0 = tiles
                j.ntiles = lib.mmad_adam_job_tiles(j)
                tiles += j.ntiles
                jobs.append(j)
        # a repacked weight without an update here (frozen, or outside the optimizer) does
        # not change in the step, so its packed copy from refresh() stays valid
        return jobs, tiles

    def prepare(self, device):
        """allocate the device job table and arrival counters (before capture: nothing may
        be allocated from the host inside one)"""
        n = sum(len(g["params"]) for g in self.optimizer.param_groups)
        self.table = torch.empty(max(n, 1) * C.sizeof(L.AdamJob), dtype=torch.uint8,
                                 device=device)
        self.arrivals = torch.zeros(max(n, 1), dtype=torch.int32, device=device)
        # each block's job index (sized for every parameter as repacked tiles or 4096-element
        # chunks, the most blocks the jobs can need)
        lib = L.load()
        blocks = 0
        for g in self.optimizer.param_groups:
            for p in g["params"]:
                j = L.AdamJob()
                j.numel = p.numel()
                blocks += max(lib.mmad_adam_job_tiles(C.byref(j)), 1)
                if p.dim() == 5:
                    blocks += p.shape[0] // 16 * max(p.shape[1] // 16, 1) + p.shape[0]
        self.block_job = torch.zeros(max(blocks, 1), dtype=torch.int32, device=device)
        if self.guard is not None and self.guard.state is None:
            self.guard.prepare(device)

    def step(self):
        """launch the fused update on the current stream (capturable: the job table is
        written by ``commit()`` once the gradients' addresses are known)"""
        jobs, tiles = self._jobs()
        if self.table is None:
            self.prepare(next(iter(self.optimizer.param_groups))["params"][0].device)
        if len(jobs) * C.sizeof(L.AdamJob) > self.table.numel():
            raise ValueError("AdamRepack: more jobs than prepared")
        if tiles > self.block_job.numel():
            raise ValueError("AdamRepack: more blocks than prepared")
        self.njobs, self.tiles = len(jobs), tiles
        self._host = bytes((L.AdamJob * len(jobs))(*jobs)) if jobs else b""
        self._host_map = torch.repeat_interleave(
            torch.arange(len(jobs), dtype=torch.int32),
            torch.tensor([j.ntiles for j in jobs], dtype=torch.int64)) if jobs else None
        if not torch.cuda.is_current_stream_capturing():
            self.commit()
        if self.guard is None:
            L.call("mmad_adam_repack", self.njobs, L.ptr(self.table), L.ptr(self.block_job),
                   self.tiles, L.ptr(self.arrivals), L.stream())
        else:
            self.guard.measure()
            L.call("mmad_adam_repack_guarded", self.njobs, L.ptr(self.table),
                   L.ptr(self.block_job), self.tiles, L.ptr(self.arrivals),
                   L.ptr(self.guard.state), L.stream())

    def commit(self):
        """copy the job table built by the last ``step()`` to the device (outside capture),
        and the guard's"""
        if self.guard is not None:
            self.guard.commit()
        if self._host:
            host = torch.frombuffer(bytearray(self._host), dtype=torch.uint8)
            self.table[:host.numel()].copy_(host)
            self.block_job[:self._host_map.numel()].copy_(self._host_map)

    def set_external(self, on):
        for plan in self.plans:
            plan.external = bool(on)

    def refresh(self):
        """repack every covered conv weight from its current fp32 values"""
        for plan in self.plans:
            plan.run_duals()

    def params(self):
        return [p for g in self.optimizer.param_groups for p in g["params"]]
