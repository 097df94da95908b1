"""explain.occlusion on the device: the three kernels of csrc/occlude.hip bit for bit against
torch / numpy restatements, and the whole call against the CPU oracle run live.

Kernels
  * mmad_occlude_windows: after every launch each slot equals the source with exactly its
    window filled (torch indexing), for float64 and float32, odd W, a clamped last window,
    overlap along d, per-sample fills and tail windows >= P.
  * mmad_occlusion_drop: "logit" is one float64 subtraction: bit-identical to torch.  "prob"
    is exp / sum / divide on C <= 3 values <= 1: both sides are within a few ulp of the true
    probability (one rounding per exp, C - 1 per sum, one per quotient, one per subtraction,
    and the library exps' own ~1 ulp), so they agree to 16 eps = 3.6e-15 absolute.
  * mmad_occlusion_map: bit-identical float32 to a numpy loop that adds the windows in the same
    ascending order in float64 and divides once.

Model level: the plain-torch oracle (tests/_golden.py) takes a Python loop over windows, in
float64 ("exact") and float32 ("ref32").  The bar is on the drops tables,
max|ours - exact| <= max(4 max|ref32 - exact|, 1e-2 max|exact|): the project's float64 bar
without its one-element exception (a forward has no mask-flip routing to excuse), and
max|exact| > 0.  bf16 compute: the yardstick of test_explain_gpu.py (normwise error at most
2 x that of the oracle under CPU autocast bf16, + 0.02), computed live."""
import numpy as np
import pytest
import torch

import multimodal_alzheimer_amd as M
from multimodal_alzheimer_amd import _lib as L
from multimodal_alzheimer_amd import classifiers, explain
from tests import _golden as G
from tests import _poison as P
from tests.test_explain_gpu import _case, _np, _oracle_forward, _oracle_model, _product
from tests.test_poisoned_alloc_gpu import run3

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE, PATCH, STRIDE = (9, 10, 13), (4, 4, 5), (3, 4, 4)      # 3 x 3 x 3 = 27 windows
DTYPES = [pytest.param(torch.float64, id="f64"), pytest.param(torch.float32, id="f32")]


def _windows_list(w):
    """[(z, y, x)] corners in ascending j"""
    return [(z, y, x) for z in w["starts"][0] for y in w["starts"][1] for x in w["starts"][2]]


def _boxed(vol, corner, patch, value):
    out = vol.clone()
    z, y, x = corner
    out[..., z:z + patch[0], y:y + patch[1], x:x + patch[2]] = value
    return out


# --------------------------------------------------------------------------- kernel 1
def _source(dtype, b=3, size=SIZE, seed=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand((b,) + size, generator=gen, device=DEV, dtype=torch.float64).to(dtype)


def _walk(dtype, m, size=SIZE, patch=PATCH, stride=STRIDE, b=3, alloc=torch.empty_like):
    """every replay's slots (a list of (m * b, ...) tensors) and the expected ones"""
    w = explain.occlusion_windows(size, patch, stride)
    corners = _windows_list(w)
    src = P.guarded(_source(dtype, b, size))
    fill = P.guarded(torch.tensor([0.25, -1.5, 1e-3][:b], dtype=torch.float64, device=DEV))
    cursor = torch.zeros((), dtype=torch.int64, device=DEV)
    slots = alloc(src.repeat(m, 1, 1, 1))
    slots.copy_(src.repeat(m, 1, 1, 1))
    got, exp = [], []
    for c in range(explain.replay_count(len(corners), m)):
        explain.occlude_windows(src, slots, fill, cursor, w)
        cursor.add_(m)
        got.append(slots.clone())
        want = src.repeat(m, 1, 1, 1)
        for i in range(m * b):
            j = c * m + i // b
            if j < len(corners):
                want[i] = _boxed(src[i % b], corners[j], patch, fill[i % b].to(dtype))
        exp.append(want)
    return got, exp


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [3, 4])
def test_windows_kernel_matches_torch_indexing(dtype, m):
    got, exp = _walk(dtype, m)
    assert len(got) == (9 if m == 3 else 7)
    for c, (a, e) in enumerate(zip(got, exp)):
        assert torch.equal(a, e), f"replay {c}: {int((a != e).sum())} voxels differ"
    if m == 4:      # the tail of the last replay (windows 27: slots 9..11) is the source again
        src = _source(dtype)
        assert torch.equal(got[-1][9:], src)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size,patch,stride", [((8, 8, 16), (4, 4, 8), (2, 4, 4)),
                                               ((8, 8, 16), (4, 4, 8), (2, 3, 3)),
                                               ((6, 6, 12), (6, 6, 12), (6, 6, 12))])
def test_windows_kernel_vector_and_element_rows(dtype, size, patch, stride):
    """W and the patch width are whole 16-byte units: strides 4 keep every row start aligned
    (the vector path), stride 3 along w puts windows at odd offsets (the element path inside
    the same launch), patch == size is one window"""
    got, exp = _walk(dtype, 2, size, patch, stride, b=2)
    for c, (a, e) in enumerate(zip(got, exp)):
        assert torch.equal(a, e), f"replay {c}: {int((a != e).sum())} voxels differ"


# --------------------------------------------------------------------------- kernel 2
def _drop_case(c, b=3, m=4, p=10):
    gen = torch.Generator(device=DEV).manual_seed(40 + c)
    logits = torch.randn((m * b, c), generator=gen, device=DEV, dtype=torch.float64)
    logits[0] = 0.0                                   # exact zeros (a ReLU-clamped head)
    logits[1] = logits[1, 0]                          # ties
    logits[2, -1] = 0.0
    logits[5] = torch.relu(logits[5])
    target = torch.tensor([0, c - 1, 1][:b], dtype=torch.int64, device=DEV)
    base = torch.randn(b, generator=gen, device=DEV, dtype=torch.float64)
    return logits, target, base, p


def _drop_reference(logits, target, base, mode):
    b = base.shape[0]
    t = target.repeat(logits.shape[0] // b)
    s = torch.softmax(logits, dim=1) if mode == "prob" else logits
    return base.repeat(logits.shape[0] // b) - s.gather(1, t[:, None])[:, 0]


@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("mode", ["logit", "prob"])
def test_drop_kernel_matches_torch_float64(c, mode):
    logits, target, base, p = _drop_case(c)
    b, m = 3, 4
    ref = _drop_reference(logits, target, base, mode).reshape(m, b)
    for cur in (0, 4, 8):                             # the last replay: rows 8, 9 then the tail
        drops = torch.full((p, b), float("nan"), dtype=torch.float64, device=DEV)
        cursor = torch.tensor(cur, dtype=torch.int64, device=DEV)
        explain.occlusion_drop(logits, target, base, cursor, drops, mode)
        rows = min(m, p - cur)
        got = drops[cur:cur + rows]
        if mode == "logit":
            assert torch.equal(got, ref[:rows])
        else:
            err = float((got - ref[:rows]).abs().max())
            print(f"C={c} cursor {cur}: prob max|err| {err:.3e}")
            assert err <= 16 * np.finfo(np.float64).eps
        untouched = torch.ones(p, dtype=torch.bool, device=DEV)
        untouched[cur:cur + rows] = False
        assert torch.isnan(drops[untouched]).all()    # tail rows and other replays' rows


# --------------------------------------------------------------------------- kernel 3
def _map_reference(drops, size, w):
    """numpy: add the windows in ascending j in float64, divide by the count, round once"""
    d = drops.cpu().numpy()
    b = d.shape[1]
    acc = np.zeros((b,) + tuple(size), dtype=np.float64)
    cnt = np.zeros(tuple(size), dtype=np.float64)
    p = w["patch"]
    for j, (z, y, x) in enumerate(_windows_list(w)):
        acc[:, z:z + p[0], y:y + p[1], x:x + p[2]] += d[j][:, None, None, None]
        cnt[z:z + p[0], y:y + p[1], x:x + p[2]] += 1
    assert cnt.min() >= 1
    return (acc / cnt).astype(np.float32)


@pytest.mark.parametrize("size,patch,stride", [(SIZE, PATCH, STRIDE), ((8, 8, 12), (4, 4, 4), None),
                                               ((5, 6, 7), (3, 2, 4), (1, 1, 1))])
def test_map_kernel_is_bit_identical_to_the_numpy_order(size, patch, stride):
    w = explain.occlusion_windows(size, patch, stride)
    gen = torch.Generator(device=DEV).manual_seed(9)
    drops = torch.randn((explain.window_count(w), 3), generator=gen, device=DEV,
                        dtype=torch.float64)
    got = explain.occlusion_map(drops, size, w)
    assert got.dtype == torch.float32 and got.shape == (3,) + tuple(size)
    ref = _map_reference(drops, size, w)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert torch.equal(got, explain.occlusion_map(drops, size, w))
    if stride is None:          # patch == stride: piecewise constant, the map is the drop
        n = [len(s) for s in w["starts"]]
        blocks = drops.t().reshape(3, *n).to(torch.float32)
        for a, p in enumerate(w["patch"]):
            blocks = blocks.repeat_interleave(p, dim=a + 1)
        assert torch.equal(got, blocks)


# ----------------------------------------------------------------------------- poison
@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_windows(dtype):
    def fn():
        got, _ = _walk(dtype, 4, alloc=lambda t: torch.empty_like(t))
        return {f"replay{c}": g for c, g in enumerate(got)}

    def bar(r):
        _, exp = _walk(dtype, 4)
        for c, e in enumerate(exp):
            assert torch.equal(r[f"replay{c}"], e)
    run3(fn, bar)


@pytest.mark.parametrize("mode", ["logit", "prob"])
def test_poisoned_drop_and_map(mode):
    w = explain.occlusion_windows(SIZE, PATCH, STRIDE)
    b, m, p = 3, 4, 27
    gen = torch.Generator(device=DEV).manual_seed(17)
    logits = torch.randn((7, m * b, 3), generator=gen, device=DEV, dtype=torch.float64)
    target = torch.tensor([0, 2, 1], dtype=torch.int64, device=DEV)
    base = torch.rand(b, generator=gen, device=DEV, dtype=torch.float64)

    def fn():
        drops = torch.empty((p, b), dtype=torch.float64, device=DEV)
        cursor = torch.zeros((), dtype=torch.int64, device=DEV)
        for c in range(7):                            # 27 rows in replays of 4: all written
            explain.occlusion_drop(P.guarded(logits[c].contiguous()), P.guarded(target),
                                   P.guarded(base), cursor, drops, mode)
            cursor.add_(m)
        return {"drops": drops, "map": explain.occlusion_map(drops, SIZE, w)}

    def bar(r):
        ref = _map_reference(r["drops"], SIZE, w)
        assert np.array_equal(r["map"].cpu().numpy().view(np.uint32), ref.view(np.uint32))
    run3(fn, bar)


# ------------------------------------------------------------------------ model level
_ORACLE = {}
CASES = {  # name -> (patch, stride)
    "pet_resnet_r10": (16, 8), "anat_r10_focal": (16, 8), "small_pet": (8, 8),
    "early_fusion": (8, 8), "anat_pet_fusion": (16, 16),
}


def _oracle_scores(ref, mode, vols, tgt, score):
    dtype = torch.float64 if mode == "f64" else torch.float32
    x = {k: v.to(dtype) for k, v in vols.items()}
    with torch.no_grad():
        if hasattr(ref, "inputs"):                    # early fusion: channel-stacked
            out = ref(*ref.inputs(x, dtype))
        elif mode == "bf16":
            with torch.autocast("cpu", dtype=torch.bfloat16):
                out = _oracle_forward(ref, x)
        else:
            out = _oracle_forward(ref, x)
    out = out.double()
    t = tgt.repeat(out.shape[0] // tgt.shape[0])
    s = torch.softmax(out, dim=1) if score == "prob" else out
    return s.gather(1, t[:, None])[:, 0]


def _oracle_occlusion(name, mode, score="logit", fill=0.0):
    """{"drops": {k: (B, n_d, n_h, n_w)}, "maps": {k: (B, D, H, W) float64}, "score": s0}: a
    Python loop over the windows of the plain-torch model (rows of one forward are windows of
    the same patients: eval-mode samples are independent)"""
    key = (name, mode, score, fill)
    if key in _ORACLE:
        return _ORACLE[key]
    g, batch, tgt = _case(name)
    ref = _oracle_model(name, mode)
    keys = G.CASES[name][3]
    vols = {k: batch[k] for k in keys}
    b = tgt.shape[0]
    patch, stride = CASES[name]
    w = explain.occlusion_windows(tuple(vols[keys[0]].shape[1:]), patch, stride)
    corners = _windows_list(w)
    s0 = _oracle_scores(ref, mode, vols, tgt, score)
    out = {"drops": {}, "maps": {}, "score": s0.numpy()}
    chunk = max(1, 6 // b)           # windows per oracle forward: small batches are the fastest
    for k in keys:
        f = vols[k].mean(dim=(1, 2, 3)) if fill == "mean" else torch.full((b,), float(fill),
                                                                          dtype=torch.float64)
        rows = []
        for c0 in range(0, len(corners), chunk):
            part = corners[c0:c0 + chunk]
            stacked = {kk: v.repeat(len(part), 1, 1, 1) for kk, v in vols.items()}
            stacked[k] = torch.cat([_boxed(vols[k], cn, w["patch"], f[:, None, None, None])
                                    for cn in part])
            sc = _oracle_scores(ref, mode, stacked, tgt, score)
            rows.append(s0.repeat(len(part)) - sc)
        d = torch.cat(rows).reshape(len(corners), b)
        out["drops"][k] = d.t().reshape(b, *[len(s) for s in w["starts"]]).numpy()
        acc = np.zeros(tuple(vols[k].shape))
        cnt = np.zeros(tuple(vols[k].shape[1:]))
        p = w["patch"]
        for j, (z, y, x) in enumerate(corners):
            acc[:, z:z + p[0], y:y + p[1], x:x + p[2]] += d[j].numpy()[:, None, None, None]
            cnt[z:z + p[0], y:y + p[1], x:x + p[2]] += 1
        out["maps"][k] = acc / cnt
    _ORACLE[key] = out
    return out


def _assert_bar(what, ours, ref32, exact):
    e_ours, e_ref = np.abs(ours - exact).max(), np.abs(ref32 - exact).max()
    print(f"{what}: max|exact| {np.abs(exact).max():.3e}, oracle fp32 err {e_ref:.3e}, "
          f"ours {e_ours:.3e}")
    assert np.abs(exact).max() > 0
    assert e_ours <= max(4 * e_ref, 1e-2 * np.abs(exact).max())


def _check_model(name, score="logit", fill=0.0, **kw):
    m, batch, tgt = _product(name)
    patch, stride = CASES[name]
    out = explain.occlusion(m, batch, target=tgt, patch=patch, stride=stride, score=score,
                            fill=fill, **kw)
    exact = _oracle_occlusion(name, "f64", score, fill)
    ref32 = _oracle_occlusion(name, "f32", score, fill)
    keys = list(kw.get("keys") or G.CASES[name][3])
    assert sorted(out["maps"]) == sorted(out["drops"]) == sorted(keys)
    assert torch.equal(out["target"], tgt)
    assert out["score"].dtype == torch.float64
    assert np.abs(_np(out["score"]) - exact["score"]).max() <= \
        max(4 * np.abs(ref32["score"] - exact["score"]).max(), 1e-2 * np.abs(exact["score"]).max())
    for k in keys:
        d = out["drops"][k]
        assert d.dtype == torch.float64 and tuple(d.shape) == exact["drops"][k].shape
        _assert_bar(f"{name}/{k}/{score} drops", _np(d), ref32["drops"][k], exact["drops"][k])
        assert out["maps"][k].dtype == torch.float32
        assert tuple(out["maps"][k].shape) == tuple(batch[k].shape)
    k = keys[0]
    _assert_bar(f"{name}/{k}/{score} map", _np(out["maps"][k]), ref32["maps"][k], exact["maps"][k])
    return out


@pytest.mark.parametrize("name,score", [("pet_resnet_r10", "logit"), ("anat_r10_focal", "logit"),
                                        ("anat_r10_focal", "prob"), ("small_pet", "logit"),
                                        ("early_fusion", "logit"), ("anat_pet_fusion", "logit")])
def test_fp32_drops_match_the_float64_oracle(name, score):
    out = _check_model(name, score)
    if name in ("early_fusion", "anat_pet_fusion"):
        assert sorted(out["maps"]) == ["mri", "pet1451"]        # one map per modality
    if name == "anat_r10_focal":
        assert out["target"].shape[0] == 3                      # m = 2: a 6-row forward


def test_bf16_drops_within_the_reference_bf16_error():
    name = "pet_resnet_r10"
    m, batch, tgt = _product(name, torch.bfloat16)
    patch, stride = CASES[name]
    out = explain.occlusion(m, batch, target=tgt, patch=patch, stride=stride)
    exact = _oracle_occlusion(name, "f64")
    ref16 = _oracle_occlusion(name, "bf16")
    for k in exact["drops"]:
        ours = _np(out["drops"][k])
        nrm = np.linalg.norm(exact["drops"][k])
        e_ours = np.linalg.norm(ours - exact["drops"][k]) / nrm
        e_ref = np.linalg.norm(ref16["drops"][k] - exact["drops"][k]) / nrm
        print(f"{name}/{k}: normwise error ours {e_ours:.3e}, oracle bf16 autocast {e_ref:.3e}")
        assert np.isfinite(ours).all()
        assert e_ours <= 2 * e_ref + 0.02, (e_ours, e_ref)


@pytest.mark.parametrize("name", ["pet_resnet_r10", "early_fusion"])
def test_graph_and_eager_paths_give_the_same_bits(name):
    m, batch, tgt = _product(name)
    patch, stride = CASES[name]
    runs = [explain.occlusion(m, batch, target=tgt, patch=patch, stride=stride, graph=g)
            for g in (True, False, True)]
    for other in runs[1:]:
        for k in runs[0]["maps"]:
            assert torch.equal(runs[0]["maps"][k], other["maps"][k]), k
            assert torch.equal(runs[0]["drops"][k], other["drops"][k]), k
        assert torch.equal(runs[0]["score"], other["score"])


def test_targets_fill_and_keys():
    name = "anat_pet_fusion"
    m, batch, tgt = _product(name)
    a = explain.occlusion(m, batch, patch=16, keys=("mri",))
    assert list(a["maps"]) == ["mri"] and list(a["drops"]) == ["mri"]
    assert torch.equal(a["target"], tgt)                        # None: the eval argmax
    assert a["windows"] == explain.occlusion_windows((32, 32, 32), 16)
    b = explain.occlusion(m, batch, target=int(tgt[0]), patch=16, keys="mri")
    assert torch.equal(b["target"], torch.full_like(tgt, int(tgt[0])))
    c = explain.occlusion(m, batch, target=tgt.cpu(), patch=16, keys=("mri",))
    assert torch.equal(c["drops"]["mri"], a["drops"]["mri"])
    with pytest.raises(ValueError):
        explain.occlusion(m, batch, target=7, patch=16)
    _check_model(name, fill="mean", keys=("mri",))              # against the oracle's own loop


def test_graph_true_on_a_tabpfn_stage_class_raises():
    m = object.__new__(classifiers.Tabular_MRT_Model)
    with pytest.raises(ValueError, match="captured"):
        explain.occlusion(m, {"mri": torch.zeros((1, 8, 8, 8), device=DEV)}, patch=4, graph=True)


# ------------------------------------------------------------------------ model state
def _train_step(m, batch):
    for p in m.parameters():
        p.grad = None
    m.train()
    o = m.general_step(batch, 0, "train")
    o["loss"].backward()
    torch.cuda.synchronize()
    return o["loss"].detach().clone(), m.model.conv1.weight.grad.detach().clone()


def test_occlusion_leaves_the_model_and_the_training_step_untouched():
    torch.manual_seed(3)
    m = M.Anat_CNN(G.anat_hparams(10)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    batch = {"mri": torch.rand((2, 32, 32, 32), generator=gen, device=DEV, dtype=torch.float64),
             "label": torch.tensor([0, 1], device=DEV)}
    state = {k: v.clone() for k, v in m.state_dict().items()}
    loss0, dw0 = _train_step(m, batch)
    m.load_state_dict(state)
    for p in m.parameters():
        p.grad = None
    frozen = next(iter(m.model.conv_seg.parameters()))
    frozen.requires_grad_(False)                                # a flag the call must put back
    flags = [p.requires_grad for p in m.parameters()]
    m.train()
    mri = batch["mri"].clone()
    out = explain.occlusion(m, batch, patch=16, score="prob")
    assert m.training and all(mod.training for mod in m.modules())
    assert [p.requires_grad for p in m.parameters()] == flags
    assert all(p.grad is None for p in m.parameters())          # no parameter has a .grad
    assert torch.equal(batch["mri"], mri)                       # the caller's volumes too
    for k, v in m.state_dict().items():                         # running statistics unchanged
        assert torch.equal(v, state[k]), k
    assert torch.isfinite(out["maps"]["mri"]).all() and torch.isfinite(out["drops"]["mri"]).all()
    frozen.requires_grad_(True)
    loss1, dw1 = _train_step(m, batch)
    assert torch.equal(loss0, loss1)
    assert torch.equal(dw0, dw1)


def test_flags_are_restored_after_an_exception_inside_a_forward():
    torch.manual_seed(4)
    m = M.Small_PET_CNN(G.pet_hparams()).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(6)
    batch = {"pet1451": torch.rand((2, 16, 16, 16), generator=gen, device=DEV,
                                   dtype=torch.float64)}
    m.train()
    flags = [p.requires_grad for p in m.parameters()]

    def boom(_mod, _args):
        raise RuntimeError("boom")
    h = m.model.register_forward_pre_hook(boom)
    try:
        with pytest.raises(RuntimeError, match="boom"):
            explain.occlusion(m, batch, patch=8, graph=False)
    finally:
        h.remove()
    assert m.training and all(mod.training for mod in m.modules())
    assert [p.requires_grad for p in m.parameters()] == flags
    out = explain.occlusion(m, batch, patch=8)                  # and the model still works
    assert out["maps"]["pet1451"].shape == (2, 16, 16, 16)
