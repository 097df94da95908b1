"""Input-gradient / attribution timings (multimodal_alzheimer_amd.explain), sides interleaved.

    python tools/bench_explain.py [--rounds 5] [--calls 20] [--skip-model]

1. Kernel: the stem's input gradient on the same bf16 dY at 8 x 128^3 and 2 x 91 x 109 x 91,
   ``stem`` = the dedicated kernel (mmad_conv3d_dgrad_raw, with its tap-image pack launch)
   against ``generic`` = weight Ci padded to 8 + pack + mmad_conv3d_dgrad + mmad_take_channel
   (volume_ops.raw_input_grad, both routes as the backward runs them), and ``stem_fwd`` = the
   stem forward on the raw f64 volume with a prepacked weight, the equal-FLOP yardstick.
   Device events around ``calls`` back-to-back launches; per round one figure per side, sides
   alternating; every side warmed at each shape.
2. Model: ``explain.saliency(method="gradient")`` on bench.py's ResNet-10 at 8 x 128^3 (bf16)
   against one eager training step of the same model (forward + full backward with weight
   gradients, no optimizer).
3. ``--occlusion`` (on its own): ``explain.occlusion`` on the same ResNet-10 at 1 x 128^3,
   patch 16, stride 8 (3375 windows, 422 forwards of 8 rows), ``graph=True`` (the replayed
   capture) against ``graph=False`` (the same launches from Python), whole calls interleaved.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multimodal_alzheimer_amd as M  # noqa: E402
from multimodal_alzheimer_amd import _lib as L  # noqa: E402
from multimodal_alzheimer_amd import explain  # noqa: E402
from multimodal_alzheimer_amd import volume_ops as V  # noqa: E402

SHAPES = [(8, 1, 128, 128, 128), (2, 1, 91, 109, 91)]
GEOM = ((2, 2, 2), (3, 3, 3), (1, 1, 1))


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls          # ms per call


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


def interleaved(sides, rounds, calls, warm=3):
    for fn in sides.values():                   # warm every side at this shape
        timed(fn, warm)
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn, calls))
    return {k: summary(v) for k, v in ms.items()}


def kernel_times(shape, rounds, calls):
    gen = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randn((64, 1, 7, 7, 7), generator=gen, device="cuda") * 0.05
    d = V.conv_desc(shape, tuple(w.shape), *GEOM)
    gy = torch.randn((shape[0], 64, d.do_, d.ho, d.wo), generator=gen, device="cuda").to(
        torch.bfloat16).contiguous(memory_format=V.CL)
    x = torch.rand(shape, generator=gen, device="cuda", dtype=torch.float64)
    wp = V.pack_weight(d, L.BF16, w, torch.bfloat16, False)
    assert L.load().mmad_stem_dgrad_ok(d, L.BF16, L.F64) == 1

    def fwd():
        with torch.no_grad():
            V.conv3d(x, w, None, *GEOM, torch.bfloat16, False, (wp, None))

    sides = {
        "stem": lambda: V.raw_input_grad(d, gy, w, torch.float64, route="stem"),
        "generic": lambda: V.raw_input_grad(d, gy, w, torch.float64, route="generic"),
        "stem_fwd": fwd,
    }
    a = sides["stem"]()
    b = sides["generic"]()
    out = interleaved(sides, rounds, calls)
    flops = 2.0 * 343 * 64 * gy.numel() / 64    # useful: one 7^3 x 64 dot product per dY voxel
    for k in out:
        out[k]["useful_TFLOPs"] = round(flops / (out[k]["median_ms"] * 1e-3) / 1e12, 1)
    out["stem"]["ratio_to_generic"] = round(
        out["stem"]["median_ms"] / out["generic"]["median_ms"], 3)
    return {"shape": list(shape), "out_dtype": "float64", "calls": calls, "rounds": rounds,
            "max_abs_diff_stem_vs_generic": float((a - b).abs().max()),
            "max_abs": float(b.abs().max()), "sides": out}


def model_times(rounds, calls, precision):
    from bench import hparams
    b, s = 8, 128
    g = torch.Generator(device="cuda").manual_seed(1000)
    batch = {"mri": torch.rand((b, s, s, s), device="cuda", dtype=torch.float64, generator=g),
             "label": torch.randint(0, 2, (b,), device="cuda", generator=g)}
    torch.manual_seed(15)
    m = M.Anat_CNN(hparams(precision)).cuda()

    def step():
        m.train()
        for p in m.parameters():
            p.grad = None
        m.general_step(batch, 0, "train")["loss"].backward()

    sides = {"saliency_gradient": lambda: explain.saliency(m, batch),
             "eager_train_step": step}
    out = interleaved(sides, rounds, calls, warm=2)
    return {"workload": f"Anat_CNN ResNet-10, batch {b} x {s}^3, {precision}, eager",
            "calls": calls, "rounds": rounds, "sides": out}


def occlusion_times(rounds, precision, patch, stride, size):
    """explain.occlusion with the replayed graph against the same launches issued from Python"""
    from bench import hparams
    g = torch.Generator(device="cuda").manual_seed(1000)
    batch = {"mri": torch.rand((1, size, size, size), device="cuda", dtype=torch.float64,
                               generator=g)}
    torch.manual_seed(15)
    m = M.Anat_CNN(hparams(precision)).cuda()
    w = explain.occlusion_windows((size,) * 3, patch, stride)
    n_win = explain.window_count(w)
    sides = {"graph": lambda: explain.occlusion(m, batch, patch=patch, stride=stride,
                                                score="prob", graph=True),
             "eager": lambda: explain.occlusion(m, batch, patch=patch, stride=stride,
                                                score="prob", graph=False)}
    a, b = sides["graph"](), sides["eager"]()
    out = interleaved(sides, rounds, 1, warm=1)
    forwards = explain.replay_count(n_win, 8)
    for k in out:
        out[k]["ms_per_forward"] = round(out[k]["median_ms"] / (forwards + 1), 4)
    out["graph"]["ratio_to_eager"] = round(out["graph"]["median_ms"] / out["eager"]["median_ms"],
                                           3)
    return {"workload": f"Anat_CNN ResNet-10, 1 x {size}^3, {precision}, patch {patch}, stride "
                        f"{stride}, score prob: {n_win} windows, {forwards} forwards of 8 rows "
                        "(+ base forward; the graph side also pays 2 warm-up forwards and the "
                        "capture per call)",
            "rounds": rounds, "bit_identical": bool(torch.equal(a["maps"]["mri"],
                                                                b["maps"]["mri"])),
            "sides": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--model-calls", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--occlusion", action="store_true",
                    help="time explain.occlusion graph=True against graph=False only")
    ap.add_argument("--occ-size", type=int, default=128)
    ap.add_argument("--occ-patch", type=int, default=16)
    ap.add_argument("--occ-stride", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_explain.py needs a HIP device: a time is only measured on one")
    if a.occlusion:
        print(json.dumps({"occlusion": occlusion_times(a.rounds, a.precision, a.occ_patch,
                                                       a.occ_stride, a.occ_size)}))
        return
    res = {"kernel": [kernel_times(s, a.rounds, a.calls) for s in SHAPES]}
    if not a.skip_model:
        res["model"] = model_times(a.rounds, a.model_calls, a.precision)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
