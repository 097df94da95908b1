"""Snapshot of the conv library's host-side routing answers (no GPU needed).

    python tests/golden/make_conv_routes_golden.py

writes tests/golden/conv_routes.json: for every (descriptor, dtype) of the table below, under
the default kernel-variant setting, under each run-time override and under each environment
switch of ENV_SETTINGS (answered by a fresh child process that has the variable set: a switch
is read once per process), the numbers Python sizes its buffers from -- BN partial rows of the
forward and of the fused dgrad, the weight-gradient workspace, the packed-weight sizes of both
directions and whether the stem reads the raw volume.  tests/test_conv_routes_cpu.py asserts the built library still gives exactly these, so
regenerate the file only from a build whose routes are known good (the commit before a routing
change), never to make that test pass.
"""
import concurrent.futures as cf
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "conv_routes.json")

BATCHES = (1, 2, 8)
CUBES = (32, 64, 96, 128, 160)
VARIANTS = ("lattice", "lattice8", "lattice5", "lattice_zp", "patchz")
# environment switches (csrc/switches.hip) and values that move at least one entry; the ones
# with a run-time name (RUNTIME_NAME) must move the same entries as that name does
ENV_SETTINGS = (
    ("MMAD_STEM", 0), ("MMAD_PATCH", 0), ("MMAD_PATCH_TZ4", 1), ("MMAD_S2CONV", 0),
    ("MMAD_PW_GEMM", 0), ("MMAD_PWGRAD", 0), ("MMAD_PWGRAD_W40", 0), ("MMAD_PWGRAD_LAT_NG", 1),
    ("MMAD_LATTICE_RAGGED", 0), ("MMAD_PW_WGRAD", 0),
    ("MMAD_WGRAD_BIG", 1), ("MMAD_WGRAD_SPLITS", 1), ("MMAD_WGRAD_SPLITS", 2),
    ("MMAD_WGRAD_1X1_SPLITS", 2),
    ("MMAD_IGEMM_BIG", 1), ("MMAD_IGEMM_BIG", -1), ("MMAD_IGEMM_BIG_MINBLK", 0),
    ("MMAD_STEM_WG2", 0), ("MMAD_STEM_QUAD", 0),
    ("MMAD_LATTICE", 0), ("MMAD_LATTICE", 2), ("MMAD_LATTICE", -1),
    ("MMAD_LATTICE8", 0), ("MMAD_LATTICE8", 2), ("MMAD_LATTICE5", 0), ("MMAD_LATTICE5", 2),
    ("MMAD_LATTICE_ZP", 0), ("MMAD_PATCHZ", 0), ("MMAD_PATCHZ", 2),
)
RUNTIME_NAME = {"MMAD_LATTICE": "lattice", "MMAD_LATTICE8": "lattice8",
                "MMAD_LATTICE5": "lattice5", "MMAD_LATTICE_ZP": "lattice_zp",
                "MMAD_PATCHZ": "patchz"}
CHILDREN = 8                      # child processes at a time
FIELDS = ("stats_rows", "dgrad_bnsum_rows", "wgrad_workspace", "packed_fwd", "packed_dgrad",
          "stem_raw_ok")


def _conv(n, ci, e, co, k, s, p, dil):
    """(xshape, wshape, stride, padding, dilation) of a cubic conv; e: one extent or three"""
    ext = (e, e, e) if isinstance(e, int) else tuple(e)
    return ((n, ci) + ext, (co, ci, k, k, k), (s,) * 3, (p,) * 3, (dil,) * 3)


def cases():
    """name -> conv arguments: the MedicalNet ResNet convs per (batch, cube), then two ragged
    MNI-derived grids"""
    out = {}
    for n in BATCHES:
        for c in CUBES:
            e1 = (c // 2 + 2 - 3) // 2 + 1      # after the stride-2 stem and the 3 / 2 / 1 pool
            e2 = (e1 + 2 - 3) // 2 + 1          # after layer2's stride-2 conv
            t = f"n{n}c{c}_"
            out[t + "stem"] = _conv(n, 1, c, 64, 7, 2, 3, 1)
            out[t + "l1"] = _conv(n, 64, e1, 64, 3, 1, 1, 1)
            out[t + "l2c1"] = _conv(n, 64, e1, 128, 3, 2, 1, 1)
            out[t + "l2sc"] = _conv(n, 64, e1, 128, 1, 2, 0, 1)
            out[t + "l2"] = _conv(n, 128, e2, 128, 3, 1, 1, 1)
            out[t + "l3c1"] = _conv(n, 128, e2, 256, 3, 1, 2, 2)
            out[t + "l3sc"] = _conv(n, 128, e2, 256, 1, 1, 0, 1)
            out[t + "l3"] = _conv(n, 256, e2, 256, 3, 1, 2, 2)
            out[t + "l4c1"] = _conv(n, 256, e2, 512, 3, 1, 4, 4)
            out[t + "l4sc"] = _conv(n, 256, e2, 512, 1, 1, 0, 1)
            out[t + "l4"] = _conv(n, 512, e2, 512, 3, 1, 4, 4)
    out["mni_l4"] = _conv(2, 512, (23, 28, 23), 512, 3, 1, 4, 4)
    out["mni_l1"] = _conv(2, 64, (46, 55, 46), 64, 3, 1, 1, 1)
    return out


def settings():
    """(label, variant name or None, value)"""
    yield "default", None, 0
    for name in VARIANTS:
        for v in (0, 2):
            yield f"{name}={v}", name, v


def query(lib, L, conv_desc):
    """name_dtype -> the six answers, under the library's current variant setting"""
    out = {}
    for name, args in cases().items():
        d = conv_desc(*args)
        for tag, dt in (("bf16", L.BF16), ("f32", L.F32)):
            out[f"{name}_{tag}"] = [
                lib.mmad_conv3d_stats_rows(d, dt),
                lib.mmad_conv3d_dgrad_bnsum_rows(d, dt),
                lib.mmad_conv3d_wgrad_workspace(d, dt),
                lib.mmad_conv_packed_elems(d, dt, 0),
                lib.mmad_conv_packed_elems(d, dt, 1),
                max(lib.mmad_stem_raw_ok(d, L.F32, dt), 2 * lib.mmad_stem_raw_ok(d, L.F64, dt)),
            ]
    return out


def child():
    """what a child process prints: query()'s answers under the environment it was started
    with and, for a run-time name in argv, [the switch's value, what set(name, 2) returned,
    the value after putting that back]"""
    sys.path.insert(0, REPO)
    from multimodal_alzheimer_amd import _lib as L
    from multimodal_alzheimer_amd.volume_ops import conv_desc
    lib = L.load()
    out = {"routes": query(lib, L, conv_desc)}
    for name in sys.argv[1:]:
        was = lib.mmad_set_kernel_variant(name.encode(), -1)
        prev = lib.mmad_set_kernel_variant(name.encode(), 2)
        lib.mmad_set_kernel_variant(name.encode(), prev)
        out["switch"] = [was, prev, lib.mmad_set_kernel_variant(name.encode(), -1)]
    print(json.dumps(out))


def ask_child(var, v):
    """child()'s answers from a fresh process started with var=v in its environment"""
    code = (f"import sys; sys.path.insert(0, {HERE!r}); "
            "import make_conv_routes_golden as m; m.child()")
    names = [RUNTIME_NAME[var]] if var in RUNTIME_NAME else []
    r = subprocess.run([sys.executable, "-c", code, *names], env={**os.environ, var: str(v)},
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{var}={v}: child failed\n{r.stderr}")
    return json.loads(r.stdout.splitlines()[-1])


def env_answers():
    """"env:MMAD_X=v" -> child()'s answers, for every ENV_SETTINGS entry"""
    with cf.ThreadPoolExecutor(max_workers=CHILDREN) as ex:
        got = list(ex.map(lambda s: ask_child(*s), ENV_SETTINGS))
    return {f"env:{var}={v}": g for (var, v), g in zip(ENV_SETTINGS, got)}


def snapshot(lib, env=None):
    """{"default": every entry, "<variant>=<v>" and "env:MMAD_X=<v>": the entries that differ
    from the default}; every override is put back to what it was.  env: env_answers()'s
    result where the caller already has it"""
    from multimodal_alzheimer_amd import _lib as L
    from multimodal_alzheimer_amd.volume_ops import conv_desc
    from tests._variants import variants
    snap = {}
    for label, name, v in settings():
        if name is None:
            snap[label] = query(lib, L, conv_desc)
            continue
        with variants(**{name: v}):
            got = query(lib, L, conv_desc)
        snap[label] = {k: r for k, r in got.items() if r != snap["default"][k]}
    for label, got in (env_answers() if env is None else env).items():
        snap[label] = {k: r for k, r in got["routes"].items() if r != snap["default"][k]}
    return snap


def main():
    sys.path.insert(0, REPO)
    from multimodal_alzheimer_amd import _lib as L
    snap = snapshot(L.load())
    with open(OUT, "w") as f:
        json.dump({"fields": FIELDS, "routes": snap}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    for label, rows in snap.items():
        print(f"{label}: {len(rows)} entries")


if __name__ == "__main__":
    main()
