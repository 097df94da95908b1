"""Host-side pin of the conv routing (no GPU, nothing is launched): the shape queries Python
sizes its buffers from reproduce tests/golden/conv_routes.json exactly, under the default
kernel-variant setting, under every run-time override and under the environment switches (each
in a child process of its own), a switch answers the same through its environment variable and
through its run-time name, csrc/switches.hip is the only reader of the environment, and a fused
dgrad + BN-sum call is refused wherever the kernel that would run the conv has no such
epilogue."""
import importlib.util
import json
import os
import re

import pytest

from multimodal_alzheimer_amd import _lib
from tests._variants import variants

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location(
        "make_conv_routes_golden", os.path.join(GOLDEN, "make_conv_routes_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from multimodal_alzheimer_amd import _build
        _build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def env_answers(lib):
    """the children's answers, one child per environment setting, asked once"""
    return _maker().env_answers()


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "conv_routes.json")) as f:
        return json.load(f)


def test_routes_match_snapshot(lib, env_answers, want):
    maker = _maker()
    assert tuple(want["fields"]) == maker.FIELDS
    got = maker.snapshot(lib, env_answers)
    assert sorted(got) == sorted(want["routes"])
    for label, rows in want["routes"].items():
        assert got[label] == rows, f"setting {label}"
    # the table is complete and the snapshot sees the routes: both dtypes of every case, and
    # overrides that move entries
    assert len(want["routes"]["default"]) == 2 * len(maker.cases())
    assert sum(1 for label, rows in want["routes"].items() if label != "default" and rows) >= 9
    for var, v in maker.ENV_SETTINGS:
        assert want["routes"][f"env:{var}={v}"], f"{var}={v} moves no entry"


def test_environment_and_run_time_name_agree(lib, env_answers, want):
    """a switch with a run-time name: the same entries move whether the value comes from the
    environment or from mmad_set_kernel_variant, the name reports the environment's value,
    and set(2) then set(previous) comes back to it -- also where that value is -1"""
    maker = _maker()
    snap = maker.snapshot(lib, env_answers)
    seen = 0
    for var, v in maker.ENV_SETTINGS:
        name = maker.RUNTIME_NAME.get(var)
        if name is None:
            continue
        label = f"env:{var}={v}"
        assert env_answers[label]["switch"] == [v, v, v], label
        if v >= 0:
            assert snap[label] == snap[f"{name}={v}"] == want["routes"][f"{name}={v}"], label
            seen += 1
    assert seen == 9
    assert env_answers["env:MMAD_LATTICE=-1"]["switch"] == [-1, -1, -1]
    assert lib.mmad_set_kernel_variant(b"stem", -1) == -1       # environment-only
    assert lib.mmad_set_kernel_variant(b"no_such_switch", 0) == -1
    assert lib.mmad_set_kernel_variant(None, 0) == -1


def test_switch_table_is_the_only_environment_reader():
    """getenv( occurs in csrc/ only in switches.hip, and every MMAD_* name its table carries
    occurs there exactly once: the 36 switches, each read in one place"""
    csrc = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))}
    assert [f for f, t in text.items() if "getenv(" in t] == ["switches.hip"]
    rows = re.findall(r'^\s*\{SW_(\w+), "(MMAD_\w+)", (?:"(\w+)"|nullptr), (-?\d+), (BOOL|INT)\},',
                      text["switches.hip"], re.M)
    assert len(rows) == 36 and all(env == "MMAD_" + sid for sid, env, _, _, _ in rows)
    for _, env, _, _, _ in rows:
        assert len(re.findall(rf"\b{env}\b", text["switches.hip"])) == 1, env
    assert sorted(n for _, _, n, _, _ in rows if n) == sorted(
        ["lattice", "lattice_zp", "lattice5", "lattice8", "lattice8_xwalk", "patchz", "pool_run",
         "pw_wg3_dedup"])
    maker = _maker()
    assert {var for var, _ in maker.ENV_SETTINGS} <= {env for _, env, _, _, _ in rows}


REFUSED = [
    # (variant, conv arguments): forced onto a kernel without the BN-sum epilogue
    ("patchz", ((8, 64, 32, 32, 32), (64, 64, 3, 3, 3), (1,) * 3, (1,) * 3, (1,) * 3)),
    ("lattice", ((2, 512, 23, 28, 23), (512, 512, 3, 3, 3), (1,) * 3, (4,) * 3, (4,) * 3)),
    ("lattice5", ((1, 512, 20, 20, 20), (512, 512, 3, 3, 3), (1,) * 3, (4,) * 3, (4,) * 3)),
]


@pytest.mark.parametrize("variant,args", REFUSED, ids=[r[0] for r in REFUSED])
def test_bnsum_refused_where_the_kernel_has_no_such_epilogue(lib, variant, args):
    """the z-walking patch conv, the ragged residue-class conv and the 5d^3 one write no
    BN-backward sums: the row query says -1 and the call returns MMAD_EUNSUPPORTED instead of
    launching a kernel that would leave the partial buffer unwritten (fake aligned pointers,
    never dereferenced)"""
    from multimodal_alzheimer_amd.volume_ops import conv_desc
    d = conv_desc(*args)
    with variants(**{variant: 2}):
        assert lib.mmad_conv3d_dgrad_bnsum_rows(d, _lib.BF16) == -1
        ptrs = [0x1000 * (i + 1) for i in range(9)]
        assert lib.mmad_conv3d_dgrad_bnsum(d, _lib.BF16, *ptrs, None) == _lib.EUNSUPPORTED
