"""The one way a test flips a run-time kernel switch (mmad_set_kernel_variant; the names are in
INTEGRATION.md's switch table)."""
import contextlib

from multimodal_alzheimer_amd import _lib


@contextlib.contextmanager
def variants(**modes):
    """mmad_set_kernel_variant(name, mode) for the block, which gets the previous modes by
    name; those are put back afterwards"""
    lib = _lib.load()
    prev = {}
    try:
        for k, v in modes.items():
            prev[k] = lib.mmad_set_kernel_variant(k.encode(), v)
            assert prev[k] >= 0, f"unknown kernel variant {k}"
        yield prev
    finally:
        for k, v in prev.items():
            lib.mmad_set_kernel_variant(k.encode(), v)
