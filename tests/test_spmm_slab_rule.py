"""Which Q slab width a row-stream product runs with (muon_amd._backend.spmm_slab_cols): 320 columns where the library
has such an instance - f32 blocks of 64 columns on a layout of 6 .. 8 row-sets per wave -, 256 everywhere else; the tune
key spmm_slab forces a width where an instance exists and is never an error where none does.  No GPU: the library's
query and its tune table work without a device."""
import pytest
import torch

from muon_amd import _ffi
from muon_amd._backend import SLAB_NARROW, SLAB_WIDE, HipBackend, spmm_slab_cols


@pytest.fixture()
def lib():
    lib = _ffi.lib()
    yield lib
    lib.mu_tune_set(b"spmm_slab", 0)
    lib.mu_tune_set(b"spmm_k", 0)


def test_widths_are_what_the_kernel_file_declares():
    assert (SLAB_NARROW, SLAB_WIDE) == (256, 320)


@pytest.mark.parametrize("B", [16, 32, 64])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_default_rule(lib, B, K):
    want = 320 if (B == 64 and K >= 6) else 256
    assert spmm_slab_cols(lib, B, K, torch.float32) == want
    assert lib.mu_spmm_stream_slab_ok(B, K, 320) == int(want == 320)
    assert lib.mu_spmm_stream_slab_ok(B, K, 256) == 1
    assert spmm_slab_cols(lib, B, K, torch.float64) == 256  # the f64 blocks keep their 256-column slabs


@pytest.mark.parametrize("B,K,want320", [(64, 6, 320), (64, 8, 320), (64, 5, 256), (32, 8, 256), (16, 6, 256)])
def test_forced_widths_and_the_fallback(lib, B, K, want320):
    assert spmm_slab_cols(lib, B, K, torch.float32, force=256) == 256
    assert spmm_slab_cols(lib, B, K, torch.float32, force=320) == want320
    assert spmm_slab_cols(lib, B, K, torch.float64, force=320) == 256
    with pytest.raises(ValueError):
        spmm_slab_cols(lib, B, K, torch.float32, force=288)


def test_query_rejects_other_widths_and_shapes(lib):
    ok = lib.mu_spmm_stream_slab_ok
    assert ok(64, 6, 288) == 0 and ok(64, 6, 512) == 0 and ok(64, 6, 0) == 0
    assert ok(64, 0, 256) == 0 and ok(64, 9, 320) == 0 and ok(48, 6, 256) == 0


def test_backend_reads_the_tune_keys(lib):
    """HipBackend.spmm_slab: the K in effect is the tune key spmm_k where set, else the layout's, else the library's
    choice for the row count; spmm_slab forces the width.  (No device: the methods only read the library.)"""
    be = HipBackend.__new__(HipBackend)
    be.lib = lib
    assert be.spmm_slab(6, 10 ** 6, 64) == 320 and be.spmm_slab(5, 10 ** 6, 64) == 256
    assert be.spmm_slab(7, 10 ** 6, 32) == 256 and be.spmm_slab(7, 10 ** 6, 64, torch.float64) == 256
    assert be.spmm_slab_ranged(7) == 320 and be.spmm_slab_ranged(4) == 256
    assert lib.mu_tune_set(b"spmm_slab", 256) == 0
    assert be.spmm_slab(6, 10 ** 6, 64) == 256 and be.spmm_slab_ranged(8) == 256
    assert lib.mu_tune_set(b"spmm_slab", 320) == 0
    assert be.spmm_slab(6, 10 ** 6, 64) == 320 and be.spmm_slab(4, 10 ** 6, 64) == 256
    assert be.spmm_slab_ranged(7) == 320 and be.spmm_slab_ranged(8) == 320 and be.spmm_slab_ranged(5) == 256
    assert lib.mu_tune_set(b"spmm_slab", 0) == 0
    assert lib.mu_tune_set(b"spmm_k", 4) == 0  # a forced K of 4 has no wide instance, whatever the layout says
    assert be.spmm_slab(6, 10 ** 6, 64) == 256
    assert lib.mu_tune_set(b"spmm_k", 8) == 0
    assert be.spmm_slab(1, 3000, 64) == 320
    assert be.spmm_slab_ranged(1) == 256  # (the ranged entry runs the layout's K as it is)
    assert lib.mu_tune_set(b"spmm_k", 0) == 0


def test_ablation_modes_keep_the_narrow_slab(lib):
    """The timing ablations (tune key spmm_mode) are 256-column instances; only the cycle accounting at K = 8 exists
    at both widths.  A product with a mode set must run what it ran before the wide instances existed."""
    be = HipBackend.__new__(HipBackend)
    be.lib = lib
    try:
        for mode in (1, 9, 128, 192):
            assert lib.mu_tune_set(b"spmm_mode", mode) == 0
            assert [be.spmm_slab(K, 10 ** 6, 64) for K in (6, 7, 8)] == [256, 256, 256]
        assert lib.mu_tune_set(b"spmm_mode", 64) == 0
        assert [be.spmm_slab(K, 10 ** 6, 64) for K in (6, 7, 8)] == [256, 256, 320]
        assert lib.mu_tune_set(b"spmm_slab", 320) == 0
        assert [be.spmm_slab(K, 10 ** 6, 64) for K in (6, 7, 8)] == [256, 256, 320]
        assert lib.mu_tune_set(b"spmm_slab", 256) == 0 and be.spmm_slab(8, 10 ** 6, 64) == 256
    finally:
        lib.mu_tune_set(b"spmm_mode", 0)
    assert spmm_slab_cols(lib, 64, 8, torch.float32, mode=64, ranged=True) == 256
