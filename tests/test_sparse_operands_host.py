"""Which operands a sparse view gets (``_core.mofa_common.sparse_operands``) and which transposition a CSR gets
(``_operators.transposed_csr``), on a recording operator set: no GPU.

The table below restates the ladder ``MofaEngine._layout_view`` had before the chooser existed, for an operator set with
every layout operator (the product's) - it is not read off the chooser:

    f32 blocks, width 16, both dimensions > 0, max(shape) * 64 < 2^32    sliced ELL of X and of its tile-staged transpose
    f32 blocks, can_stream(X, 16)                                          transpose_stream(X), then stream(X)
    f64 blocks, width 16, both dimensions > 0, max(shape) * 128 < 2^32   ell16_pair(X, wide=True)
    f64 blocks, width <= 32, both dimensions > 0                          split_streams(X)
    otherwise                                                              transpose(X), and X itself
"""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from muon_amd._backend import HipBackend
from muon_amd._core.mofa_common import sparse_operands
from muon_amd._operators import transposed_csr

F32, F64 = torch.float32, torch.float64


def _x(shape, dtype, nnz=7):
    return SimpleNamespace(shape=shape, nnz=nnz, values=SimpleNamespace(dtype=dtype))


class Recording:
    """The layout operators as tagged tuples; ``calls``: their names in call order.  The two questions are the
    product's own (neither reads its ``self``): the limits are HipBackend's."""

    def __init__(self):
        self.calls = []

    def _tag(self, name, *what):
        self.calls.append(name)
        return (name,) + what

    def ell16_fits(self, X, wide):
        self.calls.append("ell16_fits")
        return HipBackend.ell16_fits(self, X, wide)

    def can_stream(self, X, B):
        self.calls.append("can_stream")
        return HipBackend.can_stream(self, X, B)

    def ell16_pair(self, X, wide=False):
        self.calls.append("ell16_pair")
        return ("ell16_pair", "X", X, wide), ("ell16_pair", "Xt", X, wide)

    def stream(self, X):
        return self._tag("stream", X)

    def transpose_stream(self, X):
        return self._tag("transpose_stream", X)

    def split_streams(self, X):
        self.calls.append("split_streams")
        return ("split_streams", "X", X), ("split_streams", "Xt", X)

    def transpose(self, X):
        return self._tag("transpose", X)


def _want(rung, X, wide):
    return {1: (("ell16_pair", "X", X, wide), ("ell16_pair", "Xt", X, wide)),
            2: (("stream", X), ("transpose_stream", X)),
            3: (("split_streams", "X", X), ("split_streams", "Xt", X)),
            4: (X, ("transpose", X))}[rung]


# (dtype of the blocks, padded width) -> (rung, calls in order) for a shape that every layout takes
TABLE = {
    (F32, 16): (1, ["ell16_fits", "ell16_pair"]),
    (F32, 32): (2, ["can_stream", "transpose_stream", "stream"]),
    (F32, 64): (2, ["can_stream", "transpose_stream", "stream"]),
    (F64, 16): (1, ["ell16_fits", "ell16_pair"]),
    (F64, 32): (3, ["split_streams"]),
    (F64, 64): (4, ["transpose"]),
}

IDS = [f"{str(t)[6:]}-{w}" for t, w in TABLE]


@pytest.mark.parametrize("dtype,width", list(TABLE), ids=IDS)
def test_the_table_of_rungs(dtype, width):
    rung, calls = TABLE[(dtype, width)]
    be, X = Recording(), _x((300, 200), dtype)
    got = sparse_operands(be, X, width, dtype)
    assert got == _want(rung, X, dtype == F64) and be.calls == calls


@pytest.mark.parametrize("dtype,row_bytes,rung,calls", [
    (F32, 64, 2, ["ell16_fits", "can_stream", "transpose_stream", "stream"]),
    (F64, 128, 3, ["ell16_fits", "split_streams"]),
], ids=["float32", "float64"])
@pytest.mark.parametrize("flip", [False, True], ids=["tall", "broad"])
def test_width_16_at_the_addressing_limit(dtype, row_bytes, rung, calls, flip):
    """The sliced-ELL kernels reach both dense blocks with 32-bit byte offsets: the longer dimension times the bytes of a
    16-column row stays under 2^32, for X and for X^T alike."""
    n = (1 << 32) // row_bytes
    for rows, want, order in ((n, rung, calls), (n - 1, 1, ["ell16_fits", "ell16_pair"])):
        assert (rows * row_bytes == 1 << 32) == (rows == n)
        be, X = Recording(), _x((5, rows) if flip else (rows, 5), dtype)
        got = sparse_operands(be, X, 16, dtype)
        assert got == _want(want, X, dtype == F64) and be.calls == order


@pytest.mark.parametrize("dtype,width", list(TABLE), ids=IDS)
@pytest.mark.parametrize("shape", [(0, 200), (300, 0), (0, 0)])
def test_a_zero_dimension_takes_the_csr(dtype, width, shape):
    be, X = Recording(), _x(shape, dtype, nnz=0)
    got = sparse_operands(be, X, width, dtype)
    assert got == (X, ("transpose", X)) and got[0] is X
    asked = (["ell16_fits"] if width == 16 else []) + (["can_stream"] if dtype == F32 else [])
    assert be.calls == asked + ["transpose"]


@pytest.mark.parametrize("dtype,width", list(TABLE), ids=IDS)
def test_a_set_without_optional_operators_takes_the_csr(dtype, width):
    from tests.cpu_backend import CpuTestBackend

    be = CpuTestBackend()
    m = sp.random(30, 20, density=0.2, random_state=0, format="csr", dtype=np.float64)
    X = be.upload_csr(m.indptr, m.indices, m.data, m.shape, values_dtype=np.float32 if dtype == F32 else np.float64)
    Xs, Xt = sparse_operands(be, X, width, dtype)
    assert Xs is X and Xt.shape == (20, 30)
    assert np.array_equal(be._sp(Xt).toarray(), be._sp(X).toarray().T)


class _Transposes:
    def __init__(self):
        self.calls = []

    def transpose(self, X):
        self.calls.append("transpose")
        return "general"


class _BothTransposes(_Transposes):
    def transpose_csr(self, X):
        self.calls.append("transpose_csr")
        return "tile-staged"


@pytest.mark.parametrize("be,dtype,nnz,want", [
    (_BothTransposes, F32, 7, "transpose_csr"),
    (_BothTransposes, F64, 7, "transpose"),
    (_BothTransposes, F32, 0, "transpose"),
    (_Transposes, F32, 7, "transpose"),
])
def test_transposed_csr_dispatch(be, dtype, nnz, want):
    be = be()
    got = transposed_csr(be, _x((300, 200), dtype, nnz=nnz))
    assert be.calls == [want] and got == {"transpose_csr": "tile-staged", "transpose": "general"}[want]
