"""The operands ``sparse_operands`` chooses on the product's operator set, on the GPU: their types, the same bits as the
layout operators called directly, and both products against f64 arithmetic with the bounds of tests/test_gpu_ell.py.

One matrix, 257 x 1025: one row past 16 groups of 16, one column past a 1024-column slab and past two 512-column slabs;
ragged rows, empty rows, a few rows hundreds of entries long and one row with every column stored (longer than a slab).
Its values are exact in f32 once, and once not (the f64 layouts then carry a lo part)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests.synth import planted_topics_csr

pytestmark = pytest.mark.gpu

N, D = 257, 1025
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def be():
    from muon_amd._backend import get_backend

    return get_backend()


@pytest.fixture(scope="module")
def matrices():
    """{exact: the f64 scipy matrix}; read-only."""
    m = planted_topics_csr(N, D, n_topics=5, density=0.04, seed=N).astype(np.float32)
    m.data = np.log1p(m.data).astype(np.float32) + np.float32(0.125)
    keep = np.ones(N)
    keep[::7] = 0          # empty rows
    heavy = sp.random(N, D, density=0.5, random_state=N, format="csr", dtype=np.float32)
    pick = np.zeros(N)
    pick[1::13] = 1        # a few rows hundreds of entries long
    full = sp.csr_matrix((np.linspace(0.5, 1.5, D, dtype=np.float32), (np.full(D, 100), np.arange(D))), shape=(N, D))
    m = sp.csr_matrix(sp.diags(keep) @ m + sp.diags(pick) @ heavy + full).astype(np.float32)
    m.eliminate_zeros()
    m.sort_indices()
    lens = np.diff(m.indptr)
    assert lens[0] == 0 and lens[100] == D > 1024 and lens.max() == D and 300 < lens[1] < D
    exact = m.astype(np.float64)
    inexact = exact.copy()
    inexact.data = inexact.data * (1.0 + 1e-9 * np.arange(1, m.nnz + 1))  # not representable in f32
    assert np.any(inexact.data != inexact.data.astype(np.float32))
    return {True: exact, False: inexact}


def _direct(be, X, dtype, width):
    """(Xs, Xt, the type of Xs and Xt, that of their hi part or None): the layout operators called one by one."""
    from muon_amd._backend import DeviceCSR, DeviceEll, DeviceStream, SplitOperand

    if (dtype, width) == (F32, 16):
        return be.ell16(X), be.ell16(be.transpose_csr(X)), DeviceEll, None
    if dtype == F32:
        return be.stream(X), be.transpose_stream(X), DeviceStream, None
    if width == 16:
        return be.ell16(X, wide=True), be.ell16(be.transpose(X), wide=True), SplitOperand, DeviceEll
    if width == 32:
        return be.split_streams(X) + (SplitOperand, DeviceStream)
    return X, be.transpose(X), DeviceCSR, None


CASES = [(F32, 16), (F32, 32), (F64, 16), (F64, 32), (F64, 64)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "inexact"])
@pytest.mark.parametrize("dtype,width", CASES, ids=[f"{str(t)[6:]}-{w}" for t, w in CASES])
def test_chosen_operands(be, matrices, dtype, width, exact):
    from muon_amd._core.mofa_common import sparse_operands

    npt = np.float32 if dtype == F32 else np.float64
    m = matrices[exact].astype(npt)  # (f32 blocks: the view is stored in f32, as MofaEngine stores it)
    X = be.upload_csr(m.indptr, m.indices, m.data, m.shape, values_dtype=npt)
    Xs, Xt = sparse_operands(be, X, width, dtype)
    Ds, Dt, kind, part = _direct(be, X, dtype, width)
    for got, shape in ((Xs, (N, D)), (Xt, (D, N))):
        assert type(got) is kind and got.shape == shape and got.nnz == m.nnz
        if part is not None:
            assert type(got.hi) is part and (got.lo is None) == exact
            assert got.lo is None or type(got.lo) is part
    if width == 16:
        slabs = 1024 if dtype == F32 else 512
        assert all((E if dtype == F32 else E.hi).slab_cols == slabs for E in (Xs, Xt))
    if kind.__name__ == "DeviceCSR":
        assert Xs is X

    rng = np.random.default_rng(width)
    Q, Y = rng.standard_normal((D, width)).astype(npt), rng.standard_normal((N, width)).astype(npt)
    m64, tol = m.astype(np.float64), 2e-6 if dtype == F32 else 1e-13
    for got, direct, op, B in ((Xs, Ds, m64, Q), (Xt, Dt, m64.T, Y)):
        Bd = torch.from_numpy(B).to(be.device)
        out = be.spmm(got, Bd)
        assert torch.equal(out, be.spmm(direct, Bd))
        want = op @ B.astype(np.float64)
        scale = abs(op) @ np.abs(B).astype(np.float64) + 1e-300
        err = float(np.max(np.abs(be.to_host(out).astype(np.float64) - want) / scale))
        print(f"sparse_operands {dtype} B={width} exact={exact} {tuple(op.shape)}: {err:.3e} of |X||Q| (bound {tol:g})")
        assert err < tol
