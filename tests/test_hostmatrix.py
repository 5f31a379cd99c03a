"""muon_amd._hostmatrix: the one acquire path (``device_copy``), the one way back (``host_view``) and the two small
shared lookups (``modality``, ``backend_or_default``), on the CPU test operator set with counted uploads."""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import scipy.sparse as sp

import muon_amd as mu
from muon_amd import _backend, _hostmatrix as H
from muon_amd._backend import backend_or_default
from muon_amd._containers import modality
from tests.cpu_backend import CpuTestBackend


class _Counting(CpuTestBackend):
    def __init__(self):
        self.uploads = 0

    def upload_csr(self, *a, **k):
        self.uploads += 1
        return super().upload_csr(*a, **k)


@pytest.fixture
def be():
    return _Counting()


@pytest.fixture
def no_default(monkeypatch):
    def boom():
        raise AssertionError("a default backend was constructed")

    monkeypatch.setattr(_backend, "get_backend", boom)


def _canonical(seed=0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    m = sp.random(40, 30, density=0.25, format="csr", random_state=rng, dtype=np.float64)
    m.data = (1 + rng.poisson(1.0, m.nnz)).astype(dtype)
    m.sort_indices()
    m.sum_duplicates()
    assert m.has_canonical_format and m.has_sorted_indices
    return m


def _unsorted(seed=0):
    m = _canonical(seed)
    out = sp.csr_matrix((m.data[::-1].copy(), m.indices[::-1].copy(),
                         np.concatenate([[0], np.cumsum(np.diff(m.indptr)[::-1])]).astype(m.indptr.dtype)), shape=m.shape)
    out.has_sorted_indices = False
    out.has_canonical_format = False
    return out


def test_a_valid_resident_copy_is_returned_without_an_upload(be, no_default):
    m = _canonical()
    X = be.upload_csr(m.indptr, m.indices, m.data, m.shape)
    H.attach_device(m, X, be)
    be.uploads = 0
    for host_route in (False, True):
        host, got, b = H.device_copy(m, None, host_route=host_route)  # backend=None: the copy's own backend
        assert host is m and got is X and b is be
        host, got, b = H.device_copy(m, be, host_route=host_route)
        assert host is m and got is X and b is be
    assert H.resident_copy(m) == (X, be) and H.resident_copy(m, be) == (X, be)
    assert be.uploads == 0


def test_host_route_without_a_copy_or_a_backend_touches_no_device(no_default):
    m = _canonical()
    host, X, b = H.device_copy(m, None, host_route=True)
    assert host is m and X is None and b is None
    u = _unsorted()
    host, X, b = H.device_copy(u, None, host_route=True)
    assert host is not u and X is None and b is None
    assert host.has_canonical_format and np.array_equal(host.toarray(), u.toarray())
    assert not hasattr(m, H.DEVICE_ATTR) and not hasattr(u, H.DEVICE_ATTR)
    assert H.resident_copy(m) == (None, None)


@pytest.mark.parametrize("host_route", [False, True])
def test_a_canonical_float_csr_is_uploaded_once_and_attached(be, no_default, host_route):
    m = _canonical()
    host, X, b = H.device_copy(m, be, host_route=host_route)
    assert host is m and b is be and be.uploads == 1
    assert getattr(m, H.DEVICE_ATTR)[0] is X and H.resident(m, be) is X
    assert np.array_equal(be.to_host(X.values), m.data) and np.array_equal(be.to_host(X.indices), m.indices)
    host, X2, b = H.device_copy(m, be, host_route=host_route)
    assert host is m and X2 is X and b is be and be.uploads == 1


def test_without_a_backend_argument_the_default_backend_uploads(be, monkeypatch):
    monkeypatch.setattr(_backend, "get_backend", lambda: be)
    m = _canonical()
    host, X, b = H.device_copy(m)
    assert host is m and b is be and be.uploads == 1 and H.resident(m, be) is X


@pytest.mark.parametrize("make", [_unsorted, lambda: _canonical(dtype=np.int32)], ids=["unsorted", "integer"])
def test_a_canonicalised_temporary_gets_the_copy_and_the_input_none(be, no_default, make):
    m = make()
    before = (m.data.copy(), m.indices.copy(), m.indptr.copy())
    host, X, b = H.device_copy(m, be)
    assert host is not m and b is be and be.uploads >= 1
    assert not hasattr(m, H.DEVICE_ATTR) and not hasattr(host, H.DEVICE_ATTR)
    assert host.has_canonical_format and host.has_sorted_indices
    assert host.dtype == (np.float64 if m.dtype == np.int32 else m.dtype)  # (integers widen like the reference's)
    assert np.array_equal(host.toarray(), m.toarray())
    assert np.array_equal(be.to_host(X.indices), host.indices) and np.array_equal(be.to_host(X.values), host.data)
    assert all(np.array_equal(a, b_) for a, b_ in zip(before, (m.data, m.indices, m.indptr)))  # the input is untouched


def test_an_edit_in_place_refuses_the_copy_and_removes_it(be, no_default):
    m = _canonical()
    H.device_copy(m, be)
    assert hasattr(m, H.DEVICE_ATTR) and be.uploads == 1
    m.data[7] += 1.0
    assert H.resident(m, be) is None and not hasattr(m, H.DEVICE_ATTR)
    host, X, b = H.device_copy(m, be)  # ... and the edited matrix is uploaded anew
    assert host is m and be.uploads == 2 and np.array_equal(be.to_host(X.values), m.data)


def test_a_copy_attached_under_another_backend_is_refused(be, no_default):
    m, other = _canonical(), _Counting()
    _host, X, _b = H.device_copy(m, other)
    assert H.resident(m, be) is None and H.resident_copy(m, be) == (None, be)
    assert H.resident(m, other) is X  # (refused, not dropped: its own backend still finds it)
    host, Y, b = H.device_copy(m, be)
    assert host is m and Y is not X and b is be and be.uploads == 1 and H.resident(m, be) is Y


def test_host_view_sets_the_flags_and_carries_the_copy(be):
    m = _canonical()
    X = be.upload_csr(m.indptr, m.indices, m.data, m.shape)
    view = H.host_view(X, be, canonical=True)
    assert view.has_sorted_indices and view._has_canonical_format is True
    assert H.resident(view, be) is X and (view != m).nnz == 0 and view.dtype == m.dtype
    assert not any(np.shares_memory(getattr(view, k), getattr(m, k)) for k in ("data", "indices", "indptr"))
    # host arrays that exist already are reused; without `canonical` only the order of the rows is vouched for
    view = H.host_view(X, be, indices=m.indices, indptr=m.indptr)
    assert view.has_sorted_indices and getattr(view, "_has_canonical_format", None) is None
    assert np.shares_memory(view.indices, m.indices) and np.shares_memory(view.indptr, m.indptr)
    assert not np.shares_memory(view.data, m.data) and np.array_equal(view.data, m.data)
    assert H.resident(view, be) is X


def test_modality_and_its_error_text():
    a, r = mu.AnnData(_canonical()), mu.AnnData(_canonical(1))
    assert modality(a, "atac") is a and modality(a, "rna") is a
    md = mu.MuData({"atac": a})
    assert modality(md, "atac") is a
    for data, name in ((md, "rna"), (mu.MuData({"rna": r}), "atac"), (object(), "atac"), (None, "rna")):
        with pytest.raises(TypeError) as e:
            modality(data, name)
        assert str(e.value) == f"Expected AnnData or MuData object with '{name}' modality"


def test_backend_or_default(be, monkeypatch):
    assert backend_or_default(be) is be
    other = _Counting()
    monkeypatch.setattr(_backend, "get_backend", lambda: other)
    assert backend_or_default(None) is other and backend_or_default(be) is be


def test_the_module_imports_no_operator_package():
    """Loaded on its own - under a second package name whose ``__init__`` imports nothing - the module brings in
    none of ``_atac`` / ``_core`` / ``_rna`` / ``_prot`` (``muon_amd/__init__`` itself imports them all)."""
    alias = "_muon_amd_alone"
    pkg = types.ModuleType(alias)
    pkg.__path__ = [os.path.dirname(mu.__file__)]
    sys.modules[alias] = pkg
    try:
        importlib.import_module(alias + "._hostmatrix")
        loaded = {k.split(".")[1] for k in sys.modules if k.startswith(alias + ".")}
        assert "_hostmatrix" in loaded and not loaded & {"_atac", "_core", "_rna", "_prot"}, loaded
    finally:
        for k in [k for k in sys.modules if k == alias or k.startswith(alias + ".")]:
            del sys.modules[k]
