"""csrc/rank.hip on the GPU: the per-group moments and the Wilcoxon rank sums against dense numpy / scipy.stats.rankdata
on the matrix of tests/rank_fixture.py (rows at the chunk, cap and piece edges), and rank_genes_groups end to end on a
resident matrix against tests/rank_refs.py.

Bounds: on the integer matrix every sum, count, rank sum (multiples of 0.5 below 2^24) and tie term is exact in f64, so
equality is asked.  On the non-integer matrix the sums differ from numpy's by the order of at most 1100 additions:
rtol 1e-12 > 1100 * 2^-53 = 1.2e-13.  End to end the host formulas are the restatement's on exact sums: rtol 1e-10 covers
the summation inside scipy."""
import functools

import numpy as np
import pytest
import torch

from muon_amd import atac as ac
from muon_amd._atac import rank as R
from muon_amd._hostmatrix import attach_device, resident, upload_canonical
from tests import rank_fixture as F
from tests import rank_refs

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]


@functools.lru_cache(maxsize=None)
def _dense(dtype, variant="int"):
    return F.matrices(dtype, variant)[0].toarray()


@functools.lru_cache(maxsize=None)
def _want_moments(dtype, variant, name):
    lab, B = F.labels(name)
    return rank_refs.group_moments(_dense(dtype, variant), lab, B)


@functools.lru_cache(maxsize=None)
def _want_ranks(variant, name):
    lab, B = F.labels(name)
    return rank_refs.rank_sums(_dense("float64", variant), lab, B)


def _device_t(hip, dtype, variant="int"):
    _, Xt = F.matrices(dtype, variant)
    return hip.upload_csr(Xt.indptr, Xt.indices, Xt.data, Xt.shape, slab_ptr=False)


def test_limits(hip):
    assert hip.group_moments_max_groups() == 64
    assert hip.rank_row_cap() == F.ROW_CAP
    Xt = _device_t(hip, "float32")
    with pytest.raises(ValueError):
        hip.group_moments(Xt, hip.to_device(F.labels("g65")[0], np.int32), 65)


@pytest.mark.parametrize("name", F.LABEL_VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_moments_are_numpys_exactly(hip, dtype, name):
    lab, B = F.labels(name)
    Xt = _device_t(hip, dtype)
    lab_d = hip.to_device(lab, np.int32)
    got = [hip.to_host(t) for t in hip.group_moments(Xt, lab_d, B)]
    again = [hip.to_host(t) for t in hip.group_moments(Xt, lab_d, B)]
    assert got[0].dtype == np.float64 and got[1].dtype == np.float64 and got[2].dtype == np.int64
    for g, w in zip(got, _want_moments(dtype, "int", name)):
        assert g.shape == w.shape and np.array_equal(g, w)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("name", F.LABEL_VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_group_moments_of_non_integer_values(hip, dtype, name):
    lab, B = F.labels(name)
    Xt = _device_t(hip, dtype, "frac")
    lab_d = hip.to_device(lab, np.int32)
    got = [hip.to_host(t) for t in hip.group_moments(Xt, lab_d, B)]
    again = [hip.to_host(t) for t in hip.group_moments(Xt, lab_d, B)]
    ws, wss, wnz = _want_moments(dtype, "frac", name)
    np.testing.assert_allclose(got[0], ws, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[1], wss, rtol=1e-12, atol=0)
    assert np.array_equal(got[2], wnz)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.parametrize("variant", ["int", "frac"])
@pytest.mark.parametrize("name", F.LABEL_VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_sums_are_rankdatas_exactly(hip, dtype, name, variant):
    """(``skip``: ranks over the kept cells only; ``frac``: an all-equal column and a tie run of 300 across chunks)"""
    lab, B = F.labels(name)
    Xs = R.sort_rows_by_value(_device_t(hip, dtype, variant))
    lab_d = hip.to_device(lab, np.int32)
    rs, zr, tie = (hip.to_host(t) for t in hip.rank_sums(Xs, lab_d, B))
    again = [hip.to_host(t) for t in hip.rank_sums(Xs, lab_d, B)]
    nz = _want_moments("float64", variant, name)[2]
    n_b = np.bincount(lab[lab >= 0], minlength=B)
    wrs, wtie = _want_ranks(variant, name)
    assert np.array_equal(rs + (n_b[None, :] - nz) * zr[:, None], wrs)
    assert np.array_equal(tie, wtie)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((rs, zr, tie), again))


def test_kernels_and_tensor_formulation_agree(hip):
    lab, B = F.labels("skip")
    Xt = _device_t(hip, "float32")
    lab_d = hip.to_device(lab, np.int32)
    for a, b in zip(hip.group_moments(Xt, lab_d, B), R._moments_tensor(Xt, lab_d, B)):
        assert torch.equal(a, b)
    Xs = R.sort_rows_by_value(Xt)
    rs, zr, tie = hip.rank_sums(Xs, lab_d, B)
    trs, tzr, ttie = R._rank_sums_tensor(Xs, lab_d, B)
    assert torch.equal(rs, trs) and torch.equal(zr, tzr) and torch.equal(tie, ttie)


@pytest.mark.parametrize("case", list(F.CASES))
def test_end_to_end_on_the_resident_matrix(hip, case, monkeypatch):
    kw = dict(F.CASES[case])
    ad = F.anndata("float32" if len(case) % 2 else "float64", base=kw.pop("base", None))
    host, Xd = upload_canonical(hip, ad.X)
    assert host is ad.X
    attach_device(ad.X, Xd, hip)
    uploads = []
    monkeypatch.setattr(hip, "upload_csr", lambda *a, **k: uploads.append(1))
    ac.tl.rank_genes_groups(ad, "leiden", backend=hip, **kw)
    F.compare(ad.uns["rank_genes_groups"], F.expected(case), full="n_genes" not in kw)
    assert not uploads and resident(ad.X, hip) is Xd


def test_a_host_matrix_is_uploaded_once_and_stays(hip):
    ad = F.anndata("float32")
    ac.tl.rank_peaks_groups(ad, "leiden", method="wilcoxon", tie_correct=True, pts=True)
    F.compare(ad.uns["rank_genes_groups"], F.expected("wilcoxon-tie"))
    assert "genes" not in ad.uns["rank_genes_groups"]
    ent = getattr(ad.X, "_muon_amd_device", None)
    assert ent is not None and ent[0].values.is_cuda
