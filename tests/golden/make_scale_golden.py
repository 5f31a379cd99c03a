"""Writes tests/golden/scale_golden.npz: scikit-learn's PCA of the dense clipped scaled matrix, for the end-to-end cases
of tests/scale_refs.py.

Run on the CPU from the repository root (scikit-learn 1.7.2):  python tests/golden/make_scale_golden.py

The input is rna_fixture's ``b16`` matrix (log-normalised, rounded to f32) with the crafted genes of
tests/scale_refs.py appended; it is scaled and clipped in f64 by ``scale_ref`` from numpy's own moments, and
``PCA(n_components=k, svd_solver="full")`` decomposes that dense matrix.  Stored: ``components_`` (f32 head + f16 tail,
as tests/golden/rna_golden.npz), ``explained_variance_``, ``explained_variance_ratio_``.  The script asserts what the
cases rest on: sigma_{k+1} / sigma_k below 0.6 with the crafted genes in place, entries clipped at both sides and a gene
whose z is itself clipped.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import rna_fixture as fx  # noqa: E402
from tests import scale_refs as sr  # noqa: E402


def main():
    import sklearn
    from sklearn.decomposition import PCA

    out = {}
    for name, c in sr.E2E_CASES.items():
        k = fx.CASES[c["base"]]["k"]
        M = sr.e2e_matrix(name)
        A = M.astype(np.float64).toarray()
        stored = np.zeros(A.shape, dtype=bool)
        stored[np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), M.indices] = True
        mean, std = sr.moments_ref(A)
        below, above, zclip = sr.clip_counts(A, stored, mean, std, c["max_value"])
        assert below > 0 and above > 0 and zclip > 0, (below, above, zclip)
        C = sr.e2e_clipped_dense(name)
        est = PCA(n_components=k, svd_solver="full").fit(C)
        sv = np.linalg.svd(C - C.mean(axis=0), compute_uv=False)
        ratio = sv[k] / sv[k - 1]
        print(f"{name}: {C.shape[0]} x {C.shape[1]}, k = {k}, max_value = {c['max_value']}, sigma_k+1 / sigma_k = "
              f"{ratio:.3f}, stored entries clipped below / above {below} / {above}, genes with a clipped z {zclip}")
        assert ratio < 0.6
        hi, lo = fx.split_store(est.components_)
        out[f"{name}/components_hi"], out[f"{name}/components_lo"] = hi, lo
        out[f"{name}/variance"] = est.explained_variance_.astype(np.float64)
        out[f"{name}/variance_ratio"] = est.explained_variance_ratio_.astype(np.float64)
    out["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(sr.GOLDEN, **out)
    print(f"wrote {sr.GOLDEN}: {os.path.getsize(sr.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
