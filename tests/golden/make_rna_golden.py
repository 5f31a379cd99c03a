"""Writes tests/golden/rna_golden.npz: scikit-learn's answer for every case of tests/rna_fixture.py.

Run on the CPU from the repository root (scikit-learn 1.7.2):  python tests/golden/make_rna_golden.py

The inputs are regenerated, log-normalised in f64 and densified by tests/rna_fixture.py; this script runs
``PCA(n_components=k, svd_solver="full")`` on the centred (and scaled) matrix, or ``TruncatedSVD(algorithm="arpack")``
on the uncentred one, and stores ``components_``, ``explained_variance_`` and ``explained_variance_ratio_`` only.  It
prints the ratio sigma_{k+1} / sigma_k of every case: the cases cut the spectrum at its gap.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import rna_fixture as fx  # noqa: E402


def main():
    import sklearn
    from sklearn.decomposition import PCA, TruncatedSVD

    out = {}
    for name, c in fx.CASES.items():
        A = fx.prepared_dense(name)
        k = c["k"]
        if c["zero_center"]:
            est = PCA(n_components=k, svd_solver="full").fit(A)
        else:
            est = TruncatedSVD(n_components=k, algorithm="arpack", tol=1e-12, random_state=0).fit(A)
        sv = np.linalg.svd(A, compute_uv=False)
        print(f"{name}: {A.shape[0]} x {A.shape[1]}, k = {k}, sigma_k+1 / sigma_k = {sv[k] / sv[k - 1]:.3f}, "
              f"closest pair inside the top k {np.min(1 - sv[1:k] / sv[:k - 1]):.2e}")
        hi, lo = fx.split_store(est.components_)
        out[f"{name}/components_hi"], out[f"{name}/components_lo"] = hi, lo
        out[f"{name}/variance"] = est.explained_variance_.astype(np.float64)
        out[f"{name}/variance_ratio"] = est.explained_variance_ratio_.astype(np.float64)
    out["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(fx.GOLDEN, **out)
    print(f"wrote {fx.GOLDEN}: {os.path.getsize(fx.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
