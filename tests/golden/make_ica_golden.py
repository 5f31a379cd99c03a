#!/usr/bin/env python
"""Golden vectors for muon.tl.ica by EXECUTING the reference's own code against the real scikit-learn.

/root/reference/muon/_core/tools.py is loaded where it lies (the loader of make_mofa_golden.py: stubs for the
third-party modules that file imports at its top and that are absent in the build image - anndata, mudata, scanpy,
h5py, natsort, mofapy2; scikit-learn is the real one), and its own ``ica`` (:1365-1386) runs on the seeded inputs of
tests/ica_fixture.py.  ``sklearn.decomposition.FastICA`` is wrapped in a recording subclass, so ``components_``,
``mean_``, ``whitening_`` and ``n_iter_`` of the very fit the reference ran are captured.  The ``lim`` trajectory is
captured by a recorded re-run of ``_ica_par``'s / ``_ica_def``'s statements (scikit-learn's own ``_sym_decorrelation``
and contrast functions) from the recorded whitening; the re-run must reproduce the recorded iteration count.

For every converging case the generator asserts last lim < 0.9 tol and the one before > 1.1 tol (per component for
deflation): "equal iteration counts" is then a fair condition for another summation order.

Stored: X_ica in full for the n = 1031 cases; for k33 / k64 components_, mean_, n_iter and every 37th row of X_ica (the
tests rebuild the rest as (X - mean_) @ components_.T).  k6_f32 stores scikit-learn's float32 result AND its result on
X.astype(float64): the package computes in f64 and is compared with the second.

Run (in the build container):  python tests/golden/make_ica_golden.py
"""
import io
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True  # (no __pycache__ beside the fixtures: tests/test_layout.py audits this directory)

import sklearn.decomposition  # noqa: E402
from sklearn.decomposition import _fastica as skf  # noqa: E402
from sklearn.exceptions import ConvergenceWarning  # noqa: E402

import ica_fixture as fx  # noqa: E402
import make_mofa_golden as stubs  # noqa: E402  (its loader of the reference's tools.py)
from muon_amd._containers import AnnData  # noqa: E402

TOL = 1e-4
RECORDS = []


class RecordingFastICA(skf.FastICA):
    def _fit_transform(self, X, compute_sources=False):
        S = super()._fit_transform(X, compute_sources=compute_sources)
        RECORDS.append(dict(components=self.components_.copy(), mean=self.mean_.copy(),
                            whitening=self.whitening_.copy(), n_iter=int(self.n_iter_)))
        return S


def trajectory(X, rec, kw):
    """lim after every iteration, from the recorded whitening: the statements of _ica_par (one list) or _ica_def (one
    list per component)."""
    n = X.shape[0]
    K = rec["whitening"]
    k = K.shape[0]
    X1 = np.dot(K, (X - rec["mean"]).T) * np.sqrt(n)
    w_init = np.asarray(np.random.RandomState(fx.SEED).normal(size=(k, k)), dtype=X1.dtype)
    g = {"logcosh": skf._logcosh, "exp": skf._exp, "cube": skf._cube}[kw.get("fun", "logcosh")]
    fun_args = kw.get("fun_args") or {}
    max_iter = kw.get("max_iter", 200)
    if kw.get("algorithm", "parallel") == "parallel":
        W = skf._sym_decorrelation(w_init)
        lims = []
        for _ in range(max_iter):
            gwtx, g_wtx = g(np.dot(W, X1), fun_args)
            W1 = skf._sym_decorrelation(np.dot(gwtx, X1.T) / float(n) - g_wtx[:, np.newaxis] * W)
            lims.append(max(abs(abs(np.einsum("ij,ij->i", W1, W)) - 1)))
            W = W1
            if lims[-1] < TOL:
                break
        return [lims]
    W = np.zeros((k, k))
    out = []
    for j in range(k):
        w = w_init[j, :].copy()
        w /= np.sqrt((w ** 2).sum())
        lims = []
        for _ in range(max_iter):
            gwtx, g_wtx = g(np.dot(w.T, X1), fun_args)
            w1 = (X1 * gwtx).mean(axis=1) - g_wtx.mean() * w
            skf._gs_decorrelation(w1, W, j)
            w1 /= np.sqrt((w1 ** 2).sum())
            lims.append(np.abs(np.abs((w1 * w).sum()) - 1))
            w = w1
            if lims[-1] < TOL:
                break
        W[j, :] = w
        out.append(lims)
    return out


def run(ref, X, kw):
    ad = AnnData(np.zeros((X.shape[0], 1)), obsm={"X_pca": X.copy()})
    del RECORDS[:]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert ref.ica(ad, random_state=fx.SEED, **kw) is None
    assert len(RECORDS) == 1
    warned = any(issubclass(w.category, ConvergenceWarning) for w in caught)
    return np.asarray(ad.obsm["X_ica"]), RECORDS[0], warned


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the file regenerates byte for byte."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    ref = stubs.load_reference_tools()
    sklearn.decomposition.FastICA = RecordingFastICA  # (the reference imports it from there inside ica())
    out = {}
    for case, (_name, f32, kw) in fx.CASES.items():
        X = fx.case_input(case)
        S, rec, warned = run(ref, X, kw)
        assert S.dtype == X.dtype
        if f32:
            out[f"{case}_X_ica_f32"] = S
            S, rec, warned = run(ref, X.astype(np.float64), kw)
            print(case, "sklearn float32 against its float64 run: max |dS| %.3g" % np.abs(out[f"{case}_X_ica_f32"] - S).max())
        fit_kw = {a: b for a, b in kw.items() if a != "scale"}
        lims = trajectory(X.astype(np.float64), rec, fit_kw)
        assert max(len(t) for t in lims) == rec["n_iter"], (case, [len(t) for t in lims], rec["n_iter"])
        if case in fx.NOT_CONVERGING:
            assert warned and rec["n_iter"] == kw["max_iter"] and lims[0][-1] > 1.1 * TOL, case
        else:
            assert not warned, case
            for t in lims:
                assert t[-1] < 0.9 * TOL and (len(t) == 1 or t[-2] > 1.1 * TOL), (case, t[-2:])
        out[f"{case}_n_iter"] = np.array([rec["n_iter"]])
        out[f"{case}_lim"] = np.array([t[-1] for t in lims])
        out[f"{case}_components"], out[f"{case}_mean"] = rec["components"], rec["mean"]
        out[f"{case}_whitening"] = rec["whitening"]
        if case in fx.SUBSAMPLED:
            out[f"{case}_X_ica_rows"] = S[::fx.ROW_STEP]
            assert np.array_equal(fx.rebuild(out, case, X)[::fx.ROW_STEP] != 0, S[::fx.ROW_STEP] != 0)
        else:
            out[f"{case}_X_ica"] = S
        print(case, S.shape, S.dtype, "n_iter", rec["n_iter"], "last lims", ["%.3g" % v for v in lims[0][-2:]],
              "max |S| %.3g" % np.abs(S).max())
    path = os.path.join(HERE, "ica_golden.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1000 * 1024


if __name__ == "__main__":
    main()
