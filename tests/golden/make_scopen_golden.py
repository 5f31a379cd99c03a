#!/usr/bin/env python
"""Golden vectors for atac.pp.scopen by EXECUTING the reference's own code.

/root/reference/muon/_atac/preproc.py:155-236 (``scopen``) is loaded where it lies, with stubs for the third-party
modules the file imports at its top (anndata, mudata -> muon_amd._containers; scanpy._utils.view_to_actual) and for
``scopen.MF``, which is absent here and not installable.  The stand-in ``non_negative_factorization`` is the project's
code and states which solver the fixture pins:

  * it records the dense d x n matrix the reference hands it (so ``rho`` and the binarisation are the reference's);
  * ``W0, H0 = sklearn.decomposition._nmf._initialize_nmf(X, k, "nndsvd", random_state=0)``;
  * the loop of ``_fit_coordinate_descent`` through scikit-learn's own ``_update_coordinate_descent`` with
    ``l2_reg_W = l2_reg_H = alpha`` and ``l1 = 0`` (the unscaled convention of scikit-learn <= 0.24, which scOpen's MF
    module copied), recording the violation ratio after every iteration;
  * it asserts that ``_fit_coordinate_descent`` itself returns the same W, H and n_iter.

Everything after the call - the clipped product, the write-back - is the reference's statements again.  Per case the
fixture holds W0, H0, W, H, n_iter, the ratios, rho and every ROW_STEP-th row of the imputed matrix (an array bit-equal
to one of an earlier case is stored once, see main()); the inputs come from the seeded generator in
tests/scopen_fixture.py.  For every converging case the deciding ratios are asserted to lie
MARGIN away from the tolerance on either side, so that "the same number of iterations" is a fair condition for an
implementation whose iterates differ by rounding.

Run (in the build container):  python tests/golden/make_scopen_golden.py      (regenerates the file byte for byte)
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("MUON_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True  # (no __pycache__ beside the fixtures: tests/test_layout.py audits this directory)
from sklearn.decomposition import _nmf  # noqa: E402

import scopen_fixture as fx  # noqa: E402
from muon_amd._containers import AnnData, MuData, view_to_actual  # noqa: E402

RECORD = {}


def non_negative_factorization(X, n_components, alpha, max_iter, verbose=0):
    X = np.ascontiguousarray(X, dtype=np.float64)
    W0, H0 = _nmf._initialize_nmf(X, n_components, "nndsvd", random_state=0)
    W0, H0 = np.array(W0, order="C"), np.array(H0, order="C")  # (copies: the loop below works in place)
    W, Ht = W0.copy(), np.array(H0.T, order="C")
    ratios, violation_init, n_iter = [], 0.0, 0
    for n_iter in range(1, max_iter + 1):
        violation = _nmf._update_coordinate_descent(X, W, Ht, 0.0, float(alpha), False, None)
        violation += _nmf._update_coordinate_descent(X.T, Ht, W, 0.0, float(alpha), False, None)
        if n_iter == 1:
            violation_init = violation
        if violation_init == 0:
            break
        ratios.append(violation / violation_init)
        if ratios[-1] <= fx.TOL:
            break
    W2, H2, n2 = _nmf._fit_coordinate_descent(X, W0.copy(), H0.copy(), tol=fx.TOL, max_iter=max_iter, l1_reg_W=0,
                                              l1_reg_H=0, l2_reg_W=float(alpha), l2_reg_H=float(alpha), update_H=True,
                                              verbose=0, shuffle=False, random_state=None)
    assert n2 == n_iter and np.array_equal(W2, W) and np.array_equal(H2, Ht.T)
    RECORD.update(X=X, W0=W0, H0=H0, n_iter=n_iter, ratios=np.asarray(ratios))
    return W, np.ascontiguousarray(Ht.T), n_iter


def load_reference():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    mod("anndata", AnnData=AnnData)
    mod("mudata", MuData=MuData)
    mod("scanpy")
    mod("scanpy._utils", view_to_actual=view_to_actual)
    mod("scopen")
    mod("scopen.MF", non_negative_factorization=non_negative_factorization)
    muon = mod("muon")
    muon.__path__ = [os.path.join(REF, "muon")]
    atac = mod("muon._atac")
    atac.__path__ = [os.path.join(REF, "muon", "_atac")]
    spec = importlib.util.spec_from_file_location("muon._atac.preproc", os.path.join(REF, "muon/_atac/preproc.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["muon._atac.preproc"] = m
    spec.loader.exec_module(m)
    return m


def main():
    ref = load_reference()
    out = {}
    for case in fx.CASES:
        data, adata, kw = fx.case_data(case)
        RECORD.clear()
        with contextlib.redirect_stdout(io.StringIO()):  # (the reference prints its progress)
            ref.scopen(data, **kw)
        W, Ht, X_imp = np.asarray(adata.varm["scopen"]), np.asarray(adata.obsm["X_scopen"]), np.asarray(adata.X)
        n_iter, ratios = RECORD["n_iter"], RECORD["ratios"]
        s = RECORD["X"].max(axis=0)  # every cell has an open peak: the column's maximum is its scale 1 / (1 - rho)
        assert np.array_equal(RECORD["X"], (fx.counts(fx.CASES[case][0]).T > 0) * s)
        rho = 1 - 1 / s  # (the reference keeps rho to itself; this is its value to an ulp)
        assert np.array_equal(X_imp, np.clip(W @ Ht.T, 0, 1).T)
        converging = n_iter < kw.get("max_iter", 500)
        if converging:
            assert ratios[-1] < (1 - fx.MARGIN) * fx.TOL and ratios[-2] > (1 + fx.MARGIN) * fx.TOL, (case, ratios[-2:])
        out[f"{case}_W0"], out[f"{case}_H0"] = RECORD["W0"], RECORD["H0"]
        out[f"{case}_W"], out[f"{case}_H"] = W, np.ascontiguousarray(Ht.T)
        out[f"{case}_n_iter"], out[f"{case}_ratios"], out[f"{case}_rho"] = np.array([n_iter]), ratios, rho
        out[f"{case}_X_rows"] = X_imp[::fx.ROW_STEP].copy()
        print(case, "n_iter", n_iter, "converging", converging, "last ratios / tol", ratios[-2:] / fx.TOL,
              "max W", W.max(), "max H", Ht.max())
    # an array bit-equal to one stored before (k6's results for the same pattern in another form; W0 / H0 of the cases
    # that differ in the solver's arguments only) is stored as that array's NAME: scopen_fixture.load_gold resolves it
    seen, packed = {}, {}
    for key, arr in out.items():
        arr = np.asarray(arr)
        sig = (arr.dtype.str, arr.shape, arr.tobytes())
        if arr.nbytes > 1024 and sig in seen:
            packed[key + "_same_as"] = np.asarray(seen[sig])
        else:
            seen.setdefault(sig, key)
            packed[key] = arr
    path = os.path.join(HERE, "scopen_golden.npz")
    np.savez_compressed(path, **packed)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
