#!/usr/bin/env python
"""Golden vectors for muon.tl.snf by EXECUTING the reference's own code.

/root/reference/muon/_core/tools.py is loaded where it lies (the loader of make_mofa_golden.py: stubs for the
third-party modules that file imports at its top; scipy - ``scipy.stats.norm`` is the only third-party arithmetic of
``snf`` - is the real one) and its own ``snf`` (:716-920) runs on the seeded MuData objects of tests/snf_fixture.py.
The dense fused W is captured by wrapping the module's ``_sparse_csr_fast_knn``: the argument of its second call is
``csr_matrix(W)``.

For every case the generator asserts that
  * the numpy statements of tests/snf_fixture.py reproduce the reference's W to 1e-13 element-wise (they are what the
    kernel tests compare with);
  * in every row of both final selections and in every column of every dominate-set selection the k-th and the
    (k+1)-th value are at least 1e-7 apart, relatively, and neighbouring selected values of a row at least 1e-11:
    "identical index sets in identical order" is then a fair condition for another summation order (the arithmetic
    deviation is 2e-15).

Stored per case: both graphs in full, the written ``.uns`` record as JSON, every 8th row of W.

Run (in the build container):  python tests/golden/make_snf_golden.py
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True  # (no __pycache__ beside the fixtures: tests/test_layout.py audits this directory)

import snf_fixture as fx  # noqa: E402
import make_mofa_golden as stubs  # noqa: E402  (its loader of the reference's tools.py)

SELECTION_GAP = 1e-7
NEIGHBOUR_GAP = 1e-11  # ten times the value bound of the tests: an order inside a selection cannot flip within it


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the file regenerates byte for byte."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def selection_gaps(values: np.ndarray, k: int):
    """Of an ascending vector: (relative gap between the k-th and the (k+1)-th value, smallest relative gap between
    neighbouring values among the first k).  inf where there is no (k+1)-th value."""
    cut = (values[k] - values[k - 1]) / abs(values[k]) if values.size > k else np.inf
    sel = values[:k]
    inner = np.min(np.diff(sel) / np.abs(sel[1:])) if k > 1 else np.inf
    return cut, inner


def main():
    ref = stubs.load_reference_tools()
    captured = []
    original = ref._sparse_csr_fast_knn

    def recording(X, n_neighbors):
        captured.append(X.toarray())
        return original(X, n_neighbors)

    ref._sparse_csr_fast_knn = recording
    out = {}
    for case, c in fx.CASES.items():
        md = fx.mudata(case)
        del captured[:]
        assert ref.snf(md, **fx.call_kwargs(case)) is None
        assert len(captured) == 2
        W = captured[1]
        n, k, M = c["n"], c["k"], c["M"]
        assert W.shape == (n, n) and np.array_equal(W, W.T) and np.array_equal(0.5 - W, captured[0])

        # the numpy restatement (tests/snf_fixture.py) against the executing reference
        wall = [fx.np_normalize(fx.np_affinity(fx.distances(fx.coordinates(case, m)), k, c["sigma"])) for m in range(M)]
        dom_gap = np.inf
        for w in wall:
            for j in range(n):
                dom_gap = min(dom_gap, selection_gaps(np.sort(-w[:, j]), k)[0])  # descending: the k largest are kept
        new = [fx.np_dominateset(w, k) for w in wall]
        for _ in range(c["it"]):
            nxt = [new[j] @ (sum(wall[i] for i in range(M) if i != j) / (M - 1)) @ new[j].T for j in range(M)]
            wall = [fx.np_normalize(x) for x in nxt]
        mine = fx.np_normalize(np.sum(wall, axis=0) / M)
        restated = float(np.max(np.abs(mine - W) / np.abs(W)))
        assert restated <= 1e-13, (case, restated)

        key, dk, ck = fx.slot_names(case)
        cut_gap = inner_gap = np.inf
        for A in (0.5 - W, W):
            for i in range(n):
                row = np.sort(A[i][A[i] != 0])
                cut, inner = selection_gaps(row, k)
                cut_gap, inner_gap = min(cut_gap, cut), min(inner_gap, inner)
        print(f"{case}: restated against the reference {restated:.3g}; smallest gaps: final selections {cut_gap:.3g}, "
              f"inside a selection {inner_gap:.3g}, dominate sets {dom_gap:.3g}")
        assert cut_gap >= SELECTION_GAP and dom_gap >= SELECTION_GAP and inner_gap >= NEIGHBOUR_GAP, case

        for name, slot in (("distances", dk), ("connectivities", ck)):
            g = md.obsp[slot]
            assert g.shape == (n, n) and np.array_equal(np.diff(g.indptr), np.full(n, k))
            out[f"{case}_{name}_data"] = np.asarray(g.data, dtype=np.float64)
            out[f"{case}_{name}_indices"] = np.asarray(g.indices, dtype=np.int32)
            out[f"{case}_{name}_indptr"] = np.asarray(g.indptr, dtype=np.int32)
        out[f"{case}_params"] = np.array(fx.params_json(md.uns[key]))
        out[f"{case}_W_rows"] = W[::fx.ROW_STEP]
    path = os.path.join(HERE, "snf_golden.npz")
    save_npz(path, out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1000 * 1024


if __name__ == "__main__":
    main()
