#!/usr/bin/env python
"""Golden record of `muon.tl.umap`'s own code by EXECUTING the reference's `umap`
(/root/reference/muon/_core/tools.py:1209-1362) where it lies.

scanpy, umap-learn, numba and pynndescent are absent (not vendored, not installable: the layout's oracle stays unpinned),
but everything AROUND the layout is the reference's own code: the neighbours key, the `.obsp` slots handed on, the
keyword arguments that reach `sc.tl.umap`, the write-back of `X_umap` / `.uns["umap"]` into the MuData object, what
`copy` does and the `ValueError` text.  The file is loaded with the stubs of make_mofa_golden.py and RECORDING stand-ins
for `scanpy.tl.umap` (it writes a canned embedding and scanpy's documented `.uns["umap"]`) and
`scanpy.tools._utils._choose_representation`.  The MuData's modalities cover every observation, so the reference's
imputation line is not reached.

Second part: the trustworthiness (sklearn, 15 neighbours) of `tests/umap_refs.sequential_layout` - umap-learn's
published per-edge loop in plain Python - on the quality fixture of tests/umap_fixture.py for five seeds (about half a
minute each, which is why it runs here and not in a test).  tests/test_umap_host.py and tests/test_gpu_umap.py hold the
package's Jacobi form against the lowest of them.

Run (in the build container):  python tests/golden/make_umap_golden.py
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_mofa_golden as mofa_stubs  # noqa: E402
from make_cluster_golden import save_npz  # noqa: E402
from tests import umap_fixture as fx  # noqa: E402
from tests import umap_refs as R  # noqa: E402

LOG = {}


def _plain(v):
    if isinstance(v, np.ndarray):
        return {"ndarray": list(v.shape)}
    if isinstance(v, (np.integer,)):
        return int(v)
    if isinstance(v, (np.floating,)):
        return float(v)
    return v


def _sc_umap(adata, **kw):
    """scanpy.tl.umap: records what it is handed, writes a canned embedding and scanpy's documented parameters."""
    LOG["keywords"] = {k: _plain(kw[k]) for k in sorted(kw)}
    key = kw["neighbors_key"]
    LOG["adata_shape"] = list(adata.shape)
    LOG["adata_obsp_keys"] = sorted(adata.obsp)
    LOG["adata_uns_keys"] = sorted(adata.uns)
    LOG["adata_neighbors_params"] = {k: adata.uns[key]["params"][k] for k in sorted(adata.uns[key]["params"])}
    LOG["adata_neighbors_keys"] = {k: adata.uns[key][k] for k in ("connectivities_key", "distances_key")}
    LOG["obs_equal"] = bool(adata.obs.index.equals(LOG["mdata_obs"]))
    adata.obsm["X_umap"] = fx.golden_embedding(kw["n_components"])
    adata.uns["umap"] = {"params": {"a": 0.25, "b": 0.75}}
    if kw["random_state"] != 0:
        adata.uns["umap"]["params"]["random_state"] = kw["random_state"]


def _choose_representation(adata, use_rep=None, n_pcs=None, silent=False):
    LOG["representations"].append({"use_rep": use_rep, "n_pcs": n_pcs, "shape": list(adata.shape)})
    return adata.X


def load_reference():
    tools = mofa_stubs.load_reference_tools()
    sc = sys.modules["scanpy"]
    sc.tl = types.SimpleNamespace(umap=_sc_umap)
    sys.modules["scanpy.tools._utils"]._choose_representation = _choose_representation
    return tools


def record(tools, case):
    kw = dict(fx.GOLDEN_CASES[case])
    LOG.clear()
    LOG.update(representations=[])
    md = fx.golden_mudata()
    LOG["mdata_obs"] = md.obs.index
    try:
        out = tools.umap(md, **kw)
    except ValueError as e:
        return {"error": "ValueError", "message": str(e)}
    target = out if kw.get("copy") else md
    return {
        "returned": "copy" if out is not None else "None",
        "input_untouched": "X_umap" not in md.obsm and "umap" not in md.uns if kw.get("copy") else None,
        "keywords": LOG["keywords"],
        "adata_shape": LOG["adata_shape"],
        "adata_obsp_keys": LOG["adata_obsp_keys"],
        "adata_uns_keys": LOG["adata_uns_keys"],
        "adata_neighbors_params": LOG["adata_neighbors_params"],
        "adata_neighbors_keys": LOG["adata_neighbors_keys"],
        "obs_equal": LOG["obs_equal"],
        "representations": LOG["representations"],
        "X_umap_dtype": str(target.obsm["X_umap"].dtype),
        "X_umap_shape": list(target.obsm["X_umap"].shape),
        "X_umap_is_the_embedding": bool(np.array_equal(target.obsm["X_umap"],
                                                       fx.golden_embedding(LOG["keywords"]["n_components"]))),
        "uns_umap": target.uns["umap"],
    }


def sequential_trust():
    q = fx.QUALITY
    A = fx.quality_graph().tocoo()
    a, b = fx.AB
    out = []
    for seed in fx.QUALITY_SEEDS:
        Y = R.sequential_layout(fx.quality_initial(seed), A.row, A.col, A.data, q["n_epochs"], a, b, seed=seed)
        out.append(fx.trust(Y))
        print("sequential seed", seed, "trustworthiness %.6f" % out[-1], flush=True)
    return out


def main():
    tools = load_reference()
    out = {}
    for case in fx.GOLDEN_CASES:
        out[case] = np.array(json.dumps(record(tools, case), sort_keys=True))
        print(case, str(out[case])[:200])
    out["sequential_trust"] = np.asarray(sequential_trust(), dtype=np.float64)
    out["initial_trust"] = np.asarray([fx.trust(fx.quality_initial(s)) for s in fx.QUALITY_SEEDS], dtype=np.float64)
    path = os.path.join(HERE, "umap_golden.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
