#!/usr/bin/env python
"""Golden record of `muon.tl.leiden` / `muon.tl.louvain`'s own code by EXECUTING the reference's `_cluster`
(/root/reference/muon/_core/tools.py:928-1054) where it lies.

leidenalg, louvain, igraph and scanpy are absent (not vendored, not installable: the optimiser's oracle stays unpinned),
but everything AROUND the optimiser is the reference's own code: which resolution each partition is handed, the
`layer_weights`, that no `weights=` reaches a partition, the seeding call, and the write-back of a membership into
`.obs` / `.uns`.  The file is loaded with the stubs of make_mofa_golden.py and RECORDING stand-ins for leidenalg /
louvain (`RBConfigurationVertexPartition`, `Optimiser`), scanpy's `_choose_graph` and `get_igraph_from_adjacency`; the
optimiser stand-in hands back a canned membership (14 communities, so the numeric order of the categories differs from
the lexicographic one) and a canned improvement.  `natsorted` sorts the digit strings by value, as natsort does.

tests/test_cluster_host.py compares `muon_amd._core.cluster`'s argument resolution and write-back with this record.

Run (in the build container):  python tests/golden/make_cluster_golden.py
"""
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_mofa_golden as mofa_stubs  # noqa: E402
from tests.cluster_fixture import GOLDEN_CASES as CASES, GOLDEN_IMPROVEMENT as IMPROVEMENT  # noqa: E402
from tests.cluster_fixture import golden_membership as membership, golden_mudata as mudata  # noqa: E402

def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the file regenerates byte for byte."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


LOG = {}


class _Graph:
    def __init__(self, adjacency, directed):
        self.adjacency, self.directed = adjacency, directed


class _Partition:
    def __init__(self, graph, **kw):
        self.graph = graph
        self.membership = None
        LOG["partitions"].append({"directed": bool(graph.directed), "nnz": int(graph.adjacency.nnz),
                                  "keywords": {k: kw[k] for k in sorted(kw)}})


class _Optimiser:
    def set_rng_seed(self, seed):
        LOG["seed_calls"].append(seed)

    def optimise_partition_multiplex(self, partitions, layer_weights=None, **kw):
        LOG["layer_weights"] = None if layer_weights is None else list(layer_weights)
        LOG["optimiser_keywords"] = {k: kw[k] for k in sorted(kw)}
        for p in partitions:
            p.membership = membership()
        return IMPROVEMENT


def _choose_graph(adata, obsp, neighbors_key):
    """scanpy.tools._utils._choose_graph for obsp=None: the connectivities of the neighbours slot."""
    assert obsp is None
    key = "connectivities" if neighbors_key is None else adata.uns[neighbors_key]["connectivities_key"]
    LOG["graph_keys"].append(key)
    return adata.obsp[key]


def load_reference():
    tools = mofa_stubs.load_reference_tools()
    for name in ("leidenalg", "louvain"):
        m = types.ModuleType(name)
        m.RBConfigurationVertexPartition = _Partition
        m.Optimiser = _Optimiser
        sys.modules[name] = m
    sys.modules["scanpy.tools._utils"]._choose_graph = _choose_graph
    u = types.ModuleType("scanpy._utils")
    u.get_igraph_from_adjacency = lambda adjacency, directed=None: _Graph(adjacency, directed)
    sys.modules["scanpy._utils"] = u
    tools.natsorted = lambda xs: sorted(xs, key=int)  # natsort's order for strings of digits
    return tools


def record(tools, case):
    kw = dict(CASES[case])
    algorithm = kw.pop("algorithm")
    LOG.clear()
    LOG.update(partitions=[], seed_calls=[], graph_keys=[])
    md = mudata()
    try:
        out = getattr(tools, algorithm)(md, **kw)
    except KeyError as e:
        return {"error": "KeyError", "key": e.args[0]}
    assert out is None
    key = kw.get("key_added", algorithm)
    col = md.obs[key]
    return {
        "partitions": LOG["partitions"],
        "layer_weights": LOG["layer_weights"],
        "optimiser_keywords": LOG["optimiser_keywords"],
        "seed_calls": LOG["seed_calls"],
        "graph_keys": LOG["graph_keys"],
        "obs_key": key,
        "obs_dtype": str(col.dtype),
        "obs_categories": [str(x) for x in col.cat.categories],
        "obs_values": [str(x) for x in col.to_numpy()],
        "uns_key": algorithm,
        "uns": md.uns[algorithm],
    }


def main():
    tools = load_reference()
    out = {}
    for case in CASES:
        out[case] = np.array(json.dumps(record(tools, case), sort_keys=True))
    out["membership"] = np.asarray(membership(), dtype=np.int64)
    out["improvement"] = np.asarray(IMPROVEMENT)
    path = os.path.join(HERE, "cluster_golden.npz")
    save_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
