#!/usr/bin/env python
"""Golden vectors for protein normalisation (dsb, clr) by EXECUTING the reference's own code.

/root/reference/muon/_prot/preproc.py is loaded where it lies, with the real scikit-learn, scipy and pandas of the
build image; only ``anndata`` / ``mudata`` (absent there) are stubbed with muon_amd._containers.  The script then runs
the reference's own ``dsb`` (:17-224) and ``clr`` (:227-299) and writes inputs and outputs to tests/golden/prot_golden.npz.
The reference does not exist on the GPU box: tests read only the fixture.

dsb cases (130 cells x 40 proteins, 600 empty droplets, integer seed):
  int_csr     integer counts, CSR, defaults                   f32_dense   float32 dense input
  meansub     scale_factor="mean_subtract"                    isotype     three isotype controls
  clip        quantile_clipping=True                          nodenoise   denoise_counts=False
  add_layer   add_layer=True                  - the generator asserts the layer EQUALS int_csr's X: stored once
  raw_none    data_raw=None with count ranges - built to select the same droplets in the same order; asserted equal to
              int_csr's result and stored once (the RNA row sums that drive the selection are stored)
Next to int_csr, f32_dense and meansub (isotype, clip, add_layer and raw_none fit the same scaled matrix with the same
seed as int_csr: its diagnostics are theirs): per cell and model (tied, full) ``n_iter_``, the BIC, and the background
mean, from the same two ``GaussianMixture`` fits on the reference's own scaled matrix (``denoise_counts=False`` of the
same call).  The
generator asserts that no fit hit ``max_iter``, that min |BIC_tied - BIC_full| > 1e-6 |BIC|, and that both models are
chosen at least once across the fixture.

clr: three flavours x two axes, sparse and dense.  With the installed scipy the ``csr_matrix`` / ``csc_matrix`` branch
of the reference's sparse ``seurat`` path fails (``logmean.A``: the attribute was removed from scipy's matrices), so the
sparse cases go through the ``csr_array`` / ``csc_array`` branch of the same statements (:281-285).

Run (in the build container):  python tests/golden/make_prot_golden.py
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd
import scipy.sparse as sp
from sklearn.mixture import GaussianMixture

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("MUON_REFERENCE", "/root/reference")

from muon_amd._containers import AnnData, MuData  # noqa: E402

N_CELLS, N_EMPTY, N_PROT, N_GENES = 130, 600, 40, 30
SEED = 7
ISOTYPES = ["prot5", "prot17", "prot31"]


def load_reference():
    for name, attrs in (("anndata", dict(AnnData=AnnData)), ("mudata", dict(MuData=MuData))):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("muon_prot_preproc", os.path.join(REF, "muon/_prot/preproc.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def synth(seed=0, n_cells=N_CELLS, n_empty=N_EMPTY, n_prot=N_PROT):
    """Counts of all droplets (empty droplets first): ambient noise everywhere, a per-cell subset of proteins strongly
    positive (negative binomial), cell-specific background level; RNA counts whose row sums separate the two groups."""
    rng = np.random.default_rng(seed)
    ambient = rng.gamma(2.0, 1.5, n_prot)
    empty = rng.poisson(ambient * rng.gamma(4.0, 0.25, (n_empty, 1)))
    level = rng.gamma(6.0, 1.0, (n_cells, 1))
    cells = rng.poisson(ambient * level)
    pos = rng.random((n_cells, n_prot)) < rng.uniform(0.1, 0.5, (n_cells, 1))
    cells = cells + pos * rng.negative_binomial(3, 3 / (3 + rng.uniform(80, 900, (n_cells, n_prot))))
    prot = np.vstack([empty, cells]).astype(np.int64)
    rna = np.vstack([rng.poisson(1.0, (n_empty, N_GENES)), rng.poisson(150.0, (n_cells, N_GENES))]).astype(np.int64)
    return prot, rna


def names(n, prefix):
    return pd.Index([f"{prefix}{i}" for i in range(n)], dtype=object)


def adata(x, obs_names, var_names):
    return AnnData(x, obs=pd.DataFrame(index=obs_names), var=pd.DataFrame(index=var_names))


def gmm_diagnostics(scaled, seed):
    n = scaled.shape[0]
    n_iter, bic, bg = np.zeros((n, 2), np.int32), np.zeros((n, 2)), np.zeros(n)
    for c in range(n):
        x = scaled[c, :, np.newaxis]
        lows = []
        for m, ct in enumerate(("tied", "full")):
            g = GaussianMixture(n_components=2, covariance_type=ct, init_params="random", random_state=seed).fit(x)
            assert g.converged_ and g.n_iter_ < g.max_iter, (c, ct)
            n_iter[c, m], bic[c, m] = g.n_iter_, g.bic(x)
            lows.append(np.min(g.means_))
        bg[c] = lows[0] if bic[c, 0] < bic[c, 1] else lows[1]  # (the reference's rule, :193-198)
    return n_iter, bic, bg


def main():
    ref = load_reference()
    warnings.simplefilter("ignore")
    out = {}
    prot, rna = synth()
    obs_all, var = names(N_EMPTY + N_CELLS, "d"), names(N_PROT, "prot")
    cell_names = obs_all[N_EMPTY:]
    out["prot_counts"] = prot.astype(np.int32)
    out["rna_rowsum"] = rna.sum(axis=1).astype(np.int64)
    out["seed"] = np.array([SEED])
    out["isotypes"] = np.array([int(s[4:]) for s in ISOTYPES])

    def inputs(kind):
        if kind == "f32_dense":
            cells, raw = prot[N_EMPTY:].astype(np.float32), prot.astype(np.float32)
        else:
            cells, raw = sp.csr_matrix(prot[N_EMPTY:]), sp.csr_matrix(prot)
        return adata(cells, cell_names, var), adata(raw, obs_all, var)

    cases = {
        "int_csr": {},
        "f32_dense": {},
        "meansub": dict(scale_factor="mean_subtract"),
        "isotype": dict(isotype_controls=ISOTYPES),
        "clip": dict(quantile_clipping=True),
        "nodenoise": dict(denoise_counts=False),
        "add_layer": dict(add_layer=True),
    }
    chosen = set()
    for tag, kw in cases.items():
        cells, raw = inputs(tag)
        ref.dsb(cells, raw, random_state=SEED, **kw)
        res = np.asarray(cells.layers["dsb"] if tag == "add_layer" else cells.X)
        if tag == "add_layer":
            assert sp.issparse(cells.X) and np.array_equal(res, out["dsb_int_csr"])
            continue
        out[f"dsb_{tag}"] = res
        if kw.get("denoise_counts", True) and tag in ("int_csr", "f32_dense", "meansub"):
            c2, r2 = inputs(tag)
            ref.dsb(c2, r2, random_state=SEED, denoise_counts=False, **{k: v for k, v in kw.items()})
            n_iter, bic, bg = gmm_diagnostics(np.asarray(c2.X), SEED)
            gap = np.abs(bic[:, 0] - bic[:, 1])
            assert gap.min() > 1e-6 * np.abs(bic).max(), gap.min()
            chosen |= set((bic[:, 0] < bic[:, 1]).tolist())
            out[f"dsb_{tag}_n_iter"], out[f"dsb_{tag}_bic"], out[f"dsb_{tag}_bg"] = n_iter, bic, bg
            print(tag, res.dtype, "n_iter max", n_iter.max(), "tied chosen", int((bic[:, 0] < bic[:, 1]).sum()), "of",
                  len(bg), "min |BIC gap| %.3g" % gap.min())
    assert chosen == {True, False}, chosen

    # data_raw=None: the unfiltered MuData with count ranges that select the same droplets in the same order
    md = MuData({"prot": adata(sp.csr_matrix(prot), obs_all, var),
                 "rna": adata(sp.csr_matrix(rna), obs_all, names(N_GENES, "g"))})
    ranges = dict(empty_counts_range=(0.5, 2.5), cell_counts_range=(3.0, 5.0))
    got = ref.dsb(md, random_state=SEED, **ranges)
    assert list(got.mod["prot"].obs_names) == list(cell_names)
    assert np.array_equal(np.asarray(got.mod["prot"].X), out["dsb_int_csr"])
    out["raw_none_ranges"] = np.array([0.5, 2.5, 3.0, 5.0])

    # clr
    rng = np.random.default_rng(11)
    xd = rng.poisson(6.0, (24, 10)).astype(np.float64)
    xd[rng.random(xd.shape) < 0.25] = 0.0
    xp = xd + 1.0  # (no zeros: `standard` stays finite)
    xp[3, 4] = 0.0  # ... but for one entry
    out["clr_x"], out["clr_xp"] = xd, xp
    for flavor in ("seurat", "stoeckius", "standard"):
        for axis in (0, 1):
            ad = AnnData((sp.csr_array(xd) if axis == 1 else sp.csc_array(xd)) if flavor == "seurat" else sp.csr_array(xd))
            ref.clr(ad, axis=axis, flavor=flavor)
            r = ad.X
            out[f"clr_sparse_{flavor}_{axis}"] = r.toarray() if sp.issparse(r) else np.asarray(r)
            ad = AnnData((xd if flavor != "standard" else xp).copy())
            ref.clr(ad, axis=axis, flavor=flavor)
            out[f"clr_dense_{flavor}_{axis}"] = np.asarray(ad.X)
    path = os.path.join(HERE, "prot_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 300 * 1024


if __name__ == "__main__":
    main()
