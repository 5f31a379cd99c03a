"""muon.tl.mofa on MI355X.

Host side mirrors /root/reference/muon/_core/tools.py:52-287 (`_set_mofa_data_from_mudata`)
and :290-708 (`mofa`): same 40-keyword signature, same validation errors, same write-back
into ``.obsm["X_mofa"]``, ``.varm["LFs"]`` and ``.uns["mofa"]``.  The training itself
(`ent.build(); ent.run()`, :583-585, third-party mofapy2) is replaced by
``mofa_engine.MofaEngine``: HIP kernels for the factor / weight sweeps and the sparse
products, PyTorch-ROCm for the dense blocks.

Deliberate deviations, all explicit:
  * sparse modalities are NOT densified (tools.py:117-141 does ``.todense()``);
  * poisson / bernoulli views, element-wise NaN and ``spikeslab_factors=True`` run on the general engine
    (``_needs_general_engine``); SVI raises NotImplementedError;
  * MEFISTO (``smooth_covariate``) runs on ``mefisto.SmoothMofaEngine`` (one covariance over all samples, a lengthscale
    grid of our own: parity with mofapy2 unpinned); its warping, sparse-GP and group-kernel options raise
    NotImplementedError (``_smooth_options``);
  * a bad ``groups_label`` raises ValueError where the reference calls ``sys.exit()`` (:106-113);
  * the model file is HDF5 (mofapy2's layout) when h5py is importable; otherwise ``outfile`` +
    ".npz" (NumPy archive, with a warning); results reach the write-back directly, not through it.
"""
from __future__ import annotations

import logging
import os
from functools import reduce
from time import strftime
from typing import Any, Iterable, List, Mapping, Optional, Union
from warnings import warn

import numpy as np
import pandas as pd
import torch
from scipy.sparse import csr_matrix, issparse

from .._backend import backend_or_default
from .._containers import MuData, is_anndata, is_mudata
from .ica import ConvergenceWarning, ica  # noqa: F401  (mu.tl.ica: FastICA of an embedding on the device)
from .pca import pca  # noqa: F401  (scanpy's pca on the device CSR: block Lanczos on the implicitly centred operator)
from .snf import snf  # noqa: F401  (mu.tl.snf: similarity network fusion on the device)
from .cluster import leiden, louvain  # noqa: F401  (mu.tl.leiden / mu.tl.louvain: multiplex clustering on the device)
from .umap import umap  # noqa: F401  (mu.tl.umap: the layout of the multimodal neighbourhood graph on the device)

logger = logging.getLogger("muon_amd")


def _guess_likelihood(x) -> str:
    """mofapy2.build_model.utils.guess_likelihoods semantics (tools.py:272-273): binary ->
    bernoulli, integer -> poisson, otherwise gaussian."""
    v = x.data if issparse(x) else np.asarray(x)
    v = v[~np.isnan(v)] if v.dtype.kind == "f" else v
    if v.size and np.all(np.isin(v, (0, 1))):
        return "bernoulli"
    if v.size and np.all(v == np.round(v)):
        return "poisson"
    return "gaussian"


def _collect_views(mdata, groups_label, use_raw, use_layer, likelihoods, features_subset, use_obs):
    """`_set_mofa_data_from_mudata` (tools.py:52-287) without densification."""
    obs_names = mdata.obs.index.values
    mods = list(mdata.mod.keys())
    if use_obs == "intersection":
        common = reduce(np.intersect1d, [v.obs_names.values for v in mdata.mod.values()])
        # `mdata = mdata[common_obs]` in the reference (:99-101): np.intersect1d SORTS, so the samples of the model
        # are in sorted name order - found by executing the reference (tests/golden/make_mofa_golden.py); r03 kept
        # mdata's order, which changes which sample gets which row of the seeded initialisation
        obs_names = np.asarray(common)

    if groups_label is not None:
        if not isinstance(groups_label, str):
            raise ValueError("groups_label should be a string present in the observations column names")
        if groups_label not in mdata.obs.columns:
            raise ValueError("{} is not in observations names".format(groups_label))

    views = []
    for m in mods:
        adata = mdata.mod[m]
        if use_layer:
            if use_layer not in adata.layers:
                raise ValueError("Layer {} does not exist".format(use_layer))
            x = adata.layers[use_layer]
        elif use_raw:
            if getattr(adata, "raw", None) is None:
                raise ValueError(f"modality {m} has no .raw")
            x = adata.raw[:, adata.var_names].X
        else:
            x = adata.X
        # place this modality's samples into the common sample axis (union expands with missing)
        pos = pd.Index(obs_names).get_indexer(adata.obs_names)
        have = pos >= 0
        n = len(obs_names)
        if issparse(x):
            x = x.tocsr()[np.nonzero(have)[0]]
            coo = x.tocoo()
            rows = pos[have][coo.row]
            full = csr_matrix((coo.data, (rows, coo.col)), shape=(n, x.shape[1]))
            missing = np.ones(n, dtype=bool)
            missing[pos[have]] = False
            full._missing_rows = missing if missing.any() else None
            x = full
        else:
            full = np.full((n, np.asarray(x).shape[1]), np.nan)
            full[pos[have]] = np.asarray(x, dtype=np.float64)[have]
            x = full
        if features_subset is not None:
            if features_subset not in adata.var.columns:
                raise KeyError(f"There is no column {features_subset} in .var for modality {m}")
            sel = np.asarray(adata.var[features_subset].values).astype(bool)
            miss = getattr(x, "_missing_rows", None)
            x = x[:, sel] if not issparse(x) else x[:, np.nonzero(sel)[0]]
            if issparse(x):
                x._missing_rows = miss
        views.append(x)

    guessed = likelihoods is None
    if guessed:
        likelihoods = [_guess_likelihood(v) for v in views]
    assert len(likelihoods) == len(views), "Please specify one likelihood for each view"
    assert set(likelihoods).issubset({"gaussian", "bernoulli", "poisson"}), \
        "Available likelihoods are 'gaussian', 'bernoulli', 'poisson'"
    # (r03: poisson / bernoulli views and element-wise NaN run through _core/mofa_general.py - the
    #  guessed likelihoods are the ones the model is fitted with, as in the reference; r02 fitted
    #  guessed count likelihoods as gaussian with a warning)

    obs = mdata.obs.loc[obs_names]
    if groups_label is None:
        groups = np.zeros(len(obs_names), dtype=np.int64)
        group_names = ["group1"]
    else:
        labels = obs[groups_label].astype(str).values
        group_names = list(pd.unique(labels))  # order of first appearance (groupby sort=False)
        groups = pd.Index(group_names).get_indexer(labels).astype(np.int64)
    return views, groups, group_names, obs_names, likelihoods


def _has_elementwise_nan(v) -> bool:
    """NaN entries that are not whole missing samples (those are row masks: use_obs='union')."""
    if issparse(v):
        return bool(np.isnan(v.data).any())
    a = np.isnan(np.asarray(v))
    return bool((a.any(axis=1) & ~a.all(axis=1)).any())


def _needs_general_engine(backend, views, lik, groups, n_factors, spikeslab_factors, comm=None) -> bool:
    """True iff the fit goes to GeneralMofaEngine rather than the two-pass MofaEngine: pseudo-data likelihoods or
    element-wise missing values (element-wise precisions, walked in row chunks; the sparse modalities stay CSR on the
    device), and the model options the two-pass engine's kernels are not instantiated for - more than 32 factors
    (tools.py:298 takes any int), more than 64 stacked (group, factor) columns against a sparse view,
    spikeslab_factors=True (tools.py:305,486), more views x groups x factors than the sweeps' LDS tile holds
    (two_pass_fits) - the same model on the general engine's chunk passes (slower: those are rare settings).
    One decision of all ranks: the group count is the maximum over ``comm`` and a shard that needs the general engine
    decides for every rank (an engine per rank would issue different collectives and hang the fit)."""
    from .._comm import default_comm
    from .mofa_engine import two_pass_fits

    comm = default_comm(comm)
    K = int(n_factors)
    n_groups = int(np.max(groups)) + 1 if len(groups) else 1
    local = (any(l != "gaussian" for l in lik) or any(_has_elementwise_nan(v) for v in views)
             or bool(spikeslab_factors))
    if comm.world_size > 1:
        t = torch.tensor([n_groups, int(local)], dtype=torch.int64)
        if backend.name == "hip":
            t = t.to(backend.device)
        n_groups, local = (int(x) for x in comm.all_reduce_max(t).tolist())
    wide = n_groups * K > 64 and any(issparse(v) for v in views)
    return bool(local) or wide or not two_pass_fits(len(views), n_groups, K)


# the reference's defaults of smooth_kwargs (/root/reference/muon/_core/tools.py:531-545; ``covariates_names`` defaults to
# ``smooth_covariate`` itself)
SMOOTH_DEFAULTS = dict(scale_cov=False, start_opt=20, n_grid=20, opt_freq=10, model_groups=True, warping_freq=20,
                       warping_ref=0, warping_open_begin=True, warping_open_end=True, sparseGP=False, frac_inducing=None,
                       new_values=None)


def _smooth_options(smooth_covariate, smooth_warping, smooth_kwargs):
    """The MEFISTO options as the reference merges them (tools.py:531-562): ``smooth_kwargs`` over the defaults, plus
    ``warping``.  None without ``smooth_covariate``: the reference then ignores the other two (:564)."""
    if smooth_covariate is None:
        return None
    opts = {"covariates_names": smooth_covariate, **SMOOTH_DEFAULTS, **dict(smooth_kwargs or {})}
    opts["warping"] = smooth_warping
    return opts


def _smooth_new_values(opts):
    """``new_values`` as the reference hands them to ``predict_factor`` (tools.py:587-597): [P, C], a 1-d list as one
    column; None when there is nothing to interpolate."""
    nv = opts["new_values"]
    if nv is None or len(nv) == 0:
        return None
    nv = np.array(nv, dtype=np.float64)
    return nv.reshape(-1, 1) if nv.ndim == 1 else nv


def _check_smooth_options(opts, n_groups, spikeslab_factors, comm):
    """What of MEFISTO is not built raises, naming the option."""
    from .._comm import default_comm

    if opts["warping"]:
        raise NotImplementedError("smooth_warping=True (aligning the covariate across groups) is not implemented")
    if opts["sparseGP"]:
        raise NotImplementedError("smooth_kwargs['sparseGP']=True (inducing points) is not implemented")
    if opts["frac_inducing"] is not None:
        raise NotImplementedError("smooth_kwargs['frac_inducing'] (inducing points) is not implemented")
    if opts["model_groups"] and n_groups > 1:
        raise NotImplementedError("smooth_kwargs['model_groups']=True with more than one group (a group kernel) is not "
                                  "implemented: pass model_groups=False for one covariance over all samples")
    if default_comm(comm).world_size > 1:
        raise NotImplementedError("smooth_covariate runs on one rank")
    if spikeslab_factors:
        raise ValueError("spikeslab_factors=True cannot be combined with smooth_covariate (the factors' prior is the "
                         "Gaussian process)")


def _smooth_covariates(obs, obs_names, smooth_covariate, opts):
    """(covariates [N, C] f64 in the model's sample order, their names, (mean, std) of ``scale_cov`` or None)."""
    cols = [smooth_covariate] if isinstance(smooth_covariate, str) else list(smooth_covariate)
    for c in cols:
        if c not in obs.columns:
            raise KeyError(f"smooth_covariate: there is no column {c!r} in .obs")
    names = opts["covariates_names"]
    names = [names] if isinstance(names, str) else [str(n) for n in names]
    if len(names) != len(cols):
        raise ValueError(f"covariates_names has {len(names)} entries for {len(cols)} covariates")
    try:
        cov = np.column_stack([np.asarray(obs.loc[obs_names, c].values, dtype=np.float64) for c in cols])
    except (TypeError, ValueError) as e:
        raise ValueError(f"smooth_covariate: the columns {cols} must be numeric ({e})") from None
    if not np.isfinite(cov).all():
        raise ValueError(f"smooth_covariate: the columns {cols} hold NaN or infinite values")
    scaling = None
    if opts["scale_cov"]:
        mean, std = cov.mean(axis=0), cov.std(axis=0)
        std = np.where(std > 0, std, 1.0)
        cov, scaling = (cov - mean) / std, (mean, std)
    return cov, names, scaling


def _mofa_engine(backend, views, lik, groups, n_factors, spikeslab_factors, **kw):
    """The engine of a Gaussian or pseudo-data fit (_needs_general_engine decides which); ``kw`` goes to its
    constructor (``comm``, ``row_offset``, ``n_total`` among them)."""
    if _needs_general_engine(backend, views, lik, groups, n_factors, spikeslab_factors, kw.get("comm")):
        from .mofa_general import GeneralMofaEngine

        return GeneralMofaEngine(backend, views, list(lik), groups, n_factors, spikeslab_factors=bool(spikeslab_factors),
                                 **kw)
    from .mofa_engine import MofaEngine

    return MofaEngine(backend, views, groups, n_factors, **kw)


def mofa(
    data,
    groups_label: bool = None,
    use_raw: bool = False,
    use_layer: str = None,
    use_var: Optional[str] = "highly_variable",
    use_obs: Optional[str] = None,
    likelihoods: Optional[Union[str, List[str]]] = None,
    n_factors: int = 10,
    scale_views: bool = False,
    scale_groups: bool = False,
    center_groups: bool = True,
    ard_weights: bool = True,
    ard_factors: bool = True,
    spikeslab_weights: bool = True,
    spikeslab_factors: bool = False,
    n_iterations: int = 1000,
    convergence_mode: str = "fast",
    use_float32: bool = False,
    gpu_mode: bool = False,
    gpu_device: Optional[bool] = None,
    svi_mode: bool = False,
    svi_batch_size: float = 0.5,
    svi_learning_rate: float = 1.0,
    svi_forgetting_rate: float = 0.5,
    svi_start_stochastic: int = 1,
    smooth_covariate: Optional[str] = None,
    smooth_warping: bool = False,
    smooth_kwargs: Optional[Mapping[str, Any]] = None,
    save_parameters: bool = False,
    save_data: bool = True,
    save_metadata: bool = True,
    seed: int = 1,
    outfile: Optional[str] = None,
    expectations: Optional[List[str]] = None,
    save_interrupted: bool = True,
    verbose: bool = False,
    quiet: bool = True,
    copy: bool = False,
    *,
    backend=None,
    comm=None,
):
    """
    Run Multi-Omics Factor Analysis (MOFA+) on the GPU.

    Same parameters as ``muon.tl.mofa`` (reference tools.py:290-416).  ``gpu_mode`` /
    ``gpu_device`` are accepted and ignored (this implementation always runs on the GPU).
    Keyword-only extras: ``backend`` (operator set) and ``comm`` (samples sharded over ranks).

    ``smooth_covariate`` (one ``.obs`` column or a list of them) gives every factor a Gaussian-process prior over the
    covariate (MEFISTO; the model: ``muon_amd/_core/mefisto.py``).  ``smooth_kwargs`` takes ``covariates_names``,
    ``scale_cov``, ``start_opt``, ``n_grid``, ``opt_freq``, ``model_groups`` and ``new_values``; ``smooth_warping=True``,
    ``sparseGP=True``, ``frac_inducing`` and ``model_groups=True`` with several groups raise NotImplementedError.  The
    learned hyperparameters land in ``.uns["mofa"]["smooth"]``.
    """
    if is_anndata(data):
        logger.info("Wrapping an AnnData object into an MuData container")
        mdata = MuData({"data": data})
        # Modality name is used as a prefix by default
        mdata.obs = data.obs
    elif is_mudata(data):
        mdata = data
    else:
        raise TypeError("Expected an MuData object")

    if outfile is None:
        outfile = os.path.join("/tmp", "mofa_{}.hdf5".format(strftime("%Y%m%d-%H%M%S")))

    if use_var and use_var not in data.var.columns:
        warn(f"There is no column {use_var} in the provided object")
        use_var = None
    common_obs = None
    if is_mudata(data):
        common_obs = reduce(np.intersect1d, [v.obs_names.values for k, v in mdata.mod.items()])
        if len(common_obs) != mdata.n_obs:
            if not use_obs:
                raise IndexError(
                    "Not all the observations are the same across modalities. Please run `mdata.intersect_obs()` to subset the data or devise a strategy with `use_obs` ('union' or 'intersection')"
                )
            elif use_obs not in ["union", "intersection"]:
                raise ValueError(
                    f"Expected `use_obs` argument to be 'union' or 'intersection', not '{use_obs}'"
                )
        else:
            use_obs = None

    if svi_mode:
        raise NotImplementedError("stochastic variational inference (svi_mode) is not implemented")
    smooth = _smooth_options(smooth_covariate, smooth_warping, smooth_kwargs)
    if convergence_mode not in ("fast", "medium", "slow"):
        raise ValueError("convergence_mode must be 'fast', 'medium' or 'slow'")

    lik = likelihoods
    if lik is not None and (isinstance(lik, str) and isinstance(lik, Iterable)):
        lik = [lik for _ in range(len(mdata.mod))]

    logger.info("Setting data from MuData object...")
    views, groups, group_names, obs_used, lik = _collect_views(
        mdata, groups_label, use_raw, use_layer, lik, use_var, use_obs
    )

    backend = backend_or_default(backend)  # raises without a GPU: no CPU fallback

    logger.info("Building the model...")
    kw = dict(dtype=torch.float32 if use_float32 else torch.float64,
              center_groups=center_groups, scale_views=scale_views, scale_groups=scale_groups,
              ard_weights=ard_weights, ard_factors=ard_factors, spikeslab_weights=spikeslab_weights,
              seed=seed, comm=comm)
    if smooth is not None:
        from .mefisto import SmoothMofaEngine

        _check_smooth_options(smooth, len(group_names), spikeslab_factors, comm)
        cov, cov_names, scaling = _smooth_covariates(mdata.obs, obs_used, smooth_covariate, smooth)
        if ard_factors:
            logger.info("ard_factors is ignored with smooth_covariate: the factors' prior is the Gaussian process")
        eng = SmoothMofaEngine(backend, views, list(lik), groups, n_factors, cov, start_opt=smooth["start_opt"],
                               n_grid=smooth["n_grid"], opt_freq=smooth["opt_freq"], **kw)
    else:
        eng = _mofa_engine(backend, views, lik, groups, n_factors, spikeslab_factors, **kw)
    logger.info("Running the model...")
    eng.run(n_iterations=n_iterations, convergence_mode=convergence_mode)
    res = eng.results(sort_factors=True)
    if smooth is not None:
        res["smooth"]["covariates_names"] = cov_names
        res["smooth"]["covariates"] = cov
        nv = _smooth_new_values(smooth)
        if nv is not None:
            logger.info("Interpolating factors...")
            at = nv if scaling is None else (nv - scaling[0]) / scaling[1]
            res["smooth"]["new_values"] = nv
            res["smooth"]["Z_predicted"] = eng.predict(at)[:, res["order"]]

    logger.info("Saving the model...")
    try:
        written = _save_model(outfile, res, list(mdata.mod.keys()), group_names, obs_used, groups, expectations)
    except Exception as e:  # noqa: BLE001  (a failing save must not lose the fit: the slots below are still written)
        warn(f"Cannot save the model to {outfile}: {e!r}")
        written = None

    if copy:
        data = data.copy()

    # Factors: rows follow the order of the samples in data.obs (tools.py:604-627)
    z = res["Z"]
    if use_obs == "intersection":
        # the model's samples are the common cells in SORTED name order (np.intersect1d, like the reference :99-101);
        # every cell gets its own row back, by name.  (The reference assigns the sorted-order rows through a boolean
        # mask in data.obs order, :617-621 - the same thing only when the names happen to be sorted; otherwise each
        # common cell receives another cell's factors: not reproduced.)
        xm = np.full((data.n_obs, z.shape[1]), np.nan)
        if os.environ.get("MUON_AMD_MOFA_INTERSECTION_MASK", "0") == "1":
            # the reference's statement, bit for bit (:615-621): the model's rows - in sorted-name order - land in the
            # True positions of the mask in data.obs order.  Identical to the default when the names are sorted.
            xm[data.obs.index.isin(pd.Index(obs_used))] = z
        else:
            xm[data.obs.index.get_indexer(pd.Index(obs_used))] = z
        data.obsm["X_mofa"] = xm
    else:
        data.obsm["X_mofa"] = z

    # Weights (tools.py:629-641)
    w = np.concatenate(res["W"], axis=0)
    if use_var:
        lfs = np.zeros(shape=(data.n_vars, w.shape[1]))
        lfs[np.asarray(data.var[use_var]).astype(bool)] = w
        data.varm["LFs"] = lfs
    else:
        data.varm["LFs"] = w

    # Parameters (tools.py:653-678)
    data.uns["mofa"] = {
        "params": {
            "data": {
                "groups_label": groups_label,
                "use_raw": use_raw,
                "use_layer": use_layer,
                "likelihoods": np.asarray(lik).astype(str),
                "features_subset": use_var,
                "use_obs": use_obs,
                "scale_views": scale_views,
                "scale_groups": scale_groups,
                "center_groups": center_groups,
                "use_float32": use_float32,
            },
            "model": {
                "ard_factors": ard_factors,
                "ard_weights": ard_weights,
                "spikeslab_weights": spikeslab_weights,
                "spikeslab_factors": spikeslab_factors,
                "n_factors": n_factors,
            },
            "training": {
                "n_iterations": n_iterations,
                "convergence_mode": convergence_mode,
                "gpu_mode": gpu_mode,
                "seed": seed,
            },
        },
        "elbo": np.asarray(res["elbo"]),
        # (not in the reference) the file actually written: without h5py the archive is `outfile`.npz
        "model_file": str(written),
    }
    if smooth is not None:
        # (not in the reference, which leaves them in the model file) the learned GP hyperparameters per factor, in the
        # factor order of X_mofa, the lengthscale grid and - with ``new_values`` - the interpolated factors
        data.uns["mofa"]["smooth"] = {k: v for k, v in res["smooth"].items() if k != "covariates"}
    # Variance explained, R2 in % per factor (tools.py:681-697)
    variance = {m: {} for m in mdata.mod}
    for i, m in enumerate(mdata.mod):
        if len(group_names) > 1:
            for gi, g in enumerate(group_names):
                variance[m][g] = res["r2"][i, gi, :]
        else:
            variance[m] = res["r2"][i, 0, :]
    data.uns["mofa"]["variance"] = variance

    if copy:
        return data
    else:
        if not quiet:
            print("Saved MOFA embeddings in .obsm['X_mofa'] slot and their loadings in .varm['LFs'].")

    return None


def _model_datasets(res, view_names, group_names, obs_names, groups):
    """The model as {dataset path: array} in mofapy2's HDF5 layout - the paths and shapes the reference reads back
    (/root/reference/muon/_core/tools.py:604-641: expectations/Z/<group> [factors, samples], expectations/W/<view>
    [factors, features], samples/<group>) plus views/views, groups/groups, variance_explained/r2_per_factor/<group>
    [views, factors] and training_stats/elbo.  Both writers below store exactly this mapping."""
    def _bytes(names):  # UTF-8 byte strings (h5py / mofapy2's convention; `.astype("S")` raises on non-ASCII names)
        return np.char.encode(np.asarray(names).astype(str), "utf-8") if len(names) else np.asarray([], dtype="S1")

    d = {}
    for gi, g in enumerate(group_names):
        d[f"expectations/Z/{g}"] = np.ascontiguousarray(res["Z"][groups == gi].T)
        d[f"samples/{g}"] = _bytes(np.asarray(obs_names)[groups == gi])
        d[f"variance_explained/r2_per_factor/{g}"] = np.ascontiguousarray(res["r2"][:, gi, :])
    for m, w in zip(view_names, res["W"]):
        d[f"expectations/W/{m}"] = np.ascontiguousarray(np.asarray(w).T)
    d["views/views"] = _bytes(view_names)
    d["groups/groups"] = _bytes(group_names)
    d["training_stats/elbo"] = np.asarray(res["elbo"])
    if res.get("smooth") is not None:  # a fit with smooth_covariate: the hyperparameters per factor, the covariates per group
        d["training_stats/length_scales"] = np.asarray(res["smooth"]["lengthscale"], dtype=np.float64)
        d["training_stats/scales"] = np.asarray(res["smooth"]["scale"], dtype=np.float64)
        for gi, g in enumerate(group_names):
            d[f"covariates/{g}"] = np.ascontiguousarray(np.asarray(res["smooth"]["covariates"])[groups == gi])
    return d


def _save_model(outfile, res, view_names, group_names, obs_names, groups, expectations):
    """Model file (tools.py:600-602 ent.save): HDF5 with mofapy2's group layout when h5py is
    importable.  Without h5py (this image) the SAME datasets are written as a NumPy .npz whose keys are the HDF5
    paths - under a name that says so (``outfile`` + ".npz" unless it already ends in .npz): a file called *.hdf5
    that no MOFA tool can open helps nobody, and a converter is one loop
    (``for k in z.files: h5.create_dataset(k, data=z[k])``).  Returns the path written."""
    data = _model_datasets(res, view_names, group_names, obs_names, groups)
    try:
        import h5py  # noqa: F401
    except Exception:  # noqa: BLE001
        if not str(outfile).endswith(".npz"):
            warn(f"h5py is not importable: the model is saved as NumPy archive {outfile}.npz, not as HDF5")
            outfile = str(outfile) + ".npz"
        try:
            with open(outfile, "wb") as f:
                np.savez(f, **data)
        except OSError as e:  # pragma: no cover
            warn(f"Cannot save the model to {outfile}: {e}")
        return outfile
    import h5py

    with h5py.File(outfile, "w") as f:  # pragma: no cover - h5py absent in the build image
        for k, v in data.items():
            f.create_dataset(k, data=v)
    return outfile
