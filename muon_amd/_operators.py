"""The operator set host code is written against: which operators there are, which of them an implementation may
leave out, and the capability flags.  ``HipBackend`` (the product) and the CPU stand-in of the tests both inherit from
``OperatorSet``; host code asks ``has(be, "name", ...)`` or reads a flag, never ``hasattr``.

An optional operator is declared here as ``None`` and overridden by a method where it is implemented.  A name that is
not declared is an ``AttributeError`` wherever it is asked for: a misspelt probe fails instead of quietly taking the
tensor formulation.  Nothing here computes anything.

``has`` is a function, not a method, so that it answers for every object host code is handed as an operator set: a
wrapper that forwards through ``__getattr__`` (bench.py's timer, the tests' call counters), one that hides an operator
by raising ``AttributeError`` for it, and a plain class that only defines what it implements.
"""
import torch


class OperatorSet:
    # -- flags --------------------------------------------------------------------------------------------------------
    name = ""                        # "hip": the product backend (device streams, graphs, the C-ABI library)
    skinny_mixed = False             # skinny_nn / skinny_tn take an f32-stored view under an f64 block
    mofa_poisson_lik_with_b = False  # mofa_poisson_pass has mode 3 (likelihood and B in one pass)

    # -- operators every set implements: host code calls them without asking -------------------------------------------
    REQUIRED = ("empty", "zeros", "to_device", "to_host", "fetch_async", "upload_csr", "row_col_sums", "idf",
                "tfidf_scale", "compact_nonzero", "binarize_values", "transpose", "spmm", "gram", "gram_cross", "apply",
                "project_out_block", "randn")

    # -- optional operators, by domain (the kernels' files under csrc/) -------------------------------------------------
    # derived tables of a device CSR and the hand-offs of the TF-IDF sweeps (tfidf.hip, spmm_win.hip)
    with_slab_ptr = with_plans = slab_ptr_from_work = slab_ptr_width = None
    can_emit_stream = stream_layout = None
    # QC metrics and filtering (filter.hip)
    csr_qc = csr_submatrix = None
    # per-row sums of qc_metrics' qc_vars / percent_top (qc.hip)
    row_masked_sums = row_top_sums = None
    # fragment tools (fragments.hip)
    frag_ranges = frag_overlap = frag_pileup = frag_pileup_scan = frag_length_classes = None
    # transposition and row streams (transpose.hip, tpack4.hip, tperm.hip, tflat.hip, spmm_win.hip); behind can_stream: stream,
    # transpose_stream, stream_both and the status of the tile-staged fill
    transpose_csr = can_stream = stream = transpose_stream = stream_both = split_streams = None
    raise_tpack4 = tpack4_status = launch_layout = spmm_slab = None
    # the cell slice of lsi's warm start (spmm_win.hip); behind slice_plan: the rest
    slice_plan = slice_stream = spmm_slice = spmm_slice_t = spmm_slab_ranged = None
    # sliced-ELL operands of the narrow-block SpMM (spmm_ell.hip); ell16_fits(X, wide): whether its 32-bit offsets reach
    ell16_fits = ell16 = ell16_pair = spmm_ell = None
    # block orthogonalisation on the device (dense.hip); kernel switches (runtime.hip)
    chol_rinv = tune = tune_keys = None
    # neighbour search and WNN (knn.hip, wnn.hip)
    umap_strengths = wnn_bandwidth = knn_filter = knn_merge = None
    # MOFA+ (mofa.hip, mofa_stats.hip, mofa_elbo.hip, skinny.hip): what MofaEngine needs (mofa_engine.REQUIRED_OPS) ...
    mofa_update_w = mofa_update_z = mofa_rowstats_work = mofa_rowstats = None
    mofa_elbo_work = mofa_tau_elbo = mofa_w_elbo = mofa_z_sums = mofa_z_elbo = None
    # ... its faster operands, and the sweeps of GeneralMofaEngine (mofa_poisson.hip, mofa_bernoulli.hip); behind
    # mofa_stats_resid: mofa_tau_finish
    skinny_nn = skinny_tn = col_moments = densify_rows = None
    mofa_jaakkola = mofa_poisson_pseudo = mofa_poisson_pass = mofa_softplus_sweep = mofa_jaakkola_sweep = None
    mofa_gs_update = mofa_stats_resid = mofa_tau_finish = None
    # ... and the two passes of the eigen route of a fit with smooth_covariate (gp.hip; _core/mefisto.py)
    gp_project = gp_posterior = None
    # muon.prot.pp.dsb (prot.hip)
    prot_max_proteins = prot_log_moments = prot_dsb_fit = None
    # muon.tl.ica (ica.hip)
    ica_max_components = ica_sweep = None
    # muon.tl.snf (snf.hip): the five kernels are asked for together, their limits go with them
    free_memory = snf_max_k = snf_affinity_max_k = snf_max_terms = None
    snf_affinity = snf_normalize = snf_topk = snf_p_scale = snf_diffuse = None
    # muon.atac.tl.rank_peaks_groups (rank.hip)
    group_moments_max_groups = rank_row_cap = group_moments = rank_sums = None
    # muon.tl.leiden / muon.tl.louvain (cluster.hip): asked for together
    cluster_max_table = cluster_max_layers = cluster_move = cluster_segsum = None
    # muon.tl.umap (umap.hip)
    umap_max_components = umap_epoch = None
    # muon.atac.pp.scopen (nmf.hip)
    nmf_max_components = nmf_cd_sweep = None
    # muon_amd.rna.pp and muon_amd.tl.pca (rna.hip)
    gene_moments_max_blocks = gene_moments = value_sweep = shift_cols = scale_rows = None
    # muon_amd.rna.pp.scale (scale.hip)
    scale_values = scale_dense_rows = None
    # muon.atac.tl.scan_sequences (motif.hip): behind motif_scan
    motif_max_len = motif_tile = motif_group = motif_room = motif_scan = None
    # muon_amd.pp.harmony_integrate (harmony.hip): asked for together
    harmony_limits = harmony_gram = harmony_assign = harmony_objective = harmony_correct = None
    # muon_amd.pp.scrublet (scrublet.hip): the sum of two canonical CSR rows per simulated doublet (f32 values, int32 or
    # int64 indices, rows of any length), and knn_merge past its 1024 pairs: kc + cap <= knn_merge_wide_max()
    csr_pair_rows = knn_merge_wide_max = knn_merge_wide = None
    # synthetic counts of the benchmark and the tests (synth.hip)
    synth_counts = None


DECLARED = frozenset(OperatorSet.REQUIRED) | {n for n, v in vars(OperatorSet).items() if v is None and n[0] != "_"}


def has(ops, *names) -> bool:
    """True when the operator set ``ops`` implements every named operator: the attribute is there and is not None.
    A name that ``OperatorSet`` does not declare raises AttributeError, whatever ``ops`` is."""
    if not DECLARED.issuperset(names):
        raise AttributeError(f"{sorted(set(names) - DECLARED)}: no operator that OperatorSet declares")
    for n in names:  # (asked inside iteration loops: a plain loop, no generator)
        if getattr(ops, n, None) is None:
            return False
    return True


def transposed_csr(be, X):
    """X^T as a device CSR: the tile-staged transposition (``transpose_csr``: f32 values) where ``be`` has it and X
    has stored entries, else the general ``transpose``.  A dispatch, like ``has``: the operators compute."""
    if X.values.dtype == torch.float32 and X.nnz > 0 and has(be, "transpose_csr"):
        return be.transpose_csr(X)
    return be.transpose(X)
