"""muon_amd - MI355X-native TF-IDF / LSI / MOFA hot path of scverse/muon.

Drop-in namespaces for the three hot-path entry points of the reference
(/root/reference/muon/__init__.py:6-14, muon/atac.py:1):

    muon_amd.atac.pp.tfidf   <->  muon.atac.pp.tfidf
    muon_amd.atac.tl.lsi     <->  muon.atac.tl.lsi
    muon_amd.tl.mofa         <->  muon.tl.mofa
    muon_amd.pp.neighbors    <->  muon.pp.neighbors   (the consumer of X_lsi / X_mofa)
    muon_amd.prot.pp.dsb     <->  muon.prot.pp.dsb    (protein normalisation ahead of neighbors on CITE-seq data)
    muon_amd.prot.pp.clr     <->  muon.prot.pp.clr
    muon_amd.pp.filter_obs   <->  muon.pp.filter_obs  (filter_var alike; pp.qc_metrics: scanpy's QC columns they key on)
    muon_amd.pp.qc_metrics(qc_vars=, percent_top=)  <->  scanpy's calculate_qc_metrics: pct_counts_mt and
                             pct_counts_in_top_{n}_genes from the resident CSR (a masked sum and a radix select per row)
    muon_amd.pp.intersect_obs  <->  muon.pp.intersect_obs  (the cells all modalities share; device copies go along)
    muon_amd.pp.sample_obs   <->  muon.pp.sample_obs  (the reference's draws under one np.random.seed; host only)
    muon_amd.atac.tl.count_fragments_features / tss_enrichment / nucleosome_signal  <->  muon.atac.tl.* (the fragment
                             tools: gene-activity counts and the two QC columns, over a fragment table on the device;
                             atac.tl.locate_fragments reads the TSV, atac.tl.fragments_from_arrays takes its columns)
    muon_amd.tl.ica          <->  muon.tl.ica         (FastICA of X_pca / X_lsi / X_mofa: one fused sweep per iteration)
    muon_amd.pp.harmony_integrate  <->  scanpy.external.pp.harmony_integrate  (Harmony batch correction of X_pca / X_lsi:
                             the k-means rounds and the correction on f64 matrix-core kernels; the package's own statement)
    muon_amd.pp.scrublet / scrublet_simulate_doublets  <->  scanpy.pp.scrublet / scrublet_simulate_doublets  (doublet
                             detection on the resident raw counts, before normalize_total: a sparse row-pair merge, the
                             projection of the simulated rows as one SpMM, a search with k in the hundreds whose per-panel
                             merge is a workgroup-wide sort; the package's own statement, parity with scanpy not pinned)
    muon_amd.tl.snf          <->  muon.tl.snf        (similarity network fusion: P S P^T as two sparse-dense passes)
    muon_amd.atac.tl.rank_peaks_groups  <->  muon.atac.tl.rank_peaks_groups  (scanpy's rank_genes_groups on the device
                             copy of the peak matrix, then add_genes_peaks_groups; atac.tl.add_peak_annotation alike)
    muon_amd.atac.tl.scan_sequences  <->  muon.atac.tl.scan_sequences  (every window of every peak sequence against a
                             bank of position weight matrices on the f64 matrix cores; atac.tl.get_sequences reads the FASTA)

    muon_amd.atac.pp.scopen  <->  muon.atac.pp.scopen  (bounded NMF imputation of the peak matrix: it stays CSR, one fused
                             coordinate-descent sweep per half-iteration; atac.pp.binarize alike)

    muon_amd.rna.pp.normalize_total / log1p / highly_variable_genes, muon_amd.tl.pca  <->  scanpy's, the steps with which
                             the reference's tutorials open every RNA modality: the matrix stays the device CSR, PCA is
                             lsi's block Lanczos process on the implicitly centred (and scaled) operator
    muon_amd.rna.pp.scale    <->  scanpy's scale: the clipped z-scores are a sparse matrix plus one row; the dense X is
                             written once by a fused pass, and tl.pca decomposes it through the sparse form, no upload

    muon_amd.tl.leiden / muon_amd.tl.louvain  <->  muon.tl.leiden / muon.tl.louvain  (multiplex clustering over the
                             modalities' graphs: a wave per vertex groups its neighbours' communities in an LDS table)
    muon_amd.tl.umap         <->  muon.tl.umap        (the layout of the multimodal neighbourhood graph: a Jacobi epoch
                             per launch, sixteen lanes per vertex, an integer schedule and counter-based negatives)

Everything else of muon (I/O, plotting, ...) is out of scope; see DESIGN.md.
"""
from ._containers import AnnData, MuData  # duck-typed stand-ins when anndata/mudata are absent
from . import atac  # noqa: F401
from . import prot  # noqa: F401
from . import rna  # noqa: F401
from ._core import tools as tl  # noqa: F401
from ._core import preproc as pp  # noqa: F401  (mu.pp.neighbors - weighted nearest neighbours -, mu.pp.l2norm,
#   mu.pp.filter_obs / filter_var / intersect_obs on the resident device copy, qc_metrics: the columns they key on,
#   mu.pp.sample_obs)
from ._core import io  # noqa: F401  (arrays of 10x / mtx / snap files -> row-sharded device CSR)

__version__ = "0.1.0"
