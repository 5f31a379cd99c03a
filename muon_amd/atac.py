"""``muon_amd.atac`` mirrors ``muon.atac`` (/root/reference/muon/atac.py:1) for the hot path:
``atac.pp.tfidf``, ``atac.pp.binarize``, ``atac.pp.scopen`` (``_atac/scopen.py``), ``atac.tl.lsi`` and the fragment tools ``atac.tl.locate_fragments``,
``count_fragments_features``, ``tss_enrichment``, ``nucleosome_signal`` (``_atac/fragments.py``) and the ranking
``atac.tl.rank_peaks_groups``, ``rank_genes_groups``, ``add_peak_annotation``, ``add_genes_peaks_groups``
(``_atac/rank.py``) and the motif tools ``atac.tl.scan_sequences``, ``prepare_motif_scanner``, ``parse_motif_matrices``,
``get_sequences`` (``_atac/motifs.py``)."""
from ._atac import pp, tl  # noqa: F401
