"""``muon_amd.atac`` mirrors ``muon.atac`` (/root/reference/muon/atac.py:1) for the hot path:
``atac.pp.tfidf``, ``atac.pp.binarize``, ``atac.tl.lsi`` and the fragment tools ``atac.tl.locate_fragments``,
``count_fragments_features``, ``tss_enrichment``, ``nucleosome_signal`` (``_atac/fragments.py``)."""
from ._atac import pp, tl  # noqa: F401
