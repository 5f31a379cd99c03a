"""``muon_amd.rna`` mirrors ``muon.rna`` (/root/reference/muon/rna.py:1) for the steps with which every RNA modality
of a multiome or CITE-seq workflow starts: ``rna.pp.normalize_total``, ``rna.pp.log1p``,
``rna.pp.highly_variable_genes``, ``rna.pp.scale`` (``_rna/preproc.py``; scanpy's signatures, on the device CSR).  The
PCA that follows them is ``muon_amd.tl.pca``."""
from ._rna import pp  # noqa: F401
