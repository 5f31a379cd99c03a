"""``muon_amd.prot`` mirrors ``muon.prot`` (/root/reference/muon/prot.py:1) for the normalisation step of the CITE-seq
workflow: ``prot.pp.dsb``, ``prot.pp.clr``."""
from ._prot import pp  # noqa: F401
