"""Which backend operators a public call reaches, for the domains whose GPU tests compare results only: fragments, rank,
cluster, snf, motif and filter / qc.  Their kernels and their tensor formulations are built to agree, so a parity test
stays green when a call is quietly rerouted to the tensor formulation; the exact set of operators called does not.

Each case is the smallest public call of that domain's own GPU test.  The expected sets were recorded by running this
spy on the commit before the operator set was declared (`OperatorSet`, muon_amd/_operators.py), not read off the code."""
import warnings

import numpy as np
import pytest

import muon_amd as mu
from muon_amd import atac as ac
from muon_amd import tl
from tests import cluster_fixture, frag_fixture, motif_fixture, rank_fixture, snf_fixture
from tests.synth import planted_topics_csr

pytestmark = pytest.mark.gpu


class _Spy:
    """Forwards to a backend and records which of its operators were called."""

    def __init__(self, be):
        self._be, self.called = be, set()

    def __getattr__(self, name):
        got = getattr(self._be, name)
        if name.startswith("_") or not callable(got):
            return got

        def counted(*a, **k):
            self.called.add(name)
            return got(*a, **k)

        return counted


def _fragments(be):
    g = frag_fixture.load()
    a = frag_fixture.adata(g, be)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)
        ac.tl.count_fragments_features(a, frag_fixture.features(g, False), backend=be)
    ac.tl.tss_enrichment(a, frag_fixture.features(g, True), backend=be)
    ac.tl.nucleosome_signal(a, backend=be)


def _rank(be):
    ad = rank_fixture.anndata("float32")
    ac.tl.rank_genes_groups(ad, "leiden", backend=be, **rank_fixture.CASES["wilcoxon-tie"])


def _cluster(be):
    tl.leiden(cluster_fixture.mudata("n65"), backend=be, **cluster_fixture.call_kwargs("n65"))


def _snf(be):
    tl.snf(snf_fixture.mudata("n21_k20"), backend=be, **snf_fixture.call_kwargs("n21_k20"))


def _motif(be):
    ids, mats = motif_fixture.bank()
    ac.tl.scan_sequences(list(motif_fixture.sequences(be.motif_tile())), matrices=mats, motifs=ids, backend=be)
    be.called.discard("motif_tile")  # (this function's own question)


def _filter(be):
    ad = mu.AnnData(planted_topics_csr(2000, 3000, n_topics=10, density=0.01, seed=3, dtype=np.float32))
    mu.pp.qc_metrics(ad, backend=be)
    mu.pp.filter_var(ad, "n_cells_by_counts", lambda x: x >= 3, backend=be)
    mu.pp.filter_obs(ad, "n_genes_by_counts", lambda x: x >= 45, backend=be)


ROUTES = {
    "fragments": (_fragments, {"frag_ranges", "frag_overlap", "frag_pileup", "frag_pileup_scan", "frag_length_classes",
                               "with_slab_ptr", "to_device", "to_host"}),
    "rank": (_rank, {"group_moments", "group_moments_max_groups", "rank_sums", "transpose_csr", "with_slab_ptr",
                     "upload_csr", "to_device", "to_host"}),
    "cluster": (_cluster, {"cluster_move", "cluster_segsum", "cluster_max_layers", "zeros", "to_device", "to_host"}),
    "snf": (_snf, {"snf_affinity", "snf_normalize", "snf_topk", "snf_p_scale", "snf_diffuse", "snf_max_k",
                   "snf_affinity_max_k", "snf_max_terms", "free_memory", "empty", "to_device", "to_host"}),
    "motif": (_motif, {"motif_scan", "motif_max_len", "motif_group", "to_device", "to_host"}),
    "filter": (_filter, {"csr_qc", "csr_submatrix", "with_slab_ptr", "upload_csr", "to_device", "to_host"}),
}


@pytest.mark.parametrize("domain", list(ROUTES))
def test_public_call_reaches_exactly_these_operators(hip, domain):
    run, want = ROUTES[domain]
    spy = _Spy(hip)
    run(spy)
    print(f"ROUTES {domain}: {sorted(spy.called)}")
    assert spy.called == want
