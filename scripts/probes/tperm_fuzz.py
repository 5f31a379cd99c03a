#!/usr/bin/env python
"""Randomised comparison of the table-driven fill (csrc/tperm.hip) with the fill of csrc/tpack4.hip (tune tperm_off = 1)
and, for small shapes, scipy: the generator of tpack4_fuzz.py (random shapes, densities, bursts of consecutive columns,
runs of neighbouring rows with the same burst, empty rows / column ranges, forced tile widths) with row counts that give
a wave 1 .. 32 rows, the source laid out by stream_layout() - the plan's layout, which is what selects the table path.
Same ent / sptr / perm or it stops.  Usage: tperm_fuzz.py [cases] [seed]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import scipy.sparse as sp
import torch

from muon_amd._backend import _p, check, get_backend

be = get_backend()
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 120
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.default_rng(seed)


def make(n, d, dens):
    m = sp.random(n, d, density=dens, format="lil", random_state=rng, dtype=np.float32)
    for _ in range(int(rng.integers(0, 12))):
        r = int(rng.integers(0, n))
        L = int(rng.integers(20, min(d, 700) + 1)) if d > 20 else d
        c0 = int(rng.integers(0, d - L + 1))
        m[r, c0:c0 + L] = rng.random(L).astype(np.float32) + 0.25
    if n > 40 and rng.random() < 0.7:  # runs of neighbouring rows with the same burst (the rows of one or two waves)
        for _ in range(int(rng.integers(1, 4))):
            r0 = int(rng.integers(0, n - 34))
            L = int(rng.integers(33, min(d, 200) + 1)) if d > 33 else d
            c0 = int(rng.integers(0, d - L + 1))
            for r in range(r0, r0 + int(rng.integers(2, 34))):
                m[r, c0:c0 + L] = 1.5
    m = m.tocsr()
    if d > 50 and rng.random() < 0.5:  # an empty column range
        a = int(rng.integers(0, d - 10))
        keep = np.ones(d, dtype=np.float32)
        keep[a:a + int(rng.integers(1, d - a))] = 0
        m = sp.csr_matrix(m @ sp.diags(keep))
    if n > 10 and rng.random() < 0.5:  # empty rows
        keep = np.ones(n, dtype=np.float32)
        keep[::int(rng.integers(2, 9))] = 0
        m = sp.csr_matrix(sp.diags(keep) @ m)
    m.eliminate_zeros()
    m.sort_indices()
    return m.astype(np.float32)


done = with_table = multi_row = with_cont = 0
for it in range(cases):
    n = int(rng.choice([1, 17, 513, 2000, 9000, 20000, 40000, 70000, 120000, 200000]))
    d = int(rng.choice([1, 5, 33, 200, 1025, 5000, 30000, 200000]))
    dens = float(rng.choice([0.3, 0.05, 0.01, 0.002]))
    if n * d * dens > 3e7:
        dens = 3e7 / (n * d)
    m = make(n, d, dens)
    if m.nnz == 0:
        continue
    C = int(rng.choice([0, 0, 16, 48, 160, 512]))
    try:
        be.tune("tpack4_c", C)
        X = be.upload_csr(m.indptr, m.indices, m.data, m.shape, values_dtype=np.float32)
        if not be._use_tpack4(X) or be._plan_of(X, "tplan") is None:
            continue
        xs, row_dst = be.stream_layout(X)
        with be._dev_ctx():
            check(be.lib.mu_csr_stream_fill(int(xs.perm.numel()), _p(xs.perm), _p(X.indptr), _p(X.indices), _p(X.values),
                                            _p(xs.sptr), _p(xs.ent), be._stream()))
        be.tune("tperm_off", 0)
        new = be.transpose_stream(X, src=(xs, row_dst))
        table = be._plan_of(X, "tplan").get("tperm")
        assert isinstance(table, dict), (it, n, d, dens, C)
        be.tune("tperm_off", 1)
        old = be.transpose_stream(X, src=(xs, row_dst))
    finally:
        be.tune("tpack4_c", 0)
        be.tune("tperm_off", 0)
    assert torch.equal(old.sptr, new.sptr) and torch.equal(old.perm, new.perm), (it, n, d, dens, C)
    assert torch.equal(old.ent[: m.nnz], new.ent[: m.nnz]), (it, n, d, dens, C)
    assert int(table["slots"].max()) < be.lib.mu_tperm_stage_pairs()
    if m.nnz < 3e6:  # ... and the transpose itself
        mt = m.T.tocsr()
        mt.sort_indices()
        sptr, perm = be.to_host(new.sptr), be.to_host(new.perm).astype(np.int64)
        ent = be.to_host(new.ent).view(np.uint64)
        for p in np.nonzero(perm >= 0)[0][:: max(1, perm.size // 4000)]:
            r = perm[p]
            e = ent[sptr[p]:sptr[p + 1]]
            assert np.array_equal((e & np.uint64(0xffffffff)).astype(np.int64), mt.indices[mt.indptr[r]:mt.indptr[r + 1]]), (it, r)
            assert np.array_equal((e >> np.uint64(32)).astype(np.uint32),
                                  mt.data[mt.indptr[r]:mt.indptr[r + 1]].view(np.uint32)), (it, r)
    rpb, _G = be._t4_geometry(n, d, m.nnz)
    done += 1
    with_table += 1
    multi_row += rpb > 16
    with_cont += "cont" in table and bool((table["cont"] != 0xffff).any())  # (the flat read-in has no such words)
print(f"seed {seed}: {done} random cases, all through the table path ({with_table}), {multi_row} with more than one row per "
      f"wave, {with_cont} with continuation windows: the table-driven fill writes the old fill's ent / sptr / perm "
      f"(and scipy's transpose on the rows compared)")
