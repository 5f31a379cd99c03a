"""The 320-column instances of the row-stream SpMM (k_spmm_wide / k_spmm_wide_rng, csrc/spmm_win.hip) in the generated
gfx950 ISA: they exist, take all 160 KiB of LDS, do not spill, and the compiler stays out of the registers the inline
asm owns - the rule tests/test_layout.py applies to the 256-column instances.  Reads register numbers and resource
fields, nothing else."""
import os
import re
import shutil

import pytest

from muon_amd.csrc import build as csrc_build


def test_wide_slab_instances_in_the_isa(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "spmm_win.s"
    csrc_build.device_asm("spmm_win.hip", out)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN[^\n:]*k_spmm_wide[^\n:]*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S | re.M)
    # production instances: MODE = 0 (the second template argument of k_spmm_wide); the accounting instance feeds nobody
    prod = re.compile(r"(k_spmm_wide)ILi(\d)ELi0EE|(k_spmm_wide_rng)ILi(\d)EE")
    got = sorted(tuple(x for x in m.groups() if x) for m in (prod.search(n) for n, _ in kernels) if m)
    assert got == [("k_spmm_wide", "6"), ("k_spmm_wide", "7"), ("k_spmm_wide", "8"),
                   ("k_spmm_wide_rng", "6"), ("k_spmm_wide_rng", "7"), ("k_spmm_wide_rng", "8")]
    kernels = [(n, b) for n, b in kernels if prod.search(n)]
    assert len(kernels) == 6
    reg = re.compile(r"\bv(\d+)\b|v\[(\d+):(\d+)\]")
    for name, body in kernels:
        assert re.search(r"\.amdhsa_group_segment_fixed_size 163840\b", body), name  # 2 x 320 rows x 256 B
        assert "scratch_" not in body, name
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        m = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body)
        assert m and int(m.group(1)) == 126, (name, m and m.group(1))
        inasm = False
        for line in body.splitlines():
            if "#ASMSTART" in line:
                inasm = True
            elif "#ASMEND" in line:
                inasm = False
            elif not inasm and not line.lstrip().startswith((".", ";")):
                for a, b, c in reg.findall(line.split(";")[0]):
                    hi = int(a) if a else int(c)
                    assert hi < 110, (name, line)
