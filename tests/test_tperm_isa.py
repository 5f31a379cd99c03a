"""ISA audit of the table-driven fill (csrc/tperm.hip), modelled on the audit of csrc/tpack4.hip in tests/test_layout.py:
`k_tperm_move` keeps a tile header in v[72..75], 17 window slots of (column, value) in v[76..109] and their staging slots in
v[110..126], all written by loads issued from inline asm a tile ahead.  hipcc must stay below v72 (a copy or a spill of a
register whose load is in flight reads stale data), must not spill (scratch traffic shares vmcnt with the hand-placed
waits), must not issue a vector load of its own inside the kernel's loop (its wait would drain the windows just requested)
and the 16 waves of the 1024-thread workgroup must fit one CU: 128 VGPRs, at most 160 KiB of LDS."""
import os
import re
import shutil

import pytest

from muon_amd.csrc import build as csrc_build


def test_tperm_isa_keeps_out_of_the_asm_owned_registers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "tperm.s"
    csrc_build.device_asm("tperm.hip", out)
    text = out.read_text()
    assert "k_t4_fill" not in text
    kernels = re.findall(r"^(_ZN[^\n:]*k_tperm_move[^\n:]*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S | re.M)
    assert len(kernels) == 1
    name, body = kernels[0]
    m = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body)
    assert m and int(m.group(1)) == 128, m and m.group(1)
    m = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body)
    assert m and int(m.group(1)) <= 160 * 1024, m and m.group(1)
    assert "scratch_" not in body and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body)
    reg = re.compile(r"\bv(\d+)\b|v\[(\d+):(\d+)\]")
    inasm, own_loads, asm_loads = False, [], 0
    for line in body.splitlines():
        if "#ASMSTART" in line:
            inasm = True
        elif "#ASMEND" in line:
            inasm = False
        elif inasm:
            asm_loads += len(re.findall(r"^\s*global_load_", line))
        elif not line.lstrip().startswith((".", ";")):
            for a, b, c in reg.findall(line.split(";")[0]):
                assert (int(a) if a else int(c)) < 72, line
            if re.match(r"\s*(global|flat|buffer|scratch)_load", line):
                own_loads.append(line.strip())
    # hipcc's own vector loads: the two of the prologue (row pointers, the rows' places in the stream), none in the loop
    assert len(own_loads) == 2, own_loads
    assert asm_loads >= 2 * (16 * 4 + 4 + 3)  # prologue + loop: 16 circular slots x 4 loads, the continuation's 4, a header's 3
    # every plan kernel is plain C++: no asm-owned registers, no scratch
    plans = re.findall(r"^(_ZN[^\n:]*k_tperm_plan[^\n:]*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S | re.M)
    assert len(plans) == 2
    for _name, pbody in plans:
        assert "scratch_" not in pbody and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", pbody)
