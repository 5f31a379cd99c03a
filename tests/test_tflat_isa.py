"""ISA audit of the flat read-in fill (csrc/tflat.hip), with `build.device_asm` as tests/test_tperm_isa.py uses it: the 16
waves of `k_tflat_move`'s 1024-thread workgroup must fit one CU - at most 128 VGPRs, no scratch (its rounds of pairs in
flight are a statically indexed register array: a spill would put them in memory), at most 160 KiB of LDS - and the
production instance carries none of the phase-accounting instance's time stamps."""
import os
import re
import shutil

import pytest

from muon_amd.csrc import build as csrc_build


def test_tflat_isa_fits_one_cu_and_carries_no_stamps(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "tflat.s"
    csrc_build.device_asm("tflat.hip", out)
    text = out.read_text()
    bodies = {}
    for kernel in ("k_tflat_move", "k_tflat_phases"):
        # (the function's code, then its .amdhsa_kernel descriptor)
        found = re.findall(r"^(_ZN[^\n:]*" + kernel + r"[^\n:]*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S | re.M)
        assert len(found) == 1, kernel
        bodies[kernel] = found[0][1]
    for kernel, body in bodies.items():
        m = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body)
        assert m and int(m.group(1)) <= 128, (kernel, m and m.group(1))
        m = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body)
        assert m and int(m.group(1)) <= 160 * 1024, (kernel, m and m.group(1))
        assert "scratch_" not in body and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), kernel
    assert "s_memtime" not in bodies["k_tflat_move"]
    assert "s_memtime" in bodies["k_tflat_phases"]  # (the search does find a stamp where there is one)
