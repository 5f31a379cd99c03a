"""Repository contracts that need no GPU: the C-ABI library loads and exports every symbol
include/muon_amd.h declares, the ctypes table derived from it covers them, the operator set is
declared once (muon_amd/_operators.py) and both backends keep to it, and the product package
never touches the oracle (which is test infrastructure)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "muon_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mu_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from muon_amd import _ffi

    names = _declared()
    assert len(names) >= 30
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in muon_amd.h but not exported: {missing}"
    assert lib.mu_version() >= 100


def test_ffi_table_matches_header():
    from muon_amd import _ffi

    assert sorted(_ffi.SIGNATURES) == _declared()
    _ffi.lib()  # loads and binds every entry


def test_ffi_table_entries_written_out_by_hand():
    """the parser of muon_amd/_ffi.py pinned by something that is not itself: whole entries, typed in from the header"""
    from ctypes import c_char_p, c_double, c_int, c_int64, c_size_t, c_uint64, c_void_p

    from muon_amd import _ffi

    i32, i64, dbl, vp, sz, u64 = c_int, c_int64, c_double, c_void_p, c_size_t, c_uint64
    want = {
        "mu_version": (i32, []),
        "mu_last_error": (c_char_p, []),
        "mu_device_info": (i32, [i32, c_char_p, i32, vp, vp]),
        "mu_host_hash64": (i32, [vp, sz, i32, u64, vp]),
        "mu_csr_row_col_sums_worksize": (sz, [i64, i64]),
        "mu_spmm_f32": (i32, [i64, i64, vp, vp, vp, vp, i32, vp, i32, vp]),
        "mu_tpack4_geometry": (i32, [i64, i64, i64, vp, vp, vp]),
        "mu_tune_set": (i32, [c_char_p, i32]),
        "mu_mofa_poisson_blocks": (i64, [i64, i64]),
        "mu_snf_affinity_f64": (i32, [i64, i32, i64, vp, i64, vp, dbl, dbl, vp, vp]),
        "mu_cluster_move_f64": (i32, [i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]),
    }
    for name, sig in want.items():
        assert _ffi.SIGNATURES[name] == sig, name
    assert len(_ffi.SIGNATURES) == len(_declared())


def test_ffi_parser_refuses_what_it_does_not_recognise():
    from muon_amd import _ffi

    ok = "/* c */ int mu_a(int64_t n, const float* d_x, void* stream);\nsize_t mu_b(void);"
    assert _ffi.parse_header(ok) == {"mu_a": (ctypes.c_int, [ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
                                     "mu_b": (ctypes.c_size_t, [])}
    for bad, word in (("int mu_a(unsigned n);", "unsigned"), ("int mu_a(float x);", "float"),
                      ("long mu_a(int n);", "long"), ("int mu_a(int n) { return n; }", "mu_a"),
                      ("struct mu_s { int a; };", "mu_s"), ("int other(int n);", "other")):
        with pytest.raises(_ffi.MuonAmdError, match=word):
            _ffi.parse_header(bad)


def test_host_pointers_pass_through_the_derived_table():
    """`int* count`, `int64_t* rows_per_block`, `uint64_t* h_out`, `const double* h_coef`: c_void_p in the table,
    given as byref(...) or a ctypes array by the callers"""
    import numpy as np

    from muon_amd import _ffi

    lib = _ffi.lib()
    n = ctypes.c_int(-7)
    assert lib.mu_device_count(ctypes.byref(n)) in (0, -3) and n.value >= 0  # (-3: MU_ERR_NO_DEVICE, count written 0)
    rpb, G, Ct = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.mu_tpack4_geometry(1000, 9000, 5000, ctypes.byref(rpb), ctypes.byref(G), ctypes.byref(Ct)) == 0
    assert rpb.value * (G.value - 1) < 1000 <= rpb.value * G.value and Ct.value > 0  # (the row blocks cover the rows)
    ct = ctypes.c_int(0)
    assert lib.mu_tpack4_geometry(1000, 9000, 5000, None, None, ctypes.byref(ct)) == 0 and ct.value == Ct.value
    b = np.arange(64, dtype=np.uint8)
    out, again = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.mu_host_hash64(b.ctypes.data, b.size, 1, 0, ctypes.byref(out)) == 0
    assert lib.mu_host_hash64(b.ctypes.data, b.size, 2, 0, ctypes.byref(again)) == 0 and out.value == again.value != 0
    coef = (ctypes.c_double * 4)(1, 1, 1, 1)
    assert lib.mu_cluster_move_f64(0, None, 4, 4, None, None, None, None, None, None, 9, None, None, coef, 0, None, None,
                                   None, None) == -1 and lib.mu_last_error()


def _public(cls):
    """the public callables a class defines itself, read without an instance"""
    return {n for n, v in vars(cls).items() if not n.startswith("_") and callable(getattr(cls, n))}


def _optional():
    from muon_amd._operators import OperatorSet

    return {n for n, v in vars(OperatorSet).items() if not n.startswith("_") and v is None}


def test_operator_set_partitions_the_hip_backend_exactly():
    from muon_amd import _operators
    from muon_amd._backend import HipBackend
    from muon_amd._operators import OperatorSet

    required, optional = set(OperatorSet.REQUIRED), _optional()
    assert len(required) == len(OperatorSet.REQUIRED) and not (required & optional)
    assert not any(hasattr(OperatorSet, n) for n in required)  # (declared, not stubbed)
    assert _public(OperatorSet) == set() and _operators.DECLARED == required | optional
    hip = _public(HipBackend)
    assert optional - hip == set(), "declared optional, but HipBackend has no such operator"
    assert hip == optional | required, sorted(hip ^ (optional | required))
    # the flags: declared with the defaults of a set that says nothing
    assert (OperatorSet.name, OperatorSet.skinny_mixed, OperatorSet.mofa_poisson_lik_with_b) == ("", False, False)
    assert (HipBackend.name, HipBackend.skinny_mixed, HipBackend.mofa_poisson_lik_with_b) == ("hip", True, True)


def test_cpu_test_backend_is_inside_the_contract():
    import inspect

    from muon_amd._backend import HipBackend
    from muon_amd._operators import OperatorSet
    from tests.cpu_backend import CpuTestBackend

    cpu = _public(CpuTestBackend)
    assert cpu <= _optional() | set(OperatorSet.REQUIRED), sorted(cpu - _optional() - set(OperatorSet.REQUIRED))
    assert set(OperatorSet.REQUIRED) <= cpu, sorted(set(OperatorSet.REQUIRED) - cpu)
    assert issubclass(CpuTestBackend, OperatorSet) and issubclass(HipBackend, OperatorSet)
    for name in sorted(cpu & _public(HipBackend)):
        a, b = (inspect.signature(getattr(c, name)).parameters for c in (HipBackend, CpuTestBackend))
        assert [(p.name, p.default, p.kind) for p in a.values()] == [(p.name, p.default, p.kind) for p in b.values()], name


def test_has_fails_loudly_on_an_undeclared_name():
    from muon_amd._backend import HipBackend
    from muon_amd._operators import OperatorSet, has
    from tests.cpu_backend import CpuTestBackend

    class Forwarding:  # (a double that hides one operator and forwards the rest, as the GPU tests build them)
        def __getattr__(self, name):
            if name == "chol_rinv":
                raise AttributeError(name)
            return getattr(be, name)

    be = CpuTestBackend()
    for ops in (OperatorSet(), be, HipBackend, Forwarding(), object()):
        with pytest.raises(AttributeError):
            has(ops, "no_such_operator")
        with pytest.raises(AttributeError):
            has(ops, "spmm", "can_ell16")
    for name in sorted(_optional()):
        assert has(OperatorSet(), name) is False and has(HipBackend, name) is True, name
    assert has(HipBackend, *OperatorSet.REQUIRED, *sorted(_optional()))
    assert has(be) and has(be, "spmm", "chol_rinv") and not has(be, "spmm", "csr_qc") and not has(be, "csr_qc", "spmm")
    assert has(Forwarding(), "spmm", "skinny_nn") and not has(Forwarding(), "chol_rinv") and not has(object(), "spmm")


def test_error_reporting_without_gpu_calls():
    from muon_amd import _ffi

    lib = _ffi.lib()
    # argument validation happens before any HIP call: usable without a device
    rc = lib.mu_spmm_f32(1, 1, None, None, None, None, 7, None, 0, None)
    assert rc == -1 and b"B must be" in lib.mu_last_error()
    rc = lib.mu_tfidf_scale(0, 0, None, None, None, None, None, 1.0, 4 | 1, None, None, None)
    assert rc == -1 and b"log_tfidf" in lib.mu_last_error()


def test_product_never_imports_oracle():
    pat = re.compile(r"^\s*(from|import)\s+oracle\b", re.M)
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "muon_amd")):
        for f in files:
            if f.endswith(".py"):
                p = os.path.join(base, f)
                if pat.search(open(p).read()):
                    bad.append(p)
    assert not bad, bad


def test_no_reference_sources_copied():
    # the reference is read where it lies; only fixtures produced by executing it are committed
    assert not os.path.exists(os.path.join(ROOT, "muon"))
    for f in os.listdir(os.path.join(ROOT, "tests", "golden")):
        assert f.endswith((".npz", ".py")), f


def test_stream_spmm_isa_keeps_out_of_the_asm_owned_registers(tmp_path):
    """The row-stream SpMM issues its window requests from inline asm into v[110..125], registers hipcc
    must never touch (a compiler copy of a register whose load is in flight reads stale data), and
    hipcc must not spill (its scratch loads would share vmcnt with the hand-counted requests).
    Audit the generated gfx950 ISA of every instance: no scratch, no compiler-issued instruction
    naming v110+, 126 allocated VGPRs."""
    import re
    import shutil

    from muon_amd.csrc import build as csrc_build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "spmm_win.s"
    csrc_build.device_asm("spmm_win.hip", out)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN[^\n:]*k_spmm_win[^\n:]*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text,
                         flags=re.S | re.M)
    # production instances only (MODE = 0, the second template argument); the timing ablations never
    # feed results to anybody
    kernels = [(n, b) for n, b in kernels if re.search(r"k_spmm_winILi\d+ELi0ELi|k_spmm_win_rngILi\d+E", n)]
    # K = 1..8 x (f32: B = 64 / 32 / 16; f64 blocks: B = 32 / 16) + the ranged B = 64 instances of r06 (K = 1..8), whose
    # per-range set-up must not keep anything alive across the slab loop (K = 7 / 8 spilled before it was made opaque)
    assert len(kernels) == 48
    reg = re.compile(r"\bv(\d+)\b|v\[(\d+):(\d+)\]")
    for name, body in kernels:
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




def test_poisson_matrix_core_sweep_isa(tmp_path):
    """k_pois_mfma (csrc/mofa_poisson.hip, r06): the sweep costs what its instruction count says - the f32 matrix
    instructions and the vector ALU do not overlap there - so the generated gfx950 ISA is pinned: accumulators in VGPRs
    (no v_accvgpr copies around every product: the file is built with -amdgpu-mfma-vgpr-form, csrc/build.py), no spills,
    no IEEE division sequence and no libm log expansion in the transform (one v_exp_f32 per prediction, one v_rcp_f32
    where the mode needs the sigmoid, one v_log_f32 where it needs the likelihood), KP / 4 + 4 matrix instructions per
    16 x 16 tile (KP / 4 in the likelihood-only mode).  f64 models: the same kernel on v_mfma_f64_16x16x4_f64 (two own
    tiles per wave, libm in the transform)."""
    import re
    import shutil

    from muon_amd.csrc import build as csrc_build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "-amdgpu-mfma-vgpr-form" in csrc_build.EXTRA["mofa_poisson.hip"]
    out = tmp_path / "mofa_poisson.s"
    csrc_build.device_asm("mofa_poisson.hip", out)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN[^\n:]*k_pois_mfmaI([fd])Li(\d+)ELi(\d)E[^\n:]*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text,
                         flags=re.S | re.M)
    assert len(kernels) == 32  # (f32, f64) x KP = 4, 8, 12, 16 x modes 0..3
    for name, t, kp, mode, body in kernels:
        kp, mode = int(kp), int(mode)
        tiles = 4 if t == "f" else 2  # PmMap<T>::OWN: 16-row own tiles per wave, all in one unrolled step
        assert "scratch_" not in body and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        assert "accvgpr" not in body, name
        count = lambda op: len(re.findall(r"^\s*" + op + r"\b", body, flags=re.M))
        op = "v_mfma_f32_16x16x4_f32" if t == "f" else "v_mfma_f64_16x16x4_f64"
        assert count(op) == tiles * (kp // 4 + (0 if mode == 2 else 4)), name
        m = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body)
        assert m and int(m.group(1)) <= 160, (name, m and m.group(1))
        if t == "d":
            continue  # (f64: libm's exp / log1p in the transform)
        assert "v_div_" not in body and "v_ldexp" not in body, name
        assert count("v_exp_f32_e32") + count("v_exp_f32_e64") == 4 * tiles, name
        assert count("v_rcp_f32_e32") + count("v_rcp_f32_e64") == (0 if mode == 2 else 4 * tiles), name
        assert count("v_log_f32_e32") + count("v_log_f32_e64") == (4 * tiles if mode in (2, 3) else 0), name


def test_jaakkola_sweep_isa(tmp_path):
    """k_jaakkola_sweep (csrc/mofa_bernoulli.hip, r06): 14 instances - (padded width, column tiles of the packed moments) x
    f32 / f64 - each without spills and with its accumulators in VGPRs; the matrix-instruction count of a 16-row step is
    OWN x (3 KP / 4 + 4 CT): the prediction and the two variance products, then one product per column tile and
    accumulator register."""
    import re
    import shutil

    from muon_amd.csrc import build as csrc_build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "-amdgpu-mfma-vgpr-form" in csrc_build.EXTRA["mofa_bernoulli.hip"]
    out = tmp_path / "mofa_bernoulli.s"
    csrc_build.device_asm("mofa_bernoulli.hip", out)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN[^\n:]*k_jaakkola_sweepI([fd])Li(\d+)ELi(\d+)E[^\n:]*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text,
                         flags=re.S | re.M)
    assert sorted((t, int(kp), int(ct)) for _, t, kp, ct, _ in kernels) == sorted(
        (t, kp, ct) for t in "df" for kp, ct in ((4, 1), (8, 2), (8, 3), (12, 4), (12, 5), (16, 7), (16, 9)))
    for name, t, kp, ct, body in kernels:
        kp, ct = int(kp), int(ct)
        own = 2 if (t == "f" and ct <= 5) else 1
        assert "scratch_" not in body and re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        assert "accvgpr" not in body, name
        op = "v_mfma_f32_16x16x4_f32" if t == "f" else "v_mfma_f64_16x16x4_f64"
        assert len(re.findall(r"^\s*" + op + r"\b", body, flags=re.M)) == own * (3 * kp // 4 + 4 * ct), name


def test_tpack4_isa_keeps_out_of_the_asm_owned_registers(tmp_path):
    """The fourth-generation transposition (csrc/tpack4.hip) keeps the next tile's header in v[88..91] and its 18 window
    slots in v[92..127], written by loads issued from inline asm one tile ahead: hipcc must stay below v88 (a copy or a
    spill of a register whose load is in flight reads stale data) and must not spill at all in the production instances
    (scratch traffic shares vmcnt with the hand-placed waits)."""
    import re
    import shutil

    from muon_amd.csrc import build as csrc_build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "tpack4.s"
    csrc_build.device_asm("tpack4.hip", out)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN[^\n:]*k_t4_fill[^\n:]*):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S | re.M)
    assert len(kernels) == 7  # (row stream | CSR arrays) x (stream target, CSR target, stream target with phase accounting) + the row stream through circular windows
    reg = re.compile(r"\bv(\d+)\b|v\[(\d+):(\d+)\]")
    for name, body in kernels:
        production = re.search(r"k_t4_fillILb[01]ELb0ELb[01]E", name) is not None
        m = re.search(r"\.amdhsa_next_free_vgpr (\d+)", body)
        assert m and int(m.group(1)) == 128, (name, m and m.group(1))
        if production:
            assert "scratch_" not in body, name
            assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body), name
        inasm = False
        for line in body.splitlines():
            if "#ASMSTART" in line:
                inasm = True
            elif "#ASMEND" in line:
                inasm = False
            elif not inasm and not line.lstrip().startswith((".", ";")):
                for a, b, c in reg.findall(line.split(";")[0]):
                    hi = int(a) if a else int(c)
                    assert hi < 88, (name, line)


def test_every_environment_switch_is_in_the_table_of_integration_md():
    """ONE table of the switches - every MUON_AMD_* variable the package or
    bench.py reads must be a row of it, and every row must still be read somewhere."""
    import re

    read = set()
    for base, _dirs, files in os.walk(os.path.join(ROOT, "muon_amd")):
        for f in files:
            if f.endswith(".py"):
                read |= set(re.findall(r"MUON_AMD_[A-Z0-9_]+", open(os.path.join(base, f)).read()))
    read |= set(re.findall(r"MUON_AMD_[A-Z0-9_]+", open(os.path.join(ROOT, "bench.py")).read()))
    read |= set(re.findall(r"MUON_AMD_BENCH_[A-Z0-9_]+", open(os.path.join(ROOT, "scripts", "bench_mofa.py")).read()))
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("**Switches** (environment"):text.index("Folded in r06 (no longer read)")]
    rows = set(re.findall(r"MUON_AMD_[A-Z0-9_]+", table))
    assert read <= rows, sorted(read - rows)
    assert rows <= read, sorted(rows - read)
    folded = set(re.findall(r"MUON_AMD_[A-Z0-9_]+", text[text.index("Folded in r06 (no longer read)"):]))
    assert not (folded & read), sorted(folded & read)
