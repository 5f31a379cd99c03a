"""The tune keys have one declared home, the table MU_TUNE_KEYS of muon_amd/csrc/common.hpp: every key that code, tests
or scripts name is a row of it, every row is read by the library or its Python layer, the keys retired with their kernel
variants are refused, and a fresh process starts from the table's defaults.  INTEGRATION.md lists the same table.
No GPU: mu_tune_* are host code."""
import json
import os
import re
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RETIRED = ("ell_mode", "tfidf_wide", "tfidf_abl", "tn_pipe", "nn_fast_off", "tpack4_m", "scale_stream_off", "tpack4_abl",
           "tpack4_late")


def _sources(*tops, ext):
    for top in tops:
        for base, _dirs, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(ext):
                    yield os.path.join(base, f)


def _declared():
    """{name: (default, largest)} as common.hpp writes it (kTuneAny: None)"""
    src = open(os.path.join(ROOT, "muon_amd", "csrc", "common.hpp")).read()
    body = src[src.index("#define MU_TUNE_KEYS(X)"):src.index("enum TuneKey")]
    rows = re.findall(r'\bX\((\w+), (\d+), (\d+|kTuneAny), "[^"]+"\)', body)
    assert len(rows) == len(re.findall(r"^\s*X\(", body, flags=re.M)), "a row of MU_TUNE_KEYS that this test cannot read"
    return {n: (int(d), None if m == "kTuneAny" else int(m)) for n, d, m in rows}


def _table():
    from muon_amd import _ffi
    from muon_amd._backend import HipBackend

    return HipBackend.tune_keys(types.SimpleNamespace(lib=_ffi.lib()))  # (the method reads nothing but the library)


def test_the_library_lists_the_declared_table():
    from muon_amd import _ffi

    lib, declared = _ffi.lib(), _declared()
    assert len(declared) >= 10
    assert _table() == {n: d for n, (d, _m) in declared.items()}
    assert list(_table()) == list(declared)  # (in the order of the table)
    n = lib.mu_tune_count()
    assert n == len(declared)
    for i in (-1, n):
        assert lib.mu_tune_name(i) is None and lib.mu_tune_default(i) == -1


def test_every_key_that_is_named_anywhere_is_in_the_table():
    table = _table()
    named = {}
    for p in _sources("muon_amd", "tests", "scripts", ext=".py"):
        src = open(p).read()
        for key in re.findall(r'\btune\(\s*"(\w+)"\s*[,)]', src) + re.findall(r'\bmu_tune_[sg]et\(\s*b"(\w+)"\s*[,)]', src):
            named.setdefault(key, p)
    assert len(named) >= 10
    assert set(named) <= set(table), {k: os.path.relpath(p, ROOT) for k, p in named.items() if k not in table}


def test_every_key_of_the_table_is_read_by_the_package():
    read = set()
    for p in _sources(os.path.join("muon_amd", "csrc"), ext=(".hip", ".hpp")):
        read |= set(re.findall(r"\btune\(kTune_(\w+)\)", open(p).read()))
    for p in _sources("muon_amd", ext=".py"):
        read |= set(re.findall(r'\bmu_tune_get\(\s*b"(\w+)"\s*\)', open(p).read()))
    table = set(_table())
    assert table <= read, sorted(table - read)
    assert read <= table, sorted(read - table)
    # inside csrc a key is an enumerator: no look-up by string outside the C ABI's own two functions
    for p in _sources(os.path.join("muon_amd", "csrc"), ext=(".hip", ".hpp")):
        assert not re.search(r'mu_tune_[sg]et\(\s*"', open(p).read()), p


def test_retired_keys_are_refused():
    from muon_amd import _ffi

    lib = _ffi.lib()
    assert not set(RETIRED) & set(_table())
    for key in RETIRED:
        assert lib.mu_tune_set(key.encode(), 1) != 0 and b"unknown key" in lib.mu_last_error(), key
        assert lib.mu_tune_get(key.encode()) == -1, key


def test_values_outside_a_keys_range_are_refused_and_change_nothing():
    from muon_amd import _ffi

    lib = _ffi.lib()
    for name, (default, largest) in _declared().items():
        key = name.encode()
        before = lib.mu_tune_get(key)
        assert lib.mu_tune_set(key, -1) != 0 and lib.mu_tune_get(key) == before, name
        if largest is not None:
            assert lib.mu_tune_set(key, largest + 1) != 0 and name.encode() in lib.mu_last_error(), name
            assert lib.mu_tune_get(key) == before, name
            assert lib.mu_tune_set(key, largest) == 0 and lib.mu_tune_get(key) == largest, name
        assert lib.mu_tune_set(key, before) == 0 and lib.mu_tune_get(key) == before, name


def test_a_fresh_process_starts_from_the_defaults_of_the_table():
    code = ("import json; from muon_amd import _ffi; lib = _ffi.lib(); "
            "print(json.dumps({lib.mu_tune_name(i).decode(): lib.mu_tune_get(lib.mu_tune_name(i)) "
            "for i in range(lib.mu_tune_count())}))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got == _table()
    assert got["tperm_flat"] == 1 and sum(got.values()) == 1  # (the one default that is not 0)


def test_the_table_of_integration_md_is_the_declared_one():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    part = text[text.index("**Tune keys**"):text.index("Retired with v")]
    rows = re.findall(r"^\| `(\w+)` \| (\d+) \| (\d+|any) \|", part, flags=re.M)
    assert {n: (int(d), None if m == "any" else int(m)) for n, d, m in rows} == _declared()
    retired = text[text.index("Retired with v"):]
    retired = retired[:retired.index("\n\n")]
    assert set(RETIRED) <= set(re.findall(r"`(\w+)`", retired))
