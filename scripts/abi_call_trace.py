#!/usr/bin/env python
"""Record every call a checkout makes into libmuon_amd.so, and compare two such records test by test.

`record` runs in ONE process: it imports the checkout's muon_amd, loads the library, puts a recording proxy in place of
the loaded handle (`_ffi._lib`) before any backend exists, then runs `smoke()` and, in-process, pytest with the arguments
given - `--repeat N` times over, each a run of its own in the record.  Every call is written as one string, the entry
name and its arguments normalised by the type `_ffi.SIGNATURES` declares: scalars by value, `char*` by its text, pointers
as `null` or `ptr`, ctypes arrays by their contents (an array of pointers as `null` / `ptr` each), and the last argument
of an entry whose prototype ends in `void* stream` as `stream`.  The record is JSON: {"runs": [{"smoke": [call, ...],
"tests": {test id: [call, ...]}}, ...]}; the calls of a fixture belong to the test that set it up.

`compare` takes records and prints, segment by segment (smoke, then every test id), whether all runs agree.  With
`--stable-from A.json` the segments on which A's own runs disagree (a test whose calls depend on, say, the memory that
is free) are left out and named.  A host refactor leaves every remaining segment identical.  Exit status 1 otherwise.

Usage: python scripts/abi_call_trace.py record CHECKOUT OUT.json [--repeat N] [pytest arguments ...]
       python scripts/abi_call_trace.py compare [--unordered] [--stable-from PARENT.json] A.json B.json
"""
import collections
import ctypes
import json
import os
import re
import sys


def _stream_entries(header_path):
    """The entries whose prototype ends in `void* stream`."""
    with open(header_path) as f:
        src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    return set(re.findall(r"\b(mu_\w+)\s*\([^()]*\bvoid\s*\*\s*stream\s*\)", src))


def _pointer(a):
    if isinstance(a, ctypes.Array):
        if issubclass(a._type_, (ctypes.c_void_p, ctypes.c_char_p)):
            return "[" + ",".join("ptr" if v else "null" for v in a) + "]"
        return "[" + ",".join(repr(v) for v in a) + "]"
    if isinstance(a, ctypes._SimpleCData):
        a = a.value
    if a is None or (isinstance(a, int) and a == 0):
        return "null"
    return "ptr"


def _scalar(ctype, a):
    if isinstance(a, ctypes._SimpleCData):  # (a test may hand over c_int64(10) itself)
        a = a.value
    if ctype is ctypes.c_char_p:
        return repr(a.decode() if isinstance(a, bytes) else a)
    if ctype is ctypes.c_double:
        return repr(float(a))
    return repr(int(a))


class Recorder:
    """Stands where the ctypes handle stood: every `mu_*` attribute is the library's function behind a wrapper that
    appends the normalised call to `self.calls`."""

    def __init__(self, handle, signatures, stream_entries):
        self._handle, self._signatures, self._streams = handle, signatures, stream_entries
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if name not in self._signatures:
            return fn
        argtypes, streamed, calls = self._signatures[name][1], name in self._streams, self.calls

        def traced(*args):
            words = [_pointer(a) if t is ctypes.c_void_p else _scalar(t, a) for t, a in zip(argtypes, args)]
            if streamed and len(args) == len(argtypes):
                words[-1] = "stream"
            calls.append(f"{name}({', '.join(words)})")
            return fn(*args)

        self.__dict__[name] = traced
        return traced


class _Segments:
    """pytest plugin: the calls recorded while a test (its set-up and tear-down included) ran, under its id."""

    def __init__(self, recorder):
        self.recorder, self.tests = recorder, {}

    def pytest_runtest_logstart(self, nodeid, location):
        del self.recorder.calls[:]

    def pytest_runtest_logfinish(self, nodeid, location):
        self.tests[nodeid] = list(self.recorder.calls)
        del self.recorder.calls[:]


def record(checkout, out_path, repeat, pytest_args):
    checkout = os.path.abspath(checkout)
    os.chdir(checkout)
    sys.path.insert(0, checkout)
    import pytest

    import __graft_entry__ as entry
    from muon_amd import _ffi

    recorder = Recorder(_ffi.lib(), _ffi.SIGNATURES, _stream_entries(_ffi.HEADER_PATH))
    _ffi._lib = recorder
    runs = []
    import muon_amd._backend as backend

    for _ in range(repeat):
        del recorder.calls[:]
        backend._default_backend = None  # (every run makes its backend, as a process of its own would)
        entry.smoke()
        run = {"smoke": list(recorder.calls), "tests": {}}
        if pytest_args:
            plugin = _Segments(recorder)
            run["pytest_status"] = int(pytest.main(list(pytest_args) + ["-p", "no:cacheprovider"], plugins=[plugin]))
            run["tests"] = plugin.tests
        runs.append(run)
    with open(out_path, "w") as f:
        json.dump({"checkout": checkout, "pytest_args": list(pytest_args), "runs": runs}, f)
    for i, run in enumerate(runs):
        print(f"run {i}: smoke {len(run['smoke'])} calls, {len(run['tests'])} tests, "
              f"{sum(map(len, run['tests'].values()))} calls, pytest status {run.get('pytest_status')}")
    return 0 if all(run.get("pytest_status", 0) == 0 for run in runs) else 1


def _segments(run):
    return dict({"smoke()": run["smoke"]}, **run["tests"])


def compare(paths, stable_from, unordered=False):
    def load(p):
        with open(p) as f:
            return [_segments(r) for r in json.load(f)["runs"]]

    unstable = set()
    if stable_from:
        own = load(stable_from)
        unstable = {k for k in own[0] if any(r.get(k) != own[0][k] for r in own[1:])}
    runs = [r for p in paths for r in load(p)]
    names = list(runs[0])
    missing = sorted(set().union(*map(set, runs)) - set(names)) + [k for k in names if any(k not in r for r in runs)]
    bad, reordered = [], []
    for k in names:
        if k in unstable or k in missing:
            continue
        first = runs[0][k]
        for r in runs[1:]:
            if r[k] != first and unordered and sorted(r[k]) == sorted(first):
                if k not in reordered:
                    reordered.append(k)
            elif r[k] != first:
                at = next((i for i, (a, b) in enumerate(zip(first, r[k])) if a != b), min(len(first), len(r[k])))
                ca, cb = collections.Counter(first), collections.Counter(r[k])
                only = (ca - cb, cb - ca)
                bad.append((k, at, first[at] if at < len(first) else None, r[k][at] if at < len(r[k]) else None, only))
                break
    compared = [k for k in names if k not in unstable and k not in missing]
    print(f"{len(runs)} runs, {len(names)} segments, {sum(len(runs[0][k]) for k in compared)} calls compared in "
          f"{len(compared)} segments; unstable in {stable_from or '-'}: {len(unstable)}; not in every run: {len(missing)}; "
          f"different: {len(bad)}" + (f"; same calls in another order: {len(reordered)}" if unordered else ""))
    for k in sorted(unstable):
        print(f"  unstable by itself, left out: {k}")
    for k in missing:
        print(f"  not in every run: {k}")
    for k in reordered:
        print(f"  same calls in another order: {k}")
    for k, at, a, b, only in bad:
        print(f"  different: {k}\n    call {at}: {a}\n         vs: {b}")
        if unordered:
            for side, c in zip(("first", "other"), only):
                print(f"    only in the {side} run: {sorted(c.elements())}")
    return 1 if bad or missing else 0


def main():
    argv = sys.argv[1:]
    if len(argv) >= 3 and argv[0] == "record":
        rest, repeat = argv[3:], 1
        if rest[:1] == ["--repeat"]:
            repeat, rest = int(rest[1]), rest[2:]
        sys.exit(record(argv[1], argv[2], repeat, rest))
    if len(argv) >= 3 and argv[0] == "compare":
        stable, unordered = None, argv[1] == "--unordered"
        if unordered:
            del argv[1]
        if argv[1] == "--stable-from":
            stable, argv = argv[2], argv[:1] + argv[3:]
        sys.exit(compare(argv[1:], stable, unordered))
    sys.exit(__doc__)


if __name__ == "__main__":
    main()
