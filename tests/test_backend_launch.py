"""HipBackend._launch and ._work without a device: what arrives at the library, on which stream, inside which device
context, and what a status other than 0 raises.  The backend is made with ``__new__`` around a stub library whose
entries record their arguments."""
import ctypes

import pytest
import torch

from muon_amd import _ffi
from muon_amd._backend import HipBackend


class _StubLib:
    """Entries record (name, args) and return ``status``; ``mu_last_error`` is the library's message."""

    def __init__(self):
        self.calls, self.status, self.sizes = [], 0, {}

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.status
        return entry

    def mu_last_error(self):
        return b"stub: the launch was refused"

    def mu_stub_worksize(self, n):
        return self.sizes[n]


class _Ctx:
    def __init__(self, log):
        self.log = log

    def __enter__(self):
        self.log.append("enter")

    def __exit__(self, *exc):
        self.log.append("exit")
        return False


class _HostBackend(HipBackend):
    def _stream(self):
        return self.handle

    def _dev_ctx(self):
        return _Ctx(self.ctx_log)


@pytest.fixture
def be(monkeypatch):
    b = _HostBackend.__new__(_HostBackend)
    b.lib, b.device, b.handle, b.ctx_log = _StubLib(), torch.device("cpu"), 0x1000, []
    monkeypatch.setattr(_ffi, "_lib", b.lib)  # check() asks the loaded library for its message
    return b


def test_arguments_arrive_as_the_library_takes_them(be):
    t, u = torch.zeros(4), torch.ones(3, dtype=torch.float64)
    arr = (ctypes.c_int32 * 3)(1, 2, 3)
    n = ctypes.c_int(0)
    ref = ctypes.byref(n)
    be._launch(be.lib.mu_x, t, None, 7, 2.5, True, b"key", arr, ref, u)
    (name, args), = be.lib.calls
    assert name == "mu_x" and len(args) == 10
    assert args[0] == t.data_ptr() and type(args[0]) is int
    assert args[1] is None
    assert args[2] == 7 and type(args[2]) is int
    assert args[3] == 2.5 and type(args[3]) is float
    assert args[4] is True
    assert args[5] == b"key"
    assert args[6] is arr and args[7] is ref
    assert args[8] == u.data_ptr()


def test_stream_is_last_and_queried_per_call(be):
    t = torch.zeros(1)
    be._launch(be.lib.mu_x, 1, t)
    be.handle = 0x2000
    be._launch(be.lib.mu_y, t)
    be._launch(be.lib.mu_z)
    assert [(name, args[-1], len(args)) for name, args in be.lib.calls] == [("mu_x", 0x1000, 3), ("mu_y", 0x2000, 2),
                                                                             ("mu_z", 0x2000, 1)]


def test_device_context_once_around_the_call(be):
    def fn(*args):
        be.ctx_log.append("call")
        return 0

    be._launch(fn, torch.zeros(1))
    assert be.ctx_log == ["enter", "call", "exit"]


def test_status_raises_the_librarys_message_and_leaves_the_context(be):
    def fn(*args):
        be.ctx_log.append("call")
        return 3

    with pytest.raises(_ffi.MuonAmdError, match="libmuon_amd error 3: stub: the launch was refused"):
        be._launch(fn, torch.zeros(1))
    assert be.ctx_log == ["enter", "call", "exit"]


@pytest.mark.parametrize("size", [0, 5, 8, 4096])
def test_work_buffer(be, size):
    be.lib.sizes[11] = size
    work, wb = be._work(be.lib.mu_stub_worksize(11))
    assert work.dtype == torch.uint8 and work.dim() == 1 and work.numel() == size
    assert wb == size and type(wb) is int
    work, wb = be._work(be.lib.mu_stub_worksize(11), floor=8)
    assert work.dtype == torch.uint8 and work.numel() == max(size, 8)
    assert wb == size and type(wb) is int
