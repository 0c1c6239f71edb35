"""The stream rule of engine.py ("Streams") without a GPU: a fake torch and a fake library record the calls.

Every wrapper that reads, fills or returns a torch tensor waits for torch's current stream exactly when the context does not
launch on it, never when it does; the wait comes before the library call that touches torch's memory, and -- where a tensor
goes back to the caller -- the context is synchronised after it."""
import sys
import types

import pytest

from sparse_matrix_mult_amd import engine

SIDE = 0x7000                       # a raw stream value of the fake torch


class _Tensor:
    def __init__(self, n=4):
        self.n, self.device = n, ("cuda", 0)

    def data_ptr(self):
        return 0x1000

    def numel(self):
        return self.n


class _Library:
    """Every symbol is a function that records its name and succeeds; the few that report a size report a positive one."""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def call(*args):
            self.log.append(name)
            if name in ("smm_spgemm_symbolic", "smm_csr_mirror_symbolic"):
                args[-1]._obj.value = 5             # nnz, by reference
            return 5 if name in ("smm_result_nnz", "smm_csr_nnz") else 0
        return call


def _fake_torch(log, current):
    t = types.ModuleType("torch")
    stream = types.SimpleNamespace(cuda_stream=current, synchronize=lambda: log.append("torch.wait"))
    t.cuda = types.SimpleNamespace(current_stream=lambda device=None: stream)
    t.device = lambda *a: ("cuda", 0)
    t.empty = t.zeros = lambda n, **kw: _Tensor(n)
    t.int64 = t.int32 = t.float64 = None
    return t


# (context's stream, torch's current stream, do they differ)
PAIRS = [(None, 0, True), (None, SIDE, True), (0, SIDE, True), (SIDE, 0, True), (SIDE, SIDE + 8, True), (0, 0, False), (SIDE, SIDE, False)]


@pytest.fixture(params=PAIRS, ids=lambda p: f"ctx={p[0]}-torch={p[1]}")
def rig(request, monkeypatch):
    mine, current, apart = request.param
    log = []
    monkeypatch.setitem(sys.modules, "torch", _fake_torch(log, current))
    c = engine.Context.__new__(engine.Context)
    c.lib, c.handle, c.device, c.stream = _Library(log), 1, 0, mine
    ops = [engine.DeviceCSR(c, 2 + i, 3, 3, 4) for i in range(3)]
    yield types.SimpleNamespace(ctx=c, log=log, apart=apart, ops=ops)
    for o in ops:
        o.handle = None
    c.handle = None


def _check(rig, touches, returns_tensor):
    """touches: the library calls that read or write torch's memory, in order.  Different streams: a wait right before
    each of them -- nothing of the library in between --, and a context synchronise after the last when a tensor goes
    back.  Shared stream: no wait and no synchronise at all."""
    log = rig.log
    assert all(t in log for t in touches), log
    if not rig.apart:
        assert "torch.wait" not in log and "smm_ctx_synchronize" not in log, log
        return
    for t in touches:
        assert log[log.index(t) - 1] == "torch.wait", f"no wait right before {t}: {log}"
    last = max(i for i, x in enumerate(log) if x in touches)
    if returns_tensor:
        assert "smm_ctx_synchronize" in log[last + 1:], f"the context is not synchronised after {log[last]}: {log}"
    assert log.index("torch.wait") < log.index(touches[0])


def test_spgemm_torch(rig):
    out = rig.ctx.spgemm_torch(rig.ops[0], rig.ops[1])
    assert len(out) == 3
    _check(rig, ["smm_spgemm_numeric"], True)


def test_spgemm_mirrored_torch_both_halves(rig):
    rig.ctx.spgemm_mirrored_torch(rig.ops[0], rig.ops[1])
    _check(rig, ["smm_spgemm_numeric", "smm_csr_mirror_fill"], True)


@pytest.mark.parametrize("masked", [False, True])
def test_triple_sparse_torch(rig, masked):
    rig.ctx.triple_sparse_torch(rig.ops[0], rig.ops[1], mask=rig.ops[2] if masked else None)
    _check(rig, ["smm_result_copy_device"], True)


def test_csr_from_torch_and_values_changed_of_a_borrowed_operand(rig):
    b = rig.ctx.csr_from_torch(3, 3, _Tensor(), _Tensor(), _Tensor())
    _check(rig, ["smm_csr_from_device"], False)
    del rig.log[:]
    b.values_changed()
    _check(rig, ["smm_csr_update_values_device"], False)
    b.handle = None


def test_values_changed_from_an_address_leaves_the_order_to_the_caller(rig):
    rig.ops[0].values_changed(0x2000)
    assert rig.log == ["smm_csr_update_values_device"]


def test_values_into_and_pattern_torch(rig):
    rig.ops[0].values_into(_Tensor())
    _check(rig, ["smm_csr_copy_device"], True)
    del rig.log[:]
    rig.ops[0].values_into(0x2000)                      # an address: the caller's ordering
    assert rig.log == ["smm_csr_copy_device"]
    del rig.log[:]
    rig.ops[0].pattern_torch()
    _check(rig, ["smm_csr_copy_device"], False)


def test_device_blocks_and_builders_wait_before_they_read(rig):
    c, a = rig.ctx, rig.ops[0]
    for call, touch in ((lambda: c.spmm_into(a, _Tensor(), 1, 1, _Tensor(), 1), "smm_spmm"),
                        (lambda: c.sddmm_into(a, _Tensor(), 1, _Tensor(), 1, 1, _Tensor()), "smm_sddmm"),
                        (lambda: c.taper_into(_Tensor(), 1, _Tensor(), 1, 3, 3, 1, 0.5), "smm_taper_build"),
                        (lambda: c.interp_into(_Tensor(), 1, 3, 1, [[0.0, 1.0]]), "smm_interp_build"),
                        (lambda: c.innovation_solve_into(a, a, None, _Tensor(), 1, 1, _Tensor(), 1), "smm_innovation_solve")):
        del rig.log[:]
        call()
        assert touch in rig.log
        before = rig.log[:rig.log.index(touch)]
        assert ("torch.wait" in before) == rig.apart, f"{touch}: {rig.log}"
        del rig.log[:]
    c.spmm_into(a, 0x2000, 1, 1, 0x3000, 1)             # addresses: the caller's ordering
    assert "torch.wait" not in rig.log
