"""The fourteen entries of include/smm_hip.h that take a row-major block in and give a row-major block out -- smm_spmm,
smm_kron_apply, smm_triple_apply[_kron], smm_innovation_solve[_kron], their _host forms, and smm_innovation_solve_coef[_kron]
-- called through the C ABI itself, where the leading dimensions are the caller's (the Python wrappers always pass ld = k).

Pinned here: a host entry stages its blocks to the device and back without changing a bit of what its device twin computes
on the same strided layout, and writes no padding; every entry refuses each wrong argument with SMM_ERR_INVALID before it
allocates, launches or writes anything.  The smallest system on which these paths differ: D 3 x 3 and E 4 x 4 tridiagonal
(K = 12), H and A 9 x 12, R a 9 x 9 diagonal that makes H Q H^T + R strictly diagonally dominant, so that CG on 9 unknowns
is done well inside 20 iterations."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest
import scipy.sparse as sp

from helpers import rel_err
from kron_restatement import random_csr, tridiag

pytestmark = pytest.mark.gpu
VP = ctypes.c_void_p
EXACT, INVALID = 4, -2
SENTINEL = -7.25
TOL, MAXITER = 1e-8, 20
N, K = 9, 12
SHAPES = ((3, 3, 3), (3, 6, 5), (4, 6, 6))                     # (k, ld_in, ld_out)

# ops: the operand handles in call order (an R at the end may be NULL); rows of the block in and of the block out
Entry = namedtuple("Entry", "name ops in_rows out_rows kind host")
ENTRIES = [Entry(name + suffix, ops, i, o, kind, suffix == "_host")
           for name, ops, i, o, kind in (("smm_spmm", "a", K, N, "apply"),
                                         ("smm_kron_apply", "de", K, K, "apply"),
                                         ("smm_triple_apply", "hq", N, N, "apply"),
                                         ("smm_triple_apply_kron", "hde", N, N, "apply"),
                                         ("smm_innovation_solve", "hqr", N, N, "solve"),
                                         ("smm_innovation_solve_kron", "hder", N, N, "solve"))
           for suffix in ("", "_host")]
ENTRIES += [Entry("smm_innovation_solve_coef", "hqr", N, N, "coef", False),
            Entry("smm_innovation_solve_coef_kron", "hder", N, N, "coef", False)]
BY_NAME = {e.name: e for e in ENTRIES}
assert len(BY_NAME) == 14 and sum(e.host for e in ENTRIES) == 6


@pytest.fixture(scope="module")
def handles(ctx):
    D, E = tridiag(3), tridiag(4)
    H, A = random_csr(N, K, 0.4, 301), random_csr(N, K, 0.4, 302)
    dominant = np.asarray(abs(H) @ (sp.kron(D, E) @ (abs(H).T @ np.ones(N)))).ravel()
    R = sp.diags(dominant + np.random.default_rng(303).uniform(0.5, 1.5, N)).tocsr()
    hs = {key: ctx.csr_from_scipy(M) for key, M in (("d", D), ("e", E), ("h", H), ("a", A), ("r", R))}
    hs["q"] = ctx.kron_build(hs["d"], hs["e"])
    assert (hs["q"].rows, hs["q"].cols) == (K, K)
    yield hs
    for hd in hs.values():
        hd.close()


class Columns:
    """The per-column outputs of a solve (and the two histories of a recording one), holding the sentinel."""

    def __init__(self, k):
        self.arrays = [np.full(k, -7, np.int32), np.full(k, -7, np.int32), np.full(k, SENTINEL), np.full(k, SENTINEL)]
        self.hist = [np.full((MAXITER, k), SENTINEL), np.full((MAXITER, k), SENTINEL)]

    def untouched(self):
        return all(np.all(a == -7) for a in self.arrays[:2]) and all(np.all(a == SENTINEL) for a in self.arrays[2:] + self.hist)


def call(ctx, handles, ent, k, inp, ld_in, out, ld_out, cols=None, flags=EXACT, null_op=None, r=None, tol=TOL, maxiter=MAXITER,
         null_col=None, null_hist=None):
    """The entry with these arguments: its status.  inp / out are addresses (0 is NULL); null_op, null_col, null_hist: the
    position of one operand / per-column output / history passed as NULL; r: another handle in R's place."""
    ops = [handles[key].handle for key in ent.ops]
    if r is not None:
        ops[-1] = r.handle
    if null_op is not None:
        ops[null_op] = None
    args = [ctx.handle, *ops, flags, k, VP(inp), ld_in, VP(out), ld_out]
    if ent.kind != "apply":
        args += [tol, maxiter] + [None if j == null_col else VP(a.ctypes.data) for j, a in enumerate(cols.arrays)]
    if ent.kind == "coef":
        args += [None if j == null_hist else VP(a.ctypes.data) for j, a in enumerate(cols.hist)]
    return getattr(ctx.lib, ent.name)(*args)


def block(rows, k, ld, rng=None):
    """rows x ld of the sentinel, with standard normal data in the first k columns where rng is given."""
    b = np.full((rows, ld), SENTINEL)
    if rng is not None:
        b[:, :k] = rng.standard_normal((rows, k))
    return b


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ host equals device, strided
@pytest.mark.parametrize("k,ld_in,ld_out", SHAPES)
@pytest.mark.parametrize("name", [e.name for e in ENTRIES if e.host])
def test_a_host_entry_is_its_device_twin_on_strided_blocks(ctx, handles, name, k, ld_in, ld_out):
    import torch
    dev = torch.device("cuda", ctx.device)
    host, twin = BY_NAME[name], BY_NAME[name[:-len("_host")]]
    X = block(host.in_rows, k, ld_in, np.random.default_rng(310 + k + ld_in))
    Yh = block(host.out_rows, k, ld_out)
    dX, dY = torch.from_numpy(X).to(dev), torch.from_numpy(Yh).to(dev)
    torch.cuda.synchronize(dev)
    ch, cd = Columns(k), Columns(k)
    assert call(ctx, handles, host, k, X.ctypes.data, ld_in, Yh.ctypes.data, ld_out, ch) == 0, ctx.lib.smm_last_error()
    assert call(ctx, handles, twin, k, dX.data_ptr(), ld_in, dY.data_ptr(), ld_out, cd) == 0, ctx.lib.smm_last_error()
    ctx.synchronize()
    Yd = dY.cpu().numpy()
    assert np.all(Yh[:, k:] == SENTINEL), "the host entry wrote into its output's padding"
    assert np.all(Yd[:, k:] == SENTINEL), "the device entry wrote into its output's padding"
    assert np.all(np.isfinite(Yh[:, :k])) and np.any(Yh[:, :k] != SENTINEL)
    assert same_bits(Yh[:, :k], Yd[:, :k]), f"host and device differ: max rel {rel_err(Yh[:, :k], Yd[:, :k]):.3e}"
    if host.kind == "solve":
        for fld, a, b in zip(("iterations", "status", "residual_sq", "rhs_sq"), ch.arrays, cd.arrays):
            print(fld, a.tolist())
            assert same_bits(a, b), f"{fld}: host {a.tolist()}, device {b.tolist()}"
        assert np.all(ch.arrays[1] == 0) and 1 <= ch.arrays[0].max() <= MAXITER, "the system of this file converges"


# ------------------------------------------------------------------------------------------------ refusals
def refusals(ent, k):
    """(what, keyword arguments of call() that differ from the legal call): one wrong argument each."""
    yield "flag bit 1", dict(flags=EXACT | 1)
    yield "k = -1", dict(k=-1)
    yield "ld_in = k - 1", dict(ld_in=k - 1)
    yield "ld_out = k - 1", dict(ld_out=k - 1)
    yield "input NULL", dict(inp=0)
    yield "output NULL", dict(out=0)
    for j in range(len(ent.ops) - (ent.kind != "apply")):         # (a NULL R is legal)
        yield f"operand {ent.ops[j]} NULL", dict(null_op=j)
    if ent.kind == "apply":
        return
    for tol in (0.0, float("nan"), float("inf")):
        yield f"tol = {tol}", dict(tol=tol)
    yield "maxiter = -1", dict(maxiter=-1)
    for j, what in enumerate(("iterations", "status", "residual_sq", "rhs_sq")):
        yield f"{what} NULL", dict(null_col=j)
    yield "R of the wrong shape", dict(r="q")
    if ent.kind == "coef":
        yield "maxiter = 0", dict(maxiter=0)
        yield "maxiter = 65537", dict(maxiter=65537)
        yield "alpha NULL", dict(null_hist=0)
        yield "beta NULL", dict(null_hist=1)
        yield "k = 0 with d_x NULL", dict(k=0, out=0)


@pytest.mark.parametrize("name", list(BY_NAME))
def test_every_wrong_argument_is_refused_before_anything_is_written(ctx, handles, name):
    import torch
    dev = torch.device("cuda", ctx.device)
    ent, k, ld = BY_NAME[name], 3, 4
    X, Y = block(ent.in_rows, k, ld, np.random.default_rng(320)), block(ent.out_rows, k, ld)
    if ent.host:
        keep = (X, Y)
        inp, out = X.ctypes.data, Y.ctypes.data
        read_out = lambda: Y                                                       # noqa: E731
    else:
        # one buffer for both: the input, then the output behind it -- and an output range that begins inside the input's
        both = torch.from_numpy(np.concatenate([X, Y, block(1, k, ld)])).to(dev)
        torch.cuda.synchronize(dev)
        keep = both
        inp, out = both.data_ptr(), both.data_ptr() + 8 * ld * ent.in_rows
        read_out = lambda: both.cpu().numpy()[ent.in_rows:]                        # noqa: E731
    cols = Columns(k)
    legal = dict(k=k, inp=inp, ld_in=ld, out=out, ld_out=ld, cols=cols)
    assert call(ctx, handles, ent, **legal) == 0, ctx.lib.smm_last_error()
    assert call(ctx, handles, ent, **{**legal, "k": 0}) == 0, ctx.lib.smm_last_error()
    if name == "smm_innovation_solve":
        assert call(ctx, handles, ent, **{**legal, "k": 0, "out": 0}) == 0, "the plain solve takes a NULL d_x with k = 0"
    ctx.synchronize()
    assert np.any(read_out()[:, :k] != SENTINEL) and np.all(read_out()[:, k:] == SENTINEL)

    # the table, on outputs that hold the sentinel again
    cols = Columns(k)
    legal["cols"] = cols
    if ent.host:
        Y[:] = SENTINEL
    else:
        both[ent.in_rows:] = SENTINEL
        torch.cuda.synchronize(dev)
    before = ctx.live_bytes()
    rows = list(refusals(ent, k))
    if not ent.host:
        rows.append(("output range inside the input's", dict(out=inp + 8 * ld)))
    for what, wrong in rows:
        if "r" in wrong:
            wrong = {**wrong, "r": handles[wrong["r"]]}
        rc = call(ctx, handles, ent, **{**legal, **wrong})
        assert rc == INVALID, f"{name}, {what}: status {rc} ({ctx.lib.smm_last_error()})"
    assert ctx.lib.smm_ctx_synchronize(ctx.handle) == 0
    assert np.all(read_out() == SENTINEL), f"{name}: a refused call wrote into the output"
    assert cols.untouched(), f"{name}: a refused call wrote a per-column output"
    assert ctx.live_bytes() == before, f"{name}: {ctx.live_bytes() - before} bytes handed out by refused calls"
    del keep
