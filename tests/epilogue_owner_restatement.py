"""Index ownership in the CSR epilogue of smm_numeric (csrc/smm_kernels.hpp, SMM_EPI_OWNER), restated in plain Python.

A row of C of length rowlen starts at position rs of c_idx.  Its ordered list is cut into sub-runs -- (step, tile)
pieces [r0, r1), consecutive, possibly empty, covering [0, tail0) -- and a tail [tail0, rowlen).  Values are stored by
the unit (tile) that holds them.  Indices are stored by OWNERSHIP, in granules of S entries of c_idx:

    k     = rs mod S
    up(x) = the smallest y >= x with (rs + y) mod S == 0  =  ((x + k + S-1) & ~(S-1)) - k
    f(x)  = 0 if x == 0 else min(up(x), rowlen)

    a non-empty sub-run [r0, r1) stores the indices of [f(r0), f(r1));  an empty one stores nothing;
    the tail stores the indices of [f(tail0), rowlen), all of them in ONE unit: tile 0, or, for a symmetric product,
    the tile that holds the diagonal column (the first tile that is not skipped for a non-empty row).

Also here: the sub-run table of a row as smm_runs builds it (from the first-touch steps of the row), which the GPU
tests use to show that a case holds what its name says."""
import numpy as np

GRANULES = (8, 16)
TAIL_MIN_DEFAULT, TAIL_MIN_EXACT = 32, 64


def up(x, rs, S):
    k = rs & (S - 1)
    return ((x + k + S - 1) & ~(S - 1)) - k


def f(x, rs, rowlen, S):
    return 0 if x == 0 else min(up(x, rs, S), rowlen)


def owner_tile(gi, wc, symmetric):
    """The unit that stores the tail's indices of global row gi."""
    return gi // wc if symmetric else 0


def owned_ranges(subruns, tail0, rowlen, rs, S):
    """subruns: [(r0, r1)] in list order.  Returns [(value range, index range)] per sub-run, then the tail's."""
    out = []
    for r0, r1 in subruns:
        if r1 > r0:
            out.append(((r0, r1), (f(r0, rs, rowlen, S), f(r1, rs, rowlen, S))))
        else:
            out.append(((r0, r1), (r0, r0)))
    out.append(((tail0, rowlen), (f(tail0, rs, rowlen, S), rowlen)))
    return out


def check_row(subruns, tail0, rowlen, rs, S):
    """The three properties the kernel relies on.  Returns the index ranges that are not empty."""
    ranges = owned_ranges(subruns, tail0, rowlen, rs, S)
    at = 0
    kept = []
    for (v0, v1), (i0, i1) in ranges:
        assert 0 <= i0 <= i1 <= rowlen, "an owned range leaves the row"
        if i1 > i0:
            assert i0 == at, "owned ranges overlap or leave a gap"
            at = i1
            kept.append((i0, i1))
            # every owned position lies in the chunks of its value range: [v0, max(v1, i1)), at most S-1 past v1
            assert v0 <= i0 and i1 <= v1 + S - 1, "an owned range is not within S-1 of its value range"
            # whole granules, but for the row's first and last
            assert i0 == 0 or (rs + i0) % S == 0
            assert i1 == rowlen or (rs + i1) % S == 0
    assert at == rowlen, "owned ranges do not cover the row"
    return kept


# ------------------------------------------------------------------------------------------ the table of a row
def row_steps(A, B, i, gi=None):
    """First-touch steps of row i of A*B: per entry of A's row (stored order) the new columns it appends, in B's order.
    gi: global row index of a symmetric product (columns left of it are dropped), None otherwise."""
    seen = set()
    steps = []
    for j in A.indices[A.indptr[i]:A.indptr[i + 1]]:
        cols = B.indices[B.indptr[j]:B.indptr[j + 1]]
        new = [int(c) for c in cols if (gi is None or c >= gi) and c not in seen]
        # (B's rows hold no column twice in the tests that use this)
        seen.update(new)
        steps.append(new)
    return steps


def run_table(steps, wc, nct, tail_min):
    """smm_runs: ([(r0, r1, tile)] of the steps before the tail, tail0, rowlen)."""
    e_last = -1
    for e, s in enumerate(steps):
        if len(s) >= tail_min:
            e_last = e
    e0 = e_last + 1
    sub, at = [], 0
    edges = np.arange(nct + 1, dtype=np.int64) * wc
    for s in steps[:e0]:
        s = np.asarray(s, dtype=np.int64)
        assert np.all(np.diff(s) > 0), "B's rows are sorted"
        cut = at + np.searchsorted(s, edges)
        assert cut[-1] == at + len(s), "a column beyond the last tile"
        sub.extend((int(cut[t]), int(cut[t + 1]), t) for t in range(nct))
        at = int(cut[-1])
    return sub, at, at + sum(len(s) for s in steps[e0:])


def shared_geometry(ncols, lds_cols):
    """(nct, wc) of the default walk (make_geom in csrc/smm_api.hip)."""
    nct = (max(ncols, 1) + lds_cols - 1) // lds_cols
    return nct, (max(ncols, 1) + nct - 1) // nct


def exact_geometry(ncols, lds_cols, nw):
    """(nct, wc) of the SMM_EXACT walk: wc is a multiple of the nw waves (lds_cols far below the LDS limit)."""
    cols = max(ncols, 1)
    wc_max = max(lds_cols, nw)
    nct = (cols + wc_max - 1) // wc_max
    wc = (((cols + nct - 1) // nct + nw - 1) // nw) * nw
    if wc > wc_max:
        nct += 1
        wc = (((cols + nct - 1) // nct + nw - 1) // nw) * nw
    return nct, wc


def table_stats(A, B, nct, wc, tail_min, symmetric=False, row_offset=0):
    """What the rows of A*B hold under this geometry: counts of rows by kind and of sub-runs by length, the residues of
    the row starts, and every row checked against the ownership rule for both granules."""
    st = dict(tail=0, no_tail=0, all_tail=0, long=0, short=0, lead_other_tile=0, shared_granule=0, rs_mod16=set())
    rs = 0
    for i in range(A.shape[0]):
        steps = row_steps(A, B, i, i + row_offset if symmetric else None)
        sub, tail0, rowlen = run_table(steps, wc, nct, tail_min)
        if rowlen == 0:
            continue
        st["rs_mod16"].add(rs % 16)
        st["tail"] += 0 < tail0 < rowlen
        st["no_tail"] += tail0 == rowlen
        st["all_tail"] += tail0 == 0
        some = [(r0, r1, t) for r0, r1, t in sub if r1 > r0]
        st["long"] += sum(r1 - r0 >= 16 for r0, r1, _ in some)
        st["short"] += sum(r1 - r0 < 8 for r0, r1, _ in some)
        first_tile = owner_tile(i + row_offset, wc, symmetric)
        st["lead_other_tile"] += bool(some) and some[0][2] != first_tile
        for S in GRANULES:
            kept = check_row([(r0, r1) for r0, r1, _ in sub], tail0, rowlen, rs, S)
            if S == 8:          # an owner whose range holds entries of three sub-runs or more
                starts = np.asarray([r0 for r0, _, _ in some])
                st["shared_granule"] += sum(np.count_nonzero((starts >= i0) & (starts < i1)) >= 3 for i0, i1 in kept)
        rs += rowlen
    return st
