"""Operands that stand on the column widths where the sparse product's symbolic phase switches kernels, and the
dispatch of csrc/smm_api.hip restated in plain Python (expected_path), so that a GPU test can say which path it meant
to reach and a CPU test can show that the inputs reach it.

Every threshold is a function of n = columns of B (= columns of C):

    bm_words = ceil(n / 32) >= 512, 1024, 2048, 4096     LDS-hash marker class i exists            (sym_row_work, hmax[])
    n <= 63456 (CCS_MAX_WS)                               one-slab walk over the chunked column stream, against the
                                                          column-slab walk or the plain bitmap walk (use_slab_walk, sym_row_walk)
    bm_words * 32 + 31 <= 65535                           the 16-bit bitmap walk has its wide-chunk instantiation (launch_symbolic_w)
    n < 65535                                             16-bit column copy and ordered lists      (sym_row_walk)
    (bm_words + 1) * 4 <= 128 KB                          marker bitmap in LDS, against global      (sym_row_walk)

WIDTHS holds both sides of each of them."""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np
import scipy.sparse as sp

WIDTHS = (16352, 16353, 32736, 32737, 63455, 63456, 63457, 65503, 65504, 65505, 65533, 65534, 65535, 65536, 65537,
          131040, 131041, 1048544, 1048545)
POPULATIONS = ("light", "heavy")

# (lo, hi) neighbours of WIDTHS and the fields of Path the dispatch table says differ between them: {} where the pair is
# the far side of a triple and nothing may change
THRESHOLD_PAIRS = {
    (16352, 16353): {"hash_classes"},
    (32736, 32737): {"hash_classes"},
    (63455, 63456): set(),
    (63456, 63457): {"walk"},
    (65503, 65504): set(),
    (65504, 65505): {"hash_classes", "idle_col_fits16"},
    (65533, 65534): set(),
    (65534, 65535): {"list16"},
    (65535, 65536): set(),
    (65536, 65537): set(),
    (131040, 131041): {"hash_classes"},
    (1048544, 1048545): {"lds_bitmap"},
}
# the heavy population is on the column-slab walk from 63457 columns on, and that walk keeps slab-local 16-bit lists at
# every width: nothing changes at 65535 (the point of the 65535 | 65536 | 65537 triple)
THRESHOLD_PAIRS_HEAVY = {**THRESHOLD_PAIRS, (65534, 65535): set()}

N_SHORT = 30
MID = (256, 512, 1024, 2048)    # columns of the four middle rows of B: the most products of a row of each hash class
K = 10 + N_SHORT + len(MID)     # rows of B, one pattern each: dense, 8 residues, edge, 30 short, 4 middle
N_SMALL = 14                    # the first short rows hold 3 ... 5 columns: two of them fit a tiny row of C

# constants of the library that the restatement needs (csrc/smm_kernels.hpp, csrc/smm_api.hip)
HS = (512, 1024, 2048, 4096)    # smm_api.hip: constexpr int HS[NHC]
CCS_MAX_WS = 63456              # smm_kernels.hpp: constexpr int CCS_MAX_WS
WAVE = 64
TINY_G = 16                     # smm_ctx::tiny_max
LDS_COLS_SHARED, WAVES_SHARED = 20000, 16      # smm_ctx::lds_cols_shared / waves_shared
LDS_COLS, WAVES = 18000, 8                     # smm_ctx::lds_cols / waves
EXACT_SCRATCH_BYTES = 16 * WAVE + WAVE * 8     # sizeof(ExactScratch): int4 tab[WAVE] + head[WAVE * EX_UNROLL]


def special_columns(n):
    """First and last column, both sides of the first bitmap word's end, of the last full word's start, n - 2."""
    return (0, 31, 32, n - 33, n - 32, n - 2, n - 1)


class Patterns(NamedTuple):
    """Which row of B holds which pattern (the assignment is shuffled per case)."""
    dense: int
    residue: Tuple[int, ...]    # residue[r]: the row of columns c = r (mod 8)
    edge: int
    short: Tuple[int, ...]      # short[i] contains special_columns(n)[i % 7]; i < N_SMALL: 3 ... 5 columns
    mid: Tuple[int, ...]        # mid[i]: MID[i] columns, column 0 and column n - 1 among them


def _pattern_columns(n, rng):
    """The K column sets in pattern order: dense, residues 0 ... 7, edge, the short ones, the middle ones."""
    pats = [np.arange(n, dtype=np.int64)]
    pats += [np.arange(r, n, 8, dtype=np.int64) for r in range(8)]
    pats.append(np.concatenate([np.arange(40), np.arange(n - 40, n)]).astype(np.int64))
    spec = special_columns(n)
    for i in range(N_SHORT):
        length = int(rng.integers(3, 6)) if i < N_SMALL else int(rng.integers(6, 61))
        cols = np.zeros(0)
        while len(cols) != length:                # (a repeated draw: again)
            cols = np.unique(np.concatenate([rng.integers(0, n, size=length - 1), [spec[i % 7]]]))
        pats.append(cols.astype(np.int64))
    for length in MID:
        inner = 1 + rng.choice(n - 2, size=length - 2, replace=False)
        pats.append(np.sort(np.concatenate([[0], inner, [n - 1]])).astype(np.int64))
    return pats


def _csr(rows_cols, n_cols, rng):
    indptr = np.zeros(len(rows_cols) + 1, np.int32)
    indptr[1:] = np.cumsum([len(c) for c in rows_cols])
    indices = np.concatenate(rows_cols).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    m = sp.csr_matrix((rng.uniform(-1.0, 1.0, size=int(indptr[-1])), indices, indptr), shape=(len(rows_cols), n_cols))
    m.has_sorted_indices = True
    m.has_canonical_format = True
    return m


def heavy_rows(n):
    """Rows of A of the heavy population: 64 where eight dense rows alone are 8e6 products."""
    return 64 if n > 200000 else 256


def _row_recipes(n, population, m, rng):
    """Per row of A the list of PATTERN numbers it names (0 dense, 1 ... 8 residues, 9 edge, 10 ... short, 40 ... middle)."""
    small = lambda: 10 + int(rng.integers(0, N_SMALL))
    short = lambda: 10 + int(rng.integers(0, N_SHORT))
    s0, s1 = 10, 10 + 6                          # small short rows holding column 0 and column n - 1 (6 = 6 mod 7)
    res_last = 1 + (n - 1) % 8
    both_ends = [1, res_last] if res_last != 1 else [1, 5]      # two residue rows that hold column 0 and column n - 1

    # Rows on both sides of every hash class's limit (256, 512, 1024, 2048 products), all holding column 0 and column
    # n - 1: a middle row alone is the most its class takes, with a small row (3 ... 5 columns) it is the least of the next
    # class -- or of the bitmap / column-stream walk where that class does not exist at this width
    m0, m1, m2, m3 = (10 + N_SHORT + i for i in range(4))
    limits = [[m0], [m0, small()], [m0, short()], [m1], [m1, small()], [m0, m1], [m2], [m2, small()], [m1, m2], [m3],
              [m3, small()]]

    def tiny():
        return [small() for _ in range(int(rng.integers(1, 4)))]          # <= 3 x 5 = 15 products

    def hashed():                                # at most 200 products: the edge row (80) and up to two short rows, or three
        if rng.integers(0, 2):
            return [9] + [short() for _ in range(int(rng.integers(0, 3)))]
        return [short() for _ in range(3)]

    def residues(k):
        return [1 + int(r) for r in rng.choice(8, size=k, replace=False)]

    def heavy():                                 # two or three residue rows and up to three short ones or the edge row
        # (beyond 200 000 columns two: three would pass the budget of 2e7 products)
        k = 2 if n > 200000 or rng.integers(0, 3) else 3
        return residues(k) + [short() for _ in range(int(rng.integers(0, 3)))] + ([9] if rng.integers(0, 4) == 0 else [])

    def dense():
        return [0] + [short() for _ in range(int(rng.integers(0, 3)))] + ([9] if rng.integers(0, 2) else [])

    if population == "light":
        n_long = m // 16                         # the only rows that name a residue or the dense row
        recipes = [[0, 9], both_ends + [s0]] + [dense() if i % 8 == 0 else residues(int(rng.integers(1, 3))) + [short()]
                                                  for i in range(n_long - 2)]
        recipes += [[s0, s1], [9, s0, s1]] + limits      # a tiny and a hashed row that hold column 0 and column n - 1
        n_empty = 6
        while len(recipes) < m - n_empty:
            recipes.append(tiny() if rng.integers(0, 2) else hashed())
        recipes += [[] for _ in range(n_empty)]
    elif population == "heavy":
        n_heavy = (m * 76 + 99) // 100           # > 3/4 of the rows, the eight dense ones among them
        recipes = [dense() for _ in range(8)] + [both_ends + [9]] + [heavy() for _ in range(n_heavy - 9)]
        recipes += [[s0, s1]] + limits
        n_empty = 3
        while len(recipes) < m - n_empty:
            recipes.append(tiny() if rng.integers(0, 2) else hashed())
        recipes += [[] for _ in range(n_empty)]
    else:
        raise ValueError(population)
    order = rng.permutation(m)                   # classes interleaved, not grouped
    return [sorted(set(recipes[i])) for i in order]


@functools.lru_cache(maxsize=None)
def _case(n, population, seed):
    rng = np.random.default_rng([seed, n, POPULATIONS.index(population)])
    pats = _pattern_columns(n, rng)
    where = rng.permutation(K)                   # pattern p is row where[p] of B: first-touch order in both directions
    rows = [None] * K
    for p in range(K):
        rows[where[p]] = pats[p]
    B = _csr(rows, n, rng)
    m = 256 if population == "light" else heavy_rows(n)
    recipes = _row_recipes(n, population, m, rng)
    A = _csr([np.sort(where[np.array(r, dtype=np.int64)]) if r else np.zeros(0, np.int64) for r in recipes], K, rng)
    layout = Patterns(int(where[0]), tuple(int(x) for x in where[1:9]), int(where[9]),
                      tuple(int(x) for x in where[10:10 + N_SHORT]), tuple(int(x) for x in where[10 + N_SHORT:]))
    return A, B, layout


def operands(n, population, seed=0):
    """scipy CSR A (m x K) and B (K x n), canonical, values in [-1, 1).  Cached: do not modify."""
    A, B, _ = _case(n, population, seed)
    return A, B


def layout(n, population, seed=0):
    return _case(n, population, seed)[2]


def arrays(m):
    return (np.ascontiguousarray(m.indptr, dtype=np.int32), np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def oracle_result(n, population, seed=0):
    """(indptr, indices, data) of the CPU oracle for operands(n, population, seed), first-touch order.  Shared between
    the CPU and the GPU module: read only."""
    from oracle import oracle
    A, B = operands(n, population, seed)
    out = oracle.sparse(arrays(A), arrays(B), n)
    for x in out:
        x.setflags(write=False)
    return out


def abs_arrays(m):
    """arrays(|m|) without scipy's abs(), which sorts a non-canonical matrix and sums its repeated entries IN PLACE."""
    ptr, idx, val = arrays(m)
    return ptr, idx, np.abs(val)


def oracle_magnitude(n, population, seed=0):
    """The oracle on |A|, |B|: per entry of C the sum of the magnitudes of its terms (the scale of the value bound)."""
    from oracle import oracle
    A, B = operands(n, population, seed)
    return oracle.sparse(abs_arrays(A), abs_arrays(B), n)[2]


# ------------------------------------------------------------------------------ operands of the further cases
def symmetric_operands(n, row0, seed=0, m=256):
    """A row shard (m x n, global rows row0 ...) and B (n x n) for the symmetric product: the heavy population's rows of
    A, each row of the K-row B it names sent to one of the rows of this B that repeat it.  Row i of B is row i mod K of the
    K-row B; its thirteen long rows (dense, residues, middle) only in the first 2 K rows -- repeated all the way down B
    would hold n^2 / 20 = 2e8 entries -- and empty below."""
    A40, B40, lay = _case(n, "heavy", seed)
    rng = np.random.default_rng([seed, n, row0, 7])
    long_rows = {lay.dense, *lay.residue, *lay.mid}
    reps = n // K
    rows_cols = []
    for i in range(n):
        p = i % K
        if p in long_rows and i >= 2 * K:
            rows_cols.append(np.zeros(0, np.int32))
        else:
            rows_cols.append(B40.indices[B40.indptr[p]:B40.indptr[p + 1]])
    B = _csr(rows_cols, n, rng)
    a_rows = []
    for i in range(m):
        named = A40.indices[A40.indptr[i]:A40.indptr[i + 1]].astype(np.int64)
        rep = np.array([int(rng.integers(0, 2 if int(p) in long_rows else reps)) for p in named], dtype=np.int64)
        a_rows.append(np.sort(named + K * rep))
    A = _csr(a_rows, n, rng)
    return A, B


def zero_padded(A, n, row0):
    """A (m x n) as rows row0 ... row0 + m of an otherwise empty n x n matrix."""
    indptr = np.zeros(n + 1, np.int32)
    indptr[row0 + 1:row0 + A.shape[0] + 1] = A.indptr[1:]
    indptr[row0 + A.shape[0] + 1:] = A.indptr[-1]
    return sp.csr_matrix((A.data, A.indices, indptr), shape=(n, n))


def unsorted_with_repeat(B, layout_, seed=0):
    """B with the entries of every row in random order and one entry stored twice (the last column of the residue row
    that holds column n - 1, with a value of its own): neither sorted nor free of repeated columns."""
    from helpers import shuffle_rows
    n = B.shape[1]
    r = layout_.residue[(n - 1) % 8]
    S = shuffle_rows(B, seed + 11)
    at = int(S.indptr[r + 1])
    indices = np.insert(S.indices, at, n - 1).astype(np.int32)
    data = np.insert(S.data, at, 0.3125)
    indptr = S.indptr.copy()
    indptr[r + 1:] += 1
    out = sp.csr_matrix((data, indices, indptr), shape=B.shape)
    out.has_sorted_indices = False
    out.has_canonical_format = False
    return out


# ------------------------------------------------------------------------------ the dispatch, restated
class Path(NamedTuple):
    hash_classes: Tuple[bool, ...]   # which of the four LDS-hash marker classes exist
    list16: bool                     # 16-bit ordered lists (and, on the row walk, the 16-bit copy of B's columns)
    walk: str                        # "ccs": one slab of the chunked stream; "slab": column slabs; "bitmap": smm_symbolic
    idle_col_fits16: bool            # bitmap walk on 16-bit columns: the wide-chunk instantiation exists
    lds_bitmap: bool                 # bitmap walk: the marker bitmap fits LDS
    slab_dominant: bool              # use_slab_walk's `dominant`
    tps: Optional[int]               # slab walk: tiles per slab, slab width, slabs
    ws: Optional[int]
    n_slabs: Optional[int]
    n_tiny: int                      # rows per bin of the symbolic phase (row walk; the slab walk bins nothing)
    n_hash: Tuple[int, ...]
    n_rest: int
    ub: np.ndarray                   # per row of A: the capacity of its list, min(products, columns right of the diagonal)
    row_class: np.ndarray            # per row of A: -1 none, 0 ... 3 hash class, 4 rest, 5 tiny (16 lanes), 6 tiny (32 lanes)

    def dispatch(self):
        """The fields that depend on the width alone once the population is fixed."""
        return {k: getattr(self, k) for k in ("hash_classes", "list16", "walk", "idle_col_fits16", "lds_bitmap")}


def tile_geometry(n, exact=False):
    """(nct, wc) of make_geom under the default tuning."""
    cols = max(n, 1)
    if not exact:                                                        # make_geom: `if (!exact)`
        nct = (cols + LDS_COLS_SHARED - 1) // LDS_COLS_SHARED            # g.nct = ceil(cols / lds_cols_shared)
        return nct, (cols + nct - 1) // nct                              # g.wc = ceil(cols / nct)
    nw = WAVES
    lds_max = (160 * 1024 - nw * EXACT_SCRATCH_BYTES - 64 * 8) // 8 - 2  # const int64_t lds_max = ...
    wc_max = max(min(LDS_COLS, lds_max), nw)                             # wc_max = max(min(lds_cols, lds_max), nw)
    nct = (cols + wc_max - 1) // wc_max
    wf = ((cols + nct - 1) // nct + nw - 1) // nw
    if wf * nw > wc_max:                                                 # rounding up overshot the LDS budget
        nct += 1
        wf = ((cols + nct - 1) // nct + nw - 1) // nw
    return nct, wf * nw


def slab_geometry(n, exact=False):
    """(tps, ws, n_slabs) of sym_slab_walk under the default tuning: tiles per slab, slab width, slabs."""
    nct, wc = tile_geometry(n, exact)
    tps = max(1, min(8, CCS_MAX_WS // wc))                               # tps = max(1, min(8, ws_cap / g.wc))
    while tps > 1 and (160 * 1024) // ((((tps * wc + 31) // 32) + WAVE) * 4) < 28:
        tps -= 1                                                         # fewer than 28 waves per CU: one tile less
    return tps, tps * wc, (nct + tps - 1) // tps                         # p->ws = tps * g.wc; n_slabs = ceil(nct / tps)


def expected_path(n, A, B, exact=False, symmetric=False, row_offset=0, safe=False, narrow=True):
    """What smm_spgemm_symbolic does with A (m x k) and B (k x n) under the default tuning.  safe: B has unsorted rows
    or repeated columns; narrow: smm_ctx_tune_narrow."""
    m = A.shape[0]
    b_len = np.diff(B.indptr).astype(np.int64)
    na = np.diff(A.indptr).astype(np.int64)
    prod = np.zeros(m, np.int64)                                         # smm_row_work: products[row]
    np.add.at(prod, np.repeat(np.arange(m), na), b_len[A.indices])
    cap = np.full(m, n, np.int64)                                        # int64_t cap = ncols;
    if symmetric:                                                        # if (sym) cap = gi < ncols ? ncols - gi : 0
        gi = np.arange(m, dtype=np.int64) + row_offset
        cap = np.where(gi < n, n - gi, 0)
    ub = np.minimum(prod, cap)                                           # ub[row] = s < cap ? s : cap

    bm_words = (n + 31) // 32                                            # sym_row_work: bm_words = (ncols + 31) / 32
    bm_bytes = (bm_words + 1) * 4                                        # + the guard word
    hmax, classes = [], []
    for i in range(4):        # hmax[i] = (!safe && bm_bytes > HS[i] * 4) ? HS[i] / 2 : (i ? hmax[i - 1] : 0)
        exists = (not safe) and bm_bytes > HS[i] * 4
        classes.append(exists)
        hmax.append(HS[i] // 2 if exists else (hmax[i - 1] if i else 0))
    hmax1 = hmax[3]

    # smm_bin_rows<int64_t>(ub, spec{NHC, hmax}, tiny_max, prod, a_ptr)
    row_class = np.full(m, -1, np.int64)
    row_class[ub > 0] = 4                                                # b = spec.nb
    for q in (3, 2, 1, 0):                                               # if (n <= thr[q]) b = q, the smallest q last
        row_class[(ub > 0) & (ub <= hmax[q])] = q
    t1 = (prod > 0) & (prod <= TINY_G) & (na <= TINY_G)                  # u <= tiny_max && na <= tiny_max
    t2 = ~t1 & (prod > 0) & (prod <= 2 * TINY_G) & (na <= 2 * TINY_G)
    row_class[t1] = np.where(ub[t1] > 0, 5, -1)                          # b = n > 0 ? spec.tiny_bin : -1
    row_class[t2] = np.where(ub[t2] > 0, 6, -1)
    n_rest = int((row_class == 4).sum())
    n_hash = tuple(int((row_class == q).sum()) for q in range(4))
    n_tiny = int((row_class >= 5).sum())

    nct, wc = tile_geometry(n, exact)
    # use_slab_walk: wide = ncols > ws_cap && g.wc <= ws_cap && g.wc <= 32767
    wide = n > CCS_MAX_WS and wc <= CCS_MAX_WS and wc <= 32767
    dominant = hmax1 == 0 or 2 * n_rest >= m                             # r.hmax1 == 0 || 2 * sbin[SB_REST] >= m
    slab = narrow and wide and dominant and not safe                     # sym_ccs, sorted B, slab_mode: defaults
    tps = ws = n_slabs = None
    if slab:
        tps, ws, n_slabs = slab_geometry(n, exact)
        list16, walk = True, "slab"                                      # sym_slab_walk: p->list16 = true
    else:
        list16 = narrow and n < 65535                                    # sym_row_walk: narrow_idx && ncols < 65535 && b->cols < 65535
        # use_ccs = sym_ccs && list16 && !safe && ncols <= CCS_MAX_WS && nbm > 0
        walk = "ccs" if (list16 and not safe and n <= CCS_MAX_WS and n_rest > 0) else "bitmap"
    return Path(hash_classes=tuple(classes), list16=list16, walk=walk,
                idle_col_fits16=bm_words * 32 + 31 <= 65535,             # launch_symbolic_w: !I16 || words * 32 + 31 <= 65535
                lds_bitmap=bm_bytes <= 128 * 1024,                       # sym_row_walk: ldsbm = bm_bytes <= 128 * 1024
                slab_dominant=dominant, tps=tps, ws=ws, n_slabs=n_slabs,
                n_tiny=n_tiny, n_hash=n_hash, n_rest=n_rest, ub=ub, row_class=row_class)


def expected_launches(path):
    """Launch name -> whether the symbolic phase of a FRESH pair of handles launches it at least once."""
    # (smm_symbolic_hash is launched once per hash class that has rows: hash_launches counts them)
    row_walk = path.walk != "slab"
    return {
        "smm_slab_rowcnt": path.walk == "slab",
        "smm_ccs_fill": path.walk in ("ccs", "slab"),
        "smm_idx16": row_walk and path.list16,
        "smm_symbolic_hash": row_walk and any(e and c > 0 for e, c in zip(path.hash_classes, path.n_hash)),
        "smm_symbolic_tiny": row_walk and path.n_tiny > 0,
    }


def hash_launches(path):
    """Launches of smm_symbolic_hash: one per hash class that exists and has rows (sym_row_walk), none on the slab walk."""
    return sum(1 for e, c in zip(path.hash_classes, path.n_hash) if e and c > 0) if path.walk != "slab" else 0
