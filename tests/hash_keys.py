"""LdsHash (sparse_matrix_mult_amd/csrc/smm_rowclass.hpp) restated on the CPU, and the adversarial key sets of its tests.

The table has HS = 2^BITS slots, a key k starts at ((unsigned)k * mult) >> (32 - BITS) and probes linearly, wrapping at HS.
The constants are read out of the header, so a change there moves the tests with it -- or fails them loudly.  Keys whose
start slot lies in the last `window` slots of the table ("window keys") pile up at the end of the table: inserting more
than `window` of them wraps to slot 0, builds one probe chain as long as the row, and makes a lookup of an absent window
key walk that whole chain before it may answer "absent"."""
import functools
import os
import re
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse_matrix_mult_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _hash_class(src, name):
    m = re.search(r"using\s+%s\s*=\s*HashClass<\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*>" % name, src)
    assert m, f"smm_rowclass.hpp: no 'using {name} = HashClass<HS, BITS, TPR, RPB>'"
    hs, bits, tpr, rpb = (int(g) for g in m.groups())
    assert hs == 1 << bits, f"{name}: HS {hs} is not 2^{bits}"
    return types.SimpleNamespace(name=name, HS=hs, BITS=bits, TPR=tpr, RPB=rpb, MAX=hs // 2)


_SRC = _source("smm_rowclass.hpp")
assert re.search(r"MAX\s*=\s*HS_\s*/\s*2\b", _SRC), "smm_rowclass.hpp: HashClass::MAX is no longer HS / 2"
WAVE_HASH = _hash_class(_SRC, "WaveHash")
WG_HASH = _hash_class(_SRC, "WgHash")
CLASSES = {"wave": WAVE_HASH, "wg": WG_HASH}
_m = re.search(r"start\(int k\)\s*\{\s*return\s*\(\(unsigned\)k\s*\*\s*(\d+)u\)\s*>>\s*\(32\s*-\s*BITS\)", _SRC)
assert _m, "smm_rowclass.hpp: LdsHash::start is no longer ((unsigned)k * MULTu) >> (32 - BITS)"
MULT = int(_m.group(1))
assert re.search(r"s\s*=\s*\(s\s*\+\s*1\)\s*&\s*\(HS\s*-\s*1\)", _SRC), "smm_rowclass.hpp: LdsHash no longer probes linearly"


def wave_rows_per_pass(n_cu):
    """Rows that one pass of a WaveHash kernel's grid covers on a device of n_cu compute units: the largest over the three
    launches in smm_api.hip (grid = min((rows + 3) / 4, n_cu * F) workgroups of RPB rows)."""
    f = [int(x) for x in re.findall(r"\(hc\[\w+\]\s*\+\s*3\)\s*/\s*4,\s*\(int64_t\)c->n_cu\s*\*\s*(\d+)\)", _source("smm_api.hip"))]
    assert len(f) == 3, f"smm_api.hip: expected the three WaveHash launches (triple, masked dot, masked row), found {len(f)}"
    assert WAVE_HASH.RPB == 4
    return WAVE_HASH.RPB * max(f) * int(n_cu)


def start(keys, bits):
    """Start slot of every key: ((unsigned)k * mult) >> (32 - bits), in uint64."""
    k = np.asarray(keys, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    return (((k * np.uint64(MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)).astype(np.int64)


def window_keys(bits, universe, window):
    """Every key in [0, universe) whose start slot lies in the last `window` slots of the table, ascending."""
    k = np.arange(universe, dtype=np.int64)
    return k[start(k, bits) >= (1 << bits) - window]


def simulate(keys, bits):
    """Plain linear probing of distinct keys in insertion order: (slot of each key, longest probe)."""
    hs = 1 << bits
    table = np.full(hs, -1, dtype=np.int64)
    slots = np.empty(len(keys), dtype=np.int64)
    longest = 0
    for i, (k, s) in enumerate(zip(np.asarray(keys).tolist(), start(keys, bits).tolist())):
        probe = 0
        while table[s] != -1:
            assert table[s] != k and probe < hs, "simulate: a repeated key or a full table"
            s = (s + 1) & (hs - 1)
            probe += 1
        table[s] = k
        slots[i] = s
        longest = max(longest, probe)
    return slots, longest


# ------------------------------------------------------------------------------ the key sets of the GPU tests
# name -> (class, window, universe).  A universe is the number of columns of the operand that carries the keys.
KEYSETS = {"wave": ("wave", 8, 24000), "wave_one_slot": ("wave", 1, 200000), "wg": ("wg", 64, 600000)}
SPARE = 64                  # window keys beyond MAX: rows of MAX + 1, and near-misses no row ever inserts


@functools.lru_cache(maxsize=None)
def keyset(name):
    """(class, window, universe, ascending window keys) of a named key set (read-only)."""
    cname, window, universe = KEYSETS[name]
    c = CLASSES[cname]
    keys = window_keys(c.BITS, universe, window)
    keys.setflags(write=False)
    return c, window, universe, keys


@functools.lru_cache(maxsize=None)
def random_keys(name, seed=7):
    """As many distinct random keys of the same universe as keyset(name) has, in random order (read-only)."""
    c, _, universe, keys = keyset(name)
    out = np.random.default_rng(seed).choice(universe, size=len(keys), replace=False).astype(np.int64)
    out.setflags(write=False)
    return out
