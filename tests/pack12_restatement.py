"""The "pack12" layout of B's packed payload in plain Python (smm_pack12_* in csrc/smm_kernels.hpp).

A piece is the entries of one (tile, row of B), sorted by tile-local column c, 0 <= c < wc <= 32 767.  It is laid out as
slots in groups of four; lane l of the piece walk owns group l.

  slot 0 of a group   a real entry, its column as a 15-bit absolute value
  slots 1-3           an 11-bit field d: d <= MAXGAP is the next real entry, column = previous column of the group + d;
                      d == PAD is a pad, which goes to the tile's sink accumulator, (wc + 1) & ~1

Slots are assigned greedily: an entry more than MAXGAP columns behind its predecessor in the same group turns that slot
and the rest of the group into pads and opens the next group.  Pads behind the last real entry fill up the last group.

In memory, with n = slot of the last real entry + 1 and G = ceil(n / 4):
  n doubles           (a mid-piece pad holds +0.0; trailing pads have no value slot)
  plane D, G dwords   bits 0-14 the absolute column, 15-25 field 1, 26-31 the low 6 bits of field 2
  plane H, G uint16   bits 0-4 the high 5 bits of field 2, 5-15 field 3
both planes together rounded up to 8 bytes; pieces start on ALIGN units of 8 bytes.
"""
import numpy as np

PAD, MAXGAP, ALIGN = 2047, 2046, 16
SINK = "sink"


def sink_of(wc):
    return (wc + 1) & ~1


def slots_of(cols):
    """The greedy slot list of a piece: a column per real entry, None per mid-piece pad.  len() is n."""
    out = []
    prev = None
    for c in cols:
        if len(out) % 4 and c - prev > MAXGAP:
            while len(out) % 4:
                out.append(None)
        out.append(int(c))
        prev = c
    return out


def units16(length):
    """8-byte units of a piece with 16-bit columns (smm_pack_count)."""
    return (length + ((length + 3) >> 2) + ALIGN - 1) & ~(ALIGN - 1)


def units12(n):
    g = (n + 3) >> 2
    return (n + ((6 * g + 7) >> 3) + ALIGN - 1) & ~(ALIGN - 1)


def eligible(n):
    """The four-entries-per-lane piece walk reads pieces of 129..256 slots."""
    return 128 < n <= 256


def encode(cols, vals, wc):
    """(values float64[n], D uint32[G], H uint16[G]) of one piece."""
    assert wc <= 32767 and all(0 <= c < wc for c in cols)
    slots = slots_of(cols)
    n = len(slots)
    g = (n + 3) >> 2
    v = np.zeros(n)
    D = np.zeros(g, np.uint32)
    H = np.zeros(g, np.uint16)
    it = iter(vals)
    fields = []
    prev = None
    for s, c in enumerate(slots + [None] * (4 * g - n)):
        if s % 4 == 0:
            assert c is not None
            fields.append(c)
        else:
            fields.append(PAD if c is None else c - prev)
            assert c is None or 0 <= c - prev <= MAXGAP
        if c is not None:
            prev = c
            v[s] = next(it)
    for k in range(g):
        a, f1, f2, f3 = fields[4 * k:4 * k + 4]
        D[k] = a | (f1 << 15) | ((f2 & 63) << 26)
        H[k] = (f2 >> 6) | (f3 << 5)
    return v, D, H


def decode(D, H, wc):
    """Per slot of every group: the accumulator the walk adds to -- a column or SINK.  One mask, three field extracts,
    three adds, three selects per lane; behind a pad the sums mean nothing, every later field of the group is a pad too."""
    out = []
    for dw, hw in zip(D.tolist(), H.tolist()):
        c0 = dw & 0x7fff
        f1, f2, f3 = (dw >> 15) & 0x7ff, (dw >> 26) | ((hw & 31) << 6), hw >> 5
        c1 = c0 + f1
        c2 = c1 + f2
        c3 = c2 + f3
        out += [c0, SINK if f1 == PAD else c1, SINK if f2 == PAD else c2, SINK if f3 == PAD else c3]
    return out


def fill_by_windows(cols, vals, wc, wave=64):
    """smm_pack12_fill's way to the same arrays: one wave per piece, `wave` entries per window.  A window starts at a
    group's slot 0; lane l takes entry l at slot = first slot + l; every entry more than MAXGAP behind its predecessor
    inside a group moves itself and the lanes after it to the next group; the lane at a group's slot 0 builds the group's
    words from the three lanes after it, so only groups that start in lanes 0 .. wave-4 are written in this window and
    the next one starts at the first group that was not."""
    n = len(slots_of(cols))
    g = (n + 3) >> 2
    v = np.full(n, np.nan)
    D = np.zeros(g, np.uint32)
    H = np.zeros(g, np.uint16)
    written = np.zeros(g, bool)
    k1, e0, s0 = len(cols), 0, 0
    while e0 < k1:
        lanes = min(wave, k1 - e0)
        c = [int(cols[e0 + l]) for l in range(lanes)]
        slot = [s0 + l for l in range(lanes)]
        for l in range(1, lanes):
            if c[l] - c[l - 1] > MAXGAP and slot[l] & 3:
                add = 4 - (slot[l] & 3)
                for m in range(l, lanes):
                    slot[m] += add
        last = e0 + wave >= k1
        late = [l for l in range(lanes) if l >= wave - 3 and slot[l] & 3 == 0]
        L = wave if last or not late else late[0]
        for l in range(min(L, lanes)):
            v[slot[l]] = vals[e0 + l]
            if slot[l] & 3:
                continue
            f, real = [], 1
            for q in (1, 2, 3):
                member = real == q and l + q < lanes and slot[l + q] == slot[l] + q
                real += member
                f.append(c[l + q] - c[l + q - 1] if member else PAD)
            assert not written[slot[l] >> 2]
            written[slot[l] >> 2] = True
            D[slot[l] >> 2] = c[l] | (f[0] << 15) | ((f[1] & 63) << 26)
            H[slot[l] >> 2] = (f[1] >> 6) | (f[2] << 5)
            if e0 + l + real < k1:
                v[slot[l] + real:slot[l] + 4] = 0.0
        s0 = slot[L] if L < lanes else slot[lanes - 1] + 1
        e0 += L
    assert written.all() and s0 >= n
    return v, D, H
