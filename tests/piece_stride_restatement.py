"""The strided layout of the pack12 payload in plain numpy (smm_pack12_len16 / smm_pack12_fill with a stride in
csrc/smm_kernels.hpp, the rule in ensure_pack of csrc/smm_api.hip).  The pieces themselves are those of
tests/pack12_restatement.py, byte for byte; only where they lie changes.

  stride              units12(longest n): the longest piece's size in 8-byte units, a multiple of ALIGN (128 bytes);
                      units12 grows with n, so the longest n decides
  piece (tile t, row k)  starts at unit (t * rows + k) * stride; behind its n doubles, plane D and plane H nothing is
                      written up to the next piece's start, and nothing is read there
  len16[t * rows + k] n as uint16 (n <= 256) -- the only table; the compact layout's {first unit, n} descriptors are gone
  the allocation      stride * rows * nct + SLACK units

The rule (all on the host, from the counts smm_pack12_count leaves): strided iff
  the pack12 rule holds (longest n in 129..256, and under mode 1 the operand is smaller as pack12 than with 16-bit columns),
  stride * rows * nct <= 1.5 x the compact pack12 payload (a capacity condition; mode 2 waives it),
  stride * rows * nct + SLACK < 2^31 - 1 units (the walk's unit index is an int).
"""
import numpy as np

from pack12_restatement import ALIGN, eligible, encode, slots_of, units12, units16

SLACK = 304                  # units the walk can touch behind a piece's start with n clamped to 256: 64 x 32 B + 256 B + 128 B
INT32_MAX = 2 ** 31 - 1


def piece_ns(pieces):
    """pieces[t][k] = sorted tile-local columns of (tile t, row k) -> n of every piece, [nct][rows]."""
    return np.array([[len(slots_of(cols)) for cols in tile] for tile in pieces], np.int64).reshape(len(pieces), -1)


def stride_of(ns):
    return units12(int(np.max(ns))) if np.size(ns) else 0


def compact_units(ns):
    return int(sum(units12(int(n)) for n in np.ravel(ns)))


def sixteen_bit_units(lengths):
    return int(sum(units16(int(n)) for n in np.ravel(lengths)))


def pack12_rule(ns, lengths, pack12_mode=1):
    longest = int(np.max(ns)) if np.size(ns) else 0
    if pack12_mode == 0 or not eligible(longest):
        return False
    return pack12_mode == 2 or compact_units(ns) < sixteen_bit_units(lengths)


def strided_rule(ns, lengths, stride_mode=1, pack12_mode=1):
    """ns / lengths: slots and entries of every piece, [nct][rows]."""
    if stride_mode == 0 or not pack12_rule(ns, lengths, pack12_mode):
        return False
    total = stride_of(ns) * int(np.size(ns))
    if total + SLACK >= INT32_MAX:
        return False
    return stride_mode == 2 or 2 * total <= 3 * compact_units(ns)


def first_unit(t, k, rows, stride):
    return (t * rows + k) * stride


def piece_bytes(cols, vals, wc):
    """The bytes of one piece: n doubles, plane D, plane H -- no pad behind them."""
    if not len(cols):
        return b""
    v, D, H = encode(cols, vals, wc)
    return v.tobytes() + D.tobytes() + H.tobytes()


def build(pieces, values, wc, fill=0xA5):
    """(payload bytes as uint8 -- unwritten bytes hold `fill` --, len16 uint16[nct * rows], stride)."""
    nct, rows = len(pieces), len(pieces[0])
    ns = piece_ns(pieces)
    stride = stride_of(ns)
    pay = np.full(8 * (stride * nct * rows + SLACK), fill, np.uint8)
    len16 = np.zeros(nct * rows, np.uint16)
    for t in range(nct):
        for k in range(rows):
            raw = np.frombuffer(piece_bytes(pieces[t][k], values[t][k], wc), np.uint8)
            assert len(raw) <= 8 * stride
            at = 8 * first_unit(t, k, rows, stride)
            pay[at:at + len(raw)] = raw
            len16[t * rows + k] = ns[t, k]
    return pay, len16, stride


def walk_extent(n):
    """Bytes from a piece's first byte that the four-entries-per-lane walk loads for a piece of n slots: ceil(n / 4) lanes
    (lane 0 alone for an empty piece), each 32 bytes of values, a dword of plane D and a halfword of plane H behind it."""
    nl = max((n + 3) // 4, 1)
    g = (n + 3) // 4
    return max(32 * nl, 8 * n + 4 * nl, 8 * n + 4 * g + 2 * nl)


def device_bytes(ns, strided):
    """What the operand's pack12 entry holds on the device (smm_csr_device_bytes' share)."""
    cells = int(np.size(ns))
    if strided:
        return 8 * (stride_of(ns) * cells + SLACK) + 2 * cells
    return 8 * (compact_units(ns) + 4) + 8 * cells
