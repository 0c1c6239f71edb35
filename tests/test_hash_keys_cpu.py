"""Conditions on the adversarial key sets of tests/test_gpu_hash_edges.py, checked on the CPU restatement of LdsHash
(tests/hash_keys.py): enough window keys, a probe sequence that wraps past the end of the table, one chain about as
long as the row.  These are conditions on the inputs, not measurements of the device."""
import numpy as np
import pytest

import hash_keys as hk


def test_constants_are_those_of_the_header():
    for c in hk.CLASSES.values():
        assert c.HS == 1 << c.BITS and c.MAX == c.HS // 2 and c.TPR * c.RPB == 256
    assert hk.WAVE_HASH.MAX < hk.WG_HASH.MAX
    assert 0 < hk.MULT < 1 << 32 and hk.MULT % 2 == 1


def test_start_is_the_multiplicative_hash_in_32_bits():
    keys = np.array([0, 1, 2, 12345, 599999, 2**31 - 1], dtype=np.int64)
    for bits in (9, 13):
        want = [((int(k) * hk.MULT) % 2**32) >> (32 - bits) for k in keys]
        assert hk.start(keys, bits).tolist() == want
        assert hk.start(keys, bits).max() < 1 << bits


def test_simulate_is_linear_probing_with_a_wrap():
    bits = 9
    k = hk.window_keys(bits, 50000, 1)[:3]                  # three keys of the last slot: 511, then 0 and 1
    slots, longest = hk.simulate(k, bits)
    assert slots.tolist() == [511, 0, 1] and longest == 2
    other = np.array([x for x in range(2000) if hk.start([x], bits)[0] == 0][:1])
    slots, longest = hk.simulate(np.concatenate([k, other]), bits)
    assert slots.tolist() == [511, 0, 1, 2] and longest == 2


@pytest.mark.parametrize("name", list(hk.KEYSETS))
def test_window_keys_wrap_and_chain(name):
    c, window, universe, keys = hk.keyset(name)
    assert np.all(np.diff(keys) > 0) and keys[0] >= 0 and keys[-1] < universe
    assert np.all(hk.start(keys, c.BITS) >= c.HS - window)
    assert len(keys) >= c.MAX + hk.SPARE, f"{name}: only {len(keys)} window keys in [0, {universe})"
    slots, longest = hk.simulate(keys[:c.MAX], c.BITS)
    assert len(set(slots.tolist())) == c.MAX
    wrapped = int((slots < c.HS - window).sum())
    print(f"{name}: {len(keys)} window keys, longest probe {longest}, {wrapped} slots occupied after the wrap")
    assert wrapped > 0, "inserting MAX window keys does not wrap"
    assert wrapped == c.MAX - window and slots.min() == 0 and slots.max() == c.HS - 1
    assert longest >= c.MAX - window
    # an absent window key walks the whole chain: from its start slot to the first empty slot
    table = np.zeros(c.HS, dtype=bool)
    table[slots] = True
    first_empty = int(np.flatnonzero(~table)[0])
    assert first_empty == c.MAX - window
    for s in hk.start(keys[c.MAX:c.MAX + hk.SPARE], c.BITS).tolist():
        assert (c.HS - s) + first_empty >= c.MAX - window + 1


@pytest.mark.parametrize("name", list(hk.KEYSETS))
def test_random_keys_are_what_they_claim(name):
    c, _, universe, keys = hk.keyset(name)
    rnd = hk.random_keys(name)
    assert len(rnd) == len(keys) and len(set(rnd.tolist())) == len(rnd) and rnd.min() >= 0 and rnd.max() < universe
    _, longest = hk.simulate(rnd[:c.MAX], c.BITS)
    assert longest < c.MAX // 4, "the random keys are the easy case: short chains"


def test_wave_rows_per_pass_reads_the_launches():
    one = hk.wave_rows_per_pass(1)
    assert one >= hk.WAVE_HASH.RPB and one % hk.WAVE_HASH.RPB == 0 and hk.wave_rows_per_pass(256) == 256 * one
