"""tests/philox_ref.py (the host restatement of the kernels' dropout draws) against what does not depend on the library: the
published Philox4x32-10 known-answer vectors, drop_threshold_host's values for an fp32 p, and -- for the fusion's 16-bit rule -- a
literal transcription of csrc/fusion.hip keep_scale20's window logic."""
import numpy as np
import pytest

import philox_ref as PR

# (counter words c0 c1 c2 c3, key words k0 k1, output): the Random123 known-answer vectors of Philox4x32-10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
BIG_SEED = 0x1D2C3B4A5F6E7081 & ((1 << 62) - 1)


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_known_answer_vectors(ctr, key, out):
    got = PR.philox4x32_10(ctr[0] | (ctr[1] << 32), key[0] | (key[1] << 32), c2=ctr[2], c3=ctr[3])
    assert got.shape == (1, 4) and got.dtype == np.uint32
    assert tuple(int(v) for v in got[0]) == out


def test_calls_are_independent_of_the_batch():
    """an array of counters gives each counter's own words (the vectorisation mixes nothing), 64-bit counters included"""
    ctrs = [0, 1, 2, 0xffffffff, 1 << 32, (1 << 40) + 5]
    both = PR.philox4x32_10(np.array(ctrs, dtype=np.uint64), BIG_SEED)
    for i, c in enumerate(ctrs):
        assert np.array_equal(both[i], PR.philox4x32_10(c, BIG_SEED)[0])
    assert len({tuple(r) for r in both.tolist()}) == len(ctrs)


@pytest.mark.parametrize("p,thr,thr16", [(0.1, 429496736, 6553), (0.3, 1288490240, 19660), (0.25, 1073741824, 16384),
                                         (0.999, 4290672384, 65470), (0.5, 1 << 31, 1 << 15), (0.0, 0, 0)])
def test_threshold_is_that_of_an_fp32_p(p, thr, thr16):
    assert PR.threshold(p) == thr and PR.threshold(p) >> 16 == thr16
    assert PR.threshold(np.float32(p)) == thr


def test_threshold_tells_fp32_p_from_double_p_and_caps():
    assert int(0.1 * 4294967296.0) == 429496729 != PR.threshold(0.1)
    assert PR.threshold(1.0) == 0xFFFFFFFF and PR.threshold(np.nextafter(np.float32(1.0), np.float32(0.0))) == 0xFFFFFF00


def test_inv_keep_is_fp32():
    assert PR.inv_keep(0.5) == np.float32(2.0) and PR.inv_keep(0.25).dtype == np.float32
    assert PR.inv_keep(0.1) == np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))
    assert float(PR.inv_keep(0.1)) != 1.0 / (1.0 - 0.1)


@pytest.mark.parametrize("fn,group", [(PR.keep32, 4), (PR.keep16, 8)])
def test_prefix_property_shapes_and_offsets(fn, group):
    full = fn(1000, BIG_SEED, 0.3)
    for n in (1, 3, 4, 5, 7, 8, 9, 255, 999):
        assert np.array_equal(fn(n, BIG_SEED, 0.3), full[:n])
    assert np.array_equal(fn((10, 5, 20), BIG_SEED, 0.3), full.reshape(10, 5, 20))
    first = 37 * group
    assert np.array_equal(fn(1000 - first, BIG_SEED, 0.3, first=first), full[first:])
    assert full.dtype == np.bool_


def test_keep32_is_word_e_mod_4_of_call_e_div_4():
    words = PR.philox4x32_10(np.arange(6, dtype=np.uint64), 77)
    thr = PR.threshold(0.3)
    m = PR.keep32(23, 77, 0.3)
    for e in range(23):
        assert bool(m[e]) == (int(words[e >> 2, e & 3]) >= thr)


def _keep_scale20(e0, seed, thr):
    """csrc/fusion.hip keep_scale20, Philox branch, line by line: three calls, twelve named words, `hi ? word(k + 2) : word(k)`"""
    assert e0 % 4 == 0
    g0 = e0 >> 3
    r = PR.philox4x32_10(np.array([g0, g0 + 1, g0 + 2], dtype=np.uint64), seed)
    word = [int(r[i // 4, i % 4]) for i in range(12)]
    hi = (e0 & 4) != 0
    t16 = thr >> 16
    sc = [False] * 20
    for k in range(10):
        x = word[k + 2] if hi else word[k]
        sc[2 * k] = (x & 0xFFFF) >= t16
        sc[2 * k + 1] = (x >> 16) >= t16
    return sc


@pytest.mark.parametrize("seed", [99, BIG_SEED])
def test_keep16_is_keep_scale20_in_both_window_phases(seed):
    """three rows of width 5020 = 4 (mod 8): the rows start in alternate phases; every 20-element window of every row"""
    W5, rows, p = 5020, 3, 0.25
    flat = PR.keep16((rows, W5), seed, p)
    thr = PR.threshold(p)
    phases = set()
    for row in range(rows):
        for t in range(W5 // 20):
            e0 = row * W5 + 20 * t
            phases.add(e0 & 4)
            assert _keep_scale20(e0, seed, thr) == flat[row, 20 * t:20 * t + 20].tolist(), (row, t)
    assert phases == {0, 4}


@pytest.mark.parametrize("fn,bits", [(PR.keep32, 32), (PR.keep16, 16)])
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_drop_rate_within_four_sigma(fn, bits, p):
    n = 1 << 20
    # the rate the rule aims at: P(draw < threshold) for a uniform `bits`-bit draw
    q = (PR.threshold(p) >> (32 - bits)) / float(1 << bits)
    drop = 1.0 - fn(n, 4242, p).mean()
    assert abs(drop - q) <= 4.0 * (q * (1 - q) / n) ** 0.5, (drop, q)
    assert abs(q - p) < 2e-5


@pytest.mark.parametrize("fn", [PR.keep32, PR.keep16])
def test_the_high_seed_word_takes_part(fn):
    for s in (0, 77, BIG_SEED):
        a, b = fn(4096, s, 0.5), fn(4096, s + (1 << 32), 0.5)
        assert not np.array_equal(a, b)
        assert 0.4 < (a != b).mean() < 0.6               # an unrelated mask, not a shifted or partly shared one
