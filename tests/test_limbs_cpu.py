"""The three exact-sum row sinks share one CPU path (limb_init / limb_fold / limb_merge in quadrs_hip.hip, _limb_* in engine.py;
DESIGN.md section 3.24): what holds of every cell size is asserted once here, over the three of them, without a referee."""
import numpy as np
import pytest

SINKS = ("mean", "power", "spread")
W, N, POOL = 5, 11, 4                                  # an odd width, rows of 4, 4 and 3 windows


def norms():
    """finite values over the whole exponent range, zeros, subnormals, a NaN and an infinity"""
    rng = np.random.default_rng(24)
    bits = rng.integers(0, 0x7f800000, size=(N, W), dtype=np.uint32)
    bits[0, 0], bits[1, 1], bits[2, 2], bits[3, 3], bits[9, 4] = 0, 1, 0x7f7fffff, 0x7fc00000, 0x7f800000
    return bits.view(np.float32)


@pytest.mark.parametrize("sink", SINKS)
def test_two_parts_merged_are_the_whole_word_for_word(engine, sink):
    init, fold, merge = (getattr(engine, f"{sink}_{step}") for step in ("init", "fold", "merge"))
    words = getattr(engine._ffi, f"{sink.upper()}_WORDS")
    a, R = norms(), -(-N // POOL)
    whole = fold(a, POOL)
    assert whole.shape == (R, W, words) and whole.dtype == np.uint64
    assert not init(W, R).any()
    for at in range(N + 1):                            # every cut, on and off a row boundary
        x = fold(a[:at], POOL, into=init(W, R))
        y = fold(a[at:], POOL, at=at, into=init(W, R))
        assert merge(x, y) is x and x.tobytes() == whole.tobytes(), at
    with pytest.raises(ValueError):
        merge(whole, init(W, R + 1))


def test_the_spread_cell_is_the_mean_cell_and_the_power_cell(engine):
    """words 0-8 the mean's limbs, 9-26 the power's, 27 the count word of both"""
    a = norms()
    m, p, s = engine.mean_fold(a, POOL), engine.power_fold(a, POOL), engine.spread_fold(a, POOL)
    assert np.array_equal(s[..., :9], m[..., :9]) and np.array_equal(s[..., 9:27], p[..., :18])
    assert np.array_equal(s[..., 27], m[..., 9]) and np.array_equal(s[..., 27], p[..., 18])
