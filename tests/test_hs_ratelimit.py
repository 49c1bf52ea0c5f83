"""The handshake rate limiter without a GPU: the batched closed form of tests/hs_ratelimit_model.py (what the kernels
follow) against the sequential per-record rule of noise.RateLimiter, the key function, stale == absent, the model's
FULL / COMPACT / BADSRC rules, WireGuard's constants and the declarations of the new calls."""
import os
import re

import numpy as np
import pytest

import hs_ratelimit_model as RL
from wgtest import ROOT, noise, wg

COSTS = [1, 3, 50, 1 << 56]
BURSTS = [1, 5, 16]


def _pool(rng, n_src):
    """Sources of both families; several share their key and differ only in what the key ignores."""
    out = []
    for j in range(n_src):
        fam = 4 if j % 3 else 6
        base = bytes([10, j & 0xFF, j >> 8, 1]) + bytes(4) if j % 5 else bytes(8)  # (0.0.0.0 and ::/64 among them)
        out.append((fam, base + rng.bytes(8), int(rng.integers(0, 65536))))
    return out


def _steps(cost, burst):
    mx = cost * burst
    return [0, 0, cost - 1, cost, mx - 1, mx, 1, -1, -cost, -(mx + 3), 1 << 63, 2 * mx + 1]


@pytest.mark.parametrize("burst", BURSTS)
@pytest.mark.parametrize("cost", COSTS)
def test_batched_model_equals_the_sequential_rule(cost, burst):
    """Seeded random traces of calls: the clock stands still, steps back, and jumps by cost - 1, cost, max - 1, max and
    2^63. Record by record the model's OK is the sequential allow(), and after every call the buckets are equal."""
    N = noise()
    for seed in range(6):
        rng = np.random.default_rng(8100 + 97 * seed + burst)
        pool = _pool(rng, 12)
        src = RL.src_array(pool)
        model = RL.Limiter(64, cost, burst)
        seq = N.RateLimiter(cost, burst)
        now = int(rng.integers(1, 1 << 40))
        steps = _steps(cost, burst)
        for call in range(40):
            step = steps[int(rng.integers(0, len(steps)))]
            now = min(max(now + step, 1), (1 << 64) - 1)
            n = int(rng.integers(0, 60))
            hot = int(rng.integers(0, len(pool)))
            idx = [hot if rng.random() < 0.5 else int(rng.integers(0, len(pool))) for _ in range(n)]
            st, passed, summary = model.ratelimit(idx, src, now)
            want = [seq.allow(pool[i], now) for i in idx]
            assert [s == RL.RL_OK for s in st] == want, (seed, call, now)
            assert set(st) <= {RL.RL_OK, RL.RL_LIMITED} and summary["n_passed"] == sum(want)
            assert {k: tuple(v) for k, v in model.entries.items()} == {k: tuple(v) for k, v in seq.entries.items()}
            assert all(0 <= t <= cost * burst for t, _ in model.entries.values())


def test_tick_zero_limits_nothing_and_keeps_nothing():
    N = noise()
    model, seq = RL.Limiter(8, 50, 1), N.RateLimiter(50, 1)
    src = RL.src_array([(4, bytes([1, 2, 3, 4]), 9)])
    st, passed, _ = model.ratelimit([0] * 7, src, 0)
    assert st == [RL.RL_OK] * 7 and passed == list(range(7)) and not model.entries
    assert all(seq.allow((4, bytes([1, 2, 3, 4])), 0) for _ in range(7)) and not seq.entries


def test_key_function():
    N = noise()
    a4 = bytes([192, 0, 2, 7])
    assert N.ratelimit_key(4, a4 + b"\xAA" * 12) == N.ratelimit_key(4, a4 + bytes(12)) == (4, a4)
    a6 = bytes(range(1, 17))
    assert N.ratelimit_key(6, a6) == N.ratelimit_key(6, a6[:8] + bytes(8)) == (6, a6[:8])
    assert N.ratelimit_key(6, a6) != N.ratelimit_key(6, a6[:7] + b"\xFF" + a6[8:])
    same = a4 + bytes(4)
    assert N.ratelimit_key(4, same + bytes(8)) != N.ratelimit_key(6, same + bytes(8))  # equal leading bytes
    for fam in (0, 5, 255):
        with pytest.raises(ValueError):
            N.ratelimit_key(fam, a6)
    # the model's key is the same function, and ignores the port and the pad bytes too
    s = RL.src_array([(4, a4 + b"\x55" * 12, 1), (4, a4, 2), (6, a6, 3), (6, a6[:8] + b"\x77" * 8, 4), (6, same, 5), (0, a6, 6)])
    s["_pad"][1] = 9
    assert [RL.key_of(x) for x in s] == [(4, a4), (4, a4), (6, a6[:8]), (6, a6[:8]), (6, same), None]
    assert RL.key_of(s[0]) == N.ratelimit_key(4, bytes(s[0]["addr"])) and RL.key_of(s[2]) == N.ratelimit_key(6, bytes(s[2]["addr"]))
    lim = N.RateLimiter(10, 1)
    assert lim.allow((4, a4 + b"\x01" * 12, 1000), 5) and not lim.allow((4, a4 + b"\x02" * 12, 2000), 5)
    assert lim.allow((6, same + bytes(8), 1000), 5)


@pytest.mark.parametrize("cost,burst", [(1, 1), (3, 5), (50, 16)])
def test_stale_is_absent_under_a_clock_that_does_not_step_back(cost, burst):
    """Dropping the entries with now - last >= max before every call changes no answer and no surviving bucket."""
    rng = np.random.default_rng(8200 + cost)
    pool = _pool(rng, 9)
    src = RL.src_array(pool)
    keep, drop = RL.Limiter(32, cost, burst), RL.Limiter(32, cost, burst)
    now, mx, dropped = 1, cost * burst, 0
    for call in range(200):
        now += int(rng.choice([0, 1, cost - 1, cost, mx - 1, mx, mx + 1, 3 * mx]))
        idx = [int(rng.integers(0, len(pool))) for _ in range(int(rng.integers(0, 12)))]
        dropped += drop.compact(now)[1]
        a, b = keep.ratelimit(idx, src, now), drop.ratelimit(idx, src, now)
        assert a == b
        assert all(keep.entries[k] == v for k, v in drop.entries.items())
        assert all(keep.stale(k, now) for k in keep.entries if k not in drop.entries)
    assert dropped > 10


def test_sequential_expire_is_the_models_compaction():
    N = noise()
    seq, model = N.RateLimiter(3, 5), RL.Limiter(32, 3, 5)
    src = RL.src_array([(4, bytes([10, 0, 0, j]), 7) for j in range(6)])
    for now, idx in [(10, [0, 1, 2]), (20, [2, 3]), (24, [4]), (26, [5])]:
        model.ratelimit(idx, src, now)
        assert all(seq.allow((4, bytes(src[i]["addr"])), now) for i in idx)
    assert (len(model.entries) - seq.expire(36), seq.expire(36)) == (model.compact(36)[0], 0)
    assert {k: tuple(v) for k, v in model.entries.items()} == {k: tuple(v) for k, v in seq.entries.items()}
    assert sorted(k[1][3] for k in seq.entries) == [4, 5]


def test_model_full_rule():
    """U + m == C / 2 fits, U + m == C / 2 + 1 does not; m counts records; known sources are served either way."""
    src = RL.src_array([(4, bytes([10, 0, 0, j]), 1) for j in range(8)] + [(0, bytes(4), 1)])
    lim = RL.Limiter(4, 10, 2)  # C = 8: 4 entries
    assert lim.C == 8
    st, _, s = lim.ratelimit([0, 1, 0, 8], src, 100)
    assert st == [RL.RL_OK, RL.RL_OK, RL.RL_OK, RL.RL_BADSRC] and len(lim.entries) == 2
    st, _, s = lim.ratelimit([2, 3], src, 100)  # 2 + 2 == 4
    assert st == [RL.RL_OK, RL.RL_OK] and len(lim.entries) == 4
    lim.entries.pop((4, bytes([10, 0, 0, 3])))
    before = {k: list(v) for k, v in lim.entries.items()}
    st, _, s = lim.ratelimit([4, 1, 4, 1, 1], src, 100)  # 3 + 2 records of one unknown source: 5 > 4
    assert st == [RL.RL_FULL, RL.RL_OK, RL.RL_FULL, RL.RL_LIMITED, RL.RL_LIMITED]
    assert s == dict(n_passed=1, n_limited=2, n_full=2, n_badsrc=0)
    one = (4, bytes([10, 0, 0, 1]))
    assert len(lim.entries) == 3 and lim.entries[one] == [0, 100] and before[one] == [10, 100]
    assert all(lim.entries[k] == v for k, v in before.items() if k != one)
    # COMPACT reclaims only when the call's records might not fit, and only the stale entries
    st, _, s = lim.ratelimit([4], src, 100 + 20, compact=True)  # 3 + 1 <= 4: nothing dropped
    assert st == [RL.RL_OK] and len(lim.entries) == 4
    st, _, s = lim.ratelimit([5, 6], src, 100 + 25, compact=True)  # the three of tick 100 are stale, source 4 is not
    assert st == [RL.RL_OK, RL.RL_OK] and sorted(k[1][3] for k in lim.entries) == [4, 5, 6]


def test_model_dump_and_load_round_trip():
    rng = np.random.default_rng(8300)
    pool = _pool(rng, 20)
    lim = RL.Limiter(64, 3, 5)
    lim.ratelimit(list(range(20)) * 2, RL.src_array(pool), 77)
    d = lim.dump()
    assert d.dtype == RL.RL_ENTRY and d.itemsize == 32 and len(d) == len(lim.entries)
    assert d.tobytes() == RL.sorted_dump(d[::-1]).tobytes()
    assert all((x["addr"][4:] == 0).all() for x in d if x["family"] == 4) and not d["_pad"].any()
    other = RL.Limiter(64, 3, 5)
    other.load(d)
    assert other.entries == lim.entries and other.dump().tobytes() == d.tobytes()


def test_wireguard_constants():
    W = wg()
    c = W.RateLimitConfig.wireguard(1000)
    assert (c.cost, c.burst) == (50, 5) and c.max == 250
    assert W.WG_HS_RL_ENTRY_DTYPE == RL.RL_ENTRY and W.WG_HS_SRC_DTYPE == RL.HS_SRC


def test_declarations_match_the_header():
    """Every call and constant of the header's section is bound with the same values; the structs have the C sizes."""
    import ctypes
    L = wg()._lib
    text = open(os.path.join(ROOT, "include", "wgaead.h")).read()
    names = set(re.findall(r"^int (wg_hs_rl_\w+|wg_hs_ratelimit)\(", text, re.M))
    assert names == {"wg_hs_rl_reserve", "wg_hs_rl_config_set", "wg_hs_ratelimit", "wg_hs_rl_compact", "wg_hs_rl_dump",
                     "wg_hs_rl_load", "wg_hs_rl_count"}
    assert names <= {s[0] for s in L.SIGNATURES}
    for name, value in re.findall(r"^#define (WG_HS_RL_\w+) (\d+)u", text, re.M):
        assert getattr(L, name) == int(value), name
    assert (RL.RL_OK, RL.RL_LIMITED, RL.RL_FULL, RL.RL_BADSRC) == (L.WG_HS_RL_OK, L.WG_HS_RL_LIMITED, L.WG_HS_RL_FULL, L.WG_HS_RL_BADSRC)
    assert RL.MAX_BURST == L.WG_HS_RL_MAX_BURST == noise().RateLimiter.MAX_BURST
    assert ctypes.sizeof(L.WgHsRlEntry) == 32 and ctypes.sizeof(L.WgHsRlSummary) == 16 and ctypes.sizeof(L.WgHsRlBatch) == 72
