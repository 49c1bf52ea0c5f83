"""wg_hs_rl_reserve / _config_set / _compact / _dump / _load / _count and wg_hs_ratelimit on the MI355X against
tests/hs_ratelimit_model.py (pytest -m gpu). Every comparison is exact: rl_status, out_records, rl_summary and the
sorted dump after each call; every output array carries guard bytes or words behind what the call may write."""
import ctypes

import numpy as np
import pytest

import hs_cookie_model as CM
import hs_model as HM
import hs_ratelimit_model as RL
import x25519_model as XM
from wgtest import splitmix_bytes, wg

pytestmark = pytest.mark.gpu

GUARD = 0x7E7E7E7E
LIST_LENGTHS = [0, 1, 63, 64, 65, 256, 257, 1000]  # a wave, one range of 256 positions, more than one range
STATIC = splitmix_bytes(0x8400, 32)
SECRET = splitmix_bytes(0x8401, 32)


@pytest.fixture(scope="module")
def rig():
    import torch
    assert torch.cuda.is_available()
    W = wg()
    yield type("Rig", (), dict(torch=torch, dev=torch.device("cuda", 0), W=W))


def limiter(rig, max_sources, cost, burst):
    """An engine with a limiter and its model."""
    eng = rig.W.Engine(0, key_slots=4)
    eng.hs_rl_reserve(max_sources)
    eng.hs_rl_config_set(cost, burst)
    model = RL.Limiter(max_sources, cost, burst)
    assert eng.hs_rl_count() == (0, model.C)
    return eng, model


def source(j: int):
    """Source j as (family, the key's bytes): even j IPv4, odd j IPv6; a few special ones below 8."""
    special = {0: (4, bytes(4)), 1: (6, bytes(8)),  # 0.0.0.0 and ::/64
               2: (4, bytes([10, 0, 0, 1])), 3: (6, bytes([10, 0, 0, 1, 1, 0, 0, 0])),  # (one address word on the device)
               4: (4, bytes([10, 0, 0, 2])), 5: (6, bytes([10, 0, 0, 2, 0, 0, 0, 0]))}  # equal leading bytes
    if j in special:
        return special[j]
    if j % 2 == 0:
        return 4, bytes([172, (j >> 16) & 0xFF, (j >> 8) & 0xFF, j & 0xFF])
    return 6, bytes([0x20, 0x01, 0x0D, 0xB8]) + j.to_bytes(4, "big")


def ring_of(rng, ids, extra_src=3):
    """Records (random bytes around their index) whose position k comes from source ids[k], and the batch's src array:
    the records' indices are a permutation, and every datagram has its own port, pad and ignored address bytes."""
    n = len(ids)
    n_src = n + extra_src
    perm = rng.permutation(n_src)[:n]
    src = np.frombuffer(rng.bytes(24 * n_src), RL.HS_SRC).copy()
    src["family"] = 4
    for k, j in enumerate(ids):
        fam, key = source(j)
        src[perm[k]]["family"] = fam
        src[perm[k]]["addr"][:len(key)] = np.frombuffer(key, np.uint8)
    recs = np.frombuffer(rng.bytes(160 * n), HM.HS_RECORD).copy()
    recs["index"] = perm
    return recs, src


def run(rig, eng, recs, src, now, n_records=None, compact=False):
    """One wg_hs_ratelimit over guarded outputs: (status list, out_records, summary dict)."""
    torch, dev = rig.torch, rig.dev
    n = len(recs)
    d_rec = torch.from_numpy(recs.view(np.uint8).reshape(n, 160).copy()).to(dev)
    d_src = torch.from_numpy(src.view(np.uint8).reshape(len(src), 24).copy()).to(dev)
    d_now = torch.from_numpy(np.array([now], np.uint64).view(np.int64)).to(dev)
    d_hs = None if n_records is None else torch.from_numpy(np.array([n_records, GUARD, GUARD, GUARD], np.uint32).view(np.int32)).to(dev)
    d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
    d_out = torch.full((n + 1, 160), 0x7E, dtype=torch.uint8, device=dev)
    d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
    eng.hs_ratelimit(d_rec, d_hs, d_src, d_now, d_st[:n], d_out[:n], d_sum[:4], compact=compact)
    torch.cuda.synchronize()
    return read(d_st, d_out, d_sum, n, n if n_records is None else min(n, n_records))


def read(d_st, d_out, d_sum, n, nl):
    st, out, sm = d_st.cpu().numpy().view(np.uint32), d_out.cpu().numpy(), d_sum.cpu().numpy().view(np.uint32)
    assert (sm[4:] == GUARD).all(), "summary guard overwritten"
    s = dict(n_passed=int(sm[0]), n_limited=int(sm[1]), n_full=int(sm[2]), n_badsrc=int(sm[3]))
    assert (st[nl:] == GUARD).all(), "rl_status written past the records"
    assert s["n_passed"] <= nl and (out[s["n_passed"]:] == 0x7E).all(), "out_records written past n_passed"
    return st[:nl].tolist(), np.ascontiguousarray(out[:s["n_passed"]]).view(HM.HS_RECORD).reshape(-1), s


def same_table(eng, model):
    got = RL.sorted_dump(eng.hs_rl_dump())
    want = model.dump()
    assert len(got) == len(want), (len(got), len(want))
    assert got.tobytes() == want.tobytes(), [(a, b) for a, b in zip(got, want) if a != b][:3]
    assert eng.hs_rl_count() == (len(want), model.C)


def step(rig, eng, model, recs, src, now, n_records=None, compact=False):
    """One call on the device and in the model, compared; returns the model's (status, passed, summary)."""
    got = run(rig, eng, recs, src, now, n_records, compact)
    want = model.ratelimit(recs["index"], src, now, n_records, compact)
    assert got[0] == want[0], [(k, a, b) for k, (a, b) in enumerate(zip(got[0], want[0])) if a != b][:8]
    assert got[2] == want[2]
    assert got[1].tobytes() == recs[want[1]].tobytes(), "out_records"
    same_table(eng, model)
    return want


def mix(kind, n, burst):
    """The source id of each of n positions."""
    if kind == "one":
        return [9] * n
    if kind == "distinct":
        return [100 + k for k in range(n)]
    if kind == "three":  # each one's first `burst` positions straddle position 64, position 256, and the front
        x0, y0 = (57 if n > 66 else 0), (247 if n >= 257 else 0)
        ids = []
        for k in range(n):
            r = k % 3
            ids.append(11 if r == 0 and k >= x0 else 12 if r == 1 and k >= y0 else 13 if r == 2 else 1000 + k)
        return ids
    assert kind == "tail"  # a contended source in the last wave only, another at the front, distinct ones between
    t0 = max(0, n - 40)
    return [15 if k >= t0 else 16 if k % 2 == 0 and k < 90 else 2000 + k for k in range(n)]


# ---- source mixes at every length -----------------------------------------------------------------------------------
@pytest.mark.parametrize("burst", [1, 5, 16])
@pytest.mark.parametrize("n", LIST_LENGTHS)
def test_source_mixes(rig, n, burst):
    """All one source, all distinct, three interleaved, a contended source in the last wave: a first call into an empty
    table (allowance = burst) and a second one `cost` ticks later (allowance 1 for the sources that spent theirs)."""
    cost = 50
    eng, model = limiter(rig, max(n, 1), cost, burst)
    try:
        for j, kind in enumerate(["one", "distinct", "three", "tail"]):
            rng = np.random.default_rng(8400 + 16 * n + 4 * burst + j)
            eng.hs_rl_load(np.zeros(0, RL.RL_ENTRY))
            model.load(np.zeros(0, RL.RL_ENTRY))
            ids = mix(kind, n, burst)
            recs, src = ring_of(rng, ids)
            st, passed, s = step(rig, eng, model, recs, src, 1000)
            if n:
                assert s["n_full"] == 0 and s["n_badsrc"] == 0
            if kind == "one":
                assert passed == list(range(min(n, burst)))
            if kind == "distinct":
                assert s["n_passed"] == n
            if kind == "three" and n >= 257 and burst > 1:
                p11 = [k for k in passed if ids[k] == 11]
                p12 = [k for k in passed if ids[k] == 12]
                assert len(p11) == burst and len(p12) == min(burst, ids.count(12)) and p11[0] < 64 <= p11[-1] and p12[0] < 256 <= p12[-1]
            if kind == "tail" and n > 64:
                assert [k for k in passed if ids[k] == 15] == list(range(n - 40, n - 40 + burst))
            st2, passed2, s2 = step(rig, eng, model, recs, src, 1000 + cost)
            if kind == "one" and n > burst:
                assert passed2 == [0]
    finally:
        eng.close()


def test_dispatch_order_independence(rig):
    """The same records with the ring reversed: in both rings the contended sources' passing positions are their lowest."""
    rng = np.random.default_rng(8500)
    n = 1000
    ids = [21 if k % 7 == 3 else 22 if k % 11 == 5 and k > 500 else 3000 + k for k in range(n)]
    recs, src = ring_of(rng, ids)
    for order in (slice(None), slice(None, None, -1)):
        eng, model = limiter(rig, n, 3, 5)
        try:
            r, i = np.ascontiguousarray(recs[order]), ids[order]
            st, passed, s = step(rig, eng, model, r, src, 77)
            for j in (21, 22):
                pos = [k for k in range(n) if i[k] == j]
                assert [k for k in passed if i[k] == j] == pos[:5] and len(pos) > 30
        finally:
            eng.close()


def test_sequence_of_calls_over_one_table(rig):
    """Eight calls: now stands still, advances by cost - 1, cost, max - 1 and max, steps back, and is 0. The special
    sources are among them: 0.0.0.0, ::/64, and IPv4 / IPv6 keys with equal leading bytes and with equal address words."""
    cost, burst = 50, 5
    mx = cost * burst
    eng, model = limiter(rig, 300, cost, burst)
    try:
        rng = np.random.default_rng(8600)
        now = 10_000
        for call, d in enumerate([0, 0, cost - 1, cost, mx - 1, mx, -3 * cost, None]):
            now = 0 if d is None else now + d
            n = 257
            ids = [int(rng.integers(0, 8)) if rng.random() < 0.6 else int(rng.integers(8, 120)) for _ in range(n)]
            recs, src = ring_of(rng, ids)
            before = model.dump().tobytes()
            st, passed, s = step(rig, eng, model, recs, src, now)
            if call == 0:
                assert s["n_limited"] > 50 and {(4, bytes(4)), (6, bytes(8))} <= set(model.entries) and len(model.entries) > 40
            if d is None:
                assert s["n_passed"] == n and model.dump().tobytes() == before
    finally:
        eng.close()


@pytest.mark.parametrize("cost,burst", [((1 << 31) + 3, 5), (1 << 56, 16), (1, 1)])
def test_counters_around_2_32_and_2_63(rig, cost, burst):
    """tokens and last around 2^32 and 2^63 (and a sum that would wrap), loaded, judged and dumped."""
    mx = cost * burst
    eng, model = limiter(rig, 32, cost, burst)
    try:
        lasts = [(1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, 1, (1 << 32) + cost]
        tokens = [0, cost - 1, cost, mx, min(mx, (1 << 32) - 1), min(mx, 1 << 32), (1 << 64) - 1, mx - 1]
        ent = np.zeros(len(lasts), RL.RL_ENTRY)
        for j, (t, l) in enumerate(zip(tokens, lasts)):
            fam, key = source(40 + j)
            ent[j]["addr"][:len(key)] = np.frombuffer(key, np.uint8)
            ent[j]["family"], ent[j]["tokens"], ent[j]["last"] = fam, t, l
        rng = np.random.default_rng(8700)
        ids = [40 + int(rng.integers(0, len(lasts))) for _ in range(130)]
        for now in [(1 << 32) + 5, (1 << 63) - 1, (1 << 63) + cost, (1 << 64) - 1]:
            eng.hs_rl_load(ent)
            model.load(ent)
            same_table(eng, model)
            recs, src = ring_of(rng, ids)
            step(rig, eng, model, recs, src, now)
            step(rig, eng, model, recs, src, now)
    finally:
        eng.close()


def test_badsrc(rig):
    """An index at and past n_src, families 0, 5 and 255; and a batch without any src entry."""
    eng, model = limiter(rig, 64, 10, 2)
    try:
        rng = np.random.default_rng(8800)
        recs, src = ring_of(rng, [30 + k % 9 for k in range(70)])
        n_src = len(src)
        for k, fam in [(3, 0), (10, 5), (64, 255), (69, 7)]:
            src[recs[k]["index"]]["family"] = fam
        recs["index"][5], recs["index"][63], recs["index"][65] = n_src, 0xFFFFFFFF, n_src + 1
        st, passed, s = step(rig, eng, model, recs, src, 500)
        assert s["n_badsrc"] == 7 and [st[k] for k in (3, 5, 10, 63, 64, 65, 69)] == [RL.RL_BADSRC] * 7
        st, passed, s = step(rig, eng, model, recs, src, 0)  # tick 0 passes only the valid sources
        assert s == dict(n_passed=63, n_limited=0, n_full=0, n_badsrc=7)
        st, passed, s = step(rig, eng, model, recs[:9], src[:0], 600)
        assert st == [RL.RL_BADSRC] * 9
    finally:
        eng.close()


# ---- the records of wg_hs_check and of wg_hs_admit, the count on the device -----------------------------------------
def _handshake_ring(rng, n, pub, sources, secret=None, bad_every=4):
    """n initiations from the given source ids in turn (every bad_every-th with a broken mac1), their table and src."""
    buf, off, lens = bytearray(), [], []
    src = np.frombuffer(rng.bytes(24 * n), RL.HS_SRC).copy()
    for i in range(n):
        fam, key = source(sources[i % len(sources)])
        src[i]["family"] = fam
        src[i]["addr"][:len(key)] = np.frombuffer(key, np.uint8)
        m = HM.message(1, rng.bytes(120), pub)
        if secret is not None:
            m = CM.with_mac2(m, CM.cookie_of_src(secret, src[i]))
        if bad_every and i % bad_every == 1:
            m = m[:120] + bytes([m[120] ^ 1]) + m[121:]
        off.append(len(buf))
        lens.append(148)
        buf += m
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64), np.array(lens, np.uint32), src


@pytest.mark.parametrize("admit", [False, True], ids=["check", "admit"])
def test_records_of_check_and_admit_with_the_count_on_the_device(rig, admit):
    """wg_hs_check / wg_hs_admit, then wg_hs_ratelimit on their records and &summary.n_valid, back to back on one stream:
    n_valid < n, and nothing behind it is read as a record or written."""
    torch, dev = rig.torch, rig.dev
    eng, model = limiter(rig, 300, 50, 5)  # (a call's unknown RECORDS must fit, not its sources)
    try:
        rng = np.random.default_rng(8900 + admit)
        pub = eng.hs_static_set(STATIC)
        eng.hs_cookie_secret_set(SECRET)
        n = 300
        ring, off, lens, src = _handshake_ring(rng, n, pub, [30, 31, 32, 33, 30, 30, 31], secret=SECRET if admit else None)
        d_ring = torch.from_numpy(ring).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_src = torch.from_numpy(src.view(np.uint8).reshape(n, 24).copy()).to(dev)
        d_hst = torch.zeros(n, dtype=torch.int32, device=dev)
        d_rec = torch.full((n, 160), 0x7E, dtype=torch.uint8, device=dev)
        d_hsum = torch.zeros(4, dtype=torch.int32, device=dev)
        d_now = torch.from_numpy(np.array([4242], np.int64)).to(dev)
        d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
        d_out = torch.full((n + 1, 160), 0x7E, dtype=torch.uint8, device=dev)
        d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
        if admit:
            d_non = torch.from_numpy(np.frombuffer(rng.bytes(24 * n), np.uint8).reshape(n, 24).copy()).to(dev)
            d_rep = torch.zeros((n, 80), dtype=torch.uint8, device=dev)
            d_asum = torch.zeros(4, dtype=torch.int32, device=dev)
            eng.hs_admit(d_ring, d_off, d_len, d_src, d_non, d_hst, d_rec, d_hsum, d_rep, d_asum)
        else:
            eng.hs_check(d_ring, d_off, d_len, d_hst, d_rec, d_hsum)
        eng.hs_ratelimit(d_rec, d_hsum, d_src, d_now, d_st[:n], d_out[:n], d_sum[:4])
        torch.cuda.synchronize()
        want_rec = HM.check(ring, off, lens, pub)[1] if not admit else CM.admit(ring, off, lens, src, bytes(24 * n), pub, SECRET)[1]
        nv = int(d_hsum.cpu().numpy()[0])
        assert nv == len(want_rec) == n - 75
        got = read(d_st, d_out, d_sum, n, nv)
        st, passed, s = model.ratelimit(want_rec["index"], src, 4242, n_records=nv)
        assert got[0] == st and got[2] == s and got[1].tobytes() == want_rec[passed].tobytes()
        assert s["n_passed"] == 20 and s["n_limited"] == nv - 20
        same_table(eng, model)
    finally:
        eng.close()


def test_n_records_smaller_than_n(rig):
    """A device count below n, above n, and 0: positions behind it are neither judged nor counted."""
    eng, model = limiter(rig, 300, 7, 3)
    try:
        rng = np.random.default_rng(9000)
        recs, src = ring_of(rng, [50 + k % 40 for k in range(300)])
        for now, nr in [(100, 130), (100, 257), (107, 1000), (107, 0)]:
            st, passed, s = step(rig, eng, model, recs, src, now, n_records=nr)
            assert len(st) == min(nr, 300)
    finally:
        eng.close()


# ---- a full table ------------------------------------------------------------------------------------------------------
def test_full_rule_on_the_smallest_table(rig):
    """C = 8: U + m == 4 fits, 5 does not; m counts records, not sources; known sources are served, and after a refused
    call only their buckets changed. Then COMPACT: only when the call might not fit, and exactly the stale entries."""
    eng, model = limiter(rig, 4, 10, 2)
    try:
        rng = np.random.default_rng(9100)
        assert model.C == 8
        st, _, _ = step(rig, eng, model, *ring_of(rng, [60, 61, 60]), 100)
        st, _, s = step(rig, eng, model, *ring_of(rng, [62, 63]), 100)
        assert s["n_passed"] == 2 and len(model.entries) == 4
        keep = model.dump()[:3]
        eng.hs_rl_load(keep)
        model.load(keep)
        before = {k: list(v) for k, v in model.entries.items()}
        known = next(j for j in (60, 61, 62, 63) if source(j) in before and before[source(j)][0] >= 10)
        st, _, s = step(rig, eng, model, *ring_of(rng, [64, known, 64, known, known]), 100)
        assert st[0] == st[2] == RL.RL_FULL and st[1] == RL.RL_OK and s["n_full"] == 2 and len(model.entries) == 3
        assert [k for k, v in model.entries.items() if v != before[k]] == [source(known)]
        st, _, s = step(rig, eng, model, *ring_of(rng, [64]), 120, compact=True)  # 3 + 1 fits: nothing is dropped
        assert st == [RL.RL_OK] and len(model.entries) == 4
        st, _, s = step(rig, eng, model, *ring_of(rng, [65, 66]), 125)  # without the flag: FULL
        assert st == [RL.RL_FULL] * 2 and len(model.entries) == 4
        st, _, s = step(rig, eng, model, *ring_of(rng, [65, 66]), 125, compact=True)  # the three of tick 100 go
        assert st == [RL.RL_OK] * 2 and set(model.entries) == {source(64), source(65), source(66)}
        st, _, s = step(rig, eng, model, *ring_of(rng, [67, 68, 69]), 0, compact=True)  # tick 0: no table at all
        assert st == [RL.RL_OK] * 3 and len(model.entries) == 3
    finally:
        eng.close()


@pytest.mark.parametrize("m,fits", [(8, True), (9, False)])
def test_full_boundary_at_capacity_4096(rig, m, fits):
    eng, model = limiter(rig, 2048, 10, 2)
    try:
        assert model.C == 4096
        rng = np.random.default_rng(9200)
        ent = np.zeros(2040, RL.RL_ENTRY)
        for j in range(2040):
            fam, key = source(5000 + j)
            ent[j]["addr"][:len(key)] = np.frombuffer(key, np.uint8)
            ent[j]["family"], ent[j]["tokens"], ent[j]["last"] = fam, 15, 90
        eng.hs_rl_load(ent)
        model.load(ent)
        same_table(eng, model)
        ids = [9000 + k for k in range(m)] + [5000 + k for k in range(300)]
        recs, src = ring_of(rng, [ids[k] for k in rng.permutation(len(ids))])
        st, passed, s = step(rig, eng, model, recs, src, 95)
        assert (s["n_full"], s["n_passed"]) == ((0, 300 + m) if fits else (m, 300))
        assert len(model.entries) == (2040 + m if fits else 2040)
    finally:
        eng.close()


# ---- compaction, dump and load -----------------------------------------------------------------------------------------
def test_compact_alone_and_round_trip_into_a_second_context(rig):
    torch, dev = rig.torch, rig.dev
    cost, burst = 10, 3
    eng, model = limiter(rig, 512, cost, burst)
    eng2, _ = limiter(rig, 700, cost, burst)  # (another capacity: the entries hash elsewhere)
    try:
        rng = np.random.default_rng(9300)
        for call, now in enumerate([100, 110, 125]):
            ids = [int(rng.integers(0, 6)) if rng.random() < 0.3 else 7000 + int(rng.integers(150 * call, 150 * call + 200)) for _ in range(257)]
            step(rig, eng, model, *ring_of(rng, ids), now)
        for now, any_dropped in [(50, False), (129, False), (131, True), (141, True)]:  # (a clock that stepped back keeps all)
            d_now = torch.from_numpy(np.array([now], np.int64)).to(dev)
            d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
            eng.hs_rl_compact(d_now, d_sum[:4])
            torch.cuda.synchronize()
            kept, dropped = model.compact(now)
            assert d_sum.cpu().numpy().view(np.uint32).tolist() == [kept, dropped, 0, 0] + [GUARD] * 4
            assert (dropped > 0) == any_dropped and kept > 0
            same_table(eng, model)
        eng.hs_rl_compact(torch.from_numpy(np.array([150], np.int64)).to(dev))  # no summary
        assert model.compact(150)[1] == 0 and len(model.entries) > 20
        same_table(eng, model)
        dump = eng.hs_rl_dump()
        eng2.hs_rl_load(dump)
        assert RL.sorted_dump(eng2.hs_rl_dump()).tobytes() == model.dump().tobytes() and eng2.hs_rl_count() == (len(dump), 2048)
        recs, src = ring_of(rng, [int(rng.integers(0, 6)) if rng.random() < 0.5 else 7300 + int(rng.integers(0, 200)) for _ in range(257)])
        a, b = run(rig, eng, recs, src, 215), run(rig, eng2, recs, src, 215)
        assert a[0] == b[0] and a[2] == b[2] and a[1].tobytes() == b[1].tobytes()
        assert RL.sorted_dump(eng.hs_rl_dump()).tobytes() == RL.sorted_dump(eng2.hs_rl_dump()).tobytes()
        # a load that the table refuses changes nothing
        W = rig.W
        bad = dump[:2].copy()
        bad[1] = bad[0]
        for entries, code in [(bad, W._lib.WG_EINVAL), (np.zeros(1, RL.RL_ENTRY), W._lib.WG_EINVAL)]:
            with pytest.raises(W.WgError) as e:
                eng2.hs_rl_load(entries)
            assert e.value.code == code
        assert RL.sorted_dump(eng.hs_rl_dump()).tobytes() == RL.sorted_dump(eng2.hs_rl_dump()).tobytes()
        eng2.hs_rl_reserve(3000)  # a larger reserve keeps the entries
        assert eng2.hs_rl_count()[1] == 8192
        assert RL.sorted_dump(eng.hs_rl_dump()).tobytes() == RL.sorted_dump(eng2.hs_rl_dump()).tobytes()
    finally:
        eng.close()
        eng2.close()


# ---- capture -----------------------------------------------------------------------------------------------------------
def test_captured_admit_ratelimit_dh_replay(rig):
    """hs_admit -> hs_ratelimit -> hs_dh captured once on one stream and replayed three times with `now` and the nonces
    refreshed: three model steps, and dh_status and shared are written for exactly n_passed records."""
    torch, dev = rig.torch, rig.dev
    cost, burst = 50, 5
    eng, model = limiter(rig, 256, cost, burst)
    try:
        rng = np.random.default_rng(9400)
        pub = eng.hs_static_set(STATIC)
        eng.hs_cookie_secret_set(SECRET)
        n = 140
        ring, off, lens, src = _handshake_ring(rng, n, pub, [30, 31, 33, 30, 35], secret=SECRET, bad_every=7)
        eng.hs_reserve(n)
        d_ring = torch.from_numpy(ring).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
        d_src = torch.from_numpy(src.view(np.uint8).reshape(n, 24).copy()).to(dev)
        d_non = torch.zeros((n, 24), dtype=torch.uint8, device=dev)
        d_hst = torch.zeros(n, dtype=torch.int32, device=dev)
        d_rec = torch.zeros((n, 160), dtype=torch.uint8, device=dev)
        d_hsum = torch.zeros(4, dtype=torch.int32, device=dev)
        d_rep = torch.zeros((n, 80), dtype=torch.uint8, device=dev)
        d_asum = torch.zeros(4, dtype=torch.int32, device=dev)
        d_now = torch.zeros(1, dtype=torch.int64, device=dev)
        d_st = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)
        d_out = torch.full((n + 1, 160), 0x7E, dtype=torch.uint8, device=dev)
        d_sum = torch.full((8,), GUARD, dtype=torch.int32, device=dev)
        d_sh = torch.full((n + 1, 32), 0x5C, dtype=torch.uint8, device=dev)
        d_dh = torch.full((n + 4,), GUARD, dtype=torch.int32, device=dev)

        def chain():
            eng.hs_admit(d_ring, d_off, d_len, d_src, d_non, d_hst, d_rec, d_hsum, d_rep, d_asum)
            eng.hs_ratelimit(d_rec, d_hsum, d_src, d_now, d_st[:n], d_out[:n], d_sum[:4])
            eng.hs_dh(d_out[:n], d_sum[:4], d_sh[:n], d_dh[:n])

        want_rec = CM.admit(ring, off, lens, src, bytes(24 * n), pub, SECRET)[1]
        assert len(want_rec) == n - 20
        big = torch.zeros((5000, 160), dtype=torch.uint8, device=dev)
        big_st = torch.zeros(5000, dtype=torch.int32, device=dev)
        big_out = torch.zeros((5000, 160), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            with pytest.raises(rig.W.WgError) as e:  # more records than the scratch holds: a capture cannot allocate
                eng.hs_ratelimit(big, None, d_src, d_now, big_st, big_out, d_sum[:4])
            chain()
        assert e.value.code == rig.W._lib.WG_EINVAL and "wg_hs_reserve" in str(e.value)
        passed_counts = []
        for now in (9000, 9000 + cost, 9000 + cost + burst * cost):
            d_now.fill_(now)
            d_non.copy_(torch.from_numpy(np.frombuffer(rng.bytes(24 * n), np.uint8).reshape(n, 24).copy()))
            for t in (d_st, d_sum, d_dh):
                t.fill_(GUARD)
            d_out.fill_(0x7E)
            d_sh.fill_(0x5C)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = read(d_st, d_out, d_sum, n, len(want_rec))
            st, passed, s = model.ratelimit(want_rec["index"], src, now)
            assert got[0] == st and got[2] == s and got[1].tobytes() == want_rec[passed].tobytes()
            same_table(eng, model)
            npass = s["n_passed"]
            dh, sh = d_dh.cpu().numpy().view(np.uint32), d_sh.cpu().numpy()
            assert (dh[:npass] == XM.X_OK).all() and (dh[npass:] == GUARD).all(), "dh_status: exactly n_passed records"
            assert (sh[npass:] == 0x5C).all() and not (sh[:npass] == 0x5C).all(axis=1).any()
            k = passed[-1]
            assert sh[npass - 1].tobytes() == XM.x25519(STATIC, want_rec[k]["msg"][8:40].tobytes())
            passed_counts.append(npass)
        assert passed_counts == [4 * burst, 4, 4 * burst]
    finally:
        eng.close()


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors(rig):
    torch, dev, W = rig.torch, rig.dev, rig.W
    E = W._lib
    eng = W.Engine(0, key_slots=4)
    try:
        n = 16
        rng = np.random.default_rng(9500)
        recs, src = ring_of(rng, list(range(10, 10 + n)))
        d_rec = torch.from_numpy(recs.view(np.uint8).reshape(n, 160).copy()).to(dev)
        d_src = torch.from_numpy(src.view(np.uint8).reshape(len(src), 24).copy()).to(dev)
        d_now = torch.full((2,), 5, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n + 4, dtype=torch.int32, device=dev)
        d_out = torch.zeros((n + 1, 160), dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(8, dtype=torch.int32, device=dev)

        def call(**kw):
            a = dict(records=d_rec, hs_summary=None, src=d_src, now=d_now[:1], rl_status=d_st[:n], out_records=d_out[:n],
                     rl_summary=d_sum[:4])
            a.update(kw)
            eng.hs_ratelimit(a["records"], a["hs_summary"], a["src"], a["now"], a["rl_status"], a["out_records"], a["rl_summary"])

        def refused(code, **kw):
            with pytest.raises(W.WgError) as e:
                call(**kw)
            assert e.value.code == code, str(e.value)

        refused(E.WG_ENOKEY)  # no reserve
        for f in (lambda: eng.hs_rl_config_set(10, 2), lambda: eng.hs_rl_dump(), lambda: eng.hs_rl_count(),
                  lambda: eng.hs_rl_compact(d_now[:1])):
            with pytest.raises(W.WgError) as e:
                f()
            assert e.value.code == E.WG_ENOKEY
        eng.hs_rl_reserve(16)
        refused(E.WG_ENOKEY)  # no config
        with pytest.raises(W.WgError) as e:
            eng.hs_rl_compact(d_now[:1])
        assert e.value.code == E.WG_ENOKEY
        for cost, burst in [(0, 1), ((1 << 56) + 1, 1), (1, 0), (1, 17)]:
            with pytest.raises(W.WgError) as e:
                eng.hs_rl_config_set(cost, burst)
            assert e.value.code == E.WG_EINVAL
        eng.hs_rl_config_set(1 << 56, 16)
        eng.hs_rl_config_set(10, 2)
        call()
        torch.cuda.synchronize()
        assert d_sum.cpu().numpy()[:4].tolist() == [n, 0, 0, 0]
        # misalignment
        flat = torch.zeros(160 * (n + 1), dtype=torch.uint8, device=dev)
        refused(E.WG_EINVAL, records=flat[8:8 + 160 * n].view(n, 160))
        refused(E.WG_EINVAL, out_records=flat[8:8 + 160 * n].view(n, 160))
        refused(E.WG_EINVAL, now=d_sum[1:3])  # (only its address is taken)
        refused(E.WG_EINVAL, rl_summary=d_sum[1:5])
        refused(E.WG_EINVAL, src=d_src.view(-1)[4:4 + 24 * n].view(n, 24))
        # overlap of an output with another output or an input
        refused(E.WG_EINVAL, out_records=d_rec)
        refused(E.WG_EINVAL, rl_status=d_out.view(torch.int32).view(-1)[:n])
        refused(E.WG_EINVAL, rl_summary=d_st[:4])
        refused(E.WG_EINVAL, rl_status=d_src.view(torch.int32).view(-1)[:n])
        refused(E.WG_EINVAL, rl_summary=d_now.view(torch.int32)[:4])
        # unknown flags, too many records (refused before anything is read)
        b = E.WgHsRlBatch(d_rec.data_ptr(), None, d_src.data_ptr(), d_now.data_ptr(), d_st.data_ptr(), d_out.data_ptr(),
                          d_sum.data_ptr(), n, n, 2, 0)
        assert E.lib().wg_hs_ratelimit(eng.ctx, ctypes.byref(b), None) == E.WG_EINVAL
        b.flags, b.n = 0, (1 << 30) + 1
        assert E.lib().wg_hs_ratelimit(eng.ctx, ctypes.byref(b), None) == E.WG_E2BIG
        # n = 0 writes only the summary
        d_sum.fill_(GUARD)
        eng.hs_ratelimit(d_rec[:0], None, d_src, d_now[:1], d_st[:0], d_out[:0], d_sum[:4])
        torch.cuda.synchronize()
        assert d_sum.cpu().numpy().view(np.uint32).tolist() == [0, 0, 0, 0] + [GUARD] * 4
        with pytest.raises(W.WgError) as e:
            eng.hs_rl_reserve((1 << 27) + 1)
        assert e.value.code == E.WG_E2BIG
    finally:
        eng.close()
