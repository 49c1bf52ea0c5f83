"""The receive-side AllowedIPs verdict on the MI355X at its edges (pytest -m gpu): the filters and packets of
tests/rx_filter_edge_cases.py (a prefix at every length of both families, prefixes nested around every byte boundary
of a compiled node, packets at the 19/20 and 39/40-byte bounds with every version nibble) through every kernel that
holds rx_verdict: k_rx_filter (wg_rx_check), the fused verdict of wg_open_batch(..., WG_F_RX_FILTER) in the mixed
body under six slot plans, in the uniform-wave body, its fallback and the 8-lane slots it replaced, and after the
decrypt pass of an in-place open; then one engine whose filter image grows, moves, shrinks and is re-mapped.

Every expectation is oracle/rx.py's for the bytes the packet actually holds, and every comparison is exact: the
status list, the plaintext buffer as a whole (forged packets scrubbed, or untouched in place; the sentinel between
the packets intact) and the guard words behind the status array. tests/test_rx_filter_edges.py checks on the CPU that
the case set asks what it claims. The engines are this module's own: its 180 filters stay out of the session's."""
import ctypes
import functools
import os

import numpy as np
import pytest

import rx_filter_edge_cases as E
from oracle import rx
from wgtest import oracle, splitmix_np, wg

pytestmark = pytest.mark.gpu
O = oracle()
C = E.cases()
SENT = E.SENTINEL
GUARD = 0x5A5A5A5A
KEYS = splitmix_np(0xA110, 32 * E.KEY_SLOTS)
FILTER_OF_SLOT = {s: E.filter_of(C, f) for s, f in enumerate(C.slot_ids)}  # slots behind the map: no filter
LENGTHS = (48, 112, 576, 1500, 2048)  # beside the 20 / 40 B of a packet that ends with its destination


def _dev():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda", 0)


def _engine(env=None, install=True):
    """An engine created under `env` (the plan knobs are read at creation only), with the case set's filters and
    its slot map, set in two calls."""
    env = dict(env or {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = wg().Engine(0, key_slots=E.KEY_SLOTS)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    e.set_keys(0, KEYS.tobytes())
    if install:
        for fid in sorted(C.filters, key=lambda f: (f * 37) % 181):  # not in ascending order of id
            e.filter_set(fid, C.filters[fid])
        e.slot_filters_set(0, C.slot_ids[:C.split])
        e.slot_filters_set(C.split, C.slot_ids[C.split:])
    return e


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in made:
            made[key] = _engine(env)
        return made[key]
    yield get
    for e in made.values():
        e.close()


class Batch:
    """Packets (key slot, plaintext, what it is) laid out over a sentinel, sealed by the oracle, about 3 % of the
    tags forged. want: the oracle's verdict per packet for the bytes it holds."""

    def __init__(self, items, seed, unaligned=False, filter_of_slot=None):
        W = wg()
        fos = FILTER_OF_SLOT if filter_of_slot is None else filter_of_slot
        self.n = n = len(items)
        self.slots = np.array([s for s, _, _ in items], np.int64)
        self.pts = [pt for _, pt, _ in items]
        self.what = [w for _, _, w in items]
        self.lens = np.array([len(p) for p in self.pts], np.int64)
        self.max_len = int(self.lens.max())
        self.off, self.size = E.layout(self.lens, 16, unaligned)
        ctr = np.arange(n, dtype=np.uint64) * np.uint64(0x100000001) + np.uint64(seed)
        self.desc = W.pack_desc(self.off, self.off, ctr, self.lens, self.slots)
        self.plain = np.full(self.size, SENT, np.uint8)
        for i, p in enumerate(self.pts):
            self.plain[int(self.off[i]):int(self.off[i]) + len(p)] = np.frombuffer(p, np.uint8)
        self.want = [rx.process_decrypted(p, fos.get(int(s))) for s, p in zip(self.slots, self.pts)]
        self.forged = np.arange(n) % 31 == 7
        self._wire = None

    @property
    def wire(self):
        if self._wire is None:
            w = np.full(self.size, SENT, np.uint8)
            O.seal_batch(self.desc, self.plain, w, KEYS, threads=8)
            for i in np.nonzero(self.forged)[0]:
                w[int(self.off[i]) + int(self.lens[i]) + 15] ^= 0x80
            self._wire = w
        return self._wire

    def opened(self):
        """(statuses, output buffer) of an open into a buffer of its own."""
        st, out = list(self.want), self.plain.copy()
        for i in np.nonzero(self.forged)[0]:
            st[i] = rx.PKT_BADTAG
            out[int(self.off[i]):int(self.off[i]) + int(self.lens[i])] = 0
        return st, out

    def opened_in_place(self):
        """(statuses, buffer) of an open over the wire buffer itself: a forged packet keeps its ciphertext."""
        st, out = list(self.want), self.wire.copy()
        for i in range(self.n):
            o, L = int(self.off[i]), int(self.lens[i])
            if self.forged[i]:
                st[i] = rx.PKT_BADTAG
            else:
                out[o:o + L] = self.plain[o:o + L]
        return st, out

    # -- device side --------------------------------------------------------------------------------------------
    def t(self, a):
        torch, dev = _dev()
        return torch.from_numpy(a).to(dev)

    def d_desc(self):
        return self.t(wg().desc_as_int64(self.desc))

    def status(self, incoming=None):
        st = np.full(self.n + 4, GUARD, np.uint32).view(np.int32)
        st[:self.n] = 9 if incoming is None else incoming
        return self.t(st)

    def same_status(self, st, want, what):
        got = st.cpu().numpy().view(np.uint32).tolist()
        assert got[self.n:] == [GUARD] * 4, f"{what}: the words behind the status array were written"
        bad = [(i, got[i], want[i], self.what[i]) for i in range(self.n) if got[i] != want[i]]
        assert not bad, f"{what}: {len(bad)} statuses differ, (index, got, want, packet): {bad[:6]}"

    def same_bytes(self, got, want, what):
        if np.array_equal(got, want):
            return
        for i in range(self.n):  # name the first packet that differs
            o, L = int(self.off[i]), int(self.lens[i]) + 16
            assert np.array_equal(got[o:o + L], want[o:o + L]), f"{what}: {self.what[i]}"
        raise AssertionError(f"{what}: bytes that no packet owns were written")

    # -- the checks ---------------------------------------------------------------------------------------------
    def check_rx_check(self, engine, what="rx_check"):
        """wg_rx_check(WG_RX_FILTER) over the plaintexts: forged tags and a few other non-OK statuses come in and
        must go out unchanged; the plaintext buffer is only read."""
        torch, _ = _dev()
        incoming = np.zeros(self.n, np.int32)
        incoming[self.forged] = rx.PKT_BADTAG
        for k, code in enumerate((2, rx.PKT_KEEPALIVE, rx.PKT_BADIP, rx.PKT_FILTERED, rx.PKT_REPLAY)):
            incoming[13 + 97 * k:self.n:487] = code
        want = [w if c == 0 else int(c) for w, c in zip(self.want, incoming)]
        st, pt = self.status(incoming), self.t(self.plain)
        engine.rx_check(self.d_desc(), pt, st[:self.n], wg()._lib.WG_RX_FILTER)
        torch.cuda.synchronize()
        self.same_status(st, want, what)
        self.same_bytes(pt.cpu().numpy(), self.plain, what)

    def check_fused(self, engine, uniform=False, what="fused open", twice=True):
        """open(rx_filter=True) into a buffer of its own; with `twice`, a plain open and wg_rx_check after it must
        give the same statuses."""
        torch, _ = _dev()
        want_st, want_out = self.opened()
        d, wire = self.d_desc(), self.t(self.wire)
        st, out = self.status(), self.t(np.full(self.size, SENT, np.uint8))
        engine.open(d, wire, out, st[:self.n], self.max_len, uniform=uniform, rx_filter=True)
        torch.cuda.synchronize()
        self.same_status(st, want_st, what)
        self.same_bytes(out.cpu().numpy(), want_out, what)
        if twice:
            st2, out2 = self.status(), self.t(np.full(self.size, SENT, np.uint8))
            engine.open(d, wire, out2, st2[:self.n], self.max_len, uniform=uniform)
            engine.rx_check(d, out2, st2[:self.n], wg()._lib.WG_RX_FILTER)
            torch.cuda.synchronize()
            self.same_status(st2, want_st, what + ", open then rx_check")
            assert st2.cpu().numpy().tolist() == st.cpu().numpy().tolist()
            self.same_bytes(out2.cpu().numpy(), want_out, what + ", open then rx_check")

    def check_in_place(self, engine, uniform=False, what="in-place fused open"):
        """open(rx_filter=True) with the wire buffer as its output and in_off == out_off: every packet is verified
        first, and the verdict follows the decrypt pass."""
        torch, _ = _dev()
        want_st, want_buf = self.opened_in_place()
        st, buf = self.status(), self.t(self.wire.copy())
        engine.open(self.d_desc(), buf, buf, st[:self.n], self.max_len, uniform=uniform, rx_filter=True)
        torch.cuda.synchronize()
        self.same_status(st, want_st, what)
        self.same_bytes(buf.cpu().numpy(), want_buf, what)


def _label(p):
    return f"{C.names[p.fid]}, {p.kind}" + (f", to {E.ip(p.dst)}" if p.dst else "")


# ---- the case set as it stands: wg_rx_check ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_batch():
    items = [(C.slot_of[p.fid], p.pt, _label(p)) for p in C.probes]
    items.append((E.KEY_SLOTS - 1, C.probes[0].pt, "a key slot behind the slot map"))
    return Batch(items, seed=1, unaligned=True)


def test_rx_check_whole_case_set(engines):
    """k_rx_filter over every probe in one batch, the plaintexts at every offset mod 16. The statuses are those the
    case set was built with (oracle/rx.py), and the CPU tests hold them to the closed form."""
    b = plain_batch()
    assert b.want[:-1] == [p.status for p in C.probes] and b.want[-1] == rx.PKT_OK
    assert len(set((b.off % np.uint64(16)).tolist())) == 16
    b.check_rx_check(engines())


# ---- fused open, mixed plans --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Every destination probe at 20 / 40 B (the packet ends with its destination) and at one of 48 .. 2048 B in
    turn; the packet edges of (c) at their own lengths, and those with a version nibble also at 20 B and at one of
    48 .. 2048 B, so that every length holds bad-IP verdicts too."""
    rng = np.random.default_rng(E.SEED + 2)
    items, turn = [], 0
    for p in C.probes:
        slot, what = C.slot_of[p.fid], _label(p)
        if p.part == "c" or not p.dst:
            items.append((slot, p.pt, what))
            if "nibble" in p.kind:
                for L in (20, LENGTHS[turn % len(LENGTHS)]):
                    items.append((slot, E.resize(p.pt, L, rng), f"{what}, as {L} B"))
                turn += 1
            continue
        for L in (E.min_len(p.dst), LENGTHS[turn % len(LENGTHS)]):
            items.append((slot, E.resize(p.pt, L, rng), f"{what}, as {L} B"))
        turn += 1
    return Batch(items, seed=2, unaligned=True)


# the default plan of a small mixed batch (the long packets in 16-lane slots, the rest in 8), 16-lane slots, 4-lane
# slots, long packets in 16 and the rest in 4 lanes (the shortest in 2-lane slots), the same with the 2-lane part off,
# and WG_SLOT2=2 on the default plan: tests/test_gpu_poly_edges.py's plans
PLANS = [{}, {"WG_SLOT16": "1"}, {"WG_SLOT4": "1"}, {"WG_SLOT4": "2"}, {"WG_SLOT4": "2", "WG_SLOT2": "2"},
         {"WG_SLOT2": "2"}]


@pytest.mark.parametrize("plan", PLANS, ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()) or "default")
def test_fused_open_mixed_plans(engines, plan):
    """wg_open_batch(..., WG_F_RX_FILTER) without WG_F_UNIFORM over packets of 0 .. 2048 B at every offset mod 16:
    every length holds OK, FILTERED and BADIP verdicts, so every slot class of every plan writes all three."""
    b = mixed_batch()
    for L in (20, 40) + LENGTHS:
        kinds = {w for w, n in zip(b.want, b.lens) if n == L}
        assert {rx.PKT_OK, rx.PKT_FILTERED, rx.PKT_BADIP} <= kinds, (L, kinds)
    assert rx.PKT_KEEPALIVE in b.want and b.forged.sum() > 50
    b.check_fused(engines(**plan))


# ---- fused open, uniform ------------------------------------------------------------------------------------------------
UNIFORM_LENGTHS = (0, 1, 19, 20, 39, 40, 48, 300)
BODIES = ("uniform_waves", "fallback", "WG_UNI=0")


@functools.lru_cache(maxsize=None)
def uniform_batch(L, alternating):
    """Every probe cut or padded to L bytes (a destination that no longer fits makes the packet bad IP; L = 0 makes
    keepalives), each key slot's packets in runs of eight, so that every wave holds one length under one key: the
    condition of the uniform-wave body. alternating: the same packets dealt out slot after slot, so that no wave is
    under one key and every wave takes the fallback body."""
    rng = np.random.default_rng(E.SEED + 3 + L)
    runs = {}
    for p in C.probes:
        if len(p.pt) == 0:
            continue
        item = (C.slot_of[p.fid], E.resize(p.pt, L, rng), f"{_label(p)}, as {L} B")
        run = runs.setdefault(item[0], [])
        if all(item[1] != other[1] for other in run):
            run.append(item)
    for run in runs.values():
        run += [run[-1]] * (-len(run) % 8)
    if alternating:
        items = [run[k] for k in range(max(map(len, runs.values()))) for run in runs.values() if k < len(run)]
    else:
        items = [item for run in runs.values() for item in run]
    b = Batch(items, seed=3 + L, unaligned=False)
    waves = [set(b.slots[k:k + 8].tolist()) for k in range(0, b.n, 8)]
    assert b.n % 8 == 0 and all((len(w) > 1) if alternating else (len(w) == 1) for w in waves)
    return b


@pytest.mark.parametrize("body", BODIES)
@pytest.mark.parametrize("L", UNIFORM_LENGTHS)
def test_fused_open_uniform(engines, L, body):
    """WG_F_UNIFORM | WG_F_RX_FILTER at the lengths around the 20- and 40-byte bounds: open_result<8> of the
    uniform-wave body (every wave under one key), its fallback (the keys alternating inside every wave) and the
    8-lane slots of WG_UNI=0."""
    b = uniform_batch(L, body == "fallback")
    kinds = set(b.want)
    if L == 0:
        assert kinds == {rx.PKT_KEEPALIVE}
    elif L < 20:
        assert kinds == {rx.PKT_BADIP}
    else:
        assert {rx.PKT_OK, rx.PKT_FILTERED, rx.PKT_BADIP} <= kinds
    assert len(set(b.slots.tolist())) == len(C.slot_ids)
    b.check_fused(engines(WG_UNIFORM16="0", WG_UNI="0" if body == "WG_UNI=0" else "1"), uniform=True)


# ---- in-place fused open ------------------------------------------------------------------------------------------------
def test_fused_open_in_place_mixed(engines):
    """The mixed batch opened over its own wire buffer: the verify-first body, whose verdict is written after the
    decrypt pass; a forged packet keeps its ciphertext and is BADTAG."""
    mixed_batch().check_in_place(engines())


@pytest.mark.parametrize("L", [20, 40, 300])
def test_fused_open_in_place_uniform(engines, L):
    uniform_batch(L, False).check_in_place(engines(WG_UNIFORM16="0", WG_UNI="1"), uniform=True)


# ---- table lifecycle ----------------------------------------------------------------------------------------------------
def _lifecycle_dests():
    """Every destination that the case set asks of the filters used below, and the four base addresses."""
    out = []
    for p in C.probes:
        if p.dst and p.dst not in out and (p.part == "b" or p.fid in LIFE_IDS):
            out.append(p.dst)
    return out


LIFE_IDS = [E.a_filter_id(4, 9), E.a_filter_id(6, 65), E.a_filter_id(4, 13), E.a_filter_id(6, 0), E.a_filter_id(4, 31),
            E.a_filter_id(6, 121), E.a_filter_id(4, 0), E.a_filter_id(6, 128)] + sorted(C.b_kinds)[:2]


def test_table_lifecycle():
    """One engine whose filter image grows, moves, shrinks and is re-mapped; after every step wg_rx_check and a
    fused open (which reads the tables through the RxTables struct that is rebuilt only after a change) answer as the
    oracle does for the filters and the slot map as they then stand. Every key slot is asked every destination, so a
    slot that reads another filter's nodes shows. No graph is replayed across a wg_filter_set."""
    W = wg()
    L = W._lib
    dests = _lifecycle_dests()
    rng = np.random.default_rng(E.SEED + 4)
    pkts = [E.packet(d, E.min_len(d) + (k % 3) * 7, rng) for k, d in enumerate(dests)] + [b"", b"\x45" * 19]
    model, slot_ids = {}, {}
    engine = _engine(install=False)

    def check(step):
        fos = {s: (None if f == E.NO_FILTER else E.oracle_filter(model.get(f, []))) for s, f in slot_ids.items()}
        slots = sorted(slot_ids) + [E.KEY_SLOTS - 1]  # the last: never mapped
        items = [(s, pt, f"{step}: slot {s} -> filter {slot_ids.get(s, 'none')}, {pt[:40].hex()}")
                 for s in slots for pt in pkts]
        b = Batch(items, seed=50 + len(step), unaligned=True, filter_of_slot=fos)
        b.check_rx_check(engine, f"{step}, rx_check")
        b.check_fused(engine, what=f"{step}, fused open", twice=False)
        return b

    def set_filter(fid, prefixes):
        engine.filter_set(fid, prefixes)
        model[fid] = prefixes

    def set_slots(first, ids):
        engine.slot_filters_set(first, ids)
        slot_ids.update({first + k: f for k, f in enumerate(ids)})

    try:
        # 1. filters 0 .. 9; slot 10 has no filter, slot 12 an id above every id set
        for k, fid in enumerate(LIFE_IDS):
            set_filter(k, C.filters[fid])
        set_slots(0, list(range(10)) + [E.NO_FILTER, 3, 300])
        b = check("ten filters")
        assert {rx.PKT_OK, rx.PKT_FILTERED, rx.PKT_BADIP, rx.PKT_KEEPALIVE} == set(b.want)
        per_slot = [tuple(b.want[k * len(pkts):(k + 1) * len(pkts)]) for k in range(10)]
        assert len(set(per_slot)) == 10  # the ten filters answer differently: a mixed-up base shows
        # 2. filter 0 grows from 4 nodes to 21: every later filter's nodes move, the image is reallocated
        set_filter(0, [(E.ip(E.X6), 127), (E.ip(E.X4), 31)])
        check("filter 0 grown")
        # 3. filter 0 shrinks to nothing
        set_filter(0, [])
        check("filter 0 emptied")
        # 4. a sparse id: slot 12 already names it; the ids between stay empty filters
        set_filter(300, [(E.ip(E.Y4), 23), (E.ip(E.Y6), 64)])
        set_slots(13, [150, 299])
        b = check("filter 300 set")
        at = lambda s: b.want[sorted(slot_ids).index(s) * len(pkts):][:len(pkts)]  # noqa: E731
        assert rx.PKT_OK in at(12) and rx.PKT_OK not in at(13) and rx.PKT_OK not in at(14)
        # 5. only the slot map changes, from a first slot above 0
        set_slots(5, [9, 8, E.NO_FILTER, 300, 5])
        check("slots 5 .. 9 re-mapped")
        # 6. refused calls leave everything as it was
        def raw(fid, family, plen):
            arr = (L.WgPrefix * 1)()
            arr[0].family, arr[0].prefix_len = family, plen
            return engine._lib.wg_filter_set(engine.ctx, fid, ctypes.addressof(arr), 1)
        assert raw(L.WG_MAX_FILTERS, 4, 8) == L.WG_ERANGE
        assert raw(1, 5, 8) == L.WG_EINVAL
        assert raw(1, 4, 33) == L.WG_EINVAL
        assert raw(1, 6, 129) == L.WG_EINVAL
        assert engine._lib.wg_slot_filters_set(engine.ctx, E.KEY_SLOTS, 1, (ctypes.c_uint32 * 1)(0)) == L.WG_ERANGE
        check("after refused calls")
    finally:
        engine.close()
