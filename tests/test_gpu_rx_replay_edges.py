"""The replay window of wg_rx_check(WG_RX_REPLAY) on the MI355X at its edges (pytest -m gpu), on every
launch structure: the case lists of tests/replay_edge_cases.py (ring offsets and jump lengths around word
and ring boundaries at W = 64, 192 and 576, windows around 2^32, 2^63 and Reject-After-Messages, many
windows jumping by a whole window in one batch, mixed high words inside one wave, duplicates at their
extremes, W = 65536, the state calls). Every expectation is oracle.rx.ReplayWindow's; every comparison
is exact: the statuses of each batch, and after each batch top and bitmap words of every slot the test
touched and of neighbours it did not. tests/test_replay_edges.py checks the lists and the oracle on the CPU."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import replay_edge_cases as E
from oracle import rx
from wgtest import wg

pytestmark = pytest.mark.gpu

OK, REPLAY = rx.PKT_OK, rx.PKT_REPLAY


def _dev():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.device("cuda", 0)


@contextlib.contextmanager
def _engine(kind):
    """An engine whose replay checks take one launch structure: three launches (judge with the windows
    advanced by its last block, insert, fix-up + mark; 512 key slots), four (the same with a separate
    advance launch; 1024 key slots) or five (WG_RX_LAUNCHES=5 on 512 key slots). The variable is read
    when the context's receive state is created (replay_enable) and restored afterwards."""
    old = os.environ.get("WG_RX_LAUNCHES")
    os.environ["WG_RX_LAUNCHES"] = "5" if kind == "five_launches" else "3"
    try:
        e = wg().Engine(0, key_slots=1024 if kind == "four_launches" else 512)
        e.replay_enable(64)
    finally:
        if old is None:
            del os.environ["WG_RX_LAUNCHES"]
        else:
            os.environ["WG_RX_LAUNCHES"] = old
    try:
        yield e
    finally:
        e.close()


@pytest.fixture(params=["three_launches", "four_launches", "five_launches"])
def rp_engine(request):
    with _engine(request.param) as e:
        yield e


@pytest.fixture(params=["three_launches", "five_launches"])
def rp_engine_512(request):
    """512 key slots: the three-launch structure (the block-wide clear of the last block) and the
    five-launch one as a control."""
    with _engine(request.param) as e:
        yield e


def _check(engine, b):
    """One wg_rx_check(WG_RX_REPLAY) over the batch (zero-length packets): the statuses it leaves."""
    torch, dev = _dev()
    W = wg()
    n = len(b.slots)
    z = np.zeros(n, np.uint64)
    desc = W.pack_desc(z, z, b.counters, np.zeros(n, np.int64), b.slots)
    d = torch.from_numpy(W.desc_as_int64(desc)).to(dev)
    st = torch.from_numpy(b.status.astype(np.int32)).to(dev)
    engine.rx_check(d, torch.zeros(64, dtype=torch.uint8, device=dev), st, W._lib.WG_RX_REPLAY)
    torch.cuda.synchronize()
    return st.cpu().numpy().astype(np.int64).tolist()


def _assert_statuses(got, want, b, what, name=lambda s: f"slot {s}"):
    if got != want:
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} statuses differ; first at index {i}: "
                             f"{name(int(b.slots[i]))}, counter {int(b.counters[i]):#x}: "
                             f"device {got[i]}, oracle {want[i]}")


def _assert_windows(engine, Wb, expected, what, name=lambda s: f"slot {s}"):
    """expected: slot -> (top, words) from ReplayWindow.bitmap."""
    for s, (otop, owords) in expected.items():
        top, words = engine.replay_state(s, Wb)
        assert top == otop, f"{what}: {name(s)}: top {top:#x}, oracle {otop:#x}"
        words = words.tolist()
        if words != owords:
            k = next(k for k in range(len(owords)) if words[k] != owords[k])
            raise AssertionError(f"{what}: {name(s)}: word {k} of {len(owords)} is {words[k]:#018x}, "
                                 f"oracle {owords[k]:#018x} (top {top:#x}, top % W = {top % Wb})")


def _run(engine, o, Wb, b, state_slots, what, name=lambda s: f"slot {s}"):
    got = _check(engine, b)
    want = E.expect(o, engine.key_slots, b)
    _assert_statuses(got, want, b, what, name)
    _assert_windows(engine, Wb, {s: o.bitmap(s) for s in state_slots}, what, name)
    return want


# ---- 1. the boundary grid -----------------------------------------------------------------------
@pytest.mark.parametrize("top_hole", [True, False])
@pytest.mark.parametrize("Wb", E.GRID_WINDOWS)
def test_boundary_grid(rp_engine, Wb, top_hole):
    """One key slot per (band, ring offset a, length): the window is filled to T (T % W == a, around a few
    W, 2^32, 2^63, or so that the arrival is REJECT_AFTER - 1) but for three holes, one counter
    T + len - 1 arrives (a batch of one packet per slot, strictly increasing: no table), then every
    counter of [T + len - W - 2, T + len] is probed. top_hole=False puts the third hole at T - 2 so
    that the top after the fill is T exactly and the jump is len exactly (see grid_cases). A failure
    names the case. Slots n and n + 1 are never touched and must stay empty."""
    engine = rp_engine
    cases, batches = E.grid_reference(Wb, top_hole)
    n = len(cases)
    engine.replay_enable(Wb)  # empties every window
    name = lambda s: str(cases[s]) if s < n else f"untouched slot {s}"  # noqa: E731
    for what, b, want, state in batches:
        assert set(want) == ({OK, REPLAY} if what == "probe" else {OK}) and len(state) == n + 2
        _assert_statuses(_check(engine, b), want, b, what, name)
        _assert_windows(engine, Wb, state, what, name)


# ---- 2. many slots jumping by a whole window at once ----------------------------------------------
@pytest.mark.parametrize("k", E.JUMP_KS)
@pytest.mark.parametrize("Wb", [576, 1024])
def test_many_windows_jump_at_once(rp_engine_512, Wb, k):
    """All 512 windows full; one batch moves exactly k of them by W or more (W, W + 1, 10 W,
    2^33 + 7), half of the others by W - 1, a quarter by 1, the rest not at all. With 512 key slots
    and more than 8 words per window the last block of k_rp_judge lists up to 64 such slots and clears
    them block-wide; k = 63, 64, 65 and 300 fill the list to its last entry and past it. A probe of
    top - W - 1, top - W, top - 2 and top - 1 follows; all 512 windows are compared after each batch."""
    engine = rp_engine_512
    engine.replay_enable(Wb)
    fill, fill_want, after = E.jump_prefill_reference(Wb)
    o = E.copy_window(after)
    _assert_statuses(_check(engine, fill), fill_want, fill, "prefill")
    p = E.jump_plan(Wb, k)
    kind = lambda s: f"slot {s} (jump {p.jumps[s]})"  # noqa: E731
    _run(engine, o, Wb, p.batch, range(512), "jump", kind)
    want = _run(engine, o, Wb, p.probe, range(512), "probe", kind)
    assert {OK, REPLAY} == set(want)


# ---- 3. mixed high words inside one wave --------------------------------------------------------
@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("nslots", [1, 3])
def test_mixed_high_words_in_one_wave(rp_engine, nslots, sort):
    """Batches of 256 packets of one slot (then three interleaved) whose counters sit around 2^32,
    around 2^33 and at 5 * 2^32 + j: in every wave the maximum has a small low word and smaller
    counters have low words near 2^32 - 1, so a 64-bit maximum whose low word is reduced over every
    lane (not only those holding the largest high word) moves the top too far. Unsorted (the table
    path) and sorted by (slot, counter) without repeats (no table); then a probe around the new top
    and around 2^32."""
    engine = rp_engine
    engine.replay_enable(E.MIXED_W)
    o = rx.ReplayWindow(E.MIXED_W)
    for i, b in enumerate(E.mixed_batches(nslots, sort)):
        _run(engine, o, E.MIXED_W, b, range(nslots + 1), f"batch {i}")


# ---- 4. duplicates at their extremes and the rejection threshold ----------------------------------
def test_duplicates_and_reject_after(rp_engine):
    """20,000 packets over 8 slots: one (slot, counter) pair 5,000 times (only its lowest index is
    accepted), a pair whose first two copies failed authentication (they stay BADTAG, the third copy is
    accepted), one counter on all 8 slots (no duplicates), REJECT_AFTER - 1 twice (one accepted; the
    slot's top becomes REJECT_AFTER), REJECT_AFTER, REJECT_AFTER + 1 and 2^64 - 1 twice each (all
    rejected), and two descriptors whose key slot is past the table (left alone: their status stays as
    it came, and they are kept from the oracle, which knows no table size). The same batch again is
    all REPLAY but for those."""
    engine = rp_engine
    engine.replay_enable(E.DUP_W)
    o = rx.ReplayWindow(E.DUP_W)
    p = E.dup_plan(engine.key_slots)
    first = _run(engine, o, E.DUP_W, p.batch, range(9), "first")
    assert first[p.heavy[0]] == OK and first[p.badtag[2]] == OK
    again = _run(engine, o, E.DUP_W, p.batch, range(9), "again")
    assert OK not in [x for i, x in enumerate(again) if i not in set(p.outside.tolist())]
    assert [again[i] for i in p.outside] == [OK, OK]


# ---- 5. window sizes and state calls ------------------------------------------------------------
def test_largest_window(rp_engine):
    """W = 65536 (1,024 words per slot) on 6 slots: a window filled across 2^32, jumps by W - 1, W and 3
    (strictly increasing: no table), 400 probes around both ends of each new window; the full bitmaps
    of the 6 slots and of slot 6 (never touched) after every batch."""
    engine = rp_engine
    engine.replay_enable(E.MAX_W)
    for i, (b, want, state) in enumerate(E.maxw_reference()):
        _assert_statuses(_check(engine, b), want, b, f"batch {i}")
        _assert_windows(engine, E.MAX_W, dict(enumerate(state)), f"batch {i}")


def test_window_size_limits_keep_the_window(rp_engine):
    """wg_replay_enable(65536 + 64) and (65537) are refused and the window enabled before keeps
    working with its contents."""
    engine = rp_engine
    lib = wg().lib()
    engine.replay_enable(192)
    o = rx.ReplayWindow(192)
    _run(engine, o, 192, E.make_batch([0, 0, 1], [500, 400, 7]), range(3), "before")
    assert lib.wg_replay_enable(engine.ctx, 65536 + 64) == wg()._lib.WG_EINVAL
    assert lib.wg_replay_enable(engine.ctx, 65537) == wg()._lib.WG_EINVAL
    _assert_windows(engine, 192, {s: o.bitmap(s) for s in range(3)}, "after the refused calls")
    want = _run(engine, o, 192, E.make_batch([0, 0, 0, 1, 1], [500, 309, 308, 7, 8]), range(3), "after")
    assert want == [REPLAY, OK, REPLAY, REPLAY, OK]


def test_reset_state_and_enable_calls(rp_engine):
    """replay_reset(first, n) empties exactly slots first .. first + n - 1 (W = 192): the slots on both
    sides keep top and words, the reset ones read top 0 and zero words and accept counter 0 again.
    replay_state with a wrong word count is refused. replay_enable with another W empties every window."""
    engine = rp_engine
    lib, EINVAL = wg().lib(), wg()._lib.WG_EINVAL
    Wb, first, n = 192, 5, 3
    engine.replay_enable(Wb)
    o = rx.ReplayWindow(Wb)
    slots = list(range(first - 1, first + n + 1))
    ctr = [(1 << 32) - 100 + 61 * s + j for s in slots for j in (0, 3, 150, 191)]
    _run(engine, o, Wb, E.make_batch(np.repeat(slots, 4), ctr), slots, "before")
    engine.replay_reset(first, n)
    for s in range(first, first + n):
        o.reset(s)
    _assert_windows(engine, Wb, {s: o.bitmap(s) for s in slots}, "after the reset")
    assert o.bitmap(first - 1)[0] > 1 << 32 and o.bitmap(first + n)[0] > 1 << 32 and o.bitmap(first) == (0, [0, 0, 0])
    want = _run(engine, o, Wb, E.make_batch(slots, [0] * len(slots)), slots, "counter 0")
    assert want == [REPLAY] + [OK] * n + [REPLAY]
    top, bits = ctypes.c_uint64(), np.zeros(4, np.uint64)
    for words in (2, 4, 0):
        assert lib.wg_replay_state(engine.ctx, first, ctypes.byref(top), bits.ctypes.data, words) == EINVAL
    assert lib.wg_replay_state(engine.ctx, first, ctypes.byref(top), bits.ctypes.data, 3) == 0 and top.value == 1
    engine.replay_enable(576)
    empty = rx.ReplayWindow(576)
    _assert_windows(engine, 576, {s: empty.bitmap(s) for s in slots + [0, engine.key_slots - 1]}, "after enable(576)")
    _run(engine, empty, 576, E.make_batch(slots, [0] * len(slots)), slots, "counter 0 on the new window")
