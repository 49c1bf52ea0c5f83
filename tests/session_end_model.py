"""Plain-Python restatement of the end of a session on the device (include/wgaead.h, "the end of a session on the
device"), on top of hs_install_model and timers_model, neither of which it changes: wg_rx_sessions_compact over the
bucket-for-bucket Table, wg_hs_install with WG_HS_INSTALL_COMPACT, and wg_timers_sweep with WG_TIMERS_WIPE. Written from
the header only. Which bucket of a chain a live entry lands in after a compaction depends on thread order on the device;
the model places them in table order, and nothing a test compares (lookups, counts, statuses) depends on the order.
"""
from __future__ import annotations

import hs_install_model as IM
import timers_model as TM


def compact(table: IM.Table, min_retired: int = 1) -> list:
    """wg_rx_sessions_compact: [live, dropped, compacted, 0]. With at least max(min_retired, 1) retired entries the table
    is rebuilt from its live entries into the same capacity (used == count afterwards); otherwise nothing changes."""
    live, retired = table.count()
    if retired < max(int(min_retired), 1):
        return [live, 0, 0, 0]
    entries = [(e[0], e[1]) for e in table.ent if e[1] not in (0, IM.RETIRED)]  # in table order
    table.ent = [[0, 0] for _ in range(table.capacity)]
    table.used = 0
    for index, hi in entries:
        table._place(index, hi)
    return [live, retired, 1, 0]


_compact_table = compact  # (install's keyword has the function's name)


def install(table: IM.Table, state: IM.State, entries, n_entries, send_slot, recv_slot, *, compact=True, **kw):
    """wg_hs_install; with compact (WG_HS_INSTALL_COMPACT) the table is compacted in front of step 3 when the
    ring's m = min(*n_entries, n) entries would not fit (used + m > C / 2) and it holds retired entries (used > count).
    Returns what hs_install_model.install returns."""
    if compact:
        n = len(entries)
        m = n if n_entries is None else min(int(n_entries), n)
        live, retired = table.count()
        if table.used + m > table.capacity // 2 and retired:
            _compact_table(table, 1)
    return IM.install(table, state, entries, n_entries, send_slot, recv_slot, **kw)


def sweep(timers: TM.Timers, state: IM.State, now, cap_exp, cap_init, cap_keep, *, retire=False, wipe=False, **kw):
    """wg_timers_sweep; with retire and wipe (WG_TIMERS_WIPE) both keys of every listed session are zeroed in state.keys
    (the recv slot's only if it lies inside the key table). Every output is timers_model's."""
    assert retire or not wipe, "WG_TIMERS_WIPE goes with WG_TIMERS_RETIRE only"
    out = timers.sweep(now, cap_exp, cap_init, cap_keep, retire=retire, **kw)
    if wipe:
        for e in out["expired"]:
            state.keys[int(e["send_slot"])] = bytes(32)
            if int(e["recv_slot"]) < timers.K:
                state.keys[int(e["recv_slot"])] = bytes(32)
    return out
