"""The handshake rate limiter as one host would write it: WireGuard's token bucket per source, one record at a
time. The reference has no limiter; this is the plain sequential rule that wg_hs_ratelimit (include/wgaead.h)
applies to a whole ring on the device, kept here as the package's host mirror of it."""
from __future__ import annotations

U64 = (1 << 64) - 1


def ratelimit_key(family: int, addr) -> tuple[int, bytes]:
    """The bucket's key of a source: the IPv4 address, or the IPv6 /64. Never the port, the bytes behind an IPv4
    address or the low half of an IPv6 one."""
    if family not in (4, 6):
        raise ValueError(f"address family {family}")
    a = bytes(addr)
    width = 4 if family == 4 else 8
    if len(a) < width:
        raise ValueError(f"{len(a)} address bytes for family {family}")
    return family, a[:width]


class RateLimiter:
    """`cost` ticks per handshake, `burst` handshakes: allow(src, now) for one handshake message at tick `now`."""

    MAX_BURST = 16

    def __init__(self, cost: int, burst: int):
        if not 1 <= cost <= 1 << 56 or not 1 <= burst <= self.MAX_BURST:
            raise ValueError(f"ratelimit cost {cost}, burst {burst}")
        self.cost, self.burst = cost, burst
        self.entries: dict[tuple[int, bytes], list[int]] = {}  # key -> [tokens, last]

    @property
    def max(self) -> int:
        return self.cost * self.burst

    def allow(self, src, now: int) -> bool:
        """src: (family, addr) or (family, addr, port). Tick 0 is "never": nothing is limited and nothing is kept."""
        if now == 0:
            ratelimit_key(src[0], src[1])
            return True
        key = ratelimit_key(src[0], src[1])
        e = self.entries.get(key)
        if e is None:
            e = self.entries[key] = [self.max, now]
        tokens, last = e
        age = now - last if now >= last else 0
        tokens = min(self.max, min(U64, tokens + age))
        if now >= last:
            last = now
        ok = tokens >= self.cost
        if ok:
            tokens -= self.cost
        e[0], e[1] = tokens, last
        return ok

    def expire(self, now: int) -> int:
        """Drop the entries that a full bucket has replaced by now (now - last >= max); how many were dropped."""
        stale = [k for k, (_, last) in self.entries.items() if (now - last if now >= last else 0) >= self.max]
        for k in stale:
            del self.entries[k]
        return len(stale)
