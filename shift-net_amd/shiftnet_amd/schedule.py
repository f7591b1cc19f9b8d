"""Launch orders of the bf16 engine's frame-wavefront and streams schedules (Engine._shift_chain): pure host logic."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple


def wavefront_order(revs: Sequence[bool], T: int, G: int, circular: bool) -> List[Tuple[int, int]]:
    """Launch order (unit, frame group) of the frame wavefront: sweeps over the units, every unit advancing by at most one group per sweep --
    the lowest-numbered group whose inputs exist.  Unit u needs, of unit u - 1, the group itself and the group of the ONE frame its boundary
    frame borrows from: frame t0 - 1 for a forward unit, t0 + nt for a reverse one (gshift_deblur1.py:504-518); outside [0, T) that frame wraps
    (deblur2, gshift_deblur2.py:504-505) or does not exist (kept boundary frame).  On the ring the first group of a forward unit therefore comes
    last.  Pure host logic: tests/test_host_logic.py checks every order against the dependency rule."""
    ng = -(-T // G)
    groups = [(t0, min(G, T - t0)) for t0 in range(0, T, G)]
    done = [[False] * ng for _ in revs]

    def ready(u: int, j: int) -> bool:
        if u == 0:
            return True
        t0, nt = groups[j]
        tb = t0 + nt if revs[u] else t0 - 1
        if tb < 0 or tb >= T:
            tb = (tb % T) if circular else None
        need = {j} | ({tb // G} if tb is not None else set())
        return all(done[u - 1][g] for g in need)
    order: List[Tuple[int, int]] = []
    left = len(revs) * ng
    while left:
        progressed = False
        for u in range(len(revs)):
            j = next((j for j in range(ng) if not done[u][j] and ready(u, j)), None)
            if j is None:
                continue
            order.append((u, j))
            done[u][j] = True
            left -= 1
            progressed = True
        assert progressed, "frame wavefront: dependency cycle"
    return order


def stream_plan(revs: Sequence[bool], T: int, ng: int, circular: bool, ring: int):
    """Frame groups and cross-stream edges of the streams schedule (Engine._shift_chain_streams).  Returns (groups, plan): groups[g] = (t0, nt),
    ng contiguous ranges as equal as possible; plan[u][g] = (raw, war), lists of (unit, group) whose events group g's stream waits for before it
    launches unit u.  raw: the group that owns the ONE frame g's boundary frame borrows from -- frame t0 - 1 for a forward unit, t0 + nt for a
    reverse one (gshift_deblur1.py:504-518), wrapped on the ring (gshift_deblur2.py:504-505), nobody when that frame does not exist (kept
    boundary) -- must have WRITTEN unit u - 1's output.  war: unit u overwrites ring slot u % ring, last used by unit u - ring, whose output the
    groups that borrow from g were still READING in CAB2 of unit u - ring + 1.  Same-group edges are stream order.  Pure host logic
    (tests/test_host_logic.py replays every plan against the dependency rule)."""
    assert ng >= 1 and T >= ng and ring >= 2
    bounds = [T * j // ng for j in range(ng + 1)]
    groups = [(bounds[j], bounds[j + 1] - bounds[j]) for j in range(ng)]

    def lender(u: int, g: int) -> Optional[int]:
        t0, nt = groups[g]
        tb = t0 + nt if revs[u] else t0 - 1
        if tb < 0 or tb >= T:
            if not circular:
                return None
            tb %= T
        o = max(j for j in range(ng) if bounds[j] <= tb)
        return None if o == g else o
    plan = []
    for u in range(len(revs)):
        row = []
        for g in range(ng):
            ln = lender(u, g)
            raw = [(u - 1, ln)] if (u > 0 and ln is not None) else []
            uu = u - ring + 1
            war = [(uu, gg) for gg in range(ng) if gg != g and lender(uu, gg) == g] if uu >= 1 else []
            row.append((raw, war))
        plan.append(row)
    return groups, plan
