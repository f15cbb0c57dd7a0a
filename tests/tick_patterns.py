"""The fixed tick pattern of the tick-form tests (tests/test_live_tick_host.py on the CPU twin, tests/test_gpu_live_tick.py
on the GPU): what slot b passes as n_new at tick k, written out once so that both suites feed the same thing.

H stands for the hop.  Raw values: -3 must behave as 0 and H + 5 as H (the clamp is the library's).  What the pattern
holds, by construction:
  * slot 0 brings nothing at the very first tick, then 1 frame at pos 0; slot 1 brings 1 frame at pos 0;
  * ticks of 1, 2 and 3 frames (a ring shift that is 4-byte aligned only) and of H frames;
  * slot 1 is idle for ticks 1-3 while slot 0 runs, slot 0 for ticks 7-9 while slot 1 runs;
  * one -3 and one H + 5 per slot;
  * the sequences repeat until every stream has flushed, so the end of a stream falls inside a tick and flush ticks
    follow it.
"""
H = "H"
SEQUENCES = (
    (0, 1, H, 2, -3, (H, 5), 3, 0, 0, 0, 1, H),
    (1, 0, 0, 0, H, 2, 3, H, (H, 5), 1, 0, H),
    (2, 3, 0, H, 1, H, 0, 2, (H, 5), 3, -3, 1),
)


def raw_count(slot, tick, hop):
    """n_new of `slot` at `tick`, unclamped."""
    seq = SEQUENCES[slot % len(SEQUENCES)]
    v = seq[tick % len(seq)]
    if v == H:
        return hop
    if isinstance(v, tuple):
        return hop + v[1]
    return v


def clamp(n, hop):
    return min(max(int(n), 0), hop)


def all_hop(_slot, _tick, hop):
    return hop


def all_one(_slot, _tick, _hop):
    return 1
