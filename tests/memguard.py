"""Guarded arenas for the memory contract of the C ABI (tests/test_gpu_memory_contract.py, tests/test_memguard_host.py).

include/qvc.h promises that the library allocates nothing, that every scratch size comes from a *_bytes() query and
that padding is ignored.  Two kinds of kernel error break that without any parity test noticing: a store outside a
caller-owned buffer (it lands in allocator slack or in a neighbouring tensor) and a read of a byte that no step of
this call wrote (the tests repeat shapes, so the stale value is last call's right answer).  An arena makes both
visible:

    [ guard | payload | guard ]      one torch.uint8 allocation

  * the payload starts 256-byte aligned (the library checks workspace, blob and state for that) and the trailing guard
    starts at byte `nbytes` exactly -- no alignment slack after the payload, so a store one element past the end is seen;
  * each guard is GUARD = 256 KiB.  That is a condition, not a measurement: twice the largest tile one workgroup
    stores at once (64 frames x 512 channels x 4 B = 128 KiB), so a plausible over-run lands inside the arena and never
    outside the allocation;
  * FILLS are the (payload, guard) byte patterns a call is repeated under.  Under 0xFF every uninitialised byte is a NaN
    in f16, bf16 and fp32: a read that is masked by a multiply instead of a select poisons the result; 0x00 and 0x3C
    (f16 1.06, fp32 0.0115) are finite and differ, so a result that depends on them differs between the runs.

Outputs are compared bit-wise (int32 / uint8 views), so NaNs compare too.
"""
import torch

GUARD = 256 * 1024
FILLS = [(0x00, 0xA5), (0x3C, 0x5A), (0xFF, 0xFF)]


class Arena:
    """One caller-owned buffer of `nbytes` between two guards."""

    def __init__(self, name, nbytes, device, fill, guard_fill):
        self.name, self.nbytes, self.fill, self.guard_fill = name, int(nbytes), int(fill), int(guard_fill)
        self.raw = torch.empty(self.nbytes + 2 * GUARD + 256, dtype=torch.uint8, device=device)
        self.lo = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256        # everything in front of the payload is guard
        self.hi = self.lo + self.nbytes
        self.raw.fill_(self.guard_fill)
        self.payload = self.raw[self.lo:self.hi]
        self.payload.fill_(self.fill)
        assert self.payload.data_ptr() % 256 == 0 and self.raw.numel() - self.hi >= GUARD and self.lo >= GUARD

    def view(self, dtype, shape):
        """The payload as the tensor to pass (its bytes must divide into `dtype`)."""
        return self.payload.view(dtype).reshape(shape)

    def ptr(self):
        return self.payload.data_ptr()

    def refill(self):
        self.payload.fill_(self.fill)

    def check(self):
        """[] or one dict per damaged guard: name, side, distance (1 = the byte next to the payload) of the changed
        byte nearest to the payload, count of changed bytes."""
        found = []
        for side, region in (("before", self.raw[:self.lo]), ("after", self.raw[self.hi:])):
            bad = (region != self.guard_fill).nonzero().reshape(-1)
            if bad.numel():
                dist = self.lo - int(bad.max()) if side == "before" else int(bad.min()) + 1
                found.append(dict(name=self.name, side=side, distance=dist, count=int(bad.numel())))
        return found


class ArenaSet:
    """Every caller-owned buffer of one call, each in its own arena, under one (payload, guard) fill."""

    def __init__(self, device, fill, guard_fill):
        self.device, self.fill, self.guard_fill = torch.device(device), int(fill), int(guard_fill)
        self.arenas = {}
        self._inputs = {}

    def _new(self, name, nbytes):
        """The arena `name`; asked for again (a second call on the same arenas) it is handed back as it is, not refilled."""
        if name in self.arenas:
            assert self.arenas[name].nbytes == nbytes, (name, self.arenas[name].nbytes, nbytes)
            return self.arenas[name]
        a = self.arenas[name] = Arena(name, nbytes, self.device, self.fill, self.guard_fill)
        return a

    def input(self, name, host, track=True):
        """An input, device array or blob: the arena holds a copy of `host` (an existing arena is overwritten in place),
        and changed_inputs() compares against it.  track=False: a buffer the call updates in place (z of the flows)."""
        host = host.contiguous()
        raw = host.reshape(-1).view(torch.uint8)
        a = self._new(name, raw.numel())
        a.payload.copy_(raw)
        if track:
            self._inputs[name] = a.payload.clone()
        return a.view(host.dtype, tuple(host.shape))

    def output(self, name, dtype, shape):
        """An output: payload filled, exactly numel * itemsize bytes."""
        n = 1
        for s in shape:
            n *= int(s)
        return self._new(name, n * torch.empty(0, dtype=dtype).element_size()).view(dtype, tuple(shape))

    def scratch(self, name, nbytes):
        """Workspace / scratch / state of exactly `nbytes` (what the *_bytes() query returned), filled."""
        return self._new(name, nbytes).payload

    def check(self):
        return [f for a in self.arenas.values() for f in a.check()]

    def changed_inputs(self, names=None):
        """Names of the inputs (all, or those of `names`) whose payload is no longer byte-identical to what was put in."""
        return [n for n, raw in self._inputs.items() if (names is None or n in names) and not torch.equal(self.arenas[n].payload, raw)]


def describe_guards(found):
    return "; ".join(f"{f['name']}: {f['count']} byte(s) changed {f['side']} the payload, nearest {f['distance']} byte(s) from its edge"
                     for f in found)


def bits_equal(a, b):
    """Bit-wise equality of two tensors of one dtype and shape (NaN == NaN when the patterns agree)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous(), b.contiguous()
    if a.element_size() == 4:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def gap_ranges(bufs, nbytes):
    """[(lo, hi)] byte ranges of a workspace of `nbytes` that lie in no buffer of emu.workspace_map: the alignment gaps
    between the sub-buffers and the tail."""
    spans = sorted((b["offset"], b["offset"] + b["bytes"]) for b in bufs)
    gaps, at = [], 0
    for lo, hi in spans:
        assert lo >= at, "workspace buffers overlap"
        if lo > at:
            gaps.append((at, lo))
        at = hi
    assert at <= nbytes, (at, nbytes)
    if at < nbytes:
        gaps.append((at, nbytes))
    return gaps


def check_gaps(ws, bufs, fill, nbytes=None):
    """[] or [(offset of the first changed byte, changed bytes)] per gap of the workspace `ws` (uint8) that no longer
    holds `fill` everywhere."""
    found = []
    for lo, hi in gap_ranges(bufs, ws.numel() if nbytes is None else nbytes):
        bad = (ws[lo:hi] != fill).nonzero().reshape(-1)
        if bad.numel():
            found.append((lo + int(bad.min()), int(bad.numel())))
    return found
