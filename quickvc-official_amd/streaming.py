"""Exact chunked conversion of many concurrent streams (BASELINE.json configs[4]).

The reference processes a whole utterance in one shot (no chunking, no streaming).  Every
op on the path is a convolution with a bounded receptive field -- measured on the oracle: an input
frame influences output frames within +-84 frames (enc_p WN 32, flow 32, decoder ~20) -- and the speaker
embedding g is global, so a window of ``hop + 2*context`` frames reproduces its central ``hop`` frames
exactly when ``context >= 84``.  Windows are clamped to the utterance, so the first / last window touch
the true sequence edges and stay exact there too (the convs zero-pad activations at the *sequence*
edges at every layer, which a zero-padded window could not reproduce).

All windows have ONE shape, (streams, 256, hop + 2*context), so the launch sequence is captured once
in a hipGraph and replayed per chunk.  Latency of a streamed chunk = ``context`` frames of look-ahead.
"""
from __future__ import annotations

import struct
from typing import Iterator, Optional, Tuple

import torch

RECEPTIVE_FRAMES = 84      # measured (tests/test_gpu_parity.py::test_chunked_streaming_is_exact re-checks it)


class ChunkedConverter:
    """Fixed-shape, graph-replayed windowed conversion for ``streams`` concurrent utterances."""

    def __init__(self, model, streams: int, hop_frames: int = 320, context: int = 88, use_graph: bool = True):
        if context < RECEPTIVE_FRAMES:
            raise ValueError(f"context {context} < receptive field {RECEPTIVE_FRAMES}: chunks would not be exact")
        self.model, self.streams, self.hop, self.context = model, streams, hop_frames, context
        self.window = hop_frames + 2 * context
        self.engine = model.engine()
        dev = self.engine.device
        mc = model.model_config
        self.spf = model.samples_per_frame
        self._unit = torch.zeros(streams, mc.get("unit_channels", 256), self.window, device=dev)
        self._noise = torch.zeros(streams, mc["inter_channels"], self.window, device=dev)
        self._g = torch.zeros(streams, mc["gin_channels"], device=dev)
        self._out = torch.zeros(streams, 1, self.window * self.spf, device=dev)
        self._graph = None
        self._stream = torch.cuda.Stream(dev)
        # the graph bakes the workspace pointer in: own the buffer (the engine's shared one is replaced, i.e. freed,
        # as soon as somebody asks the same engine for a larger batch)
        self._ws = self.engine.alloc_workspace(streams, self.window)
        if use_graph:
            with torch.cuda.stream(self._stream):
                self.engine.infer_batch(self._unit, self._g, self._noise, self._out, ws=self._ws)      # warm-up (code objects)
                self._stream.synchronize()
                self._graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph, stream=self._stream):
                    self.engine.infer_batch(self._unit, self._g, self._noise, self._out, ws=self._ws)

    def windows(self, total_frames: int) -> Iterator[Tuple[int, int, int]]:
        """(window_start, chunk_start, chunk_len) for every hop of an utterance of ``total_frames``."""
        if total_frames < self.window:
            raise ValueError(f"utterance of {total_frames} frames is shorter than one window ({self.window})")
        for t0 in range(0, total_frames, self.hop):
            n = min(self.hop, total_frames - t0)
            a = min(max(t0 - self.context, 0), total_frames - self.window)
            yield a, t0, n

    @torch.no_grad()
    def convert(self, unit: torch.Tensor, g: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """unit (S,256,T), g (S,gin), noise (S,inter,T) -> (S,1,T*samples_per_frame); == infer_batch on the whole thing."""
        S, _, T = unit.shape
        if S != self.streams:
            raise ValueError(f"built for {self.streams} streams, got {S}")
        dev = self.engine.device
        if noise is None:
            noise = torch.randn(S, self.model.model_config["inter_channels"], T, device=dev)
        unit, noise = unit.to(dev, torch.float32), noise.to(dev, torch.float32)
        g = g.to(dev, torch.float32)
        out = torch.empty(S, 1, T * self.spf, device=dev)
        # inputs (and the noise drawn above) may still be pending on the caller's stream: order the side stream after it
        self._stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self._stream):
            for t in (unit, noise, g, out):
                t.record_stream(self._stream)
            self._g.copy_(g.reshape(S, -1))
            for a, t0, n in self.windows(T):
                self._unit.copy_(unit[:, :, a:a + self.window])
                self._noise.copy_(noise[:, :, a:a + self.window])
                if self._graph is not None:
                    self._graph.replay()
                else:
                    self.engine.infer_batch(self._unit, self._g, self._noise, self._out, ws=self._ws)
                lo = (t0 - a) * self.spf
                out[:, :, t0 * self.spf:(t0 + n) * self.spf].copy_(self._out[:, :, lo:lo + n * self.spf])
            self._stream.synchronize()
        return out


class StreamSnapshot:
    """One segment-ring stream between two calls, free of the slot, the batch size and the hop it ran under
    (qvc_stream_export_slots): ``data`` -- the kept frames of every ring, the position and the length, a uint8 tensor on
    a device or the host --, ``tag`` -- the layout fingerprint the destination must share --, the stream's speaker
    embedding ``g`` and generator ``key``, ``position`` / ``length`` from the converter's host mirrors, and
    ``rng = (seed, noise_scale)`` when the source converter draws its noise from the generator, else None.
    ``tobytes`` / ``frombytes``: a fixed header, ``g``, then the data -- for another process or machine."""

    _HEAD = struct.Struct("<8sQQqqBQdIQ")      # magic, tag, key, position, length, has rng, seed, noise_scale, len(g), len(data)
    _MAGIC = b"QVCSNAP1"

    def __init__(self, tag: int, data: torch.Tensor, g: torch.Tensor, key: int, position: int, length: int,
                 rng: Optional[Tuple[int, float]] = None):
        self.tag, self.data, self.g, self.key = int(tag), data, g, int(key) & 0xFFFFFFFFFFFFFFFF
        self.position, self.length = int(position), int(length)
        self.rng = None if rng is None else (int(rng[0]), float(rng[1]))

    def to(self, device) -> "StreamSnapshot":
        """The same snapshot with ``data`` and ``g`` on ``device`` (device data is 256-byte aligned, as an import needs)."""
        device = torch.device(device)
        if device.type == "cpu":
            data = self.data.cpu()
        else:
            from .engine import aligned_empty
            data = aligned_empty(self.data.numel(), device)
            data.copy_(self.data)
        return StreamSnapshot(self.tag, data, self.g.to(device), self.key, self.position, self.length, self.rng)

    def cpu(self) -> "StreamSnapshot":
        return self.to("cpu")

    def tobytes(self) -> bytes:
        g = self.g.detach().to("cpu", torch.float32).contiguous().reshape(-1)
        data = self.data.detach().cpu().contiguous().reshape(-1)
        seed, scale = self.rng if self.rng is not None else (0, 0.0)
        head = self._HEAD.pack(self._MAGIC, self.tag, self.key, self.position, self.length, self.rng is not None,
                               seed & 0xFFFFFFFFFFFFFFFF, scale, g.numel(), data.numel())
        return head + g.numpy().tobytes() + data.numpy().tobytes()

    @classmethod
    def frombytes(cls, raw: bytes) -> "StreamSnapshot":
        """The host snapshot ``tobytes`` wrote; ValueError for anything else."""
        n = cls._HEAD.size
        if len(raw) < n or raw[:8] != cls._MAGIC:
            raise ValueError("not a StreamSnapshot byte string")
        _magic, tag, key, position, length, has_rng, seed, scale, n_g, n_data = cls._HEAD.unpack(raw[:n])
        if len(raw) != n + 4 * n_g + n_data:
            raise ValueError(f"StreamSnapshot byte string of {len(raw)} bytes, its header says {n + 4 * n_g + n_data}")
        g = torch.frombuffer(bytearray(raw[n:n + 4 * n_g]), dtype=torch.float32) if n_g else torch.zeros(0)
        data = torch.frombuffer(bytearray(raw[n + 4 * n_g:]), dtype=torch.uint8) if n_data else torch.zeros(0, dtype=torch.uint8)
        return cls(tag, data, g, key, position, length, (seed, scale) if has_rng else None)


class StreamConverter:
    """Incremental conversion of ``streams`` concurrent streams, ``hop_frames`` new unit frames per step
    (qvc_stream_step; BASELINE.json configs[4]).  Unlike ChunkedConverter it needs nothing but the frames seen so
    far: the state (ring buffers at five points of the path, csrc/qvc_stream.h) lives in a tensor owned by this
    object, every step is ONE replay of a captured hipGraph (fixed shapes; the stream position is a device
    counter the graph itself advances), and a frame costs about (2*H + hop)/hop of its offline cost per segment
    instead of (2*88 + hop)/hop.  Output lags the input by ``self.lag`` frames -- the look-ahead the non-causal
    network needs; it is exact, including the first and last frames of a stream.

    The noise comes either as a tensor per step (``step(unit_new, noise_new)``, aligned by ``noise_lag``) or from the
    library's counter-based generator (``seed``: ``step(unit_new)`` alone; every slot draws from the key given to
    ``start`` / ``convert`` at the stream's absolute frames, so a streamed utterance equals its offline conversion under
    the same (seed, key) with nothing to align)."""

    def __init__(self, model, streams: int, hop_frames: int = 320, use_graph: bool = True, seed: Optional[int] = None,
                 noise_scale: float = 1.0):
        from .engine import aligned_empty
        self.model, self.streams, self.hop = model, int(streams), int(hop_frames)
        self.engine = model.engine()
        dev = self.engine.device
        mc = model.model_config
        n_state, n_ws = self._sizes()
        self.spf = model.samples_per_frame
        self._state = aligned_empty(n_state, dev)
        self._ws = aligned_empty(n_ws, dev)
        S, h = self.streams, self.hop
        self._unit = torch.zeros(S, mc.get("unit_channels", 256), h, device=dev)
        self._noise = torch.zeros(S, mc["inter_channels"], h, device=dev)
        self._g = torch.zeros(S, mc["gin_channels"], device=dev)
        self._out = torch.zeros(S, h * self.spf, device=dev)
        self._pos = torch.zeros(S, dtype=torch.int32, device=dev)
        self._len = torch.full((S,), 2 ** 30, dtype=torch.int32, device=dev)
        self._stream = torch.cuda.Stream(dev)
        self._graph = None
        self._pos_host = [0] * S
        self._len_host = [2 ** 30] * S
        self._keys = torch.zeros(S, dtype=torch.int64, device=dev)   # generator key per slot (read by the step as uint64)
        self._keys_host = [0] * S                                # host mirror of the keys (a snapshot carries its slot's)
        self._use_graph = use_graph
        self._rng = None                                         # (seed, noise_scale) of the generator form, once asked for
        self._rng_graph = None
        self.reset()
        if use_graph:
            with torch.cuda.stream(self._stream):
                self._one_step()                                  # warm-up (code objects)
                self._stream.synchronize()
                self._graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph, stream=self._stream):
                    self._one_step()
            self.reset()
        if seed is not None:
            self.set_seed(seed, noise_scale)

    # the three calls that differ between the segment rings and LiveConverter's window
    def _sizes(self):
        n_state, n_ws, self.lag, self.noise_lag = self.engine.stream_sizes(self.streams, self.hop)
        return n_state, n_ws

    def _engine_step(self, noise, rng) -> None:
        self.engine.stream_step(self._state, self._ws, self._unit, self._g, noise, self._out, self._pos, self._len, rng=rng)

    def _engine_reset_slot(self, slot: int, length: int) -> None:
        self.engine.stream_reset_slot(self._state, self.streams, self.hop, slot, length, self._pos, self._len)

    def _one_step(self, rng: bool = False):
        if rng:
            self._engine_step(None, (self._rng[0], self._keys, self._rng[1]))
        else:
            self._engine_step(self._noise, None)
        self._pos.add_(self.hop)                                 # inside the graph: the position advances with every replay

    def set_seed(self, seed: int, noise_scale: float = 1.0) -> None:
        """Choose the generator form's seed and noise_scale.  They are baked into the captured step, so a new pair means
        a warm-up step and a new capture: ALL slots are reset.  The same pair again is free."""
        if self._rng == (int(seed), float(noise_scale)):
            return
        self._rng = (int(seed), float(noise_scale))
        self._rng_graph = None
        if self._use_graph:
            with torch.cuda.stream(self._stream):
                self._one_step(rng=True)                          # warm-up (code objects)
                self._stream.synchronize()
                self._rng_graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._rng_graph, stream=self._stream):
                    self._one_step(rng=True)
        self.reset()

    def _after_caller(self, *tensors) -> None:
        """Order the side stream after the caller's current stream (inputs such as a freshly computed ``g`` may still be
        pending there) and keep device inputs alive until the side stream is done with them."""
        dev = self.engine.device
        self._stream.wait_stream(torch.cuda.current_stream(dev))
        for t in tensors:
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(self._stream)

    def reset(self, g: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None) -> None:
        """Start new streams in ALL slots: zero state, position 0; ``g`` (S, gin) speaker embeddings; ``lengths`` (S,) if known."""
        self._after_caller(g, lengths)
        with torch.cuda.stream(self._stream):
            self._state.zero_()
            self._pos.zero_()
            self._len.fill_(2 ** 30)
            if g is not None:
                self._g.copy_(g.reshape(self.streams, -1))
            if lengths is not None:
                self._len.copy_(torch.as_tensor(lengths, dtype=torch.int32))
        self._stream.synchronize()
        self._pos_host = [0] * self.streams
        self._len_host = [2 ** 30] * self.streams if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]

    def end(self, lengths) -> None:
        """Tell the converter where ALL streams end (frames); keep stepping until ``position - lag >= length`` to flush."""
        self._after_caller(lengths)
        with torch.cuda.stream(self._stream):
            self._len.copy_(torch.as_tensor(lengths, dtype=torch.int32))
        self._len_host = [int(v) for v in torch.as_tensor(lengths).tolist()]

    # ---- per-slot lifecycle: streams of a server start and end at different times
    def start(self, slot: int, g: torch.Tensor, length: Optional[int] = None, key: Optional[int] = None) -> None:
        """Admit a new stream into ``slot``: that slot's ring rows are zeroed and its position goes back to 0 on the
        device (qvc_stream_reset_slot); the other slots keep running and the captured graph is unchanged.  ``g`` (gin,)
        or (1, gin): the stream's speaker embedding; ``length``: its frame count if already known; ``key``: the
        stream's generator key (the slot keeps its previous one if None)."""
        if not 0 <= slot < self.streams:
            raise ValueError(f"slot {slot} outside [0, {self.streams})")
        n = 2 ** 30 if length is None else int(length)
        self._after_caller(g)
        with torch.cuda.stream(self._stream):
            self._engine_reset_slot(slot, n)
            self._g[slot].copy_(g.reshape(-1), non_blocking=True)
            if key is not None:
                k = int(key) & 0xFFFFFFFFFFFFFFFF
                self._keys[slot:slot + 1].fill_(k - (1 << 64) if k >> 63 else k)
                self._keys_host[slot] = k
        self._pos_host[slot] = 0
        self._len_host[slot] = n

    def end_slot(self, slot: int, length: int) -> None:
        """The stream in ``slot`` ends after ``length`` frames; it is flushed once ``finished(slot)``."""
        with torch.cuda.stream(self._stream):
            self._len[slot:slot + 1].fill_(int(length))
        self._len_host[slot] = int(length)

    # ---- slot snapshots: a running stream moves between slots, converters, batch sizes, hops and processes
    def _check_slot(self, slot: int) -> int:
        if not 0 <= int(slot) < self.streams:
            raise ValueError(f"slot {slot} outside [0, {self.streams})")
        return int(slot)

    def snapshot_tag(self) -> int:
        """The layout fingerprint of this converter's snapshots (the model's: no batch, no hop in it)."""
        return self.engine.stream_snapshot_tag()

    def _check_origin(self, tag: int, rng) -> None:
        """What import_slot / move_slots refuse, before anything is launched: a snapshot of another layout, or one drawn
        from the generator under another (seed, noise_scale)."""
        if tag != self.snapshot_tag():
            raise ValueError(f"snapshot tag {tag:#018x} is not this model's ({self.snapshot_tag():#018x}): another geometry or operand type")
        if rng is not None and rng != self._rng:
            raise ValueError(f"the snapshot draws its noise from the generator under (seed, noise_scale) = {rng}, this converter under {self._rng}")

    def export_slot(self, slot: int) -> StreamSnapshot:
        """The stream in ``slot`` as it stands between two calls (qvc_stream_export_slots on the side stream; the slot is
        only read and keeps running).  Nothing synchronises: position, length and key come from the host mirrors."""
        from .engine import aligned_empty
        slot = self._check_slot(slot)
        dev = self.engine.device
        with torch.cuda.stream(self._stream):
            data = aligned_empty(self.engine.stream_snapshot_bytes(), dev)
            self.engine.stream_export_slots(self._state, self.streams, self.hop, [slot], self._pos, self._len, data)
            g = self._g[slot].clone()
        cur = torch.cuda.current_stream(dev)
        cur.wait_stream(self._stream)
        data.record_stream(cur)
        g.record_stream(cur)
        return StreamSnapshot(self.snapshot_tag(), data, g, self._keys_host[slot], self._pos_host[slot], self._len_host[slot], self._rng)

    def import_slot(self, slot: int, snap: StreamSnapshot) -> None:
        """Continue the stream of ``snap`` in ``slot``: the kept frames of every ring, the position and the length
        (qvc_stream_import_slots), ``g[slot]``, the slot's generator key and the host mirrors.  The other slots and the
        captured graph are untouched.  ValueError -- before anything is launched -- when the snapshot's layout tag is not
        this model's, or when it was drawn from the generator under a (seed, noise_scale) other than this converter's."""
        from .engine import aligned_empty
        slot = self._check_slot(slot)
        self._check_origin(snap.tag, snap.rng)
        n = self.engine.stream_snapshot_bytes()
        if snap.data.numel() != n or snap.data.dtype != torch.uint8 or snap.g.numel() != self._g.shape[1]:
            raise ValueError(f"a snapshot of this model is {n} bytes with a g of {self._g.shape[1]}, got {snap.data.numel()} and {snap.g.numel()}")
        dev = self.engine.device
        self._after_caller(snap.data, snap.g)
        with torch.cuda.stream(self._stream):
            data = snap.data
            if data.device != dev or data.data_ptr() % 256 or not data.is_contiguous():
                data = aligned_empty(n, dev)
                data.copy_(snap.data, non_blocking=True)
            self.engine.stream_import_slots(self._state, self.streams, self.hop, [slot], self._pos, self._len, data)
            self._g[slot].copy_(snap.g.reshape(-1), non_blocking=True)
            self._keys[slot:slot + 1].fill_(snap.key - (1 << 64) if snap.key >> 63 else snap.key)
        self._keys_host[slot] = snap.key
        self._pos_host[slot], self._len_host[slot] = snap.position, snap.length

    def free_slot(self, slot: int) -> None:
        """Leave ``slot`` idle: zeroed rows, position 0, length 0 -- an empty stream, whose rows of the output are zeros."""
        slot = self._check_slot(slot)
        self._after_caller()
        with torch.cuda.stream(self._stream):
            self._engine_reset_slot(slot, 0)
        self._pos_host[slot], self._len_host[slot] = 0, 0

    def occupied(self, slot: int) -> bool:
        """``slot`` carries a stream that still has output to come (a slot no stream was ever admitted into counts: its
        length is unknown; ``free_slot`` or ``end_slot(slot, 0)`` says otherwise)."""
        return self._len_host[slot] > 0 and not self.finished(slot)

    def move_slots(self, slots, dst: "StreamConverter", dst_slots) -> None:
        """Move the streams in ``slots`` into ``dst_slots`` of ``dst`` -- this converter or another one of the same model, of
        any batch size and hop -- in ONE export and ONE import call, and leave the slots they came from idle
        (``free_slot``).  Feed the streams into ``dst`` from the next call on.  The snapshots stay on the device; the two
        side streams are ordered by ``wait_stream``.  ValueError, before anything is launched, as ``import_slot``."""
        from .engine import aligned_empty
        slots, dst_slots = [self._check_slot(s) for s in slots], [dst._check_slot(s) for s in dst_slots]
        if len(slots) != len(dst_slots) or len(set(slots)) != len(slots) or len(set(dst_slots)) != len(dst_slots):
            raise ValueError(f"move_slots needs as many distinct destination slots as distinct source slots, got {slots} -> {dst_slots}")
        dst._check_origin(self.snapshot_tag(), self._rng)
        if not slots or (dst is self and slots == dst_slots):
            return
        dev = self.engine.device
        if dst.engine.device != dev:
            raise ValueError("move_slots stays on one device: between devices use export_slot, StreamSnapshot.to and import_slot")
        with torch.cuda.stream(self._stream):
            data = aligned_empty(len(slots) * self.engine.stream_snapshot_bytes(), dev)
            self.engine.stream_export_slots(self._state, self.streams, self.hop, slots, self._pos, self._len, data)
            g, keys = self._g[slots], self._keys[slots]                     # copies: a move inside one converter may overlap
        if dst is not self:
            dst._stream.wait_stream(self._stream)
            for t in (data, g, keys):
                t.record_stream(dst._stream)
        with torch.cuda.stream(dst._stream):
            dst.engine.stream_import_slots(dst._state, dst.streams, dst.hop, dst_slots, dst._pos, dst._len, data)
            dst._g[dst_slots] = g
            dst._keys[dst_slots] = keys
        moved = [(self._keys_host[s], self._pos_host[s], self._len_host[s]) for s in slots]
        for s, (key, position, length) in zip(dst_slots, moved):
            dst._keys_host[s], dst._pos_host[s], dst._len_host[s] = key, position, length
        for s in slots:
            if dst is not self or s not in dst_slots:
                self.free_slot(s)

    def move_slot(self, slot: int, dst: "StreamConverter", dst_slot: int) -> None:
        """``move_slots`` for one stream."""
        self.move_slots([slot], dst, [dst_slot])

    def rebuilt(self, streams: Optional[int] = None, hop_frames: Optional[int] = None) -> "StreamConverter":
        """A new converter of the same class, model, seed and graph setting with ``streams`` slots and ``hop_frames`` per
        call (default: this converter's); every occupied slot is carried over into the same slot number, the others are
        idle.  The elastic batch and the change of hop: the streams go on where they were, nothing is cut.  ValueError
        if ``streams`` is too small for the occupied slots."""
        streams = self.streams if streams is None else int(streams)
        carried = [s for s in range(self.streams) if self.occupied(s)]
        if carried and carried[-1] >= streams:
            raise ValueError(f"slot {carried[-1]} carries a stream: {streams} slots are too few")
        seed, scale = self._rng if self._rng is not None else (None, 1.0)
        new = type(self)(self.model, streams, self.hop if hop_frames is None else int(hop_frames), use_graph=self._use_graph, seed=seed,
                         noise_scale=scale)
        self.move_slots(carried, new, carried)
        for s in range(min(streams, self.streams)):
            if s not in carried:
                new.free_slot(s)
        return new

    def position(self, slot: int) -> int:
        """First frame the NEXT step feeds into ``slot`` (host mirror of the device counter)."""
        return self._pos_host[slot]

    def finished(self, slot: int) -> bool:
        """Every output frame of the stream in ``slot`` has been produced: the slot can take a new stream."""
        return self._pos_host[slot] - self.lag >= self._len_host[slot]

    @torch.no_grad()
    def step(self, unit_new: torch.Tensor, noise_new: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Feed frames [pos, pos+hop) of every stream (unit_new (S, 256, hop)) and the noise for frames
        [pos - noise_lag, ... + hop) (noise_new (S, inter, hop)); returns the waveform of frames
        [pos - lag, pos - lag + hop) as (S, hop * samples_per_frame) -- zeros where that lies outside the stream.
        ``noise_new=None``: the generator form (needs a seed: the constructor's, ``set_seed`` or ``convert(seed=...)``)."""
        if noise_new is None and self._rng is None:
            raise ValueError("step() without noise_new needs a seed (StreamConverter(seed=...) or set_seed)")
        out = self._issue(unit_new, noise_new)
        self._pos_host = [p + self.hop for p in self._pos_host]
        return out

    def _issue(self, unit_new: torch.Tensor, noise_new: Optional[torch.Tensor], counts: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One step / tick on the side stream, ordered after the caller's stream and in front of its next work: the inputs
        (``counts``: a tick's, into ``self._n``) copied in, the captured graph replayed (or the call issued directly), a
        copy of the output."""
        dev = self.engine.device
        self._stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self._stream):
            self._unit.copy_(unit_new, non_blocking=True)
            if noise_new is not None:
                self._noise.copy_(noise_new, non_blocking=True)
            if counts is not None:
                self._n.copy_(counts)
            graph = self._graph if noise_new is not None else self._rng_graph
            if graph is not None:
                graph.replay()
            else:
                self._one_step(rng=noise_new is None)
            out = self._out.clone()
        torch.cuda.current_stream(dev).wait_stream(self._stream)
        return out

    @torch.no_grad()
    def convert(self, unit: torch.Tensor, g: torch.Tensor, noise: Optional[torch.Tensor] = None,
                lengths: Optional[torch.Tensor] = None, seed: Optional[int] = None, keys=None) -> torch.Tensor:
        """Convenience: stream whole utterances through the step interface.  unit (S, 256, T), g (S, gin),
        noise (S, inter, T) -> (S, 1, T * samples_per_frame); equals infer_batch on the whole thing.  ``lengths`` (S,):
        streams that end before T (their rows are zero after the end, as with infer_batch_ragged).
        ``seed`` / ``keys`` (S integers, default 0 .. S-1) instead of ``noise``: the generator form -- equals
        ``infer_batch_ragged(..., rng=(seed, keys, noise_scale))``; the noise_scale is the constructor's / ``set_seed``'s."""
        S, UC, T = unit.shape
        if S != self.streams:
            raise ValueError(f"built for {self.streams} streams, got {S}")
        if seed is not None and noise is not None:
            raise ValueError("pass noise or seed, not both")
        dev = self.engine.device
        inter = self.model.model_config["inter_channels"]
        use_rng = seed is not None
        if use_rng:
            self.set_seed(seed, self._rng[1] if self._rng else 1.0)
        elif noise is None:
            noise = torch.randn(S, inter, T, device=dev)
        unit = unit.to(dev, torch.float32)
        h, lag, nl, spf = self.hop, self.lag, self.noise_lag, self.spf
        self.reset(g.to(dev, torch.float32), torch.full((S,), T, dtype=torch.int32) if lengths is None else lengths)
        out = torch.zeros(S, 1, T * spf, device=dev)
        pad_u = torch.nn.functional.pad(unit, (0, h + lag))                      # frames past the end: ignored by the kernels
        if use_rng:
            u64 = [int(k) & 0xFFFFFFFFFFFFFFFF for k in (range(S) if keys is None else keys)]
            if len(u64) != S:
                raise ValueError(f"{S} streams need {S} keys, got {len(u64)}")
            with torch.cuda.stream(self._stream):
                self._keys.copy_(torch.tensor([k - (1 << 64) if k >> 63 else k for k in u64], dtype=torch.int64))
            self._keys_host = list(u64)
        else:
            pad_n = torch.nn.functional.pad(noise.to(dev, torch.float32), (nl, h + lag))   # frame f of the noise sits at column f + nl
        steps = -(-(T + lag) // h)
        for n in range(steps):
            s = n * h
            chunk = self.step(pad_u[:, :, s:s + h], None if use_rng else pad_n[:, :, s:s + h])   # noise frames [s - nl, s - nl + h)
            f0 = s - lag
            lo, hi = max(f0, 0), min(f0 + h, T)
            if hi > lo:
                out[:, 0, lo * spf:hi * spf] = chunk[:, (lo - f0) * spf:(hi - f0) * spf]
        torch.cuda.synchronize(dev)
        return out


class _Ticks:
    """What the two tick converters share, in front of their lockstep converter in the bases: the count tensor, the draw
    selection of the captured call, ``tick`` and ``step``.  Per class: ``_engine_tick``, the one engine call."""

    def _count_tensor(self) -> torch.Tensor:
        """The counts of the tick in flight (the captured call holds this tensor's pointer); zeros: the warm-up and capture
        ticks of the constructor move nothing."""
        return torch.zeros(self.streams, dtype=torch.int32, device=self.engine.device)

    def _one_step(self, rng: bool = False):
        noise, draw = (None, (self._rng[0], self._keys, self._rng[1])) if rng else (self._noise, None)
        self._engine_tick(noise, draw)                           # advances self._pos itself

    @torch.no_grad()
    def tick(self, unit_new: torch.Tensor, n_new, noise_new: Optional[torch.Tensor] = None):
        """unit_new (S, 256, hop): columns [0, n_new[b]) of row b are frames [pos, pos + n_new[b]) of slot b, the rest is
        never read; ``n_new``: a sequence of ints or a CPU int32 tensor of length S (clamped to [0, hop] on the device);
        ``noise_new`` (S, inter, hop): the draw for frames [pos - noise_lag, ... + n_new[b]) -- the same frames where
        ``noise_lag`` is 0 --, or None for the generator form.
        -> (out, n): out (S, hop * samples_per_frame) with row b valid in [:n[b] * samples_per_frame] -- frames
        [pos - lag, pos - lag + n[b]) -- and zero behind it, n the clamped counts."""
        if noise_new is None and self._rng is None:
            raise ValueError(f"tick() without noise_new needs a seed ({type(self).__name__}(seed=...) or set_seed)")
        counts = torch.as_tensor(n_new, dtype=torch.int32, device="cpu").reshape(-1)
        if counts.numel() != self.streams:
            raise ValueError(f"{self.streams} slots need {self.streams} counts, got {counts.numel()}")
        out = self._issue(unit_new, noise_new, counts)
        n = [min(max(int(v), 0), self.hop) for v in counts.tolist()]
        self._pos_host = [p + k for p, k in zip(self._pos_host, n)]     # the host mirror follows the device
        return out, n

    @torch.no_grad()
    def step(self, unit_new: torch.Tensor, noise_new: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The tick in which every slot brings ``hop`` frames (the lockstep converter's ``step``: its contract and bits)."""
        return self.tick(unit_new, [self.hop] * self.streams, noise_new)[0]


class StreamTickConverter(_Ticks, StreamConverter):
    """StreamConverter for streams that tick on their own (qvc_stream_tick): per call, slot ``b`` brings ``n_new[b]``
    frames, ``0 <= n_new[b] <= hop_frames`` -- nothing when its packet is late, several packets when it catches up, a
    short last chunk.  ``hop_frames`` is the MOST a slot may bring per tick; it sizes the buffers.  StreamConverter's
    lifecycle, lag and noise lag, and one graph replay per tick: the counts travel in a device tensor the captured call
    reads, the positions advance on the device by the clamped counts and the host mirror follows them.  A slot that
    brings nothing leaves no trace.  The segment rings are exact, so a stream's concatenated output is its
    whole-utterance conversion however it was cut into ticks.  ``step`` is the tick in which every slot brings
    ``hop_frames`` frames: bit for bit StreamConverter's."""

    def _sizes(self):
        n_state, n_ws, self.lag, self.noise_lag = self.engine.stream_tick_sizes(self.streams, self.hop)
        self._n = self._count_tensor()
        return n_state, n_ws

    def _engine_tick(self, noise, rng) -> None:
        self.engine.stream_tick(self._state, self._ws, self._unit, self._g, noise, self._out, self._n, self._pos, self._len, rng=rng)


class LiveConverter(StreamConverter):
    """Streaming with a bounded look-ahead, for EVERY decoder (qvc_live_step).  StreamConverter's surface -- ``start`` /
    ``end_slot`` / ``finished`` / ``position`` / ``reset`` / ``end`` / ``set_seed`` / ``step`` / ``convert``, one graph
    replay per step, the position a device counter the graph advances -- with the lag chosen by the caller:
    ``lag == look_ahead`` frames, ``0 <= look_ahead <= context``.  Each stream keeps ONE ring of its last
    ``window = context + look_ahead + hop`` unit frames; a step runs the whole path over that window and returns frames
    [pos - look_ahead, pos - look_ahead + hop) of the OFFLINE conversion of the stream's prefix [0, min(length, pos + hop))
    -- the result is defined exactly, whatever the look-ahead.  ``look_ahead == context`` is exact streaming: the
    concatenated outputs equal the whole-utterance conversion, also for the single-band decoder and decoders with one
    up-sampler, which StreamConverter refuses.  A frame costs ``window / hop`` of its offline cost.  Between steps the
    ring keeps its last ``window - hop`` frames left-aligned -- the layout TickConverter keeps too, so the state is shared.
    The noise tensor of ``step(unit_new, noise_new)`` is for the frames of ``unit_new`` (``noise_lag == 0``)."""

    def __init__(self, model, streams: int, hop_frames: int, look_ahead: int, use_graph: bool = True, seed: Optional[int] = None,
                 noise_scale: float = 1.0):
        self.look_ahead = int(look_ahead)
        super().__init__(model, streams, hop_frames, use_graph=use_graph, seed=seed, noise_scale=noise_scale)

    def _sizes(self):
        n_state, n_ws, self.context = self.engine.live_sizes(self.streams, self.hop, self.look_ahead)
        self.window = self.context + self.look_ahead + self.hop
        self.lag, self.noise_lag = self.look_ahead, 0
        return n_state, n_ws

    def _engine_step(self, noise, rng) -> None:
        self.engine.live_step(self._state, self._ws, self._unit, self._g, noise, self._out, self._pos, self._len, self.look_ahead, rng=rng)

    def _engine_reset_slot(self, slot: int, length: int) -> None:
        self.engine.live_reset_slot(self._state, self.streams, self.hop, self.look_ahead, slot, length, self._pos, self._len)

    # the window's state is the caller's own last context + look_ahead input frames: there is nothing computed to carry
    def _no_snapshots(self, *_args, **_kw):
        raise ValueError(f"{type(self).__name__} has no slot snapshots: its state is not covered, it is the caller's last C + L input frames "
                         "(context + look_ahead), which the caller can feed again; snapshots cover the segment rings "
                         "(StreamConverter, StreamTickConverter)")

    export_slot = import_slot = move_slot = move_slots = rebuilt = snapshot_tag = _no_snapshots


class TickConverter(_Ticks, LiveConverter):
    """LiveConverter for streams that tick on their own (qvc_live_tick): per call, slot ``b`` brings ``n_new[b]`` frames,
    ``0 <= n_new[b] <= hop_frames`` -- nothing when its packet is late, several packets when it catches up, a short last
    chunk.  ``hop_frames`` is the MOST a slot may bring per tick; it sizes the buffers and the window
    ``context + look_ahead + hop_frames``.  LiveConverter's lifecycle (``start`` / ``end_slot`` / ``finished`` /
    ``position`` / ``reset`` / ``end`` / ``set_seed``) and one graph replay per tick; the counts travel in a device
    tensor the captured call reads, the positions advance on the device by the clamped counts and the host mirror
    follows them.  A slot that brings nothing leaves no trace: its ring, its position and the other slots' outputs are
    what they would have been without it.  The state is LiveConverter's, ring layout included (qvc_live_step and
    qvc_live_tick may alternate on one state); only the workspace is larger.

    ``tick`` returns frames [pos - look_ahead, pos - look_ahead + n) of the offline conversion of the prefix
    [0, min(length, pos + n)).  With ``look_ahead == context`` the concatenated output is the whole-utterance conversion
    however the stream was cut into ticks; with less, a frame sees between ``look_ahead`` and ``look_ahead + n - 1``
    frames of look-ahead, so the output depends on the cut.  ``step`` is the tick in which every slot brings
    ``hop_frames`` frames: bit for bit LiveConverter's."""

    def _sizes(self):
        n_state, n_ws, self.context = self.engine.live_tick_sizes(self.streams, self.hop, self.look_ahead)
        self.window = self.context + self.look_ahead + self.hop
        self.lag, self.noise_lag = self.look_ahead, 0
        self._n = self._count_tensor()
        return n_state, n_ws

    def _engine_tick(self, noise, rng) -> None:
        self.engine.live_tick(self._state, self._ws, self._unit, self._g, noise, self._out, self._n, self._pos, self._len, self.look_ahead, rng=rng)

    def _engine_reset_slot(self, slot: int, length: int) -> None:
        self.engine.live_tick_reset_slot(self._state, self.streams, self.hop, self.look_ahead, slot, length, self._pos, self._len)
