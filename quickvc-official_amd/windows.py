"""Recordings of any length: exact windows over packed utterances (include/qvc.h: qvc_infer_windows_fm / _rng_fm).

Every other offline entry point sizes its buffers by ``rows x longest utterance``, so one hour-long recording makes a
batch unallocatable.  Here the rows of a call are WINDOWS of ``window_frames`` delivered frames (plus the path's
receptive field on either side), cut from utterances of any lengths that lie back to back in one packed buffer and
named by a table on the device: memory is ``rows x window`` whatever the lengths, one long recording converts at batch
rate, and every row has its own speaker row (a target speaker per region).  A window's delivered frames are the frames
of the whole-utterance conversion (``infer_ragged`` with the same g and the same noise or (seed, key)).

``plan_windows`` cuts the utterances, ``WindowConverter`` owns the buffers and ONE captured graph that is replayed per
``rows``-sized group of the plan.  ``streaming.ChunkedConverter`` stays what it is: equal-length streams, one window per
stream per replay.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch


def plan_windows(lengths: Sequence[int], window_frames: int) -> List[Tuple[int, int, int]]:
    """Rows ``(utterance, start, count)`` that cover every frame of every utterance exactly once, utterance by utterance:
    windows of ``window_frames`` frames and a shorter last one."""
    n = int(window_frames)
    if n < 1:
        raise ValueError(f"window_frames must be at least 1, got {window_frames}")
    return [(u, s, min(n, int(length) - s)) for u, length in enumerate(lengths) for s in range(0, int(length), n)]


class WindowConverter:
    """Graph-replayed conversion of utterances of ANY lengths in groups of ``rows`` windows of ``window_frames`` frames.

    The noise is the library's counter-based generator when ``seed`` is given (``convert(..., keys=)``: one key per
    utterance, default its index -- the waveform then equals ``infer_ragged(..., seed=, keys=)`` of the utterance), else
    a tensor per call (``convert(..., noise=)``, drawn with ``torch.randn`` when omitted)."""

    def __init__(self, model, rows: int, window_frames: int, seed: Optional[int] = None, noise_scale: float = 1.0, use_graph: bool = True):
        from .engine import aligned_empty
        self.model, self.rows, self.n = model, int(rows), int(window_frames)
        self.engine = model.engine()
        dev = self.engine.device
        mc = model.model_config
        n_ws, self.context = self.engine.windows_sizes(self.rows, self.n)
        self.workspace_bytes = n_ws
        self.spf = model.samples_per_frame
        self.seed, self.noise_scale = seed, float(noise_scale)
        self._uc, self._inter = mc.get("unit_channels", 256), mc["inter_channels"]
        self._ws = aligned_empty(n_ws, dev)
        self._table = torch.zeros(self.rows, 4, dtype=torch.int32, device=dev)      # all rows idle
        self._g = torch.zeros(self.rows, mc["gin_channels"], device=dev)
        self._keys = torch.zeros(self.rows, dtype=torch.int64, device=dev)
        self._stream = torch.cuda.Stream(dev)
        self._use_graph = use_graph
        self._cap = 0
        self._unit = self._out = self._noise = None
        self._graphs = {}

    def _call(self, rng: bool) -> None:
        self.engine.infer_windows(self._ws, self._unit, None if rng else self._noise, self._table, self._g, self._out, self.n,
                                  rng=(self.seed, self._keys, self.noise_scale) if rng else None)

    def _ensure(self, total: int, rng: bool) -> None:
        """Packed buffers of at least ``total`` frames (a captured graph holds their pointers and their size: growing
        them drops the graphs) and, with use_graph, the graph of this form -- captured over a table of idle rows."""
        dev = self.engine.device
        if total > self._cap:
            self._cap = total
            self._unit = torch.zeros(total, self._uc, device=dev)
            self._out = torch.zeros(total * self.spf, device=dev)
            self._noise = None
            self._graphs = {}
        if not rng and self._noise is None:
            self._noise = torch.zeros(self._inter, self._cap, device=dev)
        if self._use_graph and rng not in self._graphs:
            self._table.zero_()
            self._call(rng)                                    # warm-up (code objects)
            self._stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=self._stream):
                self._call(rng)
            self._graphs[rng] = graph

    @torch.no_grad()
    def convert(self, units, g: torch.Tensor, keys=None, noise=None, lengths=None):
        """``units``: a list of (frames, C) tensors -- the utterances as they are on disk -- or ONE packed (total, C)
        tensor with ``lengths``.  ``g``: (U, gin), one row per utterance, or (len(plan), gin), one per row of
        ``plan_windows(lengths, window_frames)`` (region targets).  ``keys``: U integers (generator form; default 0 .. U-1).
        ``noise``: a list of (inter, frames) tensors or one packed (inter, total) tensor (pointer form).
        -> a list of U fp32 waveforms (frames * samples_per_frame,) on the device."""
        dev = self.engine.device
        if torch.is_tensor(units):
            if lengths is None:
                raise ValueError("a packed units tensor needs lengths")
            lengths = [int(v) for v in lengths]
            packed = units
        else:
            lengths = [int(u.shape[0]) for u in units]
            packed = None
        U, total = len(lengths), sum(lengths)
        if U < 1 or min(lengths) < 1 or (packed is not None and int(packed.shape[0]) != total):
            raise ValueError(f"need at least one utterance of at least one frame each and units of sum(lengths) frames, got lengths {lengths}")
        rng = self.seed is not None
        if rng and noise is not None:
            raise ValueError("pass noise or build the converter with a seed, not both")
        plan = plan_windows(lengths, self.n)
        g = g.reshape(g.shape[0], -1)
        if g.shape[0] not in (U, len(plan)):
            raise ValueError(f"g needs one row per utterance ({U}) or per planned row ({len(plan)}), got {g.shape[0]}")
        keys = list(range(U)) if keys is None else [int(k) for k in keys]
        if len(keys) != U:
            raise ValueError(f"{U} utterances need {U} keys")
        base = [0] * U
        for u in range(1, U):
            base[u] = base[u - 1] + lengths[u - 1]
        groups = -(-len(plan) // self.rows)
        # the whole plan on the device up front, padded with idle rows: per group only device-to-device copies remain
        tab = torch.zeros(groups * self.rows, 4, dtype=torch.int32)
        tab[:len(plan)] = torch.tensor([[base[u], lengths[u], s, c] for u, s, c in plan], dtype=torch.int32)
        row_u = torch.tensor([u for u, _, _ in plan], dtype=torch.int64)
        key_rows = torch.zeros(groups * self.rows, dtype=torch.int64)
        key_rows[:len(plan)] = torch.tensor([k - (1 << 64) if (k & 0xFFFFFFFFFFFFFFFF) >> 63 else k & 0xFFFFFFFFFFFFFFFF
                                             for k in (keys[u] for u, _, _ in plan)], dtype=torch.int64)
        cur = torch.cuda.current_stream(dev)
        self._stream.wait_stream(cur)
        with torch.cuda.stream(self._stream):
            self._ensure(total, rng)
            tab, key_rows = tab.to(dev), key_rows.to(dev)
            g_dev = g.to(dev, torch.float32)
            g_rows = torch.zeros(groups * self.rows, g_dev.shape[1], device=dev)
            g_rows[:len(plan)] = g_dev if g_dev.shape[0] == len(plan) and len(plan) != U else g_dev.index_select(0, row_u.to(dev))
            if packed is not None:
                self._unit[:total].copy_(packed.to(dev, torch.float32))
            else:
                for u, x in enumerate(units):
                    self._unit[base[u]:base[u] + lengths[u]].copy_(x.to(dev, torch.float32))
            if not rng:
                if noise is None:
                    self._noise[:, :total].normal_()
                elif torch.is_tensor(noise):
                    self._noise[:, :total].copy_(noise.to(dev, torch.float32))
                else:
                    for u, x in enumerate(noise):
                        self._noise[:, base[u]:base[u] + lengths[u]].copy_(x.reshape(self._inter, -1).to(dev, torch.float32))
            for i in range(groups):
                lo, hi = i * self.rows, (i + 1) * self.rows
                self._table.copy_(tab[lo:hi])
                self._g.copy_(g_rows[lo:hi])
                self._keys.copy_(key_rows[lo:hi])
                if self._use_graph:
                    self._graphs[rng].replay()
                else:
                    self._call(rng)
            out = self._out[:total * self.spf].clone()
            self._stream.synchronize()
        cur.wait_stream(self._stream)
        return [out[base[u] * self.spf:(base[u] + lengths[u]) * self.spf] for u in range(U)]
