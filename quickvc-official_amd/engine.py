"""QvcEngine: owns the packed weights and workspace on one GPU and calls the C ABI.

PyTorch is used here for device memory and streams only; every FLOP of enc_p / flow / dec
runs inside libqvc_hip.so.  Buffers are PyTorch allocations handed over as raw pointers;
kernels are enqueued on ``torch.cuda.current_stream()`` so the call composes with PyTorch
work (the LSTM speaker encoder) and can be captured in a ``torch.cuda.CUDAGraph``.
"""
from __future__ import annotations

import ctypes
import functools
from typing import Dict, Optional

import torch

from . import lib as L


def aligned_empty(nbytes: int, device) -> torch.Tensor:
    return _aligned_empty(nbytes, device)


def _aligned_empty(nbytes: int, device) -> torch.Tensor:
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    shift = (-raw.data_ptr()) % 256
    return raw[shift:shift + nbytes]


def _on_device(fn):
    """Run a method with the engine's GPU as the current device: the library keys per-device state (the opt-in for
    more than 64 KiB of dynamic LDS) on hipGetDevice(), and a process may drive several GPUs."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        with torch.cuda.device(self.device):
            return fn(self, *args, **kwargs)
    return wrapper


class QvcEngine:
    def __init__(self, model_config: dict, state_dict: Optional[Dict[str, torch.Tensor]], device, parallel_branches: bool = False,
                 pack: bool = True):
        """``pack=False`` (multi-GPU start-up, ranks other than the one that owns the checkpoint): allocate the blob
        without packing anything -- ``state_dict`` may be None -- and let ``dist.broadcast_blob`` fill it."""
        self.lib = L.load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.QvcError("QvcEngine needs a HIP device (no CPU fallback)")
        with torch.cuda.device(self.device):
            L.check(self.lib, self.lib.qvc_device_check(), "qvc_device_check")
        self.model_config = dict(model_config)
        self.cfg = L.make_config(model_config)
        if pack:
            host_blob = L.pack_weights(self.lib, self.cfg, state_dict)
            self.blob = _aligned_empty(host_blob.numel(), self.device)
            self.blob.copy_(host_blob)
        else:
            n = int(self.lib.qvc_blob_bytes(ctypes.byref(self.cfg)))
            if n < 0:
                L.check(self.lib, n, "qvc_blob_bytes")
            self.blob = _aligned_empty(n, self.device)
            state_dict = state_dict or {}
        # optional fork/join resources: the three ResBlocks of a stage as parallel branches (two aux streams +
        # events).  Measured neutral on MI355X (2.934 vs 2.949 ms/step: each launch already fills the chip), and
        # concurrent kernels blur per-kernel profiles, so it is off by default.
        self._aux = ctypes.c_void_p(None)
        if parallel_branches:
            with torch.cuda.device(self.device):
                L.check(self.lib, self.lib.qvc_aux_create(ctypes.byref(self._aux)), "qvc_aux_create")
        self._ws: Optional[torch.Tensor] = None
        self._ws_key = None
        # speaker encoder: own blob, packed on first use from the same state dict
        self._spk_sd = {k: v for k, v in state_dict.items() if k.startswith("enc_spk.")}
        # posterior encoder: own blob too, packed on first use
        self._encq_sd = {k: v for k, v in state_dict.items() if k.startswith("enc_q.")}
        self._encq_blob: Optional[torch.Tensor] = None
        self._spk_blob: Optional[torch.Tensor] = None
        self._spk_ws: Optional[torch.Tensor] = None
        n = model_config["gen_istft_hop_size"] * model_config["subbands"]
        for u in model_config["upsample_rates"]:
            n *= u
        self.samples_per_frame = n

    def __del__(self):
        try:
            if getattr(self, "_aux", None) is not None and self._aux.value:
                self.lib.qvc_aux_destroy(self._aux)
                self._aux = ctypes.c_void_p(None)
        except Exception:
            pass

    # weights can also arrive from another rank (one broadcast at start-up)
    def load_blob_(self, blob: torch.Tensor) -> None:
        self.blob.copy_(blob)

    def _workspace_bytes(self, batch: int, frames: int, sources: Optional[int]) -> int:
        if sources is None:
            n, what = int(self.lib.qvc_workspace_bytes(ctypes.byref(self.cfg), batch, frames)), "qvc_workspace_bytes"
        else:
            n, what = int(self.lib.qvc_fanout_workspace_bytes(ctypes.byref(self.cfg), sources, batch, frames)), "qvc_fanout_workspace_bytes"
        if n < 0:
            L.check(self.lib, n, what)
        return n

    def alloc_workspace(self, batch: int, frames: int, sources: Optional[int] = None) -> torch.Tensor:
        """A private workspace for (batch, frames).  Anything that bakes workspace pointers into a captured graph
        must own the buffer it captured (the shared one below is replaced when a larger request arrives).
        ``sources``: the fan-out form -- ``batch`` output rows from ``sources`` encoded sources (infer_fanout_ragged);
        such a workspace also serves infer_batch_ragged at (batch, frames)."""
        return _aligned_empty(self._workspace_bytes(batch, frames, sources), self.device)

    def workspace(self, batch: int, frames: int, sources: Optional[int] = None) -> torch.Tensor:
        key = (batch, frames, sources)
        if self._ws is None or self._ws_key != key:
            n = self._workspace_bytes(batch, frames, sources)
            if self._ws is None or self._ws.numel() < n:
                self._ws = _aligned_empty(n, self.device)
            self._ws_key = key
        return self._ws

    @staticmethod
    def _f32(t: torch.Tensor, device) -> torch.Tensor:
        return t.to(device=device, dtype=torch.float32).contiguous()

    def _draw(self, noise, rng, rows: int, noise_shape):
        """The two ways to supply the N(0,1) draw: ``noise`` (a tensor of ``noise_shape``) or ``rng = (seed, keys, scale)``
        -- the counter-based generator of include/qvc.h, ``keys`` one integer per row (a sequence or an int64 tensor; on
        this device it is passed through untouched).  Exactly one of the two -> (noise tensor or None, descriptor or
        None, the tensors the descriptor points into)."""
        if (noise is None) == (rng is None):
            raise ValueError("pass exactly one of noise and rng=(seed, keys, scale)")
        if noise is not None:
            if tuple(noise.shape) != tuple(noise_shape):
                raise ValueError(f"noise must be {tuple(noise_shape)}, got {tuple(noise.shape)}")
            return self._f32(noise, self.device), None, None
        try:
            seed, keys, scale = rng
        except (TypeError, ValueError):
            raise ValueError("rng must be (seed, keys, scale)") from None
        if not torch.is_tensor(keys):
            u64 = [int(k) & 0xFFFFFFFFFFFFFFFF for k in keys]
            keys = torch.tensor([k - (1 << 64) if k >> 63 else k for k in u64], dtype=torch.int64)
        if keys.dtype != torch.int64 or tuple(keys.shape) != (rows,):
            raise ValueError(f"rng keys must be {rows} integers (int64), got {keys.dtype} {tuple(keys.shape)}")
        keys = keys.to(self.device).contiguous()       # the library reads them as uint64: the same 64 bits
        desc = L.QvcNoiseRng(int(seed) & 0xFFFFFFFFFFFFFFFF, keys.data_ptr(), float(scale))
        return None, desc, keys

    @_on_device
    def noise_fill(self, seed: int, keys, channels: int, frames: int, frame0: int = 0, scale: float = 1.0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """qvc_noise_fill: the generator's draw as a tensor -- (rows, channels, frames) fp32 for frames
        [frame0, frame0 + frames) of the rows' keys; fed to a ``noise=`` call it gives the bits of the ``rng=`` call."""
        rows = int(keys.shape[0]) if torch.is_tensor(keys) else len(keys)
        _, desc, keys_dev = self._draw(None, (seed, keys, scale), rows, None)
        if out is None:
            out = torch.empty(rows, channels, frames, dtype=torch.float32, device=self.device)
        st = self.lib.qvc_noise_fill(desc.seed, keys_dev.data_ptr(), desc.scale, rows, int(channels), int(frames), int(frame0),
                                     out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_noise_fill")
        return out

    @_on_device
    def infer_batch(self, unit: torch.Tensor, g: torch.Tensor, noise: torch.Tensor,
                    out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """unit (B,256,T), g (B,gin), noise (B,inter,T) -> (B,1,T*samples_per_frame) fp32.
        ``ws``: a caller-owned workspace from alloc_workspace(B, T) (graph owners); default = the shared one."""
        B, cu, T = unit.shape
        mc = self.model_config
        if cu != mc.get("unit_channels", 256) or g.shape != (B, mc["gin_channels"]) or \
                tuple(noise.shape) != (B, mc["inter_channels"], T):
            raise ValueError(f"bad input shapes: unit {tuple(unit.shape)}, g {tuple(g.shape)}, noise {tuple(noise.shape)}")
        unit, g, noise = (self._f32(t, self.device) for t in (unit, g, noise))
        if out is None:
            out = torch.empty(B, 1, T * self.samples_per_frame, dtype=torch.float32, device=self.device)
        if ws is None:
            ws = self.workspace(B, T)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        st = self.lib.qvc_infer_batch_ex(ctypes.byref(self.cfg), self.blob.data_ptr(), unit.data_ptr(), g.data_ptr(),
                                         noise.data_ptr(), out.data_ptr(), B, T, ws.data_ptr(), ws.numel(), stream,
                                         self._aux)
        L.check(self.lib, st, "qvc_infer_batch")
        return out

    @_on_device
    def infer_batch_ragged(self, unit: torch.Tensor, g: torch.Tensor, noise: Optional[torch.Tensor], frames: torch.Tensor,
                           out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                           unit_fm: bool = False, rng=None) -> torch.Tensor:
        """A batch of utterances of DIFFERENT lengths: unit (B,256,Tmax) / noise (B,inter,Tmax) padded (the padding's
        content is ignored), frames (B,) int32 lengths -> (B,1,Tmax*samples_per_frame); row b holds utterance b's
        waveform in its first frames[b]*samples_per_frame samples and zeros after.
        ``unit_fm``: unit is (B,Tmax,256) -- frame-major, as the reference's unit files are on disk
        (dataset/encode.py:38), so a batch read by fileio.IoPool.load_units uploads as it is.
        ``rng``: with ``noise=None``, ``(seed, keys, scale)`` -- the draw computed on the device from one key per row
        (qvc_infer_batch_ragged_rng): no noise tensor exists, and a row's result depends on its key alone."""
        mc = self.model_config
        if unit_fm:
            B, T, cu = unit.shape
        else:
            B, cu, T = unit.shape
        if cu != mc.get("unit_channels", 256) or g.shape != (B, mc["gin_channels"]) or tuple(frames.shape) != (B,):
            raise ValueError(f"bad input shapes: unit {tuple(unit.shape)}, g {tuple(g.shape)}, frames {tuple(frames.shape)}")
        noise, desc, keys_dev = self._draw(noise, rng, B, (B, mc["inter_channels"], T))
        if frames.device.type != "cuda":                       # host-side lengths can be validated for free
            if int(frames.min()) < 2 or int(frames.max()) > T:
                raise ValueError(f"frames must lie in [2, {T}], got [{int(frames.min())}, {int(frames.max())}]")
        unit, g = (self._f32(t, self.device) for t in (unit, g))
        lens = frames.to(device=self.device, dtype=torch.int32).contiguous()
        if out is None:
            out = torch.empty(B, 1, T * self.samples_per_frame, dtype=torch.float32, device=self.device)
        if ws is None:
            ws = self.workspace(B, T)
        if desc is None:
            fn = self.lib.qvc_infer_batch_ragged_fm if unit_fm else self.lib.qvc_infer_batch_ragged
            draw = noise.data_ptr()
        else:
            fn = self.lib.qvc_infer_batch_ragged_rng_fm if unit_fm else self.lib.qvc_infer_batch_ragged_rng
            draw = ctypes.byref(desc)
        st = fn(ctypes.byref(self.cfg), self.blob.data_ptr(), unit.data_ptr(), g.data_ptr(),
                draw, out.data_ptr(), B, T, lens.data_ptr(), ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_infer_batch_ragged")
        return out

    @_on_device
    def infer_fanout_ragged(self, unit: torch.Tensor, frames: torch.Tensor, src_of_row: torch.Tensor, g: torch.Tensor,
                            noise: Optional[torch.Tensor], out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                            unit_fm: bool = False, rng=None) -> torch.Tensor:
        """R output rows from U <= R distinct sources (one source listed once per target speaker): unit (U,256,Tmax)
        padded, frames (U,) int32 lengths, src_of_row (R,) int32 -- the source of every row --, g (R,gin), noise
        (R,inter,Tmax) -> (R,1,Tmax*samples_per_frame).  Row r equals row r of ``infer_batch_ragged`` on the expanded batch
        (unit[src_of_row], g, noise, frames[src_of_row]); enc_p runs once per source instead of once per row.
        Host tensors have their ranges checked; device tensors are passed through untouched (the library clamps them on
        the device and never reads them on the host, so the call can sit in a captured graph).
        ``ws``: a caller-owned workspace from alloc_workspace(R, Tmax, sources=U); ``unit_fm``: unit is (U,Tmax,256).
        ``rng``: with ``noise=None``, ``(seed, keys, scale)`` with one key per OUTPUT row (qvc_infer_fanout_ragged_rng)."""
        mc = self.model_config
        if unit_fm:
            U, T, cu = unit.shape
        else:
            U, cu, T = unit.shape
        R = int(src_of_row.shape[0]) if src_of_row.dim() == 1 else -1
        if cu != mc.get("unit_channels", 256) or tuple(frames.shape) != (U,) or R < U or g.shape != (R, mc["gin_channels"]):
            raise ValueError(f"bad input shapes: unit {tuple(unit.shape)}, frames {tuple(frames.shape)}, src_of_row {tuple(src_of_row.shape)}, "
                             f"g {tuple(g.shape)} (rows >= sources >= 1)")
        noise, desc, keys_dev = self._draw(noise, rng, R, (R, mc["inter_channels"], T))
        if frames.device.type != "cuda":                       # host-side values can be validated for free
            if int(frames.min()) < 2 or int(frames.max()) > T:
                raise ValueError(f"frames must lie in [2, {T}], got [{int(frames.min())}, {int(frames.max())}]")
        if src_of_row.device.type != "cuda":
            if int(src_of_row.min()) < 0 or int(src_of_row.max()) >= U:
                raise ValueError(f"src_of_row must lie in [0, {U - 1}], got [{int(src_of_row.min())}, {int(src_of_row.max())}]")
        unit, g = (self._f32(t, self.device) for t in (unit, g))
        lens = frames.to(device=self.device, dtype=torch.int32).contiguous()
        src = src_of_row.to(device=self.device, dtype=torch.int32).contiguous()
        if out is None:
            out = torch.empty(R, 1, T * self.samples_per_frame, dtype=torch.float32, device=self.device)
        if ws is None:
            ws = self.workspace(R, T, sources=U)
        if desc is None:
            fn = self.lib.qvc_infer_fanout_ragged_fm if unit_fm else self.lib.qvc_infer_fanout_ragged
            draw = noise.data_ptr()
        else:
            fn = self.lib.qvc_infer_fanout_ragged_rng_fm if unit_fm else self.lib.qvc_infer_fanout_ragged_rng
            draw = ctypes.byref(desc)
        st = fn(ctypes.byref(self.cfg), self.blob.data_ptr(), unit.data_ptr(), lens.data_ptr(), src.data_ptr(), g.data_ptr(),
                draw, out.data_ptr(), U, R, T, ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_infer_fanout_ragged")
        return out

    # ---- streaming: the segment rings (qvc_stream_*), the windowed step with a bounded look-ahead (qvc_live_*: every
    #      decoder, the lag is the caller's choice) and the tick forms of both (qvc_stream_tick*, qvc_live_tick*: per-slot
    #      frame counts on the device).  Sizes, one step and the per-slot reset of each; the state / workspace tensors belong to the caller.
    def _stream_sizes(self, form: str, queries, *args):
        """The values of lib.qvc_<query>(cfg, ...) -- the byte queries with ``args``, the frame queries without."""
        cfg = ctypes.byref(self.cfg)
        vals = tuple(int(getattr(self.lib, "qvc_" + q)(cfg, *(args if q.endswith("_bytes") else ()))) for q in queries)
        for v in vals:
            if v < 0:
                L.check(self.lib, v, f"qvc_{form}_*_bytes")
        return vals

    def _stream_call(self, form: str, state, ws, unit_new, g, noise_new, out, geom, ptrs, rng) -> None:
        """qvc_<form> / qvc_<form>_rng: ``geom`` the integers behind the batch (hop, look_ahead), ``ptrs`` the int32 device
        tensors in front of the workspace (n_new, pos, lens)."""
        B = unit_new.shape[0]
        if rng is not None and not (torch.is_tensor(rng[1]) and rng[1].device == self.device):
            raise ValueError(f"{form} needs the rng keys as an int64 tensor on the engine's device (slots are rewritten in place)")
        noise_new, desc, _ = self._draw(noise_new, rng, B, (B, self.model_config["inter_channels"], unit_new.shape[2]))
        fn, draw = (getattr(self.lib, "qvc_" + form), noise_new.data_ptr()) if desc is None else (getattr(self.lib, f"qvc_{form}_rng"), ctypes.byref(desc))
        st = fn(ctypes.byref(self.cfg), self.blob.data_ptr(), state.data_ptr(), state.numel(), unit_new.data_ptr(), g.data_ptr(),
                draw, out.data_ptr(), B, *geom, *(t.data_ptr() for t in ptrs), ws.data_ptr(), ws.numel(),
                torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_" + form)

    def _stream_reset_slot(self, form: str, state, batch, geom, slot, length, pos, lens) -> None:
        st = getattr(self.lib, f"qvc_{form}_reset_slot")(ctypes.byref(self.cfg), state.data_ptr(), state.numel(), batch, *geom, int(slot),
                                                         int(length), pos.data_ptr(), lens.data_ptr(),
                                                         torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, f"qvc_{form}_reset_slot")

    def stream_sizes(self, batch: int, hop: int):
        """(state_bytes, workspace_bytes, lag_frames, noise_lag_frames) for `batch` streams fed `hop` frames per step."""
        return self._stream_sizes("stream", ("stream_state_bytes", "stream_workspace_bytes", "stream_lag_frames", "stream_noise_lag_frames"),
                                  batch, hop)

    @_on_device
    def stream_step(self, state: torch.Tensor, ws: torch.Tensor, unit_new: torch.Tensor, g: torch.Tensor, noise_new: Optional[torch.Tensor],
                    out: torch.Tensor, pos: torch.Tensor, lens: torch.Tensor, rng=None) -> None:
        """One hop for every stream (all tensors fp32 / int32, contiguous, on this device; see include/qvc.h).
        ``rng``: with ``noise_new=None``, ``(seed, keys, scale)`` with ``keys`` an int64 tensor of one key per slot ON THIS
        DEVICE (qvc_stream_step_rng): the caller writes keys[slot] when it admits a stream; a captured step holds the
        array's pointer, so the tensor must outlive the graph."""
        self._stream_call("stream_step", state, ws, unit_new, g, noise_new, out, (unit_new.shape[2],), (pos, lens), rng)

    @_on_device
    def stream_reset_slot(self, state: torch.Tensor, batch: int, hop: int, slot: int, length: int, pos: torch.Tensor,
                          lens: torch.Tensor) -> None:
        """qvc_stream_reset_slot: zero slot `slot`'s ring rows, pos[slot] = 0, lens[slot] = length (on the current stream)."""
        self._stream_reset_slot("stream", state, batch, (hop,), slot, length, pos, lens)

    # ---- slot snapshots of the segment rings: what a stream is between two calls, free of batch, slot and hop
    def stream_snapshot_bytes(self) -> int:
        """Bytes of ONE slot's snapshot (qvc_stream_snapshot_bytes): a multiple of 256, a function of the model alone."""
        return self._stream_sizes("stream_snapshot", ("stream_snapshot_bytes",))[0]

    def stream_snapshot_tag(self) -> int:
        """The 64-bit fingerprint of the snapshot layout (qvc_stream_snapshot_tag): equal tags + the same checkpoint =
        interchangeable snapshots."""
        tag = ctypes.c_uint64(0)
        L.check(self.lib, self.lib.qvc_stream_snapshot_tag(ctypes.byref(self.cfg), ctypes.byref(tag)), "qvc_stream_snapshot_tag")
        return int(tag.value)

    def _stream_snapshot_call(self, name: str, state, batch, hop, slots, pos, lens, snap) -> None:
        slots = [int(s) for s in slots]
        arr = (ctypes.c_int32 * max(len(slots), 1))(*slots)
        st = getattr(self.lib, name)(ctypes.byref(self.cfg), state.data_ptr(), state.numel(), int(batch), int(hop), arr, len(slots),
                                     pos.data_ptr(), lens.data_ptr(), snap.data_ptr(), snap.numel(),
                                     torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, name)

    @_on_device
    def stream_export_slots(self, state: torch.Tensor, batch: int, hop: int, slots, pos: torch.Tensor, lens: torch.Tensor,
                            snap: torch.Tensor) -> None:
        """qvc_stream_export_slots: snapshot i of ``snap`` (uint8, 256-byte aligned, on this device, len(slots) *
        stream_snapshot_bytes()) <- slot ``slots[i]`` of ``state`` (built for ``batch`` slots and ``hop``), on the current
        stream.  Reads the state only."""
        self._stream_snapshot_call("qvc_stream_export_slots", state, batch, hop, slots, pos, lens, snap)

    @_on_device
    def stream_import_slots(self, state: torch.Tensor, batch: int, hop: int, slots, pos: torch.Tensor, lens: torch.Tensor,
                            snap: torch.Tensor) -> None:
        """qvc_stream_import_slots: slot ``slots[i]`` <- snapshot i: the kept part of that slot's ring rows, pos[slot] and
        lens[slot], nothing else.  The slot's g row and generator key are the caller's to move."""
        self._stream_snapshot_call("qvc_stream_import_slots", state, batch, hop, slots, pos, lens, snap)

    def stream_tick_sizes(self, batch: int, hop: int):
        """(state_bytes, workspace_bytes, lag_frames, noise_lag_frames) for `batch` streams that bring AT MOST `hop` frames
        per tick (qvc_stream_tick): stream_step's state, a larger workspace."""
        return self._stream_sizes("stream_tick", ("stream_state_bytes", "stream_tick_workspace_bytes", "stream_lag_frames",
                                                  "stream_noise_lag_frames"), batch, hop)

    @_on_device
    def stream_tick(self, state: torch.Tensor, ws: torch.Tensor, unit_new: torch.Tensor, g: torch.Tensor, noise_new: Optional[torch.Tensor],
                    out: torch.Tensor, n_new: torch.Tensor, pos: torch.Tensor, lens: torch.Tensor, rng=None) -> None:
        """One tick of the segment rings (all tensors fp32 / int32, contiguous, on this device; see include/qvc.h): slot b
        brings clamp(n_new[b], 0, hop) frames in the first columns of its row of ``unit_new`` (B, unit_channels, hop);
        `out` receives that many frames from pos - lag on, then zeros; ``pos`` is advanced on the device.  The state is
        stream_step's (started with stream_reset_slot); the two calls may alternate on it."""
        if n_new.dtype != torch.int32 or n_new.device != self.device or n_new.numel() != unit_new.shape[0]:
            raise ValueError("stream_tick needs n_new as an int32 tensor of one count per slot on the engine's device")
        self._stream_call("stream_tick", state, ws, unit_new, g, noise_new, out, (unit_new.shape[2],), (n_new, pos, lens), rng)

    def live_sizes(self, batch: int, hop: int, look_ahead: int):
        """(state_bytes, workspace_bytes, context_frames) for `batch` streams fed `hop` frames per step whose output lags
        the input by `look_ahead` frames (0 <= look_ahead <= context_frames); the window is context + look_ahead + hop."""
        return self._stream_sizes("live", ("live_state_bytes", "live_workspace_bytes", "live_context_frames"), batch, hop, look_ahead)

    @_on_device
    def live_step(self, state: torch.Tensor, ws: torch.Tensor, unit_new: torch.Tensor, g: torch.Tensor, noise_new: Optional[torch.Tensor],
                  out: torch.Tensor, pos: torch.Tensor, lens: torch.Tensor, look_ahead: int, rng=None) -> None:
        """One hop for every stream (all tensors fp32 / int32, contiguous, on this device; see include/qvc.h): `out`
        receives frames [pos - look_ahead, ... + hop) of the conversion of each stream's prefix.  ``noise_new``: the draw
        for the frames of ``unit_new``; ``rng``: as stream_step."""
        self._stream_call("live_step", state, ws, unit_new, g, noise_new, out, (unit_new.shape[2], int(look_ahead)), (pos, lens), rng)

    @_on_device
    def live_reset_slot(self, state: torch.Tensor, batch: int, hop: int, look_ahead: int, slot: int, length: int, pos: torch.Tensor,
                        lens: torch.Tensor) -> None:
        """qvc_live_reset_slot: zero slot `slot`'s ring rows, pos[slot] = 0, lens[slot] = length (on the current stream)."""
        self._stream_reset_slot("live", state, batch, (hop, int(look_ahead)), slot, length, pos, lens)

    def live_tick_sizes(self, batch: int, hop: int, look_ahead: int):
        """(state_bytes, workspace_bytes, context_frames) for `batch` streams that bring AT MOST `hop` frames per tick."""
        return self._stream_sizes("live_tick", ("live_tick_state_bytes", "live_tick_workspace_bytes", "live_context_frames"),
                                  batch, hop, look_ahead)

    @_on_device
    def live_tick(self, state: torch.Tensor, ws: torch.Tensor, unit_new: torch.Tensor, g: torch.Tensor, noise_new: Optional[torch.Tensor],
                  out: torch.Tensor, n_new: torch.Tensor, pos: torch.Tensor, lens: torch.Tensor, look_ahead: int, rng=None) -> None:
        """One tick (all tensors fp32 / int32, contiguous, on this device; see include/qvc.h): slot b brings
        clamp(n_new[b], 0, hop) frames in the first columns of its row of ``unit_new`` (B, unit_channels, hop); `out`
        receives that many frames from pos - look_ahead on, then zeros; ``pos`` is advanced on the device."""
        if n_new.dtype != torch.int32 or n_new.device != self.device or n_new.numel() != unit_new.shape[0]:
            raise ValueError("live_tick needs n_new as an int32 tensor of one count per slot on the engine's device")
        self._stream_call("live_tick", state, ws, unit_new, g, noise_new, out, (unit_new.shape[2], int(look_ahead)), (n_new, pos, lens), rng)

    @_on_device
    def live_tick_reset_slot(self, state: torch.Tensor, batch: int, hop: int, look_ahead: int, slot: int, length: int,
                             pos: torch.Tensor, lens: torch.Tensor) -> None:
        """qvc_live_tick_reset_slot: zero slot `slot`'s ring rows, pos[slot] = 0, lens[slot] = length (on the current stream)."""
        self._stream_reset_slot("live_tick", state, batch, (hop, int(look_ahead)), slot, length, pos, lens)

    # ---- exact windows over packed utterances (qvc_infer_windows_*): recordings of any length at bounded memory
    def windows_sizes(self, rows: int, window_frames: int):
        """(workspace_bytes, context_frames) for calls of `rows` windows that deliver `window_frames` frames each."""
        return self._stream_sizes("windows", ("windows_workspace_bytes", "live_context_frames"), rows, window_frames)

    @_on_device
    def infer_windows(self, ws: torch.Tensor, unit_packed: torch.Tensor, noise_packed: Optional[torch.Tensor], table: torch.Tensor,
                      g: torch.Tensor, out_packed: torch.Tensor, window_frames: int, rng=None) -> None:
        """One call of `rows` windows (all tensors contiguous on this device; see include/qvc.h): ``unit_packed``
        (total_frames, unit_channels) fp32, ``noise_packed`` (inter, total_frames) fp32 or None with ``rng = (seed, keys,
        scale)`` (keys: an int64 tensor of one key per ROW on this device), ``table`` (rows, 4) int32 -- base, length,
        start, count per row --, ``g`` (rows, gin), ``out_packed`` (total_frames * samples_per_frame,) fp32: row r writes
        its ``count`` frames from frame base + start on and nothing else."""
        mc = self.model_config
        rows, total = int(table.shape[0]), int(unit_packed.shape[0])
        if table.dtype != torch.int32 or tuple(table.shape) != (rows, 4) or unit_packed.dim() != 2 or unit_packed.shape[1] != mc.get("unit_channels", 256) \
                or tuple(g.shape) != (rows, mc["gin_channels"]) or out_packed.numel() != total * self.samples_per_frame:
            raise ValueError(f"bad input shapes: table {tuple(table.shape)}, unit_packed {tuple(unit_packed.shape)}, g {tuple(g.shape)}, "
                             f"out_packed {tuple(out_packed.shape)}")
        for t in (table, unit_packed, g, out_packed) + (() if noise_packed is None else (noise_packed,)):
            if t.device.type != "cuda" or not t.is_contiguous() or (t is not table and t.dtype != torch.float32):
                raise ValueError("infer_windows needs contiguous fp32 / int32 tensors on the engine's device")
        if rng is not None and not (torch.is_tensor(rng[1]) and rng[1].device == self.device):
            raise ValueError("infer_windows needs the rng keys as an int64 tensor on the engine's device")
        noise_packed, desc, _ = self._draw(noise_packed, rng, rows, (mc["inter_channels"], total))
        fn, draw = (self.lib.qvc_infer_windows_fm, noise_packed.data_ptr()) if desc is None else (self.lib.qvc_infer_windows_rng_fm, ctypes.byref(desc))
        st = fn(ctypes.byref(self.cfg), self.blob.data_ptr(), unit_packed.data_ptr(), draw, table.data_ptr(), g.data_ptr(), out_packed.data_ptr(),
                rows, int(window_frames), total, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_infer_windows_fm")

    def _pack_spk(self) -> None:
        if self._spk_blob is None:
            if not self._spk_sd:
                raise L.QvcError("the state dict holds no enc_spk.* weights")
            host = L.pack_weights(self.lib, self.cfg, self._spk_sd, which="spk")
            self._spk_blob = _aligned_empty(host.numel(), self.device)
            self._spk_blob.copy_(host)

    @_on_device
    def speaker_embed_ragged(self, mel: torch.Tensor, frames: torch.Tensor, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """embed_utterance for rows of DIFFERENT lengths: mel (U, n_mel, Fmax) padded (the padding's content is ignored),
        frames (U,) int32 valid frames per row -- on the device it is never read on the host, so the call can sit in a
        captured graph -- -> g (U, gin).  Row u equals ``speaker_embed(mel[u:u+1, :, :frames[u]])`` bit for bit; a row
        of 0 frames gives zeros.  ``ws``: a caller-owned workspace (graph owners); default = the shared one."""
        if mel.dim() != 3 or mel.shape[1] != int(self.cfg.n_mel_channels) or mel.shape[2] < 1 or tuple(frames.shape) != (mel.shape[0],):
            raise ValueError(f"mel must be (U, {int(self.cfg.n_mel_channels)}, frames) and frames (U,), got {tuple(mel.shape)}, {tuple(frames.shape)}")
        self._pack_spk()
        mel = self._f32(mel, self.device)
        frames = frames.to(device=self.device, dtype=torch.int32).contiguous()
        U, _, F = mel.shape
        n = int(self.lib.qvc_spk_ragged_workspace_bytes(ctypes.byref(self.cfg), U, F))
        if n < 0:
            L.check(self.lib, n, "qvc_spk_ragged_workspace_bytes")
        if ws is None:
            if self._spk_ws is None or self._spk_ws.numel() < n:
                self._spk_ws = _aligned_empty(n, self.device)
            ws = self._spk_ws
        g = torch.empty(U, self.model_config["gin_channels"], dtype=torch.float32, device=self.device)
        st = self.lib.qvc_speaker_embed_ragged(ctypes.byref(self.cfg), self._spk_blob.data_ptr(), mel.data_ptr(), frames.data_ptr(),
                                               g.data_ptr(), U, F, ws.data_ptr(), ws.numel(),
                                               torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_speaker_embed_ragged")
        return g

    @_on_device
    def speaker_embed(self, mel: torch.Tensor) -> torch.Tensor:
        """SpeakerEncoder.embed_utterance for a batch (models.py:528-546): mel (U, n_mel, F) -> g (U, gin)."""
        if mel.dim() != 3 or mel.shape[1] != int(self.cfg.n_mel_channels) or mel.shape[2] < 1:
            raise ValueError(f"mel must be (U, {int(self.cfg.n_mel_channels)}, frames), got {tuple(mel.shape)}")
        self._pack_spk()
        mel = self._f32(mel, self.device)
        U, _, F = mel.shape
        n = int(self.lib.qvc_spk_workspace_bytes(ctypes.byref(self.cfg), U, F))
        if n < 0:
            L.check(self.lib, n, "qvc_spk_workspace_bytes")
        if self._spk_ws is None or self._spk_ws.numel() < n:
            self._spk_ws = _aligned_empty(n, self.device)
        g = torch.empty(U, self.model_config["gin_channels"], dtype=torch.float32, device=self.device)
        st = self.lib.qvc_speaker_embed(ctypes.byref(self.cfg), self._spk_blob.data_ptr(), mel.data_ptr(), g.data_ptr(),
                                        U, F, self._spk_ws.data_ptr(), self._spk_ws.numel(),
                                        torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_speaker_embed")
        return g

    @_on_device
    def enc_q(self, spec: torch.Tensor, g: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
        """Posterior encoder, models.py:617: spec (B, spec_channels, T), g (B, gin), noise (B, inter, T) -> z [B][T][inter]."""
        B, cs, T = spec.shape
        mc = self.model_config
        if cs != int(self.cfg.spec_channels) or g.shape != (B, mc["gin_channels"]) or tuple(noise.shape) != (B, mc["inter_channels"], T):
            raise ValueError(f"bad input shapes: spec {tuple(spec.shape)}, g {tuple(g.shape)}, noise {tuple(noise.shape)}")
        if self._encq_blob is None:
            if not self._encq_sd:
                raise L.QvcError("the state dict holds no enc_q.* weights")
            host = L.pack_weights(self.lib, self.cfg, self._encq_sd, which="encq")
            self._encq_blob = _aligned_empty(host.numel(), self.device)
            self._encq_blob.copy_(host)
        spec, g, noise = (self._f32(t, self.device) for t in (spec, g, noise))
        z = torch.empty(B, T, mc["inter_channels"], dtype=torch.float32, device=self.device)
        ws = self.workspace(B, T)
        st = self.lib.qvc_enc_q(ctypes.byref(self.cfg), self._encq_blob.data_ptr(), spec.data_ptr(), g.data_ptr(), noise.data_ptr(),
                                z.data_ptr(), B, T, ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_enc_q")
        return z

    @_on_device
    def flow_forward(self, z_fm: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
        """ResidualCouplingBlock.forward(reverse=False), models.py:618: z [B][T][inter] -> z_p (a new tensor)."""
        B, T, _ = z_fm.shape
        z = self._f32(z_fm, self.device).clone()
        g = self._f32(g, self.device)
        ws = self.workspace(B, T)
        st = self.lib.qvc_flow_forward(ctypes.byref(self.cfg), self.blob.data_ptr(), z.data_ptr(), g.data_ptr(), B, T,
                                       ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_flow_forward")
        return z

    @_on_device
    def infer_batch_timed(self, unit, g, noise, out=None, max_records: int = 512):
        """Same launches with per-launch HIP-event timing; returns (out, [dict(name, ms, flops, bytes)])."""
        B, _, T = unit.shape
        unit, g, noise = (self._f32(t, self.device) for t in (unit, g, noise))
        if out is None:
            out = torch.empty(B, 1, T * self.samples_per_frame, dtype=torch.float32, device=self.device)
        ws = self.workspace(B, T)
        rec = (L.QvcLaunchRecord * max_records)()
        n = ctypes.c_int32(0)
        st = self.lib.qvc_infer_batch_timed(ctypes.byref(self.cfg), self.blob.data_ptr(), unit.data_ptr(), g.data_ptr(),
                                            noise.data_ptr(), out.data_ptr(), B, T, ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream(self.device).cuda_stream, rec, max_records,
                                            ctypes.byref(n))
        L.check(self.lib, st, "qvc_infer_batch_timed")
        return out, [dict(name=rec[i].name.decode(), ms=float(rec[i].ms), flops=float(rec[i].flops),
                          bytes=float(rec[i].bytes)) for i in range(min(n.value, max_records))]

    # ---- stage entry points (frame-major tensors), used by the stage-level parity tests
    @_on_device
    def enc_p(self, unit, noise):
        B, _, T = unit.shape
        unit, noise = self._f32(unit, self.device), self._f32(noise, self.device)
        z = torch.empty(B, T, self.model_config["inter_channels"], dtype=torch.float32, device=self.device)
        ws = self.workspace(B, T)
        st = self.lib.qvc_enc_p(ctypes.byref(self.cfg), self.blob.data_ptr(), unit.data_ptr(), noise.data_ptr(),
                                z.data_ptr(), B, T, ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_enc_p")
        return z

    @_on_device
    def wn_stack(self, which: int, x_fm, g=None):
        """WN.forward (modules.py:69-114) of stack ``which`` (0 = enc_p.enc, 1+i = flow.flows[2i].enc): [B][T][hidden] -> same."""
        B, T, _ = x_fm.shape
        x = self._f32(x_fm, self.device)
        gg = self._f32(g, self.device) if g is not None else None
        out = torch.empty_like(x)
        ws = self.workspace(B, T)
        st = self.lib.qvc_wn_stack(ctypes.byref(self.cfg), self.blob.data_ptr(), int(which), x.data_ptr(),
                                   gg.data_ptr() if gg is not None else None, out.data_ptr(), B, T, ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_wn_stack")
        return out

    @_on_device
    def flow_reverse(self, z_fm, g):
        B, T, _ = z_fm.shape
        z = self._f32(z_fm, self.device).clone()
        g = self._f32(g, self.device)
        ws = self.workspace(B, T)
        st = self.lib.qvc_flow_reverse(ctypes.byref(self.cfg), self.blob.data_ptr(), z.data_ptr(), g.data_ptr(), B, T,
                                       ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_flow_reverse")
        return z

    @_on_device
    def dec_trunk(self, z_fm, g):
        B, T, _ = z_fm.shape
        z, g = self._f32(z_fm, self.device), self._f32(g, self.device)
        frames = T * (self.samples_per_frame // (self.model_config["gen_istft_hop_size"] * self.model_config["subbands"])) + 1
        pc = self.model_config["subbands"] * 2 * (self.model_config["gen_istft_n_fft"] // 2 + 1)
        post = torch.empty(B, frames, pc, dtype=torch.float32, device=self.device)
        ws = self.workspace(B, T)
        st = self.lib.qvc_dec_trunk(ctypes.byref(self.cfg), self.blob.data_ptr(), z.data_ptr(), g.data_ptr(),
                                    post.data_ptr(), B, T, ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_dec_trunk")
        return post

    @_on_device
    def istft_synth(self, post_fm, want_bands: bool = False):
        B, F, _ = post_fm.shape
        post = self._f32(post_fm, self.device)
        hop, sb = self.model_config["gen_istft_hop_size"], self.model_config["subbands"]
        out = torch.empty(B, 1, sb * hop * (F - 1), dtype=torch.float32, device=self.device)
        ymb = torch.empty(B, sb, hop * (F - 1), dtype=torch.float32, device=self.device) if want_bands else None
        st = self.lib.qvc_istft_synth(ctypes.byref(self.cfg), self.blob.data_ptr(), post.data_ptr(), out.data_ptr(),
                                      ymb.data_ptr() if want_bands else None, B, F,
                                      torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib, st, "qvc_istft_synth")
        return (out, ymb) if want_bands else out
