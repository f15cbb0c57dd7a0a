"""``SynthesizerTrn`` -- the reference's model object, re-hosted on HIP kernels.

Drop-in surface (models.py:549-642 of the reference, used by convert.py:35-41,81):
same constructor signature (unknown kwargs swallowed), same ``state_dict`` keys and
shapes (so ``utils.load_checkpoint`` of the reference's ``.pth`` works unchanged),
``.cuda()``, ``.eval()``, ``.parameters()``, ``.infer(unit, mel)``.

What is different underneath: the sub-modules below are *parameter holders* only.
There is no PyTorch forward for enc_p / flow / dec: ``infer`` and ``infer_batch``
hand the raw tensors to ``libqvc_hip.so`` (engine.py), which runs the whole path as
hand-written gfx950 kernels -- the speaker encoder (3-layer LSTM)
included.  If the HIP library is missing or no GPU is present, ``infer`` raises; there is
no CPU fallback and no torch forward anywhere in this module.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import Tensor, nn


# ----------------------------------------------------------------------------- holders
class ConvParams(nn.Module):
    """Parameters of one Conv1d / ConvTranspose1d, weight-normed or plain.

    Weight-normed convs expose ``bias, weight_g, weight_v`` (old-style
    ``torch.nn.utils.weight_norm`` naming); plain ones ``weight, bias``.
    ``shape`` is the weight shape: (Cout, Cin, K) for Conv1d, (Cin, Cout, K) for
    ConvTranspose1d -- ``weight_g`` is (shape[0], 1, 1) either way.
    """

    def __init__(self, shape: Sequence[int], weight_norm: bool, bias: bool = True, bias_size: Optional[int] = None):
        super().__init__()
        shape = tuple(int(s) for s in shape)
        nb = shape[0] if bias_size is None else int(bias_size)
        if weight_norm:
            self.bias = nn.Parameter(torch.zeros(nb)) if bias else None
            self.weight_g = nn.Parameter(torch.ones(shape[0], 1, 1))
            self.weight_v = nn.Parameter(torch.zeros(shape))
        else:
            self.weight = nn.Parameter(torch.zeros(shape))
            self.bias = nn.Parameter(torch.zeros(nb)) if bias else None


class WNParams(nn.Module):
    """modules.py:37-67: optional cond_layer, n in_layers (h->2h, k), n res_skip_layers (1x1)."""

    def __init__(self, hidden: int, kernel_size: int, n_layers: int, gin_channels: int):
        super().__init__()
        assert kernel_size % 2 == 1, f"kernel should be odd number, but {kernel_size}"
        self.hidden_channels, self.kernel_size, self.n_layers, self.gin_channels = hidden, kernel_size, n_layers, gin_channels
        if gin_channels != 0:
            self.cond_layer = ConvParams((2 * hidden * n_layers, gin_channels, 1), True)
        self.in_layers = nn.ModuleList(ConvParams((2 * hidden, hidden, kernel_size), True) for _ in range(n_layers))
        self.res_skip_layers = nn.ModuleList(
            ConvParams(((2 * hidden if i < n_layers - 1 else hidden), hidden, 1), True) for i in range(n_layers))


class CondNormalWNParams(nn.Module):
    """models.py:54-73."""

    def __init__(self, in_ch: int, out_ch: int, hidden: int, kernel_size: int, n_layers: int, gin: int):
        super().__init__()
        self.pre = ConvParams((hidden, in_ch, 1), False)
        self.enc = WNParams(hidden, kernel_size, n_layers, gin)
        self.proj = ConvParams((2 * out_ch, hidden, 1), False)


class CouplingLayerParams(nn.Module):
    """modules.py:173-197."""

    def __init__(self, channels: int, hidden: int, kernel_size: int, n_layers: int, gin: int):
        super().__init__()
        assert channels % 2 == 0, "channels should be divisible by 2"
        self.pre = ConvParams((hidden, channels // 2, 1), False)
        self.enc = WNParams(hidden, kernel_size, n_layers, gin)
        self.post = ConvParams((channels // 2, hidden, 1), False)


class _NoParams(nn.Module):
    """Placeholder for the reference's parameter-free Flip (modules.py:165-170) so that
    ``flow.flows`` keeps its even indices for the coupling layers."""


class CouplingBlockParams(nn.Module):
    """models.py:17-37."""

    def __init__(self, channels: int, hidden: int, kernel_size: int, n_layers: int, n_flows: int, gin: int):
        super().__init__()
        self.flows = nn.ModuleList()
        for _ in range(n_flows):
            self.flows.append(CouplingLayerParams(channels, hidden, kernel_size, n_layers, gin))
            self.flows.append(_NoParams())


class ResBlock1Params(nn.Module):
    """modules.py:128-145."""

    def __init__(self, ch: int, k: int):
        super().__init__()
        self.convs1 = nn.ModuleList(ConvParams((ch, ch, k), True) for _ in range(3))
        self.convs2 = nn.ModuleList(ConvParams((ch, ch, k), True) for _ in range(3))


class _Window(nn.Module):
    def __init__(self, n_fft: int):
        super().__init__()
        self.register_buffer("window", torch.hann_window(n_fft))


def pqmf_filters(subbands: int = 4, taps: int = 62, cutoff_ratio: float = 0.15, beta: float = 9.0):
    """Cosine-modulated PQMF bank (the design used by pqmf.py:16-44,65-76 of the reference):
    Kaiser-windowed sinc prototype, band k modulated by (2k+1)*pi/(2*subbands).
    Returns (analysis (S,1,taps+1), synthesis (1,S,taps+1)) fp32 tensors."""
    import numpy as np
    n = np.arange(taps + 1, dtype=np.float64)
    centred = n - 0.5 * taps
    with np.errstate(invalid="ignore", divide="ignore"):
        proto = np.sin(np.pi * cutoff_ratio * centred) / (np.pi * centred)
    proto[taps // 2] = cutoff_ratio
    proto *= np.kaiser(taps + 1, beta)
    ana = np.zeros((subbands, taps + 1))
    syn = np.zeros((subbands, taps + 1))
    for k in range(subbands):
        arg = (2 * k + 1) * (np.pi / (2 * subbands)) * (n - (taps - 1) / 2.0)
        ana[k] = 2.0 * proto * np.cos(arg + ((-1) ** k) * np.pi / 4.0)
        syn[k] = 2.0 * proto * np.cos(arg - ((-1) ** k) * np.pi / 4.0)
    return torch.from_numpy(ana).float().unsqueeze(1), torch.from_numpy(syn).float().unsqueeze(0)


class _PQMFBuffers(nn.Module):
    """Buffers the reference's PQMF module registers (pqmf.py:83-90)."""

    def __init__(self, subbands: int):
        super().__init__()
        ana, syn = pqmf_filters(subbands)
        self.register_buffer("analysis_filter", ana)
        self.register_buffer("synthesis_filter", syn)
        upd = torch.zeros(subbands, subbands, subbands)
        for k in range(subbands):
            upd[k, k, 0] = 1.0
        self.register_buffer("updown_filter", upd)


class GeneratorParams(nn.Module):
    """Parameters of the three generators, models.py:98-160 / 195-248 / 304-358."""

    def __init__(self, kind: str, initial_channel: int, resblock_kernel_sizes, resblock_dilation_sizes,
                 upsample_rates, upsample_initial_channel: int, upsample_kernel_sizes,
                 n_fft: int, hop: int, subbands: int, gin_channels: int):
        super().__init__()
        self.kind = kind
        self.subbands = int(subbands) if kind != "istft" else 1
        n_bins = n_fft // 2 + 1
        self.conv_pre = ConvParams((upsample_initial_channel, initial_channel, 7), True)
        self.cond = ConvParams((upsample_initial_channel, gin_channels, 1), False)
        self.ups = nn.ModuleList()
        ch = upsample_initial_channel
        for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
            cin, ch = upsample_initial_channel // (2 ** i), upsample_initial_channel // (2 ** (i + 1))
            self.ups.append(ConvParams((cin, ch, k), True, bias_size=ch))
        self.resblocks = nn.ModuleList()
        for i in range(len(self.ups)):
            c = upsample_initial_channel // (2 ** (i + 1))
            for k, _d in zip(resblock_kernel_sizes, resblock_dilation_sizes):
                self.resblocks.append(ResBlock1Params(c, k))
        post_name = "conv_post" if kind == "istft" else "subband_conv_post"
        setattr(self, post_name, ConvParams((self.subbands * 2 * n_bins, ch, 7), True))
        self.stft = _Window(n_fft)
        if kind == "multiband":
            self.pqmf = _PQMFBuffers(self.subbands)
        if kind == "multistream":
            upd = torch.zeros(self.subbands, self.subbands, self.subbands)
            for k in range(self.subbands):
                upd[k, k, 0] = 1.0
            self.register_buffer("updown_filter", upd)
            self.multistream_conv_post = ConvParams((1, 4, 63), True, bias=False)


# ----------------------------------------------------------------------------- speaker encoder
class _LSTMParams(nn.Module):
    """Parameters of ``nn.LSTM(input, hidden, layers)`` under PyTorch's own names (weight_ih_l{k}, weight_hh_l{k},
    bias_ih_l{k}, bias_hh_l{k}; gate order i, f, g, o) -- what the reference's checkpoint stores for ``enc_spk.lstm``."""

    def __init__(self, input_size: int, hidden: int, layers: int):
        super().__init__()
        for k in range(layers):
            cin = input_size if k == 0 else hidden
            setattr(self, f"weight_ih_l{k}", nn.Parameter(torch.zeros(4 * hidden, cin)))
            setattr(self, f"weight_hh_l{k}", nn.Parameter(torch.zeros(4 * hidden, hidden)))
            setattr(self, f"bias_ih_l{k}", nn.Parameter(torch.zeros(4 * hidden)))
            setattr(self, f"bias_hh_l{k}", nn.Parameter(torch.zeros(4 * hidden)))


class _LinearParams(nn.Module):
    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin))
        self.bias = nn.Parameter(torch.zeros(cout))


class SpeakerEncoder(nn.Module):
    """Parameter holder for ``enc_spk.*`` (models.py:507-513: 3-layer LSTM 80 -> hidden, Linear hidden -> embedding).

    No forward: ``SynthesizerTrn.speaker_embed`` runs ``embed_utterance`` (models.py:528-546) on the HIP kernels of
    csrc/qvc_spk.hip; the fp32 torch restatement used to check them lives in ``oracle/qvc_oracle.py``."""

    def __init__(self, mel_n_channels=80, model_num_layers=3, model_hidden_size=256, model_embedding_size=256):
        super().__init__()
        self.lstm = _LSTMParams(mel_n_channels, model_hidden_size, model_num_layers)
        self.linear = _LinearParams(model_hidden_size, model_embedding_size)


# ----------------------------------------------------------------------------- the model
class SynthesizerTrn(nn.Module):
    """QuickVC generator with the hot path on gfx950 kernels (reference: models.py:549-642)."""

    def __init__(self, spec_channels: int, segment_size: int, inter_channels: int, hidden_channels: int,
                 resblock_kernel_sizes: List[int], resblock_dilation_sizes: List[List[int]],
                 upsample_rates: List[int], upsample_initial_channel: int, upsample_kernel_sizes: List[int],
                 gen_istft_n_fft: int, gen_istft_hop_size: int,
                 istft_vits: bool = False, ms_istft_vits: bool = False, mb_istft_vits: bool = False,
                 subbands=False, gin_channels: int = 0, operand_dtype: str = "f16", verbose: bool = False,
                 **kwargs):
        super().__init__()
        if verbose:
            print(f"Loaded but not used: {kwargs}")
        if kwargs.get("resblock"):
            assert kwargs["resblock"] == "1", "ResBlock2 support is droped."   # models.py:574-575
        kind = "multiband" if mb_istft_vits else ("multistream" if ms_istft_vits else ("istft" if istft_vits else None))
        if kind is None:
            raise RuntimeError(f"Not-supported decoder flag: {mb_istft_vits}/{ms_istft_vits}/{istft_vits}")
        self.segment_size = segment_size
        unit_channels = 256                                                      # models.py:579
        self.model_config = dict(
            unit_channels=unit_channels, inter_channels=inter_channels, hidden_channels=hidden_channels,
            gin_channels=gin_channels, resblock_kernel_sizes=list(resblock_kernel_sizes),
            resblock_dilation_sizes=[list(d) for d in resblock_dilation_sizes],
            upsample_rates=list(upsample_rates), upsample_initial_channel=upsample_initial_channel,
            upsample_kernel_sizes=list(upsample_kernel_sizes), gen_istft_n_fft=gen_istft_n_fft,
            gen_istft_hop_size=gen_istft_hop_size, subbands=(int(subbands) if kind != "istft" else 1),
            decoder=kind, operand_dtype=operand_dtype, spec_channels=int(spec_channels))

        self.enc_q = CondNormalWNParams(spec_channels, inter_channels, hidden_channels, 5, 16, gin_channels)
        self.enc_p = CondNormalWNParams(unit_channels, inter_channels, hidden_channels, 5, 16, 0)
        self.flow = CouplingBlockParams(inter_channels, hidden_channels, 5, 4, 4, gin_channels)
        self.enc_spk = SpeakerEncoder(model_hidden_size=gin_channels, model_embedding_size=gin_channels)
        self.dec = GeneratorParams(kind, inter_channels, resblock_kernel_sizes, resblock_dilation_sizes,
                                   upsample_rates, upsample_initial_channel, upsample_kernel_sizes,
                                   gen_istft_n_fft, gen_istft_hop_size, subbands, gin_channels)
        self._engine = None          # built lazily, rebuilt after the weights change
        self._engine_key = None

    # ---- samples per unit frame (320 for the shipped config)
    @property
    def samples_per_frame(self) -> int:
        c = self.model_config
        n = c["gen_istft_hop_size"] * c["subbands"]
        for u in c["upsample_rates"]:
            n *= u
        return n

    # ---- engine management
    def _weights_version(self):
        return tuple(p._version for p in self.parameters()) + (str(next(self.parameters()).device),)

    def engine(self):
        """The HIP engine for the current weights (packs them on first use / after a reload)."""
        from .engine import QvcEngine   # imports the ctypes binding; raises if the .so is missing
        key = self._weights_version()
        if self._engine is None or self._engine_key != key:
            device = next(self.parameters()).device
            if device.type != "cuda":
                raise RuntimeError("SynthesizerTrn hot path runs on an MI355X only: call .cuda() first "
                                   "(there is no CPU fallback)")
            sd = {k: v.detach() for k, v in self.state_dict().items()}
            self._engine = QvcEngine(self.model_config, sd, device)
            self._engine_key = key
        return self._engine

    def forward(self, *args, **kwargs):
        raise NotImplementedError("training forward (models.py:593-623) is outside the inference hot path")

    # ---- reference API
    @torch.no_grad()
    def infer(self, unit: Tensor, mel: Tensor, noise: Optional[Tensor] = None) -> Tensor:
        """models.py:625-642.  unit (1,256,F), mel (1,80,F') -> (1,1,320*F) fp32.

        ``noise`` (1, inter, F) optionally replaces the internal N(0,1) draw of
        models.py:94 so a caller can reproduce a run.
        """
        g = self.speaker_embed(mel)                                               # models.py:635
        return self.infer_batch(unit, g, noise)

    @torch.no_grad()
    def infer_long(self, unit: Tensor, g_or_mel: Tensor, window_frames: int = 1024, rows: int = 32, noise: Optional[Tensor] = None,
                   seed: Optional[int] = None, key: int = 0, noise_scale: float = 1.0) -> Tensor:
        """``infer`` for ONE recording of any length at bounded memory: unit (1,256,F), ``g_or_mel`` the speaker embedding
        (1,gin) / (1,gin,1) or the target's mel (1,80,F') -> (1,1,320*F) fp32, equal to ``infer`` on the whole recording.
        The recording is cut into windows of ``window_frames`` delivered frames that run ``rows`` at a time
        (windows.WindowConverter); the converter is kept for the next call of the same geometry.
        ``noise`` (1, inter, F) / ``seed``, ``key``, ``noise_scale``: as ``infer_batch``."""
        from .windows import WindowConverter
        if noise is not None and seed is not None:
            raise ValueError("pass noise or seed, not both")
        mel = g_or_mel.dim() == 3 and g_or_mel.shape[-1] > 1                      # (1, n_mel, F'), not (1, gin, 1)
        g = self.speaker_embed(g_or_mel) if mel else g_or_mel.reshape(1, -1)
        at = (self._weights_version(), int(rows), int(window_frames), seed, float(noise_scale))
        if getattr(self, "_long", None) is None or self._long[0] != at:
            self._long = (at, WindowConverter(self, rows, window_frames, seed=seed, noise_scale=noise_scale))
        frames = unit.reshape(-1, unit.shape[-1]).t().contiguous()                # (F, 256): as on disk
        out = self._long[1].convert([frames], g, keys=[key], noise=None if noise is None else [noise.reshape(noise.shape[-2], -1)])
        return out[0].reshape(1, 1, -1)

    @torch.no_grad()
    def posterior(self, spec: Tensor, g: Tensor, noise: Optional[Tensor] = None):
        """The analysis half of ``forward`` (models.py:617-618): z ~ enc_q(spec | g), z_p = flow(z, g).

        spec (B, spec_channels, T), g (B, gin) or (B, gin, 1), noise (B, inter, T) optional -> (z, z_p), both (B, inter, T).
        """
        eng = self.engine()
        g = g.reshape(g.shape[0], -1)
        if noise is None:
            noise = torch.randn(spec.shape[0], self.model_config["inter_channels"], spec.shape[2], device=spec.device)
        z = eng.enc_q(spec, g, noise)
        z_p = eng.flow_forward(z, g)
        return z.transpose(1, 2).contiguous(), z_p.transpose(1, 2).contiguous()

    @torch.no_grad()
    def speaker_embed(self, mel: Tensor) -> Tensor:
        """SpeakerEncoder.embed_utterance (models.py:528-546) for a batch: mel (U, 80, F') -> g (U, gin).

        Runs the persistent-LSTM HIP kernels (csrc/qvc_spk.hip).  Speaker widths the kernels do not cover
        (gin > 256 or gin % 8 != 0) raise ``QvcError`` (QVC_ERR_BAD_CONFIG from the library): there is no torch path.
        """
        return self.engine().speaker_embed(mel)

    @torch.no_grad()
    def speaker_embed_waves(self, waves, front, trim_top_db: Optional[float] = 20.0) -> Tensor:
        """The target side of convert.py:64-77 for a batch of recordings of ANY lengths: ``waves`` is a list of 1-D float
        arrays / tensors at the model's sampling rate, ``front`` a ``MelFrontend`` -> g (U, gin).

        The rows are padded into one upload, then silence trim (``trim_top_db=None`` skips it), mel and the speaker
        encoder run back to back on the device lengths -- no host sync in between -- and each row equals
        ``speaker_embed(front(trim(w)))`` of that recording alone.  The frame counts are read back once at the end: a
        recording too short for one mel frame raises ``ValueError`` (as it does alone)."""
        import numpy as np
        eng = self.engine()
        rows = [torch.as_tensor(np.asarray(w, dtype=np.float32) if not torch.is_tensor(w) else w).reshape(-1) for w in waves]
        if not rows:
            raise ValueError("no waveform given")
        lens = [int(r.numel()) for r in rows]
        if max(lens) <= (front.n_fft - front.hop) // 2:                      # host-known: not even the longest row has a frame
            raise ValueError(f"waveforms {list(range(len(rows)))} are too short for one mel frame")
        host = torch.zeros(len(rows), max(max(lens), 1), dtype=torch.float32).pin_memory()
        for u, r in enumerate(rows):
            host[u, :lens[u]] = r.to(device="cpu", dtype=torch.float32)
        wave = host.to(eng.device, non_blocking=True)
        samples = torch.tensor(lens, dtype=torch.int32).pin_memory().to(eng.device, non_blocking=True)
        g, empty = self._embed_wave_batch(wave, samples, front, trim_top_db)
        if empty:
            raise ValueError(f"waveforms {empty} are too short for one mel frame after trimming")
        return g

    def _embed_wave_batch(self, wave: Tensor, samples: Tensor, front, trim_top_db: Optional[float]):
        """The device side of ``speaker_embed_waves`` and ``speaker_embed_files``: wave (U, max_samples) fp32 and samples
        (U,) int32, both on the device -> (g (U, gin), the rows without a mel frame).  Trim, mel and the speaker encoder
        run back to back on the device lengths; the frame counts are the one read-back, after everything is enqueued."""
        from .frontend import trim_bounds
        start = None
        if trim_top_db is not None:
            start, samples = trim_bounds(wave, samples, top_db=trim_top_db)
        mel, frames = front.ragged(wave, samples, start)
        g = self.engine().speaker_embed_ragged(mel, frames)
        return g, [u for u, f in enumerate(frames.tolist()) if f <= 0]

    def stage_target_files(self, paths, sr: int, pool, headers=None, buf: Optional[Tensor] = None) -> dict:
        """The host half of ``speaker_embed_files``: the recordings ``paths`` as ONE pinned byte buffer -- U slots of raw
        payload and the (code, channels, frames) row table behind them -- ready for one upload.  ``pool`` is a
        ``fileio.IoPool``; ``headers`` = ``pool.wav_headers(paths)`` when the caller has read them already; ``buf`` a
        pinned uint8 tensor to fill when it is large enough (a caller that stages the next batch while this one embeds
        keeps two).  Needs no GPU: a helper thread may run it.

        A file takes the native route -- its payload read by the pool straight into its slot, as it is on disk -- when
        the header reader accepted it, its rate is ``sr`` and it has one or two channels.  Every other file (another rate,
        f64, more channels, anything the reader refused) goes through ``frontend.load_wav`` as before, so a broken file
        raises what it raised before, and its floats are stored in its slot as an f32 mono row."""
        import numpy as np
        from .fileio import PCM_BYTES, PCM_F32, QVC_IO_OK
        from .frontend import load_wav
        paths = list(paths)
        if not paths:
            raise ValueError("no waveform given")
        hdr, st = pool.wav_headers(paths) if headers is None else headers
        native = [u for u in range(len(paths)) if st[u] == QVC_IO_OK and hdr[u].rate == int(sr) and hdr[u].channels in (1, 2)]
        is_native = set(native)
        hosted = [u for u in range(len(paths)) if u not in is_native]
        host_waves = [np.ascontiguousarray(load_wav(paths[u], int(sr)), dtype=np.float32).reshape(-1) for u in hosted]
        order = native + hosted                                               # row r of the batch is file order[r]: one pool call fills rows 0 .. len(native)-1
        rows = [(hdr[u].code, hdr[u].channels, int(hdr[u].frames)) for u in native] + [(PCM_F32, 1, int(w.size)) for w in host_waves]
        if max(r[2] for r in rows) >= 1 << 31:
            raise ValueError("a recording of 2^31 samples or more does not fit a row")
        need = max(max(PCM_BYTES[c] * ch * n for c, ch, n in rows), 1)
        slot_bytes = -(-need // 16) * 16
        U = len(rows)
        total = U * slot_bytes + U * 12
        if buf is None or buf.numel() < total:
            buf = torch.empty(total, dtype=torch.uint8).pin_memory()
        if native:
            got, st2 = pool.load_wavs([paths[u] for u in native], buf, slot_bytes)
            for r, u in enumerate(native):
                if st2[r] != QVC_IO_OK or (got[r].code, got[r].channels, int(got[r].frames)) != rows[r]:
                    raise ValueError(f"{paths[u]}: changed since its header was read (status {st2[r]})")
        for r, w in enumerate(host_waves, start=len(native)):
            buf[r * slot_bytes:r * slot_bytes + 4 * w.size] = torch.from_numpy(w).view(torch.uint8)
        buf[U * slot_bytes:total].view(torch.int32).view(U, 3).copy_(torch.tensor(rows, dtype=torch.int32))
        return dict(buf=buf, total=total, slot_bytes=slot_bytes, rows=U, order=order, counts=[r[2] for r in rows],
                    max_samples=max(max(r[2] for r in rows), 1))

    @torch.no_grad()
    def speaker_embed_staged(self, staged: dict, front, trim_top_db: Optional[float] = 20.0) -> Tensor:
        """The device half of ``speaker_embed_files`` for what ``stage_target_files`` prepared: one upload (payload bytes
        and row table), one decode launch (``frontend.pcm_to_wave``), then what ``speaker_embed_waves`` runs."""
        from .frontend import pcm_to_wave
        eng = self.engine()
        U, order, counts = staged["rows"], staged["order"], staged["counts"]
        if max(counts) <= (front.n_fft - front.hop) // 2:                     # host-known (header counts): not even the longest row has a frame
            raise ValueError(f"waveforms {list(range(U))} are too short for one mel frame")
        dev = staged["buf"][:staged["total"]].to(eng.device, non_blocking=True)
        nb = U * staged["slot_bytes"]
        rows_dev = dev[nb:].view(torch.int32).view(U, 3)
        wave, samples = pcm_to_wave(dev[:nb], staged["slot_bytes"], rows_dev, staged["max_samples"])
        g_rows, empty = self._embed_wave_batch(wave, samples, front, trim_top_db)
        if empty:
            raise ValueError(f"waveforms {sorted(order[r] for r in empty)} are too short for one mel frame after trimming")
        g = torch.empty_like(g_rows)
        g[torch.as_tensor(order, device=g_rows.device)] = g_rows
        return g

    @torch.no_grad()
    def speaker_embed_files(self, paths, front, pool, trim_top_db: Optional[float] = 20.0) -> Tensor:
        """``speaker_embed_waves([load_wav(p, sr) for p in paths], front, trim_top_db)`` bit for bit, without the host
        decode: the recordings' headers and raw payloads are read on ``pool`` (a ``fileio.IoPool``) into one pinned byte
        buffer, uploaded once and turned into the padded fp32 batch by one launch -> g (U, gin).  Files that need
        resampling, f64 files, files of more than two channels and files the native header reader refuses are decoded by
        ``load_wav`` as before and ride the same batch (``stage_target_files``).  ``front`` is a ``MelFrontend`` (its
        sampling rate is the model's).  The "too short for one mel frame" errors are ``speaker_embed_waves``'s."""
        return self.speaker_embed_staged(self.stage_target_files(paths, front.sr, pool), front, trim_top_db)

    @torch.no_grad()
    def infer_batch(self, unit: Tensor, g: Tensor, noise: Optional[Tensor] = None, seed: Optional[int] = None, keys=None,
                    noise_scale: float = 1.0) -> Tensor:
        """Batched path: unit (B,256,F), g (B,gin) or (B,gin,1), noise (B,inter,F) -> (B,1,320*F).
        ``seed``: draw the noise on the device instead (the library's counter-based generator): row b's draw is a function
        of (seed, keys[b], channel, frame) alone -- ``keys`` B integers, default 0 .. B-1 -- scaled by ``noise_scale``."""
        eng = self.engine()
        if seed is not None:
            B, F = unit.shape[0], unit.shape[2]
            return eng.infer_batch_ragged(unit, g.reshape(B, -1), None, torch.full((B,), F, dtype=torch.int32),
                                          rng=self._rng(seed, keys, noise_scale, B, noise))
        if noise is None:
            noise = torch.randn(unit.shape[0], self.model_config["inter_channels"], unit.shape[2],
                                device=unit.device, dtype=torch.float32)
        return eng.infer_batch(unit, g.reshape(g.shape[0], -1), noise)

    @staticmethod
    def _rng(seed, keys, noise_scale, rows: int, noise):
        if noise is not None:
            raise ValueError("pass noise or seed, not both")
        keys = list(range(rows)) if keys is None else keys
        if (int(keys.shape[0]) if torch.is_tensor(keys) else len(keys)) != rows:
            raise ValueError(f"{rows} rows need {rows} keys")
        return (int(seed), keys, float(noise_scale))

    @torch.no_grad()
    def infer_ragged(self, units, g: Tensor, noises=None, seed: Optional[int] = None, keys=None, noise_scale: float = 1.0):
        """Utterances of DIFFERENT lengths in one launch sequence (the reference converts any length per call,
        convert.py:58-86): ``units`` is a list of (256, F_b) / (1, 256, F_b) tensors, g (B, gin) or (B, gin, 1),
        ``noises`` an optional list of (inter, F_b) draws.  Returns a list of (1, 320*F_b) fp32 waveforms -- each
        equal to the utterance converted alone (every conv sees ITS sequence end, not the padded batch's).
        ``seed`` / ``keys`` / ``noise_scale``: as ``infer_batch`` -- with them an utterance's waveform does not depend on
        the batch it is converted in either."""
        eng = self.engine()
        dev = eng.device
        us = [u.reshape(-1, u.shape[-1]) for u in units]
        lens = [int(u.shape[-1]) for u in us]
        B, tmax, inter = len(us), max(lens), self.model_config["inter_channels"]
        rng = self._rng(seed, keys, noise_scale, B, noises) if seed is not None else None
        unit = torch.zeros(B, us[0].shape[0], tmax, device=dev, dtype=torch.float32)
        noise = torch.zeros(B, inter, tmax, device=dev, dtype=torch.float32) if rng is None else None
        for b, u in enumerate(us):
            unit[b, :, :lens[b]] = u.to(dev, torch.float32)
            if rng is None:
                n = noises[b].reshape(inter, -1).to(dev, torch.float32) if noises is not None else \
                    torch.randn(inter, lens[b], device=dev, dtype=torch.float32)
                noise[b, :, :lens[b]] = n
        out = eng.infer_batch_ragged(unit, g.reshape(B, -1), noise, torch.tensor(lens, dtype=torch.int32), rng=rng)
        spf = self.samples_per_frame
        return [out[b, :, :lens[b] * spf] for b in range(B)]

    @torch.no_grad()
    def infer_fanout(self, units, src_of_row, g: Tensor, noises=None, seed: Optional[int] = None, keys=None, noise_scale: float = 1.0):
        """Any-to-many conversion: ``units`` is the list of U DISTINCT sources ((256, F_u) / (1, 256, F_u) tensors),
        ``src_of_row`` a list of R ints -- the source of every output row, each in [0, U) --, g (R, gin) or (R, gin, 1) the
        target speaker of every row, ``noises`` an optional list of R draws (inter, F_src).  Returns a list of R
        (1, 320*F_src) fp32 waveforms, each equal to what ``infer_ragged`` gives for that (source, g, noise); every
        source is encoded once (enc_p does not see the speaker, models.py:638-640).
        ``seed`` / ``keys`` (one per OUTPUT row, default 0 .. R-1) / ``noise_scale``: as ``infer_batch``."""
        eng = self.engine()
        dev = eng.device
        us = [u.reshape(-1, u.shape[-1]) for u in units]
        lens = [int(u.shape[-1]) for u in us]
        src = [int(s) for s in src_of_row]
        U, R, tmax, inter = len(us), len(src), max(lens), self.model_config["inter_channels"]
        if not 1 <= U <= R or min(src) < 0 or max(src) >= U:
            raise ValueError(f"{R} rows over {U} sources: every row names a source in [0, {U}) and rows >= sources >= 1")
        unit = torch.zeros(U, us[0].shape[0], tmax, device=dev, dtype=torch.float32)
        for u, x in enumerate(us):
            unit[u, :, :lens[u]] = x.to(dev, torch.float32)
        rng = self._rng(seed, keys, noise_scale, R, noises) if seed is not None else None
        noise = torch.zeros(R, inter, tmax, device=dev, dtype=torch.float32) if rng is None else None
        for r, s in enumerate(src):
            if rng is not None:
                break
            n = noises[r].reshape(inter, -1).to(dev, torch.float32) if noises is not None else \
                torch.randn(inter, lens[s], device=dev, dtype=torch.float32)
            noise[r, :, :lens[s]] = n
        out = eng.infer_fanout_ragged(unit, torch.tensor(lens, dtype=torch.int32), torch.tensor(src, dtype=torch.int32),
                                      g.reshape(R, -1), noise, rng=rng)
        spf = self.samples_per_frame
        return [out[r, :, :lens[s] * spf] for r, s in enumerate(src)]
