"""Test-side fp64/fp32 restatement of the single-band iSTFT decoder (iSTFT_Generator, models.py:98-192).

Composed from the oracle's pieces (oracle/qvc_oracle.py: cond_normal_wn, flow_reverse, resblock1,
istft_closed_form); only what differs from the multistream decoder is written out here:
  * up-sampler i is ConvTranspose1d(k, u, padding=(k-u)//2) with no output_padding (models.py:124-127),
  * conv_post is ``dec.conv_post`` with 2*(n_fft/2+1) output channels (models.py:139),
  * exp / pi*sin / iSTFT give the waveform directly: no band split, no synthesis FIR (models.py:171-176).
tests/golden/make_golden_istft.py pins this restatement against the reference's own taps.
"""
from typing import Optional

import torch
import torch.nn.functional as F

import qvc_oracle as oracle


def decoder_forward_single(sd, cfg, z, g, taps: Optional[dict] = None):
    """z (B, inter, T), g (B, gin, 1) -> (B, 1, hop * T * prod(upsample_rates))."""
    p = "dec"
    n_fft, hop = int(cfg["gen_istft_n_fft"]), int(cfg["gen_istft_hop_size"])
    n_bins = n_fft // 2 + 1
    ks, ds = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    x = F.conv1d(z, oracle.conv_weight(sd, f"{p}.conv_pre"), oracle.conv_bias(sd, f"{p}.conv_pre"), padding=3)
    x = x + F.conv1d(g, oracle.conv_weight(sd, f"{p}.cond"), oracle.conv_bias(sd, f"{p}.cond"))
    if taps is not None:
        taps["dec.conv_pre"] = x.clone()
    for i, (u, ku) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, oracle.LRELU_SLOPE)
        x = F.conv_transpose1d(x, oracle.conv_weight(sd, f"{p}.ups.{i}"), oracle.conv_bias(sd, f"{p}.ups.{i}"),
                               stride=u, padding=(ku - u) // 2)
        if taps is not None:
            taps[f"dec.ups.{i}"] = x.clone()
        acc = None
        for j, (k, d) in enumerate(zip(ks, ds)):
            r = oracle.resblock1(sd, f"{p}.resblocks.{i * len(ks) + j}", x, k, d)
            if taps is not None:
                taps[f"dec.resblocks.{i * len(ks) + j}"] = r.clone()
            acc = r if acc is None else acc + r
        x = acc / len(ks)
    x = F.leaky_relu(x)                                   # slope 0.01
    x = torch.cat([x[:, :, 1:2], x], dim=2)               # ReflectionPad1d((1, 0))
    x = F.conv1d(x, oracle.conv_weight(sd, f"{p}.conv_post"), oracle.conv_bias(sd, f"{p}.conv_post"), padding=3)
    if taps is not None:
        taps["dec.conv_post"] = x.clone()
    return oracle.istft_closed_form(x[:, :n_bins], x[:, n_bins:], n_fft, hop).unsqueeze(1)


def infer_from_g_single(sd, cfg, unit, g, noise, taps: Optional[dict] = None):
    """SynthesizerTrn.infer after the speaker encoder with the single-band decoder:
    unit (B, 256, T), g (B, gin, 1), noise (B, inter, T) -> (B, 1, 320*T) at the shipped rates."""
    sd = {k: v.float() for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    inter, hidden = int(cfg["inter_channels"]), int(cfg["hidden_channels"])
    with torch.no_grad():
        wn = oracle.wn_geometry(cfg)
        z_p, mu, logs = oracle.cond_normal_wn(sd, "enc_p", unit.float(), noise.float(), hidden, inter, None, taps,
                                              wn["kernel_size"], wn["enc_layers"])
        if taps is not None:
            taps["enc_p.mu"], taps["enc_p.logs"], taps["enc_p.z_p"] = mu.clone(), logs.clone(), z_p.clone()
        z = oracle.flow_reverse(sd, z_p, g.float(), inter, hidden, wn["n_flows"], taps, wn["kernel_size"], wn["flow_layers"])
        return decoder_forward_single(sd, cfg, z, g.float(), taps)


def post_frames_to_wave(post_fm, n_fft: int = 16, hop: int = 4):
    """(B, F, 18) frame-major conv_post output -> (B, 1, hop*(F-1)) via the oracle's closed-form iSTFT."""
    x = post_fm.double().transpose(1, 2)
    n_bins = n_fft // 2 + 1
    return oracle.istft_closed_form(x[:, :n_bins], x[:, n_bins:], n_fft, hop).unsqueeze(1)
