"""The model geometries the suite runs out of the space validate() accepts (csrc/qvc_plan.h).

A helper module, not a conftest: tests/test_config_space_host.py (emulation against the oracle, routes, the negative
table), tests/test_gpu_config_space.py (the kernels against the oracle and the emulation) and the extended cases of
tests/test_gpu_memory_contract.py import it.

ROWS is the table.  Every row is the base (DEFAULT_MODEL_CONFIG at inter 32, hidden 32, upsample_initial_channel 64,
gin 16) with `over` applied, and optionally a WaveNet geometry `wn` = (wn_kernel_size, enc_layers, flow_layers, n_flows)
-- the four optional keys lib.make_config reads; the reference's constructor pins them at (5, 16, 4, 4), so those rows
have no counterpart in the reference and take their weights from wn_state_dict() below.

Measured values, dB of waveform SNR against the fp32 oracle per batch member at B 2, T 23, inputs seed 71:
  emu_f16, emu_bf16x   the host emulation (oracle/qvc_emu.cpp), measured on a CPU; test_config_space_host.py re-measures
                       them and fails when the table is stale;
  gpu_f16, gpu_bf16x   the kernels, measured on an MI355X (None: not run -- bf16x runs only where emu_bf16x >= 43 dB).
The single-band rows (`emulated` False) have no emulated values: the emulation's backend is frozen before that decoder and
the path refuses it there (tests/test_istft_single_band.py), so they run in f16 against the oracle only.
"""
import functools

import torch

B, T, RAGGED = 2, 23, [23, 9]     # 23: a multiple of no tile size; 9: ends inside the first tile of every stage
WEIGHTS_SEED, WN_SEED, INPUTS_SEED = 311, 5, 71

BASE = dict(inter_channels=32, hidden_channels=32, upsample_initial_channel=64, gin_channels=16)
_ISTFT = dict(ms_istft_vits=False, istft_vits=True, subbands=1)


def _row(over=None, wn=None, emu_f16=None, emu_bf16x=None, gpu_f16=None, gpu_bf16x=None, why=""):
    over = over or {}
    # the host emulation is frozen before the single-band decoder and refuses it (tests/test_istft_single_band.py):
    # those rows have no emulated values and no per-launch comparison, only the oracle's assertions
    return dict(over=over, wn=wn, emulated=not over.get("istft_vits", False), emu_f16=emu_f16, emu_bf16x=emu_bf16x, gpu_f16=gpu_f16,
                gpu_bf16x=gpu_bf16x, why=why)


ROWS = {
    # ---- decoder and width rows (reachable from SynthesizerTrn)
    "up16_k17_up2_k2": _row(dict(upsample_rates=[16, 2], upsample_kernel_sizes=[17, 2]), emu_f16=[54.3, 53.2], emu_bf16x=[48.1, 47.7],
                            gpu_f16=[53.8, 53.6], gpu_bf16x=[47.9, 48.0], why="stride 16 first, k == s second"),
    "up2_k63_up3_k63": _row(dict(upsample_rates=[2, 3], upsample_kernel_sizes=[63, 63]), emu_f16=[51.8, 51.2], emu_bf16x=[45.6, 46.2],
                            gpu_f16=[50.8, 51.6], gpu_bf16x=[45.9, 45.9], why="kernel 63: 32 and 21 polyphase taps"),
    "up3_k4_up16_k64": _row(dict(upsample_rates=[3, 16], upsample_kernel_sizes=[4, 64]), emu_f16=[54.3, 54.3], emu_bf16x=[48.1, 48.0],
                            gpu_f16=[53.9, 54.9], gpu_bf16x=[48.1, 47.9], why="stride 16 with kernel 64"),
    "one_up8": _row(dict(upsample_rates=[8], upsample_kernel_sizes=[15]), emu_f16=[53.6, 53.7], emu_bf16x=[48.8, 48.9],
                    gpu_f16=[53.3, 53.8], gpu_bf16x=[48.7, 48.9], why="one up-sampler"),
    "rb_k1_k15_k13": _row(dict(resblock_kernel_sizes=[1, 15, 13], resblock_dilation_sizes=[[1, 1, 1], [16, 1, 7], [2, 16, 16]]),
                          emu_f16=[53.9, 53.6], emu_bf16x=[48.4, 48.4],
                          gpu_f16=[54.0, 53.6], gpu_bf16x=[48.0, 48.0], why="ResBlock kernel 1, and k 15 at dilation 16: a 224-row halo"),
    "rb_k9_d16": _row(dict(resblock_kernel_sizes=[9, 9, 9], resblock_dilation_sizes=[[16, 16, 16]] * 3), emu_f16=[54.2, 54.3], emu_bf16x=[47.5, 48.3],
                      gpu_f16=[54.2, 54.6], gpu_bf16x=[48.1, 48.5], why="every dilation 16"),
    "init32": _row(dict(upsample_initial_channel=32), emu_f16=[53.6, 53.7], emu_bf16x=[47.0, 48.0],
                   gpu_f16=[52.8, 53.5], gpu_bf16x=[46.5, 47.9], why="an 8-channel last stage"),
    "all_min": _row(dict(inter_channels=8, hidden_channels=8, upsample_initial_channel=32, gin_channels=4), emu_f16=[52.4, 52.9], emu_bf16x=[45.2, 46.5],
                    gpu_f16=[52.3, 53.0], gpu_bf16x=[44.1, 46.4], why="every minimum"),
    "h256_gin512": _row(dict(inter_channels=8, hidden_channels=256, gin_channels=512), emu_f16=[53.6, 52.6], emu_bf16x=[46.8, 44.6],
                        gpu_f16=[53.7, 54.7], gpu_bf16x=[47.1, 45.4], why="cond_gemv at gin 512, 16-wave WaveNet with pre / post fused into the stack launch"),
    "inter256_h8": _row(dict(inter_channels=256, hidden_channels=8), emu_f16=[51.8, 54.5], emu_bf16x=[45.7, 47.2],
                        gpu_f16=[52.2, 54.7], gpu_bf16x=[45.8, 47.3], why="natural projection rows + sample launch; inter > hidden"),
    "init1024": _row(dict(upsample_initial_channel=1024), emu_f16=[53.3, 53.6], emu_bf16x=[47.1, 47.1],
                     gpu_f16=[53.2, 54.0], gpu_bf16x=[47.0, 47.4], why="8-wave pair layout at MF 4 (512 channels)"),
    "init768": _row(dict(upsample_initial_channel=768), emu_f16=[53.1, 52.7], emu_bf16x=[46.2, 46.2],
                    gpu_f16=[52.8, 53.4], gpu_bf16x=[46.3, 46.2], why="8-wave pair layout at MF 3 (384 channels)"),
    "ch104": _row(dict(upsample_initial_channel=416, hidden_channels=104, inter_channels=72, gin_channels=20),
                  emu_f16=[53.4, 54.2], emu_bf16x=[48.0, 47.8],
                  gpu_f16=[54.1, 54.3], gpu_bf16x=[48.1, 47.7], why="channel counts that are multiples of 8 only"),
    "mb_up16_up1": _row(dict(ms_istft_vits=False, mb_istft_vits=True, upsample_rates=[16, 1], upsample_kernel_sizes=[17, 1]),
                        emu_f16=[51.8, 51.3], emu_bf16x=[45.8, 45.6],
                        gpu_f16=[51.4, 51.9], gpu_bf16x=[45.8, 45.8], why="multiband decoder; a stride-1 second stage"),
    "one_up4_init768": _row(dict(upsample_rates=[4], upsample_kernel_sizes=[7], upsample_initial_channel=768),
                            emu_f16=[53.0, 53.4], emu_bf16x=[48.7, 48.6],
                            gpu_f16=[52.6, 54.4], gpu_bf16x=[48.4, 48.6], why="a 384-channel LAST stage: conv_post and the tail as two launches"),
    "one_up8_init528": _row(dict(upsample_rates=[8], upsample_kernel_sizes=[9], upsample_initial_channel=528),
                            emu_f16=[53.4, 54.0], emu_bf16x=[53.4, 54.0],
                            gpu_f16=[53.4, 54.5], gpu_bf16x=[53.4, 54.5], why="264 channels: three row chunks, so conv1 / conv2 as launches of their own (unfused pairs)"),
    "istft_ups3": _row(dict(_ISTFT, upsample_rates=[2, 1, 16], upsample_kernel_sizes=[4, 3, 64]),
                       gpu_f16=[53.3, 53.3], gpu_bf16x=None, why="single band, three up-samplers: stride 1 in the middle, stride 16 with kernel 64 (k - s even)"),
    # (make_synthetic_state_dict scales an up-sampler's weights for stride 4.5: its gain is sqrt(4.5 / stride) whatever the
    # kernel.  Four small strides -- [2, 3, 1, 4] was tried -- multiply to 4x, conv_post's log-magnitudes reach 12 and exp()
    # turns f16's rounding into 40-46 dB on the GPU and 45-49 dB in an f16-rounded oracle alike; these strides multiply to 1.3x)
    "istft_ups4": _row(dict(_ISTFT, upsample_rates=[16, 1, 8, 2], upsample_kernel_sizes=[32, 3, 16, 4], upsample_initial_channel=128),
                       gpu_f16=[54.7, 55.4], gpu_bf16x=None, why="single band, four up-samplers, a stride-1 second stage"),
    # ---- WaveNet rows (C ABI / make_config keys only)
    "wn_k3": _row(wn=(3, 16, 4, 4), emu_f16=[58.3, 58.3], emu_bf16x=[49.4, 48.7],
                  gpu_f16=[58.6, 58.7], gpu_bf16x=[49.5, 49.2], why="taps 3"),
    "wn_k1": _row(wn=(1, 16, 4, 4), emu_f16=[59.0, 58.3], emu_bf16x=[49.6, 48.7],
                  gpu_f16=[59.1, 58.4], gpu_bf16x=[49.5, 48.9], why="taps 1: no halo"),
    "wn_k7": _row(wn=(7, 16, 4, 4), emu_f16=[59.0, 58.8], emu_bf16x=[49.6, 48.5],
                  gpu_f16=[58.9, 58.4], gpu_bf16x=[49.3, 48.6], why="taps 7: a 4-fragment window, no stack kernel"),
    "wn_k15": _row(wn=(15, 16, 4, 4), emu_f16=[58.7, 58.9], emu_bf16x=[49.4, 49.4],
                   gpu_f16=[58.9, 58.8], gpu_bf16x=[49.1, 49.3], why="taps 15: 4 layers fill the 6-fragment window"),
    "wn_enc1_flow1": _row(wn=(5, 1, 1, 4), emu_f16=[60.2, 60.4], emu_bf16x=[49.9, 49.4],
                          gpu_f16=[60.0, 60.2], gpu_bf16x=[49.8, 49.7], why="one-layer stacks: the first layer is the last"),
    "wn_enc3_flow2": _row(wn=(5, 3, 2, 4), emu_f16=[60.3, 60.4], emu_bf16x=[49.6, 49.5],
                          gpu_f16=[60.2, 60.3], gpu_bf16x=[49.8, 49.4], why="stacks of 3 and 2 layers in one launch"),
    "wn_enc17_flow5": _row(wn=(5, 17, 5, 4), emu_f16=[58.6, 59.0], emu_bf16x=[49.0, 48.9],
                           gpu_f16=[58.8, 59.0], gpu_bf16x=[49.0, 48.8], why="17 layers (more than a launch holds) and a 4-fragment flow window"),
    "wn_enc64_flow8_f2": _row(wn=(5, 64, 8, 2), emu_f16=[55.1, 54.5], emu_bf16x=[48.0, 47.5],
                              gpu_f16=[55.6, 55.4], gpu_bf16x=[48.2, 47.4], why="the layer maxima's neighbourhood: 16 and 2 chunks of 4; two flows"),
    "wn_flow16": _row(wn=(5, 16, 16, 4), emu_f16=[58.4, 57.8], emu_bf16x=[49.1, 48.9],
                      gpu_f16=[58.6, 58.1], gpu_bf16x=[49.2, 48.9], why="deep coupling layers: 4 launches each, pre / post as convs"),
    "wn_k9_flow2": _row(wn=(9, 16, 2, 4), emu_f16=[58.6, 59.0], emu_bf16x=[49.5, 48.9],
                        gpu_f16=[58.6, 58.8], gpu_bf16x=[49.3, 49.2], why="taps 9: per-layer enc_p, 2-layer coupling stacks"),
    "wn_flows2": _row(wn=(5, 16, 4, 2), emu_f16=[58.9, 58.9], emu_bf16x=[49.8, 49.4],
                      gpu_f16=[58.8, 58.8], gpu_bf16x=[49.6, 49.4], why="two flows"),
    "wn_flows6": _row(wn=(5, 16, 4, 6), emu_f16=[58.2, 58.4], emu_bf16x=[49.2, 49.0],
                      gpu_f16=[58.7, 58.6], gpu_bf16x=[49.2, 49.1], why="six flows"),
    "wn_flows16": _row(wn=(5, 4, 4, 16), emu_f16=[58.8, 58.5], emu_bf16x=[49.1, 49.1],
                       gpu_f16=[58.5, 58.6], gpu_bf16x=[49.1, 49.1], why="sixteen flows"),
    "wn_enc14": _row(wn=(5, 14, 4, 4), emu_f16=[59.0, 59.1], emu_bf16x=[49.1, 49.3],
                     gpu_f16=[58.9, 59.2], gpu_bf16x=[49.4, 49.3], why="a whole 14-layer stack in one launch, 6-fragment window"),
    "wn_k15_h256": _row(dict(hidden_channels=256), wn=(15, 16, 4, 4), emu_f16=[60.7, 60.3], emu_bf16x=[51.1, 50.5],
                        gpu_f16=[60.1, 60.4], gpu_bf16x=[51.1, 50.5], why="the widest WaveNet at the longest kernel: pre / post fused into the 6-fragment stack launch"),
}

WN_DEFAULT = (5, 16, 4, 4)        # models.py:582-584


def constructor_config(name):
    """The reference-style constructor dict of a row (what SynthesizerTrn(**cfg) and the oracle take), the WaveNet keys included."""
    import quickvc_official_amd as q
    row = ROWS[name]
    cfg = dict(q.DEFAULT_MODEL_CONFIG, **BASE)
    cfg.update(row["over"])
    if row["wn"] is not None:
        cfg.update(zip(("wn_kernel_size", "enc_layers", "flow_layers", "n_flows"), row["wn"]))
    return cfg


def wn_state_dict(sd, cfg, seed=WN_SEED):
    """`sd` (from make_synthetic_state_dict on the reference's fixed geometry) with enc_p.enc.* and flow.flows.{2i}.*
    replaced by seeded tensors for cfg's (wn_kernel_size, enc_layers, flow_layers, n_flows): in_layers (2h, h, k),
    res_skip (2h, h, 1) with h rows on the last layer, cond_layer (2h * layers, gin, 1) on the flows, pre (h, inter / 2, 1)
    and post (inter / 2, h, 1).  weight_g = ||v|| times a factor in [0.8, 1.2], so the weight-norm fold is no no-op."""
    k, enc_layers, flow_layers, n_flows = (int(cfg.get(key, d)) for key, d in zip(("wn_kernel_size", "enc_layers", "flow_layers", "n_flows"), WN_DEFAULT))
    H, C, gin = int(cfg["hidden_channels"]), int(cfg["inter_channels"]), int(cfg["gin_channels"])
    gen = torch.Generator().manual_seed(seed)
    sd = {key: v for key, v in sd.items() if not key.startswith(("enc_p.enc.", "flow."))}

    def normed(name, v, bias):
        sd[name + ".weight_v"] = v
        sd[name + ".weight_g"] = v.flatten(1).norm(dim=1).reshape(-1, 1, 1) * (0.8 + 0.4 * torch.rand(v.shape[0], 1, 1, generator=gen))
        sd[name + ".bias"] = bias

    def stack(prefix, layers, cond):
        for i in range(layers):
            normed(f"{prefix}.in_layers.{i}", torch.randn(2 * H, H, k, generator=gen) / (H * k) ** 0.5, 0.1 * torch.randn(2 * H, generator=gen))
            rows = 2 * H if i < layers - 1 else H
            normed(f"{prefix}.res_skip_layers.{i}", 0.5 * torch.randn(rows, H, 1, generator=gen) / H ** 0.5, 0.1 * torch.randn(rows, generator=gen))
        if cond:
            normed(f"{prefix}.cond_layer", torch.randn(2 * H * layers, gin, 1, generator=gen) / gin ** 0.5, 0.1 * torch.randn(2 * H * layers, generator=gen))

    stack("enc_p.enc", enc_layers, False)
    for i in range(n_flows):
        p = f"flow.flows.{2 * i}"
        sd[f"{p}.pre.weight"] = torch.randn(H, C // 2, 1, generator=gen) / (C // 2) ** 0.5
        sd[f"{p}.pre.bias"] = 0.05 * torch.randn(H, generator=gen)
        stack(f"{p}.enc", flow_layers, True)
        sd[f"{p}.post.weight"] = 0.5 * torch.randn(C // 2, H, 1, generator=gen) / H ** 0.5
        sd[f"{p}.post.bias"] = 0.05 * torch.randn(C // 2, generator=gen)
    return sd


@functools.lru_cache(maxsize=None)
def problem(name):
    """(constructor config, model_config for lib.make_config / QvcEngine, state dict) of a row."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict
    cfg = constructor_config(name)
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, WEIGHTS_SEED)
    mc = dict(model.model_config)
    if ROWS[name]["wn"] is not None:
        mc.update({key: cfg[key] for key in ("wn_kernel_size", "enc_layers", "flow_layers", "n_flows")})
        sd = wn_state_dict(sd, cfg)
    return cfg, mc, sd


@functools.lru_cache(maxsize=None)
def inputs(name, batch=B, frames=T):
    """(unit, g, noise) of a row; treat them as read-only (they are shared)."""
    from quickvc_official_amd.synth import make_synthetic_inputs
    cfg = constructor_config(name)
    return make_synthetic_inputs(batch, frames, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=INPUTS_SEED)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(waveform (B, 1, N), taps) of the fp32 oracle for inputs(name), computed once; read-only."""
    import qvc_oracle as oracle
    import istft_ref
    cfg, _mc, sd = problem(name)
    unit, g, noise = inputs(name)
    taps = {}
    fn = istft_ref.infer_from_g_single if cfg.get("istft_vits") else oracle.infer_from_g
    ref = fn(sd, cfg, unit, g.unsqueeze(-1), noise, taps)
    return ref, taps


def samples_per_frame(cfg):
    n = cfg["gen_istft_hop_size"] * (1 if cfg.get("istft_vits") else cfg["subbands"])
    for u in cfg["upsample_rates"]:
        n *= u
    return n


# ---------------------------------------------------------------- routes
def wn_windows(cfg):
    """Python restatement of the plan's WaveNet choice (csrc/qvc_plan.h: wn_stack_nf, wn_stack_ok; qvc_kernels.h: wn_chunk)
    -> dict(enc=(chunk, nf) or None, flow=(chunk, nf) or None): layers per whole-stack launch and its window in 16-column
    fragments, None where the stack runs one launch per layer.  The host test checks it against the step kinds."""
    k, enc_layers, flow_layers, _n = (int(cfg.get(key, d)) for key, d in zip(("wn_kernel_size", "enc_layers", "flow_layers", "n_flows"), WN_DEFAULT))

    def one(layers):
        chunk = 4 if layers % 4 == 0 else layers
        nf = -(-(32 + (k - 1) * chunk) // 16)
        halo = (k - 1) // 2 * chunk
        ok = chunk <= 16 and (nf == 3 or (nf == 6 and halo >= 16 and halo + 32 <= 64))
        return (chunk, nf) if ok else None
    return dict(enc=one(enc_layers), flow=one(flow_layers))


def routes(cfg, info):
    """The set of route names a row takes, from its config and qvc_plan_info (the host test checks both against the step
    kinds the emulation reports, where the emulation runs the row)."""
    w = wn_windows(cfg)
    found = set()
    for part in ("enc", "flow"):
        found.add("wn_per_layer" if w[part] is None else f"wn_stack_nf{w[part][1]}")
    found.add("pairs_fused" if info[7] else "pairs_unfused")
    if info[7]:
        for i in range(min(len(cfg["upsample_rates"]), 2)):
            found.add(f"pair_waves{info[5 + i]}")
    found.add("tail_one_launch" if info[4] else "tail_two_launches")
    found.add("proj_paired" if info[0] else "proj_natural")
    return found


REQUIRED_ROUTES = {"wn_per_layer", "wn_stack_nf3", "wn_stack_nf6", "pairs_fused", "pairs_unfused", "pair_waves4", "pair_waves8",
                   "tail_one_launch", "tail_two_launches", "proj_paired", "proj_natural"}


# ---------------------------------------------------------------- configurations validate() must refuse
def _c(**over):
    return over


# name -> overrides of the base model_config (make_config keys); every one a single step outside a bound of validate()
NEGATIVE = {
    "inter_not_x8": _c(inter_channels=36), "hidden_not_x8": _c(hidden_channels=36), "unit_not_x8": _c(unit_channels=252),
    "inter_0": _c(inter_channels=0), "hidden_0": _c(hidden_channels=0), "gin_0": _c(gin_channels=0), "unit_0": _c(unit_channels=0),
    "hidden_264": _c(hidden_channels=264), "gin_not_x4": _c(gin_channels=18), "gin_516": _c(gin_channels=516),
    "wn_k0": _c(wn_kernel_size=0), "wn_k4": _c(wn_kernel_size=4), "wn_k17": _c(wn_kernel_size=17),
    "enc_layers_0": _c(enc_layers=0), "enc_layers_65": _c(enc_layers=65), "flow_layers_0": _c(flow_layers=0), "flow_layers_65": _c(flow_layers=65),
    "n_flows_0": _c(n_flows=0), "n_flows_3": _c(n_flows=3), "n_flows_18": _c(n_flows=18),
    "n_ups_0": _c(upsample_rates=[], upsample_kernel_sizes=[]),
    "resblocks_2": _c(resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3, 5]] * 2),
    "resblocks_4": _c(resblock_kernel_sizes=[3, 7, 11, 3], resblock_dilation_sizes=[[1, 3, 5]] * 4),
    "init_0": _c(upsample_initial_channel=0), "init_not_x8": _c(upsample_initial_channel=68),
    "init_stage_not_x8": _c(upsample_initial_channel=48),          # 48 -> 24 -> 12
    "rate_0": _c(upsample_rates=[0, 4], upsample_kernel_sizes=[1, 16]), "rate_17": _c(upsample_rates=[17, 2], upsample_kernel_sizes=[18, 2]),
    "up_k_below_rate": _c(upsample_rates=[5, 4], upsample_kernel_sizes=[4, 16]), "up_k_65": _c(upsample_rates=[4, 4], upsample_kernel_sizes=[65, 16]),
    "up_k_parity_stage0": _c(upsample_rates=[5, 4], upsample_kernel_sizes=[15, 16]),       # k - s + 1 - i odd
    "up_k_parity_stage1": _c(upsample_rates=[5, 4], upsample_kernel_sizes=[16, 15]),
    "ms_three_ups": _c(upsample_rates=[2, 2, 2], upsample_kernel_sizes=[3, 2, 2]),          # output_padding 1 - i < 0
    "istft_k_parity": _c(decoder="istft", subbands=1, upsample_rates=[5, 4], upsample_kernel_sizes=[16, 16]),
    "rb_k0": _c(resblock_kernel_sizes=[0, 7, 11]), "rb_k4": _c(resblock_kernel_sizes=[3, 4, 11]), "rb_k17": _c(resblock_kernel_sizes=[3, 7, 17]),
    "rb_dil_0": _c(resblock_dilation_sizes=[[1, 3, 5], [0, 3, 5], [1, 3, 5]]), "rb_dil_17": _c(resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 17]]),
    "n_fft_32": _c(gen_istft_n_fft=32), "hop_8": _c(gen_istft_hop_size=8),
    "ms_subbands_2": _c(subbands=2), "istft_subbands_4": _c(decoder="istft", subbands=4, upsample_rates=[10, 8], upsample_kernel_sizes=[20, 16]),
    # the stride-1 FIRST stage of the multistream / multiband decoders: ConvTranspose1d(output_padding=1, stride=1) does
    # not exist (PyTorch refuses output_padding >= stride), so the reference cannot build the model
    "ms_stride1_first": _c(upsample_rates=[1, 1], upsample_kernel_sizes=[2, 1]),
    "mb_stride1_first": _c(decoder="multiband", upsample_rates=[1, 4], upsample_kernel_sizes=[2, 16]),
    "ms_stride1_only": _c(upsample_rates=[1], upsample_kernel_sizes=[2]),
}
# fields make_config does not read from the dict: set on the qvc_config itself
NEGATIVE_FIELDS = {"decoder_3": dict(decoder=3), "decoder_neg": dict(decoder=-1), "operand_dtype_3": dict(operand_dtype=3),
                   "fir_taps_31": dict(fir_taps=31), "n_resblocks_0": dict(n_resblocks=0), "n_ups_5": dict(n_ups=5)}


def negative_config(name):
    """qvc_config of one entry of the negative table."""
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    model = q.SynthesizerTrn(641, 32, **dict(q.DEFAULT_MODEL_CONFIG, **BASE))
    mc = dict(model.model_config)
    if name in NEGATIVE_FIELDS:
        c = L.make_config(mc)
        for field, value in NEGATIVE_FIELDS[name].items():
            setattr(c, field, value)
        return c
    mc.update(NEGATIVE[name])
    return L.make_config(mc)
