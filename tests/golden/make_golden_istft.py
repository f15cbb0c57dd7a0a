#!/usr/bin/env python3
"""Generate the single-band (iSTFT_Generator, istft_vits=True) golden vectors from the REFERENCE itself.

Run in the build container only (it needs /root/reference, which never travels):

    python tests/golden/make_golden_istft.py

Same procedure as make_golden.py (whose shims and reference runner it reuses): the unmodified reference
``models.py`` builds the single-band decoder, loads the deterministic synthetic checkpoint of this repo's
``SynthesizerTrn``, runs enc_p -> flow(reverse) -> dec with recorded noise, and its taps are stored as
data-only fixtures (large taps as strided subsamples).  Before writing, the test-side restatement
(tests/istft_ref.py) must reproduce every tap.  Seeds and configs go to istft_manifest.json.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden import REFERENCE, install_shims, run_reference, subsample   # noqa: E402


def main():
    install_shims()
    sys.path.insert(0, REFERENCE)
    import models as ref_models                                       # the reference, unmodified
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    import istft_ref

    torch.manual_seed(0)
    torch.set_num_threads(8)
    mini = dict(q.MINI_MODEL_CONFIG, ms_istft_vits=False, istft_vits=True, upsample_rates=[10, 8], upsample_kernel_sizes=[20, 16])
    three = dict(mini, upsample_rates=[8, 5, 2], upsample_kernel_sizes=[16, 9, 4])
    cases = [
        # name, model config, seed, batch, frames, subsample limit
        ("istft_mini", mini, 1234, 2, 12, 16384),
        ("istft_full_b1", q.ISTFT_MODEL_CONFIG, 1234, 1, 250, 4096),
        ("istft_ups3", three, 2345, 2, 9, 8192),
    ]
    manifest = {}
    for name, cfg, seed, batch, frames, limit in cases:
        print(f"== {name}: B={batch} T={frames}")
        ours = q.SynthesizerTrn(641, 32, **cfg)
        sd = make_synthetic_state_dict(ours, seed)
        ref_sd = ref_models.SynthesizerTrn(641, 32, **cfg).state_dict()
        assert type(ref_models.SynthesizerTrn(641, 32, **cfg).dec).__name__ == "iSTFT_Generator"
        assert list(ref_sd.keys()) == list(sd.keys()), "state-dict keys/order differ from the reference"
        for k in ref_sd:
            assert tuple(ref_sd[k].shape) == tuple(sd[k].shape), (k, ref_sd[k].shape, sd[k].shape)

        unit, g, noise = make_synthetic_inputs(batch, frames, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=0)
        _net, taps = run_reference(ref_models, cfg, sd, unit, g.unsqueeze(-1), noise)
        taps["dec.conv_post"] = taps.pop("dec.subband_conv_post")    # the runner's name for whichever conv_post ran
        spf = 4
        for u in cfg["upsample_rates"]:
            spf *= u
        assert tuple(taps["o"].shape) == (batch, 1, spf * frames), taps["o"].shape
        assert tuple(taps["dec.conv_post"].shape) == (batch, 18, frames * spf // 4 + 1)

        # pin the restatement against every tap
        otaps = {}
        o_re = istft_ref.infer_from_g_single(sd, cfg, unit, g.unsqueeze(-1), noise, otaps)
        otaps["o"] = o_re
        otaps["enc_p.enc.out"] = otaps["enc_p.enc.layer15.out"]
        worst = 0.0
        for k, v in taps.items():
            assert k in otaps, k
            diff = (otaps[k] - v).abs().max().item()
            scale = v.abs().max().item()
            worst = max(worst, diff / max(scale, 1e-9))
            assert diff <= 2e-5 * max(1.0, scale), f"{name}:{k}: restatement differs from the reference by {diff}"
        print(f"   restatement == reference on {len(taps)} taps (worst rel-to-max diff {worst:.2e})")

        arrays = {}
        for k, v in taps.items():
            arrays[k] = subsample(v, limit if k != "o" else 1 << 30)
            arrays[k + "::shape"] = np.asarray(v.shape, dtype=np.int64)
            arrays[k + "::sumsq"] = np.asarray([float(v.double().pow(2).sum())])
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 1 << 20, path
        manifest[name] = {"config": cfg, "weights_seed": seed, "inputs_seed0": 0, "batch": batch, "frames": frames,
                          "subsample_limit": limit, "file": f"{name}.npz", "taps": sorted(taps.keys())}
        print(f"   wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")

    with open(os.path.join(HERE, "istft_manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("done")


if __name__ == "__main__":
    main()
