"""CPU tests of the single-band iSTFT decoder (iSTFT_Generator, istft_vits=True): plan / size queries / packer /
streaming refusal through the C ABI, the frozen host emulation refusing it, the new kernels' resource remarks,
and the test-side restatement (tests/istft_ref.py) against the reference's goldens."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ROOT

QVC_ERR_BAD_CONFIG = -2


def istft_manifest():
    with open(os.path.join(GOLDEN, "istft_manifest.json")) as f:
        return json.load(f)


def load_istft_case(name):
    entry = istft_manifest()[name]
    return entry, dict(np.load(os.path.join(GOLDEN, entry["file"])))


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from quickvc_official_amd import lib as L
    return L.load_library()


def _cfg(mc, dtype="f16"):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    model = q.SynthesizerTrn(641, 32, **mc)
    return model, L.make_config(dict(model.model_config, operand_dtype=dtype))


def _three_stage():
    import quickvc_official_amd as q
    return dict(q.ISTFT_MODEL_CONFIG, upsample_rates=[8, 5, 2], upsample_kernel_sizes=[16, 9, 4])


def test_istft_model_config_geometry():
    import quickvc_official_amd as q
    model = q.SynthesizerTrn(641, 32, **q.ISTFT_MODEL_CONFIG)
    assert model.samples_per_frame == 320 and model.model_config["decoder"] == "istft" and model.model_config["subbands"] == 1
    sd = model.state_dict()
    assert tuple(sd["dec.conv_post.weight_v"].shape) == (18, 128, 7)
    assert not any(k.startswith(("dec.subband_conv_post", "dec.multistream_conv_post", "dec.pqmf")) for k in sd)


@pytest.mark.parametrize("which", ["shipped", "three_stage"])
def test_plan_and_size_queries_accept_single_band(built, which):
    import quickvc_official_amd as q
    mc = q.ISTFT_MODEL_CONFIG if which == "shipped" else _three_stage()
    for dt in ("f16", "bf16x", "bf16"):
        _m, cfg = _cfg(mc, dt)
        info = (ctypes.c_int32 * 8)()
        assert built.qvc_plan_info(ctypes.byref(cfg), info) == 0
        assert info[4] == 1                                      # conv_post + single-band tail as one launch
        assert built.qvc_blob_bytes(ctypes.byref(cfg)) > 0
        assert built.qvc_workspace_bytes(ctypes.byref(cfg), 2, 50) > 0


def test_pack_weights_accepts_single_band_state_dict(built):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.synth import make_synthetic_state_dict
    for mc in (q.ISTFT_MODEL_CONFIG, _three_stage()):
        model, cfg = _cfg(mc)
        sd = make_synthetic_state_dict(model, 3)
        blob = L.pack_weights(built, cfg, sd)
        assert blob.numel() == built.qvc_blob_bytes(ctypes.byref(cfg)) and blob.float().abs().sum() > 0
    model, cfg = _cfg(q.ISTFT_MODEL_CONFIG)
    sd = make_synthetic_state_dict(model, 3)
    missing = {k: v for k, v in sd.items() if not k.startswith("dec.conv_post.")}
    with pytest.raises(L.QvcError, match="missing"):
        L.pack_weights(built, cfg, missing)
    # the packed conv_post changes with dec.conv_post (and only the single-band decoder reads that key)
    other = dict(sd); other["dec.conv_post.weight_v"] = sd["dec.conv_post.weight_v"] * -1.0
    assert not torch.equal(L.pack_weights(built, cfg, other), L.pack_weights(built, cfg, sd))


def test_validation_rules_of_single_band(built):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    info = (ctypes.c_int32 * 8)()

    def status(mc, **over):
        cfg = L.make_config(dict(q.SynthesizerTrn(641, 32, **mc).model_config, operand_dtype="f16"))
        for k, v in over.items():
            setattr(cfg, k, v)
        return built.qvc_plan_info(ctypes.byref(cfg), info)

    assert status(q.ISTFT_MODEL_CONFIG) == 0
    assert status(dict(q.ISTFT_MODEL_CONFIG, upsample_kernel_sizes=[19, 16])) == QVC_ERR_BAD_CONFIG   # k - s odd
    assert status(dict(q.ISTFT_MODEL_CONFIG, upsample_kernel_sizes=[20, 7])) == QVC_ERR_BAD_CONFIG    # k < s
    assert status(q.ISTFT_MODEL_CONFIG, subbands=4) == QVC_ERR_BAD_CONFIG
    assert status(q.ISTFT_MODEL_CONFIG, n_fft=32) == QVC_ERR_BAD_CONFIG
    assert status(q.ISTFT_MODEL_CONFIG, fir_taps=0) == 0                                             # ignored for one band
    # the band-synthesis decoders keep their own rules: the shipped geometry is legal, [10, 8]/[20, 16] is not
    assert status(q.DEFAULT_MODEL_CONFIG) == 0
    assert status(dict(q.DEFAULT_MODEL_CONFIG, upsample_rates=[10, 8], upsample_kernel_sizes=[20, 16])) == QVC_ERR_BAD_CONFIG


def test_streaming_rejects_single_band(built):
    import quickvc_official_amd as q
    _m, cfg = _cfg(q.ISTFT_MODEL_CONFIG)
    assert built.qvc_stream_state_bytes(ctypes.byref(cfg), 2, 20) == QVC_ERR_BAD_CONFIG
    assert built.qvc_stream_workspace_bytes(ctypes.byref(cfg), 2, 20) == QVC_ERR_BAD_CONFIG
    assert built.qvc_stream_lag_frames(ctypes.byref(cfg)) == QVC_ERR_BAD_CONFIG


def test_unmodified_host_emulation_refuses_single_band(built):
    """oracle/qvc_emu.cpp's backend only knows the four-band tail: the path must refuse the decoder on it
    (compile-time capability check) instead of writing a four-band tail into a 4x smaller output buffer."""
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.synth import make_synthetic_state_dict, make_synthetic_inputs
    from emu import load_emu
    mc = dict(q.MINI_MODEL_CONFIG, ms_istft_vits=False, istft_vits=True, upsample_rates=[10, 8], upsample_kernel_sizes=[20, 16])
    model, cfg = _cfg(mc)
    blob = L.pack_weights(built, cfg, make_synthetic_state_dict(model, 1))
    emu = load_emu()
    B, T = 1, 3
    unit, g, noise = make_synthetic_inputs(B, T, 256, mc["inter_channels"], mc["gin_channels"], seed0=0)
    n_ws = int(built.qvc_workspace_bytes(ctypes.byref(cfg), B, T))
    raw = torch.zeros(n_ws + 256, dtype=torch.uint8)
    shift = (-raw.data_ptr()) % 256
    ws = raw[shift:shift + n_ws]
    guard = 4096
    out = torch.full((B * 320 * T + guard,), 7.0)
    st = emu.qvc_emu_infer_batch(ctypes.byref(cfg), blob.data_ptr(), unit.contiguous().data_ptr(), g.contiguous().data_ptr(),
                                 noise.contiguous().data_ptr(), out.data_ptr(), B, T, ws.data_ptr(), n_ws)
    assert st == QVC_ERR_BAD_CONFIG
    assert torch.all(out == 7.0)                              # nothing was written


def test_single_band_kernels_have_no_scratch(built):
    """hipcc resource remarks of the new instantiations: no scratch, and the occupancy the launch geometry assumes
    (post_tail_kernel<T, 2, 1>: four 4-wave workgroups per CU = 4 waves per SIMD)."""
    hot = {"post_tail_kernelIDF16_Li2ELi1E": ("qvc_conv_f16", 4), "post_tail_kernelIDF16bLi2ELi1E": ("qvc_conv_bf16", 4),
           "istft_synth_kernelILi1E": ("qvc_small", 2)}
    seen = set()
    for tag, (obj, occ) in hot.items():
        name = None
        for line in open(os.path.join(ROOT, "quickvc-official_amd", "csrc", "_obj", obj + ".remarks.txt")):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            if not name or tag not in name:
                continue
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m:
                assert int(m.group(1)) == 0, (name, line)
                seen.add(tag)
            m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
            if m:
                assert int(m.group(1)) >= occ, (name, line)
    assert seen == set(hot), set(hot) - seen


@pytest.mark.parametrize("name", ["istft_mini", "istft_full_b1", "istft_ups3"])
def test_restatement_reproduces_reference_goldens(name):
    """tests/istft_ref.py (composed from the oracle's pieces) against the taps recorded from the reference's
    iSTFT_Generator: the bound the generator asserted, 2e-5 * max(1, |tap|max), on every stored tap."""
    import istft_ref
    from helpers import regenerate, subsample
    entry, arrays = load_istft_case(name)
    _m, sd, unit, g, noise = regenerate(entry)
    taps = {}
    o = istft_ref.infer_from_g_single(sd, entry["config"], unit, g.unsqueeze(-1), noise, taps)
    taps["o"] = o
    taps["enc_p.enc.out"] = taps["enc_p.enc.layer15.out"]
    for k in entry["taps"]:
        v = taps[k]
        assert tuple(v.shape) == tuple(arrays[k + "::shape"]), k
        mine = subsample(v, entry["subsample_limit"] if k != "o" else 1 << 30)
        ref = arrays[k]
        scale = float(np.abs(ref).max())
        assert float(np.abs(mine - ref).max()) <= 2e-5 * max(1.0, scale), k
    assert o.shape[-1] == 320 * entry["frames"]                 # hop 4 x prod(upsample_rates) = 320 in all three
