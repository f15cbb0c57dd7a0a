"""The accepted configuration space on the host (no GPU): every row of tests/config_space.py through the host
emulation (oracle/qvc_emu.cpp: the real plan, the real packer, the product's launch sequence) against the fp32 oracle,
the route every row takes, and the configurations validate() must refuse.

Tolerance: the emulated whole path in f16 is >= 50 dB of waveform SNR per utterance against the oracle -- the bar the
emulation already meets on the shipped, mini and odd configurations (tests/test_host_side.py).  The bf16x emulation is
measured, not bounded here: its value decides whether the GPU test runs a row in bf16x (>= 43 dB, see
tests/test_gpu_config_space.py).  Both values are stored in the table and re-measured here to 0.5 dB, so that the table
the GPU test reads cannot go stale.

The emulation reports the KIND of every launch (emu.EmuWindowRun.steps); kernel names exist only on the device (the
timed entry point), where tests/test_gpu_config_space.py records them.
"""
import ctypes
from collections import Counter

import pytest
import torch

import config_space as CS
import emu as E
from helpers import snr_db

QVC_ERR_BAD_CONFIG = -2
ROUTES = {}          # row -> routes, filled by test_row_on_the_host, read by test_table_reaches_every_route


@pytest.fixture(scope="module")
def hip():
    from quickvc_official_amd import lib as L
    return L.load_library()          # host-only entry points (packer, size queries, plan info) work without a GPU


def _plan_info(hip, name):
    from quickvc_official_amd import lib as L
    _cfg, mc, _sd = CS.problem(name)
    c = L.make_config(dict(mc, operand_dtype="f16"))
    info, info_e = (ctypes.c_int32 * 8)(), (ctypes.c_int32 * 8)()
    assert hip.qvc_plan_info(ctypes.byref(c), info) == 0
    assert E.load_emu().qvc_emu_plan_flags(ctypes.byref(c), info_e) == 0 and list(info_e) == list(info)
    return list(info)


def _sequence(kinds):
    """The launch sequence, runs of one kind folded: 'gemv conv wn_stack x4 conv ...'."""
    out = []
    for k in kinds:
        if out and out[-1][0] == k:
            out[-1][1] += 1
        else:
            out.append([k, 1])
    return " ".join(k if n == 1 else f"{k} x{n}" for k, n in out)


@pytest.mark.parametrize("name", list(CS.ROWS))
def test_row_on_the_host(hip, name):
    from quickvc_official_amd import lib as L
    cfg, mc, sd = CS.problem(name)
    unit, g, noise = CS.inputs(name)
    row = CS.ROWS[name]
    c = L.make_config(dict(mc, operand_dtype="f16"))
    assert (c.wn_kernel_size, c.enc_layers, c.flow_layers, c.n_flows) == (row["wn"] or CS.WN_DEFAULT)
    # every size query of the conversion path and the posterior encoder accepts the configuration
    cp = ctypes.byref(c)
    sizes = dict(blob=hip.qvc_blob_bytes(cp), workspace=hip.qvc_workspace_bytes(cp, CS.B, CS.T),
                 fanout=hip.qvc_fanout_workspace_bytes(cp, 1, CS.B, CS.T), encq_blob=hip.qvc_encq_blob_bytes(cp))
    assert all(v > 0 for v in sizes.values()), sizes
    # the route
    info = _plan_info(hip, name)
    ROUTES[name] = CS.routes(cfg, info)
    ref, _taps = CS.reference(name)
    assert ref.shape == (CS.B, 1, CS.T * CS.samples_per_frame(cfg)) and bool(torch.isfinite(ref).all())
    if not row["emulated"]:
        # the single-band decoder: the emulation's backend is frozen before it and the path refuses it there, so the row has
        # the oracle's assertions on the GPU only.  Checked, so that the flag cannot outlive that state.
        with pytest.raises(AssertionError, match="unsupported model configuration"):
            E.emu_infer(mc, sd, unit, g, noise, "f16")
        assert row["emu_f16"] is None and row["emu_bf16x"] is None
        print(f"{name}: not emulated; plan info {info}; routes {sorted(ROUTES[name])}")
        return
    n, kinds = E.window_run(mc, sd, unit, g, noise, dtype="f16", lens=CS.RAGGED).steps()
    assert n == len(kinds) > 0
    count = Counter(kinds)
    # config_space.wn_windows and routes restate the plan: checked against the launches the path issues
    w = CS.wn_windows(cfg)
    want_stack = (c.enc_layers // w["enc"][0] if w["enc"] else 0) + c.n_flows * (c.flow_layers // w["flow"][0] if w["flow"] else 0)
    want_layer = (0 if w["enc"] else c.enc_layers) + c.n_flows * (0 if w["flow"] else c.flow_layers)
    assert (count["wn_stack"], count["wn"]) == (want_stack, want_layer), (dict(count), w)
    assert (count["post_tail"], count["tail"]) == ((1, 0) if info[4] else (0, 1)), (dict(count), info)
    assert count["sample"] == (0 if info[0] else 1)
    n_pairs = 3 * len(cfg["upsample_rates"])
    assert count["pair3"] == n_pairs if info[7] else count["pair3"] < 3 * n_pairs, (dict(count), info)
    print(f"{name}: {len(kinds)} launches: {_sequence(kinds)}; plan info {info}; routes {sorted(ROUTES[name])}")
    # the emulated whole path against the oracle
    got = {}
    for dt in ("f16", "bf16x"):
        out = E.emu_infer(mc, sd, unit, g, noise, dt)
        got[dt] = [snr_db(ref[b], out[b]) for b in range(CS.B)]
    print(f"{name}: emulation vs oracle f16 {got['f16']}, bf16x {got['bf16x']}")
    assert min(got["f16"]) >= 50.0, got
    for dt in ("f16", "bf16x"):
        stored = row["emu_" + dt]
        assert stored is not None and len(stored) == CS.B, f"{name}: no emu_{dt} in the table (measured {got[dt]})"
        assert all(abs(a - b) <= 0.5 for a, b in zip(stored, got[dt])), (name, dt, stored, got[dt])


def test_table_reaches_every_route(hip):
    """The rows together take every route the plan can choose; a table that clusters again fails here."""
    reached = {}
    for name in CS.ROWS:
        r = ROUTES.get(name)
        if r is None:                                    # this test run alone
            r = CS.routes(CS.problem(name)[0], _plan_info(hip, name))
        for route in r:
            reached.setdefault(route, []).append(name)
    for route in sorted(reached):
        print(f"{route}: {', '.join(reached[route])}")
    assert set(reached) >= CS.REQUIRED_ROUTES, sorted(CS.REQUIRED_ROUTES - set(reached))
    assert 20 <= len(CS.ROWS) <= 35


def _tensors(sd):
    from quickvc_official_amd import lib as L
    keep, arr = [], (L.QvcTensor * len(sd))()
    for i, (name, t) in enumerate(sd.items()):
        tc = t.detach().float().contiguous()
        keep.append(tc)
        arr[i].name, arr[i].data, arr[i].ndim = name.encode(), tc.data_ptr(), tc.dim()
        for d in range(tc.dim()):
            arr[i].shape[d] = tc.shape[d]
    return keep, arr


@pytest.mark.parametrize("name", list(CS.NEGATIVE) + list(CS.NEGATIVE_FIELDS))
def test_refused_configurations(hip, name):
    """One step outside each bound of validate(), and the stride-1 first stage of the multistream / multiband decoders
    (a ConvTranspose1d the reference cannot build): every size query and the packer answer QVC_ERR_BAD_CONFIG."""
    c = CS.negative_config(name)
    cp = ctypes.byref(c)
    got = dict(blob=hip.qvc_blob_bytes(cp), workspace=hip.qvc_workspace_bytes(cp, 2, 23), fanout=hip.qvc_fanout_workspace_bytes(cp, 1, 2, 23),
               stream_state=hip.qvc_stream_state_bytes(cp, 2, 16), stream_workspace=hip.qvc_stream_workspace_bytes(cp, 2, 16),
               encq_blob=hip.qvc_encq_blob_bytes(cp))
    _cfg, _mc, sd = CS.problem("one_up8")
    keep, arr = _tensors({k: v for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point() and v.dim() <= 4})
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    got["pack_weights"] = hip.qvc_pack_weights(cp, arr, len(arr), buf.data_ptr(), buf.numel())
    got["encq_pack_weights"] = hip.qvc_encq_pack_weights(cp, arr, len(arr), buf.data_ptr(), buf.numel())
    info = (ctypes.c_int32 * 8)()
    got["plan_info"] = hip.qvc_plan_info(cp, info)
    assert all(v == QVC_ERR_BAD_CONFIG for v in got.values()), got


def test_the_base_of_the_negative_table_is_accepted(hip):
    """... so that each entry is refused for its one change."""
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    model = q.SynthesizerTrn(641, 32, **dict(q.DEFAULT_MODEL_CONFIG, **CS.BASE))
    assert hip.qvc_blob_bytes(ctypes.byref(L.make_config(model.model_config))) > 0
    # the neighbours of the refused stride-1 first stage that PyTorch can build stay accepted
    ok = [dict(upsample_rates=[2, 1], upsample_kernel_sizes=[3, 1]),                                   # stride 1 second
          dict(decoder="istft", subbands=1, upsample_rates=[1, 4], upsample_kernel_sizes=[3, 16])]    # single band: no output_padding
    for over in ok:
        assert hip.qvc_blob_bytes(ctypes.byref(L.make_config(dict(model.model_config, **over)))) > 0, over


def test_oracle_refuses_what_validate_refuses_for_stride_one():
    """The reason for the refusal, executed: the reference's own constructor call for that stage raises."""
    x = torch.zeros(1, 4, 5)
    w = torch.zeros(4, 2, 2)
    with pytest.raises(RuntimeError):
        torch.nn.functional.conv_transpose1d(x, w, stride=1, padding=1, output_padding=1)
