"""The memory contract of every entry point of include/qvc.h, on an MI355X (run with -m gpu).

Every caller-owned buffer of a call -- inputs, device length / map arrays and blobs, not only outputs -- sits in its own
guarded arena (tests/memguard.py), outputs and scratch start from a fill, and the raw C ABI is called with
workspace_bytes / state_bytes exactly as the size query returns them.  Per fill (0x00, 0x3C, 0xFF = NaN in every type):
status 0; every guard intact; inputs and blobs byte-identical to before; for whole-path calls the workspace bytes that
lie in no buffer of the workspace map untouched.  Across the fills: every output bit-identical (a result that depends
on a byte this call did not write differs), and the 0x00 run torch.equal to what the ordinary QvcEngine /
StreamConverter / front-end call returns for the same inputs (so the harness calls the ABI correctly).  Under 0xFF the
padding of every ragged input is NaN as well, and rows past a member's end are exactly zero where the header says so.

Shapes are the smallest that still take every tile edge.  Nothing here passes a buffer smaller than its query says: an
over-run this file can observe stays inside an arena.

What it cannot see: a read outside a buffer whose value is then discarded, and an over-run from one workspace
sub-buffer into the next (left to tests/test_gpu_step_parity.py).
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import config_space as CS
import emu as E
import memguard as M
import stepcheck as S
from helpers import GOLDEN, load_case, regenerate

pytestmark = pytest.mark.gpu

DEBUG_DEFAULTS = {"post_tail": 1, "post_tail_nf": 4, "pair_wide_launch": 1, "pair_cm4": 1, "conv_cl": 1, "wn_chunk": 0,
                  "pair_chain3": 0, "wn_kernel": 0, "launch_stop": -1}
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from quickvc_official_amd import lib as L
    l = L.load_library()                       # raises if the HIP library is missing: no fallback
    assert l.qvc_device_check() == 0
    return l


@pytest.fixture(autouse=True)
def _debug_switches_at_defaults():
    from quickvc_official_amd import lib as L
    for k, v in DEBUG_DEFAULTS.items():
        L.debug_set(k, v)
    yield
    for k, v in DEBUG_DEFAULTS.items():
        L.debug_set(k, v)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ the driver
def drive(dev, call, fills=M.FILLS, locate=None):
    """Runs call(A, poison) -> dict(status, outs {name: device tensor}[, gaps (workspace, buffers)][, zero [tensors]]) once
    per fill on fresh arenas and asserts (a)-(e) and (g) of the module docstring; returns the outputs of the first fill."""
    results = []
    for fill, guard in fills:
        A = M.ArenaSet(dev, fill, guard)
        r = call(A, fill == 0xFF)
        torch.cuda.synchronize()
        assert r["status"] == 0, (hex(fill), r["status"])
        damaged = A.check()
        assert not damaged, f"fill {fill:#x}: {M.describe_guards(damaged)}"
        assert A.changed_inputs() == [], hex(fill)
        if "gaps" in r:
            ws, bufs = r["gaps"]
            found = M.check_gaps(ws, bufs, fill)
            assert not found, f"fill {fill:#x}: workspace bytes outside every buffer changed (first offset, count): {found}"
        for k, z in enumerate(r.get("zero", ())):
            assert z.numel() == 0 or float(z.abs().max()) == 0.0, (hex(fill), "rows past the end", k)
        results.append({k: v.clone() for k, v in r["outs"].items()})
    for (fill, _g), res in zip(fills[1:], results[1:]):
        for k, v in res.items():
            if not M.bits_equal(v, results[0][k]):
                where = locate(fills[0], (fill, _g)) if locate is not None else ""
                n = int((v.reshape(-1).view(torch.uint8) != results[0][k].reshape(-1).view(torch.uint8)).sum())
                raise AssertionError(f"output {k!r} depends on what the buffers held: fill {fill:#x} differs from fill "
                                     f"{fills[0][0]:#x} in {n} byte(s). {where}")
    return results[0]


# ------------------------------------------------------------------ whole path
class PathCase:
    """One whole-path problem: entry = plain | ragged | ragged_fm | fanout | fanout_fm.  Fan-out: unit / lens per source,
    src per row, g / noise per row."""

    def __init__(self, mc, sd, dtype, unit, g, noise, lens=None, entry="plain", src=None, junk_padding=True):
        from quickvc_official_amd import lib as L
        self.L, self.hip = L, L.load_library()
        self.mc, self.sd, self.dtype, self.entry = dict(mc, operand_dtype=dtype), sd, dtype, entry
        self.cfg = L.make_config(self.mc)
        self.blob = L.pack_weights(self.hip, self.cfg, sd)
        self.unit, self.g, self.noise = unit.float().contiguous(), g.float().contiguous(), noise.float().contiguous()
        self.lens, self.src, self.junk_padding = lens, src, junk_padding
        self.fan = entry.startswith("fanout")
        self.R, _c, self.T = self.noise.shape
        self.U = self.unit.shape[0]
        self.spf = E.samples_per_frame(self.cfg)
        self.n_path = int(self.hip.qvc_workspace_bytes(ctypes.byref(self.cfg), self.R, self.T))
        self.n_ws = int(self.hip.qvc_fanout_workspace_bytes(ctypes.byref(self.cfg), self.U, self.R, self.T)) if self.fan else self.n_path
        assert self.n_path > 0 and self.n_ws >= self.n_path
        self.bufs = E.workspace_map(E.load_emu_windows(), self.cfg, self.R, self.T)
        if self.fan:                                                   # the per-row length array behind the path's workspace
            self.bufs = self.bufs + [dict(name="row_frames", offset=self.n_path, bytes=self.R * 4, elem="i32", groups=1, rows=1,
                                          channels=1, mul=0, add=0)]

    def row_lens(self, lens=None, src=None):
        lens = self.lens if lens is None else lens
        if lens is None:
            return None
        src = self.src if src is None else src
        return [lens[s] for s in src] if self.fan else list(lens)

    def setup(self, A, poison, lens=None, src=None):
        lens = self.lens if lens is None else lens
        src = self.src if src is None else src
        unit, noise = self.unit.clone(), self.noise.clone()
        if lens is not None and self.junk_padding:                     # "the padding's content is ignored"
            ju, jn = (NAN, NAN) if poison else (300.0, -55.0)
            for b, n in enumerate(lens):
                unit[b, :, n:] = ju
            for r, n in enumerate(self.row_lens(lens, src)):
                noise[r, :, n:] = jn
        if self.entry.endswith("_fm"):
            unit = unit.transpose(1, 2).contiguous()
        t = dict(blob=A.input("blob", self.blob), unit=A.input("unit", unit), g=A.input("g", self.g), noise=A.input("noise", noise),
                 ws=A.scratch("workspace", self.n_ws), out=A.output("out", torch.float32, (self.R, 1, self.T * self.spf)))
        if lens is not None:
            t["lens"] = A.input("frames_dev", torch.tensor(lens, dtype=torch.int32))
        if self.fan:
            t["src"] = A.input("src_of_row_dev", torch.tensor(src, dtype=torch.int32))
        return t

    def invoke(self, t):
        hip, cfgp = self.hip, ctypes.byref(self.cfg)
        p = {k: v.data_ptr() for k, v in t.items()}
        if self.entry == "plain":
            return hip.qvc_infer_batch(cfgp, p["blob"], p["unit"], p["g"], p["noise"], p["out"], self.R, self.T, p["ws"], self.n_ws, _stream())
        if self.fan:
            fn = hip.qvc_infer_fanout_ragged_fm if self.entry == "fanout_fm" else hip.qvc_infer_fanout_ragged
            return fn(cfgp, p["blob"], p["unit"], p["lens"], p["src"], p["g"], p["noise"], p["out"], self.U, self.R, self.T, p["ws"],
                      self.n_ws, _stream())
        fn = hip.qvc_infer_batch_ragged_fm if self.entry == "ragged_fm" else hip.qvc_infer_batch_ragged
        return fn(cfgp, p["blob"], p["unit"], p["g"], p["noise"], p["out"], self.R, self.T, p["lens"], p["ws"], self.n_ws, _stream())

    def call(self, A, poison, lens=None, src=None):
        t = self.setup(A, poison, lens, src)
        st = self.invoke(t)
        r = dict(status=st, outs=dict(out=t["out"]), gaps=(t["ws"], self.bufs))
        rl = self.row_lens(lens, src)
        if rl is not None:
            r["zero"] = [t["out"][b, :, n * self.spf:] for b, n in enumerate(rl)]
        return r

    def engine_result(self, dev):
        """The ordinary QvcEngine call for the same inputs (shared workspace, torch allocations)."""
        from quickvc_official_amd.engine import QvcEngine
        eng = QvcEngine(self.mc, self.sd, dev)
        unit, g, noise = self.unit.to(dev), self.g.to(dev), self.noise.to(dev)
        fm = self.entry.endswith("_fm")
        if fm:
            unit = unit.transpose(1, 2).contiguous()
        if self.entry == "plain":
            out = eng.infer_batch(unit, g, noise)
        elif self.fan:
            out = eng.infer_fanout_ragged(unit, torch.tensor(self.lens, dtype=torch.int32), torch.tensor(self.src, dtype=torch.int32), g, noise, unit_fm=fm)
        else:
            out = eng.infer_batch_ragged(unit, g, noise, torch.tensor(self.lens, dtype=torch.int32), unit_fm=fm)
        torch.cuda.synchronize()
        return out

    # ---- which launch is to blame when two fills disagree
    def _lens_of(self, buf):
        """Valid rows' lengths per member of one workspace buffer.  Fan-out: enc_p's buffers are indexed by source."""
        if self.lens is None:
            return None
        if self.fan and buf["name"] in ("xw", "xw2", "oacc", "acts", "stats"):
            return list(self.lens) + [0] * (self.R - self.U)
        return self.row_lens()

    def launch_names(self, dev):
        """Kernel names of the timed twin (plain batch, same shapes): one per step of the conversion path."""
        A = M.ArenaSet(dev, 0x00, 0xA5)
        p = {k: v.data_ptr() for k, v in self.setup(A, False).items()}
        recs, n = (self.L.QvcLaunchRecord * 4096)(), ctypes.c_int32(0)
        st = self.hip.qvc_infer_batch_timed(ctypes.byref(self.cfg), p["blob"], p["unit"], p["g"], p["noise"], p["out"], self.R, self.T,
                                            p["ws"], self.n_ws, _stream(), recs, 4096, ctypes.byref(n))
        torch.cuda.synchronize()
        assert st == 0, st
        return [recs[i].name.decode() for i in range(n.value)]

    def locate(self, dev, fill_a, fill_b):
        """Runs to launch_stop = n under both fills for n = 1, 2, ... and compares the valid rows of every mapped buffer
        and the output, over the elements either run has written: the smallest n that differs names launch n - 1."""
        L = self.L
        N = L.debug_get("launch_steps")
        kinds = None if self.fan else self.launch_names(dev)           # the fan-out path has no timed twin
        specs = [b for b in self.bufs if b["elem"] != "i32"] + [S.output_spec(self.R, self.R * self.T * self.spf)]
        for n in range(1, N + 1):
            snaps = []
            for fill, guard in (fill_a, fill_b):
                A = M.ArenaSet(dev, fill, guard)
                L.debug_set("launch_stop", n)
                r = self.call(A, fill == 0xFF)
                torch.cuda.synchronize()
                L.debug_set("launch_stop", -1)
                assert r["status"] == 0
                snaps.append((A.arenas["workspace"].payload.cpu(), r["outs"]["out"].reshape(-1).cpu()))
            for buf in specs:
                d = first_difference(snaps[0], snaps[1], fill_a[0], fill_b[0], buf, self.R, self._lens_of(buf))
                if d is not None:
                    kind = f" ({kinds[n - 1]})" if kinds and n - 1 < len(kinds) else ""
                    return f"First launch to blame: step {n - 1}{kind} of {N}: {d}"
        return f"No launch of {N} differs over the rows the map calls valid: the output depends on a row past a member's end."


def first_difference(snap_a, snap_b, fill_a, fill_b, buf, B, lens):
    """None, or where two snapshots (workspace bytes, output fp32) that started from different fills first differ in
    `buf`, over its valid rows and over the elements at least one run wrote (bytes that still hold both fills are not a
    difference): buffer, member, frame, channel and both values, as stepcheck.describe words them."""
    es = 4 if buf["elem"] == "f32" else 2
    shape = (buf["groups"], B, buf["rows"], buf["channels"])

    def raw(snap):
        if buf["name"] == "out":
            return snap[1].reshape(-1).view(torch.uint8)
        return snap[0][buf["offset"]:buf["offset"] + buf["bytes"]]
    a, b = raw(snap_a).reshape(*shape, es), raw(snap_b).reshape(*shape, es)
    written = ((a != fill_a) | (b != fill_b)).any(-1)
    valid = torch.zeros(shape[0], B, shape[2], 1, dtype=torch.bool)
    for m, n in enumerate(S.valid_rows(buf, lens, B)):
        valid[:, m, :n] = True
    bad = (a != b).any(-1) & written & valid
    if not bool(bad.any()):
        return None
    g, m, t, c = np.unravel_index(int(torch.argmax(bad.reshape(-1).to(torch.uint8))), shape)
    va, _ = S.view(snap_a, buf, B)
    vb, _ = S.view(snap_b, buf, B)
    return (f"{buf['name']} ({buf['elem']}): group {g} b {m} frame {t} (mod 32: {t % 32}, mod 64: {t % 64}) channel {c} (mod 16: {c % 16}), "
            f"fill {fill_a:#x} gives {float(va[g, m, t, c]):.6g} vs fill {fill_b:#x} {float(vb[g, m, t, c]):.6g}; "
            f"{int(bad.sum())} of {int(valid.expand(shape).sum())} valid elements differ")


def _check_path(dev, case):
    got = drive(dev, case.call, locate=lambda fa, fb: case.locate(dev, fa, fb))
    ref = case.engine_result(dev)
    assert torch.equal(got["out"], ref), "the 0x00 run differs from the ordinary engine call"
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0


@functools.lru_cache(maxsize=None)
def _shipped_problem():
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_inputs, make_synthetic_state_dict
    cfg = dict(q.DEFAULT_MODEL_CONFIG)
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, 901)
    unit, g, noise = make_synthetic_inputs(3, 70, 256, cfg["inter_channels"], cfg["gin_channels"], seed0=901)
    return model.model_config, sd, unit, g, noise


SHIPPED_LENS = [70, 33, 2]       # a partial 32- and 64-frame tile, ends inside halos, a 2-frame member: the step-parity case


@pytest.mark.parametrize("entry", ["plain", "ragged", "ragged_fm"])
@pytest.mark.parametrize("dtype", ["f16", "bf16x", "bf16"])
def test_whole_path_shipped_config(lib, dev, dtype, entry):
    mc, sd, unit, g, noise = _shipped_problem()
    _check_path(dev, PathCase(mc, sd, dtype, unit, g, noise, None if entry == "plain" else SHIPPED_LENS, entry))


def _small_config(name):
    """(model_config, state dict) of the other configurations, B = 2, T = 24."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict
    if name in CS.ROWS:                                                # the accepted configuration space (tests/config_space.py)
        _cfg, mc, sd = CS.problem(name)
        return mc, sd
    if name in ("wide", "multiband"):
        import test_gpu_step_parity as SP
        mc, sd, *_ = SP._other(name)
        return mc, sd
    cfg = {"odd": dict(q.ODD_MODEL_CONFIG),
           "mini256": dict(q.MINI_MODEL_CONFIG, inter_channels=256),          # natural proj rows + sample_kernel
           "istft": dict(q.ISTFT_MODEL_CONFIG, inter_channels=64, hidden_channels=64, upsample_initial_channel=128, gin_channels=64)}[name]
    model = q.SynthesizerTrn(641, 32, **cfg)
    return model.model_config, make_synthetic_state_dict(model, 311)


@pytest.mark.parametrize("entry", ["plain", "ragged"])
@pytest.mark.parametrize("name", ["wide", "multiband", "odd", "mini256", "istft"] + list(CS.ROWS))
def test_whole_path_other_configs(lib, dev, name, entry):
    """... and every row of tests/config_space.py: new halo and tile shapes are where a store lands past a buffer."""
    from quickvc_official_amd.synth import make_synthetic_inputs
    mc, sd = _small_config(name)
    if name == "mini256":
        info = (ctypes.c_int32 * 8)()
        from quickvc_official_amd import lib as L
        assert lib.qvc_plan_info(ctypes.byref(L.make_config(dict(mc, operand_dtype="f16"))), info) == 0 and info[0] == 0, list(info)
    unit, g, noise = make_synthetic_inputs(2, 24, 256, mc["inter_channels"], mc["gin_channels"], seed0=71)
    _check_path(dev, PathCase(mc, sd, "f16", unit, g, noise, None if entry == "plain" else [24, 9], entry))


def _fanout_case(name, entry="fanout", junk_padding=True):
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_inputs, make_synthetic_state_dict
    from test_gpu_fanout import LENS, MAP
    if name == "shipped":
        mc, sd, *_ = _shipped_problem()
    else:
        cfg = dict(q.MINI_MODEL_CONFIG) if name == "mini" else dict(q.MINI_MODEL_CONFIG, inter_channels=256)
        model = q.SynthesizerTrn(641, 32, **cfg)
        mc, sd = model.model_config, make_synthetic_state_dict(model, 1234)
    unit, _g, _n = make_synthetic_inputs(len(LENS), max(LENS), 256, mc["inter_channels"], mc["gin_channels"], seed0=900)
    _u, g, noise = make_synthetic_inputs(len(MAP), max(LENS), 256, mc["inter_channels"], mc["gin_channels"], seed0=950)
    return PathCase(mc, sd, "f16", unit, g, noise, list(LENS), entry, list(MAP), junk_padding)


@pytest.mark.parametrize("entry", ["fanout", "fanout_fm"])
@pytest.mark.parametrize("name", ["shipped", "mini", "mini256"])
def test_fanout(lib, dev, name, entry):
    """Map and lengths in guarded device arrays; EPI_STATS (paired rows) / the plain conv (mini256) and sample_rows_kernel."""
    _check_path(dev, _fanout_case(name, entry))


# ------------------------------------------------------------------ stage entry points
def _simple(dev, call, reference):
    got = drive(dev, call)
    want = reference()
    torch.cuda.synchronize()
    for k, v in want.items():
        assert torch.equal(got[k], v.reshape(got[k].shape)), f"{k}: the 0x00 run differs from the ordinary call"
        assert bool(torch.isfinite(v).all()), k
    return got


@pytest.fixture(scope="module")
def stage(dev):
    """Shipped config, f16, B = 2, T = 37: engine, host blob and inputs of every stage entry point."""
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.engine import QvcEngine
    from quickvc_official_amd.synth import make_synthetic_inputs
    mc, sd, *_ = _shipped_problem()
    mc = dict(mc, operand_dtype="f16")
    eng = QvcEngine(mc, sd, dev)
    B, T = 2, 37
    unit, g, noise = make_synthetic_inputs(B, T, 256, 192, 256, seed0=37)
    gen = torch.Generator().manual_seed(37)
    return dict(eng=eng, cfg=eng.cfg, blob=L.pack_weights(eng.lib, eng.cfg, sd), B=B, T=T, unit=unit, g=g, noise=noise,
                x_fm=torch.randn(B, T, 192, generator=gen), z_fm=torch.randn(B, T, 192, generator=gen),
                post_fm=0.3 * torch.randn(B, T * 20 + 1, 72, generator=gen),
                n_ws=int(eng.lib.qvc_workspace_bytes(ctypes.byref(eng.cfg), B, T)))


def _ptr(t):
    return None if t is None else t.data_ptr()


def test_stage_enc_p(lib, dev, stage):
    s, cfgp = stage, ctypes.byref(stage["cfg"])

    def call(A, poison):
        blob, unit, noise = A.input("blob", s["blob"]), A.input("unit", s["unit"]), A.input("noise", s["noise"])
        ws, z = A.scratch("workspace", s["n_ws"]), A.output("z_p_fm", torch.float32, (s["B"], s["T"], 192))
        st = lib.qvc_enc_p(cfgp, _ptr(blob), _ptr(unit), _ptr(noise), _ptr(z), s["B"], s["T"], _ptr(ws), s["n_ws"], _stream())
        return dict(status=st, outs=dict(z=z))
    _simple(dev, call, lambda: dict(z=s["eng"].enc_p(s["unit"].to(dev), s["noise"].to(dev))))


@pytest.mark.parametrize("which", [0, 1])
def test_stage_wn_stack(lib, dev, stage, which):
    s, cfgp = stage, ctypes.byref(stage["cfg"])

    def call(A, poison):
        blob, x = A.input("blob", s["blob"]), A.input("x_fm", s["x_fm"])
        g = A.input("g", s["g"]) if which else None
        ws, out = A.scratch("workspace", s["n_ws"]), A.output("out_fm", torch.float32, (s["B"], s["T"], 192))
        st = lib.qvc_wn_stack(cfgp, _ptr(blob), which, _ptr(x), _ptr(g), _ptr(out), s["B"], s["T"], _ptr(ws), s["n_ws"], _stream())
        return dict(status=st, outs=dict(out=out))
    _simple(dev, call, lambda: dict(out=s["eng"].wn_stack(which, s["x_fm"].to(dev), s["g"].to(dev) if which else None)))


@pytest.mark.parametrize("direction", ["reverse", "forward"])
def test_stage_flow(lib, dev, stage, direction):
    """qvc_flow_reverse / qvc_flow_forward: in place on z, which is therefore input and output at once."""
    s, cfgp = stage, ctypes.byref(stage["cfg"])
    fn = lib.qvc_flow_reverse if direction == "reverse" else lib.qvc_flow_forward

    def call(A, poison):
        blob, g = A.input("blob", s["blob"]), A.input("g", s["g"])
        z = A.input("z_fm", s["z_fm"], track=False)
        ws = A.scratch("workspace", s["n_ws"])
        st = fn(cfgp, _ptr(blob), _ptr(z), _ptr(g), s["B"], s["T"], _ptr(ws), s["n_ws"], _stream())
        return dict(status=st, outs=dict(z=z))
    eng_fn = s["eng"].flow_reverse if direction == "reverse" else s["eng"].flow_forward
    got = _simple(dev, call, lambda: dict(z=eng_fn(s["z_fm"].to(dev), s["g"].to(dev))))
    assert not torch.equal(got["z"].cpu(), s["z_fm"])


def test_stage_dec_trunk(lib, dev, stage):
    s, cfgp = stage, ctypes.byref(stage["cfg"])
    F = s["T"] * 20 + 1

    def call(A, poison):
        blob, z, g = A.input("blob", s["blob"]), A.input("z_fm", s["z_fm"]), A.input("g", s["g"])
        ws, post = A.scratch("workspace", s["n_ws"]), A.output("post_fm", torch.float32, (s["B"], F, 72))
        st = lib.qvc_dec_trunk(cfgp, _ptr(blob), _ptr(z), _ptr(g), _ptr(post), s["B"], s["T"], _ptr(ws), s["n_ws"], _stream())
        return dict(status=st, outs=dict(post=post))
    _simple(dev, call, lambda: dict(post=s["eng"].dec_trunk(s["z_fm"].to(dev), s["g"].to(dev))))


@pytest.mark.parametrize("bands", [False, True], ids=["out", "out+y_mb"])
def test_stage_istft_synth(lib, dev, stage, bands):
    s, cfgp = stage, ctypes.byref(stage["cfg"])
    F = s["T"] * 20 + 1

    def call(A, poison):
        blob, post = A.input("blob", s["blob"]), A.input("post_fm", s["post_fm"])
        out = A.output("out", torch.float32, (s["B"], 1, 16 * (F - 1)))
        ymb = A.output("y_mb", torch.float32, (s["B"], 4, 4 * (F - 1))) if bands else None
        st = lib.qvc_istft_synth(cfgp, _ptr(blob), _ptr(post), _ptr(out), _ptr(ymb), s["B"], F, _stream())
        return dict(status=st, outs=dict(out=out, ymb=ymb) if bands else dict(out=out))

    def reference():
        r = s["eng"].istft_synth(s["post_fm"].to(dev), want_bands=bands)
        return dict(out=r[0], ymb=r[1]) if bands else dict(out=r)
    _simple(dev, call, reference)


def test_stage_posterior_pair(lib, dev):
    """qvc_enc_q (own blob) and qvc_flow_forward on its z, mini_q shapes, f16."""
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.engine import QvcEngine
    from quickvc_official_amd.synth import make_synthetic_posterior_inputs, make_synthetic_state_dict
    entry = json.load(open(os.path.join(GOLDEN, "manifest.json")))["mini_q"]
    cfg = entry["config"]
    model = q.SynthesizerTrn(641, 32, **cfg)
    sd = make_synthetic_state_dict(model, entry["weights_seed"])
    B, T, C = entry["batch"], entry["frames"], cfg["inter_channels"]
    spec, g, noise = make_synthetic_posterior_inputs(B, T, 641, C, cfg["gin_channels"], seed0=entry["inputs_seed0"])
    eng = QvcEngine(dict(model.model_config, operand_dtype="f16"), sd, dev)
    cfgp = ctypes.byref(eng.cfg)
    qblob = L.pack_weights(lib, eng.cfg, {k: v for k, v in sd.items() if k.startswith("enc_q.")}, which="encq")
    blob = L.pack_weights(lib, eng.cfg, sd)
    n_ws = int(lib.qvc_workspace_bytes(cfgp, B, T))

    def call_q(A, poison):
        b, sp, gg, nz = A.input("encq_blob", qblob), A.input("spec", spec), A.input("g", g), A.input("noise", noise)
        ws, z = A.scratch("workspace", n_ws), A.output("z_fm", torch.float32, (B, T, C))
        st = lib.qvc_enc_q(cfgp, _ptr(b), _ptr(sp), _ptr(gg), _ptr(nz), _ptr(z), B, T, _ptr(ws), n_ws, _stream())
        return dict(status=st, outs=dict(z=z))
    z = _simple(dev, call_q, lambda: dict(z=eng.enc_q(spec.to(dev), g.to(dev), noise.to(dev))))["z"].cpu()

    def call_f(A, poison):
        b, gg, zz = A.input("blob", blob), A.input("g", g), A.input("z_fm", z, track=False)
        ws = A.scratch("workspace", n_ws)
        st = lib.qvc_flow_forward(cfgp, _ptr(b), _ptr(zz), _ptr(gg), B, T, _ptr(ws), n_ws, _stream())
        return dict(status=st, outs=dict(zp=zz))
    _simple(dev, call_f, lambda: dict(zp=eng.flow_forward(z.to(dev), g.to(dev))))


# ------------------------------------------------------------------ one conv through the MFMA kernel
CONV_ROWS = [(3, 40, 80, 21, 5, 1), (1, 8, 4, 700, 3, 1), (1, 512, 128, 1, 1, 1), (2, 128, 72, 130, 7, 1)]   # rows of CONV_CASES


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", CONV_ROWS)
def test_conv1d(lib, dev, case, dtype):
    """w_scratch_host is a HOST buffer the packer writes: it gets a guarded arena of its own on the CPU."""
    from quickvc_official_amd import lib as L
    from test_gpu_parity import CONV_CASES
    B, cin, cout, T, k, dil, slope = next(c for c in CONV_CASES if tuple(c[:6]) == case)
    gen = torch.Generator().manual_seed(cin * 7 + cout + k + dil)
    x = torch.randn(B, cin, T, generator=gen)
    w = torch.randn(cout, cin, k, generator=gen) / (cin * k) ** 0.5
    bias = torch.randn(cout, generator=gen) * 0.1
    nb, nw = int(lib.qvc_conv1d_scratch_bytes(cout, cin, k)), int(lib.qvc_conv1d_workspace_bytes(B, cout, cin, T))
    assert nb > 0 and nw > 0

    def call(A, poison):
        host = M.Arena("w_scratch_host", nb, "cpu", A.fill, A.guard_fill)
        xd, y = A.input("x", x), A.output("y", torch.float32, (B, cout, T))
        sdev, ws = A.scratch("w_scratch_dev", nb), A.scratch("workspace", nw)
        st = lib.qvc_conv1d(_ptr(xd), w.data_ptr(), bias.data_ptr(), _ptr(y), B, cin, cout, T, k, dil, slope, L.DTYPES[dtype],
                            host.ptr(), _ptr(sdev), nb, _ptr(ws), nw, _stream())
        torch.cuda.synchronize()
        assert host.check() == [], M.describe_guards(host.check())
        return dict(status=st, outs=dict(y=y))

    def reference():
        al = lambda t: t.data_ptr() + ((-t.data_ptr()) % 256)
        sh, sd_, ws = (torch.empty(nb + 256, dtype=torch.uint8), torch.empty(nb + 256, dtype=torch.uint8, device=dev),
                       torch.empty(nw + 256, dtype=torch.uint8, device=dev))
        xd, y = x.to(dev), torch.empty(B, cout, T, device=dev)
        assert lib.qvc_conv1d(xd.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), B, cin, cout, T, k, dil, slope, L.DTYPES[dtype],
                              al(sh), al(sd_), nb, al(ws), nw, _stream()) == 0
        torch.cuda.synchronize()
        return dict(y=y)
    w0, b0 = w.clone(), bias.clone()
    _simple(dev, call, reference)
    assert torch.equal(w, w0) and torch.equal(bias, b0)


# ------------------------------------------------------------------ streaming
@functools.lru_cache(maxsize=None)
def _stream_model():
    entry, _ = load_case("full_b1")
    model, sd, _u, _g, _n = regenerate(entry)
    model.load_state_dict(sd)
    return model, sd


@pytest.mark.parametrize("hop,T,lens", [(7, 121, [121, 121, 121]), (40, 200, [200, 143, 57])], ids=["hop7", "hop40-ragged"])
def test_stream_steps_to_the_flush(lib, dev, hop, T, lens):
    """Every qvc_stream_step of three streams to the flush: hop 7 (rows that are no multiple of 16 bytes: the 4-byte
    fallback of copy_batch_kernel) and hop 40 with streams that end at different frames.  `state` is zeroed as the
    header requires; the stream workspace, out, unit_new, noise_new, pos_dev, len_dev start from the fill; the frames of
    unit_new / noise_new outside a stream are junk (NaN under 0xFF).  The concatenated output is identical across fills
    and equals StreamConverter's."""
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.streaming import StreamConverter
    from quickvc_official_amd.synth import make_synthetic_inputs
    model, sd = _stream_model()
    mc = dict(model.model_config, operand_dtype="f16")
    cfg = L.make_config(mc)
    cfgp = ctypes.byref(cfg)
    blob = L.pack_weights(lib, cfg, sd)
    S_, C, UC = 3, 192, 256
    unit, g, noise = make_synthetic_inputs(S_, T, UC, C, 256, seed0=6400)
    n_state, n_ws = int(lib.qvc_stream_state_bytes(cfgp, S_, hop)), int(lib.qvc_stream_workspace_bytes(cfgp, S_, hop))
    lag, nl = int(lib.qvc_stream_lag_frames(cfgp)), int(lib.qvc_stream_noise_lag_frames(cfgp))
    spf = E.samples_per_frame(cfg)
    assert n_state > 0 and n_ws > 0 and lag > 0
    steps = -(-(T + lag) // hop)

    def call(A, poison):
        junk_u, junk_n = (NAN, NAN) if poison else (123.0, -55.0)
        bl, gg = A.input("blob", blob), A.input("g", g)
        ln = A.input("len_dev", torch.tensor(lens, dtype=torch.int32))
        state = A.scratch("state", n_state)
        state.zero_()                                                   # "ZEROED before a stream's first step"
        ws, out = A.scratch("workspace", n_ws), A.output("out", torch.float32, (S_, hop * spf))
        whole = torch.zeros(S_, 1, T * spf, device=dev)
        status = 0
        for n in range(steps):
            s = n * hop
            u_new, n_new = torch.full((S_, UC, hop), junk_u), torch.full((S_, C, hop), junk_n)
            for b, end in enumerate(lens):
                lo, hi = s, min(s + hop, end)
                if hi > lo:
                    u_new[b, :, :hi - lo] = unit[b, :, lo:hi]
                a = s - nl                                              # noise frames [s - nl, s - nl + hop)
                lo, hi = max(a, 0), min(a + hop, end)
                if hi > lo:
                    n_new[b, :, lo - a:hi - a] = noise[b, :, lo:hi]
            ud, nd = A.input("unit_new", u_new), A.input("noise_new", n_new)
            pos = A.input("pos_dev", torch.full((S_,), s, dtype=torch.int32))
            out.view(torch.uint8).fill_(A.fill)
            st = lib.qvc_stream_step(cfgp, _ptr(bl), _ptr(state), n_state, _ptr(ud), _ptr(gg), _ptr(nd), _ptr(out), S_, hop, _ptr(pos),
                                     _ptr(ln), _ptr(ws), n_ws, _stream())
            status = status or st
            assert A.changed_inputs(("unit_new", "noise_new", "pos_dev")) == [], n
            f0 = s - lag                                                # the chunk holds frames [f0, f0 + hop)
            lo, hi = max(f0, 0), min(f0 + hop, T)
            if hi > lo:
                whole[:, 0, lo * spf:hi * spf] = out[:, (lo - f0) * spf:(hi - f0) * spf]
            if f0 + hop <= 0 or f0 >= T:
                assert float(out.abs().max()) == 0.0, n                 # "zeros outside [0, len[b])"
        return dict(status=status, outs=dict(whole=whole), zero=[whole[b, :, end * spf:] for b, end in enumerate(lens)])

    def reference():
        m = model.to(dev).eval()
        conv = StreamConverter(m, streams=S_, hop_frames=hop, use_graph=False)
        return dict(whole=conv.convert(unit.to(dev), g.to(dev), noise.to(dev), lengths=torch.tensor(lens, dtype=torch.int32)))
    _simple(dev, call, reference)


def test_stream_reset_slot(lib, dev):
    """state pre-filled 0x3C, slot 1 of 3 reset: guards intact, every state byte that changed is now 0, pos_dev / len_dev
    changed at index 1 only."""
    from quickvc_official_amd import lib as L
    model, _sd = _stream_model()
    cfg = L.make_config(dict(model.model_config, operand_dtype="f16"))
    cfgp = ctypes.byref(cfg)
    hop = 40
    n_state = int(lib.qvc_stream_state_bytes(cfgp, 3, hop))
    A = M.ArenaSet(dev, 0x3C, 0x5A)
    state = A.scratch("state", n_state)
    pos = A.input("pos_dev", torch.tensor([11, 22, 33], dtype=torch.int32), track=False)
    ln = A.input("len_dev", torch.tensor([44, 55, 66], dtype=torch.int32), track=False)
    st = lib.qvc_stream_reset_slot(cfgp, _ptr(state), n_state, 3, hop, 1, 777, _ptr(pos), _ptr(ln), _stream())
    torch.cuda.synchronize()
    assert st == 0
    assert A.check() == [], M.describe_guards(A.check())
    changed = state != 0x3C
    assert 0 < int(changed.sum()) < n_state and bool((state[changed] == 0).all())
    assert pos.tolist() == [11, 0, 33] and ln.tolist() == [44, 777, 66]


# ------------------------------------------------------------------ speaker encoder, mel, trim
CYCLE = (1, 50, 127, 128, 129, 192, 193, 300, 321)               # tests/test_gpu_target_batches.py


def _spk_engine(dev, which, dtype):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    from quickvc_official_amd.engine import QvcEngine
    entry, _ = load_case(which)
    _m, sd, _u, _g, _n = regenerate(entry)
    model = q.SynthesizerTrn(641, 32, **entry["config"])
    eng = QvcEngine(dict(model.model_config, operand_dtype=dtype), sd, dev)
    blob = L.pack_weights(eng.lib, eng.cfg, {k: v for k, v in sd.items() if k.startswith("enc_spk.")}, which="spk")
    return eng, blob


def _mels(frames, fmax, seed0, pad):
    from quickvc_official_amd.synth import make_synthetic_mel
    mel = torch.full((len(frames), 80, fmax), pad)
    for u, f in enumerate(frames):
        mel[u, :, :f] = make_synthetic_mel(max(f, 1), 80, seed=seed0 + 13 * u)[0, :, :f]
    return mel


def _spk_ragged_call(lib, eng, blob, frames, fmax, seed0, junk_padding=True):
    U, gin = len(frames), int(eng.cfg.gin_channels)
    n_ws = int(lib.qvc_spk_ragged_workspace_bytes(ctypes.byref(eng.cfg), U, fmax))
    assert n_ws > 0

    def call(A, poison, frames=frames):
        mel = _mels(frames if junk_padding else [fmax] * U, fmax, seed0, NAN if poison else 9.5)
        b, m, fr = A.input("spk_blob", blob), A.input("mel", mel), A.input("frames_dev", torch.tensor(frames, dtype=torch.int32))
        ws, g = A.scratch("workspace", n_ws), A.output("g", torch.float32, (U, gin))
        st = lib.qvc_speaker_embed_ragged(ctypes.byref(eng.cfg), _ptr(b), _ptr(m), _ptr(fr), _ptr(g), U, fmax, _ptr(ws), n_ws, _stream())
        return dict(status=st, outs=dict(g=g))
    return call


@pytest.mark.parametrize("which,dtype", [("mini", "f16"), ("mini", "bf16"), ("full_b1", "f16")], ids=["mini-f16", "mini-bf16", "gin256-f16"])
def test_speaker_embed_ragged(lib, dev, which, dtype):
    eng, blob = _spk_engine(dev, which, dtype)
    frames = [CYCLE[u % len(CYCLE)] for u in range(19)] if which == "mini" else [100, 129, 250, 321]
    call = _spk_ragged_call(lib, eng, blob, frames, 321, 100)
    _simple(dev, call, lambda: dict(g=eng.speaker_embed_ragged(_mels(frames, 321, 100, 0.0).to(dev), torch.tensor(frames, dtype=torch.int32, device=dev))))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_speaker_embed_uniform(lib, dev, dtype):
    eng, blob = _spk_engine(dev, "mini", dtype)
    U, F = 3, 300
    mel = _mels([F] * U, F, 500, 0.0)
    n_ws = int(lib.qvc_spk_workspace_bytes(ctypes.byref(eng.cfg), U, F))
    assert n_ws > 0

    def call(A, poison):
        b, m = A.input("spk_blob", blob), A.input("mel", mel)
        ws, g = A.scratch("workspace", n_ws), A.output("g", torch.float32, (U, 64))
        st = lib.qvc_speaker_embed(ctypes.byref(eng.cfg), _ptr(b), _ptr(m), _ptr(g), U, F, _ptr(ws), n_ws, _stream())
        return dict(status=st, outs=dict(g=g))
    _simple(dev, call, lambda: dict(g=eng.speaker_embed(mel.to(dev))))


FRONT_SAMPLES = [80000, 2000, 641]


def _front(dev):
    from quickvc_official_amd.frontend import MelFrontend
    return MelFrontend(1280, 80, 16000, 320, 1280, 0.0, None, device=dev)


def _waves(samples, pad, silence=False):
    """(U, max) rows: a tone plus noise (with a silent lead-in and tail when `silence`: something for the trim to cut)."""
    gen = torch.Generator().manual_seed(77)
    N = max(samples)
    t = torch.arange(N) / 16000.0
    wave = (0.3 * torch.sin(2 * np.pi * 220.0 * t)[None] + 0.05 * torch.randn(len(samples), N, generator=gen)).clamp(-1, 1)
    for u, n in enumerate(samples):
        if silence and n >= 8192:
            wave[u, :2048] = 0.0
            wave[u, n - 3072:n] = 0.0
        wave[u, n:] = pad
    return wave


@pytest.mark.parametrize("samples,U", [(80000, 2), (2000, 3), (641, 1)])
def test_wave_to_mel(lib, dev, samples, U):
    fe = _front(dev)
    table, wave = fe.table.cpu(), _waves([samples] * U, 0.0)
    n_ws = int(lib.qvc_mel_workspace_bytes(1280, 320, U, samples))
    assert n_ws > 0

    def call(A, poison):
        tb, w = A.input("table", table), A.input("wave", wave)
        ws, mel = A.scratch("workspace", n_ws), A.output("mel", torch.float32, (U, 80, fe.frames(samples)))
        st = lib.qvc_wave_to_mel(_ptr(tb), 1280, 320, 80, _ptr(w), _ptr(mel), U, samples, _ptr(ws), n_ws, _stream())
        return dict(status=st, outs=dict(mel=mel))
    _simple(dev, call, lambda: dict(mel=fe(wave.to(dev))))


def _mel_ragged_call(lib, fe, table, samples, starts=None, junk_padding=True):
    """Row u is the samples[u] samples from starts[u] on; what lies past start + samples is padding."""
    U, N = len(samples), max(FRONT_SAMPLES)
    n_ws = int(lib.qvc_mel_ragged_workspace_bytes(1280, 320, U, N))
    assert n_ws > 0
    fmax = fe.frames(N)

    def call(A, poison, samples=samples):
        ends = [n + (starts[u] if starts else 0) for u, n in enumerate(samples)]
        wave = _waves(ends if junk_padding else [N] * U, NAN if poison else 7.0)
        tb, w = A.input("table", table), A.input("wave", wave)
        sm = A.input("samples_dev", torch.tensor(samples, dtype=torch.int32))
        sa = A.input("start_dev", torch.tensor(starts, dtype=torch.int32)) if starts is not None else None
        ws = A.scratch("workspace", n_ws)
        mel, frames = A.output("mel", torch.float32, (U, 80, fmax)), A.output("frames_dev", torch.int32, (U,))
        st = lib.qvc_wave_to_mel_ragged(_ptr(tb), 1280, 320, 80, _ptr(w), _ptr(sa), _ptr(sm), _ptr(mel), _ptr(frames), U, N, _ptr(ws), n_ws,
                                        _stream())
        return dict(status=st, outs=dict(mel=mel, frames=frames), zero=[mel[u, :, fe.frames(n):] for u, n in enumerate(samples)])
    return call


@pytest.mark.parametrize("starts", [None, [517, 100, 0]], ids=["from0", "start_dev"])
def test_wave_to_mel_ragged(lib, dev, starts):
    fe = _front(dev)
    samples = [n - s for n, s in zip(FRONT_SAMPLES, starts or [0, 0, 0])]
    call = _mel_ragged_call(lib, fe, fe.table.cpu(), samples, starts)

    def reference():
        mel, frames = fe.ragged(_waves(FRONT_SAMPLES, 0.0).to(dev), torch.tensor(samples, dtype=torch.int32, device=dev),
                                None if starts is None else torch.tensor(starts, dtype=torch.int32, device=dev))
        return dict(mel=mel, frames=frames)
    got = _simple(dev, call, reference)
    assert got["frames"].tolist() == [fe.frames(n) for n in samples]


def test_trim_bounds(lib, dev):
    from quickvc_official_amd.frontend import trim_bounds
    samples = FRONT_SAMPLES
    U, N = len(samples), max(samples)
    n_ws = int(lib.qvc_trim_workspace_bytes(U, N, 2048, 512))
    assert n_ws > 0

    def call(A, poison):
        w = A.input("wave", _waves(samples, NAN if poison else 7.0, silence=True))
        sm = A.input("samples_dev", torch.tensor(samples, dtype=torch.int32))
        ws = A.scratch("workspace", n_ws)
        start, length = A.output("start_dev", torch.int32, (U,)), A.output("len_dev", torch.int32, (U,))
        st = lib.qvc_trim_bounds(_ptr(w), _ptr(sm), _ptr(start), _ptr(length), U, N, 20.0, 2048, 512, _ptr(ws), n_ws, _stream())
        return dict(status=st, outs=dict(start=start, length=length))

    def reference():
        start, length = trim_bounds(_waves(samples, 0.0, silence=True).to(dev), torch.tensor(samples, dtype=torch.int32, device=dev))
        return dict(start=start, length=length)
    got = _simple(dev, call, reference)
    assert got["start"].tolist()[1:] == [0, 0] and got["length"].tolist()[1:] == [2000, 641]      # quiet-free / shorter than a frame
    assert got["start"][0] > 0 and got["start"][0] + got["length"][0] < 80000                    # cut on both sides


# ------------------------------------------------------------------ stale workspace: a shorter call on a longer call's bytes
def _stale(dev, call, full, short, names=("out",)):
    """call(A, poison, lens): once with every member at full length, again on the SAME arenas (not refilled) with the
    short lengths -- bit-identical to the short lengths on fresh arenas."""
    A = M.ArenaSet(dev, 0x3C, 0x5A)
    first = call(A, False, full)
    torch.cuda.synchronize()
    assert first["status"] == 0
    first = {k: first["outs"][k].clone() for k in names}
    again = call(A, False, short)
    torch.cuda.synchronize()
    assert again["status"] == 0 and A.check() == [], M.describe_guards(A.check())
    B_ = M.ArenaSet(dev, 0x3C, 0x5A)
    fresh = call(B_, False, short)
    torch.cuda.synchronize()
    assert fresh["status"] == 0
    for k in names:
        assert M.bits_equal(again["outs"][k], fresh["outs"][k]), f"{k}: a call on the rows a longer call left behind differs from a fresh one"
        assert not M.bits_equal(again["outs"][k], first[k]), k
    return fresh


def _stale_path_case(kind):
    if kind == "fanout":
        return _fanout_case("mini", junk_padding=False)
    mc, sd, unit, g, noise = _shipped_problem()
    return PathCase(mc, sd, "f16", unit, g, noise, SHIPPED_LENS, "ragged", junk_padding=False)


@pytest.mark.parametrize("kind", ["ragged", "fanout"])
def test_stale_workspace_whole_path(lib, dev, kind):
    case = _stale_path_case(kind)
    _stale(dev, case.call, [case.T] * case.U, case.lens)


@pytest.mark.parametrize("kind", ["ragged", "fanout"])
def test_stale_workspace_graph_replay(lib, dev, kind):
    """The production form: ONE captured graph, replayed at full length and then with the lengths shortened in place."""
    case = _stale_path_case(kind)
    full, short = [case.T] * case.U, case.lens
    A = M.ArenaSet(dev, 0x3C, 0x5A)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        t = case.setup(A, False, full)
        assert case.invoke(t) == 0                                     # warm-up (code objects)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            assert case.invoke(t) == 0
        A.arenas["workspace"].refill()
        A.arenas["out"].refill()
        graph.replay()
        side.synchronize()
        long_out = t["out"].clone()
        A.input("frames_dev", torch.tensor(short, dtype=torch.int32))  # in place: the graph only holds the pointer
        graph.replay()
        side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    assert A.check() == [] and A.changed_inputs() == [], M.describe_guards(A.check())
    fresh = case.call(M.ArenaSet(dev, 0x3C, 0x5A), False, short)
    torch.cuda.synchronize()
    assert fresh["status"] == 0
    assert M.bits_equal(t["out"], fresh["outs"]["out"]) and not M.bits_equal(t["out"], long_out)
    for z in fresh["zero"]:
        assert z.numel() == 0 or float(z.abs().max()) == 0.0


def test_stale_workspace_speaker_embed_ragged(lib, dev):
    eng, blob = _spk_engine(dev, "mini", "f16")
    frames = [CYCLE[u % len(CYCLE)] for u in range(19)]
    call = _spk_ragged_call(lib, eng, blob, frames, 321, 100, junk_padding=False)
    _stale(dev, call, [321] * 19, frames, names=("g",))


def test_stale_workspace_wave_to_mel_ragged(lib, dev):
    fe = _front(dev)
    call = _mel_ragged_call(lib, fe, fe.table.cpu(), FRONT_SAMPLES, junk_padding=False)
    _stale(dev, call, [max(FRONT_SAMPLES)] * 3, FRONT_SAMPLES, names=("mel", "frames"))


# ------------------------------------------------------------------ the checker sees device-side stores
def test_checker_sees_a_device_store_past_a_payload(dev):
    """A plain torch indexed store of one element just past a payload -- a legal write inside the arena's allocation."""
    A = M.ArenaSet(dev, 0x00, 0xA5)
    out = A.output("out", torch.float32, (3, 7))
    A.scratch("workspace", 1000)
    a = A.arenas["out"]
    past = a.raw[a.lo:a.hi + 4].view(torch.float32)                     # the payload and one more element
    past[torch.tensor([out.numel()], device=dev)] = 1.0
    torch.cuda.synchronize()
    assert A.check() == [dict(name="out", side="after", distance=1, count=4)]     # 1.0f = 00 00 80 3f: no byte is a5
    a.raw[a.lo - 4:a.lo].view(torch.float32)[torch.tensor([0], device=dev)] = -2.0
    torch.cuda.synchronize()
    assert [(f["name"], f["side"], f["distance"]) for f in A.check()] == [("out", "before", 1), ("out", "after", 1)]
    assert bool((out == 0).all())
