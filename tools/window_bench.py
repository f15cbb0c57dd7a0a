"""One long recording through the exact windows over packed utterances (qvc_infer_windows_rng_fm) against the existing
whole-utterance entry point: the shipped config in bf16x, ONE utterance of `frames` unit frames (default 16 384, 5.5 min).
  baseline   qvc_infer_batch_ragged_rng at B = 1 on the whole utterance (one call; its workspace grows with the length)
  windows    the window form at (rows, n) = (16, 1024) and (32, 512): the whole utterance = ceil(frames / n / rows) calls
Every form is ONE captured graph per call; the forms are timed in alternating rounds of one process (HIP events around the
replays of a whole conversion, inputs random) and the median round is reported, with both workspace sizes beside the
times.  No test asserts a time; the baseline is the ragged entry point in the same run, never the window form itself.
usage: python tools/window_bench.py [frames] [rounds]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quickvc_official_amd as q  # noqa: E402
from quickvc_official_amd.engine import aligned_empty  # noqa: E402
from quickvc_official_amd.synth import make_synthetic_state_dict  # noqa: E402
from quickvc_official_amd.windows import plan_windows  # noqa: E402

SEED = 0x5EED


class Ragged:
    """qvc_infer_batch_ragged_rng at B = 1 on the whole utterance, one graph."""

    def __init__(self, eng, units, g, stream):
        T = units.shape[0]
        self.stream, self.calls = stream, 1
        self.unit, self.g = units.unsqueeze(0).contiguous(), g
        self.frames = torch.tensor([T], dtype=torch.int32, device=eng.device)
        self.keys = torch.zeros(1, dtype=torch.int64, device=eng.device)
        self.out = torch.empty(1, 1, T * eng.samples_per_frame, device=eng.device)
        self.ws = eng.alloc_workspace(1, T)
        self.workspace_bytes = self.ws.numel()
        call = lambda: eng.infer_batch_ragged(self.unit, self.g, None, self.frames, out=self.out, ws=self.ws, unit_fm=True,
                                              rng=(SEED, self.keys, 1.0))
        with torch.cuda.stream(stream):
            call()
            stream.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=stream):
                call()

    def convert(self):
        self.graph.replay()


class Windows:
    """The window form at (rows, n): the plan's groups, each a table copy and one replay of one graph."""

    def __init__(self, eng, units, g, stream, rows, n):
        T = units.shape[0]
        self.stream, self.units = stream, units
        plan = plan_windows([T], n)
        self.calls = -(-len(plan) // rows)
        tab = torch.zeros(self.calls * rows, 4, dtype=torch.int32)
        tab[:len(plan)] = torch.tensor([[0, T, s, c] for _u, s, c in plan], dtype=torch.int32)
        self.groups = tab.reshape(self.calls, rows, 4).to(eng.device)
        self.table = torch.zeros(rows, 4, dtype=torch.int32, device=eng.device)
        self.g = g.expand(rows, -1).contiguous()
        self.keys = torch.zeros(rows, dtype=torch.int64, device=eng.device)
        self.out = torch.empty(T * eng.samples_per_frame, device=eng.device)
        self.workspace_bytes, self.context = eng.windows_sizes(rows, n)
        self.ws = aligned_empty(self.workspace_bytes, eng.device)
        call = lambda: eng.infer_windows(self.ws, self.units, None, self.table, self.g, self.out, n, rng=(SEED, self.keys, 1.0))
        with torch.cuda.stream(stream):
            call()
            stream.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=stream):
                call()

    def convert(self):
        for i in range(self.calls):
            self.table.copy_(self.groups[i])
            self.graph.replay()


def timed(form, n=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(form.stream):
        form.convert()                                   # warm-up
        e0.record(form.stream)
        for _ in range(n):
            form.convert()
        e1.record(form.stream)
    form.stream.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    model = q.SynthesizerTrn(641, 32, **q.DEFAULT_MODEL_CONFIG, operand_dtype="bf16x")
    model.load_state_dict(make_synthetic_state_dict(model, 1234))
    model = model.cuda().eval()
    eng = model.engine()
    gen = torch.Generator().manual_seed(77)
    units = torch.randn(frames, 256, generator=gen).cuda()         # random inputs (zero operands let the chip clock higher)
    g = torch.nn.functional.normalize(torch.rand(1, 256, generator=gen), dim=1).cuda()
    stream = torch.cuda.Stream()
    forms = {"ragged_b1": Ragged(eng, units, g, stream)}
    for rows, n in ((16, 1024), (32, 512)):
        forms[f"windows_r{rows}_n{n}"] = Windows(eng, units, g, stream, rows, n)
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, form in forms.items():
            ms[k].append(timed(form))
    torch.cuda.synchronize()
    # the same conversion: the window forms against the baseline's waveform
    base = forms["ragged_b1"].out.reshape(-1)
    res = {"frames": frames, "dtype": "bf16x", "rounds": rounds, "forms": {}}
    for k, form in forms.items():
        mid = sorted(ms[k])[len(ms[k]) // 2]
        err = float(((form.out.reshape(-1) - base).double() ** 2).sum())
        res["forms"][k] = {"ms_per_utterance": mid, "ms_rounds": [round(v, 3) for v in ms[k]], "us_per_frame": mid * 1e3 / frames,
                           "calls_per_utterance": form.calls, "workspace_bytes": int(form.workspace_bytes),
                           "vs_ragged_b1": mid / sorted(ms["ragged_b1"])[len(ms["ragged_b1"]) // 2],
                           "snr_db_vs_ragged_b1": None if err == 0 else 10.0 * torch.log10((base.double() ** 2).sum() / err).item(),
                           "bit_equal_to_ragged_b1": err == 0}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
