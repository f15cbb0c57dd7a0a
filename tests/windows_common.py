"""What the two test files of the exact windows over packed utterances share (tests/test_windows_host.py,
tests/test_gpu_windows.py): the table, the packing and the mini base model."""
import functools

import torch

NEW = ("qvc_windows_workspace_bytes", "qvc_infer_windows_fm", "qvc_infer_windows_rng_fm")
SENTINEL = -12345.0


def table_rows(lengths, n, bases=None):
    """[(base, length, start, count)] of plan_windows over utterances packed back to back (or at `bases`)."""
    from quickvc_official_amd.windows import plan_windows
    if bases is None:
        bases, at = [], 0
        for length in lengths:
            bases.append(at)
            at += length
    return [(bases[u], lengths[u], s, c) for u, s, c in plan_windows(lengths, n)]


def groups_of(rows, per, idle=(0, 0, 0, 0)):
    """The table cut into groups of `per` rows, the last one padded with idle rows -> (groups, per, 4) int32."""
    rows = list(rows)
    while len(rows) % per:
        rows.append(idle)
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, per, 4)


@functools.lru_cache(maxsize=None)
def mini_problem():
    """(model_config, state dict) of the mini base model (MINI_MODEL_CONFIG, synthetic weights); read-only."""
    import quickvc_official_amd as q
    from quickvc_official_amd.synth import make_synthetic_state_dict
    model = q.SynthesizerTrn(641, 32, **q.MINI_MODEL_CONFIG)
    return dict(model.model_config), make_synthetic_state_dict(model, 1234)


@functools.lru_cache(maxsize=None)
def packed_inputs(lengths, inter, gin, seed0, extra=0):
    """Utterances of `lengths` (a tuple) back to back, then `extra` frames that belong to nobody:
    units (total, 256), noise (inter, total), g (U, gin); read-only."""
    from quickvc_official_amd.synth import make_synthetic_inputs
    total = sum(lengths) + extra
    unit, g, noise = make_synthetic_inputs(len(lengths) + 1, max(max(lengths), extra, 2), 256, inter, gin, seed0=seed0)
    units, noises, at = torch.zeros(total, 256), torch.zeros(inter, total), 0
    for u, length in enumerate(tuple(lengths) + ((extra,) if extra else ())):
        units[at:at + length] = unit[u, :, :length].t()
        noises[:, at:at + length] = noise[u, :, :length]
        at += length
    return units.contiguous(), noises.contiguous(), g[:len(lengths)].contiguous()
