"""Times the speaker-encoder launches (qvc_speaker_embed) against torch.nn.LSTM on the same GPU.
usage: python tools/spk_bench.py [utterances ...]
       python tools/spk_bench.py --ragged [rows ...]     ragged batches (qvc_speaker_embed_ragged): rows of 100-400 mel
                                                         frames (2-8 s) against the uniform call at 400 frames and
                                                         against one call per row"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quickvc_official_amd as q  # noqa: E402
from quickvc_official_amd.synth import make_synthetic_mel, make_synthetic_state_dict  # noqa: E402


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def ragged_leg(model, rows):
    eng = model.engine()
    gen = torch.Generator().manual_seed(3)
    for U in rows or [64, 512]:
        frames = torch.randint(100, 401, (U,), generator=gen)
        frames[0] = 400
        base = torch.cat([make_synthetic_mel(400, 80, seed=u % 32) for u in range(min(U, 32))], 0).cuda()
        mel = base.repeat((U + 31) // 32, 1, 1)[:U].contiguous()
        fr = frames.to(device="cuda", dtype=torch.int32)
        g = eng.speaker_embed_ragged(mel, fr)
        same = all(torch.equal(g[u:u + 1], eng.speaker_embed(mel[u:u + 1, :, :int(frames[u])])) for u in range(0, U, max(1, U // 8)))
        t_rag = timed(lambda: eng.speaker_embed_ragged(mel, fr))
        t_uni = timed(lambda: eng.speaker_embed(mel))
        t_one = timed(lambda: eng.speaker_embed(mel[:1, :, :250]))
        print(f"rows={U:4d} F=100..400: ragged {t_rag:.3f} ms, uniform at 400 frames {t_uni:.3f} ms, one row of 250 frames "
              f"{t_one:.3f} ms (x{U} = {t_one * U:.1f} ms one call per row), rows equal single calls: {same}", flush=True)


def main():
    model = q.SynthesizerTrn(641, 32, **q.DEFAULT_MODEL_CONFIG)
    model.load_state_dict(make_synthetic_state_dict(model, 1234))
    model = model.cuda().eval()
    if "--ragged" in sys.argv[1:]:
        ragged_leg(model, [int(x) for x in sys.argv[1:] if x != "--ragged"])
        return
    for U in [int(x) for x in sys.argv[1:]] or [1, 32]:
        mel = torch.cat([make_synthetic_mel(250, 80, seed=u) for u in range(U)], 0).cuda()
        g = model.speaker_embed(mel)
        ref = torch.cat([model.enc_spk.embed_utterance(m[None].transpose(1, 2)) for m in mel], 0)
        err = ((g - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
        t_hip = timed(lambda: model.speaker_embed(mel))
        t_torch = timed(lambda: model.enc_spk.embed_utterance(mel[:1].transpose(1, 2)), n=5)
        print(f"U={U:3d} F=250: HIP {t_hip:.3f} ms for all utterances, torch.nn.LSTM {t_torch:.3f} ms per utterance, "
              f"rel err vs torch fp32 {err:.2e}", flush=True)


if __name__ == "__main__":
    main()
