#!/usr/bin/env python3
"""tools/pcm_bench.py -- the two sample-format launches alone (frontend.pcm_to_wave, frontend.wave_to_pcm16) on one GPU:
ms per call from device events around back-to-back calls (so a short launch also counts the host's enqueue), the bytes a
call moves (payload read once + floats written once; floats read + int16 written) and that rate as a fraction of the
6.29 TB/s copy rate DESIGN uses as the HBM yardstick.  The 64-row shapes are what one chunk of targets is (and fit the
256 MiB cache); the 2048-row ones are larger than the cache.  One JSON line per shape."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from quickvc_official_amd.frontend import pcm_to_wave, wave_to_pcm16

dev = torch.device("cuda:0")
res = []
for rows, sec, code, ch in ((64, 8, 2, 1), (2048, 8, 2, 1), (64, 8, 3, 2), (2048, 8, 5, 2)):
    n = sec * 16000
    bps = {2: 2, 3: 3, 5: 4}[code] * ch
    slot = -(-n * bps // 16) * 16
    pcm = torch.randint(0, 255, (rows * slot,), dtype=torch.uint8, device=dev)
    table = torch.tensor([[code, ch, n]] * rows, dtype=torch.int32, device=dev)
    for _ in range(20):
        pcm_to_wave(pcm, slot, table, n)
    torch.cuda.synchronize()
    iters = 200 if rows == 64 else 30
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # the wrapper allocates its outputs from torch's cache; time the launches back to back
    e0.record()
    for _ in range(iters):
        pcm_to_wave(pcm, slot, table, n)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    nbytes = rows * n * bps + rows * n * 4
    res.append(dict(kernel="pcm_to_wave", rows=rows, seconds=sec, code=code, channels=ch, ms_per_call=ms, bytes=nbytes,
                    GBps=nbytes / ms / 1e6, frac_of_6290GBps=nbytes / ms / 1e6 / 6290.0))
for numel in (32 * 400 * 320, 256 * 1024 * 1024 // 4 * 3):
    x = torch.randn(numel, device=dev)
    out = torch.empty(numel, dtype=torch.int16, device=dev)
    for _ in range(10):
        wave_to_pcm16(x, out=out)
    torch.cuda.synchronize()
    iters = 100
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        wave_to_pcm16(x, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    res.append(dict(kernel="wave_to_pcm16", n=numel, ms_per_call=ms, bytes=numel * 6, GBps=numel * 6 / ms / 1e6,
                    frac_of_6290GBps=numel * 6 / ms / 1e6 / 6290.0))
for r in res:
    print(json.dumps(r))
