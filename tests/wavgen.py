"""A small RIFF writer for the wav I/O tests (tests/test_wav_io_host.py, tests/test_gpu_wav_io.py): scipy cannot write
24-bit or extensible files, and the tests need extra chunks, odd chunk sizes and damaged headers."""
import struct

import numpy as np

FORMATS = ("u8", "s16", "s24", "s32", "f32")
CODE = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 5}               # QVC_PCM_* of include/qvc_io.h
BYTES = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}
GUID_TAIL = b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xAA\x00\x38\x9B\x71"


def samples(fmt, frames, channels, seed):
    """(frames, channels) test data of a format, its extreme values and (for s32) values that round in float32 among them."""
    rng = np.random.RandomState(seed)
    n = frames * channels
    if fmt == "u8":
        x = rng.randint(0, 256, size=n).astype(np.uint8)
        edge = [0, 255, 128, 127]
    elif fmt == "s16":
        x = rng.randint(-32768, 32768, size=n).astype(np.int16)
        edge = [-32768, 32767, 0, -1]
    elif fmt == "s24":
        x = rng.randint(-(1 << 23), 1 << 23, size=n).astype(np.int32)
        edge = [-(1 << 23), (1 << 23) - 1, 0, -1]
    elif fmt == "s32":
        x = rng.randint(-(1 << 31), 1 << 31, size=n, dtype=np.int64).astype(np.int32)
        edge = [-(1 << 31), (1 << 31) - 1, (1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 31) - 65, (1 << 31) - 64, 3]
    elif fmt == "f32":
        x = (rng.randn(n) * 0.3).astype(np.float32)
        edge = [1.0, -1.0, 0.0, 1e-39, -1e-39, 1.17549435e-38, 3.0]       # denormals too; no NaN (torch.equal could not compare it)
    elif fmt == "f64":
        x = rng.randn(n) * 0.3
        edge = [1.0, -1.0]
    else:
        raise ValueError(fmt)
    k = min(len(edge), n)
    x[:k] = np.asarray(edge[:k], dtype=x.dtype)
    return x.reshape(frames, channels)


def payload(fmt, data):
    """The little-endian interleaved bytes of (frames, channels) data."""
    if fmt == "s24":
        b = data.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3]
        return np.ascontiguousarray(b).tobytes()
    dt = {"u8": "u1", "s16": "<i2", "s32": "<i4", "f32": "<f4", "f64": "<f8"}[fmt]
    return np.ascontiguousarray(data.astype(dt)).tobytes()


def chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")


def fmt_chunk(fmt, channels, rate, extensible=False, tag=None, bits=None, block_align=None):
    nbytes = BYTES[fmt]
    bits = 8 * nbytes if bits is None else bits
    block_align = nbytes * channels if block_align is None else block_align
    tag = (3 if fmt in ("f32", "f64") else 1) if tag is None else tag
    head = struct.pack("<HIIHH", channels, rate, rate * block_align, block_align, bits)
    if not extensible:
        return chunk(b"fmt ", struct.pack("<H", tag) + head)
    ext = struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + GUID_TAIL
    return chunk(b"fmt ", struct.pack("<H", 0xFFFE) + head + ext)


def wav_bytes(fmt, data, rate=16000, extensible=False, extra="none", declared=None, riff=b"RIFF", **fmt_kw):
    """A whole file: `extra` = "none", "before" (an odd-sized LIST chunk in front of data: its pad byte must be skipped) or
    "after" (a chunk behind data); `declared` overrides the data chunk's size field."""
    body = payload(fmt, data)
    dchunk = b"data" + struct.pack("<I", len(body) if declared is None else declared) + body + (b"\x00" if len(body) & 1 else b"")
    parts = [fmt_chunk(fmt, data.shape[1], rate, extensible, **fmt_kw)]
    if extra == "before":
        parts.append(chunk(b"LIST", b"INFOabc"))                          # 7 bytes + pad
    parts.append(dchunk)
    if extra == "after":
        parts.append(chunk(b"LIST", b"INFOxyzzy"))
    rest = b"WAVE" + b"".join(parts)
    return riff + struct.pack("<I", len(rest)) + rest


def write_wav(path, fmt, frames, channels=1, seed=0, **kw):
    """Writes the file, returns its (frames, channels) data."""
    data = samples(fmt, frames, channels, seed)
    with open(path, "wb") as f:
        f.write(wav_bytes(fmt, data, **kw))
    return data


def damaged_corpus(count=300, seed=1234):
    """`count` byte strings: a valid file (extensible s16 stereo, a LIST chunk, 9 frames) cut at every length, then copies
    with 1 .. 4 random header bytes overwritten."""
    good = wav_bytes("s16", samples("s16", 9, 2, 3), extensible=True, extra="before")
    out = [good[:n] for n in range(len(good))][:count]
    rng = np.random.RandomState(seed)
    head = len(good) - 36                                                  # everything in front of the payload
    while len(out) < count:
        b = bytearray(good)
        for _ in range(rng.randint(1, 5)):
            b[rng.randint(0, head)] = rng.randint(0, 256)
        out.append(bytes(b))
    return out
