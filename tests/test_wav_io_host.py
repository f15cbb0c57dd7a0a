"""CPU tests (no GPU) of the wav side of libqvc_io.so (include/qvc_io.h): the header reader against scipy.io.wavfile.read
over a matrix of sample formats, channel counts, header forms, extra chunks and lengths; what it refuses; raw payloads
into byte slots; damaged headers; the 16-bit writer against scipy.io.wavfile.write; and the .npy header that used to
throw from a pool thread."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import wavgen
from helpers import ROOT

OK, ERR_OPEN, ERR_FORMAT, ERR_SHAPE, ERR_IO = 0, -2, -3, -4, -5


@pytest.fixture(scope="module")
def fileio():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from quickvc_official_amd import fileio
    return fileio


@pytest.fixture(scope="module")
def pool(fileio):
    p = fileio.IoPool(4)
    yield p
    p.close()


def _scipy_read(path):
    from scipy.io import wavfile
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rate, data = wavfile.read(path)
    return rate, (1 if data.ndim == 1 else data.shape[1]), data.shape[0]


def test_every_declared_symbol_is_exported_and_the_abi_is_8(fileio):
    from quickvc_official_amd import lib as L
    for header, lib, prefix, new in (("qvc_io.h", fileio.load_library(), "qvc_io_", ("qvc_io_wav_headers", "qvc_io_load_wavs", "qvc_io_write_wavs_pcm16")),
                                     ("qvc.h", L.load_library(), "qvc_", ("qvc_pcm_to_wave_ragged", "qvc_wave_to_pcm16"))):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        names = set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text))
        assert set(new) <= names, (header, set(new) - names)
        for n in sorted(names):
            assert hasattr(lib, n), f"{n} declared in include/{header} but not exported"
    assert L.load_library().qvc_abi_version() == 8
    assert "#define QVC_ABI_VERSION 8" in open(os.path.join(ROOT, "include", "qvc.h")).read()


def test_headers_equal_scipy_over_the_format_matrix(pool, tmp_path):
    paths = []
    for fmt in wavgen.FORMATS:
        for ch in (1, 2, 3):
            for ext in (False, True):
                for extra in ("none", "before", "after"):
                    for frames in (0, 1, 7, 1001):
                        p = str(tmp_path / f"{fmt}_{ch}_{int(ext)}_{extra}_{frames}.wav")
                        wavgen.write_wav(p, fmt, frames, ch, seed=len(paths), rate=16000 + len(paths), extensible=ext, extra=extra)
                        paths.append((p, fmt, ch))
    assert len(paths) == 360
    hdr, st = pool.wav_headers([p for p, _, _ in paths])
    assert st == [OK] * len(paths)
    for i, (p, fmt, ch) in enumerate(paths):
        h = hdr[i]
        assert (h.rate, h.channels, h.frames) == _scipy_read(p), p
        assert (h.code, h.bits) == (wavgen.CODE[fmt], 8 * wavgen.BYTES[fmt]), p
        blob = open(p, "rb").read()
        assert blob[h.data_offset - 8:h.data_offset - 4] == b"data", p


def test_headers_of_the_golden_recording_and_of_a_truncated_file(pool, tmp_path):
    golden = os.path.join(ROOT, "tests", "golden", "p225_001.wav")
    data = wavgen.samples("s16", 100, 2, 5)
    whole = wavgen.wav_bytes("s16", data, declared=4 * 100 + 4000)       # declares 1000 frames more than it holds
    cut = str(tmp_path / "cut.wav")
    open(cut, "wb").write(whole)
    mid = str(tmp_path / "mid.wav")
    open(mid, "wb").write(wavgen.wav_bytes("s24", wavgen.samples("s24", 50, 1, 6))[:-31])   # ends inside a frame: 39 whole frames + 2 bytes
    hdr, st = pool.wav_headers([golden, cut, mid])
    assert st == [OK, OK, OK]
    assert (hdr[0].rate, hdr[0].channels, hdr[0].frames) == _scipy_read(golden)
    assert (hdr[1].rate, hdr[1].channels, hdr[1].frames) == _scipy_read(cut) == (16000, 2, 100)
    assert (hdr[2].rate, hdr[2].channels, hdr[2].frames) == (16000, 1, 39)


def test_refusals_have_their_own_status_and_spare_the_good_file(pool, tmp_path):
    s16 = wavgen.samples("s16", 12, 1, 1)
    good = wavgen.wav_bytes("s16", s16)
    cases = {
        "rifx": wavgen.wav_bytes("s16", s16, riff=b"RIFX"),
        "f64": wavgen.wav_bytes("f64", wavgen.samples("f64", 12, 1, 2)),
        "adpcm": wavgen.wav_bytes("s16", s16, tag=2),
        "bits12": wavgen.wav_bytes("s16", s16, bits=12),
        "nofmt": good[:12] + good[12 + 24:],
        "nodata": good[:12 + 24],
        "align": wavgen.wav_bytes("s16", wavgen.samples("s16", 12, 2, 3), block_align=2),
        "empty": b"",
    }
    names = list(cases)
    paths = []
    for n in names:
        paths.append(str(tmp_path / f"{n}.wav"))
        open(paths[-1], "wb").write(cases[n])
    paths.insert(3, str(tmp_path / "good.wav"))
    names.insert(3, "good")
    open(paths[3], "wb").write(good)
    hdr, st = pool.wav_headers(paths)
    assert dict(zip(names, st)) == {n: (OK if n == "good" else ERR_FORMAT) for n in names}
    assert (hdr[3].rate, hdr[3].channels, hdr[3].code, hdr[3].frames) == (16000, 1, 2, 12)
    lib = pool.lib
    from quickvc_official_amd.fileio import WavHeader, _paths
    import ctypes
    out, status = (WavHeader * len(paths))(), (ctypes.c_int32 * len(paths))()
    assert lib.qvc_io_wav_headers(pool._h, _paths(paths), len(paths), out, status) == ERR_FORMAT     # the first non-OK status
    assert lib.qvc_io_wav_headers(pool._h, _paths(paths[3:4]), 1, out, None) == OK


def test_load_wavs_copies_the_payload_and_nothing_else(pool, tmp_path):
    specs = [("u8", 2, 33), ("s16", 1, 1001), ("s24", 1, 7), ("s24", 2, 5), ("s32", 2, 64), ("f32", 1, 0), ("f32", 2, 19)]
    paths, bodies = [], []
    for i, (fmt, ch, frames) in enumerate(specs):
        p = str(tmp_path / f"l{i}.wav")
        data = wavgen.write_wav(p, fmt, frames, ch, seed=40 + i, extra=("none", "before", "after")[i % 3], extensible=bool(i & 1))
        paths.append(p)
        bodies.append(wavgen.payload(fmt, data))
    slot = max(len(b) for b in bodies)
    dst = torch.full((len(paths) * slot,), 0xA5, dtype=torch.uint8)
    hdr, st = pool.load_wavs(paths, dst, slot)
    assert st == [OK] * len(paths)
    for i, b in enumerate(bodies):
        got = dst[i * slot:(i + 1) * slot].numpy()
        assert got[:len(b)].tobytes() == b, specs[i]
        assert (got[len(b):] == 0xA5).all(), specs[i]
        assert (hdr[i].code, hdr[i].channels, hdr[i].frames) == (wavgen.CODE[specs[i][0]], specs[i][1], specs[i][2])
    # a slot one byte too small for the longest payload, a missing path: their own statuses, the others still load
    dst.fill_(0xA5)
    longest = max(range(len(bodies)), key=lambda i: len(bodies[i]))
    small = torch.full(((len(paths) + 1) * (slot - 1),), 0xA5, dtype=torch.uint8)
    hdr, st = pool.load_wavs(paths + [str(tmp_path / "missing.wav")], small, slot - 1)
    assert st == [ERR_SHAPE if i == longest else OK for i in range(len(paths))] + [ERR_OPEN]
    assert (small[longest * (slot - 1):(longest + 1) * (slot - 1)] == 0xA5).all()      # the refused payload wrote nothing
    with pytest.raises(ValueError):
        pool.load_wavs(paths, dst[:slot], slot)


def test_damaged_headers_always_return_a_status(pool, tmp_path):
    blobs = wavgen.damaged_corpus(300)
    assert len(blobs) == 300 and len(set(blobs)) > 250
    paths = []
    for i, b in enumerate(blobs):
        paths.append(str(tmp_path / f"d{i}.wav"))
        open(paths[-1], "wb").write(b)
    hdr, st = pool.wav_headers(paths)
    assert set(st) <= {OK, ERR_FORMAT} and ERR_FORMAT in st
    slot = 64
    dst = torch.zeros(len(paths) * slot, dtype=torch.uint8)
    hdr2, st2 = pool.load_wavs(paths, dst, slot)
    assert set(st2) <= {OK, ERR_FORMAT, ERR_SHAPE, ERR_IO}
    for i in range(len(paths)):
        assert (st2[i] == ERR_FORMAT) == (st[i] == ERR_FORMAT), i
        if st[i] == OK:                                                    # what it accepted is self-consistent
            assert hdr[i].channels >= 1 and hdr[i].frames >= 0 and 0 < hdr[i].data_offset <= len(blobs[i])
            assert hdr[i].frames * hdr[i].channels * (hdr[i].bits // 8) <= len(blobs[i]) - hdr[i].data_offset


def test_write_wavs_pcm16_equals_scipy(pool, tmp_path):
    from scipy.io import wavfile
    rng = np.random.RandomState(8)
    lens = (0, 1, 4097)
    src = torch.from_numpy(rng.randint(-32768, 32768, size=(3, 4100)).astype(np.int16))
    outs = [str(tmp_path / f"o{i}.wav") for i in range(3)]
    pool.write_wavs_pcm16(outs, src, lens, 16000)
    for i, n in enumerate(lens):
        ref = str(tmp_path / f"r{i}.wav")
        wavfile.write(ref, 16000, src[i, :n].numpy())
        assert open(ref, "rb").read() == open(outs[i], "rb").read(), n
    hdr, st = pool.wav_headers(outs)
    assert st == [OK] * 3 and [h.frames for h in hdr] == list(lens)
    with pytest.raises(ValueError):
        pool.write_wavs_pcm16(outs, src.float(), lens, 16000)


def test_npy_header_with_only_spaces_after_fortran_order_is_a_format_error(fileio, pool, tmp_path):
    head = b"{'descr': '<f4', 'shape': (3, 256), 'fortran_order':"
    head += b" " * (118 - len(head))
    p = str(tmp_path / "spaces.npy")
    open(p, "wb").write(b"\x93NUMPY\x01\x00" + bytes([len(head) & 255, len(head) >> 8]) + head + b"\x00" * 3072)
    with pytest.raises(fileio.QvcIoError, match=r"\(-3\)"):
        fileio.npy_shape(p)
    with pytest.raises(fileio.QvcIoError, match=r"\(-3\)"):
        pool.npy_shapes([p])
