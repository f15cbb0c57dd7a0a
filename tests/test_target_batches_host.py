"""CPU tests (no GPU) of the ragged target-batch entry points: qvc_trim_bounds, qvc_wave_to_mel_ragged,
qvc_speaker_embed_ragged and their workspace queries (include/qvc.h), plus the host logic that cuts a shard's
targets into batches (convert.py)."""
import ctypes
import sys

import numpy as np
import pytest

from helpers import ROOT

NEW_SYMBOLS = ("qvc_trim_workspace_bytes", "qvc_trim_bounds", "qvc_mel_ragged_workspace_bytes", "qvc_wave_to_mel_ragged",
               "qvc_spk_ragged_workspace_bytes", "qvc_speaker_embed_ragged")


@pytest.fixture(scope="module")
def built():
    """Build (or reuse) the product library; host entry points only."""
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from quickvc_official_amd import lib as L
    return L.load_library()


def _cfg(**over):
    import quickvc_official_amd as q
    from quickvc_official_amd import lib as L
    cfg = L.make_config(dict(q.MINI_MODEL_CONFIG))
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def test_new_symbols_are_exported_and_the_abi_version_stays(built):
    for n in NEW_SYMBOLS:
        assert hasattr(built, n), n
    assert built.qvc_abi_version() == 8
    header = open(f"{ROOT}/include/qvc.h").read()
    for n in NEW_SYMBOLS:
        assert n + "(" in header, n


def test_spk_ragged_workspace_query(built):
    cfg = _cfg()
    q = lambda U, F: int(built.qvc_spk_ragged_workspace_bytes(ctypes.byref(cfg), U, F))
    prev = 0
    for U, F in ((1, 1), (1, 128), (1, 129), (1, 321), (19, 321), (19, 400), (64, 400)):
        n = q(U, F)
        assert n > 0 and n % 256 == 0 and n >= prev, (U, F, n, prev)
        # the uniform layout at the cap plus the partial map
        assert n > int(built.qvc_spk_workspace_bytes(ctypes.byref(cfg), U, F))
        prev = n
    assert q(0, 100) == -1 and q(-3, 100) == -1 and q(4, 0) == -1
    assert int(built.qvc_spk_ragged_workspace_bytes(None, 4, 100)) == -1
    bad = _cfg(gin_channels=300)
    assert int(built.qvc_spk_workspace_bytes(ctypes.byref(bad), 4, 100)) == -2
    assert int(built.qvc_spk_ragged_workspace_bytes(ctypes.byref(bad), 4, 100)) == -2


def test_mel_ragged_workspace_query(built):
    q = lambda U, N, n_fft=1280, hop=320: int(built.qvc_mel_ragged_workspace_bytes(n_fft, hop, U, N))
    prev = 0
    for U, N in ((1, 641), (1, 2000), (4, 2000), (4, 80000), (64, 80000)):
        n = q(U, N)
        assert n > 0 and n % 256 == 0 and n >= prev, (U, N)
        assert n == int(built.qvc_mel_workspace_bytes(1280, 320, U, N))
        prev = n
    assert q(0, 16000) == -1 and q(2, 0) == -1
    assert q(2, 480) == int(built.qvc_mel_workspace_bytes(1280, 320, 2, 480)) == -1      # no row can have a frame
    assert q(2, 16000, n_fft=1000) == int(built.qvc_mel_workspace_bytes(1000, 320, 2, 16000)) == -2


def test_trim_workspace_query(built):
    q = lambda U, N, fl=2048, hop=512: int(built.qvc_trim_workspace_bytes(U, N, fl, hop))
    prev = 0
    for U, N in ((1, 1), (1, 2048), (5, 2048), (5, 128000), (64, 128000)):
        n = q(U, N)
        assert n > 0 and n % 256 == 0 and n >= prev, (U, N)
        assert n >= U * -(-N // 512) * 4
        prev = n
    assert q(0, 16000) == -1 and q(3, 0) == -1
    assert q(3, 16000, fl=2048, hop=500) == -2 and q(3, 16000, fl=1000, hop=1000) == -2 and q(3, 16000, hop=0) == -2


def test_null_pointers_are_refused_before_anything_is_launched(built):
    cfg = _cfg()
    assert built.qvc_speaker_embed_ragged(ctypes.byref(cfg), None, None, None, None, 1, 50, None, 0, None) == -1
    assert built.qvc_wave_to_mel_ragged(None, 1280, 320, 80, None, None, None, None, None, 1, 16000, None, 0, None) == -1
    assert built.qvc_trim_bounds(None, None, None, None, 1, 16000, 20.0, 2048, 512, None, 0, None) == -1


def test_target_chunks_and_wav_header_lengths(built, tmp_path):
    """convert.py cuts the length-sorted targets into chunks of at most 64 rows / about 64 MB of padded upload, and
    sorts them by the sample count load_wav will return -- read from the wav header alone."""
    from scipy.io import wavfile
    from quickvc_official_amd.convert import target_chunks, wav_samples
    from quickvc_official_amd.frontend import load_wav
    assert target_chunks([]) == []
    assert target_chunks([5] * 64) == [(0, 64)]
    assert target_chunks([5] * 65) == [(0, 64), (64, 65)]
    counts = sorted([100, 200, 300, 4000, 5000])
    assert target_chunks(counts, rows=2) == [(0, 2), (2, 4), (4, 5)]
    chunks = target_chunks(counts, rows=64, max_bytes=4 * 4000)              # 4000 floats of padded batch at most
    assert chunks == [(0, 3), (3, 4), (4, 5)]
    for lo, hi in chunks[:1]:
        assert (hi - lo) * counts[hi - 1] * 4 <= 4 * 4000
    rng = np.random.RandomState(1)
    for rate, n, dt in ((16000, 12345, np.int16), (22050, 7001, np.int16), (48000, 9999, np.float32), (8000, 4000, np.int16)):
        x = rng.uniform(-0.5, 0.5, n)
        p = str(tmp_path / f"w_{rate}.wav")
        wavfile.write(p, rate, (x * 32767).astype(np.int16) if dt == np.int16 else x.astype(np.float32))
        assert wav_samples(p, 16000) == len(load_wav(p, 16000)), rate
