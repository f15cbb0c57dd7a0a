"""The counter-based noise generator (csrc/qvc_kernels.h: philox4x32_10, noise_normal4; include/qvc.h: qvc_noise_rng), on
the host: no GPU.

This file holds the generator's RESTATEMENT in numpy -- uint64 arithmetic for Philox4x32-10, float64 for the Box-Muller
transform -- written from DESIGN.md's recipe, not from the C++.  It is what tests/test_gpu_native_noise.py compares
qvc_noise_fill against.  Checked here: the Random123 known answers, the statistics of the draw, the exported symbols, an
AddressSanitizer + UBSan build of a stand-alone program that calls the host instantiation of the same inlined function,
the CLI's new flags and the engine's argument check.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT

M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------ the restatement
def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (values < 2^32) of one shape, key: two -> four uint64 arrays (values < 2^32)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def counters(seed, key, frame, group):
    """(counter, key) of the call that yields channels 4*group .. 4*group+3 at `frame` for utterance key `key`."""
    seed, key = int(seed) & (2 ** 64 - 1), int(key) & (2 ** 64 - 1)
    frame = np.asarray(frame, dtype=np.int64).astype(np.uint64) & M32              # the absolute frame as uint32
    group = np.asarray(group, dtype=np.uint64)
    frame, group = np.broadcast_arrays(frame, group)
    full = lambda v: np.full(frame.shape, v, dtype=np.uint64)
    return (frame, group, full(key & 0xFFFFFFFF), full(key >> 32)), (full(seed & 0xFFFFFFFF), full(seed >> 32))


def normals4(seed, key, frame, group, scale=1.0):
    """float64 (..., 4): the normals of channels 4*group .. 4*group+3."""
    ctr, k = counters(seed, key, frame, group)
    x = philox4x32_10(ctr, k)
    out = []
    for h in range(2):
        u1 = ((x[2 * h] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24        # (0, 1]
        u2 = (x[2 * h + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24                     # [0, 1)
        r = np.sqrt(-2.0 * np.log(u1))
        out += [r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)]
    return np.stack(out, axis=-1) * scale


def noise_tensor(seed, keys, channels, frames, frame0=0, scale=1.0):
    """What qvc_noise_fill writes: float64 (rows, channels, frames) for frames [frame0, frame0 + frames)."""
    assert channels % 4 == 0
    t = np.arange(frame0, frame0 + frames)[None, :]
    g = np.arange(channels // 4)[:, None]
    rows = []
    for key in keys:
        n = normals4(seed, key, t, g, scale)                                   # (groups, frames, 4)
        rows.append(n.transpose(0, 2, 1).reshape(channels, frames))
    return np.stack(rows)


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """The three Random123 known-answer vectors of philox4x32-10."""
    got = philox4x32_10([np.array([c]) for c in ctr], [np.array([k]) for k in key])
    assert tuple(int(g[0]) for g in got) == want


def test_statistics_of_the_draw():
    """4096 frames x 256 channels of one key (1e6 draws): moments and correlations.  The sampling error at 1e6 draws is
    1e-3 for mean and variance, 5e-3 for the kurtosis and 1e-3 for a correlation."""
    n = noise_tensor(seed=20240611, keys=[7], channels=256, frames=4096)[0]     # (256, 4096)
    mean, var = n.mean(), n.var()
    kurt = ((n - mean) ** 4).mean() / var ** 2
    print(f"mean {mean:.4f} var {var:.4f} kurtosis {kurt:.3f} max |n| {np.abs(n).max():.2f}")
    assert abs(mean) < 0.01 and abs(var - 1.0) < 0.01 and abs(kurt - 3.0) < 0.05
    assert np.isfinite(n).all() and np.abs(n).max() <= np.sqrt(48 * np.log(2.0)) + 1e-9     # u1 >= 2^-24

    def corr(a, b):
        return float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1])
    frames = corr(n[:, :-1], n[:, 1:])
    q = n.reshape(64, 4, 4096)                                                  # (group, channel of the call, frame)
    within = [corr(q[:, i], q[:, j]) for i in range(4) for j in range(i + 1, 4)]
    groups = corr(q[:-1], q[1:])                                                # the same channel slot of neighbouring calls
    print(f"corr frames {frames:.1e} groups {groups:.1e} within a call {max(abs(c) for c in within):.1e}")
    assert abs(frames) < 0.01 and abs(groups) < 0.01 and all(abs(c) < 0.01 for c in within)
    # another key, another seed: unrelated draws
    other = noise_tensor(seed=20240611, keys=[8], channels=256, frames=4096)[0]
    reseed = noise_tensor(seed=20240612, keys=[7], channels=256, frames=4096)[0]
    assert abs(corr(n, other)) < 0.01 and abs(corr(n, reseed)) < 0.01


def test_layout_of_the_restatement():
    """Channel c of frame t is element c % 4 of the call (frame t, group c // 4); frame0 shifts the frames, the scale
    multiplies, equal keys give equal rows."""
    a = noise_tensor(3, [5, 9, 5], 8, 6, frame0=5)
    assert a.shape == (3, 8, 6) and np.array_equal(a[0], a[2]) and not np.array_equal(a[0], a[1])
    assert a[1, 6, 2] == normals4(3, 9, 7, 1)[2]
    assert np.array_equal(noise_tensor(3, [9], 8, 3, frame0=8)[0], a[1][:, 3:])
    assert np.array_equal(noise_tensor(3, [9], 8, 6, frame0=5, scale=0.5)[0], 0.5 * a[1])
    # keys and seeds use all 64 bits
    assert not np.array_equal(noise_tensor(3, [9 + 2 ** 32], 8, 6, 5)[0], a[1])
    assert not np.array_equal(noise_tensor(3 + 2 ** 32, [9], 8, 6, 5)[0], a[1])


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    from quickvc_official_amd import lib as L
    return L.load_library()


NEW_SYMBOLS = ("qvc_infer_batch_ragged_rng", "qvc_infer_batch_ragged_rng_fm", "qvc_infer_fanout_ragged_rng",
               "qvc_infer_fanout_ragged_rng_fm", "qvc_stream_step_rng", "qvc_noise_fill")


def test_new_symbols_are_exported_and_the_abi_version_stays(built):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qvc.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/qvc.h"
        assert hasattr(built, name), f"{name} is not exported"
        assert getattr(built, name).argtypes is not None, f"{name} has no binding in lib.py"
    assert "typedef struct qvc_noise_rng" in header
    assert built.qvc_abi_version() == 8
    # null descriptor / null keys / a channel count the groups of four do not divide: refused on the host, nothing launched
    assert built.qvc_noise_fill(1, None, 1.0, 1, 8, 4, 0, None, None) == -1
    import ctypes
    from quickvc_official_amd import lib as L
    assert built.qvc_infer_batch_ragged_rng(None, None, None, None, None, None, 1, 4, None, None, 0, None) == -1
    assert ctypes.sizeof(L.QvcNoiseRng) == 24                           # uint64, pointer, float + padding: the C struct


HOST_MAIN = r"""
// Stand-alone caller of the HOST instantiation of the generator (csrc/qvc_kernels.h), built with ASan + UBSan.
#include <cinttypes>
#include <cstdio>
#include "qvc_kernels.h"
int main() {
  const uint64_t seed = 0x0123456789abcdefull;
  const uint64_t keys[4] = {0ull, 7ull, 0xffffffffffffffffull, 0x100000002ull};
  const uint32_t frames[6] = {0u, 1u, 17u, 250u, 0x7fffffffu, 0xffffffffu};
  uint64_t x_or = 0, sum = 0, n = 0;
  double nsum = 0.0, nabs = 0.0;
  for (uint64_t key : keys)
    for (uint32_t f0 : frames)
      for (uint32_t df = 0; df < 8; ++df)
        for (uint32_t g = 0; g < 24; ++g) {
          const uint32_t f = f0 + df;     // wraps at 2^32, as the kernels' uint32 frame does
          const qvc::U32x4 x = qvc::philox4x32_10(f, g, (uint32_t)key, (uint32_t)(key >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
          const qvc::Normal4 z = qvc::noise_normal4((uint32_t)seed, (uint32_t)(seed >> 32), key, f, g, 1.0f);
          for (int i = 0; i < 4; ++i) {
            x_or ^= (uint64_t)x.v[i] << (8 * (n % 5));
            sum += (uint64_t)x.v[i] * (n + 1);
            nsum += z.v[i]; nabs += z.v[i] < 0 ? -z.v[i] : z.v[i];
            ++n;
          }
        }
  std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %.9f %.9f\n", n, x_or, sum, nsum, nabs);
  return 0;
}
"""


def test_host_instantiation_under_asan_ubsan(tmp_path):
    """A -fsanitize=address,undefined build of a stand-alone program (its own main) that calls the host-callable
    generator over 4608 counters: clean under both sanitizers, the integer side equal to the restatement bit for bit
    (two checksums over every Philox word), the normals equal within fp32 evaluation error."""
    src = tmp_path / "noise_host_main.cpp"
    src.write_text(HOST_MAIN)
    exe = str(tmp_path / "noise_host_main")
    csrc = os.path.join(ROOT, "quickvc-official_amd", "csrc")
    res = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", csrc, "-o", exe, str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0 and run.stderr == "", run.stderr
    n, x_or, total, nsum, nabs = run.stdout.split()

    seed = 0x0123456789abcdef
    want_or = want_sum = count = 0
    want_nsum = want_nabs = 0.0
    for key in (0, 7, 2 ** 64 - 1, 0x100000002):
        for f0 in (0, 1, 17, 250, 0x7fffffff, 0xffffffff):
            f = (np.arange(8, dtype=np.int64)[:, None] + f0) & 0xFFFFFFFF
            g = np.arange(24, dtype=np.int64)[None, :]
            ctr, k = counters(seed, key, f, g)
            words = np.stack(philox4x32_10(ctr, k), axis=-1).reshape(-1)          # order: df, g, word
            z = normals4(seed, key, f, g).reshape(-1)
            for w in words.tolist():
                want_or ^= (w << (8 * (count % 5))) & (2 ** 64 - 1)
                want_sum = (want_sum + w * (count + 1)) & (2 ** 64 - 1)
                count += 1
            want_nsum += float(z.sum())
            want_nabs += float(np.abs(z).sum())
    assert int(n) == count == 4 * 4 * 6 * 8 * 24
    assert int(x_or) == want_or and int(total) == want_sum
    # per value: |r| <= 5.77, the fp32 rounding of 2 pi u2 and a few ulp in logf / sqrtf / sincosf -> 6e-6
    tol = count * 6e-6
    assert abs(float(nsum) - want_nsum) <= tol and abs(float(nabs) - want_nabs) <= tol, (nsum, want_nsum, nabs, want_nabs)


def test_cli_lists_the_noise_flags():
    res = subprocess.run([sys.executable, "-m", "quickvc_official_amd.convert", "--help"], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    assert "--noise {torch,native}" in res.stdout and "--noise-scale" in res.stdout


def test_engine_wants_exactly_one_of_noise_and_rng():
    """QvcEngine's draw argument check (infer_batch_ragged, infer_fanout_ragged, stream_step go through it before they
    touch the device): both or neither of noise and rng is a ValueError; so is a key list of the wrong length."""
    from quickvc_official_amd.engine import QvcEngine
    eng = object.__new__(QvcEngine)                                   # no device here: the check needs none
    noise = torch.zeros(2, 32, 23)
    with pytest.raises(ValueError, match="exactly one"):
        eng._draw(None, None, 2, (2, 32, 23))
    with pytest.raises(ValueError, match="exactly one"):
        eng._draw(noise, (1, [0, 1], 1.0), 2, (2, 32, 23))
    eng.device = torch.device("cpu")
    with pytest.raises(ValueError, match="keys"):
        eng._draw(None, (1, [0, 1, 2], 1.0), 2, (2, 32, 23))
    with pytest.raises(ValueError, match="rng must be"):
        eng._draw(None, 5, 2, (2, 32, 23))
    with pytest.raises(ValueError, match="noise must be"):
        eng._draw(torch.zeros(2, 32, 22), None, 2, (2, 32, 23))
    n, desc, keys = eng._draw(None, (2 ** 64 - 1, [0, 2 ** 63 + 5], 0.5), 2, (2, 32, 23))
    assert n is None and desc.seed == 2 ** 64 - 1 and desc.scale == 0.5
    assert keys.dtype == torch.int64 and keys.tolist() == [0, 2 ** 63 + 5 - 2 ** 64]     # the same 64 bits
