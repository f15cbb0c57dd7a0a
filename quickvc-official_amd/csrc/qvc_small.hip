// qvc_small.hip -- the HBM-bound kernels around the conv trunk:
//   * cond_gemv_kernel   : all 1x1 conditioning convs on g (modules.py:54,84; models.py:328,372)
//   * sample_kernel      : z_p = mu + noise*exp(logs) (models.py:93-94), noise read in (B,C,T)
//   * sample_rows_kernel : the same for R output rows that draw from U <= R encoded sources (fan-out)
//   * sample_rng_kernel / sample_rows_rng_kernel : the two above with the noise computed (noise_normal4), not read
//   * noise_fill_kernel  : that generator's draw written out as a (rows, C, T) tensor
//   * istft_synth_kernel : exp / pi*sin / 16-point inverse real DFT / Hann overlap-add /
//                          envelope / x4 zero-stuff / 63-tap synthesis FIR in ONE pass
//                          (single-band decoder: the overlap-add output is the waveform)
//                          (models.py:394-406, pqmf.py:106-117) -- no complex tensors, no
//                          zero-stuffed intermediate, each post-conv frame read once (+halo).
//   * fm_to_cm_kernel    : frame-major -> (B,C,T) for the unit-test conv entry point.
//   * copy_batch_kernel / copy_counted_kernel : the batched strided copies of the streaming drivers (qvc_stream.h)
//   * window_gather_kernel / window_deliver_kernel : the table-driven movers around the exact windows over packed
//                          utterances (qvc_stream.h: infer_windows)
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <type_traits>
#include "qvc_launch_util.h"
#include "qvc_select.h"
#include "qvc_tail_impl.h"

namespace qvc {

// ------------------------------------------------------------------ cond GEMV
// out[b][row] = bias[row] + sum_k w[row][k] * g[b][k].  A workgroup owns kGR rows x kGB utterances: its weight rows
// (contiguous in memory) and the g vectors ([k][b], so the 32 utterances of one k sit in 32 different banks) are
// staged into LDS with ALL loads of a thread in flight at once -- one memory round trip per workgroup -- and each
// thread then owns one (row, utterance) pair and walks k out of LDS.  ~0.1 GFLOP in total: latency-sized, it only
// has to stay out of the way.  (Round 1 walked the weight row from global memory, 16 loads at a time: four
// dependent round trips per workgroup, 16-19 us.)
constexpr int kGR = 16, kGB = 32, kGS = kGB + 1, kGT = kGR * kGB;
// the g region doubles as the [kGB][kGR + 1] output transpose buffer: small gin must not let that run into the weights
__host__ __device__ constexpr int gemv_g_floats(int gin) { return gin * kGS > kGB * (kGR + 1) ? gin * kGS : kGB * (kGR + 1); }
__global__ __launch_bounds__(kGT) void cond_gemv_kernel(const GemvArgs a) {
  extern __shared__ float s_gv[];                       // [max(gin*kGS, kGB*(kGR+1))] g / output transpose, then [kGR][gin] weights
  float* s_g = s_gv;
  float* s_w = s_gv + gemv_g_floats(a.gin);
  const int tid = threadIdx.x;
  const int r = tid >> 5, bl = tid & 31;
  const int row0 = blockIdx.x * kGR;
  const int row = row0 + r;
  const int wq = (kGR * a.gin) >> 2;                    // float4 pieces of the weight block (gin % 4 == 0)
  const int wlim = (a.rows - row0 < kGR ? a.rows - row0 : kGR) * (a.gin >> 2);
  constexpr int kWU = 4, kGU = 16;
  for (int b0 = 0; b0 < a.batch; b0 += kGB) {
    __syncthreads();
    float4 wv[kWU];
    if (b0 == 0) {
      // (gin <= 512, checked by the launcher: kWU * kGT float4 cover the 16 rows)
#pragma unroll
      for (int u = 0; u < kWU; ++u) {
        const int i = tid + u * kGT;
        wv[u] = i < wlim ? reinterpret_cast<const float4*>(a.w + (size_t)row0 * a.gin)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    const int items = a.gin * kGB;
    for (int base = tid; base < items; base += kGT * kGU) {
      float v[kGU];
#pragma unroll
      for (int u = 0; u < kGU; ++u) {                   // coalesced along k
        const int idx = base + u * kGT;
        const int bb = idx / a.gin, k = idx - bb * a.gin;
        v[u] = (idx < items && b0 + bb < a.batch) ? a.g[(size_t)(b0 + bb) * a.gin + k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kGU; ++u) {
        const int idx = base + u * kGT;
        const int bb = idx / a.gin, k = idx - bb * a.gin;
        if (idx < items) s_g[k * kGS + bb] = v[u];      // [k][kGS] keeps the transposing store conflict-free
      }
    }
    if (b0 == 0) {
#pragma unroll
      for (int u = 0; u < kWU; ++u) {
        const int i = tid + u * kGT;
        if (i < wq) reinterpret_cast<float4*>(s_w)[i] = wv[u];
      }
    }
    __syncthreads();
    float res = 0.f;
    if (row < a.rows && b0 + bl < a.batch) {
      const float* wr = s_w + r * a.gin;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
      int k = 0;
#pragma unroll 8
      for (; k + 4 <= a.gin; k += 4) {
        const float4 w4 = *reinterpret_cast<const float4*>(wr + k);
        s0 = fmaf(w4.x, s_g[(k + 0) * kGS + bl], s0); s1 = fmaf(w4.y, s_g[(k + 1) * kGS + bl], s1);
        s2 = fmaf(w4.z, s_g[(k + 2) * kGS + bl], s2); s3 = fmaf(w4.w, s_g[(k + 3) * kGS + bl], s3);
      }
      res = (s0 + s1) + (s2 + s3) + a.bias[row];
    }
    // the table is [utterance][row]: through LDS, so that 16 neighbouring lanes store the 16 rows of one utterance
    // (64 contiguous bytes) instead of every lane a 4-byte piece of a different 26 KB-apart line
    __syncthreads();                                    // everybody is done reading s_g
    s_g[bl * (kGR + 1) + r] = res;
    __syncthreads();
    {
      const int ob = tid >> 4, orow = tid & 15;         // kGT = 32 utterances x 16 rows
      if (row0 + orow < a.rows && b0 + ob < a.batch) a.out[(size_t)(b0 + ob) * a.rows + row0 + orow] = s_g[ob * (kGR + 1) + orow];
    }
  }
}

int launch_gemv(const GemvArgs& a, void* stream) {
  if (a.rows <= 0) return QVC_OK;
  const size_t lds = ((size_t)gemv_g_floats(a.gin) + (size_t)kGR * a.gin) * 4;
  if (a.gin % 4 || a.gin > 512 || lds > 160 * 1024) return QVC_ERR_BAD_CONFIG;
  return launch_big_lds<cond_gemv_kernel>(dim3((unsigned)ceil_div(a.rows, kGR)), dim3(kGT), lds, static_cast<hipStream_t>(stream), a);
}

// ------------------------------------------------------------------ sampling
// z[b][t][c] = mu + noise[b][c][t] * exp(logs): the noise arrives in the reference's (B, C, T) layout, everything
// else is frame-major, so a 32 x 32 tile goes through LDS -- both the read (along t) and the write (along c) are
// coalesced (reading the noise with c fastest cost a 64-byte sector per 4 bytes).
__global__ __launch_bounds__(256) void sample_kernel(const SampleArgs a) {
  __shared__ float s_n[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32, b = blockIdx.z;
#pragma unroll
  for (int cc = ty; cc < 32; cc += 8) {
    const int c = c0 + cc, t = t0 + tx;
    s_n[cc][tx] = (c < a.C && t < a.frames) ? a.noise[((size_t)b * a.C + c) * a.frames + t] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int tt = ty; tt < 32; tt += 8) {
    const int t = t0 + tt, c = c0 + tx;
    if (t < a.frames && c < a.C) {
      const size_t bt = (size_t)b * a.frames + t;
      const float mu = a.stats[bt * 2 * a.C + c], logs = a.stats[bt * 2 * a.C + a.C + c];
      a.z[bt * a.C + c] = gauss_sample(mu, 0.f, s_n[tx][tt], logs, 0.f);   // (the projection added the biases)
    }
  }
}

// The same draw with the normals computed (SampleArgs::rng) instead of read: a thread owns the four channels of one
// noise_normal4 call at one frame, so there is no noise tile and no LDS transpose -- 8 neighbouring threads read and
// write 128 contiguous bytes of a frame.  Same tile and grid as sample_kernel.
__global__ __launch_bounds__(256) void sample_rng_kernel(const SampleArgs a) {
  const int t = blockIdx.x * 32 + (threadIdx.x >> 3), c = blockIdx.y * 32 + (threadIdx.x & 7) * 4, b = blockIdx.z;
  if (t >= a.frames || c >= a.C) return;
  const int frame0 = a.pos ? a.pos[b] - a.off : 0;
  const Normal4 n = noise_normal4(a.rng.seed_lo, a.rng.seed_hi, a.rng.keys[b], (uint32_t)frame0 + (uint32_t)t, (uint32_t)(c >> 2), a.rng.scale);
  const size_t bt = (size_t)b * a.frames + t;
  const float4 mu = *reinterpret_cast<const float4*>(a.stats + bt * 2 * a.C + c);
  const float4 ls = *reinterpret_cast<const float4*>(a.stats + bt * 2 * a.C + a.C + c);
  *reinterpret_cast<float4*>(a.z + bt * a.C + c) =
      make_float4(gauss_sample(mu.x, 0.f, n.v[0], ls.x, 0.f), gauss_sample(mu.y, 0.f, n.v[1], ls.y, 0.f),
                  gauss_sample(mu.z, 0.f, n.v[2], ls.z, 0.f), gauss_sample(mu.w, 0.f, n.v[3], ls.w, 0.f));
}

int launch_sample(const SampleArgs& a, void* stream) {
  if (a.batch <= 0 || a.frames <= 0 || a.C <= 0) return QVC_ERR_BAD_ARG;
  if (!a.noise) {
    if (!a.rng.keys || a.C % 4 || !a.stats || !a.z) return QVC_ERR_BAD_ARG;
    hipLaunchKernelGGL(sample_rng_kernel, dim3((unsigned)ceil_div(a.frames, 32), (unsigned)ceil_div(a.C, 32), (unsigned)a.batch), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)ceil_div(a.frames, 32), (unsigned)ceil_div(a.C, 32), (unsigned)a.batch), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

// ------------------------------------------------------------------ sampling, R rows from U sources (fan-out)
// sample_kernel with a row map (SampleRowsArgs): output row r draws from the statistics of source clamp(src[r]) with
// its own noise -- the same 32 x 32 LDS transpose of the noise tile, so the noise is read along t and z written
// along c.  Frames from the row's length on are written as zeros (nothing of the padding is read: neither the noise's
// nor the statistics'); the workgroup of a row's first tile also hands the row's length over (one thread).
__global__ __launch_bounds__(256) void sample_rows_kernel(const SampleRowsArgs a) {
  __shared__ float s_n[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32, r = blockIdx.z;
  const int T = a.frames_max, C = a.C;
  int s = a.src[r];
  s = s < 0 ? 0 : (s < a.sources ? s : a.sources - 1);
  const int flen = a.frames[s];
  const int len = flen < 0 ? 0 : (flen < T ? flen : T);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.row_frames[r] = flen;   // consumers clamp (ragged_len)
#pragma unroll
  for (int cc = ty; cc < 32; cc += 8) {
    const int c = c0 + cc, t = t0 + tx;
    s_n[cc][tx] = (c < C && t < len) ? a.noise[((size_t)r * C + c) * T + t] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int tt = ty; tt < 32; tt += 8) {
    const int t = t0 + tt, c = c0 + tx;
    if (t < T && c < C) {
      float z = 0.f;
      if (t < len) {
        const float* st = a.stats + ((size_t)s * T + t) * 2 * C;
        z = gauss_sample(st[c], 0.f, s_n[tx][tt], st[C + c], 0.f);
      }
      a.z[((size_t)r * T + t) * C + c] = z;
    }
  }
}

// sample_rows_kernel with the normals computed (SampleRowsArgs::rng): key rng.keys[r] of the OUTPUT row, frame t of the
// source; a thread owns four channels of one frame as in sample_rng_kernel.
__global__ __launch_bounds__(256) void sample_rows_rng_kernel(const SampleRowsArgs a) {
  const int t = blockIdx.x * 32 + (threadIdx.x >> 3), c = blockIdx.y * 32 + (threadIdx.x & 7) * 4, r = blockIdx.z;
  const int T = a.frames_max, C = a.C;
  int s = a.src[r];
  s = s < 0 ? 0 : (s < a.sources ? s : a.sources - 1);
  const int flen = a.frames[s];
  const int len = flen < 0 ? 0 : (flen < T ? flen : T);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.row_frames[r] = flen;   // consumers clamp (ragged_len)
  if (t >= T || c >= C) return;
  float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < len) {
    const Normal4 n = noise_normal4(a.rng.seed_lo, a.rng.seed_hi, a.rng.keys[r], (uint32_t)t, (uint32_t)(c >> 2), a.rng.scale);
    const float* st = a.stats + ((size_t)s * T + t) * 2 * C;
    const float4 mu = *reinterpret_cast<const float4*>(st + c), ls = *reinterpret_cast<const float4*>(st + C + c);
    z = make_float4(gauss_sample(mu.x, 0.f, n.v[0], ls.x, 0.f), gauss_sample(mu.y, 0.f, n.v[1], ls.y, 0.f),
                    gauss_sample(mu.z, 0.f, n.v[2], ls.z, 0.f), gauss_sample(mu.w, 0.f, n.v[3], ls.w, 0.f));
  }
  *reinterpret_cast<float4*>(a.z + ((size_t)r * T + t) * C + c) = z;
}

int launch_sample_rows(const SampleRowsArgs& a, void* stream) {
  if (a.sources <= 0 || a.rows < a.sources || a.rows > 65535 || a.frames_max <= 0 || a.C <= 0) return QVC_ERR_BAD_ARG;
  if (!a.noise && a.rng.keys) {
    if (!a.stats || !a.z || !a.src || !a.frames || !a.row_frames || a.C % 4) return QVC_ERR_BAD_ARG;
    hipLaunchKernelGGL(sample_rows_rng_kernel, dim3((unsigned)ceil_div(a.frames_max, 32), (unsigned)ceil_div(a.C, 32), (unsigned)a.rows), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
  }
  if (!a.stats || !a.noise || !a.z || !a.src || !a.frames || !a.row_frames) return QVC_ERR_BAD_ARG;
  hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)ceil_div(a.frames_max, 32), (unsigned)ceil_div(a.C, 32), (unsigned)a.rows), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

// ------------------------------------------------------------------ the generator's draw as a tensor
// out[r][c][t - frame0] = the normal every draw site computes for (rng.keys[r], channel c, absolute frame t), in the
// reference's (rows, channels, frames) layout.  A thread owns the four channels of one call; consecutive threads walk
// along the frames, so each of its four stores is coalesced.
__global__ __launch_bounds__(256) void noise_fill_kernel(const NoiseRng rng, int channels, int frames, int frame0, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y, r = blockIdx.z;
  if (t >= frames) return;
  const Normal4 n = noise_normal4(rng.seed_lo, rng.seed_hi, rng.keys[r], (uint32_t)frame0 + (uint32_t)t, (uint32_t)g, rng.scale);
  float* o = out + ((size_t)r * channels + (size_t)g * 4) * frames + t;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[(size_t)i * frames] = n.v[i];
}

int launch_noise_fill(const NoiseRng& rng, int rows, int channels, int frames, int frame0, float* out, void* stream) {
  if (!rng.keys || !out || rows <= 0 || rows > 65535 || channels <= 0 || channels % 4 || channels / 4 > 65535 || frames <= 0) return QVC_ERR_BAD_ARG;
  hipLaunchKernelGGL(noise_fill_kernel, dim3((unsigned)ceil_div(frames, 256), (unsigned)(channels / 4), (unsigned)rows), dim3(256), 0,
                     static_cast<hipStream_t>(stream), rng, channels, frames, frame0, out);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

// ------------------------------------------------------------------ iSTFT + band synthesis tail
// (formulas and the per-item math: qvc_tail_impl.h)
// Four bands: one block = OT consecutive output samples = OT/4 band samples (+-7/8 halo) = OT/16 frames (+-3/4).
// One band (QVC_DEC_ISTFT, models.py:171-176): the iSTFT output is the waveform, one block = OT samples = OT/4 frames
// (+-2: the overlap-add's reach), no FIR.
template <int NB> struct SynthTile;
template <> struct SynthTile<kBands> {
  static constexpr int OT = 912;           // output samples per block: 57 + 7 = 64 frames x 4 bands = exactly one
                                           // (frame, band) item per thread in the DFT phase (1024 needed two rounds)
  static constexpr int NY = OT / 4 + 15;   // band samples needed: [a0-7, a0+OT/4+7]
  static constexpr int NFR = OT / 16 + 7;  // frames needed: [f0-3, f0+OT/16+3]
  static constexpr int HL = 3;
};
template <> struct SynthTile<1> {
  static constexpr int OT = 1008;          // 252 + 4 = 256 frames: one DFT item per thread
  static constexpr int NY = 1;             // (no band-sample buffer)
  static constexpr int NFR = OT / 4 + 4;   // frames needed: [f0-2, f0+OT/4+2)
  static constexpr int HL = 2;
};

template <int NB>
__global__ __launch_bounds__(256) void istft_synth_kernel(const TailArgs a) {
  using G = SynthTile<NB>;
  constexpr int PC = NB * 2 * kBins;       // post-conv channels per frame
  constexpr int VW = NB == 1 ? 2 : 4;      // staging vector width (a single band's 18-float frames are 8-byte aligned)
  using V = typename std::conditional<NB == 1, float2, float4>::type;
  __shared__ __attribute__((aligned(16))) float s_post[G::NFR * PC];     // 20.4 KB (one band: 18 KB)
  __shared__ float s_xw[NB][G::NFR][17];                                 // windowed frames (padded)
  __shared__ float s_y[NB][G::NY + 1];

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int o0 = blockIdx.x * G::OT;
  const int a0 = NB == 1 ? o0 : o0 >> 2;   // first band sample owned by this block
  const int f_lo = (a0 >> 2) - G::HL;      // first frame staged
  const int Lpad = 4 * (a.F - 1);          // band signal length of the (padded) buffers
  const int Fb = ragged_len(a.rg, b, a.F);  // this utterance's frames are [Flo, Fb) of the buffer (ragged batches,
  const int Flo = ragged_lo(a.rg, b);       // streaming windows): its iSTFT envelope starts / ends there
  const int L = Fb > 0 ? 4 * (Fb - 1) : 0;  // its band signal is [4*Flo, L); samples outside are zeros
  const float* pb = a.post + (size_t)b * a.F * PC;

  // ---- stage frames [f_lo, f_lo+NFR) x PC channels (contiguous in memory), vector loads, coalesced
  {   // all of a thread's loads go out before its first LDS store (one per loop trip = serialised round trips)
    constexpr int kChunks = G::NFR * (PC / VW), kPer = (kChunks + 255) / 256;
    V v[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = tid + u * 256;
      const int fr = i / (PC / VW), c4 = i - fr * (PC / VW);
      const int t = f_lo + fr;
      v[u] = V{};
      if (i < kChunks && t >= Flo && t < Fb) v[u] = *reinterpret_cast<const V*>(pb + (size_t)t * PC + c4 * VW);
    }
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int i = tid + u * 256;
      if (i < kChunks) *reinterpret_cast<V*>(&s_post[i * VW]) = v[u];
    }
  }
  __syncthreads();

  // ---- per (frame, band): polar -> 16-point inverse real DFT -> Hann window
  for (int item = tid; item < G::NFR * NB; item += 256) {
    const int fr = item / NB, k = item % NB;
    float xw[16];
    tail_dft(&s_post[fr * PC + k * 2 * kBins], xw);
#pragma unroll
    for (int m = 0; m < 16; ++m) s_xw[k][fr][m] = xw[m];
  }
  __syncthreads();

  if constexpr (NB == 1) {
    // ---- overlap-add + envelope = the waveform: thread -> 4 consecutive samples n = a0 + 4*j + r
    for (int j = tid; j < G::OT / 4; j += 256) {
      const int n = a0 + 4 * j;
      float y[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = tail_ola(n + r, Flo, Fb, L, [&](int t, int m) { return s_xw[0][t - f_lo][m]; });
      float* ob = a.out + (size_t)b * Lpad;
      if (n + 3 < Lpad) *reinterpret_cast<float4*>(ob + n) = make_float4(y[0], y[1], y[2], y[3]);
      else for (int r = 0; r < 4; ++r) if (n + r < Lpad) ob[n + r] = y[r];
      if (a.y_mb) for (int r = 0; r < 4; ++r) if (n + r < Lpad) a.y_mb[(size_t)b * Lpad + n + r] = y[r];
    }
    return;
  }

  // ---- overlap-add + envelope: band samples n = a0 - 7 + i
  for (int item = tid; item < G::NY * NB; item += 256) {
    const int k = item / G::NY, i = item - k * G::NY;
    const int n = a0 - 7 + i;
    const float y = tail_ola(n, Flo, Fb, L, [&](int t, int m) { return s_xw[k][t - f_lo][m]; });
    s_y[k][i] = y;
    if (a.y_mb && i >= 7 && i < 7 + G::OT / 4 && n < Lpad)
      a.y_mb[((size_t)b * NB + k) * Lpad + n] = y;
  }
  __syncthreads();

  // ---- polyphase synthesis FIR: thread -> 4 consecutive outputs o = o0 + 4*tid + r
  if (tid < G::OT / 4) {
    const int ia = tid + 7;                                  // s_y index of band sample a = a0 + tid
    float out[4];
    tail_fir<kTaps>([&](int k, int d) { return s_y[k][ia + d]; }, a.fir, out);
    const int o = o0 + 4 * tid;
    const int n_out = 4 * Lpad;
    if (o >= 4 * L || o < 16 * Flo) out[0] = out[1] = out[2] = out[3] = 0.f;   // outside this utterance (both bounds are multiples of 4)
    if (o + 3 < n_out) {
      *reinterpret_cast<float4*>(a.out + (size_t)b * n_out + o) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
      for (int r = 0; r < 4; ++r) if (o + r < n_out) a.out[(size_t)b * n_out + o + r] = out[r];
    }
  }
}

int launch_tail(const TailArgs& a, void* stream) {
  if (a.bands != 1 && a.bands != kBands) return QVC_ERR_BAD_ARG;
  const int n_out = a.bands * 4 * (a.F - 1);
  if (n_out <= 0) return QVC_ERR_BAD_ARG;
  if (a.bands == 1)
    hipLaunchKernelGGL(istft_synth_kernel<1>, dim3((unsigned)ceil_div(n_out, SynthTile<1>::OT), (unsigned)a.batch), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(istft_synth_kernel<kBands>, dim3((unsigned)ceil_div(n_out, SynthTile<kBands>::OT), (unsigned)a.batch), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

// ------------------------------------------------------------------ frame-major -> channel-major
__global__ __launch_bounds__(256) void fm_to_cm_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                       int batch, int frames, int channels) {
  const size_t n = (size_t)batch * frames * channels;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int t = (int)(i % frames);
    const size_t bc = i / frames;
    const int c = (int)(bc % channels);
    const size_t b = bc / channels;
    dst[i] = src[(b * frames + t) * channels + c];
  }
}

int launch_fm_to_cm(const float* src, float* dst, int batch, int frames, int channels, void* stream) {
  const size_t n = (size_t)batch * frames * channels;
  const unsigned blocks = (unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256);
  hipLaunchKernelGGL(fm_to_cm_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), src, dst, batch,
                     frames, channels);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

// ------------------------------------------------------------------ batched strided copies (qvc_stream.h)
struct CopyBatchArgs {
  CopyDesc d[kCopyBatchMax];
  uint32_t first[kCopyBatchMax + 1];   // first workgroup of descriptor i; first[n] = grid size
  uint32_t vec[kCopyBatchMax];         // bytes per element: 16 when every address / pitch / width allows it, else 4
  int32_t n;
};
constexpr int kCopyPerThread = 4;      // elements per thread: 16 KiB per workgroup at 16 bytes per element

template <typename V>
__device__ inline void copy_span(const CopyDesc& d, uint32_t wg) {
  const uint32_t wv = d.width / (uint32_t)sizeof(V);
  const uint32_t total = wv * d.rows;
  const uint32_t e0 = wg * (256u * kCopyPerThread) + threadIdx.x;
  V v[kCopyPerThread];
  uint32_t off[kCopyPerThread];
#pragma unroll
  for (int k = 0; k < kCopyPerThread; ++k) {
    const uint32_t e = e0 + (uint32_t)k * 256u;
    const uint32_t row = e / wv, col = e - row * wv;
    off[k] = e < total ? row * d.dpitch + col * (uint32_t)sizeof(V) : 0xffffffffu;
    v[k] = V{};
    if (e < total && d.src) v[k] = *reinterpret_cast<const V*>(static_cast<const char*>(d.src) + (size_t)row * d.spitch + (size_t)col * sizeof(V));
  }
#pragma unroll
  for (int k = 0; k < kCopyPerThread; ++k)
    if (off[k] != 0xffffffffu) *reinterpret_cast<V*>(static_cast<char*>(d.dst) + off[k]) = v[k];
}

__global__ __launch_bounds__(256) void copy_batch_kernel(const CopyBatchArgs a) {
  int i = 0;
  while (i + 1 < a.n && blockIdx.x >= a.first[i + 1]) ++i;    // <= 12 descriptors: a scalar scan
  if (a.vec[i] == 16) copy_span<uint4>(a.d[i], blockIdx.x - a.first[i]);
  else copy_span<uint32_t>(a.d[i], blockIdx.x - a.first[i]);
}

int launch_copy_batch(const CopyDesc* d, int n, void* stream) {
  if (n <= 0) return QVC_OK;
  if (!d || n > kCopyBatchMax) return QVC_ERR_BAD_ARG;
  CopyBatchArgs a{};
  a.n = 0;
  uint32_t wgs = 0;
  for (int i = 0; i < n; ++i) {
    const CopyDesc& c = d[i];
    if (!c.dst || (c.width | c.dpitch | c.spitch) & 3u || (reinterpret_cast<uintptr_t>(c.dst) | reinterpret_cast<uintptr_t>(c.src)) & 3u)
      return QVC_ERR_BAD_ARG;
    if (c.width == 0 || c.rows == 0) continue;
    const bool wide = !(((c.width | c.dpitch | c.spitch) & 15u) || ((reinterpret_cast<uintptr_t>(c.dst) | reinterpret_cast<uintptr_t>(c.src)) & 15u));
    const uint32_t v = wide ? 16u : 4u;
    const uint64_t total = (uint64_t)(c.width / v) * c.rows;
    // 32-bit element and destination-offset arithmetic in the kernel
    if (total >= (1ull << 31) || (uint64_t)c.rows * c.dpitch >= (1ull << 32)) return QVC_ERR_BAD_ARG;
    a.d[a.n] = c; a.vec[a.n] = v; a.first[a.n] = wgs;
    wgs += (uint32_t)((total + 256u * kCopyPerThread - 1) / (256u * kCopyPerThread));
    ++a.n;
  }
  if (a.n == 0) return QVC_OK;
  a.first[a.n] = wgs;
  hipLaunchKernelGGL(copy_batch_kernel, dim3(wgs), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

// ------------------------------------------------------------------ count-aware batched copies (qvc_stream.h: stream_tick)
// copy_batch_kernel's job with the bytes per slot taken from n_new on the device.  A workgroup serves one chunk of ONE
// slot of one descriptor, so n is uniform in it: the early return of an idle slot and the choice of the vector width
// are not divergent.  A descriptor whose addresses, pitches, fixed part and width are multiples of 16 (wide) moves 16
// bytes per lane whenever n * unit and n * shift are too -- the frame-major rings always, the (B, C, T) unit ring when
// n % 4 == 0 -- and otherwise covers the same chunk with 4-byte elements in four passes: its shift is then 4-byte aligned
// only.  Every copy goes ring -> scratch or scratch -> ring, never in place, so no pass ordering is needed.
struct CopyCountedArgs {
  CountedDesc d[kCopyBatchMax];
  uint32_t first[kCopyBatchMax + 1];   // first workgroup of descriptor i; first[n] = grid size
  uint32_t chunks[kCopyBatchMax];      // workgroups per slot
  uint32_t wide[kCopyBatchMax];        // 1: sized in 16-byte elements (see above), 0: in 4-byte elements
  int32_t n;
  CountedHead h;
};

template <typename V>
__device__ inline void counted_span(const CountedDesc& d, uint32_t slot, uint32_t chunk, uint32_t passes, uint32_t n, bool zero_only) {
  const uint32_t wv = d.width / (uint32_t)sizeof(V);
  const uint32_t total = wv * d.rows;
  const uint32_t valid = zero_only ? 0u : d.fixed + n * d.unit;                // bytes of a row that come from src
  char* dst = static_cast<char*>(d.dst) + (size_t)slot * d.rows * d.dpitch;
  const char* src = static_cast<const char*>(d.src) + (size_t)slot * d.rows * d.spitch + (size_t)n * d.shift;
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t e0 = (chunk * passes + p) * (256u * kCopyPerThread) + threadIdx.x;
    V v[kCopyPerThread];
    uint32_t off[kCopyPerThread];
#pragma unroll
    for (int k = 0; k < kCopyPerThread; ++k) {
      const uint32_t e = e0 + (uint32_t)k * 256u;
      const uint32_t row = e / wv, col = (e - row * wv) * (uint32_t)sizeof(V);
      off[k] = e < total ? row * d.dpitch + col : 0xffffffffu;
      v[k] = V{};
      if (e < total && col < valid) v[k] = *reinterpret_cast<const V*>(src + (size_t)row * d.spitch + col);
    }
#pragma unroll
    for (int k = 0; k < kCopyPerThread; ++k)
      if (off[k] != 0xffffffffu) *reinterpret_cast<V*>(dst + off[k]) = v[k];
  }
}

__global__ __launch_bounds__(256) void copy_counted_kernel(const CopyCountedArgs a) {
  if (blockIdx.x == 0) {       // the tick's bookkeeping: nothing else in this launch reads what it writes
    for (int b = (int)threadIdx.x; b < a.h.slots; b += 256) {
      const int nb = tick_count(a.h.n_new, b, a.h.hop);
      if (a.h.pos_eff) {
        a.h.pos_eff[b] = nb > 0 ? a.h.pos[b] : a.h.idle_pos;
        a.h.len_eff[b] = nb > 0 ? counted_len(a.h, b, nb) : 0;
      }
      if (a.h.pos_add && nb > 0) a.h.pos_add[b] += nb;
    }
  }
  int i = 0;
  while (i + 1 < a.n && blockIdx.x >= a.first[i + 1]) ++i;    // <= 12 descriptors: a scalar scan
  const uint32_t wg = blockIdx.x - a.first[i];
  const uint32_t slot = wg / a.chunks[i], chunk = wg - slot * a.chunks[i];
  const uint32_t n = (uint32_t)tick_count(a.h.n_new, (int)slot, a.h.hop);
  const bool idle_zero = (a.d[i].flags & kCountedIdleZero) != 0;
  if (n == 0 && !idle_zero) return;
  if (a.wide[i] && !((n * a.d[i].unit | n * a.d[i].shift) & 15u)) counted_span<uint4>(a.d[i], slot, chunk, 1, n, n == 0);
  else counted_span<uint32_t>(a.d[i], slot, chunk, a.wide[i] ? 4u : 1u, n, n == 0);
}

int launch_copy_counted(const CountedHead& h, const CountedDesc* d, int n, void* stream) {
  if (n <= 0) return QVC_OK;
  if (!d || n > kCopyBatchMax || !h.n_new || h.slots < 1 || h.hop < 1) return QVC_ERR_BAD_ARG;
  if ((h.pos_eff != nullptr) != (h.len_eff != nullptr) || (h.pos_eff && (!h.pos || !h.lens))) return QVC_ERR_BAD_ARG;
  CopyCountedArgs a{};
  a.h = h;
  a.n = 0;
  uint64_t wgs = 0;
  for (int i = 0; i < n; ++i) {
    const CountedDesc& c = d[i];
    const uint32_t sizes = c.width | c.dpitch | c.spitch | c.fixed | c.unit | c.shift;
    const uintptr_t addrs = reinterpret_cast<uintptr_t>(c.dst) | reinterpret_cast<uintptr_t>(c.src);
    if (!c.dst || (sizes & 3u) || (addrs & 3u)) return QVC_ERR_BAD_ARG;
    if (!c.src && (c.fixed | c.unit | c.shift)) return QVC_ERR_BAD_ARG;
    if ((uint64_t)c.fixed + (uint64_t)h.hop * c.unit > c.width || c.width > c.dpitch) return QVC_ERR_BAD_ARG;
    if (c.src && (uint64_t)h.hop * c.shift + c.fixed + (uint64_t)h.hop * c.unit > c.spitch) return QVC_ERR_BAD_ARG;
    if (c.width == 0 || c.rows == 0) continue;
    // a slot's rows are whole multiples of 16 bytes apart when the pitches are, so one test serves every slot
    const bool wide = !(((c.width | c.dpitch | c.spitch | c.fixed) & 15u) || (addrs & 15u));
    const uint64_t total = (uint64_t)(c.width / (wide ? 16u : 4u)) * c.rows;      // elements per slot
    // 32-bit element and in-slot offset arithmetic in the kernel (the 4-byte passes of a wide descriptor: 4 * total)
    if (total * 4 >= (1ull << 31) || (uint64_t)c.rows * c.dpitch >= (1ull << 32) || (uint64_t)c.rows * c.spitch >= (1ull << 32)) return QVC_ERR_BAD_ARG;
    a.d[a.n] = c; a.wide[a.n] = wide ? 1u : 0u; a.first[a.n] = (uint32_t)wgs;
    a.chunks[a.n] = (uint32_t)((total + 256u * kCopyPerThread - 1) / (256u * kCopyPerThread));
    wgs += (uint64_t)a.chunks[a.n] * (uint32_t)h.slots;
    if (wgs >= (1ull << 31)) return QVC_ERR_BAD_ARG;
    ++a.n;
  }
  if (a.n == 0) return h.pos_eff || h.pos_add ? QVC_ERR_BAD_ARG : QVC_OK;     // bookkeeping rides on a copy: none to ride on
  a.first[a.n] = (uint32_t)wgs;
  hipLaunchKernelGGL(copy_counted_kernel, dim3((unsigned)wgs), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

// ------------------------------------------------------------------ windows over packed utterances (qvc_stream.h: infer_windows)
// Pure byte movers around the path, driven by the table in device memory: a workgroup serves one 1024-element chunk of
// ONE row (blockIdx.y), so the row's clamped table entry (window_row) is uniform in it and an idle row's early return is
// not divergent.  V = float4 where the channel count / samples per frame and the caller's pointers allow it, else float.
// Every address is formed from the clamped entry: reads stay in [base, base + length) <= total frames of the packed
// buffers, the delivery in [base + start, base + start + count), everything else in the workspace's own rows.
constexpr int kWinPerThread = 4;
constexpr unsigned kWinChunk = 256u * kWinPerThread;

template <typename V>
__global__ __launch_bounds__(256) void window_gather_kernel(const WindowArgs a, unsigned unit_chunks) {
  constexpr int VE = (int)(sizeof(V) / 4);
  const int r = blockIdx.y;
  const WindowRow w = window_row(a.win, r, a.n, a.total);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.pos_eff[r] = w.count > 0 ? w.start + a.C : a.W;
    a.len_eff[r] = w.count > 0 ? w.length : 0;
  }
  if (w.count == 0) return;
  const int f0 = w.start - a.C;                          // the frame of window row 0
  if (blockIdx.x < unit_chunks) {
    // ---- units: [total][Cu] -> [W][Cu], whole frames, coalesced along the channels on both sides
    const unsigned cv = (unsigned)a.unit_channels / VE;
    const size_t total = (size_t)a.W * cv;
    const float* src = a.unit_packed + (size_t)w.base * a.unit_channels;
    float* dst = a.unit_win + (size_t)r * a.W * a.unit_channels;
    V v[kWinPerThread];
    size_t at[kWinPerThread];
#pragma unroll
    for (int k = 0; k < kWinPerThread; ++k) {
      const size_t e = (size_t)blockIdx.x * kWinChunk + (unsigned)k * 256u + threadIdx.x;
      const size_t row = e / cv;
      const unsigned c = (unsigned)(e - row * cv) * VE;
      const int f = f0 + (int)row;
      at[k] = e < total ? row * a.unit_channels + c : ~(size_t)0;
      v[k] = V{};
      if (e < total && f >= 0 && f < w.length) v[k] = *reinterpret_cast<const V*>(src + (size_t)f * a.unit_channels + c);
    }
#pragma unroll
    for (int k = 0; k < kWinPerThread; ++k)
      if (at[k] != ~(size_t)0) *reinterpret_cast<V*>(dst + at[k]) = v[k];
    return;
  }
  // ---- noise (pointer form): (inter, total) -> (inter, W), coalesced along the frames on both sides
  const size_t total = (size_t)a.inter * a.W;
  float* dst = a.noise_win + (size_t)r * total;
  float v[kWinPerThread];
  size_t at[kWinPerThread];
#pragma unroll
  for (int k = 0; k < kWinPerThread; ++k) {
    const size_t e = (size_t)(blockIdx.x - unit_chunks) * kWinChunk + (unsigned)k * 256u + threadIdx.x;
    const size_t c = e / (unsigned)a.W;
    const int f = f0 + (int)(e - c * (unsigned)a.W);
    at[k] = e < total ? e : ~(size_t)0;
    v[k] = 0.f;
    if (e < total && f >= 0 && f < w.length) v[k] = a.noise_packed[c * (size_t)a.total + (size_t)w.base + (size_t)f];
  }
#pragma unroll
  for (int k = 0; k < kWinPerThread; ++k)
    if (at[k] != ~(size_t)0) dst[at[k]] = v[k];
}

template <typename V>
__global__ __launch_bounds__(256) void window_deliver_kernel(const WindowArgs a) {
  constexpr int VE = (int)(sizeof(V) / 4);
  const int r = blockIdx.y;
  const WindowRow w = window_row(a.win, r, a.n, a.total);
  const size_t total = (size_t)w.count * ((unsigned)a.spf / VE);      // elements of the row's delivered frames: one run
  if ((size_t)blockIdx.x * kWinChunk >= total) return;
  const float* src = a.wave + ((size_t)r * a.wave_rows + a.first) * a.spf;
  float* dst = a.out_packed + ((size_t)w.base + (size_t)w.start) * a.spf;
  V v[kWinPerThread];
#pragma unroll
  for (int k = 0; k < kWinPerThread; ++k) {
    const size_t e = (size_t)blockIdx.x * kWinChunk + (unsigned)k * 256u + threadIdx.x;
    v[k] = V{};
    if (e < total) v[k] = *reinterpret_cast<const V*>(src + e * VE);
  }
#pragma unroll
  for (int k = 0; k < kWinPerThread; ++k) {
    const size_t e = (size_t)blockIdx.x * kWinChunk + (unsigned)k * 256u + threadIdx.x;
    if (e < total) *reinterpret_cast<V*>(dst + e * VE) = v[k];
  }
}

// what both launches check of the geometry: the grid's y is the row, first + n rows of the waveform exist
static bool window_args_ok(const WindowArgs& a) {
  return a.win && a.rows >= 1 && a.rows <= 65535 && a.n >= 1 && a.C >= 0 && a.W == 2 * a.C + a.n && a.total >= 1 && a.total <= kWindowMaxTotal;
}

int launch_window_gather(const WindowArgs& a, void* stream) {
  if (!window_args_ok(a) || !a.unit_packed || !a.unit_win || a.unit_channels < 1 || !a.pos_eff || !a.len_eff) return QVC_ERR_BAD_ARG;
  if (a.noise_packed && (!a.noise_win || a.inter < 1)) return QVC_ERR_BAD_ARG;
  const bool wide = a.unit_channels % 4 == 0 && !((reinterpret_cast<uintptr_t>(a.unit_packed) | reinterpret_cast<uintptr_t>(a.unit_win)) & 15u);
  const uint64_t unit_chunks = ((uint64_t)a.W * (a.unit_channels / (wide ? 4 : 1)) + kWinChunk - 1) / kWinChunk;
  const uint64_t noise_chunks = a.noise_packed ? ((uint64_t)a.W * a.inter + kWinChunk - 1) / kWinChunk : 0;
  if (unit_chunks + noise_chunks >= (1ull << 31)) return QVC_ERR_BAD_ARG;
  const dim3 grid((unsigned)(unit_chunks + noise_chunks), (unsigned)a.rows);
  if (wide) hipLaunchKernelGGL(window_gather_kernel<float4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a, (unsigned)unit_chunks);
  else hipLaunchKernelGGL(window_gather_kernel<float>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a, (unsigned)unit_chunks);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

int launch_window_deliver(const WindowArgs& a, void* stream) {
  if (!window_args_ok(a) || !a.wave || !a.out_packed || a.spf < 1 || a.first < 0 || a.wave_rows < a.first + a.n) return QVC_ERR_BAD_ARG;
  const bool wide = a.spf % 4 == 0 && !((reinterpret_cast<uintptr_t>(a.wave) | reinterpret_cast<uintptr_t>(a.out_packed)) & 15u);
  const uint64_t chunks = ((uint64_t)a.n * (a.spf / (wide ? 4 : 1)) + kWinChunk - 1) / kWinChunk;
  if (chunks >= (1ull << 31)) return QVC_ERR_BAD_ARG;
  const dim3 grid((unsigned)chunks, (unsigned)a.rows);
  if (wide) hipLaunchKernelGGL(window_deliver_kernel<float4>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(window_deliver_kernel<float>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

// ------------------------------------------------------------------ the launchers of the six chosen families
// choose_* (qvc_select.h) decides, dispatch_* (the translation unit that holds the kernels) launches; here the choice's
// operand / stream type picks the instantiation entry.
int launch_conv(const ConvDesc& d, ConvArgs a, int batch, int epi, int dtype, void* stream, LaunchChoice& c) {
  conv_geometry(a, d);
  c = choose_conv(d, a, batch, epi, dtype);
  if (c.status != QVC_OK) return c.status;
  return c.op == QVC_F16 ? dispatch_conv<_Float16>(c, a, stream) : dispatch_conv<__bf16>(c, a, stream);
}

int launch_post_tail(const ConvDesc& d, PostTailArgs a, int batch, int dtype, void* stream, LaunchChoice& c) {
  conv_geometry(a.c, d);
  c = choose_post_tail(d, a, batch, dtype);
  if (c.status != QVC_OK) return c.status;
  return c.op == QVC_F16 ? dispatch_post_tail<_Float16>(c, a, stream) : dispatch_post_tail<__bf16>(c, a, stream);
}

bool wn_stack_supported(const ConvDesc& din, int layers) { return wn_stack_ok(din, layers); }

int launch_wn_stack(const ConvDesc& din, const WnStackArgs& a, int batch, int dtype, void* stream, LaunchChoice& c) {
  c = choose_wn_stack(din, a, batch, dtype);
  if (c.status != QVC_OK) return c.status;
  if (c.family == LF_WN_STACK2) return c.op == QVC_F16 ? dispatch_wn_stack2<_Float16>(c, a, stream) : dispatch_wn_stack2<__bf16>(c, a, stream);
  return c.op == QVC_F16 ? dispatch_wn_stack<_Float16>(c, a, stream) : dispatch_wn_stack<__bf16>(c, a, stream);
}

int launch_wn(const ConvDesc& din, const WnArgs& a, int batch, int dtype, void* stream, LaunchChoice& c) {
  c = choose_wn(din, a, batch, dtype);
  if (c.status != QVC_OK) return c.status;
  return c.op == QVC_F16 ? dispatch_wn<_Float16>(c, a, stream) : dispatch_wn<__bf16>(c, a, stream);
}

int launch_pair3(const ConvDesc* d1, const ConvDesc* d2, const PairArgs3& a, int batch, int dtype, void* stream, LaunchChoice& c) {
  c = choose_pair(d1, d2, a, batch, dtype);
  if (c.status != QVC_OK) return c.status;
  if (c.op == QVC_F16) return dispatch_pair<_Float16, _Float16>(c, a, stream);
  return c.ts == QVC_BF16 ? dispatch_pair<__bf16, __bf16>(c, a, stream) : dispatch_pair<__bf16, _Float16>(c, a, stream);   // QVC_BF16X: f16 stream
}

int launch_chain(const ConvDesc* d1, const ConvDesc* d2, ChainArgs a, int batch, int dtype, void* stream, LaunchChoice& c) {
  c = choose_chain(d1, d2, a, batch, dtype);
  if (c.status != QVC_OK) return c.status;
  a.halo = c.halo; a.margin = c.margin; a.NT = c.NT;
  if (c.op == QVC_F16) return dispatch_chain<_Float16, _Float16>(c, a, stream);
  return c.ts == QVC_BF16 ? dispatch_chain<__bf16, __bf16>(c, a, stream) : dispatch_chain<__bf16, _Float16>(c, a, stream);
}

// the forms of qvc_kernels.h: the choice is not handed back
int launch_conv(const ConvDesc& d, ConvArgs a, int batch, int epi, int dtype, void* stream) { LaunchChoice c; return launch_conv(d, a, batch, epi, dtype, stream, c); }
int launch_post_tail(const ConvDesc& d, PostTailArgs a, int batch, int dtype, void* stream) { LaunchChoice c; return launch_post_tail(d, a, batch, dtype, stream, c); }
int launch_wn_stack(const ConvDesc& din, const WnStackArgs& a, int batch, int dtype, void* stream) { LaunchChoice c; return launch_wn_stack(din, a, batch, dtype, stream, c); }
int launch_wn(const ConvDesc& din, WnArgs a, int batch, int dtype, void* stream) { LaunchChoice c; return launch_wn(din, a, batch, dtype, stream, c); }
int launch_pair3(const ConvDesc* d1, const ConvDesc* d2, const PairArgs3& a, int batch, int dtype, void* stream) { LaunchChoice c; return launch_pair3(d1, d2, a, batch, dtype, stream, c); }
int launch_chain(const ConvDesc* d1, const ConvDesc* d2, const ChainArgs& a, int batch, int dtype, void* stream) { LaunchChoice c; return launch_chain(d1, d2, a, batch, dtype, stream, c); }

}  // namespace qvc
