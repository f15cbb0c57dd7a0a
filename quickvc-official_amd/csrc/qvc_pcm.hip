// qvc_pcm.hip -- sample formats either side of the float path (include/qvc.h): raw wav payloads -> the padded fp32 batch
// the trim / mel kernels take (qvc_pcm_to_wave_ragged), fp32 waveforms -> 16-bit PCM (qvc_wave_to_pcm16).
//
// Both are streaming kernels: every byte is read once and written once, so the only thing to get right is the access
// width.  A lane of the decode handles GROUP = 8 consecutive frames of one row: 8 .. 64 payload bytes, fetched with
// 16-byte loads where the format's group size is a multiple of 16 (12-byte loads for mono s24, one 8-byte load for mono
// u8), and two 16-byte stores.  The format is a property of the ROW (blockIdx.y), so the switch over it is uniform per
// workgroup.  The one group of a row that straddles its end is decoded sample by sample from single bytes; groups past
// the end store zeros.  The grid is sized by max_samples: the host never learns a row's length.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/qvc.h"

namespace qvc {

enum { PCM_U8 = 1, PCM_S16 = 2, PCM_S24 = 3, PCM_S32 = 4, PCM_F32 = 5 };   // qvc_pcm_row.code (QVC_PCM_* of qvc_io.h)
constexpr int PCM_GROUP = 8;

__host__ __device__ constexpr int pcm_sample_bytes(int code) {
  return code == PCM_U8 ? 1 : code == PCM_S16 ? 2 : code == PCM_S24 ? 3 : (code == PCM_S32 || code == PCM_F32) ? 4 : 0;
}

// one sample from its little-endian bits (the low pcm_sample_bytes(CODE) bytes of raw): frontend.load_wav's arithmetic
template <int CODE>
__device__ __forceinline__ float pcm_value(uint32_t raw) {
  if constexpr (CODE == PCM_U8) return ((float)(int)(raw & 0xFFu) - 128.f) * (1.f / 128.f);
  else if constexpr (CODE == PCM_S16) return (float)(int)(int16_t)(raw & 0xFFFFu) * (1.f / 32768.f);
  else if constexpr (CODE == PCM_S24) return (float)((int32_t)(raw << 8) >> 8) * (1.f / 8388608.f);
  else if constexpr (CODE == PCM_S32) return (float)(int32_t)raw * (1.f / 2147483648.f);     // int -> float: nearest even
  else return __uint_as_float(raw);
}

struct alignas(4) PcmWord3 { uint32_t a, b, c; };

// the sample at byte `o` of a group held in dwords w[0 .. NW)
template <int CODE, int NW>
__device__ __forceinline__ float pcm_at(const uint32_t (&w)[NW], int o) {
  constexpr int B = pcm_sample_bytes(CODE);
  const int d = o >> 2, sh = (o & 3) * 8;
  uint32_t raw = w[d] >> sh;
  if (sh + 8 * B > 32) raw |= w[d + 1 < NW ? d + 1 : d] << (32 - sh);     // an s24 sample across two dwords (never the last one)
  return pcm_value<CODE>(raw);
}

// GROUP whole frames at `src` (aligned as the format's group size allows: see the file comment) -> out[GROUP]
template <int CODE, int CH>
__device__ __forceinline__ void pcm_group(const uint8_t* __restrict__ src, float (&out)[PCM_GROUP]) {
  constexpr int B = pcm_sample_bytes(CODE), NW = PCM_GROUP * B * CH / 4;
  uint32_t w[NW];
  if constexpr (NW % 4 == 0) {
#pragma unroll
    for (int i = 0; i < NW / 4; ++i) {
      const uint4 v = reinterpret_cast<const uint4*>(src)[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
  } else if constexpr (NW % 3 == 0) {
#pragma unroll
    for (int i = 0; i < NW / 3; ++i) {
      const PcmWord3 v = reinterpret_cast<const PcmWord3*>(src)[i];
      w[3 * i] = v.a; w[3 * i + 1] = v.b; w[3 * i + 2] = v.c;
    }
  } else {
    static_assert(NW == 2, "mono u8: one 8-byte load");
    const uint2 v = *reinterpret_cast<const uint2*>(src);
    w[0] = v.x; w[1] = v.y;
  }
#pragma unroll
  for (int j = 0; j < PCM_GROUP; ++j) {
    const float a = pcm_at<CODE, NW>(w, j * CH * B);
    if constexpr (CH == 2) out[j] = (a + pcm_at<CODE, NW>(w, (j * CH + 1) * B)) * 0.5f;
    else out[j] = a;
  }
}

// frame `f` of a row, byte by byte (the group that straddles the row's end)
template <int CODE>
__device__ __forceinline__ float pcm_frame(const uint8_t* __restrict__ row, int64_t f, int ch) {
  constexpr int B = pcm_sample_bytes(CODE);
  const uint8_t* p = row + f * (B * ch);
  float acc = 0.f;
  for (int c = 0; c < ch; ++c) {
    uint32_t raw = 0;
#pragma unroll
    for (int b = 0; b < B; ++b) raw |= (uint32_t)p[c * B + b] << (8 * b);
    acc = c == 0 ? pcm_value<CODE>(raw) : (acc + pcm_value<CODE>(raw)) * 0.5f;
  }
  return acc;
}

struct PcmArgs {
  const uint8_t* pcm; const qvc_pcm_row* rows; float* wave; int32_t* samples_dev;
  int64_t slot_bytes; int32_t max_samples, vec_store;
};

template <int CODE>
__device__ __forceinline__ void pcm_decode(const uint8_t* __restrict__ row, int ch, int n, int s0, float (&out)[PCM_GROUP]) {
  if (s0 + PCM_GROUP <= n) {
    const uint8_t* src = row + (int64_t)s0 * (pcm_sample_bytes(CODE) * ch);
    if (ch == 2) pcm_group<CODE, 2>(src, out); else pcm_group<CODE, 1>(src, out);
  } else {
#pragma unroll
    for (int j = 0; j < PCM_GROUP; ++j) out[j] = s0 + j < n ? pcm_frame<CODE>(row, s0 + j, ch) : 0.f;
  }
}

__global__ __launch_bounds__(256) void pcm_to_wave_kernel(const PcmArgs a) {
  const int u = blockIdx.y;
  const int64_t s0l = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PCM_GROUP;
  const qvc_pcm_row r = a.rows[u];
  const int B = pcm_sample_bytes(r.code);
  int n = 0;
  if (B > 0 && (r.channels == 1 || r.channels == 2)) {
    const int64_t cap = a.slot_bytes / (B * r.channels);
    n = (int)min((int64_t)max(r.frames, 0), min((int64_t)a.max_samples, cap));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.samples_dev[u] = n;
  if (s0l >= a.max_samples) return;
  const int s0 = (int)s0l;
  float out[PCM_GROUP];
#pragma unroll
  for (int j = 0; j < PCM_GROUP; ++j) out[j] = 0.f;
  if (s0 < n) {                                                  // every byte read lies below n * frame bytes <= slot_bytes
    const uint8_t* row = a.pcm + (int64_t)u * a.slot_bytes;
    switch (r.code) {
      case PCM_U8: pcm_decode<PCM_U8>(row, r.channels, n, s0, out); break;
      case PCM_S16: pcm_decode<PCM_S16>(row, r.channels, n, s0, out); break;
      case PCM_S24: pcm_decode<PCM_S24>(row, r.channels, n, s0, out); break;
      case PCM_S32: pcm_decode<PCM_S32>(row, r.channels, n, s0, out); break;
      default: pcm_decode<PCM_F32>(row, r.channels, n, s0, out); break;
    }
  }
  float* dst = a.wave + (int64_t)u * a.max_samples + s0;
  if (a.vec_store && s0 + PCM_GROUP <= a.max_samples) {          // rows start 16-byte aligned: max_samples % 4 == 0
    reinterpret_cast<float4*>(dst)[0] = make_float4(out[0], out[1], out[2], out[3]);
    reinterpret_cast<float4*>(dst)[1] = make_float4(out[4], out[5], out[6], out[7]);
  } else {
#pragma unroll
    for (int j = 0; j < PCM_GROUP; ++j)
      if (s0 + j < a.max_samples) dst[j] = out[j];
  }
}

__device__ __forceinline__ int pcm16_of(float x) {
  if (x != x) return 0;
  return (int)fminf(fmaxf(rintf(x * 32768.f), -32768.f), 32767.f);
}

// 8 floats -> 8 int16 per lane and step (two 16-byte loads, one 16-byte store) when both pointers are 16-byte aligned;
// the last n % 8 values, and everything when they are not, one by one
__global__ __launch_bounds__(256) void wave_to_pcm16_kernel(const float* __restrict__ wave, int16_t* __restrict__ pcm, int64_t n, int vec) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const int64_t groups = vec ? n / 8 : 0;
  for (int64_t g = tid; g < groups; g += nth) {
    const float4 x = reinterpret_cast<const float4*>(wave)[2 * g], y = reinterpret_cast<const float4*>(wave)[2 * g + 1];
    uint4 q;
    q.x = (uint32_t)(pcm16_of(x.x) & 0xFFFF) | ((uint32_t)pcm16_of(x.y) << 16);
    q.y = (uint32_t)(pcm16_of(x.z) & 0xFFFF) | ((uint32_t)pcm16_of(x.w) << 16);
    q.z = (uint32_t)(pcm16_of(y.x) & 0xFFFF) | ((uint32_t)pcm16_of(y.y) << 16);
    q.w = (uint32_t)(pcm16_of(y.z) & 0xFFFF) | ((uint32_t)pcm16_of(y.w) << 16);
    reinterpret_cast<uint4*>(pcm)[g] = q;
  }
  for (int64_t i = groups * 8 + tid; i < n; i += nth) pcm[i] = (int16_t)pcm16_of(wave[i]);
}

}  // namespace qvc

using namespace qvc;

extern "C" int qvc_pcm_to_wave_ragged(const void* pcm, int64_t slot_bytes, const qvc_pcm_row* rows_dev, float* wave,
                                      int32_t* samples_dev, int32_t utterances, int32_t max_samples, void* stream) {
  if (!pcm || !rows_dev || !wave || !samples_dev || utterances < 1 || utterances > 65535 || max_samples < 1 || max_samples > INT32_MAX - 2 * PCM_GROUP)
    return QVC_ERR_BAD_ARG;
  if (slot_bytes < 16 || slot_bytes % 16 != 0 || reinterpret_cast<uintptr_t>(pcm) % 16 != 0) return QVC_ERR_BAD_ARG;
  PcmArgs a;
  a.pcm = static_cast<const uint8_t*>(pcm); a.rows = rows_dev; a.wave = wave; a.samples_dev = samples_dev;
  a.slot_bytes = slot_bytes; a.max_samples = max_samples;
  a.vec_store = (reinterpret_cast<uintptr_t>(wave) % 16 == 0 && max_samples % 4 == 0) ? 1 : 0;
  const int64_t groups = ((int64_t)max_samples + PCM_GROUP - 1) / PCM_GROUP;
  hipLaunchKernelGGL(pcm_to_wave_kernel, dim3((unsigned)((groups + 255) / 256), (unsigned)utterances), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

extern "C" int qvc_wave_to_pcm16(const float* wave, int16_t* pcm, int64_t n, void* stream) {
  if (!wave || !pcm || n < 1) return QVC_ERR_BAD_ARG;
  const int vec = (reinterpret_cast<uintptr_t>(wave) % 16 == 0 && reinterpret_cast<uintptr_t>(pcm) % 16 == 0) ? 1 : 0;
  const int64_t work = vec ? (n + 7) / 8 : n;
  int64_t blocks = (work + 255) / 256;
  if (blocks > (1 << 16)) blocks = 1 << 16;                     // the kernel strides over the rest
  hipLaunchKernelGGL(wave_to_pcm16_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), wave, pcm, n, vec);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}
