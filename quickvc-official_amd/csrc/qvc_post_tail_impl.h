// qvc_post_tail_impl.h -- subband_conv_post (k 7, reflect-padded, models.py:388-390) + the iSTFT / band-synthesis
// tail (models.py:394-406) in ONE launch: the 72-channel post-conv frames go from the MFMA accumulators through LDS
// straight into the inverse DFT -- they are never written to memory (the two-launch form hands 46 MB over per step).
//
// One workgroup (4 waves = 2 along the rows, 3 fragments each [72 -> 96 rows] x 2 along the frames) owns NT = 2*NF*16
// post-conv frames [f_lo, f_lo + NT) and the NT - 7 output frames in their middle (the tail's +-3/4-frame halo is
// recomputed by the neighbours: 5.8 % at NT = 128).  Phases, with a barrier between each:
//   stage   act(mean of the three ResBlock outputs) for input rows [f_lo - 3 - 1(reflect), ...) -> LDS tile (operand type)
//   GEMM    acc = conv_post                                   (same K order as conv_mfma_kernel: same bits)
//   post    acc + bias -> LDS fp32 [frame][72], OVER the dead input tile
//   DFT     per (frame, band): 18 values -> 16 windowed samples, in place
//   OLA     band samples [a0 - 7, a0 + OT/4 + 7]
//   FIR     OT output samples, 16-byte stores
// Uses conv_post's packed weights as they are (ConvDesc MF 3 / WM 2 / 1 chunk, checked by post_tail_supported).
//
// NB = 1, the single-band decoder (models.py:164-176: conv_post with 18 channels, its iSTFT output IS the waveform):
// 4 waves along the frames, each multiplying the row fragments of wave 0 of conv_post's packing [18 -> 32 rows] for
// NF*16 frames; the tile's NT - 4 output frames sit between a +-2-frame overlap-add halo (the conv's +-3 frames are
// the input tile's halo rows), and the OLA phase writes 4 waveform samples per frame, 16 bytes per lane.  No FIR.
#pragma once
#include "qvc_conv_impl.h"
#include "qvc_tail_impl.h"

namespace qvc {

// (PostTailGeom<NF, NB>, the tile geometry, and post_tail_lds: qvc_select.h -- the chooser sizes the launch from them)
template <typename T, int NF, int NB = kBands>
// (three workgroups per CU at NF 4, four at NF 2: the phases of one workgroup are serial -- memory, MFMA, VALU/LDS
//  in turn -- so it is the neighbours that fill each unit; measured 94 -> 78 us going from two to three)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NF == 2 ? 4 : 3, NF == 2 ? 4 : 3)))
void post_tail_kernel(const PostTailArgs A) {
  using O = Op<T>;
  using frag = typename O::frag;
  using G = PostTailGeom<NF, NB>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int MF = G::MF, WM = G::WM, PS = G::PS;
  constexpr int NT = G::NT, OT = G::OT, NY = G::NY;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int lrow = lane & 15, lq = lane >> 4;
  const int b = blockIdx.y;
  const int o0 = blockIdx.x * OT;
  const int a0 = NB == 1 ? o0 : o0 >> 2;        // first band sample owned by this block (one band: = output sample)
  const int f_lo = (a0 >> 2) - G::HL;           // first post-conv frame of the tile
  const int Lpad = 4 * (A.F - 1);
  const int n_out = NB * Lpad;
  const int Fb = ragged_len(A.rg, b, A.F);      // this utterance's post-conv frames are [Flo, Fb)
  const int Flo = ragged_lo(A.rg, b);
  const int L = Fb > 0 ? 4 * (Fb - 1) : 0;
  float* outb = A.out + (size_t)b * n_out;

  if (f_lo >= Fb || f_lo + NT <= Flo) {         // no frame of this utterance in the tile: its samples are zeros
    for (int j = tid; j < OT / 4; j += 256) {
      const int o = o0 + 4 * j;
      if (o + 3 < n_out) *reinterpret_cast<float4*>(outb + o) = make_float4(0.f, 0.f, 0.f, 0.f);
      else for (int r = 0; r < 4; ++r) if (o + r < n_out) outb[o + r] = 0.f;
    }
    return;
  }

  const int taps = A.c.taps;
  const int R = NT + taps - 1;
  const int rowbytes = A.c.CinP * 2;
  const int cpr = A.c.CinP >> 3;
  const Swz sm = swz_mode(cpr);
  const int t_base = f_lo - A.c.left;           // input frame (after the reflect pad) of tile row 0
  const int Tin = ragged_len(A.c.rg, b, A.c.T_in);
  const int Tlo = ragged_lo(A.c.rg, b);
  const int in_bytes = R * rowbytes, post_bytes = NT * PS * 4;
  const int tile_bytes = ((in_bytes > post_bytes ? in_bytes : post_bytes) + 15) & ~15;   // == post_tail_lds()'s first region
  float* s_post = reinterpret_cast<float*>(smem);
  float* s_y = reinterpret_cast<float*>(smem + tile_bytes);       // [band][NY + 1]

  // ------------------------------------------------------------------ stage: act(mean(x, x2, x3)) -> operand-type tile
  // A thread keeps its 16-byte column c8 and walks rows r0, r0 + rstep, ... (256 threads = rstep whole rows when
  // cpr divides 256: 128 channels -> 16 rows per pass); all loads of a batch go out before the first conversion.
  {
    constexpr int kU = 5;
    const size_t boff = (size_t)b * A.c.x_bs + A.c.x_c0;
    const T* xb = static_cast<const T*>(A.c.x) + boff;
    const T* xb2 = static_cast<const T*>(A.c.x2) + boff;
    const T* xb3 = static_cast<const T*>(A.c.x3) + boff;
    const float slope = A.c.slope_in;
    const bool regular = (256 % cpr) == 0;
    const int rstep = regular ? 256 / cpr : 0;
    const int total = R * cpr;
    for (int base = tid; base < total; base += 256 * kU) {
      uint4 v1[kU], v2[kU], v3[kU];
      int dst[kU];
      int r = base / cpr, c8 = base - r * cpr;
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int idx = base + u * 256;
        if (!regular) { r = idx / cpr; c8 = idx - r * cpr; }
        const int ti = t_base + r;
        int src;
        const bool ok = in_row(ti, Tlo, Tin, A.c.reflect, src) && idx < total && (c8 * 8 < A.c.Cin);
        v1[u] = make_uint4(0u, 0u, 0u, 0u); v2[u] = v1[u]; v3[u] = v1[u];
        if (ok) {
          const size_t o = (size_t)src * A.c.x_ts + c8 * 8;
          v1[u] = *reinterpret_cast<const uint4*>(xb + o);
          v2[u] = *reinterpret_cast<const uint4*>(xb2 + o);
          v3[u] = *reinterpret_cast<const uint4*>(xb3 + o);
        }
        dst[u] = idx < total ? tile_at(0, r, c8, rowbytes, sm) : -1;
        r += rstep;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (dst[u] < 0) continue;
        frag h1, h2, h3, h;
        __builtin_memcpy(&h1, &v1[u], 16); __builtin_memcpy(&h2, &v2[u], 16); __builtin_memcpy(&h3, &v3[u], 16);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          h[i] = O::cvt(lrelu(((float)h1[i] + (float)h2[i] + (float)h3[i]) * (1.f / 3.f), slope));
        *reinterpret_cast<frag*>(smem + dst[u]) = h;
      }
    }
  }
  __syncthreads();

  // ------------------------------------------------------------------ GEMM (A from global through the ring, B from the tile)
  f32x4 acc[MF][NF];
  QVC_ZERO_ACC(acc);
  const frag* ap = static_cast<const frag*>(A.c.w) + ((size_t)wm * A.c.nIt * MF) * 64 + lane;
  if (NB == 4 && wm == 0) {
    gemm_loop<T, MF, NF, QVC_PF_CONV>(acc, ap, A.c.nIt, A.c.KS, 1, smem, rowbytes, sm, wn * (NF * 16) + lrow, lq);
  } else {        // four bands, rows 48..95: the third fragment (80..95) is all padding -- 72 channels -- and is neither
                  // loaded nor multiplied; one band: rows 0..31 (18 channels), the packing's waves 1..3 are never read
    f32x4 (&acc2)[2][NF] = reinterpret_cast<f32x4 (&)[2][NF]>(acc);
    gemm_loop<T, 2, NF, QVC_PF_CONV, MF>(acc2, ap, A.c.nIt, A.c.KS, 1, smem, rowbytes, sm, wn * (NF * 16) + lrow, lq);
  }
  __syncthreads();                              // every wave is done with the input tile

  // ------------------------------------------------------------------ post-conv frames -> LDS fp32 [frame][PS]
#pragma unroll
  for (int m = 0; m < (NB == 1 ? 2 : MF); ++m) {
    const int v = (wm * MF + m) * 16 + lq * 4;
    if (v >= G::PC) continue;                   // (one band: rows 16..19 land in the frame's padded 20-float row)
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (A.c.bias) bias = *reinterpret_cast<const float4*>(A.c.bias + v);
#pragma unroll
    for (int n = 0; n < NF; ++n) {
      const int fr = wn * (NF * 16) + n * 16 + lrow;
      const int t = f_lo + fr;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t >= Flo && t < Fb) val = make_float4(acc[m][n][0] + bias.x, acc[m][n][1] + bias.y, acc[m][n][2] + bias.z, acc[m][n][3] + bias.w);
      *reinterpret_cast<float4*>(&s_post[fr * PS + v]) = val;
    }
  }
  __syncthreads();

  // ------------------------------------------------------------------ per (frame, band): polar -> inverse DFT -> window, in place
  for (int item = tid; item < NT * NB; item += 256) {
    const int fr = item / NB, k = item % NB;
    float* sp = &s_post[fr * PS + k * 2 * kBins];
    float xw[16];
    tail_dft(sp, xw);
#pragma unroll
    for (int m = 0; m < 16; ++m) sp[m] = xw[m];
  }
  __syncthreads();

  if constexpr (NB == 1) {
    // ---------------------------------------------------------------- overlap-add + envelope = the waveform: 4 samples per item
    for (int j = tid; j < OT / 4; j += 256) {
      const int n = a0 + 4 * j;
      float y[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = tail_ola(n + r, Flo, Fb, L, [&](int t, int m) { return s_post[(t - f_lo) * PS + m]; });
      if (n + 3 < n_out) *reinterpret_cast<float4*>(outb + n) = make_float4(y[0], y[1], y[2], y[3]);
      else for (int r = 0; r < 4; ++r) if (n + r < n_out) outb[n + r] = y[r];
    }
    return;
  }

  // ------------------------------------------------------------------ overlap-add + envelope: band samples n = a0 - 7 + i
  for (int item = tid; item < NY * kBands; item += 256) {
    const int k = item / NY, i = item - k * NY;
    const int n = a0 - 7 + i;
    s_y[k * (NY + 1) + i] = tail_ola(n, Flo, Fb, L, [&](int t, int m) { return s_post[(t - f_lo) * PS + k * 2 * kBins + m]; });
  }
  __syncthreads();

  // ------------------------------------------------------------------ synthesis FIR: 4 consecutive outputs per item
  for (int j = tid; j < OT / 4; j += 256) {
    const int ia = j + 7;
    float out[4];
    tail_fir<kTaps>([&](int k, int d) { return s_y[k * (NY + 1) + ia + d]; }, A.fir, out);
    const int o = o0 + 4 * j;
    if (o >= 4 * L || o < 16 * Flo) out[0] = out[1] = out[2] = out[3] = 0.f;
    if (o + 3 < n_out) {
      *reinterpret_cast<float4*>(outb + o) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
      for (int r = 0; r < 4; ++r) if (o + r < n_out) outb[o + r] = out[r];
    }
  }
}

template <typename T>
int dispatch_post_tail(const LaunchChoice& c, const PostTailArgs& a, void* stream) {
  return lift<2, 4>(c.NF, [&](auto NF) {
    return lift<1, kBands>(c.bands, [&](auto NB) -> int {
      if constexpr (post_tail_built(QVC_V(NF), QVC_V(NB))) return launch_chosen<post_tail_kernel<T, QVC_V(NF), QVC_V(NB)>>(c, a, stream);
      else return QVC_ERR_BAD_CONFIG;
    });
  });
}

}  // namespace qvc
