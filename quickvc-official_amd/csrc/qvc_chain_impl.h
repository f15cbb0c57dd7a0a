// qvc_chain_impl.h -- a whole ResBlock1 (modules.py:147-154: three pairs x = x + conv2(lrelu(conv1(lrelu(x)))) with
// dilations d0, d1, d2) in ONE launch, for the chains whose receptive field is short (kernel 3: 12 frames per side).
//
// Why: the fused pair kernel (rbpair_kernel) reads a chain's stream twice (tile + residual) and writes it once per
// pair, and its memory phases do not overlap its GEMMs (204 us of GEMMs + 68 us of memory phases per
// three-chain launch, additive).  For the k = 3 chain those phases are as long as for k = 11 while its GEMMs are a
// quarter of the work -- so its three pairs are chained on chip: the stream is read ONCE (tile + 2 x 12 halo frames),
// stays in LDS as a raw f16 tile (the residual) next to the activated operand tile, and is written ONCE.
// Price: 2 x halo frames recomputed per tile (144-frame tile, 120 produced: +20 % of the chain's MFMA work, the
// cheapest chain) and one more barrier per pair.
//
// Same math per element as three rbpair launches: same K order, the stream rounded to its memory type after every
// pair, the intermediates zeroed outside the utterance -- results are bit-identical (GPU test).
#pragma once
#include "qvc_conv_impl.h"

namespace qvc {

template <typename T, int MF, int NF, int NWV, typename TS>
__global__ __launch_bounds__(NWV * 64) void rbchain_kernel(const ChainArgs A) {
  using O = Op<T>;
  using frag = typename O::frag;
  using OS = Op<TS>;
  using sfrag = typename OS::frag;
  static_assert(MF % 2 == 0, "lane-packed rows in 16-byte pieces");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NTHR = NWV * 64;
  constexpr int ROWS = NF * 16;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wm = __builtin_amdgcn_readfirstlane(tid >> 6);      // all waves split the rows (WN = 1)
  const int lrow = lane & 15, lq = lane >> 4;
  const int b = blockIdx.y;
  const PairArgs a0 = A.p[0];                 // a copy: a reference into the by-value arguments would send them to scratch
  const int C = a0.C, CP = a0.CP;
  const int rowbytes = CP * 2, cpr = CP >> 3;
  const Swz sm = swz_mode(cpr);
  const int q0 = blockIdx.x * A.NT;
  const int F0 = q0 - A.halo;                  // frame of tile row 0
  const int Tb = ragged_len(A.rg, b, a0.T), Tlo = ragged_lo(A.rg, b);
  if (q0 >= Tb) return;
  char* act = smem;                            // activated operand tile: row mrg + r <-> frame F0 + r
  char* raw = smem + (size_t)(ROWS + 2 * A.margin) * rowbytes;   // the stream itself (residual), row r <-> frame F0 + r
  const int mrg = A.margin;
  const int cb = wm * MF * 16 + lq * 4 * MF;   // first of this lane's 4 * MF consecutive channels

  {   // ---- stage: raw x and lrelu(x) (operand type); margins of the operand tile = zeros
    const TS* xb = static_cast<const TS*>(a0.x) + (size_t)b * a0.bs;
    for (int i = tid; i < 2 * mrg * cpr; i += NTHR) {
      const int r = i / cpr, c8 = i - r * cpr;
      const int row = r < mrg ? r : ROWS + r;
      *reinterpret_cast<uint4*>(tile_at(act, row, c8, rowbytes, sm)) = make_uint4(0u, 0u, 0u, 0u);
    }
    stage_stream_tile<T, TS, NTHR>(xb, C, cpr, ROWS * cpr, F0, Tlo, Tb, a0.slope, tid,
        [&](int r, int c8, const uint4& x, frag o) {
          *reinterpret_cast<uint4*>(tile_at(raw, r, c8, rowbytes, sm)) = x;
          *reinterpret_cast<frag*>(tile_at(act, mrg + r, c8, rowbytes, sm)) = o;
        },
        [](bool) {});
  }
  __syncthreads();

  for (int q = 0; q < A.n; ++q) {
    PairArgs a = A.p[0];                       // scalar selects (a dynamic index into the kernel arguments would go through scratch)
    if (q == 1) a = A.p[1];
    if (q == 2) a = A.p[2];
    const int h2 = (a.k - 1) / 2, h1 = h2 * a.dil;
    const bool last = q == A.n - 1;
    f32x4 acc[MF][NF];
    {   // ---- GEMM1 (dilation d_q) over the whole tile, bias + lrelu -> the operand tile, in place
      QVC_ZERO_ACC(acc);
      const frag* ap = static_cast<const frag*>(a.w1) + ((size_t)wm * a.nIt * MF) * 64 + lane;
      gemm_loop<T, MF, NF, QVC_PF_CONV>(acc, ap, a.nIt, a.KS, a.dil, act, rowbytes, sm, mrg - h1 + lrow, lq);
      float4 bias[MF];
#pragma unroll
      for (int m = 0; m < MF; ++m) bias[m] = *reinterpret_cast<const float4*>(a.b1 + cb + m * 4);
      __syncthreads();                         // every wave is done reading the operand tile
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        const int r = n * 16 + lrow;
        const int f = F0 + r;
        const bool inside = f >= Tlo && f < Tb;                  // conv2 zero-pads outside the utterance
#pragma unroll
        for (int m = 0; m < MF; m += 2) {
          const int v = cb + m * 4;
          if (v >= CP) continue;
          frag h;
          if (inside && v < C) {
            h = pack8_lrelu<T>(acc[m][n], bias[m], acc[m + 1][n], bias[m + 1], a.slope);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (T)0.f;
          }
          *reinterpret_cast<frag*>(tile_at(act, mrg + r, v >> 3, rowbytes, sm)) = h;
        }
      }
    }
    __syncthreads();
    {   // ---- GEMM2 (dilation 1) + bias + residual (raw tile) -> the stream: back into both tiles, or out to memory
      QVC_ZERO_ACC(acc);
      const frag* ap = static_cast<const frag*>(a.w2) + ((size_t)wm * a.nIt * MF) * 64 + lane;
      gemm_loop<T, MF, NF, QVC_PF_CONV>(acc, ap, a.nIt, a.KS, 1, act, rowbytes, sm, mrg - h2 + lrow, lq);
      float4 bias[MF];
#pragma unroll
      for (int m = 0; m < MF; ++m) bias[m] = *reinterpret_cast<const float4*>(a.b2 + cb + m * 4);
      if (!last) __syncthreads();              // every wave is done reading the intermediate: the next pair's input may overwrite it
      TS* yb = static_cast<TS*>(A.n == 3 ? A.p[2].y : A.p[1].y) + (size_t)b * a.bs;   // the chain's output (scalar select)
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        const int r = n * 16 + lrow;
        const int f = F0 + r;
        const bool inside = f >= Tlo && f < Tb;
#pragma unroll
        for (int m = 0; m < MF; m += 2) {
          const int v = cb + m * 4;
          if (v >= C) continue;
          char* rp = tile_at(raw, r, v >> 3, rowbytes, sm);
          sfrag h = pack8_res<TS>(acc[m][n], bias[m], acc[m + 1][n], bias[m + 1], *reinterpret_cast<const sfrag*>(rp));
          if (last) {
            if (r >= A.halo && r < A.halo + A.NT && f < Tb) *reinterpret_cast<sfrag*>(yb + (size_t)f * C + v) = h;
          } else {
            if (!inside) {
#pragma unroll
              for (int e = 0; e < 8; ++e) h[e] = (TS)0.f;        // the next pair's convs zero-pad outside the utterance
            }
            *reinterpret_cast<sfrag*>(rp) = h;
            *reinterpret_cast<frag*>(tile_at(act, mrg + r, v >> 3, rowbytes, sm)) = act8<T, TS>(h, a.slope);
          }
        }
      }
    }
    if (!last) __syncthreads();
  }
}

// a.halo / margin / NT: the choice's (launch_chain copies them in)
template <typename T, typename TS>
int dispatch_chain(const LaunchChoice& c, const ChainArgs& a, void* stream) {
  return lift<2, 4>(c.MF, [&](auto MF) {
    return lift<4, 8>(c.waves, [&](auto NWV) {
      return lift<9, 8, 6, 5, 4>(c.NF, [&](auto NF) -> int {
        if constexpr (chain_built(QVC_V(MF), QVC_V(NF), QVC_V(NWV)))
          return launch_chosen<rbchain_kernel<T, QVC_V(MF), QVC_V(NF), QVC_V(NWV), TS>>(c, a, stream);
        else return QVC_ERR_BAD_CONFIG;
      });
    });
  });
}

}  // namespace qvc
