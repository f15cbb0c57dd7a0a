// qvc_kernels.h -- launch-side view of the gfx950 kernels (arguments + launcher prototypes).
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include "qvc_plan.h"

namespace qvc {

enum XKind : int32_t {
  XK_OP_FM = 0,    // operand type (f16/bf16), frame-major [B][T][C]
  XK_F32_FM = 1,   // fp32, frame-major
  XK_F32_CM = 2    // fp32, channel-major (B, C, T) -- the reference's external layout
};

// Ragged batches and streaming windows: where does utterance b start and end inside the buffer a launch works on?
// Buffer row r (at `mul` rows per unit frame) of utterance b is absolute frame  (pos[b] - off) * mul + r  of its
// sequence, which is lens[b] * mul + add frames long.  Every conv zero-pads at the two ends of ITS sequence -- not of
// the padded buffer, not of a streaming window -- so the staging code masks rows outside [lo, hi):
//     lo = max(0, (off - pos[b]) * mul)          hi = min(T, (lens[b] - pos[b] + off) * mul + add)
// Rows outside are never read unmasked, which is why nothing has to be zeroed between launches.
//   lens == nullptr: the sequence ends with the buffer (hi = T);  pos == nullptr: it starts with it (pos = off = 0).
// The arrays live wherever the launch's other pointers live (device memory; host memory in the CPU emulation).
struct Ragged {
  const int32_t* lens = nullptr;
  const int32_t* pos = nullptr;
  int32_t mul = 1, add = 0, off = 0;
};
#if defined(__HIPCC__)
#define QVC_HD __host__ __device__ __forceinline__
#else
#define QVC_HD inline
#endif
// (by value and always inlined: a reference to a member of the by-value kernel arguments would make the compiler
//  copy the whole argument struct to scratch memory -- measured: 296 B of scratch and half the occupancy)
QVC_HD int ragged_len(const Ragged r, int b, int T) {          // hi
  if (!r.lens) return T;
  int d = r.lens[b] - (r.pos ? r.pos[b] - r.off : 0);          // unit frames of the sequence left from buffer row 0
  d = d < 0 ? 0 : (d < T ? d : T);                             // clamped BEFORE scaling: "unknown length" is 2^30
  const int n = d * r.mul + r.add;
  return n < 0 ? 0 : (n < T ? n : T);
}
QVC_HD int ragged_lo(const Ragged r, int b) {                  // lo
  if (!r.pos) return 0;
  const int d = r.off - r.pos[b];
  return d <= 0 ? 0 : d * r.mul;
}

// ---- the N(0,1) draw of models.py:94 without a noise tensor: a counter-based generator evaluated where the draw is
// consumed.  The value is a pure function of (seed, utterance key, channel, absolute frame) -- not of the batch, the
// shard, the padding or the streaming window an utterance happens to sit in.  Philox4x32-10 (Salmon et al., SC'11;
// the Random123 constants) with key (seed_lo, seed_hi) and counter (frame, channel / 4, key_lo, key_hi); one call
// yields the four normals of channels 4g .. 4g+3 at that frame -- what a lane of the EPI_SAMPLE epilogue holds.
struct NoiseRng {
  const uint64_t* keys = nullptr;   // one key per row / stream slot (device memory); null = the noise comes as a tensor
  uint32_t seed_lo = 0, seed_hi = 0;
  float scale = 1.f;                // noise_scale: multiplies the normal before gauss_sample (n * 1.0f is exact)
};
struct U32x4 { uint32_t v[4]; };
struct Normal4 { float v[4]; };
QVC_HD U32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return U32x4{{c0, c1, c2, c3}};
}
// ONE definition, always inlined, for every draw site (conv epilogue, sample_rng_kernel, sample_rows_rng_kernel,
// noise_fill_kernel) and the host: 24-bit uniforms u1 in (0, 1], u2 in [0, 1), Box-Muller with the accurate logf /
// sqrtf / sincosf.  Contraction is off and no product feeds a sum, so every call site gives the same bits.
QVC_HD Normal4 noise_normal4(uint32_t seed_lo, uint32_t seed_hi, uint64_t key, uint32_t frame, uint32_t group, float scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const U32x4 x = philox4x32_10(frame, group, (uint32_t)key, (uint32_t)(key >> 32), seed_lo, seed_hi);
  constexpr float k24 = 5.9604644775390625e-08f, kTwoPi = 6.283185307179586f;   // 2^-24
  Normal4 out;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float u1 = (float)((x.v[2 * h] >> 8) + 1u) * k24;
    const float u2 = (float)(x.v[2 * h + 1] >> 8) * k24;
    const float r = sqrtf(-2.f * logf(u1));
    float s, c;
    sincosf(kTwoPi * u2, &s, &c);
    out.v[2 * h] = (r * c) * scale;
    out.v[2 * h + 1] = (r * s) * scale;
  }
  return out;
}

// Arguments of one implicit-GEMM conv launch.  All strides in elements.
struct ConvArgs {
  // ---- input
  const void* x = nullptr;
  int32_t x_kind = XK_F32_FM;
  int64_t x_bs = 0;        // batch stride
  int32_t x_ts = 0;        // frame stride (frame-major) / channel stride (channel-major)
  int32_t x_c0 = 0;        // first channel of the slice (frame-major)
  int32_t Cin = 0, CinP = 0, T_in = 0;
  float slope_in = 1.f;    // leaky-ReLU slope applied while staging (1 = identity)
  // XK_OP_FM only: with x2/x3 set the staged value is act(mean(x, x2, x3)) -- the MRF average of the three
  // ResBlock outputs (models.py:378-384) is taken on the fly by its consumer, in fp32
  const void* x2 = nullptr; const void* x3 = nullptr;
  int32_t reflect = 0;     // 1: ReflectionPad1d((1,0)) in front of a 'same' conv (models.py:345,388)
  // ---- weights (A stream) and biases
  const void* w = nullptr;
  const float* bias = nullptr;     // [MP] or null
  const float* bbias = nullptr;    // per-utterance bias (conditioning), natural channel order
  int64_t bbias_bs = 0;
  int32_t taps = 1, dil = 1, left = 0, KS = 1, nIt = 1, nchunk = 1, M = 0;
  // ---- output mapping: column q, virtual row v -> frame o = q*up_s + v/Cout - up_p, channel v%Cout
  int32_t Nq = 0, up_s = 1, up_p = 0, Cout = 0, T_out = 0;
  // ---- epilogue
  const float* res = nullptr; int64_t res_bs = 0; int32_t res_ts = 0, res_c0 = 0; float res_sign = 1.f;
  const void* res16 = nullptr;     // residual in the operand type (same strides as res; res_c0 ignored)
  float* y32 = nullptr; int64_t y32_bs = 0; int32_t y32_ts = 0, y32_c0 = 0; float y_scale = 1.f; int32_t y_accum = 0;
  void* y16 = nullptr; int64_t y16_bs = 0; int32_t y16_ts = 0; float slope_out = 1.f;
  // res/skip split (WN 1x1, modules.py:104-112): rows >= split go to y32b[.. v-split] += val
  float* y32b = nullptr; int32_t split = 0;
  int32_t gau_H = 0;       // EPI_GAU: hidden size (rows are [tanh | sigmoid]); EPI_SAMPLE / EPI_STATS: inter channels (rows [mu | log sigma])
  // EPI_SAMPLE: y32[b][q][c] = (mu + bias) + noise[b][c][q] * exp(log sigma + bias), noise in the reference's (B, C, T)
  const float* noise = nullptr; int64_t noise_bs = 0; int32_t noise_ts = 0;
  // EPI_STATS: y32[b][q][c] = mu + bias, y32[b][q][gau_H + c] = log sigma + bias (the layout EPI_STD gives natural rows)
  int32_t ksize = 0;       // polyphase (up_s > 1): kernel size of the transposed conv -- phases with fewer real taps skip their zero ones
  int32_t lp = 0;          // ConvDesc::lp (lane-packed rows): EPI_STD with only a y16 output (the polyphase up-samplers)
  Ragged rg;               // per-utterance INPUT length (in T_in units); see Ragged
  // EPI_SAMPLE with noise == nullptr and rng.keys set: the normals are computed in the epilogue (noise_normal4) for
  // key rng.keys[b], channel group ch / 4 and the row's absolute frame, (rg.pos ? rg.pos[b] - rg.off : 0) + q
  NoiseRng rng;
};
// The geometry fields of a conv launch, from its descriptor (the one place that copies them).
inline void conv_geometry(ConvArgs& a, const ConvDesc& d) {
  a.Cin = d.Cin; a.CinP = d.CinP; a.taps = d.taps; a.dil = d.dil; a.left = d.left;
  a.KS = d.KS(); a.nIt = d.nIt(); a.nchunk = d.nchunk; a.M = d.M;
  a.up_s = d.up_s; a.up_p = d.up_p; a.Cout = d.Cout; a.lp = d.lp; a.ksize = d.ksize;
}

// Arguments of one fused ResBlock1 pair (modules.py:148-153):  y = x + conv2(lrelu(conv1(lrelu(x)))).
// x / y are frame-major tensors in the operand type (the MRF mean of the three ResBlocks, models.py:378-384,
// is taken by the consumer of the y tensors while it stages its input).
struct PairArgs {
  const void* x = nullptr; int64_t bs = 0; int32_t T = 0, C = 0, CP = 0;
  const void* w1 = nullptr; const float* b1 = nullptr;
  const void* w2 = nullptr; const float* b2 = nullptr;
  int32_t k = 1, dil = 1, KS = 1, nIt = 1;
  float slope = 0.1f;
  void* y = nullptr;
};

// Up to three INDEPENDENT pairs in one launch: pair q of the three ResBlocks of a stage (kernel sizes 3 / 7 / 11).
// Workgroup x serves chain x % n, tile x / n, so the workgroups that share a CU have different durations and drift
// out of phase: one's staging / epilogue (memory) runs under another's GEMMs (MFMA).  All chains share T, C, CP.
struct PairArgs3 {
  PairArgs p[3];
  int32_t n = 1;
  Ragged rg;               // per-utterance length (in T units), shared by the chains
  // 1: chain = blockIdx.z (grid tiles x batch x n): all workgroups of the first chain are dispatched before the second
  //    chain's -- the one-workgroup-per-CU layouts, where the launch then behaves like n launches back to back without
  //    the gaps between them; 0: chain = blockIdx.x % n (chains interleaved on the CUs)
  int32_t chain_major = 0;
#ifdef QVC_STAMP
  unsigned long long* stamps = nullptr;   // developer build only (tools/conv_bench): [workgroup][64] phase stamps of wave 0
#endif
};

// A whole ResBlock1 -- n chained pairs (dilations d_0 .. d_{n-1}) -- in ONE launch (qvc_chain_impl.h), for chains whose
// receptive field is short: p[0].x is read once (tile + halo), p[n-1].y written once, the stream stays on chip in
// between.  p[q].x / p[q].y of the inner pairs are the buffers the pair-by-pair path would use (the host emulation
// replays the chain that way).  halo / margin / NT are filled by the launcher (qvc_select.h: chain_geom).
struct ChainArgs {
  PairArgs p[3];
  int32_t n = 3;
  Ragged rg;
  int32_t halo = 0, margin = 0, NT = 0;
};

// One fused WaveNet layer (modules.py:87-112): k-tap conv h->2h + conditioning + tanh*sigmoid gate, then the
// 1x1 h->2h whose first half is added to the residual stream x and second half to the skip accumulator
// (all of it to the accumulator on the last layer).  x is ping-ponged (x_in -> x_out) because neighbouring
// workgroups read each other's halo frames; oacc is updated in place.
struct WnArgs {
  const float* x_in = nullptr; float* x_out = nullptr; float* oacc = nullptr;
  int64_t bs = 0; int32_t T = 0, H = 0, HP = 0;
  const void* w_in = nullptr; const void* w_rs = nullptr; const float* b_rs = nullptr;
  const float* bbias = nullptr; int64_t bbias_bs = 0;
  int32_t taps = 1, KS = 1, nIt1 = 1, last = 0;
  Ragged rg;
};

// A whole WaveNet stack (modules.py:69-114) in one launch: every workgroup carries a 32-frame output tile
// plus (taps-1)/2 * layers halo frames per side through all layers (overlap-tiled: the halo is recomputed,
// which is free because the layer is bound by weight delivery into the CU, not by the MFMA pipe).
constexpr int kWnMaxLayers = 16;
constexpr int kWnOutFrames = 32;
struct WnStackArgs {
  const float* x0 = nullptr;   // [B][T][H] stack input (pre conv output)
  float* out = nullptr;        // [B][T][H] sum of the skip paths (the stack's output)
  int64_t bs = 0; int32_t T = 0, H = 0, HP = 0;
  const void* w_in[kWnMaxLayers] = {}; const void* w_rs[kWnMaxLayers] = {}; const float* b_rs[kWnMaxLayers] = {};
  const float* bbias = nullptr; int64_t bbias_bs = 0;     // + l*2H per layer
  int32_t layers = 0, taps = 1, KS = 1, nIt1 = 1;
  // a stack may be split over several launches (less halo to recompute per launch): x_out receives the residual
  // stream for the next launch, accum continues the skip sum already in `out`, final_layer marks the launch that
  // holds the network's last layer (whose 1x1 has no residual half)
  float* x_out = nullptr; int32_t accum = 0, final_layer = 1;
  // Optional fused 1x1 convs of a coupling layer (modules.py:212-217): with w_pre the stack input is computed in the
  // kernel, x0 = W_pre * z[:, pre_c0 : pre_c0+pre_cin] + b_pre; with w_post the kernel ends with
  // z[:, post_c0 : post_c0+post_m] -= W_post * out + b_post (in place; the two channel slices are disjoint).
  const void* w_pre = nullptr; const float* b_pre = nullptr; int32_t pre_cin = 0, pre_c0 = 0, pre_KS = 0;
  const void* w_post = nullptr; const float* b_post = nullptr; int32_t post_m = 0, post_c0 = 0, post_mf = 0;
  float* z = nullptr; int64_t z_bs = 0; int32_t z_ts = 0;
  float post_sign = -1.f;   // -1: reverse flow, x1 - m (modules.py:217); +1: forward flow, m + x1
  Ragged rg;
  int32_t wide = 0;          // the 64-frame tile of the continuous-stream kernel may be used (choose_wn_stack decides)
#ifdef QVC_STAMP
  unsigned long long* stamps = nullptr;   // developer build only (tools/conv_bench): [workgroup][16 waves][32] phase stamps
#endif
};

struct GemvArgs {
  const float* w; const float* bias; const float* g; float* out;
  int32_t rows, gin, batch;
};

struct SampleArgs {   // z = mu + noise * exp(logs)   (models.py:93-94)
  const float* stats; const float* noise; float* z;
  int32_t batch, frames, C;
  // noise == nullptr and rng.keys set: drawn in the kernel for key rng.keys[b] at absolute frame (pos ? pos[b] - off : 0) + t
  NoiseRng rng = {};
  const int32_t* pos = nullptr; int32_t off = 0;
};

#if defined(__HIPCC__)
// The draw of models.py:93-94 from the projection's raw rows and their biases.  ONE definition, always inlined, for the
// conv epilogue (EPI_SAMPLE), sample_kernel and sample_rows_kernel: the compiler contracts it the same way in all
// three, so a statistics hand-over through memory (fp32, nothing rounded) gives the bits of the fused epilogue.
__device__ __forceinline__ float gauss_sample(float mu, float bm, float n, float ls, float bl) {
  return (mu + bm) + n * expf(ls + bl);
}
#endif

// Fan-out (one source, many target speakers): R output rows drawn from the statistics of U <= R encoded sources.
//   z[r][t][c] = mu[s][t][c] + noise[r][c][t] * exp(logs[s][t][c]),  s = clamp(src[r], 0, U - 1),  t < frames[s]
// and zeros from a row's length on (every consumer masks those frames).  The same launch hands the per-row lengths
// over: row_frames[r] = frames[s], the Ragged::lens of every launch after it.  src / frames / row_frames are device
// arrays; the grid comes from the host-known caps (R, T, C) alone.
struct SampleRowsArgs {
  const float* stats;       // [U][T][2C]: mu + bias | log sigma + bias
  const float* noise;       // (R, C, T), the reference's layout
  float* z;                 // [R][T][C]
  const int32_t* src;       // [R]
  const int32_t* frames;    // [U]
  int32_t* row_frames;      // [R]
  int32_t sources, rows, frames_max, C;
  NoiseRng rng = {};        // noise == nullptr and rng.keys set: drawn in the kernel for key rng.keys[r] at the source's frame t
};

constexpr int kBands = 4, kBins = 9, kPostC = kBands * 2 * kBins, kTaps = 63;   // tail geometry: sub-bands, bins per band, post-conv channels, FIR taps
struct TailArgs {     // models.py:394-406 / pqmf.py:106-117; single band: models.py:171-176
  const float* post;  // [B][F][subbands*18]
  const float* fir;   // [subbands][63], gain folded (unused for one band)
  float* out;         // [B][subbands*hop*(F-1)]
  float* y_mb;        // optional [B][subbands][hop*(F-1)]
  int32_t batch, F;
  Ragged rg;          // per-utterance frame count min(F, lens*mul + add); samples past it are written as zeros
  int32_t bands = 4;  // 4: iSTFT per band + synthesis FIR; 1: the iSTFT output is the waveform (QVC_DEC_ISTFT)
};

// subband_conv_post + tail in one launch (qvc_post_tail_impl.h): `c` = the conv_post launch without an output
// pointer, the rest = TailArgs.  The post-conv frames stay in the CU.
struct PostTailArgs {
  ConvArgs c;
  const float* fir = nullptr;   // [subbands][63], gain folded (four bands only)
  float* out = nullptr;         // [B][16*(F-1)]; one band: [B][4*(F-1)]
  int32_t F = 0;                // post-conv frames (= c.T_in + 1)
  Ragged rg;                    // as TailArgs::rg
};
// Bands of the fused conv_post + tail kernel that walks `d` (0: none).  Four bands: conv_post's packed weights as 2
// waves x 3 row fragments [72 -> 96 rows]; one band (QVC_DEC_ISTFT): the first wave's stream of a 4-wave x 2-fragment
// packing [18 -> 128 rows], rows 0..31.  Both with a 128-frame tile.
inline int post_tail_bands(const ConvDesc& d) {
  if (d.nchunk != 1 || d.up_s != 1 || d.dil != 1 || d.gau || d.lp || (int64_t)(128 + d.taps - 1) * d.CinP * 2 > 96 * 1024) return 0;
  if (d.M == 72 && d.MF == 3 && d.WM == 2) return 4;
  if (d.M == 18 && d.MF == 2 && d.WM == 4) return 1;
  return 0;
}
inline bool post_tail_supported(const ConvDesc& d) { return post_tail_bands(d) != 0; }

// Layout decisions of the plan for `cfg` (qvc_plan_info, include/qvc.h; the emulation exports the same as a test hook):
// out[0] enc_p.proj rows paired [mu | log sigma] (sampling in the epilogue), out[1] its fragments per wave,
// out[2..3] up-samplers 0 / 1 lane-packed, out[4] conv_post + tail can run as one launch,
// out[5..6] waves per workgroup of the stage 0 / 1 ResBlock pairs, out[7] all pairs fusable
inline int plan_flags(const qvc_config* cfg, int32_t out[8]) {
  if (!cfg || !out) return QVC_ERR_BAD_ARG;
  const Plan P = build_plan(*cfg);
  if (P.status != QVC_OK) return P.status;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = P.enc_proj.gau; out[1] = P.enc_proj.MF;
  for (size_t i = 0; i < P.stages.size() && i < 2; ++i) {
    out[2 + i] = P.stages[i].up.lp;
    out[5 + i] = block_waves(P.stages[i].c1[0]);
  }
  out[4] = post_tail_supported(P.conv_post) ? 1 : 0;
  out[7] = 1;
  for (const StagePlan& st : P.stages) out[7] = out[7] && pairs_fusable(P.cfg, st);
  return QVC_OK;
}

// One LSTM layer's recurrence over all partials (models.py:510,516): gates = xp[t] + W_hh h[t-1], PyTorch gate
// order i,f,g,o.  The input projection xp (with b_ih + b_hh) comes from a conv launch.
struct LstmArgs {
  const float* xp;      // fp32, 4H per frame
  int32_t shared;       // 1: xp is [U][F][4H], partial p reads frames spk_start(p)+t; 0: xp is [P][S][4H]
  int32_t F, n_part, S, P, H;
  const void* w_hh;     // [wave][k-step][8 fragments][64 lanes][8], see spk_hh_row
  void* hseq;           // [P16][S][HP] operand type (P, H padded to 16 / 32): input of the next layer (null on the last)
  float* hfin;          // [P][H] fp32: h after the last step (last layer only)
  // Ragged batches (all null = the uniform layout above): partial p reads row prow[p] from frame pstart[p] for
  // psteps[p] steps (see SpkMapArgs).  P and S are then the host-known caps -- they size the grid and stride the
  // buffers --, phdr[0] is the number of partials and phdr[1] the step bound of the launch.
  const int32_t* prow = nullptr; const int32_t* pstart = nullptr; const int32_t* psteps = nullptr;
  const int32_t* phdr = nullptr;
};

struct SpkEmbedArgs {   // relu(linear(h)) / ||.||, mean over an utterance's partials (models.py:514-518,539)
  const float* hfin; const float* lw; const float* lb; float* g;
  int32_t utterances, n_part, H;
  const int32_t* poff = nullptr;   // ragged batches: row u owns partials [poff[u], poff[u+1]); none = a zero row
};

// The partial map of a ragged batch, built on the device by one small launch: row u of frames[u] mel frames (clamped
// to [0, F]) has spk_partials(frames[u]) partials (none at 0 frames); poff is the exclusive scan of those counts, every
// partial gets one {row, first frame, steps} entry, entries past the count up to the cap P = U * spk_partials(F) get
// 0 steps, hdr = {count, longest partial}.
struct SpkMapArgs {
  const int32_t* frames = nullptr;
  int32_t U = 0, F = 0, P = 0;
  int32_t* flen = nullptr; int32_t* poff = nullptr; int32_t* prow = nullptr; int32_t* pstart = nullptr;
  int32_t* psteps = nullptr; int32_t* phdr = nullptr;
};

// Developer / test switches.  Process-wide integers that start at their production value and change ONLY through
// qvc_debug_set() (include/qvc.h): the library never reads the environment, so nothing inherited by a deployment
// can alter launch shapes or kernel selection.  The GPU tests flip them in-process to prove the variants equal.
enum DebugSwitch : int32_t {
  DBG_POST_TAIL = 0,        // 1 (default): conv_post + iSTFT / band synthesis as one launch where post_tail_supported(); 0: two launches
  DBG_POST_TAIL_NF,         // column fragments per wave of post_tail_kernel: 4 (default, 128-frame tile) or 2
  DBG_PAIR_WIDE_LAUNCH,     // 1 (default): the three chains of an 8-wave pair layout share a launch; 0: one chain per launch
  DBG_PAIR_CM4,             // 1 (default): chain-major grid for three-chain launches of 4-wave layouts; 0: chains interleaved (x % n)
  DBG_CONV_CL,              // 1 (default): chunk-loop variant of the conv kernel where it applies; 0: one workgroup per row chunk
  DBG_WN_CHUNK,             // 0 (default): 4 WaveNet layers per stack launch; n > 0: n layers; -1: one launch per layer, pre / post as convs
  DBG_PAIR_CHAIN3,          // 0 (default): off; 1: the three pairs of a short-kernel ResBlock chained in one launch (qvc_chain_impl.h:
                            //    bit-identical, measured SLOWER -- the k 3 pairs cost less riding in the three-chain launches)
  DBG_WN_KERNEL,            // WaveNet stack kernel variant (0 = default; 1 generic, 2 / 3 the 32- / 64-frame continuous-stream tile)
  DBG_LAUNCH_STOP,          // -1 (default): off; n >= 0: the whole-path entry points issue only their steps [0, n) (Path::step)
  DBG_LIVE_TRIM,            // 1 (default): qvc_live_step drops the rows a stage can no longer use before the next stage; 0: every stage over the whole window
  DBG_COUNT
};
inline std::atomic<int32_t>* debug_table() {
  static std::atomic<int32_t> t[DBG_COUNT] = {{1}, {4}, {1}, {1}, {1}, {0}, {0}, {0}, {-1}, {1}};
  return t;
}
inline int debug_get(int which) { return debug_table()[which].load(std::memory_order_relaxed); }
inline const char* const* debug_names() {
  static const char* const n[DBG_COUNT] = {"post_tail", "post_tail_nf", "pair_wide_launch", "pair_cm4", "conv_cl", "wn_chunk", "pair_chain3", "wn_kernel",
                                           "launch_stop", "live_trim"};
  return n;
}
// Layers per whole-stack WaveNet launch.  The debug switch "wn_chunk" overrides it (tuning runs; -1 = no stack kernel
// at all: one fused launch per layer and the coupling layers' pre / post as separate convs -- the path taken by
// configurations the stack kernel does not cover, selectable so that the tests can exercise it).
inline int wn_chunk(int layers) {
  const int env = debug_get(DBG_WN_CHUNK);
  if (env < 0) return 0;
  if (env > 0) return env <= layers ? env : layers;
  return layers % 4 == 0 ? 4 : layers;
}
// Read-only companion of launch_stop (qvc_debug_get "launch_steps"): the steps the last whole-path call would have issued.
inline std::atomic<int32_t>& debug_launch_steps() {
  static std::atomic<int32_t> n{0};
  return n;
}

// Launchers return a QVC_* status.  `stream` is a hipStream_t.  The six kernel families below are chosen in qvc_select.h
// (choose_*: instantiation, tile, grid, LDS) and dispatched by the device translation units (dispatch_*).
int launch_conv(const ConvDesc& d, ConvArgs a, int batch, int epi, int dtype, void* stream);
// n pairs (1..3) of equal shape class in one launch; d1[i] / d2[i] are chain i's convs
int launch_pair3(const ConvDesc* d1, const ConvDesc* d2, const PairArgs3& a, int batch, int dtype, void* stream);
// the n pairs of one ResBlock chained in one launch (chain_supported() says when); d1[q] / d2[q] are pair q's convs
int launch_chain(const ConvDesc* d1, const ConvDesc* d2, const ChainArgs& a, int batch, int dtype, void* stream);
bool wn_stack_supported(const ConvDesc& din, int layers);
int launch_wn_stack(const ConvDesc& din, const WnStackArgs& a, int batch, int dtype, void* stream);
int launch_wn(const ConvDesc& din, WnArgs a, int batch, int dtype, void* stream);
int launch_gemv(const GemvArgs& a, void* stream);

// ---- several strided copies / zero fills in ONE launch (the streaming step's ring hand-offs and slides: ~35 strided
//      memcpys of a few hundred KB each cost ~5 us apiece as separate graph nodes).  All sizes in bytes, multiples of
//      4; src == nullptr fills with zeros.  The regions written by one batch must not overlap anything the same batch
//      reads or writes -- the descriptors run concurrently.
struct CopyDesc {
  void* dst;
  const void* src;
  uint32_t dpitch, spitch, width, rows;
};
constexpr int kCopyBatchMax = 12;
int launch_copy_batch(const CopyDesc* d, int n, void* stream);

// ---- the tick forms (qvc_stream.h: stream_tick, live_tick): slot b brings n = clamp(n_new[b], 0, hop) frames, the counts
//      in device memory, so what moves is decided on the device.  One definition of the clamp for the kernel and the
//      host twin.
QVC_HD int tick_count(const int32_t* n_new, int b, int hop) {
  const int n = n_new[b];
  return n < 0 ? 0 : (n < hop ? n : hop);
}

// ---- the mover of a tick (qvc_stream.h: CountedQueue): copy_batch's job -- several independent strided
//      copies / zero fills in ONE launch -- with what moves per slot decided on the device by n = tick_count(n_new, slot,
//      hop).  A descriptor covers `slots` slots of `rows` rows each; slot s starts s * rows * dpitch bytes into dst and
//      s * rows * spitch bytes into src.  Of every row of a slot it writes `width` bytes:
//          [0, fixed + n * unit)      copied from the slot's source row, read from byte n * shift on
//          [fixed + n * unit, width)  zeros
//      (src == nullptr: fixed = unit = shift = 0, a zero fill).  A slot with n == 0 is not touched at all -- neither read
//      nor written -- unless the descriptor says kCountedIdleZero: then its `width` bytes are zeros and src is not read.
//      All sizes in bytes, multiples of 4, fixed + hop * unit <= width <= dpitch; the widest read of a source row,
//      hop * shift + fixed + hop * unit, is the caller's to keep inside the row.  As with copy_batch, nothing a launch
//      writes may overlap what the same launch reads or writes.
struct CountedDesc {
  void* dst;
  const void* src;
  uint32_t dpitch, spitch;
  uint32_t fixed, unit, shift, width;
  uint32_t rows;          // per slot
  uint32_t flags;
};
constexpr uint32_t kCountedIdleZero = 1u;
// What the launch shares: the counts and, by its first workgroup, the two pieces of per-slot bookkeeping of a tick.
//   pos_eff / len_eff (with pos and lens; all four or none): what the segments' launches see in this tick --
//       n > 0: pos[b], lens[b];   n == 0: idle_pos, 0 -- an empty sequence in every segment (idle_pos >= every segment's
//       Ragged::off), so an idle slot's tiles return at once
//       len_cap (the window, live_tick): n > 0: len_eff[b] = min(lens[b], pos[b] + n) -- the sequence ends behind the
//       slot's n new frames, so the zero-filled rows behind them are past its end and not frames of it
//   pos_add: pos_add[b] += n (nothing else in the same launch may read it)
struct CountedHead {
  const int32_t* n_new = nullptr;
  int32_t slots = 0, hop = 0;
  const int32_t* pos = nullptr; const int32_t* lens = nullptr;
  int32_t* pos_eff = nullptr; int32_t* len_eff = nullptr;
  int32_t idle_pos = 0;
  int32_t* pos_add = nullptr;
  bool len_cap = false;
};
// len_eff of a slot with n > 0 new frames: one definition for the kernel and the host twin
QVC_HD int counted_len(const CountedHead& h, int b, int n) {
  const int len = h.lens[b], end = h.pos[b] + n;
  return h.len_cap && end < len ? end : len;
}
int launch_copy_counted(const CountedHead& h, const CountedDesc* d, int n, void* stream);

// ---- exact windows over packed utterances (qvc_stream.h: infer_windows): the rows of a call are windows of W = 2C + n
//      frames cut from utterances that lie back to back in packed buffers, named by a table in device memory (qvc_window,
//      include/qvc.h).  One definition of the clamp for the two kernels and the host twin: whatever the table holds,
//      0 <= base <= total, 0 <= length <= total - base, 0 <= start <= length, 0 <= count <= min(n, length - start) -- so
//      every frame a row reads lies in [base, base + length) and every frame it delivers in [base + start, base + start + count).
struct WindowRow { int32_t base, length, start, count; };
QVC_HD WindowRow window_row(const qvc_window* win, int r, int n, int total) {
  WindowRow w{win[r].base, win[r].length, win[r].start, win[r].count};
  w.base = w.base < 0 ? 0 : (w.base < total ? w.base : total);
  const int room = total - w.base;
  w.length = w.length < 0 ? 0 : (w.length < room ? w.length : room);
  w.start = w.start < 0 ? 0 : (w.start < w.length ? w.start : w.length);
  const int most = w.length - w.start < n ? w.length - w.start : n;
  w.count = w.count < 0 ? 0 : (w.count < most ? w.count : most);
  return w;
}
// The two launches around the path.  Row r's window row i is frame start - C + i of its utterance.
//   gather   unit_win [rows][W][unit_channels] <- unit_packed [total][unit_channels]; with noise_packed (inter, total):
//            noise_win (rows, inter, W) <- its columns; window rows outside [0, length) are written as 0.0.  pos_eff /
//            len_eff: what the path's launches see -- start + C at buffer row W - n and length; an idle row (count 0) gets
//            W and 0, an empty sequence in every segment as an idle tick slot's, and none of its window is written
//   deliver  out_packed[(base + start) * spf ...] <- rows [first, first + count) of the row's waveform in
//            wave (rows, wave_rows * spf)
struct WindowArgs {
  const qvc_window* win = nullptr;
  int32_t rows = 0, n = 0, C = 0, W = 0, total = 0;
  const float* unit_packed = nullptr; float* unit_win = nullptr; int32_t unit_channels = 0;
  const float* noise_packed = nullptr; float* noise_win = nullptr; int32_t inter = 0;
  int32_t* pos_eff = nullptr; int32_t* len_eff = nullptr;
  const float* wave = nullptr; int32_t wave_rows = 0, first = 0, spf = 0; float* out_packed = nullptr;
};
// the most total_frames a call takes: start + C and every frame index stay inside int32
constexpr int32_t kWindowMaxTotal = INT32_MAX - (1 << 25);
int launch_window_gather(const WindowArgs& a, void* stream);
int launch_window_deliver(const WindowArgs& a, void* stream);

int launch_sample(const SampleArgs& a, void* stream);
int launch_sample_rows(const SampleRowsArgs& a, void* stream);
// (rows, channels, frames) fp32 in the reference's layout, frames [frame0, frame0 + frames): the tensor the draw sites would compute
int launch_noise_fill(const NoiseRng& rng, int rows, int channels, int frames, int frame0, float* out, void* stream);
int launch_tail(const TailArgs& a, void* stream);
int launch_post_tail(const ConvDesc& d, PostTailArgs a, int batch, int dtype, void* stream);   // bands = post_tail_bands(d)

}  // namespace qvc
