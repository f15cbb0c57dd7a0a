// qvc_stream.h -- incremental (streaming) conversion: one hop of new unit frames per call, state carried in a
// caller-owned buffer (BASELINE.json configs[4]).  Written once and parameterised on the backend like qvc_path.h.
//
// The reference converts a whole utterance in one shot (no chunking, no streaming).  Every op on
// the path is a convolution with a bounded, symmetric receptive field (modules.py:64, models.py:327-357) and g is
// global, so the path can run as a pipeline of SEGMENTS, each fed from a ring buffer that keeps the last 2*H frames
// of its input (H = the segment's one-sided receptive field):
//
//     E   enc_p                          ring: unit frames              H = enc_layers * (k-1)/2         (32)
//     F_k coupling layer k of the flow   ring: z before that layer      H = flow_layers * (k-1)/2        (8 each)
//     D1  conv_pre + ups[0] + MRF 0      ring: z after the flow         H = 3 + taps + ceil(mrf0 / r0)   (20)
//     D2  ups[1] + MRF 1 + conv_post + iSTFT / band synthesis           H in unit frames                 (6)
//         ring: the three ResBlock outputs of stage 0
//
// A step appends `hop` new frames to E's ring, runs every segment over its window of 2*H + hop frames, hands the
// CENTRAL hop frames of each result to the next ring (the H frames at either edge lack context and are dropped) and
// slides the rings.  A frame therefore costs (2*H + hop) / hop of its offline cost per segment -- 1.08x overall at
// hop 320 -- instead of (2*88 + hop) / hop for windows over the whole path, and the output lags the input by
// lag() = sum of the H's (90 frames at the shipped config): the look-ahead a non-causal network needs anyway.
// Inside a segment the fused kernels keep their layers' state on chip, so there are no per-layer caches to carry.
// Sequence starts and ends inside a window are exact: every kernel masks its input rows by the absolute position
// of the window (Ragged: pos / lens), i.e. each conv zero-pads at the sequence's own ends.
#pragma once
#include "qvc_path.h"

namespace qvc {

struct StreamGeom {
  int32_t status = QVC_OK;
  int32_t hop = 0, He = 0, Hf = 0, Hd1 = 0, Hd2 = 0, nf = 0, r0 = 1;
  int lag() const { return He + nf * Hf + Hd1 + Hd2; }
  int max_window() const { return hop + 2 * std::max(std::max(He, Hf), std::max(Hd1, Hd2)); }
};

inline StreamGeom stream_geom(const Plan& P, int hop) {
  StreamGeom G;
  const qvc_config& c = P.cfg;
  if (P.status != QVC_OK) { G.status = P.status; return G; }
  if (hop < 1 || c.n_ups != 2 || c.n_flows > 16) { G.status = hop < 1 ? QVC_ERR_BAD_ARG : QVC_ERR_BAD_CONFIG; return G; }
  // the halo / lag arithmetic below is the band-synthesis decoders' (63-tap FIR, output_padding 1-i): streaming the
  // single-band decoder is not built
  if (c.decoder == QVC_DEC_ISTFT) { G.status = QVC_ERR_BAD_CONFIG; return G; }
  const int K2 = (c.wn_kernel_size - 1) / 2;
  G.hop = hop; G.nf = c.n_flows; G.r0 = c.upsample_rates[0];
  G.He = c.enc_layers * K2;
  G.Hf = c.flow_layers * K2;
  auto mrf = [&]() {   // one-sided reach of a ResBlock stack in its own frames: sum over pairs of (k-1)/2 * (d + 1)
    int worst = 0;
    for (int j = 0; j < c.n_resblocks; ++j) {
      int s = 0;
      for (int q = 0; q < 3; ++q) s += (c.resblock_kernel_sizes[j] - 1) / 2 * (c.resblock_dilations[j][q] + 1);
      worst = std::max(worst, s);
    }
    return worst;
  }();
  const int taps0 = P.stages[0].up.taps, taps1 = P.stages[1].up.taps;
  const int r1 = c.upsample_rates[1];
  G.Hd1 = 3 + taps0 + ceil_div(mrf, G.r0) + 1;                               // conv_pre (k 7), ups[0], MRF 0, margin
  // ups[1] (in stage-0 frames) + [MRF 1 + conv_post (k 7 + reflect) + iSTFT overlap + 63-tap FIR] (stage-1 frames)
  G.Hd2 = ceil_div(taps1 + ceil_div(mrf + 4 + 2 + 2, r1) + 1, G.r0) + 1;
  return G;
}

// What every streaming entry point starts from: the plan and the stream geometry for (cfg, hop), or why not.
inline int stream_plan(const qvc_config* cfg, int hop, Plan& P, StreamGeom& G) {
  if (!cfg || hop <= 0) return QVC_ERR_BAD_ARG;
  P = build_plan(*cfg);
  G = stream_geom(P, hop);
  return G.status;
}

struct StreamState {     // byte offsets into the caller-owned state buffer
  int64_t unit = 0;      // fp32 (B, unit_channels, 2*He + hop), the reference's (B, C, T) layout
  int64_t zf[16] = {};   // fp32 [B][2*Hf + hop][C]: z in front of coupling layer k
  int64_t zd = 0;        // fp32 [B][2*Hd1 + hop][C]: z after the flow
  int64_t s0[3] = {};    // operand type [B][(2*Hd2 + hop) * r0][ch0]: stage-0 ResBlock outputs
  int64_t bytes = 0;
};

inline StreamState carve_stream_state(const Plan& P, const StreamGeom& G, int B) {
  StreamState S;
  const qvc_config& c = P.cfg;
  int64_t off = 0;
  auto take = [&](int64_t n) { int64_t o = off; off = align_up(off + n, 256); return o; };
  S.unit = take((int64_t)B * c.unit_channels * (2 * G.He + G.hop) * 4);
  for (int k = 0; k < G.nf; ++k) S.zf[k] = take((int64_t)B * (2 * G.Hf + G.hop) * c.inter_channels * 4);
  S.zd = take((int64_t)B * (2 * G.Hd1 + G.hop) * c.inter_channels * 4);
  for (int j = 0; j < 3; ++j) S.s0[j] = take((int64_t)B * (2 * G.Hd2 + G.hop) * G.r0 * P.stages[0].ch * 2);
  S.bytes = off;
  return S;
}

struct StreamScratch {   // carved from the END of the step's workspace, after the path's own workspace
  int64_t path_bytes = 0;   // workspace of the widest segment
  int64_t noise = 0;        // fp32 (B, C, 2*He + hop): the step's noise placed at the frames enc_p really outputs
  int64_t zwork[2] = {};    // fp32 [B][2*Hf + hop][C]: the coupling layer updates z in place on a copy of its ring
                            // (two of them: layer k's result feeds the copy for layer k+1 in the same launch)
  int64_t wave = 0;         // fp32 (B, spf * (2*Hd2 + hop))
  int64_t tmp[21] = {};     // slide buffers, one per ring (unit, zf[0..nf), zd, s0[0..3)): that ring's kept part
  int64_t bytes = 0;
};

inline int samples_per_frame(const Plan& P) { return P.total_up * P.cfg.hop * P.cfg.subbands; }

inline StreamScratch carve_stream_scratch(const Plan& P, const StreamGeom& G, int B) {
  StreamScratch X;
  const qvc_config& c = P.cfg;
  X.path_bytes = carve_workspace(P, B, G.max_window()).bytes;
  int64_t off = X.path_bytes;
  auto take = [&](int64_t n) { int64_t o = off; off = align_up(off + n, 256); return o; };
  X.noise = take((int64_t)B * c.inter_channels * (2 * G.He + G.hop) * 4);
  for (int k = 0; k < 2; ++k) X.zwork[k] = take((int64_t)B * (2 * G.Hf + G.hop) * c.inter_channels * 4);
  X.wave = take((int64_t)B * samples_per_frame(P) * (2 * G.Hd2 + G.hop) * 4);
  int r = 0;
  X.tmp[r++] = take((int64_t)B * c.unit_channels * 2 * G.He * 4);
  for (int k = 0; k < G.nf; ++k) X.tmp[r++] = take((int64_t)B * 2 * G.Hf * c.inter_channels * 4);
  X.tmp[r++] = take((int64_t)B * 2 * G.Hd1 * c.inter_channels * 4);
  for (int j = 0; j < 3; ++j) X.tmp[r++] = take((int64_t)B * 2 * G.Hd2 * G.r0 * P.stages[0].ch * 2);
  X.bytes = off;
  return X;
}

// One step.  Backend adds:  int copy_batch(const CopyDesc* d, int n)  -- n independent strided copies / zero fills in
// one launch (qvc_kernels.h).  All data movement of a step goes through it: 10 launches where one memcpy per
// hand-off / slide would be ~35.
//   unit_new  (B, unit_channels, hop) fp32: unit frames [pos, pos + hop) of every stream
//   noise_new (B, inter, hop) fp32:         the N(0,1) draw of models.py:94 for frames [pos - He, pos - He + hop)
//                                           (the frames enc_p finishes in this step)
//   out       (B, hop * samples_per_frame): waveform of frames [pos - lag, pos - lag + hop); zeros where that is
//                                           outside [0, lens[b])
//   pos, lens (B,) int32 in the backend's memory: first new frame of this step / sequence length (large if unknown)
//   rng       with noise_new == nullptr: the draw is computed in enc_p's draw site for key rng->keys[slot] at the absolute
//             frame of every window row (Path::rng) -- no noise staging, X.noise stays untouched
template <class Backend>
int stream_step(const Plan& P, const char* blob, char* state, char* ws, const float* unit_new, const float* g,
                const float* noise_new, float* out, int B, int hop, const int32_t* pos, const int32_t* lens, Backend& be,
                const NoiseRng* rng = nullptr) {
  const StreamGeom G = stream_geom(P, hop);
  if (G.status != QVC_OK) return G.status;
  const StreamState S = carve_stream_state(P, G, B);
  const StreamScratch X = carve_stream_scratch(P, G, B);
  const qvc_config& c = P.cfg;
  const int C = c.inter_channels, UC = c.unit_channels;
  const int h = hop, He = G.He, Hf = G.Hf, Hd1 = G.Hd1, Hd2 = G.Hd2;
  int st = QVC_OK;
  auto ok = [&](int rc) { if (st == QVC_OK && rc != QVC_OK) st = rc; };
  CopyDesc cd[kCopyBatchMax];
  int ncd = 0;
  auto flush = [&]() { if (ncd) ok(be.copy_batch(cd, ncd)); ncd = 0; };
  // queue a strided copy (src == nullptr: zero fill); the descriptors between two flushes run as ONE launch and must be
  // independent of each other
  auto add = [&](void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    if (ncd == kCopyBatchMax) flush();
    if ((dpitch | spitch | width | rows) >> 32) { ok(QVC_ERR_BAD_ARG); return; }
    cd[ncd++] = CopyDesc{dst, src, (uint32_t)dpitch, (uint32_t)spitch, (uint32_t)width, (uint32_t)rows};
  };
  // the rings slide at the END of the step, all of them in two launches (out to the scratch, back in: the kept part and
  // its destination overlap).  A ring is read by exactly one segment per step, so nothing needs it slid earlier.
  struct Slide { char* ring; size_t rows, keep, hopb; };
  Slide slides[21];
  int nslide = 0;
  auto slide = [&](char* ring, size_t rows, size_t keep, size_t hopb) { slides[nslide++] = Slide{ring, rows, keep, hopb}; };
  auto make = [&](int T, int lag_before) {
    Path<Backend> p{P, blob, ws, carve_workspace(P, B, T), B, T, be};
    p.lens = lens; p.pos = pos; p.off = lag_before + (T - h);      // buffer row `off` is absolute frame pos[b]
    p.wn_wide = false;
    return p;
  };
  const size_t zrow = (size_t)C * 4;                               // one frame of z
  const int Tf = 2 * Hf + h;
  // hand the central hop frames of a segment's result (`src`, frame pitch zrow, `srcT` frames per stream) to coupling
  // layer k: into its ring's tail AND -- together with the ring's kept part -- into the work copy the layer updates
  auto feed_flow = [&](int k, const char* src, int srcT) {
    char* ring = state + S.zf[k];
    char* zw = ws + X.zwork[k & 1];
    add(ring + (size_t)2 * Hf * zrow, (size_t)Tf * zrow, src, (size_t)srcT * zrow, (size_t)h * zrow, (size_t)B);
    add(zw, (size_t)Tf * zrow, ring, (size_t)Tf * zrow, (size_t)2 * Hf * zrow, (size_t)B);
    add(zw + (size_t)2 * Hf * zrow, (size_t)Tf * zrow, src, (size_t)srcT * zrow, (size_t)h * zrow, (size_t)B);
    flush();
  };

  {   // the conditioning table (cond rows x g) once per step: every segment's workspace keeps it at the same place
    Path<Backend> p = make(Tf, 0);
    p.cond_table(g);
    ok(p.status);
  }
  // ---- E: enc_p over the unit ring
  {
    const int T = 2 * He + h;
    char* ring = state + S.unit;
    char* nz = ws + X.noise;                                       // zeros either side of the step's noise
    add(ring + (size_t)2 * He * 4, (size_t)T * 4, unit_new, (size_t)h * 4, (size_t)h * 4, (size_t)B * UC);
    if (noise_new) {
      add(nz, (size_t)T * 4, nullptr, 0, (size_t)He * 4, (size_t)B * C);
      add(nz + (size_t)He * 4, (size_t)T * 4, noise_new, (size_t)h * 4, (size_t)h * 4, (size_t)B * C);
      add(nz + (size_t)(He + h) * 4, (size_t)T * 4, nullptr, 0, (size_t)He * 4, (size_t)B * C);
    }
    flush();
    Path<Backend> p = make(T, 0);
    if (!noise_new && rng) p.rng = *rng;     // (neither: enc_p refuses)
    p.enc_p(reinterpret_cast<const float*>(ring), noise_new ? reinterpret_cast<const float*>(nz) : nullptr, p.template wsp<float>(p.W.z));
    ok(p.status);
    if (G.nf > 0) feed_flow(0, ws + p.W.z + (size_t)He * zrow, T);
    else {
      add(state + S.zd + (size_t)2 * Hd1 * zrow, (size_t)(2 * Hd1 + h) * zrow, ws + p.W.z + (size_t)He * zrow, (size_t)T * zrow, (size_t)h * zrow, (size_t)B);
      flush();
    }
    slide(ring, (size_t)B * UC, (size_t)2 * He * 4, (size_t)h * 4);
  }
  // ---- F_k: one coupling layer per segment, in place on a copy of its ring (its edge rows come out wrong and
  //      must not be written back: the ring has to keep the untouched values for the next step's context)
  for (int k = 0; k < G.nf; ++k) {
    char* zw = ws + X.zwork[k & 1];
    Path<Backend> p = make(Tf, He + k * Hf);
    p.flow_step(P.flow[(size_t)k], reinterpret_cast<float*>(zw), -1.f);
    ok(p.status);
    if (k + 1 < G.nf) feed_flow(k + 1, zw + (size_t)Hf * zrow, Tf);
    else {
      add(state + S.zd + (size_t)2 * Hd1 * zrow, (size_t)(2 * Hd1 + h) * zrow, zw + (size_t)Hf * zrow, (size_t)Tf * zrow, (size_t)h * zrow, (size_t)B);
      flush();
    }
    slide(state + S.zf[k], (size_t)B, (size_t)2 * Hf * zrow, (size_t)h * zrow);
  }
  // ---- D1: conv_pre + stage 0; its three ResBlock outputs feed the stage-0 rings
  const int ch0 = P.stages[0].ch, r0 = G.r0;
  {
    const int T = 2 * Hd1 + h;
    char* ring = state + S.zd;
    Path<Backend> p = make(T, He + G.nf * Hf);
    p.dec_front(reinterpret_cast<const float*>(ring));
    ok(p.status);
    const size_t row = (size_t)ch0 * 2;
    for (int j = 0; j < 3; ++j) {
      const int jj = j < c.n_resblocks ? j : 0;
      add(state + S.s0[j] + (size_t)2 * Hd2 * r0 * row, (size_t)(2 * Hd2 + h) * r0 * row,
          ws + p.W.ra[0][(size_t)jj] + (size_t)Hd1 * r0 * row, (size_t)T * r0 * row, (size_t)h * r0 * row, (size_t)B);
    }
    flush();
    slide(ring, (size_t)B, (size_t)2 * Hd1 * zrow, (size_t)h * zrow);
  }
  // ---- D2: remaining stages + conv_post + iSTFT / band synthesis; the central hop frames are the step's output
  {
    const int T = 2 * Hd2 + h;
    const int spf = samples_per_frame(P);
    Path<Backend> p = make(T, He + G.nf * Hf + Hd1);
    for (int j = 0; j < 3; ++j) p.s0_override[j] = state + S.s0[j];
    p.dec_back_wave(p.template wsp<float>(p.W.post), reinterpret_cast<float*>(ws + X.wave));
    ok(p.status);
    add(out, (size_t)h * spf * 4, ws + X.wave + (size_t)Hd2 * spf * 4, (size_t)T * spf * 4, (size_t)h * spf * 4, (size_t)B);
    const size_t row = (size_t)ch0 * 2;
    for (int j = 0; j < 3; ++j) slide(state + S.s0[j], (size_t)B, (size_t)2 * Hd2 * r0 * row, (size_t)h * r0 * row);
  }
  // ---- slide every ring by one hop: kept parts out (in the launch that also delivers the output), then back in
  for (int r = 0; r < nslide; ++r) add(ws + X.tmp[r], slides[r].keep, slides[r].ring + slides[r].hopb, slides[r].keep + slides[r].hopb, slides[r].keep, slides[r].rows);
  flush();
  for (int r = 0; r < nslide; ++r) add(slides[r].ring, slides[r].keep + slides[r].hopb, ws + X.tmp[r], slides[r].keep, slides[r].keep, slides[r].rows);
  flush();
  return st;
}

// ---------------------------------------------------------------- windowed step with a bounded look-ahead (live_step)
// The segment rings above are exact and cheap, but their output lags the input by lag() frames and stream_geom takes
// the band-synthesis decoders with two up-samplers only.  live_step trades cost for latency and takes EVERY plan: it
// keeps ONE ring -- the last W = C + L + hop unit frames of each stream (and, for the pointer form of the noise, their
// noise frames) -- and runs the whole path (Path::infer) over that window, whose last row is the newest frame:
//
//     row:   0 ............. C ......... C+hop ......... C+L = W-hop ............ W
//            |  left context  | delivered |   look-ahead  |  this step's new frames |
//     frame: pos-L-C       pos-L       pos-L+hop         pos                     pos+hop
//
// The window ends where the stream has got to, so the kernels see a sequence that ends there (Ragged: the buffer end is
// the sequence end unless lens[b] comes first): the delivered frames [pos - L, pos - L + hop) are those of the OFFLINE
// conversion of the prefix [0, min(len, pos + hop)) -- exact by definition, not an approximation of the whole-utterance
// result.  L = look_ahead in [0, C] is the caller's trade: 0 = no lag at all, C = the whole receptive field, where the
// prefix conversion and the whole-utterance conversion agree on the delivered frames (exact streaming).
// C bounds the one-sided receptive field of the path in unit frames: the window's first row is not the sequence start
// (once pos - L > C), so the rows nearer than C to it lack left context and are never delivered.
//     C = He + nf * Hf + Hdec,   Hdec = 3 (conv_pre) + r_0,   r_n = mrf + 8 at the last stage's output
//     (conv_post k 7 + reflect pad, iSTFT overlap, synthesis FIR),   r_i = taps_i + ceil(r_{i+1} / rate_i) + 1 at stage
//     i's input, + mrf for the ResBlocks of stage i - 1 in front of it
// (89 at the shipped config; stream_geom's lag is 90, the measured receptive field 84).
// Plain form: every stage over all W rows -- a frame costs W / hop of its offline cost in every stage.
// Trimmed form (the default): a stage's first rows lack left context and no later stage can use them, so they are
// dropped before the next stage runs.  Three segments, each a Path with its own T and off and a compact hand-off through
// copy_batch, as stream_step's:
//     E  enc_p                    rows [0, W)                    T = W
//     F  the flow                 rows [He, W)                   T = W - He
//     D  the decoder and the tail rows [He + nf * Hf, W)         T = Hdec + L + hop, delivered rows [Hdec, Hdec + hop)
// The decoder -- 80 % of the path's FLOPs -- then costs (Hdec + L + hop) / hop per frame instead of W / hop (49 rows
// instead of 113 at the shipped config, hop 16, L 8).  Every delivered row keeps the left context its stage needs, so
// both forms compute the same values for it.
struct LiveGeom {
  int32_t status = QVC_OK;
  int32_t He = 0, Hf = 0, nf = 0, Hdec = 0;
  int32_t hop = 0, L = 0, W = 0;                   // set by live_plan
  int C() const { return He + nf * Hf + Hdec; }
};

inline LiveGeom live_geom(const Plan& P) {
  LiveGeom G;
  if (P.status != QVC_OK) { G.status = P.status; return G; }
  const qvc_config& c = P.cfg;
  const int K2 = (c.wn_kernel_size - 1) / 2;
  G.He = c.enc_layers * K2; G.Hf = c.flow_layers * K2; G.nf = c.n_flows;
  int mrf = 0;               // one-sided reach of a ResBlock stack in its own frames (as in stream_geom)
  for (int j = 0; j < c.n_resblocks; ++j) {
    int s = 0;
    for (int q = 0; q < 3; ++q) s += (c.resblock_kernel_sizes[j] - 1) / 2 * (c.resblock_dilations[j][q] + 1);
    mrf = std::max(mrf, s);
  }
  int r = mrf + 8;
  for (int i = c.n_ups - 1; i >= 0; --i) {
    r = P.stages[(size_t)i].up.taps + ceil_div(r, c.upsample_rates[i]) + 1;
    if (i > 0) r += mrf;
  }
  G.Hdec = 3 + r;
  return G;
}

// What every live entry point starts from: the plan and the window for (cfg, hop, look_ahead), or why not.
inline int live_plan(const qvc_config* cfg, int hop, int look_ahead, Plan& P, LiveGeom& G) {
  if (!cfg || hop < 1) return QVC_ERR_BAD_ARG;
  P = build_plan(*cfg);
  G = live_geom(P);
  if (G.status != QVC_OK) return G.status;
  if (look_ahead < 0 || look_ahead > G.C()) return G.status = QVC_ERR_BAD_ARG;
  if ((int64_t)G.C() + look_ahead + hop > (1 << 24)) return G.status = QVC_ERR_BAD_ARG;
  G.hop = hop; G.L = look_ahead; G.W = G.C() + look_ahead + hop;
  return QVC_OK;
}

struct LiveState {       // byte offsets into the caller-owned state buffer
  int64_t unit = 0;      // fp32 (B, unit_channels, W), the reference's (B, C, T) layout
  int64_t noise = 0;     // fp32 (B, inter_channels, W): the noise of the same frames (pointer form only)
  int64_t bytes = 0;
};

inline LiveState carve_live_state(const Plan& P, const LiveGeom& G, int B) {
  LiveState S;
  int64_t off = 0;
  auto take = [&](int64_t n) { int64_t o = off; off = align_up(off + n, 256); return o; };
  S.unit = take((int64_t)B * P.cfg.unit_channels * G.W * 4);
  S.noise = take((int64_t)B * P.cfg.inter_channels * G.W * 4);
  S.bytes = off;
  return S;
}

struct LiveScratch {     // carved from the END of the step's workspace, after the path's own workspace
  int64_t path_bytes = 0;   // carve_workspace(P, B, W): the widest segment
  int64_t zf = 0;           // fp32 [B][W - He][C]: z handed to the flow, updated in place (trimmed form)
  int64_t zd = 0;           // fp32 [B][W - He - nf * Hf][C]: z handed to the decoder (trimmed form)
  int64_t wave = 0;         // fp32 (B, spf * W): the window's waveform (trimmed form: of the decoder's rows)
  int64_t tmp[2] = {};      // slide buffers: the kept W - hop frames of the unit / noise ring
  int64_t bytes = 0;
};

inline LiveScratch carve_live_scratch(const Plan& P, const LiveGeom& G, int B) {
  LiveScratch X;
  X.path_bytes = carve_workspace(P, B, G.W).bytes;
  int64_t off = X.path_bytes;
  auto take = [&](int64_t n) { int64_t o = off; off = align_up(off + n, 256); return o; };
  X.zf = take((int64_t)B * (G.W - G.He) * P.cfg.inter_channels * 4);
  X.zd = take((int64_t)B * (G.W - G.He - G.nf * G.Hf) * P.cfg.inter_channels * 4);
  X.wave = take((int64_t)B * samples_per_frame(P) * G.W * 4);
  X.tmp[0] = take((int64_t)B * P.cfg.unit_channels * (G.W - G.hop) * 4);
  X.tmp[1] = take((int64_t)B * P.cfg.inter_channels * (G.W - G.hop) * 4);
  X.bytes = off;
  return X;
}

// The path over the window held in the rings -- what a step runs between appending the new frames and delivering:
// the plain form or the three trimmed segments.  `unit` / `noise`: the rings (noise == nullptr: the generator form, rng).
// pos / lens: buffer row T - hop of a segment over the window's last T rows is absolute frame pos[b].  The window's
// waveform ends up in X.wave: wave_rows rows per stream, the hop delivered ones from row `first` on.
template <class Backend>
int live_window(const Plan& P, const LiveGeom& G, const LiveScratch& X, const char* blob, char* ws, const float* unit, const float* g,
                const float* noise, int B, const int32_t* pos, const int32_t* lens, Backend& be, const NoiseRng* rng, bool trim,
                size_t& wave_rows, size_t& first) {
  const qvc_config& c = P.cfg;
  const size_t W = (size_t)G.W;
  int st = QVC_OK;
  auto ok = [&](int rc) { if (st == QVC_OK && rc != QVC_OK) st = rc; };
  // one strided copy per hand-off, each a launch of its own
  auto hand = [&](void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    if ((dpitch | spitch | width | rows) >> 32) { ok(QVC_ERR_BAD_ARG); return; }
    const CopyDesc cd{dst, src, (uint32_t)dpitch, (uint32_t)spitch, (uint32_t)width, (uint32_t)rows};
    ok(be.copy_batch(&cd, 1));
  };
  // a segment over the window's last T rows: its buffer row T - hop is absolute frame pos[b]
  auto make = [&](int T) {
    Path<Backend> p{P, blob, ws, carve_workspace(P, B, T), B, T, be};
    p.lens = lens; p.pos = pos; p.off = T - G.hop;
    p.wn_wide = false;
    return p;
  };
  float* wave = reinterpret_cast<float*>(ws + X.wave);
  wave_rows = W; first = (size_t)G.C();
  if (!trim) {
    Path<Backend> p = make(G.W);
    if (!noise && rng) p.rng = *rng;         // (neither: enc_p refuses)
    p.infer(unit, g, noise, wave);
    ok(p.status);
  } else {
    const size_t zrow = (size_t)c.inter_channels * 4;              // one frame of z
    const int Tf = G.W - G.He, Td = Tf - G.nf * G.Hf;
    {   // E: the conditioning table (every segment's workspace keeps it at the same place) and enc_p
      Path<Backend> p = make(G.W);
      if (!noise && rng) p.rng = *rng;
      p.cond_table(g);
      p.enc_p(unit, noise, p.template wsp<float>(p.W.z));
      ok(p.status);
      hand(ws + X.zf, (size_t)Tf * zrow, ws + p.W.z + (size_t)G.He * zrow, W * zrow, (size_t)Tf * zrow, (size_t)B);
    }
    {   // F: the flow, in place on its rows
      Path<Backend> p = make(Tf);
      p.flow(reinterpret_cast<float*>(ws + X.zf));
      ok(p.status);
      hand(ws + X.zd, (size_t)Td * zrow, ws + X.zf + (size_t)(Tf - Td) * zrow, (size_t)Tf * zrow, (size_t)Td * zrow, (size_t)B);
    }
    {   // D: the decoder and the tail
      Path<Backend> p = make(Td);
      p.dec_trunk_wave(reinterpret_cast<const float*>(ws + X.zd), p.template wsp<float>(p.W.post), wave);
      ok(p.status);
    }
    wave_rows = (size_t)Td; first = (size_t)G.Hdec;
  }
  return st;
}

// One step (G from live_plan).  Backend: as stream_step.
//   unit_new  (B, unit_channels, hop) fp32: unit frames [pos, pos + hop) of every stream
//   noise_new (B, inter, hop) fp32:         the N(0,1) draw of models.py:94 for the SAME frames (no noise lag)
//   out       (B, hop * samples_per_frame): waveform of frames [pos - L, pos - L + hop); zeros where that is outside
//                                           [0, lens[b])
//   pos, lens, rng: as stream_step (rng: the draw at the absolute frame of every window row; the noise ring stays untouched)
//   trim      false: the plain form (one Path over the window)
template <class Backend>
int live_step(const Plan& P, const LiveGeom& G, const char* blob, char* state, char* ws, const float* unit_new, const float* g,
              const float* noise_new, float* out, int B, const int32_t* pos, const int32_t* lens, Backend& be,
              const NoiseRng* rng = nullptr, bool trim = true) {
  if (G.status != QVC_OK || G.W < 2) return G.status != QVC_OK ? G.status : QVC_ERR_BAD_ARG;
  const LiveState S = carve_live_state(P, G, B);
  const LiveScratch X = carve_live_scratch(P, G, B);
  const qvc_config& c = P.cfg;
  const size_t W = (size_t)G.W, h = (size_t)G.hop, keep = W - h;
  const size_t spf = (size_t)samples_per_frame(P);
  int st = QVC_OK;
  auto ok = [&](int rc) { if (st == QVC_OK && rc != QVC_OK) st = rc; };
  CopyDesc cd[kCopyBatchMax];
  int ncd = 0;
  auto flush = [&]() { if (ncd) ok(be.copy_batch(cd, ncd)); ncd = 0; };
  auto add = [&](void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    if ((dpitch | spitch | width | rows) >> 32) { ok(QVC_ERR_BAD_ARG); return; }
    cd[ncd++] = CopyDesc{dst, src, (uint32_t)dpitch, (uint32_t)spitch, (uint32_t)width, (uint32_t)rows};
  };
  char* uring = state + S.unit;
  char* nring = state + S.noise;
  const size_t urows = (size_t)B * c.unit_channels, nrows = (size_t)B * c.inter_channels;
  // ---- append the new frames behind the kept ones
  add(uring + keep * 4, W * 4, unit_new, h * 4, h * 4, urows);
  if (noise_new) add(nring + keep * 4, W * 4, noise_new, h * 4, h * 4, nrows);
  flush();
  const float* unit = reinterpret_cast<const float*>(uring);
  const float* noise = noise_new ? reinterpret_cast<const float*>(nring) : nullptr;
  size_t wave_rows = 0, first = 0;                                 // rows of X.wave, and the first delivered one
  ok(live_window(P, G, X, blob, ws, unit, g, noise, B, pos, lens, be, rng, trim, wave_rows, first));
  // ---- deliver rows [first, first + hop) and slide the rings by one hop: kept parts out, then back in (they overlap
  //      their destination)
  add(out, h * spf * 4, ws + X.wave + first * spf * 4, wave_rows * spf * 4, h * spf * 4, (size_t)B);
  add(ws + X.tmp[0], keep * 4, uring + h * 4, W * 4, keep * 4, urows);
  if (noise_new) add(ws + X.tmp[1], keep * 4, nring + h * 4, W * 4, keep * 4, nrows);
  flush();
  add(uring, W * 4, ws + X.tmp[0], keep * 4, keep * 4, urows);
  if (noise_new) add(nring, W * 4, ws + X.tmp[1], keep * 4, keep * 4, nrows);
  flush();
  return st;
}

// ---------------------------------------------------------------- the tick form: per-slot frame counts per step (live_tick)
// live_step moves every slot by exactly `hop` frames.  A tick lets slot b bring n = clamp(n_new[b], 0, hop) frames, the
// counts in device memory: a late packet (n = 0), a client catching up, a last chunk shorter than hop.  The windowed
// step makes that well defined -- a window whose last row is the newest frame is a sequence that ends there, however
// many frames were appended to get there -- provided the ring is kept RIGHT-aligned:
//
//     INVARIANT  between ticks, ring row r of slot b holds frame pos[b] - W + r (the last W frames; live_step's ring
//                keeps W - hop frames LEFT-aligned between steps).
//     EXCLUSIVE  the two layouts differ, so a tick state is never passed to live_step, nor a lockstep state to live_tick.
//
// A tick is  tick_rings -> the window (live_window, unchanged) -> tick_deliver:
//   tick_rings    shifts every ring row of a slot left by n and appends its n new frames, in place, and writes the
//                 position the window's launches see, pos_eff[b] = pos[b] + n - hop: buffer row W - hop is then that
//                 absolute frame, exactly as live_step's p.off = T - hop assumes, so the segments run unchanged.
//                 pos_eff is negative early in a stream (first tick with n = 1: 1 - hop); ragged_lo / ragged_len and
//                 the generator's frame counter only ever use pos - off, which is negative for a young stream in
//                 live_step too.  A slot with n == 0 gets an empty sequence (len_eff = 0, pos_eff = W: hi = 0 in every
//                 segment), so its tiles return at once and its ring rows and pos are not touched.
//   tick_deliver  the delivered rows [first, first + hop) hold the n frames [pos - L, pos - L + n) at their END:
//                 those go to the front of out[b], zeros behind them, and pos[b] += n.
// With every n == hop: pos_eff = pos, len_eff = lens and the window's launches and bits are live_step's.
// Delivered frame f was computed with the frames up to pos + n - 1 in the window: L + n - 1 - (f - (pos - L)) frames of
// look-ahead, between L and L + n - 1.  With L = C every frame has its whole receptive field whatever n was, so the
// output does not depend on how the stream was cut into ticks; with L < C it legitimately does.
// Backend adds:  static constexpr bool kLiveTick = true  with  int tick_rings(const TickRingsArgs&);
//                int tick_deliver(const TickDeliverArgs&);   -- one that does not say so gets QVC_ERR_BAD_CONFIG.
template <class B, class = void> constexpr bool live_tick_backend = false;
template <class B> constexpr bool live_tick_backend<B, std::void_t<decltype(B::kLiveTick)>> = B::kLiveTick;

struct TickScratch {     // live_step's scratch, then the tick's effective positions and lengths
  LiveScratch live;
  int64_t pos_eff = 0, len_eff = 0;   // int32 [B] each
  int64_t bytes = 0;
};

inline TickScratch carve_tick_scratch(const Plan& P, const LiveGeom& G, int B) {
  TickScratch X;
  X.live = carve_live_scratch(P, G, B);
  int64_t off = X.live.bytes;
  auto take = [&](int64_t n) { int64_t o = off; off = align_up(off + n, 256); return o; };
  X.pos_eff = take((int64_t)B * 4);
  X.len_eff = take((int64_t)B * 4);
  X.bytes = off;
  return X;
}

// One tick (G from live_plan; the state is carved as live_step's, carve_live_state, and holds the right-aligned rings).
//   unit_new  (B, unit_channels, hop) fp32: columns [0, n) of row b are frames [pos[b], pos[b] + n); the rest is not read
//   noise_new (B, inter, hop) fp32:         the same rule, the draw for the same frames
//   out       (B, hop * samples_per_frame): n * spf samples of frames [pos - L, pos - L + n) of the offline conversion
//                                           of the prefix [0, min(lens, pos + n)), zeros outside [0, lens[b]); then zeros
//   n_new     (B,) int32 in the backend's memory, clamped to [0, hop] there; pos is advanced by n there too
template <class Backend>
int live_tick(const Plan& P, const LiveGeom& G, const char* blob, char* state, char* ws, const float* unit_new, const float* g,
              const float* noise_new, float* out, int B, const int32_t* n_new, int32_t* pos, const int32_t* lens, Backend& be,
              const NoiseRng* rng = nullptr, bool trim = true) {
  if constexpr (live_tick_backend<Backend>) {
    if (G.status != QVC_OK || G.W < 2) return G.status != QVC_OK ? G.status : QVC_ERR_BAD_ARG;
    const LiveState S = carve_live_state(P, G, B);
    const TickScratch X = carve_tick_scratch(P, G, B);
    int st = QVC_OK;
    auto ok = [&](int rc) { if (st == QVC_OK && rc != QVC_OK) st = rc; };
    float* uring = reinterpret_cast<float*>(state + S.unit);
    float* nring = noise_new ? reinterpret_cast<float*>(state + S.noise) : nullptr;
    int32_t* pos_eff = reinterpret_cast<int32_t*>(ws + X.pos_eff);
    int32_t* len_eff = reinterpret_cast<int32_t*>(ws + X.len_eff);
    TickRingsArgs ra;
    ra.unit_ring = uring; ra.unit_new = unit_new; ra.noise_ring = nring; ra.noise_new = noise_new;
    ra.B = B; ra.UC = P.cfg.unit_channels; ra.NC = P.cfg.inter_channels; ra.W = G.W; ra.hop = G.hop;
    ra.n_new = n_new; ra.pos = pos; ra.lens = lens; ra.pos_eff = pos_eff; ra.len_eff = len_eff;
    ok(be.tick_rings(ra));
    size_t wave_rows = 0, first = 0;
    ok(live_window(P, G, X.live, blob, ws, uring, g, nring, B, pos_eff, len_eff, be, rng, trim, wave_rows, first));
    TickDeliverArgs da;
    da.wave = reinterpret_cast<const float*>(ws + X.live.wave); da.out = out;
    da.B = B; da.rows = (int32_t)wave_rows; da.first = (int32_t)first; da.hop = G.hop; da.spf = samples_per_frame(P);
    da.n_new = n_new; da.pos = pos;
    ok(be.tick_deliver(da));
    return st;
  } else {
    return QVC_ERR_BAD_CONFIG;
  }
}

}  // namespace qvc
