// qvc_path.h -- the launch sequence of the hot path, written once and parameterised on a backend.
//
// Backend = what "launch" means: the product's HipBackend (qvc_api.hip) enqueues gfx950 kernels
// on a stream; the test-only host emulation under oracle/ replays the very same sequence on the
// CPU from the same packed blob, which lets the orchestration (buffers, strides, flip folding,
// fused epilogues) be checked against the oracle without a GPU.  The product never links the
// emulation.
//
// A backend provides:  int conv(const ConvDesc&, const ConvArgs&, int batch, int epi, int dtype);
//                      int pair3(const ConvDesc* d1, const ConvDesc* d2, const PairArgs3&, int batch, int dtype);
//                      bool chain_ok(const ConvDesc* d1, const ConvDesc* d2, int n);
//                      int chain(const ConvDesc* d1, const ConvDesc* d2, const ChainArgs&, int batch, int dtype);
//                      int wn(const ConvDesc& in, const ConvDesc& rs, const WnArgs&, int batch, int dtype);
//                      int wn_stack_chunk(int layers);   (layers per whole-stack launch, 0 = one launch per layer)
//                      int wn_stack(const ConvDesc& in, const ConvDesc& rs, const ConvDesc& rs_last, const WnStackArgs&,
//                                   int batch, int dtype, const ConvDesc* pre, const ConvDesc* post);
//                      int gemv(const GemvArgs&); int sample(const SampleArgs&); int zero(void* ptr, size_t bytes);
//                      int tail(const TailArgs&); bool post_tail_ok(const ConvDesc&);
//                      int post_tail(const ConvDesc&, const PostTailArgs&, int batch, int dtype);
//                      optional:  static constexpr bool kSingleBandTail = true -- tail (TailArgs::bands == 1) and
//                      post_tail (post_tail_bands(d) == 1) run the single-band decoder (QVC_DEC_ISTFT).  A backend that
//                      does not say so gets QVC_ERR_BAD_CONFIG from the path for that decoder
//                      optional:  static constexpr bool kFanout = true  with  int sample_rows(const SampleRowsArgs&);
//                      and conv(..., EPI_STATS, ...) -- the fan-out form of the path (Path::infer_fanout).  A backend
//                      that does not say so gets QVC_ERR_BAD_CONFIG from it
//                      optional:  static constexpr bool kNoiseRng = true -- conv(..., EPI_SAMPLE, ...), sample and
//                      sample_rows honour ConvArgs::rng / SampleArgs::rng / SampleRowsArgs::rng when the noise pointer
//                      is null (Path::rng: the draw computed where it is consumed).  A backend that does not say so
//                      gets QVC_ERR_BAD_CONFIG from the path in that mode
//                      void fork(int n); void branch(int j); void branch_done(int j); void join(int n);
//                      (stream fork/join; no-ops on one stream)
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <type_traits>
#include "qvc_select.h"

namespace qvc {

// Backend::kSingleBandTail, false for a backend that does not state it (one written before the single-band decoder
// existed keeps building and refuses that decoder instead of running the four-band tail).
template <class B, class = void> constexpr bool single_band_tail = false;
template <class B> constexpr bool single_band_tail<B, std::void_t<decltype(B::kSingleBandTail)>> = B::kSingleBandTail;

// Backend::kFanout, false for a backend that does not state it (it then needs neither sample_rows nor EPI_STATS).
template <class B, class = void> constexpr bool fanout_backend = false;
template <class B> constexpr bool fanout_backend<B, std::void_t<decltype(B::kFanout)>> = B::kFanout;

// Backend::kNoiseRng, false for a backend that does not state it (it never sees a launch without its noise tensor).
template <class B, class = void> constexpr bool noise_rng_backend = false;
template <class B> constexpr bool noise_rng_backend<B, std::void_t<decltype(B::kNoiseRng)>> = B::kNoiseRng;

// Kinds of the steps a Path issues (one per backend call that enqueues device work), in the order they are counted.
// (A single-band launch is counted as STEP_POST_TAIL1 / STEP_TAIL1: the same backend calls, told apart for the tests.)
enum StepKind : int32_t {
  STEP_CONV = 0, STEP_ZERO, STEP_GEMV, STEP_SAMPLE, STEP_WN, STEP_WN_STACK, STEP_CHAIN, STEP_PAIR3, STEP_POST_TAIL,
  STEP_POST_TAIL1, STEP_TAIL, STEP_TAIL1, STEP_SAMPLE_ROWS, STEP_KINDS
};

template <class Backend>
struct Path {
  const Plan& P;
  const char* blob;
  char* ws;
  Workspace W;
  int B, T;
  Backend& be;
  int status = QVC_OK;
  // ragged batches / streaming windows (see Ragged): per-utterance sequence lengths, and -- for a window that is not
  // the whole sequence -- the absolute unit frame `pos[b]` that sits at buffer row `off`
  const int32_t* lens = nullptr;
  const int32_t* pos = nullptr;
  int32_t off = 0;
  Ragged rg(int mul, int add = 0) const { Ragged r; r.lens = lens; r.pos = pos; r.mul = mul; r.add = add; r.off = off; return r; }
  // unit frames as they are on disk (dataset/encode.py:38: (frames, 256) per utterance), i.e. [B][T][unit_channels],
  // instead of the reference's in-memory (B, 256, T) (data_utils_new_new.py:121-122 transposes after loading)
  bool unit_fm = false;
  // streaming: stage-0 ResBlock outputs handed over from a previous window instead of this call's own (dec_back)
  const void* s0_override[3] = {nullptr, nullptr, nullptr};
  // the WaveNet stacks may run in the continuous-stream kernel's 64-frame tile (choose_wn_stack picks it where the grid
  // is large); the streaming windows keep the 32-frame tile, not measured there
  bool wn_wide = true;
  // the N(0,1) draw of models.py:94 computed at its draw site (NoiseRng) -- used where a call passes noise == nullptr
  NoiseRng rng;
  // which source of the draw a call with this `noise` pointer uses; false (and status set) if there is none
  bool draw_ok(const float* noise) {
    if (noise) return true;
    if (!rng.keys) status = QVC_ERR_BAD_ARG;
    else if (!noise_rng_backend<Backend>) status = QVC_ERR_BAD_CONFIG;
    return status == QVC_OK;
  }
  // Step window (tests): every backend call that enqueues device work is one step, numbered from 0 in issue order.
  // Steps outside [step_lo, step_hi) are counted but not issued; nothing else the path does changes.  The whole-path
  // state lives in the workspace and the output buffers, so a run can be stopped after any step and resumed from a
  // copy of those buffers (the GPU test replays each launch on the host emulation from such a snapshot).
  int step_n = 0, step_lo = 0, step_hi = INT_MAX;
  int32_t* step_kinds = nullptr; int max_step_kinds = 0;   // optional: the kind of every counted step
  bool step(StepKind k) {
    const int s = step_n++;
    if (step_kinds && s < max_step_kinds) step_kinds[s] = k;
    return s >= step_lo && s < step_hi;
  }

  template <typename U> U* wsp(int64_t off) const { return reinterpret_cast<U*>(ws + off); }
  int dtype_wn() const { return wn_dtype(P.cfg); }     // enc_p / enc_q / flow
  int dtype_dec() const { return dec_dtype(P.cfg); }   // generator convs
  int dtype_pair() const { return pair_dtype(P.cfg); } // fused ResBlock pairs (may differ: QVC_BF16X)

  ConvArgs args(const ConvDesc& d, const char* wb = nullptr) const {
    ConvArgs a;
    if (!wb) wb = blob;
    a.w = wb + d.w_off;
    a.bias = d.b_off >= 0 ? reinterpret_cast<const float*>(wb + d.b_off) : nullptr;
    conv_geometry(a, d);
    return a;
  }
  // ---- what a conv launch is told about its tensors, stated once (static: the speaker paths below use them too)
  // it reads fp32 frame-major rows, `t` per batch member, of C channels each -- all of them from channel c0 on
  static void in_f32_frames(ConvArgs& a, const float* x, int t, int C, int c0 = 0) { a.x = x; a.x_kind = XK_F32_FM; a.x_bs = (int64_t)t * C; a.x_ts = C; a.x_c0 = c0; a.T_in = t; }
  // it reads frame-major rows in the operand type
  static void in_op_frames(ConvArgs& a, const void* x, int t, int C) { a.x = x; a.x_kind = XK_OP_FM; a.x_bs = (int64_t)t * C; a.x_ts = C; a.T_in = t; }
  // its output is as long as its input, and member b's rows end where `r` says
  static void out_same_length(ConvArgs& a, int t, const Ragged& r) { a.Nq = t; a.T_out = t; a.rg = r; }
  // it writes fp32 frame-major rows of C channels, its own from channel c0 on
  static void out_f32_frames(ConvArgs& a, float* y, int t, int C, int c0 = 0) { a.y32 = y; a.y32_bs = (int64_t)t * C; a.y32_ts = C; a.y32_c0 = c0; }
  // it writes frame-major rows in the operand type, through a leaky ReLU of `slope` (1: as they are)
  static void out_op_frames(ConvArgs& a, void* y, int t, int C, float slope) { a.y16 = y; a.y16_bs = (int64_t)t * C; a.y16_ts = C; a.slope_out = slope; }

  void conv(const ConvDesc& d, const ConvArgs& a, int dt, int epi = EPI_STD) {
    if (status != QVC_OK) return;
    const ConvDesc g = generic_layout(d);
    ConvArgs ga = a; ga.nchunk = g.nchunk;
    if (step(STEP_CONV)) status = be.conv(g, ga, B, epi, dt);
  }
  void zero(int64_t off, int64_t bytes) {
    if (status != QVC_OK) return;
    if (step(STEP_ZERO)) status = be.zero(ws + off, (size_t)bytes);
  }

  // ---- conditioning table: bb[b][row] for every cond row (flow WN layers + dec.cond; enc_q: its WN layers, own blob)
  void cond_table(const float* g) { cond_table(blob, P.cond_w_off, P.cond_b_off, P.cond_rows, g); }
  void cond_table(const char* wb, int64_t w_off, int64_t b_off, int rows, const float* g) {
    if (status != QVC_OK) return;
    GemvArgs ga{reinterpret_cast<const float*>(wb + w_off), reinterpret_cast<const float*>(wb + b_off),
                g, wsp<float>(W.bb), rows, P.cfg.gin_channels, B};
    if (step(STEP_GEMV)) status = be.gemv(ga);
  }

  // ---- the whole conversion path: unit frames, speaker embedding, noise -> waveform (every backend's whole-path
  // entry points call this, so they issue the same steps)
  void infer(const float* unit, const float* g, const float* noise, float* out) {
    cond_table(g);
    enc_p(unit, noise, wsp<float>(W.z));
    flow(wsp<float>(W.z));
    dec_trunk_wave(wsp<float>(W.z), wsp<float>(W.post), out);
  }

  // ---- the same path for R = B output rows that come from U <= R distinct sources (any-to-many conversion: one source
  // listed once per target speaker).  Nothing ahead of the draw z_p = mu + eps * exp(log sigma) depends on the speaker
  // (models.py:638-640: only flow and dec see g), so enc_p runs once per SOURCE, as far as the projection's statistics,
  // and a row-sampling step draws every row from its source's statistics with its own noise.  The two halves differ in
  // batch and lengths only: B and lens are switched in between.
  //   unit (U, ...) / frames [U]: the sources;  src [R]: the source of every row (device; clamped to [0, U-1] there);
  //   g (R, gin), noise (R, C, T), out (R, ...): per row;  row_frames [R]: scratch, receives frames[src[r]]
  void infer_fanout(const float* unit, const int32_t* frames, const int32_t* src, int U, const float* g, const float* noise,
                    float* out, int32_t* row_frames) {
    if constexpr (fanout_backend<Backend>) {
      const int R = B;
      if (U < 1 || U > R) { status = QVC_ERR_BAD_ARG; return; }
      if (!draw_ok(noise)) return;
      cond_table(g);                                 // R rows of conditioning
      B = U; lens = frames;
      enc(P.enc_pre, P.enc_wn, P.enc_proj, blob, unit, P.cfg.unit_channels, unit_fm,
          reinterpret_cast<const float*>(blob + P.enc_wn.inbias_off), 0, nullptr, nullptr);   // -> W.stats, rows 0 .. U-1
      B = R;
      if (status != QVC_OK) return;
      SampleRowsArgs sa{wsp<float>(W.stats), noise, wsp<float>(W.z), src, frames, row_frames, U, R, T, P.cfg.inter_channels};
      if (!noise) sa.rng = rng;
      if (step(STEP_SAMPLE_ROWS)) status = be.sample_rows(sa);
      lens = row_frames;
      flow(wsp<float>(W.z));
      dec_trunk_wave(wsp<float>(W.z), wsp<float>(W.post), out);
    } else {
      status = QVC_ERR_BAD_CONFIG;
    }
  }

  // ---- layers [l0, l0 + n) of `wn`, weights in blob `wb`, as ONE stack launch: the part every such launch shares --
  // weights, geometry, mask and tile
  WnStackArgs stack_args(const WNPlan& wn, const char* wb, int l0, int n) const {
    const ConvDesc& din = wn.in_conv[0];
    WnStackArgs a;
    a.bs = (int64_t)T * P.cfg.hidden_channels; a.T = T; a.H = P.cfg.hidden_channels; a.HP = din.CinP;
    for (int l = 0; l < n; ++l) {
      a.w_in[l] = wb + wn.in_conv[l0 + l].w_off; a.w_rs[l] = wb + wn.rs_conv[l0 + l].w_off;
      a.b_rs[l] = reinterpret_cast<const float*>(wb + wn.rs_conv[l0 + l].b_off);
    }
    a.layers = n; a.taps = din.taps; a.KS = din.KS(); a.nIt1 = din.nIt();
    a.rg = rg(1); a.wide = wn_wide ? 1 : 0;
    return a;
  }
  // ---- WN stack over xw (in place) accumulating into oacc (modules.py:69-114)
  // bb: conditioning rows for layer 0 (+ l*2H per layer), bb_bs: batch stride (0 = shared)
  void wn(const WNPlan& wn, const float* bb, int64_t bb_bs, const char* wb = nullptr) {
    if (!wb) wb = blob;
    const int H = P.cfg.hidden_channels;
    const int64_t bs = (int64_t)T * H;
    // Whole-stack kernel, in launches of `chunk` layers: fewer layers per launch = less halo to recompute
    // (4 layers: 48-frame window for 32 output frames; 16 layers: 96), more launches = more x round trips.
    const int chunk = be.wn_stack_chunk(wn.layers);
    if (chunk > 0 && wn.layers % chunk == 0 && wn_stack_ok(wn.in_conv[0], chunk)) {
      for (int l0 = 0; l0 < wn.layers; l0 += chunk) {
        const int part = l0 / chunk;
        WnStackArgs a = stack_args(wn, wb, l0, chunk);
        a.x0 = wsp<float>(part % 2 == 0 ? W.xw : W.xw2); a.out = wsp<float>(W.oacc);
        a.bbias = bb + (int64_t)l0 * 2 * H; a.bbias_bs = bb_bs;
        a.final_layer = l0 + chunk == wn.layers ? 1 : 0; a.accum = l0 > 0 ? 1 : 0;
        a.x_out = a.final_layer ? nullptr : wsp<float>(part % 2 == 0 ? W.xw2 : W.xw);
        if (status == QVC_OK && step(STEP_WN_STACK)) status = be.wn_stack(wn.in_conv[0], wn.rs_conv[0], wn.rs_conv[wn.layers - 1], a, B, dtype_wn(), nullptr, nullptr);
      }
      return;
    }
    zero(W.oacc, (int64_t)B * bs * 4);
    for (int l = 0; l < wn.layers; ++l) {
      const ConvDesc& din = wn.in_conv[l];
      const ConvDesc& drs = wn.rs_conv[l];
      WnArgs a;
      a.x_in = wsp<float>(l % 2 == 0 ? W.xw : W.xw2);
      a.x_out = wsp<float>(l % 2 == 0 ? W.xw2 : W.xw);
      a.oacc = wsp<float>(W.oacc);
      a.bs = bs; a.T = T; a.H = H; a.HP = din.CinP;
      a.w_in = wb + din.w_off; a.w_rs = wb + drs.w_off;
      a.b_rs = reinterpret_cast<const float*>(wb + drs.b_off);
      a.bbias = bb + (int64_t)l * 2 * H; a.bbias_bs = bb_bs;
      a.taps = din.taps; a.KS = din.KS(); a.nIt1 = din.nIt(); a.last = l == wn.layers - 1 ? 1 : 0;
      a.rg = rg(1);
      if (status == QVC_OK && step(STEP_WN)) status = be.wn(din, drs, a, B, dtype_wn());
    }
  }

  // ---- enc_p (models.py:75-95) and enc_q (the same with cond = g, :582,617; own plan and blob): x, noise -> z.
  // x: Cx channels, frame- or channel-major; wb: the blob the three descriptors point into; bb / bb_bs: see wn.
  // z_out == nullptr: stop at the projection and leave its statistics, fp32 [mu + b | log sigma + b] per frame, in
  // W.stats (paired rows: EPI_STATS instead of the sampling epilogue; natural rows: the conv below as it is)
  void enc(const ConvDesc& pre, const WNPlan& w, const ConvDesc& proj, const char* wb, const float* x, int Cx, bool x_fm,
           const float* bb, int64_t bb_bs, const float* noise, float* z_out) {
    const int H = P.cfg.hidden_channels, C = P.cfg.inter_channels;
    if (z_out && !draw_ok(noise)) return;
    {
      ConvArgs a = args(pre, wb);
      if (x_fm) in_f32_frames(a, x, T, Cx);
      else { a.x = x; a.x_kind = XK_F32_CM; a.x_bs = (int64_t)Cx * T; a.x_ts = T; a.T_in = T; }   // the reference's (B, C, T)
      out_same_length(a, T, rg(1));
      out_f32_frames(a, wsp<float>(W.xw), T, H);
      conv(pre, a, dtype_wn());
    }
    wn(w, bb, bb_bs, wb);
    {
      ConvArgs a = args(proj, wb);
      in_f32_frames(a, wsp<float>(W.oacc), T, H);
      out_same_length(a, T, rg(1));
      if (z_out && proj_and_sample(proj, a, noise, z_out)) return;
      out_f32_frames(a, wsp<float>(W.stats), T, 2 * C);
      if (!z_out && proj.gau) a.gau_H = C;
      conv(proj, a, dtype_wn(), !z_out && proj.gau ? EPI_STATS : EPI_STD);
    }
    if (status != QVC_OK || !z_out) return;
    SampleArgs sa{wsp<float>(W.stats), noise, z_out, B, T, C};
    if (!noise) { sa.rng = rng; sa.pos = pos; sa.off = off; }
    if (step(STEP_SAMPLE)) status = be.sample(sa);
  }
  void enc_p(const float* unit, const float* noise, float* z_out) {
    enc(P.enc_pre, P.enc_wn, P.enc_proj, blob, unit, P.cfg.unit_channels, unit_fm,
        reinterpret_cast<const float*>(blob + P.enc_wn.inbias_off), 0, noise, z_out);
  }
  // the conditioning GEMV (cond_layer on g + in_layer biases: enc_q's own table) comes first
  void enc_q(const EncQPlan& Q, const char* qblob, const float* spec, const float* g, const float* noise, float* z_out) {
    cond_table(qblob, Q.cond_w_off, Q.cond_b_off, Q.cond_rows, g);
    enc(Q.pre, Q.wn, Q.proj, qblob, spec, Q.spec_channels, false, wsp<float>(W.bb), Q.cond_rows, noise, z_out);
  }
  // proj packed with paired [mu | log sigma] rows (make_proj): z = mu + noise * exp(log sigma) in the conv epilogue
  bool proj_and_sample(const ConvDesc& d, ConvArgs& a, const float* noise, float* z_out) {
    if (!d.gau) return false;
    const int C = P.cfg.inter_channels;
    a.gau_H = C; a.noise = noise; a.noise_bs = (int64_t)C * T; a.noise_ts = T;
    if (!noise) a.rng = rng;
    out_f32_frames(a, z_out, T, C);
    conv(d, a, dtype_wn(), EPI_SAMPLE);
    return true;
  }

  // ---- flow (models.py:39-51, modules.py:199-224); z updated in place.  reverse (the conversion path): the plan's
  // steps in order, x1 <- x1 - m.  forward (the posterior direction, models.py:618): the same steps in the opposite
  // order, x1 <- m + x1 -- every coupling layer sees the same channel flip in both directions (layer l is preceded by
  // l flips going forward and by n-l going back, n even), so the flip-folded pre / post weights serve both.
  void flow(float* z, bool forward = false) {
    const float sign = forward ? 1.f : -1.f;
    const size_t n = P.flow.size();
    for (size_t s = 0; s < n; ++s) flow_step(P.flow[forward ? n - 1 - s : s], z, sign);
  }
  void flow_step(const FlowStepPlan& f, float* z, float sign) {
    const int H = P.cfg.hidden_channels, C = P.cfg.inter_channels;
    const float* bb = wsp<float>(W.bb) + f.cond_row0;
    const ConvDesc& din = f.wn.in_conv[0];
    if (f.wn.layers == be.wn_stack_chunk(f.wn.layers) && wn_fuse_ok(din, f.pre, f.post, f.wn.layers)) {
      // the whole coupling layer in ONE launch: pre 1x1 -> 4 WaveNet layers -> post 1x1 -> x1 -= m
      WnStackArgs a = stack_args(f.wn, blob, 0, f.wn.layers);
      a.bbias = bb; a.bbias_bs = P.cond_rows;
      a.w_pre = blob + f.pre.w_off; a.b_pre = reinterpret_cast<const float*>(blob + f.pre.b_off);
      a.pre_cin = f.pre.Cin; a.pre_c0 = f.in_c0; a.pre_KS = f.pre.KS();
      a.w_post = blob + f.post.w_off; a.b_post = reinterpret_cast<const float*>(blob + f.post.b_off);
      a.post_m = f.post.M; a.post_c0 = f.out_c0; a.post_mf = f.post.MF;
      a.z = z; a.z_bs = (int64_t)T * C; a.z_ts = C; a.post_sign = sign;
      if (status == QVC_OK && step(STEP_WN_STACK))
        status = be.wn_stack(din, f.wn.rs_conv[0], f.wn.rs_conv[f.wn.layers - 1], a, B, dtype_wn(), &f.pre, &f.post);
      return;
    }
    {
      ConvArgs a = args(f.pre);
      in_f32_frames(a, z, T, C, f.in_c0);
      out_same_length(a, T, rg(1));
      out_f32_frames(a, wsp<float>(W.xw), T, H);
      conv(f.pre, a, dtype_wn());
    }
    wn(f.wn, bb, P.cond_rows);
    {   // x1 <- x1 -/+ post(h)   (modules.py:214-217)
      ConvArgs a = args(f.post);
      in_f32_frames(a, wsp<float>(W.oacc), T, H);
      out_same_length(a, T, rg(1));
      a.res = z; a.res_bs = (int64_t)T * C; a.res_ts = C; a.res_c0 = f.out_c0; a.res_sign = sign;
      out_f32_frames(a, z, T, C, f.out_c0);
      conv(f.post, a, dtype_wn());
    }
  }

  // ---- generator trunk (models.py:372-390).  dec_front = conv_pre + stage 0 (its three ResBlock outputs end up in
  // W.ra[0][j]); dec_back = the remaining stages + conv_post, reading stage 0's outputs (or s0_override: streaming).
  void dec_trunk(const float* z, float* post_out) { dec_part(z, post_out, 0, (int)P.stages.size(), true, true); }
  void dec_front(const float* z) { dec_part(z, nullptr, 0, 1, true, false); }
  void dec_back(float* post_out) { dec_part(nullptr, post_out, 1, (int)P.stages.size(), false, true); }
  // ... all the way to the waveform: conv_post and the tail as ONE launch where the backend has it (the post-conv
  // frames then never reach `post_buf`), else conv_post -> post_buf -> tail
  void dec_trunk_wave(const float* z, float* post_buf, float* wave) { dec_part(z, post_buf, 0, (int)P.stages.size(), true, true, wave); }
  void dec_back_wave(float* post_buf, float* wave) { dec_part(nullptr, post_buf, 1, (int)P.stages.size(), false, true, wave); }
  bool single_band() const { return P.cfg.decoder == QVC_DEC_ISTFT; }
  void dec_part(const float* z, float* post_out, int stage_lo, int stage_hi, bool with_pre, bool with_post, float* wave = nullptr) {
    if (wave && single_band() && !single_band_tail<Backend>) status = QVC_ERR_BAD_CONFIG;
    if (with_pre) dec_conv_pre(z);
    for (int i = stage_lo; i < stage_hi; ++i) {
      const Stage g = stage(i);
      dec_upsample(i, g);
      dec_resblocks(i, g);
    }
    if (with_post) dec_conv_post(post_out, wave);
  }

  // Stage i of the generator: t_in rows of ch_in channels in, t_out rows of ch channels out, `rate` rows per unit frame
  // at its OUTPUT, where its ResBlocks work (its up-sampler reads at rate / up_s).  The one place that knows the
  // geometry, for the stages a call runs and the ones it skips alike.
  struct Stage { int t_in, ch_in, t_out, ch, rate; };
  Stage stage(int i) const {
    Stage g{0, 0, T, P.cfg.upsample_initial_channel, 1};         // conv_pre's output
    for (int k = 0; k <= i; ++k) {
      const ConvDesc& up = P.stages[(size_t)k].up;
      g.t_in = g.t_out; g.ch_in = g.ch;
      g.t_out = (g.t_in - 1) * up.up_s - 2 * up.up_p + P.cfg.upsample_kernel_sizes[k] + up_output_padding(P.cfg, k);   // models.py:335 / :124-127
      g.ch = P.stages[(size_t)k].ch; g.rate *= up.up_s;
    }
    return g;
  }
  // input = MRF mean of stage i's ResBlock outputs (each ResBlock's final tensor sits in its `ra` buffer), t rows of C
  void mean_input(ConvArgs& a, int i, int t, int C) {
    const int NB = P.cfg.n_resblocks;
    auto src = [&](int j) -> const void* { return (i == 0 && s0_override[j]) ? s0_override[j] : wsp<void>(W.ra[(size_t)i][(size_t)j]); };
    in_op_frames(a, src(0), t, C);
    a.x2 = src(NB > 1 ? 1 : 0);
    a.x3 = src(NB > 2 ? 2 : 0);
  }
  // conv_pre(k7) + cond(g), then the first stage's leaky ReLU fused into the store
  void dec_conv_pre(const float* z) {
    ConvArgs a = args(P.conv_pre);
    in_f32_frames(a, z, T, P.cfg.inter_channels);
    out_same_length(a, T, rg(1));
    a.bbias = wsp<float>(W.bb) + P.dec_cond_row0; a.bbias_bs = P.cond_rows;
    out_op_frames(a, wsp<void>(W.c0), T, P.cfg.upsample_initial_channel, 0.1f);
    conv(P.conv_pre, a, dtype_dec());
  }
  // lrelu(0.1) -> ConvTranspose1d as `up_s` polyphase filters; the output raw, in the operand type
  void dec_upsample(int i, const Stage& g) {
    const ConvDesc& up = P.stages[(size_t)i].up;
    ConvArgs a = args(up);
    if (i == 0) in_op_frames(a, wsp<void>(W.c0), g.t_in, g.ch_in);
    else { mean_input(a, i - 1, g.t_in, g.ch_in); a.slope_in = 0.1f; }
    a.Nq = (g.t_out - 1 + up.up_p) / up.up_s + 1; a.T_out = g.t_out; a.rg = rg(g.rate / up.up_s);
    out_op_frames(a, wsp<void>(W.u[(size_t)i]), g.t_out, g.ch, 1.f);
    conv(up, a, dtype_dec());
  }
  // lrelu(0.01) -> ReflectionPad1d((1,0)) -> subband_conv_post(k7) / conv_post (single band), then the tail if `wave`
  void dec_conv_post(float* post_out, float* wave) {
    const int last = (int)P.stages.size() - 1;
    const Stage g = stage(last);
    const int F = g.t_out + 1;
    ConvArgs a = args(P.conv_post);
    mean_input(a, last, g.t_out, g.ch);
    a.slope_in = 0.01f; a.reflect = 1;
    a.Nq = F; a.T_out = F; a.rg = rg(g.rate);
    if (wave && be.post_tail_ok(P.conv_post)) {
      if (status != QVC_OK) return;
      PostTailArgs pt;
      pt.c = a; pt.fir = single_band() ? nullptr : reinterpret_cast<const float*>(blob + P.fir_off); pt.out = wave; pt.F = F;
      pt.rg = rg(P.total_up, 1);
      if (step(single_band() ? STEP_POST_TAIL1 : STEP_POST_TAIL)) status = be.post_tail(P.conv_post, pt, B, dtype_dec());
      return;
    }
    out_f32_frames(a, post_out, F, P.post_channels);
    conv(P.conv_post, a, dtype_dec());
    if (wave) tail(post_out, wave, nullptr, F);
  }

  // ---- the ResBlocks of stage i.  They are independent until their mean.  Pair q of all three chains goes out as ONE
  // launch (workgroups of chains with different kernel sizes interleave on the CUs, see rbpair_kernel); a stage whose
  // pairs cannot run fused falls back to one launch per conv, optionally on parallel branches (streams).
  // Stream of ResBlock j: u -> ra -> rb -> ra; src[j] is what it reads next.  The MRF mean of the three final tensors is
  // taken by the consumer (next up-sampler / conv_post) while it stages its input, so nothing is accumulated here.
  using Streams = const void* [QVC_MAX_RESBLOCKS];
  void dec_resblocks(int i, const Stage& g) {
    Streams src;
    bool chained[QVC_MAX_RESBLOCKS] = {};
    for (const void*& s : src) s = wsp<void>(W.u[(size_t)i]);
    if (!pairs_fusable(P.cfg, P.stages[(size_t)i])) return resblocks_unfused(i, g, src);
    const PairLaunch shape = pair_launch(P.stages[(size_t)i], g);
    if (!shape.few_tiles) resblocks_chained(i, g, src, chained);
    resblocks_fused(i, g, shape, chained, src);
  }
  void* pair_dst(int i, int j, int q) const { return wsp<void>(q == 1 ? W.rb[(size_t)i][(size_t)j] : W.ra[(size_t)i][(size_t)j]); }
  PairArgs pair_args(int i, const Stage& g, int j, int q, const void* x, void* dst) const {
    const ConvDesc& d1 = P.stages[(size_t)i].c1[(size_t)j * 3 + q];
    const ConvDesc& d2 = P.stages[(size_t)i].c2[(size_t)j * 3 + q];
    PairArgs pa;
    pa.x = x; pa.bs = (int64_t)g.t_out * g.ch; pa.T = g.t_out; pa.C = g.ch; pa.CP = d1.CinP;
    pa.w1 = blob + d1.w_off; pa.b1 = reinterpret_cast<const float*>(blob + d1.b_off);
    pa.w2 = blob + d2.w_off; pa.b2 = reinterpret_cast<const float*>(blob + d2.b_off);
    pa.k = d1.taps; pa.dil = d1.dil; pa.KS = d1.KS(); pa.nIt = d1.nIt(); pa.slope = 0.1f;
    pa.y = dst;
    return pa;
  }
  // The shape of the fused launches.  One launch for the three chains, chain-major grid (blockIdx.z = chain, longest
  // kernel first): the dispatcher hands out all workgroups of the k 11 chain first and the shorter chains backfill the
  // CUs as they free up -- longest-processing-time-first, so the launch ends on short workgroups.  Interleaving the
  // chains on the CUs (x % n) left long workgroups for the end: with one 8-wave workgroup per CU (stage 1) 261 us against
  // 226 us for three launches and 199 us chain-major; with two 4-wave workgroups per CU (stage 2) chain-major takes
  // another 45 us off the step (2.11 -> 2.065 ms, same box, alternating runs).  Tiny batches (40-80 workgroups per
  // chain) interleave: everything runs at once, in the time of the longest chain (batch 1: 3 x 43 us instead of
  // 3 x (19 + 31 + 43) us).
  // per_launch: all the chains, or 1 (one chain per launch); chain_major 0: 4-wave layouts interleave the chains (x % n)
  struct PairLaunch { bool few_tiles; int per_launch, chain_major; };
  PairLaunch pair_launch(const StagePlan& st, const Stage& g) const {
    const int NB = P.cfg.n_resblocks;
    const bool few_tiles = (int64_t)B * g.t_out * NB <= 256 * 32;
    const bool wide = block_waves(st.c1[0]) != kWaves;
    return {few_tiles, (!wide || few_tiles || debug_get(DBG_PAIR_WIDE_LAUNCH)) ? NB : 1, ((wide || debug_get(DBG_PAIR_CM4)) && !few_tiles) ? 1 : 0};
  }
  // A ResBlock with a short kernel (k 3: 12 frames of receptive field per side) runs as ONE launch, its three pairs
  // chained on chip (qvc_chain_impl.h): its stream is read once and written once instead of three times each.  The
  // other chains keep the pair-by-pair launches.  (Not for tiny batches: everything in the time of the longest chain is
  // better, see pair_launch.)
  void resblocks_chained(int i, const Stage& g, Streams& src, bool* chained) {
    const StagePlan& st = P.stages[(size_t)i];
    for (int j = 0; j < P.cfg.n_resblocks; ++j) {
      ConvDesc d1s[3], d2s[3];
      for (int q = 0; q < 3; ++q) { d1s[q] = st.c1[(size_t)j * 3 + q]; d2s[q] = st.c2[(size_t)j * 3 + q]; }
      if (!be.chain_ok(d1s, d2s, 3)) continue;
      ChainArgs ca; ca.n = 3; ca.rg = rg(g.rate);
      for (int q = 0; q < 3; ++q) {
        ca.p[q] = pair_args(i, g, j, q, src[j], pair_dst(i, j, q));
        src[j] = ca.p[q].y;
      }
      if (status == QVC_OK && step(STEP_CHAIN)) status = be.chain(d1s, d2s, ca, B, dtype_pair());
      chained[j] = true;
    }
  }
  // Pair q of the ResBlocks that are not chained, `shape.per_launch` of them per launch
  void resblocks_fused(int i, const Stage& g, const PairLaunch& shape, const bool* chained, Streams& src) {
    const StagePlan& st = P.stages[(size_t)i];
    int rest[QVC_MAX_RESBLOCKS], n_rest = 0;
    for (int j = 0; j < P.cfg.n_resblocks; ++j) if (!chained[j]) rest[n_rest++] = j;
    if (n_rest == 0) return;
    const int n = std::min(shape.per_launch, n_rest);
    for (int q = 0; q < 3; ++q) for (int j0 = 0; j0 < n_rest; j0 += n) {
      PairArgs3 a3; a3.n = n; a3.rg = rg(g.rate); a3.chain_major = n > 1 ? shape.chain_major : 0;
      ConvDesc d1s[3], d2s[3];
      // the chain with the largest kernel first: its workgroups are the longest, so they should start earliest
      int order[3] = {0, 0, 0};
      for (int s = 0; s < n; ++s) order[s] = rest[j0 + s];
      std::sort(order, order + n, [&](int x, int y) { return st.c1[(size_t)x * 3 + q].nIt() > st.c1[(size_t)y * 3 + q].nIt(); });
      for (int s = 0; s < n; ++s) {
        const int j = order[s];
        a3.p[s] = pair_args(i, g, j, q, src[j], pair_dst(i, j, q));
        d1s[s] = st.c1[(size_t)j * 3 + q]; d2s[s] = st.c2[(size_t)j * 3 + q];
        src[j] = a3.p[s].y;
      }
      if (status == QVC_OK && step(STEP_PAIR3)) status = be.pair3(d1s, d2s, a3, B, dtype_pair());
    }
  }
  // One launch per pair, or per conv where a pair cannot run fused, ResBlock j on branch j
  void resblocks_unfused(int i, const Stage& g, Streams& src) {
    const StagePlan& st = P.stages[(size_t)i];
    const int NB = P.cfg.n_resblocks;
    const int64_t bs = (int64_t)g.t_out * g.ch;
    be.fork(NB);                                   // branches wait for everything enqueued so far
    for (int q = 0; q < 3; ++q)
      for (int j = 0; j < NB; ++j) {
        be.branch(j);
        const ConvDesc& d1 = st.c1[(size_t)j * 3 + q];
        const ConvDesc& d2 = st.c2[(size_t)j * 3 + q];
        void* dst = pair_dst(i, j, q);
        if (pair_supported(d1, d2) && d1.lp && d2.lp) {
          PairArgs3 a1; a1.n = 1; a1.rg = rg(g.rate);
          a1.p[0] = pair_args(i, g, j, q, src[j], dst);
          if (status == QVC_OK && step(STEP_PAIR3)) status = be.pair3(&d1, &d2, a1, B, dtype_pair());
        } else {
          void* xt = wsp<char>(W.xt[(size_t)i]) + (size_t)j * (size_t)B * (size_t)bs * 2;
          ConvArgs a = args(d1);                   // lrelu -> dilated conv -> lrelu (stored already activated)
          in_op_frames(a, src[j], g.t_out, g.ch); a.slope_in = 0.1f;
          out_same_length(a, g.t_out, rg(g.rate));
          out_op_frames(a, xt, g.t_out, g.ch, 0.1f);
          conv(d1, a, dtype_dec());
          ConvArgs a2 = args(d2);                  // conv -> + x
          in_op_frames(a2, xt, g.t_out, g.ch);
          out_same_length(a2, g.t_out, rg(g.rate));
          a2.res16 = src[j]; a2.res_bs = bs; a2.res_ts = g.ch;
          out_op_frames(a2, dst, g.t_out, g.ch, 1.f);
          conv(d2, a2, dtype_dec());
        }
        if (q == 2) be.branch_done(j);
        src[j] = dst;
      }
    be.join(NB);                                   // main stream continues when every branch is done
  }

  void tail(const float* post, float* out, float* y_mb, int F) {
    if (status == QVC_OK && single_band() && !single_band_tail<Backend>) status = QVC_ERR_BAD_CONFIG;
    if (status != QVC_OK) return;
    TailArgs ta{post, reinterpret_cast<const float*>(blob + P.fir_off), out, y_mb, B, F};
    ta.rg = rg(P.total_up, 1);
    if (single_band()) { ta.fir = nullptr; ta.bands = 1; }
    if (step(single_band() ? STEP_TAIL1 : STEP_TAIL)) status = be.tail(ta);
  }
};

// ---- speaker encoder (models.py:507-546): per layer one conv launch (input projection of all frames) and one
// persistent recurrence launch, then the embedding head.  Backend adds:  int lstm(const LstmArgs&, int KS, int dtype);
//                                                                        int spk_embed(const SpkEmbedArgs&);
// map: the partial map of a ragged batch (spk_path_ragged), null for the uniform layout.
template <class Backend>
int spk_layers(const SpkPlan& S, int dtype, const char* blob, char* ws, const SpkWorkspace& W, const float* mel, float* g,
               int U, int F, Backend& be, const SpkMapArgs* map) {
  using Conv = Path<Backend>;
  const int H = S.H, n_part = spk_partials(F), St = spk_steps(F), P = U * n_part;
  for (int l = 0; l < kSpkLayers; ++l) {
    const ConvDesc& d = S.ih[l];
    ConvArgs ca;
    ca.w = blob + d.w_off; ca.bias = reinterpret_cast<const float*>(blob + d.b_off);
    conv_geometry(ca, d);     // a 1x1 conv (make_conv(4H, Cin, 1, 1))
    Ragged valid;             // ragged: the staging masks frames past a row's (a partial's) end, the padding is never read
    if (l == 0) {     // mel (U, n_mel, F) as handed to infer() (convert.py:77); the transpose of models.py:635 is the staging
      ca.x = mel; ca.x_kind = XK_F32_CM; ca.x_bs = (int64_t)S.n_mel * F; ca.x_ts = F; ca.T_in = F;
      if (map) valid.lens = map->flen;
      Conv::out_same_length(ca, F, valid);
      Conv::out_f32_frames(ca, reinterpret_cast<float*>(ws + W.xp0), F, 4 * H);
    } else {
      Conv::in_op_frames(ca, ws + W.hseq, St, S.HP);
      if (map) valid.lens = map->psteps;
      Conv::out_same_length(ca, St, valid);
      Conv::out_f32_frames(ca, reinterpret_cast<float*>(ws + W.xp), St, 4 * H);
    }
    int rc = be.conv(d, ca, l == 0 ? U : P, EPI_STD, dtype);
    if (rc != QVC_OK) return rc;
    LstmArgs la;
    la.xp = reinterpret_cast<const float*>(ws + (l == 0 ? W.xp0 : W.xp));
    la.shared = l == 0 ? 1 : 0;
    la.F = F; la.n_part = n_part; la.S = St; la.P = P; la.H = H;
    la.w_hh = blob + S.hh_off[l];
    la.hseq = l + 1 < kSpkLayers ? ws + W.hseq : nullptr;
    la.hfin = l + 1 < kSpkLayers ? nullptr : reinterpret_cast<float*>(ws + W.hfin);
    if (map) { la.prow = map->prow; la.pstart = map->pstart; la.psteps = map->psteps; la.phdr = map->phdr; }
    rc = be.lstm(la, S.KS, dtype);
    if (rc != QVC_OK) return rc;
  }
  SpkEmbedArgs ea{reinterpret_cast<const float*>(ws + W.hfin), reinterpret_cast<const float*>(blob + S.lin_w_off),
                  reinterpret_cast<const float*>(blob + S.lin_b_off), g, U, n_part, H};
  if (map) ea.poff = map->poff;
  return be.spk_embed(ea);
}
template <class Backend>
int spk_path(const SpkPlan& S, int dtype, const char* blob, char* ws, const SpkWorkspace& W, const float* mel, float* g,
             int U, int F, Backend& be) {
  return spk_layers(S, dtype, blob, ws, W, mel, g, U, F, be, nullptr);
}

// ---- the same for a ragged batch: mel (U, n_mel, F) padded, frames[u] valid frames per row, on the device.  One
// small launch builds the partial map (SpkMapArgs); every launch after it is sized from the host-known cap
// (U * spk_partials(F) partials of spk_steps(F) steps) and takes rows, starts and step counts from the map, so no
// length is read on the host.  Backend adds:  int spk_map(const SpkMapArgs&);  W = carve_spk_ragged_workspace(S, U, F).
template <class Backend>
int spk_path_ragged(const SpkPlan& S, int dtype, const char* blob, char* ws, const SpkWorkspace& W, const float* mel,
                    const int32_t* frames, float* g, int U, int F, Backend& be) {
  auto i32 = [&](int64_t off) { return reinterpret_cast<int32_t*>(ws + off); };
  SpkMapArgs ma;
  ma.frames = frames; ma.U = U; ma.F = F; ma.P = U * spk_partials(F);
  ma.flen = i32(W.flen); ma.poff = i32(W.poff); ma.prow = i32(W.prow); ma.pstart = i32(W.pstart);
  ma.psteps = i32(W.psteps); ma.phdr = i32(W.phdr);
  const int rc = be.spk_map(ma);
  return rc != QVC_OK ? rc : spk_layers(S, dtype, blob, ws, W, mel, g, U, F, be, &ma);
}

}  // namespace qvc
