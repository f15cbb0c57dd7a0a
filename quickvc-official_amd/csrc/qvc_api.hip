// qvc_api.hip -- the C ABI of include/qvc.h: argument checks + the launch sequence of the path.
//
// Everything here is host code that only *enqueues* kernels on the caller's stream: no
// allocation, no synchronisation, no host read of device data, so a whole qvc_infer_batch
// call can be captured into a hipGraph by the caller.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#include "qvc_path.h"
#include "qvc_stream.h"
#include "qvc_pack_util.h"

namespace qvc {
int launch_fm_to_cm(const float* src, float* dst, int batch, int frames, int channels, void* stream);
#ifdef QVC_SATCOUNT
unsigned long long sat_count_conv_f16(bool reset);
unsigned long long sat_count_conv_bf16(bool reset);
unsigned long long sat_count_wn2(bool reset);
unsigned long long sat_count_spk(bool reset);
unsigned long long sat_count_chain(bool reset);
#endif
}

struct qvc_aux {
  hipStream_t streams[2];
  hipEvent_t fork, done[3];
};

namespace {
using namespace qvc;

struct HipBackend {
  static constexpr bool kSingleBandTail = true;   // the launchers pick the kernels by TailArgs::bands / post_tail_bands(conv_post)
  hipStream_t stream0, stream;                    // the caller's stream / the current branch's
  qvc_aux* aux;                                   // streams and events of the parallel ResBlock branches, or none: one stream
  bool ok = true;
  explicit HipBackend(void* s, qvc_aux* aux = nullptr) : stream0(static_cast<hipStream_t>(s)), stream(stream0), aux(aux) {}
  // Stream fork/join for the parallel ResBlock branches: branches 1 and 2 run on the auxiliary streams, branch 0 and any
  // further one on the caller's
  hipStream_t of(int j) const { return (aux && j >= 1 && j <= 2) ? aux->streams[j - 1] : stream0; }
  void fork(int n) {
    stream = stream0;
    if (!aux) return;
    if (hipEventRecord(aux->fork, stream0) != hipSuccess) ok = false;
    for (int j = 1; j < n && j <= 2; ++j) if (hipStreamWaitEvent(aux->streams[j - 1], aux->fork, 0) != hipSuccess) ok = false;
  }
  void branch(int j) { stream = of(j); }
  void branch_done(int j) { if (aux && j < 3 && hipEventRecord(aux->done[j], of(j)) != hipSuccess) ok = false; }
  void join(int n) {
    for (int j = 1; aux && j < n && j <= 2; ++j) if (hipStreamWaitEvent(stream0, aux->done[j], 0) != hipSuccess) ok = false;
    stream = stream0;
  }
  int finish() const { return ok ? QVC_OK : QVC_ERR_LAUNCH; }
  int conv(const ConvDesc& d, const ConvArgs& a, int batch, int epi, int dtype) { return launch_conv(d, a, batch, epi, dtype, stream); }
  int pair3(const ConvDesc* d1, const ConvDesc* d2, const PairArgs3& a, int batch, int dtype) { return launch_pair3(d1, d2, a, batch, dtype, stream); }
  bool chain_ok(const ConvDesc* d1, const ConvDesc* d2, int n) const { return debug_get(DBG_PAIR_CHAIN3) != 0 && chain_supported(d1, d2, n); }
  int chain(const ConvDesc* d1, const ConvDesc* d2, const ChainArgs& a, int batch, int dtype) { return launch_chain(d1, d2, a, batch, dtype, stream); }
  int wn(const ConvDesc& din, const ConvDesc&, const WnArgs& a, int batch, int dtype) { return launch_wn(din, a, batch, dtype, stream); }
  // (the stack kernel recomputes halo frames but a layer is bound by its weight stream, not by MFMA work: measured
  // no slower than one launch per layer at any batch, 16.4 vs 17.9 us per layer at batch 1 -- so it runs wherever it applies)
  int wn_stack_chunk(int layers) const { return wn_chunk(layers); }
  int wn_stack(const ConvDesc& din, const ConvDesc&, const ConvDesc&, const WnStackArgs& a, int batch, int dtype, const ConvDesc*, const ConvDesc*) { return launch_wn_stack(din, a, batch, dtype, stream); }
  int gemv(const GemvArgs& a) { return launch_gemv(a, stream); }
  int sample(const SampleArgs& a) { return launch_sample(a, stream); }
  static constexpr bool kFanout = true;           // Path::infer_fanout: EPI_STATS in launch_conv + the row-sampling launch
  int sample_rows(const SampleRowsArgs& a) { return launch_sample_rows(a, stream); }
  static constexpr bool kNoiseRng = true;         // the three draw sites compute the noise when a launch carries a NoiseRng
  int tail(const TailArgs& a) { return launch_tail(a, stream); }
  bool post_tail_ok(const ConvDesc& d) const { return debug_get(DBG_POST_TAIL) != 0 && post_tail_supported(d); }
  int post_tail(const ConvDesc& d, const PostTailArgs& a, int batch, int dtype) { return launch_post_tail(d, a, batch, dtype, stream); }
  int zero(void* p, size_t bytes) { return hipMemsetAsync(p, 0, bytes, stream) == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH; }
  int copy_batch(const CopyDesc* d, int n) { return launch_copy_batch(d, n, stream); }
  static constexpr bool kStreamTick = true;       // stream_tick, live_tick: copy_batch's job with the bytes per slot taken from device counts
  int copy_counted(const CountedHead& h, const CountedDesc* d, int n) { return launch_copy_counted(h, d, n, stream); }
  static constexpr bool kWindows = true;          // infer_windows: the table-driven gather and delivery around the window
  int window_gather(const WindowArgs& a) { return launch_window_gather(a, stream); }
  int window_deliver(const WindowArgs& a) { return launch_window_deliver(a, stream); }
};
using Ctx = Path<HipBackend>;

// Same launches, each bracketed by events on the stream (diagnostics only).  Every method: the launch, then the
// record's name -- from the launch's LaunchChoice (qvc_select.h) where a chooser picked the kernel -- and its algorithmic
// flops / bytes.
struct TimedBackend {
  static constexpr bool kSingleBandTail = true;
  void fork(int) {} void branch(int) {} void branch_done(int) {} void join(int) {}
  hipStream_t stream;
  qvc_launch_record* rec; int max_rec; int n = 0;
  std::vector<hipEvent_t> ev;
  bool ok = true;
  void mark() { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess || hipEventRecord(e, stream) != hipSuccess) ok = false; ev.push_back(e); }
  template <class F> int timed(F launch) { if (ev.empty()) mark(); const int st = launch(); mark(); return st; }
  void note(double flops, double bytes, const char* fmt, ...) {
    if (n < max_rec) {
      va_list ap; va_start(ap, fmt); std::vsnprintf(rec[n].name, sizeof(rec[n].name), fmt, ap); va_end(ap);
      rec[n].flops = flops; rec[n].bytes = bytes; rec[n].ms = 0.f;
    }
    ++n;
  }
  static const char* tn(int dtype) { return dtype == QVC_F16 ? "f16" : (dtype == QVC_BF16X ? "bf16x" : "bf16"); }
  int conv(const ConvDesc& d, const ConvArgs& a, int batch, int epi, int dtype) {
    LaunchChoice c;
    const int st = timed([&] { return launch_conv(d, a, batch, epi, dtype, stream, c); });
    // algorithmic work: a transposed conv does k MACs per (input frame, ci, co), a conv taps MACs per output
    const double macs = d.up_s > 1 ? (double)batch * a.T_in * d.Cin * d.Cout * (double)d.ksize
                                   : (double)batch * a.Nq * (double)d.M * d.taps * d.Cin;
    const double in_b = (double)batch * a.T_in * d.Cin * (a.x_kind == XK_OP_FM ? 2 : 4) * (a.x2 ? 3 : 1);
    double out_b = 0;
    const double outs = (double)batch * a.T_out * d.Cout;
    if (epi == EPI_GAU) out_b = (double)batch * a.Nq * a.gau_H * 2;
    else if (epi == EPI_SAMPLE) out_b = (double)batch * a.Nq * a.gau_H * 8;      // noise in, z out
    else {
      if (a.y32) out_b += outs * 4 * (a.y_accum ? 2 : 1);
      if (a.y16) out_b += outs * 2;
      if (a.res) out_b += outs * 4;
      if (a.res16) out_b += outs * 2;
      if (a.y32b) out_b += (double)batch * a.Nq * (d.M - a.split) * 8;
    }
    note(2.0 * macs, in_b + out_b + (double)d.w_bytes(), "conv<%s,MF%d,NF%d,WM%d,%s>", tn(dtype), d.MF, c.NF, d.WM,
         epi == EPI_GAU ? "gau" : (epi == EPI_SAMPLE ? "smp" : "std"));
    return st;
  }
  int pair3(const ConvDesc* d1, const ConvDesc* d2, const PairArgs3& a, int batch, int dtype) {
    LaunchChoice c;
    const int st = timed([&] { return launch_pair3(d1, d2, a, batch, dtype, stream, c); });
    // one kernel symbol serves 1..3 chains per launch; the record's flops / bytes are those of the whole launch
    double fl = 0, by = 0;
    for (int i = 0; i < a.n; ++i) {
      const double outs = (double)batch * a.p[i].T * a.p[i].C;
      fl += 2.0 * 2.0 * outs * a.p[i].C * a.p[i].k;
      by += outs * 2 * 2 + (double)d1[i].w_bytes() + (double)d2[i].w_bytes();   // algorithmic: the stream read once, written once (the kernel's second read of x for the residual is NOT counted: it shows up as traffic / algorithmic > 1)
    }
    note(fl, by, "rbpair<%s,MF%d,NF%d,WM%d>", tn(dtype), d1[0].MF, c.NF, d1[0].WM);
    return st;
  }
  bool chain_ok(const ConvDesc* d1, const ConvDesc* d2, int n) const { return debug_get(DBG_PAIR_CHAIN3) != 0 && chain_supported(d1, d2, n); }
  int chain(const ConvDesc* d1, const ConvDesc* d2, const ChainArgs& a, int batch, int dtype) {
    LaunchChoice c;
    const int st = timed([&] { return launch_chain(d1, d2, a, batch, dtype, stream, c); });
    const double outs = (double)batch * a.p[0].T * a.p[0].C;
    note(a.n * 2.0 * 2.0 * outs * a.p[0].C * a.p[0].k, outs * 2 * 2 + a.n * ((double)d1[0].w_bytes() + (double)d2[0].w_bytes()),
         "rbchain<%s,MF%d,NF%d,WM%d,k%d>", tn(dtype), d1[0].MF, c.NF, d1[0].WM, d1[0].taps);
    return st;
  }
  int wn(const ConvDesc& din, const ConvDesc& drs, const WnArgs& a, int batch, int dtype) {
    LaunchChoice c;
    const int st = timed([&] { return launch_wn(din, a, batch, dtype, stream, c); });
    const double cols = (double)batch * a.T;
    note(2.0 * cols * a.H * (2.0 * a.H * a.taps + (double)drs.M), cols * a.H * 4 * (a.last ? 3 : 5) + (double)din.w_bytes() + (double)drs.w_bytes(),
         "wn_layer<%s,W%d,NF%d%s>", tn(dtype), din.WM, c.NF, a.last ? ",last" : "");
    return st;
  }
  int wn_stack_chunk(int layers) const { return wn_chunk(layers); }
  int wn_stack(const ConvDesc& din, const ConvDesc& drs, const ConvDesc& drs_last, const WnStackArgs& a, int batch, int dtype,
               const ConvDesc* dpre, const ConvDesc* dpost) {
    LaunchChoice c;
    const int st = timed([&] { return launch_wn_stack(din, a, batch, dtype, stream, c); });
    const double cols = (double)batch * a.T;
    const double fl = 2.0 * cols * a.H * (a.layers * 2.0 * a.H * a.taps + (a.layers - (a.final_layer ? 1 : 0)) * (double)drs.M + (a.final_layer ? (double)drs_last.M : 0.0));
    const double fuse_fl = (dpre ? 2.0 * cols * dpre->M * dpre->Cin : 0.0) + (dpost ? 2.0 * cols * dpost->M * dpost->Cin : 0.0);
    note(fl + fuse_fl, cols * a.H * 8 + a.layers * ((double)din.w_bytes() + (double)drs.w_bytes()), "%s<%s,W%d,L%d%s%s>",
         c.family == LF_WN_STACK2 ? "wn_stack2" : "wn_stack", tn(dtype), din.WM, a.layers, dpre ? ",pre+post" : "",
         c.family == LF_WN_STACK2 && c.NF == 5 ? ",64f" : "");
    return st;
  }
  int gemv(const GemvArgs& a) {
    const int st = timed([&] { return launch_gemv(a, stream); });
    note(2.0 * a.rows * a.gin * a.batch, (double)a.rows * a.gin * 4 + (double)a.batch * (a.rows + a.gin) * 4, "cond_gemv");
    return st;
  }
  int sample(const SampleArgs& a) {
    const int st = timed([&] { return launch_sample(a, stream); });
    note(0, (double)a.batch * a.frames * a.C * 16, "sample");
    return st;
  }
  // per band and frame 18 fp32 rows in, 4 samples out (four bands, or the single-band decoder's one)
  int tail(const TailArgs& a) {
    const int st = timed([&] { return launch_tail(a, stream); });
    const bool one = a.bands == 1;
    note(0, (double)a.batch * ((double)a.F * (one ? 18 : 72) * 4 + (one ? 4.0 : 16.0) * (a.F - 1) * 4), one ? "istft1" : "istft_synth");
    return st;
  }
  bool post_tail_ok(const ConvDesc& d) const { return debug_get(DBG_POST_TAIL) != 0 && post_tail_supported(d); }
  // algorithmic: the three stage-final ResBlock streams read once, the waveform written once, conv_post's weights
  // (single band: its 18 rows, half of the packed stream)
  int post_tail(const ConvDesc& d, const PostTailArgs& a, int batch, int dtype) {
    const int st = timed([&] { return launch_post_tail(d, a, batch, dtype, stream); });
    const bool one = post_tail_bands(d) == 1;
    note(2.0 * batch * (double)a.F * d.M * d.taps * d.Cin,
         (double)batch * ((double)a.c.T_in * d.Cin * 2 * 3 + (one ? 4.0 : 16.0) * (a.F - 1) * 4) + (double)d.w_bytes() / (one ? 2 : 1),
         one ? "post_tail1<%s>" : "post_tail<%s>", tn(dtype));
    return st;
  }
  int zero(void* p, size_t bytes) {
    const int st = timed([&] { return hipMemsetAsync(p, 0, bytes, stream) == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH; });
    note(0, (double)bytes, "memset");
    return st;
  }
  int finish() {
    if (!ok || hipStreamSynchronize(stream) != hipSuccess) ok = false;
    for (int i = 0; i + 1 < (int)ev.size() && i < max_rec; ++i) {
      float ms = 0.f;
      if (ok && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) rec[i].ms = ms;
    }
    for (hipEvent_t e : ev) hipEventDestroy(e);
    ev.clear();
    return ok ? QVC_OK : QVC_ERR_LAUNCH;
  }
};

// What every entry point that runs the path, or a stage of it, does: argument check, plan, workspace carve-up, the
// path context on the caller's backend; `body` issues the launches.  whole: a whole-path entry point, which honours the
// step window "launch_stop" and reports "launch_steps" (host-side bookkeeping only).
template <class Backend, class Body>
int run_path(Backend& be, bool whole, bool args_ok, const qvc_config* cfg, const void* blob, int batch, int frames, void* ws,
             int64_t ws_bytes, Body body) {
  if (!args_ok || !cfg || !blob || !ws || batch <= 0 || frames <= 1) return QVC_ERR_BAD_ARG;
  const Plan P = build_plan(*cfg);
  if (P.status != QVC_OK) return P.status;
  const Workspace W = carve_workspace(P, batch, frames);
  if (ws_bytes < W.bytes) return QVC_ERR_SMALL_BUFFER;
  if ((reinterpret_cast<uintptr_t>(ws) & 255) || (reinterpret_cast<uintptr_t>(blob) & 255)) return QVC_ERR_BAD_ARG;
  Path<Backend> c{P, static_cast<const char*>(blob), static_cast<char*>(ws), W, batch, frames, be};
  const int stop = debug_get(DBG_LAUNCH_STOP);
  if (whole && stop >= 0) c.step_hi = stop;
  body(c);
  if (whole) debug_launch_steps().store(c.step_n, std::memory_order_relaxed);
  const int fin = be.finish();
  return c.status != QVC_OK ? c.status : fin;
}

// qvc_noise_rng -> the kernels' view of it (false: no descriptor or no key array, the caller's error)
bool rng_view(const qvc_noise_rng* r, NoiseRng& v) {
  if (!r || !r->keys_dev) return false;
  v.keys = r->keys_dev; v.seed_lo = (uint32_t)r->seed; v.seed_hi = (uint32_t)(r->seed >> 32); v.scale = r->scale;
  return true;
}

// qvc_infer_batch_ragged / _fm: the whole path over utterances of different lengths (unit_fm: units frame-major as on disk).
// Exactly one of noise / rng: the _rng twins pass the generator and no tensor.
int infer_ragged(const qvc_config* cfg, const void* blob_dev, const float* unit, bool unit_fm, const float* g, const float* noise,
                 float* out, int32_t batch, int32_t max_frames, const int32_t* frames_dev, void* workspace, int64_t workspace_bytes,
                 void* stream, const qvc_noise_rng* rng = nullptr) {
  HipBackend be(stream);
  NoiseRng rv;
  const bool draw = rng ? (!noise && rng_view(rng, rv)) : noise != nullptr;
  return run_path(be, true, unit && g && draw && out && frames_dev, cfg, blob_dev, batch, max_frames, workspace, workspace_bytes,
                  [&](Ctx& c) { c.lens = frames_dev; c.unit_fm = unit_fm; c.rng = rv; c.infer(unit, g, noise, out); });
}

// qvc_infer_fanout_ragged / _fm: `rows` output rows from `sources` encoded sources.  The per-row length array follows the
// workspace of (rows, max_frames), which is carved as for every other entry point.
inline int64_t fanout_tail_bytes(int32_t rows) { return align_up((int64_t)rows * 4, 256); }
int infer_fanout(const qvc_config* cfg, const void* blob_dev, const float* unit, bool unit_fm, const int32_t* frames_dev,
                 const int32_t* src_dev, const float* g, const float* noise, float* out, int32_t sources, int32_t rows,
                 int32_t max_frames, void* workspace, int64_t workspace_bytes, void* stream, const qvc_noise_rng* rng = nullptr) {
  HipBackend be(stream);
  NoiseRng rv;
  const bool draw = rng ? (!noise && rng_view(rng, rv)) : noise != nullptr;
  const bool ok = unit && frames_dev && src_dev && g && draw && out && sources >= 1 && sources <= rows;
  return run_path(be, true, ok, cfg, blob_dev, rows, max_frames, workspace, workspace_bytes - (ok ? fanout_tail_bytes(rows) : 0), [&](Ctx& c) {
    c.unit_fm = unit_fm; c.rng = rv;
    c.infer_fanout(unit, frames_dev, src_dev, sources, g, noise, out, c.wsp<int32_t>(c.W.bytes));
  });
}

// What every streaming step / tick entry point does (qvc_stream_step, qvc_live_step, qvc_live_tick and their _rng twins:
// exactly one of noise_new / rng): the draw, the host checks of qvc_stream.h (pointers and batch, then `need` -- the plan
// and the bytes the call needs --, then the two sizes), the alignments, and `step` on the caller's stream.
template <class NeedFn, class StepFn>
int run_stream(bool ptrs_ok, const float* noise_new, const qvc_noise_rng* rng, const void* blob_dev, void* state, int64_t state_bytes,
               void* workspace, int64_t workspace_bytes, int32_t batch, void* stream, NeedFn need, StepFn step) {
  NoiseRng rv;
  const bool draw = rng ? (!noise_new && rng_view(rng, rv)) : noise_new != nullptr;
  const int st = stream_checks(ptrs_ok && draw && blob_dev && state && workspace, batch, state_bytes, workspace_bytes, need);
  if (st != QVC_OK) return st;
  if ((reinterpret_cast<uintptr_t>(workspace) & 255) || (reinterpret_cast<uintptr_t>(blob_dev) & 255) || (reinterpret_cast<uintptr_t>(state) & 255))
    return QVC_ERR_BAD_ARG;
  HipBackend be(stream);
  const int rc = step(be, rng ? &rv : nullptr);
  return rc != QVC_OK ? rc : be.finish();
}

// qvc_stream_step (tick == false: no n_new_dev, pos_dev is only read) and qvc_stream_tick (the tick's scratch; pos_dev is
// the caller's int32_t*)
int stream_step_api(bool tick, const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                    const float* g, const float* noise_new, const qvc_noise_rng* rng, float* out, int32_t batch, int32_t hop,
                    const int32_t* n_new_dev, const int32_t* pos_dev, const int32_t* len_dev, void* workspace, int64_t workspace_bytes,
                    void* stream) {
  Plan P; StreamGeom G;
  return run_stream(unit_new && g && out && (n_new_dev || !tick) && pos_dev && len_dev, noise_new, rng, blob_dev, state, state_bytes, workspace,
                    workspace_bytes, batch, stream,
    [&](StreamBytes& b) {
      const int gs = stream_plan(cfg, hop, P, G);
      if (gs == QVC_OK) b = {carve_stream_state(P, G, batch).bytes, carve_stream_scratch(P, G, batch, tick).bytes};
      return gs;
    },
    [&](HipBackend& be, const NoiseRng* rv) {
      const char* blob = static_cast<const char*>(blob_dev);
      char* st = static_cast<char*>(state);
      char* ws = static_cast<char*>(workspace);
      return tick ? stream_tick(P, blob, st, ws, unit_new, g, noise_new, out, batch, hop, n_new_dev, const_cast<int32_t*>(pos_dev), len_dev, be, rv)
                  : stream_step(P, blob, st, ws, unit_new, g, noise_new, out, batch, hop, pos_dev, len_dev, be, rv);
    });
}

// qvc_live_step (tick == false: no n_new_dev, pos_dev is only read) and qvc_live_tick (pos_dev is the caller's int32_t*)
int live_step_api(bool tick, const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                  const float* g, const float* noise_new, const qvc_noise_rng* rng, float* out, int32_t batch, int32_t hop,
                  int32_t look_ahead, const int32_t* n_new_dev, const int32_t* pos_dev, const int32_t* len_dev, void* workspace,
                  int64_t workspace_bytes, void* stream) {
  Plan P; LiveGeom G;
  return run_stream(unit_new && g && out && (n_new_dev || !tick) && pos_dev && len_dev, noise_new, rng, blob_dev, state, state_bytes, workspace,
                    workspace_bytes, batch, stream,
    [&](StreamBytes& b) {
      const int gs = live_plan(cfg, hop, look_ahead, P, G);
      if (gs == QVC_OK) b = {carve_live_state(P, G, batch).bytes, carve_live_scratch(P, G, batch, tick).bytes};
      return gs;
    },
    [&](HipBackend& be, const NoiseRng* rv) {
      const bool trim = debug_get(DBG_LIVE_TRIM) != 0;
      const char* blob = static_cast<const char*>(blob_dev);
      char* st = static_cast<char*>(state);
      char* ws = static_cast<char*>(workspace);
      return tick ? live_tick(P, G, blob, st, ws, unit_new, g, noise_new, out, batch, n_new_dev, const_cast<int32_t*>(pos_dev), len_dev, be, rv, trim)
                  : live_step(P, G, blob, st, ws, unit_new, g, noise_new, out, batch, pos_dev, len_dev, be, rv, trim);
    });
}

// What the three *_reset_slot entry points do: reset_slot of qvc_stream.h with memsets on the caller's stream, then
// pos[slot] = 0 and lens[slot] = length there too (no host buffer involved).
template <class RingsFn>
int reset_slot_api(void* state, int64_t state_bytes, int32_t batch, int32_t slot, int32_t length, int32_t* pos_dev, int32_t* len_dev,
                   void* stream, RingsFn rings) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  bool ok = true;
  const int rc = reset_slot(state, state_bytes, batch, slot, length, pos_dev, len_dev, rings,
                            [&](char* p, size_t n) { ok = ok && hipMemsetAsync(p, 0, n, st) == hipSuccess; });
  if (rc != QVC_OK) return rc;
  ok = ok && hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(pos_dev + slot), 0, 1, st) == hipSuccess;
  ok = ok && hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(len_dev + slot), length, 1, st) == hipSuccess;
  return ok ? QVC_OK : QVC_ERR_LAUNCH;
}

// qvc_stream_export_slots / qvc_stream_import_slots: snapshot_slots of qvc_stream.h (the checks, then copy_batch launches
// only) on the caller's stream.
int snapshot_api(bool import, const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop, const int32_t* slots_host,
                 int32_t n_slots, int32_t* pos_dev, int32_t* len_dev, void* snap_dev, int64_t snap_bytes, void* stream) {
  HipBackend be(stream);
  const int rc = snapshot_slots(import, be, cfg, state, state_bytes, batch, hop, slots_host, n_slots, pos_dev, len_dev, snap_dev, snap_bytes);
  return rc != QVC_OK ? rc : be.finish();
}

// qvc_infer_windows_fm / _rng_fm: infer_windows of qvc_stream.h (the checks, then gather, the window, deliver) on the
// caller's stream.  Exactly one of noise_packed / rng; a descriptor without keys counts as no draw.
int windows_api(const qvc_config* cfg, const void* blob_dev, const float* unit_fm_packed, const float* noise_packed, const qvc_noise_rng* rng,
                const qvc_window* win_dev, const float* g, float* out_packed, int32_t rows, int32_t window_frames, int32_t total_frames,
                void* workspace, int64_t workspace_bytes, void* stream) {
  HipBackend be(stream);
  NoiseRng rv;
  if (rng) rng_view(rng, rv);
  const int rc = infer_windows(be, cfg, blob_dev, unit_fm_packed, noise_packed, rng ? &rv : nullptr, win_dev, g, out_packed, rows, window_frames,
                               total_frames, workspace, workspace_bytes, debug_get(DBG_LIVE_TRIM) != 0);
  return rc != QVC_OK ? rc : be.finish();
}

}  // namespace

extern "C" {

int qvc_abi_version(void) { return QVC_ABI_VERSION; }

const char* qvc_status_string(int status) {
  switch (status) {
    case QVC_OK: return "ok";
    case QVC_ERR_BAD_ARG: return "bad argument (null pointer, non-positive size, misaligned buffer or bad enum)";
    case QVC_ERR_BAD_CONFIG: return "unsupported model configuration";
    case QVC_ERR_MISSING_TENSOR: return "a state-dict tensor needed by the path is missing";
    case QVC_ERR_BAD_SHAPE: return "a state-dict tensor has an unexpected shape";
    case QVC_ERR_SMALL_BUFFER: return "blob or workspace smaller than the matching *_bytes() query";
    case QVC_ERR_LAUNCH: return "HIP kernel launch failed";
    case QVC_ERR_NO_DEVICE: return "no gfx950 HIP device visible";
    default: return "unknown status";
  }
}

int qvc_debug_set(const char* name, int32_t value) {
  if (!name) return QVC_ERR_BAD_ARG;
  for (int i = 0; i < DBG_COUNT; ++i)
    if (std::strcmp(name, debug_names()[i]) == 0) { debug_table()[i].store(value, std::memory_order_relaxed); return QVC_OK; }
  return QVC_ERR_BAD_ARG;
}

int qvc_debug_get(const char* name, int32_t* value) {
  if (!name || !value) return QVC_ERR_BAD_ARG;
  for (int i = 0; i < DBG_COUNT; ++i)
    if (std::strcmp(name, debug_names()[i]) == 0) { *value = debug_get(i); return QVC_OK; }
  if (std::strcmp(name, "launch_steps") == 0) { *value = debug_launch_steps().load(std::memory_order_relaxed); return QVC_OK; }
  return QVC_ERR_BAD_ARG;
}

int qvc_debug_saturations(int64_t* count, int32_t reset) {
  if (!count) return QVC_ERR_BAD_ARG;
#ifdef QVC_SATCOUNT
  const unsigned long long v[5] = {sat_count_conv_f16(reset != 0), sat_count_conv_bf16(reset != 0), sat_count_wn2(reset != 0), sat_count_spk(reset != 0),
                                   sat_count_chain(reset != 0)};
  unsigned long long sum = 0;
  for (unsigned long long x : v) { if (x == ~0ull) return QVC_ERR_LAUNCH; sum += x; }
  *count = (int64_t)sum;
  return QVC_OK;
#else
  (void)reset;
  *count = -1;
  return QVC_ERR_BAD_CONFIG;      // the product library does not count (no instruction is spent on it)
#endif
}

int qvc_device_check(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return QVC_ERR_NO_DEVICE;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return QVC_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return QVC_ERR_NO_DEVICE;
  return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? QVC_OK : QVC_ERR_NO_DEVICE;
}

int64_t qvc_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t frames) {
  if (!cfg || batch <= 0 || frames <= 1) return QVC_ERR_BAD_ARG;
  Plan P = build_plan(*cfg);
  if (P.status != QVC_OK) return P.status;
  return carve_workspace(P, batch, frames).bytes;
}

int qvc_plan_info(const qvc_config* cfg, int32_t info[8]) { return plan_flags(cfg, info); }

int qvc_aux_create(qvc_aux** out) {
  if (!out) return QVC_ERR_BAD_ARG;
  qvc_aux* a = new (std::nothrow) qvc_aux();
  if (!a) return QVC_ERR_BAD_ARG;
  bool ok = true;
  for (auto& s : a->streams) ok = ok && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&a->fork, hipEventDisableTiming) == hipSuccess;
  for (auto& e : a->done) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  if (!ok) { delete a; return QVC_ERR_LAUNCH; }
  *out = a;
  return QVC_OK;
}

int qvc_aux_destroy(qvc_aux* a) {
  if (!a) return QVC_ERR_BAD_ARG;
  for (auto& s : a->streams) hipStreamDestroy(s);
  hipEventDestroy(a->fork);
  for (auto& e : a->done) hipEventDestroy(e);
  delete a;
  return QVC_OK;
}

int qvc_infer_batch(const qvc_config* cfg, const void* blob_dev, const float* unit, const float* g,
                    const float* noise, float* out, int32_t batch, int32_t frames, void* workspace,
                    int64_t workspace_bytes, void* stream) {
  return qvc_infer_batch_ex(cfg, blob_dev, unit, g, noise, out, batch, frames, workspace, workspace_bytes, stream, nullptr);
}

int qvc_infer_batch_ex(const qvc_config* cfg, const void* blob_dev, const float* unit, const float* g,
                       const float* noise, float* out, int32_t batch, int32_t frames, void* workspace,
                       int64_t workspace_bytes, void* stream, qvc_aux* aux) {
  HipBackend be(stream, aux);
  return run_path(be, true, unit && g && noise && out, cfg, blob_dev, batch, frames, workspace, workspace_bytes,
                  [&](Ctx& c) { c.infer(unit, g, noise, out); });
}

int qvc_infer_batch_ragged(const qvc_config* cfg, const void* blob_dev, const float* unit, const float* g,
                           const float* noise, float* out, int32_t batch, int32_t max_frames, const int32_t* frames_dev,
                           void* workspace, int64_t workspace_bytes, void* stream) {
  return infer_ragged(cfg, blob_dev, unit, false, g, noise, out, batch, max_frames, frames_dev, workspace, workspace_bytes, stream);
}

int qvc_infer_batch_ragged_fm(const qvc_config* cfg, const void* blob_dev, const float* unit_fm, const float* g,
                              const float* noise, float* out, int32_t batch, int32_t max_frames, const int32_t* frames_dev,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  return infer_ragged(cfg, blob_dev, unit_fm, true, g, noise, out, batch, max_frames, frames_dev, workspace, workspace_bytes, stream);
}

int qvc_infer_batch_ragged_rng(const qvc_config* cfg, const void* blob_dev, const float* unit, const float* g,
                               const qvc_noise_rng* rng, float* out, int32_t batch, int32_t max_frames, const int32_t* frames_dev,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (!rng) return QVC_ERR_BAD_ARG;
  return infer_ragged(cfg, blob_dev, unit, false, g, nullptr, out, batch, max_frames, frames_dev, workspace, workspace_bytes, stream, rng);
}

int qvc_infer_batch_ragged_rng_fm(const qvc_config* cfg, const void* blob_dev, const float* unit_fm, const float* g,
                                  const qvc_noise_rng* rng, float* out, int32_t batch, int32_t max_frames, const int32_t* frames_dev,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  if (!rng) return QVC_ERR_BAD_ARG;
  return infer_ragged(cfg, blob_dev, unit_fm, true, g, nullptr, out, batch, max_frames, frames_dev, workspace, workspace_bytes, stream, rng);
}

int qvc_noise_fill(uint64_t seed, const uint64_t* keys_dev, float scale, int32_t rows, int32_t channels, int32_t frames,
                   int32_t frame0, float* noise_out, void* stream) {
  const qvc_noise_rng r{seed, keys_dev, scale};
  NoiseRng rv;
  if (!rng_view(&r, rv)) return QVC_ERR_BAD_ARG;
  return launch_noise_fill(rv, rows, channels, frames, frame0, noise_out, stream);
}

int64_t qvc_fanout_workspace_bytes(const qvc_config* cfg, int32_t sources, int32_t rows, int32_t max_frames) {
  if (sources < 1 || sources > rows) return QVC_ERR_BAD_ARG;
  const int64_t n = qvc_workspace_bytes(cfg, rows, max_frames);
  return n < 0 ? n : n + fanout_tail_bytes(rows);
}

int qvc_infer_fanout_ragged(const qvc_config* cfg, const void* blob_dev, const float* unit, const int32_t* frames_dev,
                            const int32_t* src_of_row_dev, const float* g, const float* noise, float* out, int32_t sources,
                            int32_t rows, int32_t max_frames, void* workspace, int64_t workspace_bytes, void* stream) {
  return infer_fanout(cfg, blob_dev, unit, false, frames_dev, src_of_row_dev, g, noise, out, sources, rows, max_frames, workspace,
                      workspace_bytes, stream);
}

int qvc_infer_fanout_ragged_fm(const qvc_config* cfg, const void* blob_dev, const float* unit_fm, const int32_t* frames_dev,
                               const int32_t* src_of_row_dev, const float* g, const float* noise, float* out, int32_t sources,
                               int32_t rows, int32_t max_frames, void* workspace, int64_t workspace_bytes, void* stream) {
  return infer_fanout(cfg, blob_dev, unit_fm, true, frames_dev, src_of_row_dev, g, noise, out, sources, rows, max_frames, workspace,
                      workspace_bytes, stream);
}

int qvc_infer_fanout_ragged_rng(const qvc_config* cfg, const void* blob_dev, const float* unit, const int32_t* frames_dev,
                                const int32_t* src_of_row_dev, const float* g, const qvc_noise_rng* rng, float* out, int32_t sources,
                                int32_t rows, int32_t max_frames, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!rng) return QVC_ERR_BAD_ARG;
  return infer_fanout(cfg, blob_dev, unit, false, frames_dev, src_of_row_dev, g, nullptr, out, sources, rows, max_frames, workspace,
                      workspace_bytes, stream, rng);
}

int qvc_infer_fanout_ragged_rng_fm(const qvc_config* cfg, const void* blob_dev, const float* unit_fm, const int32_t* frames_dev,
                                   const int32_t* src_of_row_dev, const float* g, const qvc_noise_rng* rng, float* out, int32_t sources,
                                   int32_t rows, int32_t max_frames, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!rng) return QVC_ERR_BAD_ARG;
  return infer_fanout(cfg, blob_dev, unit_fm, true, frames_dev, src_of_row_dev, g, nullptr, out, sources, rows, max_frames, workspace,
                      workspace_bytes, stream, rng);
}

int64_t qvc_stream_state_bytes(const qvc_config* cfg, int32_t batch, int32_t hop) {
  Plan P; StreamGeom G;
  const int st = batch > 0 ? stream_plan(cfg, hop, P, G) : QVC_ERR_BAD_ARG;
  return st != QVC_OK ? st : carve_stream_state(P, G, batch).bytes;
}

int64_t qvc_stream_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t hop) {
  Plan P; StreamGeom G;
  const int st = batch > 0 ? stream_plan(cfg, hop, P, G) : QVC_ERR_BAD_ARG;
  return st != QVC_OK ? st : carve_stream_scratch(P, G, batch).bytes;
}

int32_t qvc_stream_lag_frames(const qvc_config* cfg) {
  Plan P; StreamGeom G;
  const int st = stream_plan(cfg, 1, P, G);
  return st != QVC_OK ? st : G.lag();
}

int32_t qvc_stream_noise_lag_frames(const qvc_config* cfg) {
  Plan P; StreamGeom G;
  const int st = stream_plan(cfg, 1, P, G);
  return st != QVC_OK ? st : G.He;
}

int qvc_stream_step(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                    const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, const int32_t* pos_dev,
                    const int32_t* len_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  return stream_step_api(false, cfg, blob_dev, state, state_bytes, unit_new, g, noise_new, nullptr, out, batch, hop, nullptr, pos_dev, len_dev, workspace,
                         workspace_bytes, stream);
}

int qvc_stream_step_rng(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                        const float* g, const qvc_noise_rng* rng, float* out, int32_t batch, int32_t hop, const int32_t* pos_dev,
                        const int32_t* len_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!rng) return QVC_ERR_BAD_ARG;
  return stream_step_api(false, cfg, blob_dev, state, state_bytes, unit_new, g, nullptr, rng, out, batch, hop, nullptr, pos_dev, len_dev, workspace,
                         workspace_bytes, stream);
}

int qvc_stream_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop, int32_t slot,
                          int32_t length, int32_t* pos_dev, int32_t* len_dev, void* stream) {
  return reset_slot_api(state, state_bytes, batch, slot, length, pos_dev, len_dev, stream, [&](Rings& R) {
    Plan P; StreamGeom G;
    const int gs = stream_plan(cfg, hop, P, G);
    if (gs == QVC_OK) R = stream_rings(P, G, batch);
    return gs;
  });
}

int64_t qvc_stream_snapshot_bytes(const qvc_config* cfg) {
  SnapLayout L;
  const int st = stream_snapshot(cfg, L);
  return st != QVC_OK ? st : L.bytes;
}

int qvc_stream_snapshot_tag(const qvc_config* cfg, uint64_t* tag) {
  SnapLayout L;
  return tag ? stream_snapshot(cfg, L, tag) : QVC_ERR_BAD_ARG;
}

int qvc_stream_export_slots(const qvc_config* cfg, const void* state, int64_t state_bytes, int32_t batch, int32_t hop,
                            const int32_t* slots_host, int32_t n_slots, const int32_t* pos_dev, const int32_t* len_dev, void* snap_dev,
                            int64_t snap_bytes, void* stream) {
  return snapshot_api(false, cfg, const_cast<void*>(state), state_bytes, batch, hop, slots_host, n_slots, const_cast<int32_t*>(pos_dev),
                      const_cast<int32_t*>(len_dev), snap_dev, snap_bytes, stream);      // an export only reads them
}

int qvc_stream_import_slots(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop, const int32_t* slots_host,
                            int32_t n_slots, int32_t* pos_dev, int32_t* len_dev, const void* snap_dev, int64_t snap_bytes, void* stream) {
  return snapshot_api(true, cfg, state, state_bytes, batch, hop, slots_host, n_slots, pos_dev, len_dev, const_cast<void*>(snap_dev), snap_bytes,
                      stream);                                                          // an import only reads the snapshots
}

int64_t qvc_stream_tick_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t hop) {
  Plan P; StreamGeom G;
  const int st = batch > 0 ? stream_plan(cfg, hop, P, G) : QVC_ERR_BAD_ARG;
  return st != QVC_OK ? st : carve_stream_scratch(P, G, batch, true).bytes;
}

int qvc_stream_tick(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                    const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, const int32_t* n_new_dev,
                    int32_t* pos_dev, const int32_t* len_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  return stream_step_api(true, cfg, blob_dev, state, state_bytes, unit_new, g, noise_new, nullptr, out, batch, hop, n_new_dev, pos_dev, len_dev,
                         workspace, workspace_bytes, stream);
}

int qvc_stream_tick_rng(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                        const float* g, const qvc_noise_rng* rng, float* out, int32_t batch, int32_t hop, const int32_t* n_new_dev,
                        int32_t* pos_dev, const int32_t* len_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!rng) return QVC_ERR_BAD_ARG;
  return stream_step_api(true, cfg, blob_dev, state, state_bytes, unit_new, g, nullptr, rng, out, batch, hop, n_new_dev, pos_dev, len_dev,
                         workspace, workspace_bytes, stream);
}

int32_t qvc_live_context_frames(const qvc_config* cfg) {
  Plan P; LiveGeom G;
  const int st = live_plan(cfg, 1, 0, P, G);
  return st != QVC_OK ? st : G.C();
}

int64_t qvc_live_state_bytes(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead) {
  Plan P; LiveGeom G;
  const int st = batch > 0 ? live_plan(cfg, hop, look_ahead, P, G) : QVC_ERR_BAD_ARG;
  return st != QVC_OK ? st : carve_live_state(P, G, batch).bytes;
}

int64_t qvc_live_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead) {
  Plan P; LiveGeom G;
  const int st = batch > 0 ? live_plan(cfg, hop, look_ahead, P, G) : QVC_ERR_BAD_ARG;
  return st != QVC_OK ? st : carve_live_scratch(P, G, batch).bytes;
}

int qvc_live_step(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                  const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, int32_t look_ahead,
                  const int32_t* pos_dev, const int32_t* len_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  return live_step_api(false, cfg, blob_dev, state, state_bytes, unit_new, g, noise_new, nullptr, out, batch, hop, look_ahead, nullptr, pos_dev, len_dev,
                       workspace, workspace_bytes, stream);
}

int qvc_live_step_rng(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                      const float* g, const qvc_noise_rng* rng, float* out, int32_t batch, int32_t hop, int32_t look_ahead,
                      const int32_t* pos_dev, const int32_t* len_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!rng) return QVC_ERR_BAD_ARG;
  return live_step_api(false, cfg, blob_dev, state, state_bytes, unit_new, g, nullptr, rng, out, batch, hop, look_ahead, nullptr, pos_dev, len_dev,
                       workspace, workspace_bytes, stream);
}

int qvc_live_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop, int32_t look_ahead,
                        int32_t slot, int32_t length, int32_t* pos_dev, int32_t* len_dev, void* stream) {
  return reset_slot_api(state, state_bytes, batch, slot, length, pos_dev, len_dev, stream, [&](Rings& R) {
    Plan P; LiveGeom G;
    const int gs = live_plan(cfg, hop, look_ahead, P, G);
    if (gs == QVC_OK) R = live_rings(P, G, batch);
    return gs;
  });
}

// The tick state IS the lockstep state (qvc_stream.h: live_rings, SHARED): the two names below are kept as aliases.
int64_t qvc_live_tick_state_bytes(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead) {
  return qvc_live_state_bytes(cfg, batch, hop, look_ahead);
}

int64_t qvc_live_tick_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead) {
  Plan P; LiveGeom G;
  const int st = batch > 0 ? live_plan(cfg, hop, look_ahead, P, G) : QVC_ERR_BAD_ARG;
  return st != QVC_OK ? st : carve_live_scratch(P, G, batch, true).bytes;
}

int qvc_live_tick(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                  const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, int32_t look_ahead,
                  const int32_t* n_new_dev, int32_t* pos_dev, const int32_t* len_dev, void* workspace, int64_t workspace_bytes,
                  void* stream) {
  return live_step_api(true, cfg, blob_dev, state, state_bytes, unit_new, g, noise_new, nullptr, out, batch, hop, look_ahead, n_new_dev, pos_dev,
                       len_dev, workspace, workspace_bytes, stream);
}

int qvc_live_tick_rng(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes, const float* unit_new,
                      const float* g, const qvc_noise_rng* rng, float* out, int32_t batch, int32_t hop, int32_t look_ahead,
                      const int32_t* n_new_dev, int32_t* pos_dev, const int32_t* len_dev, void* workspace, int64_t workspace_bytes,
                      void* stream) {
  if (!rng) return QVC_ERR_BAD_ARG;
  return live_step_api(true, cfg, blob_dev, state, state_bytes, unit_new, g, nullptr, rng, out, batch, hop, look_ahead, n_new_dev, pos_dev,
                       len_dev, workspace, workspace_bytes, stream);
}

int qvc_live_tick_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop, int32_t look_ahead,
                             int32_t slot, int32_t length, int32_t* pos_dev, int32_t* len_dev, void* stream) {
  return qvc_live_reset_slot(cfg, state, state_bytes, batch, hop, look_ahead, slot, length, pos_dev, len_dev, stream);
}

int64_t qvc_windows_workspace_bytes(const qvc_config* cfg, int32_t rows, int32_t window_frames) {
  Plan P; LiveGeom G;
  const int st = rows > 0 && rows <= 65535 ? window_plan(cfg, window_frames, P, G) : QVC_ERR_BAD_ARG;
  return st != QVC_OK ? st : carve_window_scratch(P, G, rows).bytes;
}

int qvc_infer_windows_fm(const qvc_config* cfg, const void* blob_dev, const float* unit_fm_packed, const float* noise_packed,
                         const qvc_window* win_dev, const float* g, float* out_packed, int32_t rows, int32_t window_frames,
                         int32_t total_frames, void* workspace, int64_t workspace_bytes, void* stream) {
  return windows_api(cfg, blob_dev, unit_fm_packed, noise_packed, nullptr, win_dev, g, out_packed, rows, window_frames, total_frames, workspace,
                     workspace_bytes, stream);
}

int qvc_infer_windows_rng_fm(const qvc_config* cfg, const void* blob_dev, const float* unit_fm_packed, const qvc_noise_rng* rng,
                             const qvc_window* win_dev, const float* g, float* out_packed, int32_t rows, int32_t window_frames,
                             int32_t total_frames, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!rng) return QVC_ERR_BAD_ARG;
  return windows_api(cfg, blob_dev, unit_fm_packed, nullptr, rng, win_dev, g, out_packed, rows, window_frames, total_frames, workspace,
                     workspace_bytes, stream);
}

int qvc_infer_batch_timed(const qvc_config* cfg, const void* blob_dev, const float* unit, const float* g,
                          const float* noise, float* out, int32_t batch, int32_t frames, void* workspace,
                          int64_t workspace_bytes, void* stream, qvc_launch_record* records, int32_t max_records,
                          int32_t* n_records) {
  TimedBackend be{static_cast<hipStream_t>(stream), records, max_records};
  return run_path(be, true, unit && g && noise && out && records && max_records > 0 && n_records, cfg, blob_dev, batch, frames, workspace,
                  workspace_bytes, [&](Path<TimedBackend>& c) { c.infer(unit, g, noise, out); *n_records = be.n; });
}

int qvc_enc_p(const qvc_config* cfg, const void* blob_dev, const float* unit, const float* noise, float* z_p_fm,
              int32_t batch, int32_t frames, void* workspace, int64_t workspace_bytes, void* stream) {
  HipBackend be(stream);
  return run_path(be, false, unit && noise && z_p_fm, cfg, blob_dev, batch, frames, workspace, workspace_bytes,
                  [&](Ctx& c) { c.enc_p(unit, noise, z_p_fm); });
}

int qvc_wn_stack(const qvc_config* cfg, const void* blob_dev, int32_t which, const float* x_fm, const float* g,
                 float* out_fm, int32_t batch, int32_t frames, void* workspace, int64_t workspace_bytes, void* stream) {
  HipBackend be(stream);
  return run_path(be, false, x_fm && out_fm && which >= 0 && (which == 0 || g), cfg, blob_dev, batch, frames, workspace, workspace_bytes, [&](Ctx& c) {
    const Plan& P = c.P;
    const FlowStepPlan* f = nullptr;
    for (const FlowStepPlan& s : P.flow) if (s.layer == which - 1) f = &s;
    if (which > cfg->n_flows || (which > 0 && !f)) { c.status = QVC_ERR_BAD_ARG; return; }
    const size_t bytes = (size_t)batch * frames * cfg->hidden_channels * 4;
    if (hipMemcpyAsync(c.wsp<float>(c.W.xw), x_fm, bytes, hipMemcpyDeviceToDevice, be.stream) != hipSuccess) { c.status = QVC_ERR_LAUNCH; return; }
    if (which == 0) {
      c.wn(P.enc_wn, reinterpret_cast<const float*>(c.blob + P.enc_wn.inbias_off), 0);
    } else {
      c.cond_table(g);
      c.wn(f->wn, c.wsp<float>(c.W.bb) + f->cond_row0, P.cond_rows);
    }
    if (c.status == QVC_OK && hipMemcpyAsync(out_fm, c.wsp<float>(c.W.oacc), bytes, hipMemcpyDeviceToDevice, be.stream) != hipSuccess) c.status = QVC_ERR_LAUNCH;
  });
}

int qvc_flow_reverse(const qvc_config* cfg, const void* blob_dev, float* z_fm, const float* g, int32_t batch,
                     int32_t frames, void* workspace, int64_t workspace_bytes, void* stream) {
  HipBackend be(stream);
  return run_path(be, false, z_fm && g, cfg, blob_dev, batch, frames, workspace, workspace_bytes,
                  [&](Ctx& c) { c.cond_table(g); c.flow(z_fm); });
}

int qvc_flow_forward(const qvc_config* cfg, const void* blob_dev, float* z_fm, const float* g, int32_t batch,
                     int32_t frames, void* workspace, int64_t workspace_bytes, void* stream) {
  HipBackend be(stream);
  return run_path(be, true, z_fm && g, cfg, blob_dev, batch, frames, workspace, workspace_bytes,
                  [&](Ctx& c) { c.cond_table(g); c.flow(z_fm, /*forward=*/true); });
}

int qvc_enc_q(const qvc_config* cfg, const void* encq_blob_dev, const float* spec, const float* g, const float* noise,
              float* z_fm, int32_t batch, int32_t frames, void* workspace, int64_t workspace_bytes, void* stream) {
  HipBackend be(stream);
  return run_path(be, true, spec && g && noise && z_fm, cfg, encq_blob_dev, batch, frames, workspace, workspace_bytes, [&](Ctx& c) {
    const EncQPlan Q = build_encq_plan(*cfg);
    if (Q.status != QVC_OK) c.status = Q.status;
    else c.enc_q(Q, c.blob, spec, g, noise, z_fm);
  });
}

int qvc_dec_trunk(const qvc_config* cfg, const void* blob_dev, const float* z_fm, const float* g, float* post_fm,
                  int32_t batch, int32_t frames, void* workspace, int64_t workspace_bytes, void* stream) {
  HipBackend be(stream);
  return run_path(be, false, z_fm && g && post_fm, cfg, blob_dev, batch, frames, workspace, workspace_bytes,
                  [&](Ctx& c) { c.cond_table(g); c.dec_trunk(z_fm, post_fm); });
}

int qvc_istft_synth(const qvc_config* cfg, const void* blob_dev, const float* post_fm, float* out, float* y_mb,
                    int32_t batch, int32_t post_frames, void* stream) {
  if (!cfg || !blob_dev || !post_fm || !out || batch <= 0 || post_frames <= 1) return QVC_ERR_BAD_ARG;
  Plan P = build_plan(*cfg);
  if (P.status != QVC_OK) return P.status;
  TailArgs ta{post_fm, reinterpret_cast<const float*>(static_cast<const char*>(blob_dev) + P.fir_off), out, y_mb, batch,
              post_frames};
  if (cfg->decoder == QVC_DEC_ISTFT) { ta.fir = nullptr; ta.bands = 1; }
  return launch_tail(ta, stream);
}

int64_t qvc_conv1d_scratch_bytes(int32_t cout, int32_t cin, int32_t k) {
  if (cout <= 0 || cin <= 0 || k <= 0 || cout % 4 || cin % 8) return QVC_ERR_BAD_ARG;
  ConvDesc d = make_conv(cout, cin, k, 1);
  return align_up(d.w_bytes(), 256) + align_up(d.b_bytes(), 256);
}

int64_t qvc_conv1d_workspace_bytes(int32_t batch, int32_t cout, int32_t cin, int32_t frames) {
  if (batch <= 0 || cout <= 0 || cin <= 0 || frames <= 0) return QVC_ERR_BAD_ARG;
  return align_up((int64_t)batch * frames * cout * 4, 256);
}

int qvc_conv1d(const float* x, const float* w_host, const float* bias_host, float* y, int32_t batch, int32_t cin,
               int32_t cout, int32_t frames, int32_t k, int32_t dilation, float slope_in, int32_t operand_dtype,
               void* w_scratch_host, void* w_scratch_dev, int64_t scratch_bytes, void* workspace,
               int64_t workspace_bytes, void* stream) {
  if (!x || !w_host || !y || !w_scratch_host || !w_scratch_dev || !workspace) return QVC_ERR_BAD_ARG;
  if (batch <= 0 || frames <= 0 || k <= 0 || k % 2 == 0 || dilation <= 0 || cout % 4 || cin % 8) return QVC_ERR_BAD_ARG;
  if (operand_dtype != QVC_BF16 && operand_dtype != QVC_F16) return QVC_ERR_BAD_ARG;
  ConvDesc d = make_conv(cout, cin, k, dilation);
  d.w_off = 0; d.b_off = align_up(d.w_bytes(), 256);
  if (scratch_bytes < d.b_off + align_up(d.b_bytes(), 256)) return QVC_ERR_SMALL_BUFFER;
  if (workspace_bytes < qvc_conv1d_workspace_bytes(batch, cout, cin, frames)) return QVC_ERR_SMALL_BUFFER;
  pack_plain_conv(d, w_host, bias_host, operand_dtype, static_cast<char*>(w_scratch_host));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(w_scratch_dev, w_scratch_host, (size_t)(d.b_off + d.b_bytes()), hipMemcpyHostToDevice, s) != hipSuccess)
    return QVC_ERR_LAUNCH;
  ConvArgs a;
  a.w = w_scratch_dev;
  a.bias = reinterpret_cast<const float*>(static_cast<const char*>(w_scratch_dev) + d.b_off);
  a.x = x; a.x_kind = XK_F32_CM; a.x_bs = (int64_t)cin * frames; a.x_ts = frames; a.T_in = frames; a.slope_in = slope_in;
  a.Nq = frames; a.T_out = frames;
  a.y32 = static_cast<float*>(workspace); a.y32_bs = (int64_t)frames * cout; a.y32_ts = cout;
  int st = launch_conv(d, a, batch, EPI_STD, operand_dtype, stream);
  if (st != QVC_OK) return st;
  return launch_fm_to_cm(static_cast<const float*>(workspace), y, batch, frames, cout, stream);
}

}  // extern "C"
