// emu_twin.cpp -- TEST INFRASTRUCTURE: the CPU twin of qvc_live_step, qvc_live_tick and qvc_stream_tick.
//
// The host emulation under oracle/ is frozen, and its backend sits in an unnamed namespace of oracle/qvc_emu.cpp, so this
// translation unit includes that file.  The frozen EmuBackend does not state kStreamTick; TickEmuBackend derives from it,
// states the constant and adds the host version of the count-aware batched copy both ticks move their data with
// (csrc/qvc_small.hip: copy_counted_kernel).  CountingBackend derives from that and counts the launches that move data
// (copy_batch, copy_counted): live_step, live_tick, stream_step and stream_tick (csrc/qvc_stream.h) are instantiated on
// it, so a host test can pin how a step groups its copies into launches.  Built by build.py into
// oracle/_build/libqvc_emu_twin.so and loaded only by the tests.
// RecordingBackend derives from CountingBackend and writes down every copy_batch / copy_counted call of one stream_step
// or stream_tick, descriptor by descriptor (qvc_emu_stream_moves; tests/test_stream_moves_host.py).  The slot snapshots
// (snapshot_slots: qvc_emu_stream_export_slots / _import_slots) run on the same host copy_batch.  The emulation's
// backend has no single-band tail and no generator form of the noise: band-synthesis decoders, pointer form only.
// WindowsEmuBackend derives from CountingBackend, states kWindows and restates the two table-driven kernels of the exact
// windows over packed utterances (qvc_emu_infer_windows_fm; tests/test_windows_host.py).
// TraceBackend stands alone: it computes nothing and writes down every backend call of a Path, field by field
// (qvc_emu_path_trace; tests/test_path_trace_host.py) -- every decoder and every form, since nothing is run.
// SelectBackend walks the same calls and writes down, per launch, the choice its family's chooser returns
// (csrc/qvc_select.h; qvc_emu_launch_trace; tests/test_launch_trace_host.py).
#include "../oracle/qvc_emu.cpp"

#include <array>
#include <string>
#include <type_traits>

namespace {

struct TickEmuBackend : EmuBackend {
  // csrc/qvc_small.hip copy_counted_kernel: the bookkeeping, then every descriptor slot by slot
  static constexpr bool kStreamTick = true;
  int copy_counted(const qvc::CountedHead& h, const qvc::CountedDesc* d, int n) {
    if (n <= 0) return QVC_OK;
    if (!d || n > qvc::kCopyBatchMax || !h.n_new || h.slots < 1 || h.hop < 1) return QVC_ERR_BAD_ARG;
    if ((h.pos_eff != nullptr) != (h.len_eff != nullptr) || (h.pos_eff && (!h.pos || !h.lens))) return QVC_ERR_BAD_ARG;
    for (int i = 0; i < n; ++i) {
      const qvc::CountedDesc& c = d[i];
      if (!c.dst || (!c.src && (c.fixed | c.unit | c.shift))) return QVC_ERR_BAD_ARG;
      if ((uint64_t)c.fixed + (uint64_t)h.hop * c.unit > c.width || c.width > c.dpitch) return QVC_ERR_BAD_ARG;
      if (c.src && (uint64_t)h.hop * c.shift + c.fixed + (uint64_t)h.hop * c.unit > c.spitch) return QVC_ERR_BAD_ARG;
    }
    for (int b = 0; b < h.slots; ++b) {
      const int nb = qvc::tick_count(h.n_new, b, h.hop);
      if (h.pos_eff) { h.pos_eff[b] = nb > 0 ? h.pos[b] : h.idle_pos; h.len_eff[b] = nb > 0 ? qvc::counted_len(h, b, nb) : 0; }
      if (h.pos_add && nb > 0) h.pos_add[b] += nb;
    }
    for (int i = 0; i < n; ++i) {
      const qvc::CountedDesc& c = d[i];
      for (int b = 0; b < h.slots; ++b) {
        const size_t nb = (size_t)qvc::tick_count(h.n_new, b, h.hop);
        if (nb == 0 && !(c.flags & qvc::kCountedIdleZero)) continue;
        const size_t valid = nb == 0 ? 0 : c.fixed + nb * c.unit;
        for (size_t r = 0; r < c.rows; ++r) {
          char* dst = static_cast<char*>(c.dst) + ((size_t)b * c.rows + r) * c.dpitch;
          if (valid) std::memcpy(dst, static_cast<const char*>(c.src) + ((size_t)b * c.rows + r) * c.spitch + nb * c.shift, valid);
          std::memset(dst + valid, 0, c.width - valid);
        }
      }
    }
    return QVC_OK;
  }
};

// calls of copy_batch, descriptors in them, and two words that stay 0 (the launches of a mechanism that is gone: the
// recorded rows keep their four-word shape) -- since qvc_emu_twin_counts
int64_t g_counts[4] = {0, 0, 0, 0};
int64_t g_counted[2] = {0, 0};      // calls of copy_counted, descriptors in them -- since qvc_emu_stream_tick_counts

struct CountingBackend : TickEmuBackend {
  int copy_batch(const qvc::CopyDesc* d, int n) { ++g_counts[0]; g_counts[1] += n; return TickEmuBackend::copy_batch(d, n); }
  int copy_counted(const qvc::CountedHead& h, const qvc::CountedDesc* d, int n) { ++g_counted[0]; g_counted[1] += n; return TickEmuBackend::copy_counted(h, d, n); }
};

// The backend of qvc_emu_infer_windows_fm: states kWindows and restates the two table-driven kernels of
// csrc/qvc_small.hip (window_gather_kernel, window_deliver_kernel) in plain C++, row by row on the same clamp (window_row).
struct WindowsEmuBackend : CountingBackend {
  static constexpr bool kWindows = true;
  int window_gather(const qvc::WindowArgs& a) {
    if (!a.win || !a.unit_packed || !a.unit_win || !a.pos_eff || !a.len_eff || (a.noise_packed && !a.noise_win)) return QVC_ERR_BAD_ARG;
    for (int r = 0; r < a.rows; ++r) {
      const qvc::WindowRow w = qvc::window_row(a.win, r, a.n, a.total);
      a.pos_eff[r] = w.count > 0 ? w.start + a.C : a.W;
      a.len_eff[r] = w.count > 0 ? w.length : 0;
      if (w.count == 0) continue;
      const size_t Cu = (size_t)a.unit_channels, W = (size_t)a.W;
      for (size_t i = 0; i < W; ++i) {
        const int f = w.start - a.C + (int)i;
        float* dst = a.unit_win + ((size_t)r * W + i) * Cu;
        if (f >= 0 && f < w.length) std::memcpy(dst, a.unit_packed + ((size_t)w.base + (size_t)f) * Cu, Cu * 4);
        else std::fill(dst, dst + Cu, 0.f);
      }
      if (!a.noise_packed) continue;
      for (size_t c = 0; c < (size_t)a.inter; ++c)
        for (size_t i = 0; i < W; ++i) {
          const int f = w.start - a.C + (int)i;
          a.noise_win[((size_t)r * a.inter + c) * W + i] = f >= 0 && f < w.length ? a.noise_packed[c * (size_t)a.total + (size_t)w.base + (size_t)f] : 0.f;
        }
    }
    return QVC_OK;
  }
  int window_deliver(const qvc::WindowArgs& a) {
    if (!a.win || !a.wave || !a.out_packed || a.wave_rows < a.first + a.n) return QVC_ERR_BAD_ARG;
    for (int r = 0; r < a.rows; ++r) {
      const qvc::WindowRow w = qvc::window_row(a.win, r, a.n, a.total);
      if (w.count > 0)
        std::memcpy(a.out_packed + ((size_t)w.base + (size_t)w.start) * a.spf, a.wave + ((size_t)r * a.wave_rows + a.first) * a.spf,
                    (size_t)w.count * a.spf * 4);
    }
    return QVC_OK;
  }
};

bool g_trim = true;

int live_rings_of(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead, qvc::Rings& R) {
  qvc::Plan P; qvc::LiveGeom G;
  const int gs = qvc::live_plan(cfg, hop, look_ahead, P, G);
  if (gs == QVC_OK) R = qvc::live_rings(P, G, batch);
  return gs;
}

// qvc_emu_live_step (n_new == nullptr) and qvc_emu_live_tick: the checks of the C ABI's scaffold, then the driver
int live_call(const qvc_config* cfg, const void* blob, void* state, int64_t state_bytes, const float* unit_new, const float* g,
              const float* noise_new, float* out, int32_t batch, int32_t hop, int32_t look_ahead, bool tick, const int32_t* n_new,
              int32_t* pos, const int32_t* lens, void* workspace, int64_t workspace_bytes) {
  qvc::Plan P; qvc::LiveGeom G;
  const int st = qvc::stream_checks(blob && state && unit_new && g && noise_new && out && (n_new || !tick) && pos && lens && workspace, batch,
                                    state_bytes, workspace_bytes, [&](qvc::StreamBytes& b) {
    const int gs = qvc::live_plan(cfg, hop, look_ahead, P, G);
    if (gs == QVC_OK) b = {qvc::carve_live_state(P, G, batch).bytes, qvc::carve_live_scratch(P, G, batch, tick).bytes};
    return gs;
  });
  if (st != QVC_OK) return st;
  CountingBackend be;
  const char* w = static_cast<const char*>(blob);
  char* s = static_cast<char*>(state);
  char* ws = static_cast<char*>(workspace);
  return tick ? qvc::live_tick(P, G, w, s, ws, unit_new, g, noise_new, out, batch, n_new, pos, lens, be, nullptr, g_trim)
              : qvc::live_step(P, G, w, s, ws, unit_new, g, noise_new, out, batch, pos, lens, be, nullptr, g_trim);
}

// qvc_emu_twin_stream_step (tick == false) and qvc_emu_stream_tick on backend `be`: the checks of the C ABI's scaffold,
// then the driver
template <class Backend>
int stream_call(Backend& be, const qvc_config* cfg, const void* blob, void* state, int64_t state_bytes, const float* unit_new,
                const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, bool tick, const int32_t* n_new,
                int32_t* pos, const int32_t* lens, void* workspace, int64_t workspace_bytes) {
  qvc::Plan P; qvc::StreamGeom G;
  const int st = qvc::stream_checks(blob && state && unit_new && g && noise_new && out && (n_new || !tick) && pos && lens && workspace, batch,
                                    state_bytes, workspace_bytes, [&](qvc::StreamBytes& b) {
    const int gs = qvc::stream_plan(cfg, hop, P, G);
    if (gs == QVC_OK) b = {qvc::carve_stream_state(P, G, batch).bytes, qvc::carve_stream_scratch(P, G, batch, tick).bytes};
    return gs;
  });
  if (st != QVC_OK) return st;
  const char* w = static_cast<const char*>(blob);
  char* s = static_cast<char*>(state);
  char* ws = static_cast<char*>(workspace);
  return tick ? qvc::stream_tick(P, w, s, ws, unit_new, g, noise_new, out, batch, hop, n_new, pos, lens, be)
              : qvc::stream_step(P, w, s, ws, unit_new, g, noise_new, out, batch, hop, pos, lens, be);
}

// The recording backend of qvc_emu_stream_moves: every copy_batch / copy_counted call of one driver call, written down in
// call order and then forwarded, so the run stays a real run.  A pointer is two words, (region, byte offset): the index
// of the buffer of the call it points into -- the order of kMoveRegions -- or kMoveNull with offset 0.  One call is
//   copy_batch:    0, n, then per descriptor  dst, src, dpitch, spitch, width, rows
//   copy_counted:  1, n, slots, hop, idle_pos, n_new, pos, lens, pos_eff, len_eff, pos_add, then per descriptor
//                  dst, src, dpitch, spitch, fixed, unit, shift, width, rows, flags
// tests/golden/make_golden_stream_moves.py reads this layout.
constexpr int kMoveRegions = 8;        // state, workspace, unit_new, noise_new, out, pos, lens, n_new
constexpr int kMoveNull = kMoveRegions;
constexpr int kMoveOutside = -100;     // qvc_emu_stream_moves: a pointer outside every region
struct MoveRegion { const void* base; int64_t bytes; };
struct RecordingBackend : CountingBackend {
  std::array<MoveRegion, kMoveRegions> region = {};
  std::vector<int64_t> words;
  bool outside = false;
  void ptr(const void* p) {
    int r = p ? -1 : kMoveNull;
    int64_t off = 0;
    for (int i = 0; p && i < kMoveRegions; ++i) {
      const int64_t d = static_cast<const char*>(p) - static_cast<const char*>(region[(size_t)i].base);
      if (region[(size_t)i].base && d >= 0 && d < region[(size_t)i].bytes) { r = i; off = d; break; }
    }
    outside = outside || r < 0;
    words.push_back(r); words.push_back(off);
  }
  int copy_batch(const qvc::CopyDesc* d, int n) {
    words.push_back(0); words.push_back(n);
    for (int i = 0; d && i < n; ++i) {
      ptr(d[i].dst); ptr(d[i].src);
      for (uint32_t v : {d[i].dpitch, d[i].spitch, d[i].width, d[i].rows}) words.push_back(v);
    }
    return CountingBackend::copy_batch(d, n);
  }
  int copy_counted(const qvc::CountedHead& h, const qvc::CountedDesc* d, int n) {
    for (int64_t v : {1, n, h.slots, h.hop, h.idle_pos}) words.push_back(v);
    for (const void* p : {(const void*)h.n_new, (const void*)h.pos, (const void*)h.lens, (const void*)h.pos_eff, (const void*)h.len_eff, (const void*)h.pos_add}) ptr(p);
    for (int i = 0; d && i < n; ++i) {
      ptr(d[i].dst); ptr(d[i].src);
      for (uint32_t v : {d[i].dpitch, d[i].spitch, d[i].fixed, d[i].unit, d[i].shift, d[i].width, d[i].rows, d[i].flags}) words.push_back(v);
    }
    return CountingBackend::copy_counted(h, d, n);
  }
};

// The recording backend of qvc_emu_path_trace: it computes nothing.  Every method of the backend contract (csrc/qvc_path.h)
// appends one record -- the call's name, its non-Args parameters, the ConvDesc fields the launchers read and EVERY field of
// its Args struct -- and returns QVC_OK, so a Path instantiated on it leaves the list of launches the GPU would be handed.
// A record is  kind (index into kTraceKinds), n, then n words.  A pointer is two words, (region, byte offset), as in
// RecordingBackend; a float is its bit pattern; everything else its value.  Each struct below is one PUT that lists its
// fields; the static_assert next to it fails when the struct grows, so a new field cannot be left out silently.  The
// words are named after the listing itself (PUT stringifies it): qvc_emu_path_trace_layout, for the golden generator's
// --dump and its coverage checks.
constexpr const char* kTraceKinds[] = {"conv", "pair3", "chain", "wn", "wn_stack", "gemv", "sample", "sample_rows", "tail", "post_tail", "zero",
                                       "fork", "branch", "branch_done", "join", "lstm", "spk_embed", "spk_map", "steps"};
constexpr int kTraceKindCount = (int)(sizeof(kTraceKinds) / sizeof(kTraceKinds[0]));
constexpr int kTraceSteps = kTraceKindCount - 1;     // the closing record of a Path form: the StepKind of every step
enum TraceRegion { TR_BLOB, TR_WORKSPACE, TR_UNIT, TR_G, TR_NOISE, TR_OUT, TR_LENS, TR_POS, TR_FRAMES, TR_SRC, TR_ROW_FRAMES, TR_KEYS, TR_MEL,
                   TR_Z, TR_STATE, TR_COUNT };     // TR_Z: z or spec; TR_STATE: the streaming use's stage-0 hand-over; TR_COUNT = null
#define PUT(...) put(#__VA_ARGS__, __VA_ARGS__)
struct TraceBackend {
  static constexpr bool kSingleBandTail = true, kFanout = true, kNoiseRng = true;
  std::array<MoveRegion, TR_COUNT> region = {};
  std::vector<int64_t> words;
  std::vector<std::string>* names = nullptr;     // layout mode: the name of every word
  std::string cur;
  bool outside = false;
  size_t open_at = 0;

  void word(int64_t v, const char* suffix = "") { words.push_back(v); if (names) names->push_back(cur + suffix); }
  void ptr(const void* p) {
    int r = p ? -1 : (int)TR_COUNT;
    int64_t off = 0;
    for (int i = 0; p && i < TR_COUNT; ++i) {
      const int64_t d = static_cast<const char*>(p) - static_cast<const char*>(region[(size_t)i].base);
      if (region[(size_t)i].base && d >= 0 && d < region[(size_t)i].bytes) { r = i; off = d; break; }
    }
    outside = outside || r < 0;
    word(r); word(off, "+");
  }
  // one argument of a PUT: an array element by element, a pointer as (region, offset), a float as its bits, an integer as
  // its value, a struct through its listing (fields)
  template <class T> void one(const T& v) {
    if constexpr (std::is_array_v<T>) {
      const std::string outer = cur;
      for (size_t i = 0; i < std::extent_v<T>; ++i) { cur = outer + "[" + std::to_string(i) + "]"; one(v[i]); }
      cur = outer;
    } else if constexpr (std::is_same_v<T, const qvc::ConvDesc*>) {
      const int has = v != nullptr;
      PUT(has); fields(v ? *v : qvc::ConvDesc());
    } else if constexpr (std::is_pointer_v<T>) {
      ptr(v);
    } else if constexpr (std::is_floating_point_v<T>) {
      const float f = (float)v; uint32_t u; std::memcpy(&u, &f, 4); word(u);
    } else if constexpr (std::is_arithmetic_v<T> || std::is_enum_v<T>) {
      word((int64_t)v);
    } else {
      fields(v);
    }
  }
  // `list` is the text of the arguments: word names are the field names, "a.x" -> "x", nested "rg.lens"
  template <class... A> void put(const char* list, const A&... a) {
    const std::string outer = cur;
    const char* p = list;
    auto next = [&] {
      while (*p == ' ' || *p == ',') ++p;
      const char* e = p;
      while (*e && *e != ',') ++e;
      std::string s(p, e);
      p = e;
      const size_t dot = s.find('.');
      return (outer.empty() ? "" : outer + ".") + (dot == std::string::npos ? s : s.substr(dot + 1));
    };
    ((cur = next(), one(a)), ...);
    cur = outer;
  }
  static_assert(sizeof(qvc::Ragged) == 32 && sizeof(qvc::NoiseRng) == 24, "list the new field below");
  void fields(const qvc::Ragged& a) { PUT(a.lens, a.pos, a.mul, a.add, a.off); }
  void fields(const qvc::NoiseRng& a) { PUT(a.keys, a.seed_lo, a.seed_hi, a.scale); }
  static_assert(sizeof(qvc::ConvArgs) == 352, "list the new field below");
  void fields(const qvc::ConvArgs& a) {
    PUT(a.x, a.x_kind, a.x_bs, a.x_ts, a.x_c0, a.Cin, a.CinP, a.T_in, a.slope_in, a.x2, a.x3, a.reflect, a.w, a.bias, a.bbias, a.bbias_bs,
        a.taps, a.dil, a.left, a.KS, a.nIt, a.nchunk, a.M, a.Nq, a.up_s, a.up_p, a.Cout, a.T_out, a.res, a.res_bs, a.res_ts, a.res_c0,
        a.res_sign, a.res16, a.y32, a.y32_bs, a.y32_ts, a.y32_c0, a.y_scale, a.y_accum, a.y16, a.y16_bs, a.y16_ts, a.slope_out, a.y32b,
        a.split, a.gau_H, a.noise, a.noise_bs, a.noise_ts, a.ksize, a.lp, a.rg, a.rng);
  }
  static_assert(sizeof(qvc::PairArgs) == 96, "list the new field below");
  void fields(const qvc::PairArgs& a) { PUT(a.x, a.bs, a.T, a.C, a.CP, a.w1, a.b1, a.w2, a.b2, a.k, a.dil, a.KS, a.nIt, a.slope, a.y); }
  // the ConvDesc fields the launchers read
  void fields(const qvc::ConvDesc& d) { PUT(d.MF, d.WM, d.nchunk, d.lp, d.gau, d.M, d.taps); }
  static_assert(sizeof(qvc::LaunchChoice) == 104, "list the new field below");
  void fields(const qvc::LaunchChoice& c) {
    PUT(c.status, c.family, c.op, c.ts, c.MF, c.NF, c.WM, c.waves, c.epi, c.cl, c.last, c.pm, c.bands, c.ring, c.halo, c.margin, c.NT, c.grid, c.block,
        c.lds, c.optin_above);
  }
  // descriptors [0, n) of a launch of up to three chains / pairs; the rest as a default descriptor
  struct Descs { const qvc::ConvDesc* d; int n; };
  void fields(const Descs& v) {
    const std::string outer = cur;
    for (int i = 0; i < 3; ++i) { cur = outer + "[" + std::to_string(i) + "]"; fields(i < v.n && v.d ? v.d[i] : qvc::ConvDesc()); }
    cur = outer;
  }

  void open(int kind) { words.push_back(kind); words.push_back(0); open_at = words.size(); }
  int close() { words[open_at - 1] = (int64_t)(words.size() - open_at); return QVC_OK; }

  int conv(const qvc::ConvDesc& d, const qvc::ConvArgs& a, int batch, int epi, int dtype) { open(0); PUT(batch, epi, dtype, d, a); return close(); }
  static_assert(sizeof(qvc::PairArgs3) == 336, "list the new field below");
  int pair3(const qvc::ConvDesc* d1s, const qvc::ConvDesc* d2s, const qvc::PairArgs3& a, int batch, int dtype) {
    const Descs d1{d1s, a.n}, d2{d2s, a.n};
    open(1); PUT(batch, dtype, d1, d2, a.p, a.n, a.rg, a.chain_major); return close();
  }
  bool chain_ok(const qvc::ConvDesc* d1, const qvc::ConvDesc* d2, int n) const { return qvc::debug_get(qvc::DBG_PAIR_CHAIN3) != 0 && qvc::chain_supported(d1, d2, n); }
  static_assert(sizeof(qvc::ChainArgs) == 344, "list the new field below");
  int chain(const qvc::ConvDesc* d1s, const qvc::ConvDesc* d2s, const qvc::ChainArgs& a, int batch, int dtype) {
    const Descs d1{d1s, a.n}, d2{d2s, a.n};
    open(2); PUT(batch, dtype, d1, d2, a.p, a.n, a.rg, a.halo, a.margin, a.NT); return close();
  }
  static_assert(sizeof(qvc::WnArgs) == 136, "list the new field below");
  int wn(const qvc::ConvDesc& din, const qvc::ConvDesc& drs, const qvc::WnArgs& a, int batch, int dtype) {
    open(3);
    PUT(batch, dtype, din, drs, a.x_in, a.x_out, a.oacc, a.bs, a.T, a.H, a.HP, a.w_in, a.w_rs, a.b_rs, a.bbias, a.bbias_bs, a.taps, a.KS, a.nIt1, a.last, a.rg);
    return close();
  }
  int wn_stack_chunk(int layers) const { return qvc::wn_chunk(layers); }
  static_assert(sizeof(qvc::WnStackArgs) == 600, "list the new field below");
  int wn_stack(const qvc::ConvDesc& din, const qvc::ConvDesc& drs, const qvc::ConvDesc& drs_last, const qvc::WnStackArgs& a, int batch, int dtype,
               const qvc::ConvDesc* pre, const qvc::ConvDesc* post) {
    open(4);
    PUT(batch, dtype, din, drs, drs_last, pre, post, a.x0, a.out, a.bs, a.T, a.H, a.HP, a.w_in, a.w_rs, a.b_rs, a.bbias, a.bbias_bs, a.layers, a.taps,
        a.KS, a.nIt1, a.x_out, a.accum, a.final_layer, a.w_pre, a.b_pre, a.pre_cin, a.pre_c0, a.pre_KS, a.w_post, a.b_post, a.post_m, a.post_c0,
        a.post_mf, a.z, a.z_bs, a.z_ts, a.post_sign, a.rg, a.wide);
    return close();
  }
  static_assert(sizeof(qvc::GemvArgs) == 48, "list the new field below");
  int gemv(const qvc::GemvArgs& a) { open(5); PUT(a.w, a.bias, a.g, a.out, a.rows, a.gin, a.batch); return close(); }
  static_assert(sizeof(qvc::SampleArgs) == 80, "list the new field below");
  int sample(const qvc::SampleArgs& a) { open(6); PUT(a.stats, a.noise, a.z, a.batch, a.frames, a.C, a.rng, a.pos, a.off); return close(); }
  static_assert(sizeof(qvc::SampleRowsArgs) == 88, "list the new field below");
  int sample_rows(const qvc::SampleRowsArgs& a) {
    open(7); PUT(a.stats, a.noise, a.z, a.src, a.frames, a.row_frames, a.sources, a.rows, a.frames_max, a.C, a.rng); return close();
  }
  static_assert(sizeof(qvc::TailArgs) == 80, "list the new field below");
  int tail(const qvc::TailArgs& a) { open(8); PUT(a.post, a.fir, a.out, a.y_mb, a.batch, a.F, a.rg, a.bands); return close(); }
  bool post_tail_ok(const qvc::ConvDesc& d) const { return qvc::debug_get(qvc::DBG_POST_TAIL) != 0 && qvc::post_tail_supported(d); }
  static_assert(sizeof(qvc::PostTailArgs) == 408, "list the new field below");
  int post_tail(const qvc::ConvDesc& d, const qvc::PostTailArgs& a, int batch, int dtype) {
    open(9); PUT(batch, dtype, d, a.c, a.fir, a.out, a.F, a.rg); return close();
  }
  int zero(void* ptr, size_t bytes) { open(10); PUT(ptr, bytes); return close(); }
  void fork(int n) { open(11); PUT(n); close(); }
  void branch(int j) { open(12); PUT(j); close(); }
  void branch_done(int j) { open(13); PUT(j); close(); }
  void join(int n) { open(14); PUT(n); close(); }
  static_assert(sizeof(qvc::LstmArgs) == 88, "list the new field below");
  int lstm(const qvc::LstmArgs& a, int KS, int dtype) {
    open(15); PUT(KS, dtype, a.xp, a.shared, a.F, a.n_part, a.S, a.P, a.H, a.w_hh, a.hseq, a.hfin, a.prow, a.pstart, a.psteps, a.phdr); return close();
  }
  static_assert(sizeof(qvc::SpkEmbedArgs) == 56, "list the new field below");
  int spk_embed(const qvc::SpkEmbedArgs& a) { open(16); PUT(a.hfin, a.lw, a.lb, a.g, a.utterances, a.n_part, a.H, a.poff); return close(); }
  static_assert(sizeof(qvc::SpkMapArgs) == 72, "list the new field below");
  int spk_map(const qvc::SpkMapArgs& a) { open(17); PUT(a.frames, a.U, a.F, a.P, a.flen, a.poff, a.prow, a.pstart, a.psteps, a.phdr); return close(); }
};

// The recording backend of qvc_emu_launch_trace: the same walk, but what it writes down of a call is the CHOICE the
// chooser of its kernel family returns (csrc/qvc_select.h: choose_*, every field of LaunchChoice), behind the few inputs
// the rules read and the record names of the timed entry point are built from.  The calls that are not one of the six
// families leave a record without words (tail: its bands), so that the list stays the list of launches.  The chooser is
// asked, nothing is refused: a choice's status is a word of the record like any other.
struct SelectBackend : TraceBackend {
  // the choice, and whether its tuple is one the library instantiates (the family's *_built)
  int chosen(const qvc::LaunchChoice& c) { const int built = qvc::choice_built(c); PUT(c, built); return close(); }
  int conv(const qvc::ConvDesc& d, const qvc::ConvArgs& a, int batch, int epi, int dtype) {
    const int up_s = d.up_s, nchunk = d.nchunk, Nq = a.Nq, mean3 = a.x2 != nullptr;
    const qvc::LaunchChoice c = qvc::choose_conv(d, a, batch, epi, dtype);
    open(0); PUT(batch, epi, dtype, up_s, nchunk, Nq, mean3); return chosen(c);
  }
  int pair3(const qvc::ConvDesc* d1, const qvc::ConvDesc* d2, const qvc::PairArgs3& a, int batch, int dtype) {
    const int T = a.p[0].T;
    const qvc::LaunchChoice c = qvc::choose_pair(d1, d2, a, batch, dtype);
    open(1); PUT(batch, dtype, a.n, a.chain_major, T); return chosen(c);
  }
  int chain(const qvc::ConvDesc* d1, const qvc::ConvDesc* d2, const qvc::ChainArgs& a, int batch, int dtype) {
    const int T = a.p[0].T, k = d1 ? d1[0].taps : 0;
    const qvc::LaunchChoice c = d1 ? qvc::choose_chain(d1, d2, a, batch, dtype) : qvc::LaunchChoice();
    open(2); PUT(batch, dtype, a.n, T, k); return chosen(c);
  }
  int wn(const qvc::ConvDesc& din, const qvc::ConvDesc&, const qvc::WnArgs& a, int batch, int dtype) {
    const int W = din.WM;
    const qvc::LaunchChoice c = qvc::choose_wn(din, a, batch, dtype);
    open(3); PUT(batch, dtype, a.T, W); return chosen(c);
  }
  int wn_stack(const qvc::ConvDesc& din, const qvc::ConvDesc&, const qvc::ConvDesc&, const qvc::WnStackArgs& a, int batch, int dtype,
               const qvc::ConvDesc* pre, const qvc::ConvDesc*) {
    const int W = din.WM, fused = pre != nullptr;
    const qvc::LaunchChoice c = qvc::choose_wn_stack(din, a, batch, dtype);
    open(4); PUT(batch, dtype, a.T, a.layers, a.wide, fused, W); return chosen(c);
  }
  int gemv(const qvc::GemvArgs&) { open(5); return close(); }
  int sample(const qvc::SampleArgs&) { open(6); return close(); }
  int sample_rows(const qvc::SampleRowsArgs&) { open(7); return close(); }
  int tail(const qvc::TailArgs& a) { open(8); PUT(a.bands); return close(); }
  int post_tail(const qvc::ConvDesc& d, const qvc::PostTailArgs& a, int batch, int dtype) {
    const qvc::LaunchChoice c = qvc::choose_post_tail(d, a, batch, dtype);
    open(9); PUT(batch, dtype, a.F); return chosen(c);
  }
  int zero(void*, size_t) { open(10); return close(); }
  void fork(int) { open(11); close(); }
  void branch(int) { open(12); close(); }
  void branch_done(int) { open(13); close(); }
  void join(int) { open(14); close(); }
  int lstm(const qvc::LstmArgs&, int, int) { open(15); return close(); }
  int spk_embed(const qvc::SpkEmbedArgs&) { open(16); return close(); }
  int spk_map(const qvc::SpkMapArgs&) { open(17); return close(); }
};
#undef PUT

// the forms of qvc_emu_path_trace, in the order of its `form` argument
enum TraceForm { TF_UNIFORM, TF_RAGGED_FM, TF_RAGGED_RNG, TF_FANOUT, TF_FANOUT_RNG, TF_ENC_Q, TF_FLOW_FORWARD, TF_ENC_P, TF_DEC_TRUNK, TF_STREAM_DEC,
                 TF_SPK, TF_SPK_RAGGED, TF_COUNT };
constexpr int kTraceSwitches = 5;      // pair_chain3, post_tail, wn_chunk (the emulation's three), pair_cm4, pair_wide_launch
// ... and, for the launch trace, the three the choosers read (csrc/qvc_select.h)
constexpr int kSelectSwitches = 8;
constexpr int kTraceSwitch[kSelectSwitches] = {qvc::DBG_PAIR_CHAIN3, qvc::DBG_POST_TAIL, qvc::DBG_WN_CHUNK, qvc::DBG_PAIR_CM4, qvc::DBG_PAIR_WIDE_LAUNCH,
                                               qvc::DBG_CONV_CL, qvc::DBG_POST_TAIL_NF, qvc::DBG_WN_KERNEL};

// One form of the path (TraceForm) for (cfg, B rows of T frames; U sources of a fan-out, U utterances of T mel frames of
// the speaker forms) on the recording backend: rec[0, *used) receives every backend call in order (TraceBackend states the
// layout), closed for the Path forms by a "steps" record that holds the StepKind of every step.  The buffers are sized as
// the entry points of include/qvc.h ask and never read or written.  switches (null: the defaults) = the values of
// kTraceSwitch for the call, set in this library's own debug table and put back before it returns.
// QVC_ERR_SMALL_BUFFER: more than `cap` words; kMoveOutside: a launch named a pointer outside every buffer of the call.
// (the body of qvc_emu_path_trace and qvc_emu_launch_trace: Backend = what a call leaves in the record, n_sw = the first
//  n_sw switches of kTraceSwitch come with the call)
template <class Backend>
int trace_form(const qvc_config* cfg, int32_t form, int32_t B, int32_t T, int32_t U, const int32_t* switches, int n_sw, int64_t* rec, int64_t cap,
               int64_t* used) {
  using namespace qvc;
  if (!cfg || !rec || !used || form < 0 || form >= TF_COUNT || B <= 0 || T <= 1 || U <= 0) return QVC_ERR_BAD_ARG;
  const bool spk = form == TF_SPK || form == TF_SPK_RAGGED;
  const Plan P = build_plan(*cfg);
  const EncQPlan Q = build_encq_plan(*cfg);
  const SpkPlan S = build_spk_plan(*cfg);
  const int plan_status = spk ? S.status : (form == TF_ENC_Q ? Q.status : P.status);
  if (plan_status != QVC_OK) return plan_status;
  const Workspace W = spk ? Workspace() : carve_workspace(P, B, T);
  const SpkWorkspace SW = form == TF_SPK ? carve_spk_workspace(S, U, T) : carve_spk_ragged_workspace(S, U, T);
  const int64_t rows = std::max(B, U), C = cfg->inter_channels, t0 = spk ? 0 : (int64_t)T * P.stages[0].rate;
  std::array<int64_t, TR_COUNT> bytes = {};
  bytes[TR_BLOB] = spk ? S.blob_bytes : (form == TF_ENC_Q ? Q.blob_bytes : P.blob_bytes);
  bytes[TR_WORKSPACE] = spk ? SW.bytes : W.bytes;
  bytes[TR_UNIT] = rows * cfg->unit_channels * T * 4;
  bytes[TR_G] = rows * cfg->gin_channels * 4;
  bytes[TR_NOISE] = rows * C * T * 4;
  bytes[TR_OUT] = spk ? 0 : rows * std::max<int64_t>({(int64_t)T * samples_per_frame(P), ((int64_t)T * P.total_up + 1) * P.post_channels, T * C}) * 4;
  bytes[TR_LENS] = bytes[TR_POS] = bytes[TR_FRAMES] = bytes[TR_SRC] = bytes[TR_ROW_FRAMES] = rows * 4;
  bytes[TR_KEYS] = rows * 8;
  bytes[TR_MEL] = rows * S.n_mel * T * 4;
  bytes[TR_Z] = rows * std::max<int64_t>(C, Q.spec_channels) * T * 4;
  bytes[TR_STATE] = spk ? 0 : 3 * rows * t0 * P.stages[0].ch * 2;
  Backend be;
  std::array<void*, TR_COUNT> buf = {};
  bool alloc_ok = true;
  for (int i = 0; i < TR_COUNT; ++i) {
    buf[(size_t)i] = std::malloc((size_t)std::max<int64_t>(bytes[(size_t)i], 1));
    alloc_ok = alloc_ok && buf[(size_t)i];
    be.region[(size_t)i] = {buf[(size_t)i], bytes[(size_t)i]};
  }
  auto f32 = [&](int r) { return static_cast<float*>(buf[(size_t)r]); };
  auto i32 = [&](int r) { return static_cast<int32_t*>(buf[(size_t)r]); };
  int32_t saved[kSelectSwitches];
  for (int i = 0; i < n_sw; ++i) {
    saved[i] = debug_get(kTraceSwitch[i]);
    if (switches) debug_table()[kTraceSwitch[i]].store(switches[i], std::memory_order_relaxed);
  }
  int st = alloc_ok ? QVC_OK : QVC_ERR_BAD_ARG;
  std::vector<int32_t> kinds(4096, -1);
  int steps = 0;
  if (st == QVC_OK && spk) {
    const char* blob = static_cast<const char*>(buf[TR_BLOB]);
    char* ws = static_cast<char*>(buf[TR_WORKSPACE]);
    st = form == TF_SPK ? spk_path(S, dec_dtype(*cfg), blob, ws, SW, f32(TR_MEL), f32(TR_G), U, T, be)
                        : spk_path_ragged(S, dec_dtype(*cfg), blob, ws, SW, f32(TR_MEL), i32(TR_FRAMES), f32(TR_G), U, T, be);
  } else if (st == QVC_OK) {
    NoiseRng rng;
    rng.keys = static_cast<const uint64_t*>(buf[TR_KEYS]); rng.seed_lo = 0x1234567u; rng.seed_hi = 0x89abcdeu; rng.scale = 0.75f;
    auto path = [&] {
      Path<Backend> c{P, static_cast<const char*>(buf[TR_BLOB]), static_cast<char*>(buf[TR_WORKSPACE]), W, B, T, be};
      c.step_n = steps; c.step_kinds = kinds.data(); c.max_step_kinds = (int)kinds.size();
      return c;
    };
    Path<Backend> c = path();
    switch (form) {
      case TF_UNIFORM: c.infer(f32(TR_UNIT), f32(TR_G), f32(TR_NOISE), f32(TR_OUT)); break;
      case TF_RAGGED_FM: c.lens = i32(TR_LENS); c.unit_fm = true; c.infer(f32(TR_UNIT), f32(TR_G), f32(TR_NOISE), f32(TR_OUT)); break;
      case TF_RAGGED_RNG: c.lens = i32(TR_LENS); c.rng = rng; c.infer(f32(TR_UNIT), f32(TR_G), nullptr, f32(TR_OUT)); break;
      case TF_FANOUT:
        c.infer_fanout(f32(TR_UNIT), i32(TR_FRAMES), i32(TR_SRC), U, f32(TR_G), f32(TR_NOISE), f32(TR_OUT), i32(TR_ROW_FRAMES));
        break;
      case TF_FANOUT_RNG:
        c.unit_fm = true; c.rng = rng;
        c.infer_fanout(f32(TR_UNIT), i32(TR_FRAMES), i32(TR_SRC), U, f32(TR_G), nullptr, f32(TR_OUT), i32(TR_ROW_FRAMES));
        break;
      case TF_ENC_Q: c.enc_q(Q, c.blob, f32(TR_Z), f32(TR_G), f32(TR_NOISE), f32(TR_OUT)); break;
      case TF_FLOW_FORWARD: c.cond_table(f32(TR_G)); c.flow(f32(TR_Z), /*forward=*/true); break;
      case TF_ENC_P: c.enc_p(f32(TR_UNIT), f32(TR_NOISE), f32(TR_Z)); break;
      case TF_DEC_TRUNK: c.cond_table(f32(TR_G)); c.dec_trunk(f32(TR_Z), f32(TR_OUT)); break;
      default: {   // TF_STREAM_DEC: two segments of a streaming step, as Segments::make sets them up (csrc/qvc_stream.h)
        c.lens = i32(TR_LENS); c.pos = i32(TR_POS); c.off = 7; c.wn_wide = false;
        c.dec_front(f32(TR_Z));
        st = c.status; steps = c.step_n;
        Path<Backend> d = path();
        d.lens = i32(TR_LENS); d.pos = i32(TR_POS); d.off = 11; d.wn_wide = false;
        for (int j = 0; j < 3; ++j) d.s0_override[j] = static_cast<char*>(buf[TR_STATE]) + (int64_t)j * rows * t0 * P.stages[0].ch * 2;
        if (st == QVC_OK) { d.dec_back_wave(d.template wsp<float>(d.W.post), f32(TR_OUT)); st = d.status; steps = d.step_n; }
        break;
      }
    }
    if (form != TF_STREAM_DEC) { st = c.status; steps = c.step_n; }
    if (steps > (int)kinds.size()) st = QVC_ERR_SMALL_BUFFER;
    be.open(kTraceSteps);
    for (int i = 0; st == QVC_OK && i < steps; ++i) be.words.push_back(kinds[(size_t)i]);
    be.close();
  }
  for (int i = 0; i < n_sw; ++i) debug_table()[kTraceSwitch[i]].store(saved[i], std::memory_order_relaxed);
  for (void* p : buf) std::free(p);
  if (st != QVC_OK) return st;
  if (be.outside) return kMoveOutside;
  *used = (int64_t)be.words.size();
  if (*used > cap) return QVC_ERR_SMALL_BUFFER;
  std::memcpy(rec, be.words.data(), be.words.size() * sizeof(int64_t));
  return QVC_OK;
}

// The layout of the records of a trace as text, one line per kind: "<kind> <name of word 0> <name of word 1> ..."
// (a pointer is "<field>" "<field>+": region, offset).  Returns the bytes the text needs, the closing 0 included; the text
// is written when `cap` holds it.
template <class Backend>
int64_t trace_layout(char* text, int64_t cap) {
  using namespace qvc;
  std::vector<std::string> names;
  Backend be;
  be.names = &names;
  std::string out;
  auto line = [&](int kind) {
    out += kTraceKinds[kind];
    for (const std::string& n : names) out += " " + n;
    out += "\n";
    names.clear();
  };
  ConvDesc d[3];
  for (ConvDesc& x : d) x.CinP = kKStep;      // (a descriptor the choosers can size a tile for; the layout holds names only)
  int kind = 0;
  be.conv(d[0], ConvArgs(), 0, 0, 0); line(kind++);
  be.pair3(d, d, PairArgs3(), 0, 0); line(kind++);
  be.chain(d, d, ChainArgs(), 0, 0); line(kind++);
  be.wn(d[0], d[0], WnArgs(), 0, 0); line(kind++);
  be.wn_stack(d[0], d[0], d[0], WnStackArgs(), 0, 0, nullptr, nullptr); line(kind++);
  be.gemv(GemvArgs()); line(kind++);
  be.sample(SampleArgs()); line(kind++);
  be.sample_rows(SampleRowsArgs()); line(kind++);
  be.tail(TailArgs()); line(kind++);
  be.post_tail(d[0], PostTailArgs(), 0, 0); line(kind++);
  be.zero(nullptr, 0); line(kind++);
  be.fork(0); line(kind++);
  be.branch(0); line(kind++);
  be.branch_done(0); line(kind++);
  be.join(0); line(kind++);
  be.lstm(LstmArgs(), 0, 0); line(kind++);
  be.spk_embed(SpkEmbedArgs()); line(kind++);
  be.spk_map(SpkMapArgs()); line(kind++);
  line(kind++);      // "steps": one word per step, no names
  const int64_t need = (int64_t)out.size() + 1;
  if (text && cap >= need) std::memcpy(text, out.c_str(), (size_t)need);
  return need;
}

}  // namespace

extern "C" {

int qvc_emu_path_trace(const qvc_config* cfg, int32_t form, int32_t B, int32_t T, int32_t U, const int32_t* switches, int64_t* rec, int64_t cap,
                       int64_t* used) {
  return trace_form<TraceBackend>(cfg, form, B, T, U, switches, kTraceSwitches, rec, cap, used);
}
int64_t qvc_emu_path_trace_layout(char* text, int64_t cap) { return trace_layout<TraceBackend>(text, cap); }

// The same walk on SelectBackend: per launch-family call the choice its chooser returns.  switches: kSelectSwitches values,
// the five of qvc_emu_path_trace and then conv_cl, post_tail_nf, wn_kernel.
int qvc_emu_launch_trace(const qvc_config* cfg, int32_t form, int32_t B, int32_t T, int32_t U, const int32_t* switches, int64_t* rec, int64_t cap,
                         int64_t* used) {
  return trace_form<SelectBackend>(cfg, form, B, T, U, switches, kSelectSwitches, rec, cap, used);
}
int64_t qvc_emu_launch_trace_layout(char* text, int64_t cap) { return trace_layout<SelectBackend>(text, cap); }

// The library's debug switch "live_trim" for the twin: 1 (default) the trimmed form, 0 the plain one.  One switch, two names.
void qvc_emu_live_trim(int32_t on) { g_trim = on != 0; }
void qvc_emu_live_tick_trim(int32_t on) { g_trim = on != 0; }

// Same signature as qvc_live_step, host pointers, no stream.
int qvc_emu_live_step(const qvc_config* cfg, const void* blob, void* state, int64_t state_bytes, const float* unit_new,
                      const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, int32_t look_ahead,
                      const int32_t* pos, const int32_t* lens, void* workspace, int64_t workspace_bytes) {
  return live_call(cfg, blob, state, state_bytes, unit_new, g, noise_new, out, batch, hop, look_ahead, false, nullptr,
                   const_cast<int32_t*>(pos), lens, workspace, workspace_bytes);      // live_step only reads pos
}

// Same signature as qvc_live_tick, host pointers, no stream.
int qvc_emu_live_tick(const qvc_config* cfg, const void* blob, void* state, int64_t state_bytes, const float* unit_new,
                      const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, int32_t look_ahead,
                      const int32_t* n_new, int32_t* pos, const int32_t* lens, void* workspace, int64_t workspace_bytes) {
  return live_call(cfg, blob, state, state_bytes, unit_new, g, noise_new, out, batch, hop, look_ahead, true, n_new, pos, lens,
                   workspace, workspace_bytes);
}

// Same signature as qvc_infer_windows_fm, host pointers (the table too), no stream: infer_windows (csrc/qvc_stream.h) on
// WindowsEmuBackend, trimmed or plain by qvc_emu_live_trim.  The pointer form only: the emulation has no generator.
int qvc_emu_infer_windows_fm(const qvc_config* cfg, const void* blob, const float* unit_fm_packed, const float* noise_packed,
                             const qvc_window* win, const float* g, float* out_packed, int32_t rows, int32_t window_frames,
                             int32_t total_frames, void* workspace, int64_t workspace_bytes) {
  WindowsEmuBackend be;
  return qvc::infer_windows(be, cfg, blob, unit_fm_packed, noise_packed, nullptr, win, g, out_packed, rows, window_frames, total_frames, workspace,
                            workspace_bytes, g_trim);
}

// ... and what a backend without kWindows gets from the same driver (the frozen one): nothing is touched.
int qvc_emu_infer_windows_frozen(const qvc_config* cfg, int32_t rows, int32_t window_frames) {
  EmuBackend be;
  char* a = reinterpret_cast<char*>(uintptr_t(1) << 20);     // any aligned non-null address: never followed
  return qvc::infer_windows(be, cfg, a, reinterpret_cast<const float*>(a), reinterpret_cast<const float*>(a), nullptr,
                            reinterpret_cast<const qvc_window*>(a), reinterpret_cast<const float*>(a), reinterpret_cast<float*>(a), rows,
                            window_frames, 1, a, INT64_MAX, true);
}

// Same signature as qvc_infer_batch_ragged_fm, host pointers, no stream: the frozen emulation's whole path over units as
// they are on disk ([B][max_frames][unit_channels]) -- what a window's delivered frames are compared with.
int qvc_emu_infer_batch_ragged_fm(const qvc_config* cfg, const void* blob, const float* unit_fm, const float* g, const float* noise,
                                  float* out, int32_t batch, int32_t max_frames, const int32_t* frames_host, void* workspace,
                                  int64_t workspace_bytes) {
  if (!cfg || !blob || !unit_fm || !g || !noise || !out || !frames_host || !workspace || batch <= 0 || max_frames <= 1) return QVC_ERR_BAD_ARG;
  return std::min(0, run_path(cfg, blob, batch, max_frames, workspace, workspace_bytes, Window(), [&](qvc::Path<EmuBackend>& c) {
    c.lens = frames_host; c.unit_fm = true; c.infer(unit_fm, g, noise, out);
  }));
}

// Same signature as qvc_live_reset_slot / qvc_live_tick_reset_slot, host pointers, no stream.
int qvc_emu_live_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop, int32_t look_ahead,
                            int32_t slot, int32_t length, int32_t* pos, int32_t* lens) {
  const int st = qvc::reset_slot(state, state_bytes, batch, slot, length, pos, lens,
                                 [&](qvc::Rings& R) { return live_rings_of(cfg, batch, hop, look_ahead, R); },
                                 [](char* p, size_t n) { std::memset(p, 0, n); });
  if (st == QVC_OK) { pos[slot] = 0; lens[slot] = length; }
  return st;
}

int qvc_emu_live_tick_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop,
                                 int32_t look_ahead, int32_t slot, int32_t length, int32_t* pos, int32_t* lens) {
  return qvc_emu_live_reset_slot(cfg, state, state_bytes, batch, hop, look_ahead, slot, length, pos, lens);
}

// Byte offset and size of slot `slot`'s unit ring (which = 0) / noise ring (1) in the state: the tests compare an idle
// slot's ring bytes before and after a tick, and the kept W - hop frames of a slot's rows after a step and after a tick.
int qvc_emu_live_tick_ring(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead, int32_t slot, int32_t which,
                           int64_t* offset, int64_t* bytes) {
  if (!offset || !bytes || batch <= 0 || slot < 0 || slot >= batch || which < 0 || which > 1) return QVC_ERR_BAD_ARG;
  qvc::Rings R;
  const int gs = live_rings_of(cfg, batch, hop, look_ahead, R);
  if (gs != QVC_OK) return gs;
  const qvc::ByteRange s = qvc::slot_range(R.r[which], slot);
  *offset = s.off; *bytes = s.bytes;
  return QVC_OK;
}

// Same signature as qvc_emu_stream_step (the frozen emulation's export cannot count): stream_step on the counting backend.
int qvc_emu_twin_stream_step(const qvc_config* cfg, const void* blob, void* state, int64_t state_bytes, const float* unit_new,
                             const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, const int32_t* pos,
                             const int32_t* lens, void* workspace, int64_t workspace_bytes) {
  CountingBackend be;
  return stream_call(be, cfg, blob, state, state_bytes, unit_new, g, noise_new, out, batch, hop, false, nullptr,
                     const_cast<int32_t*>(pos), lens, workspace, workspace_bytes);    // stream_step only reads pos
}

// Same signature as qvc_stream_tick, host pointers, no stream.
int qvc_emu_stream_tick(const qvc_config* cfg, const void* blob, void* state, int64_t state_bytes, const float* unit_new,
                        const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, const int32_t* n_new,
                        int32_t* pos, const int32_t* lens, void* workspace, int64_t workspace_bytes) {
  CountingBackend be;
  return stream_call(be, cfg, blob, state, state_bytes, unit_new, g, noise_new, out, batch, hop, true, n_new, pos, lens, workspace,
                     workspace_bytes);
}

// One qvc_emu_twin_stream_step (n_new == nullptr) or one qvc_emu_stream_tick on the recording backend: the call runs as
// usual and rec[0, *used) receives every copy_batch / copy_counted call of it in order (RecordingBackend states the layout).
// QVC_ERR_SMALL_BUFFER: more than `cap` words; kMoveOutside: a launch named a pointer outside every buffer of the call.
int qvc_emu_stream_moves(const qvc_config* cfg, const void* blob, void* state, int64_t state_bytes, const float* unit_new,
                         const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, const int32_t* n_new,
                         int32_t* pos, const int32_t* lens, void* workspace, int64_t workspace_bytes, int64_t* rec, int64_t cap,
                         int64_t* used) {
  if (!rec || !used || !cfg || batch <= 0 || hop <= 0) return QVC_ERR_BAD_ARG;
  qvc::Plan P; qvc::StreamGeom G;
  const int gs = qvc::stream_plan(cfg, hop, P, G);
  if (gs != QVC_OK) return gs;
  const int64_t col = (int64_t)batch * hop * 4;
  RecordingBackend be;
  be.region = {{{state, state_bytes}, {workspace, workspace_bytes}, {unit_new, col * cfg->unit_channels}, {noise_new, col * cfg->inter_channels},
                {out, col * qvc::samples_per_frame(P)}, {pos, batch * 4}, {lens, batch * 4}, {n_new, n_new ? batch * 4 : 0}}};
  const int st = stream_call(be, cfg, blob, state, state_bytes, unit_new, g, noise_new, out, batch, hop, n_new != nullptr, n_new, pos, lens,
                             workspace, workspace_bytes);
  if (st != QVC_OK) return st;
  if (be.outside) return kMoveOutside;
  *used = (int64_t)be.words.size();
  if (*used > cap) return QVC_ERR_SMALL_BUFFER;
  std::memcpy(rec, be.words.data(), be.words.size() * sizeof(int64_t));
  return QVC_OK;
}

// The frozen backend, which does not state kStreamTick, through the same driver: what a backend without the hook gets.
int qvc_emu_stream_tick_frozen(const qvc_config* cfg, int32_t batch, int32_t hop) {
  qvc::Plan P; qvc::StreamGeom G;
  const int gs = qvc::stream_plan(cfg, hop, P, G);
  if (gs != QVC_OK) return gs;
  EmuBackend be;
  return qvc::stream_tick(P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, batch, hop, nullptr, nullptr, nullptr, be);
}

// ... and its sibling for the window.
int qvc_emu_live_tick_frozen(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead) {
  qvc::Plan P; qvc::LiveGeom G;
  const int gs = qvc::live_plan(cfg, hop, look_ahead, P, G);
  if (gs != QVC_OK) return gs;
  EmuBackend be;
  return qvc::live_tick(P, G, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, batch, nullptr, nullptr, nullptr, be);
}

// Same signature as qvc_stream_reset_slot, host pointers, no stream.
int qvc_emu_stream_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop, int32_t slot,
                              int32_t length, int32_t* pos, int32_t* lens) {
  const int st = qvc::reset_slot(state, state_bytes, batch, slot, length, pos, lens, [&](qvc::Rings& R) {
    qvc::Plan P; qvc::StreamGeom G;
    const int gs = qvc::stream_plan(cfg, hop, P, G);
    if (gs == QVC_OK) R = qvc::stream_rings(P, G, batch);
    return gs;
  }, [](char* p, size_t n) { std::memset(p, 0, n); });
  if (st == QVC_OK) { pos[slot] = 0; lens[slot] = length; }
  return st;
}

// Same signatures as qvc_stream_export_slots / qvc_stream_import_slots, host pointers, no stream: the same checks and the
// same descriptors (snapshot_slots of csrc/qvc_stream.h), run by the host copy_batch.
int qvc_emu_stream_export_slots(const qvc_config* cfg, const void* state, int64_t state_bytes, int32_t batch, int32_t hop,
                                const int32_t* slots, int32_t n_slots, const int32_t* pos, const int32_t* lens, void* snap, int64_t snap_bytes) {
  CountingBackend be;
  return qvc::snapshot_slots(false, be, cfg, const_cast<void*>(state), state_bytes, batch, hop, slots, n_slots, const_cast<int32_t*>(pos),
                             const_cast<int32_t*>(lens), snap, snap_bytes);
}

int qvc_emu_stream_import_slots(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop, const int32_t* slots,
                                int32_t n_slots, int32_t* pos, int32_t* lens, const void* snap, int64_t snap_bytes) {
  CountingBackend be;
  return qvc::snapshot_slots(true, be, cfg, state, state_bytes, batch, hop, slots, n_slots, pos, lens, const_cast<void*>(snap), snap_bytes);
}

// Ring `ring` of the segment rings' table for slot `slot`: v = {offset of the slot's rows in the state, their bytes
// (slot_range), rows per slot, kept bytes per row, new bytes per row}.  ring >= the table's size: QVC_ERR_BAD_ARG.
int qvc_emu_stream_ring(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t slot, int32_t ring, int64_t* v) {
  if (!v || batch <= 0 || slot < 0 || slot >= batch || ring < 0) return QVC_ERR_BAD_ARG;
  qvc::Plan P; qvc::StreamGeom G;
  const int gs = qvc::stream_plan(cfg, hop, P, G);
  if (gs != QVC_OK) return gs;
  const qvc::Rings R = qvc::stream_rings(P, G, batch);
  if (ring >= R.n) return QVC_ERR_BAD_ARG;
  const qvc::ByteRange s = qvc::slot_range(R.r[ring], slot);
  v[0] = s.off; v[1] = s.bytes; v[2] = R.r[ring].rows; v[3] = R.r[ring].keep; v[4] = R.r[ring].hopb;
  return QVC_OK;
}

// counts[2] = calls of copy_counted, descriptors in them since the last call of this function; the counts are cleared.
void qvc_emu_stream_tick_counts(int64_t* counts) {
  for (int i = 0; i < 2; ++i) { if (counts) counts[i] = g_counted[i]; g_counted[i] = 0; }
}

// counts[4] = calls of copy_batch, descriptors in them, 0, 0 since the last call of this function; the counts are cleared.
void qvc_emu_twin_counts(int64_t* counts) {
  for (int i = 0; i < 4; ++i) { if (counts) counts[i] = g_counts[i]; g_counts[i] = 0; }
}

}  // extern "C"
