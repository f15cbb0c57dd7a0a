// emu_twin.cpp -- TEST INFRASTRUCTURE: the CPU twin of qvc_live_step, qvc_live_tick and qvc_stream_tick.
//
// The host emulation under oracle/ is frozen, and its backend sits in an unnamed namespace of oracle/qvc_emu.cpp, so this
// translation unit includes that file.  The frozen EmuBackend does not state kLiveTick; TickEmuBackend derives from it,
// states the constant and adds host versions of the two launches a tick brackets the window with (csrc/qvc_small.hip:
// tick_rings_kernel, tick_deliver_kernel).  CountingBackend derives from that and counts the launches that move data
// (copy_batch, tick_rings, tick_deliver): live_step, live_tick and stream_step (csrc/qvc_stream.h) are instantiated on
// it, so a host test can pin how a step groups its copies into launches.  Built by build.py into
// oracle/_build/libqvc_emu_twin.so and loaded only by the tests.  The same backend states kStreamTick and adds the host
// version of the count-aware batched copy (csrc/qvc_small.hip: copy_counted_kernel), on which stream_tick is instantiated.
// RecordingBackend derives from CountingBackend and writes down every copy_batch / copy_counted call of one stream_step
// or stream_tick, descriptor by descriptor (qvc_emu_stream_moves; tests/test_stream_moves_host.py).  The emulation's
// backend has no single-band tail and no generator form of the noise: band-synthesis decoders, pointer form only.
#include "../oracle/qvc_emu.cpp"

#include <array>

namespace {

struct TickEmuBackend : EmuBackend {
  static constexpr bool kLiveTick = true;
  // a row is read whole before it is written, as the kernel's passes are
  static void shift_row(float* ring, const float* fresh, int W, int n) {
    std::vector<float> v((size_t)W);
    for (int r = 0; r < W; ++r) v[(size_t)r] = r < W - n ? ring[r + n] : fresh[r - (W - n)];
    std::memcpy(ring, v.data(), (size_t)W * 4);
  }
  int tick_rings(const qvc::TickRingsArgs& a) {
    if (!a.unit_ring || !a.unit_new || !a.n_new || !a.pos || !a.lens || !a.pos_eff || !a.len_eff) return QVC_ERR_BAD_ARG;
    if ((a.noise_ring == nullptr) != (a.noise_new == nullptr) || a.W <= a.hop || a.hop < 1) return QVC_ERR_BAD_ARG;
    for (int b = 0; b < a.B; ++b) {
      const int n = qvc::tick_count(a.n_new, b, a.hop);
      a.pos_eff[b] = n > 0 ? a.pos[b] + n - a.hop : a.W;
      a.len_eff[b] = n > 0 ? a.lens[b] : 0;
      if (n == 0) continue;
      for (int c = 0; c < a.UC; ++c) {
        const size_t row = (size_t)b * a.UC + c;
        shift_row(a.unit_ring + row * a.W, a.unit_new + row * a.hop, a.W, n);
      }
      for (int c = 0; a.noise_ring && c < a.NC; ++c) {
        const size_t row = (size_t)b * a.NC + c;
        shift_row(a.noise_ring + row * a.W, a.noise_new + row * a.hop, a.W, n);
      }
    }
    return QVC_OK;
  }
  int tick_deliver(const qvc::TickDeliverArgs& a) {
    if (!a.wave || !a.out || !a.n_new || !a.pos || a.first < 0 || a.first + a.hop > a.rows) return QVC_ERR_BAD_ARG;
    const size_t total = (size_t)a.hop * a.spf;
    for (int b = 0; b < a.B; ++b) {
      const int n = qvc::tick_count(a.n_new, b, a.hop);
      const float* src = a.wave + ((size_t)b * a.rows + (size_t)(a.first + a.hop - n)) * a.spf;
      float* dst = a.out + (size_t)b * total;
      for (size_t e = 0; e < total; ++e) dst[e] = e < (size_t)n * a.spf ? src[e] : 0.f;
      a.pos[b] += n;
    }
    return QVC_OK;
  }
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
      if (h.pos_eff) { h.pos_eff[b] = nb > 0 ? h.pos[b] : h.idle_pos; h.len_eff[b] = nb > 0 ? h.lens[b] : 0; }
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

// calls of copy_batch, descriptors in them, calls of tick_rings, calls of tick_deliver -- since qvc_emu_twin_counts
int64_t g_counts[4] = {0, 0, 0, 0};
int64_t g_counted[2] = {0, 0};      // calls of copy_counted, descriptors in them -- since qvc_emu_stream_tick_counts

struct CountingBackend : TickEmuBackend {
  int copy_batch(const qvc::CopyDesc* d, int n) { ++g_counts[0]; g_counts[1] += n; return TickEmuBackend::copy_batch(d, n); }
  int tick_rings(const qvc::TickRingsArgs& a) { ++g_counts[2]; return TickEmuBackend::tick_rings(a); }
  int tick_deliver(const qvc::TickDeliverArgs& a) { ++g_counts[3]; return TickEmuBackend::tick_deliver(a); }
  int copy_counted(const qvc::CountedHead& h, const qvc::CountedDesc* d, int n) { ++g_counted[0]; g_counted[1] += n; return TickEmuBackend::copy_counted(h, d, n); }
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

}  // namespace

extern "C" {

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
// slot's ring bytes before and after a tick.
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

// counts[4] = calls of copy_batch, descriptors in them, calls of tick_rings, calls of tick_deliver since the last call
// of this function; the counts are cleared.
void qvc_emu_twin_counts(int64_t* counts) {
  for (int i = 0; i < 4; ++i) { if (counts) counts[i] = g_counts[i]; g_counts[i] = 0; }
}

}  // extern "C"
