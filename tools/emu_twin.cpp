// emu_twin.cpp -- TEST INFRASTRUCTURE: the CPU twin of qvc_live_step and qvc_live_tick.
//
// The host emulation under oracle/ is frozen, and its backend sits in an unnamed namespace of oracle/qvc_emu.cpp, so this
// translation unit includes that file.  The frozen EmuBackend does not state kLiveTick; TickEmuBackend derives from it,
// states the constant and adds host versions of the two launches a tick brackets the window with (csrc/qvc_small.hip:
// tick_rings_kernel, tick_deliver_kernel).  CountingBackend derives from that and counts the launches that move data
// (copy_batch, tick_rings, tick_deliver): live_step, live_tick and stream_step (csrc/qvc_stream.h) are instantiated on
// it, so a host test can pin how a step groups its copies into launches.  Built by build.py into
// oracle/_build/libqvc_emu_twin.so and loaded only by the host tests.  The emulation's backend has no single-band tail
// and no generator form of the noise: band-synthesis decoders, pointer form only.
#include "../oracle/qvc_emu.cpp"

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
};

// calls of copy_batch, descriptors in them, calls of tick_rings, calls of tick_deliver -- since qvc_emu_twin_counts
int64_t g_counts[4] = {0, 0, 0, 0};

struct CountingBackend : TickEmuBackend {
  int copy_batch(const qvc::CopyDesc* d, int n) { ++g_counts[0]; g_counts[1] += n; return TickEmuBackend::copy_batch(d, n); }
  int tick_rings(const qvc::TickRingsArgs& a) { ++g_counts[2]; return TickEmuBackend::tick_rings(a); }
  int tick_deliver(const qvc::TickDeliverArgs& a) { ++g_counts[3]; return TickEmuBackend::tick_deliver(a); }
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
  qvc::Plan P; qvc::StreamGeom G;
  const int st = qvc::stream_checks(blob && state && unit_new && g && noise_new && out && pos && lens && workspace, batch, state_bytes,
                                    workspace_bytes, [&](qvc::StreamBytes& b) {
    const int gs = qvc::stream_plan(cfg, hop, P, G);
    if (gs == QVC_OK) b = {qvc::carve_stream_state(P, G, batch).bytes, qvc::carve_stream_scratch(P, G, batch).bytes};
    return gs;
  });
  if (st != QVC_OK) return st;
  CountingBackend be;
  return qvc::stream_step(P, static_cast<const char*>(blob), static_cast<char*>(state), static_cast<char*>(workspace), unit_new, g,
                          noise_new, out, batch, hop, pos, lens, be);
}

// counts[4] = calls of copy_batch, descriptors in them, calls of tick_rings, calls of tick_deliver since the last call
// of this function; the counts are cleared.
void qvc_emu_twin_counts(int64_t* counts) {
  for (int i = 0; i < 4; ++i) { if (counts) counts[i] = g_counts[i]; g_counts[i] = 0; }
}

}  // extern "C"
