// emu_tick.cpp -- TEST INFRASTRUCTURE: the CPU twin of qvc_live_tick.
//
// As tests/emu_live.cpp: the host emulation under oracle/ is frozen and its backend sits in an unnamed namespace of
// oracle/qvc_emu.cpp, so this translation unit includes that file.  The frozen EmuBackend does not state kLiveTick; the
// backend here derives from it, states the constant and adds host versions of the two launches a tick brackets the
// window with (csrc/qvc_small.hip: tick_rings_kernel, tick_deliver_kernel), then live_tick (csrc/qvc_stream.h) is
// instantiated on it.  Built by build.py into oracle/_build/libqvc_emu_tick.so and loaded only by
// tests/test_live_tick_host.py.  Band-synthesis decoders, pointer form of the noise only, as the emulation.
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

bool g_tick_trim = true;

}  // namespace

extern "C" {

// The library's debug switch "live_trim" for the twin: 1 (default) the trimmed form, 0 the plain one.
void qvc_emu_live_tick_trim(int32_t on) { g_tick_trim = on != 0; }

// Same signature as qvc_live_tick, host pointers, no stream.
int qvc_emu_live_tick(const qvc_config* cfg, const void* blob, void* state, int64_t state_bytes, const float* unit_new,
                      const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, int32_t look_ahead,
                      const int32_t* n_new, int32_t* pos, const int32_t* lens, void* workspace, int64_t workspace_bytes) {
  if (!blob || !state || !unit_new || !g || !noise_new || !out || !n_new || !pos || !lens || !workspace || batch <= 0) return QVC_ERR_BAD_ARG;
  qvc::Plan P; qvc::LiveGeom G;
  const int gs = qvc::live_plan(cfg, hop, look_ahead, P, G);
  if (gs != QVC_OK) return gs;
  if (state_bytes < qvc::carve_live_state(P, G, batch).bytes || workspace_bytes < qvc::carve_tick_scratch(P, G, batch).bytes)
    return QVC_ERR_SMALL_BUFFER;
  TickEmuBackend be;
  return qvc::live_tick(P, G, static_cast<const char*>(blob), static_cast<char*>(state), static_cast<char*>(workspace), unit_new, g,
                        noise_new, out, batch, n_new, pos, lens, be, nullptr, g_tick_trim);
}

// Same signature as qvc_live_tick_reset_slot, host pointers, no stream.
int qvc_emu_live_tick_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop,
                                 int32_t look_ahead, int32_t slot, int32_t length, int32_t* pos, int32_t* lens) {
  if (!state || !pos || !lens || batch <= 0 || slot < 0 || slot >= batch || length < 0) return QVC_ERR_BAD_ARG;
  qvc::Plan P; qvc::LiveGeom G;
  const int gs = qvc::live_plan(cfg, hop, look_ahead, P, G);
  if (gs != QVC_OK) return gs;
  const qvc::LiveState S = qvc::carve_live_state(P, G, batch);
  if (state_bytes < S.bytes) return QVC_ERR_SMALL_BUFFER;
  const int64_t ub = (int64_t)P.cfg.unit_channels * G.W * 4, nb = (int64_t)P.cfg.inter_channels * G.W * 4;
  std::memset(static_cast<char*>(state) + S.unit + slot * ub, 0, (size_t)ub);
  std::memset(static_cast<char*>(state) + S.noise + slot * nb, 0, (size_t)nb);
  pos[slot] = 0; lens[slot] = length;
  return QVC_OK;
}

// Byte offset and size of slot `slot`'s unit ring (which = 0) / noise ring (1) in the state: the tests compare an idle
// slot's ring bytes before and after a tick.
int qvc_emu_live_tick_ring(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead, int32_t slot, int32_t which,
                           int64_t* offset, int64_t* bytes) {
  if (!offset || !bytes || batch <= 0 || slot < 0 || slot >= batch || which < 0 || which > 1) return QVC_ERR_BAD_ARG;
  qvc::Plan P; qvc::LiveGeom G;
  const int gs = qvc::live_plan(cfg, hop, look_ahead, P, G);
  if (gs != QVC_OK) return gs;
  const qvc::LiveState S = qvc::carve_live_state(P, G, batch);
  const int64_t per = (int64_t)(which ? P.cfg.inter_channels : P.cfg.unit_channels) * G.W * 4;
  *offset = (which ? S.noise : S.unit) + slot * per;
  *bytes = per;
  return QVC_OK;
}

}  // extern "C"
