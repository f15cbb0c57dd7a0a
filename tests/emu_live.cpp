// emu_live.cpp -- TEST INFRASTRUCTURE: the CPU twin of qvc_live_step.
//
// The host emulation under oracle/ is frozen, and its backend sits in an unnamed namespace of oracle/qvc_emu.cpp, so this
// translation unit includes that file and instantiates live_step (csrc/qvc_stream.h) on the same EmuBackend.  Built by
// build.py into oracle/_build/libqvc_emu_live.so and loaded only by tests/test_live_host.py.  The emulation's backend
// has no single-band tail and no generator form of the noise: band-synthesis decoders, pointer form only.
#include "../oracle/qvc_emu.cpp"

namespace { bool g_live_trim = true; }

extern "C" {

// The library's debug switch "live_trim" for the twin: 1 (default) the trimmed form, 0 the plain one.
void qvc_emu_live_trim(int32_t on) { g_live_trim = on != 0; }

// Same signature as qvc_live_step, host pointers, no stream.
int qvc_emu_live_step(const qvc_config* cfg, const void* blob, void* state, int64_t state_bytes, const float* unit_new,
                      const float* g, const float* noise_new, float* out, int32_t batch, int32_t hop, int32_t look_ahead,
                      const int32_t* pos, const int32_t* lens, void* workspace, int64_t workspace_bytes) {
  if (!blob || !state || !unit_new || !g || !noise_new || !out || !pos || !lens || !workspace || batch <= 0) return QVC_ERR_BAD_ARG;
  qvc::Plan P; qvc::LiveGeom G;
  const int gs = qvc::live_plan(cfg, hop, look_ahead, P, G);
  if (gs != QVC_OK) return gs;
  if (state_bytes < qvc::carve_live_state(P, G, batch).bytes || workspace_bytes < qvc::carve_live_scratch(P, G, batch).bytes)
    return QVC_ERR_SMALL_BUFFER;
  EmuBackend be;
  return qvc::live_step(P, G, static_cast<const char*>(blob), static_cast<char*>(state), static_cast<char*>(workspace), unit_new, g,
                        noise_new, out, batch, pos, lens, be, nullptr, g_live_trim);
}

// Same signature as qvc_live_reset_slot, host pointers, no stream.
int qvc_emu_live_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop, int32_t look_ahead,
                            int32_t slot, int32_t length, int32_t* pos, int32_t* lens) {
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

}  // extern "C"
