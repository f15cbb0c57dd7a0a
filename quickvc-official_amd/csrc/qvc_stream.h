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
//
// Two bodies share this file, each ONE body on two movers -- the step, and the tick: the step with per-slot frame counts on
// the same state: stream_run (the segment rings above: stream_step and stream_tick) and live_run (one window over the
// whole path, below: live_step and live_tick).  What they share is stated once:
//   Rings         the ring table of a driver (stream_rings / live_rings): where every ring lies in the state and its
//                 geometry.  The state size, the slide buffers of the scratch, the slide loops and the per-slot reset
//                 (reset_slot, slot_range) all read the table, so a ring is added or resized in ONE place.  So do the
//                 snapshot of a slot (SnapLayout: the kept parts, pos and len) and its export / import (move_slots).
//   movers        the queue all data movement of a call goes through: CopyQueue in front of the backend's copy_batch
//                 (every slot moves by hop frames), CountedQueue in front of copy_counted (slot b moves by its n frames).
//                 Both speak the same verbs, rows always PER SLOT:
//                   fresh   a slot's new frames of this call (step: hop; tick: n, then zeros up to hop and a tail)
//                   kept    a fixed number of bytes per row;  slid: the same, read from the slot's new frames into the row on
//                   zeros   a zero fill
//                   append / slide_out / slide_back   a ring's new frames behind its kept ones; the kept parts out to the
//                           slide buffers and back in (RingMoves: written once on fresh / slid / kept)
//                   open    the pos / lens arrays the segments' launches read (prefix: a tick's sequence ends behind the
//                           slot's new frames);  advance: the stream positions move on
//                   flush   what was queued since the last flush runs as ONE launch;  ok / st: the first error
//   Segments      the factory of a step's Path segments.
//   stream_checks the pure-host checks of an entry point (the C ABI's scaffold in qvc_api.hip and the CPU twin call it).
// A third driver, at the end of the file, is offline: infer_windows runs live_window over windows cut from packed
// utterances of any lengths, named by a table in device memory (no state, no rings: one gather and one deliver launch).
#pragma once
#include "qvc_path.h"

namespace qvc {

// One-sided reach of a ResBlock stack in its own frames: the worst over the blocks of sum over pairs of (k-1)/2 * (d + 1).
inline int mrf_reach(const qvc_config& c) {
  int worst = 0;
  for (int j = 0; j < c.n_resblocks; ++j) {
    int s = 0;
    for (int q = 0; q < 3; ++q) s += (c.resblock_kernel_sizes[j] - 1) / 2 * (c.resblock_dilations[j][q] + 1);
    worst = std::max(worst, s);
  }
  return worst;
}

// A ring of the state buffer, batch-major: `rows` rows per stream of keep + hopb bytes each.  A step appends hopb bytes
// behind the first `keep` of every row and then slides the row left by hopb.
struct Ring { int64_t off, rows, keep, hopb; };

constexpr int kMaxRings = 1 + 16 + 1 + 3;   // the segment rings at the most coupling layers: unit, zf[0..16), zd, s0[0..3)
struct Rings {          // a driver's rings in the order they lie in the state; bytes = the state's size
  Ring r[kMaxRings] = {};
  int n = 0;
  Carver cv;
  void add(int B, int64_t rows, int64_t keep, int64_t hopb) { r[n++] = Ring{cv.take(B * rows * (keep + hopb)), rows, keep, hopb}; }
  int64_t bytes() const { return cv.off; }
  // the slide buffers of a step's scratch, one per ring: that ring's kept part
  void carve_tmp(Carver& x, int B, int64_t* tmp) const { for (int i = 0; i < n; ++i) tmp[i] = x.take(B * r[i].rows * r[i].keep); }
};

// Every ring is batch-major, so a stream's rows are one contiguous range per ring.
struct ByteRange { int64_t off, bytes; };
inline ByteRange slot_range(const Ring& r, int slot) {
  const int64_t per = r.rows * (r.keep + r.hopb);
  return ByteRange{r.off + slot * per, per};
}

// Starts a new stream in `slot` on the host side: the checks of every *_reset_slot entry point in their order, then
// zero(p, n) for the slot's range of every ring.  rings(R) -> status fills the driver's table.
template <class RingsFn, class Zero>
int reset_slot(void* state, int64_t state_bytes, int batch, int slot, int length, const void* pos, const void* lens, RingsFn rings, Zero zero) {
  if (!state || !pos || !lens || batch <= 0 || slot < 0 || slot >= batch || length < 0) return QVC_ERR_BAD_ARG;
  Rings R;
  const int gs = rings(R);
  if (gs != QVC_OK) return gs;
  if (state_bytes < R.bytes()) return QVC_ERR_SMALL_BUFFER;
  for (int i = 0; i < R.n; ++i) {
    const ByteRange s = slot_range(R.r[i], slot);
    zero(static_cast<char*>(state) + s.off, (size_t)s.bytes);
  }
  return QVC_OK;
}

// What a stream IS between two calls: the kept part of its rows of every ring, plus pos and len (stream_tick's INVARIANT: the
// hop part of a row is rewritten before it is read).  The snapshot of ONE slot, written once on the table: per ring, in
// table order, rows x keep bytes (a row's kept part, rows back to back), each ring 256-byte aligned; then pos and len as
// two int32.  It depends on the kept geometry only -- never on the batch, the slot or the hop of the state it is cut from.
struct SnapLayout {
  int64_t ring[kMaxRings] = {};   // byte offset of ring i's kept rows
  int64_t pos = 0;                // pos at this offset, len 4 bytes behind it
  int64_t bytes = 0;              // a multiple of 256: snapshots lie back to back
};
inline SnapLayout snap_layout(const Rings& R) {
  SnapLayout L;
  Carver cv;
  for (int i = 0; i < R.n; ++i) L.ring[i] = cv.take(R.r[i].rows * R.r[i].keep);
  L.pos = cv.take(8);
  L.bytes = cv.off;
  return L;
}

// The pure-host checks of a step / tick entry point, in the order the status codes are pinned to: pointers and batch,
// the plan (need(b) -> status fills the bytes the call needs), the two buffer sizes.
struct StreamBytes { int64_t state = 0, ws = 0; };
template <class NeedFn>
int stream_checks(bool ptrs_ok, int batch, int64_t state_bytes, int64_t ws_bytes, NeedFn need) {
  if (!ptrs_ok || batch <= 0) return QVC_ERR_BAD_ARG;
  StreamBytes b;
  const int gs = need(b);
  if (gs != QVC_OK) return gs;
  return state_bytes < b.state || ws_bytes < b.ws ? QVC_ERR_SMALL_BUFFER : QVC_OK;
}

// A mover's ring verbs, written once on its fresh / slid / kept (one frame of a ring row: hopb / hop bytes): a ring's
// new frames of this call behind its kept ones; then, for the first `count` rings of R, the kept parts out to the slide
// buffers -- from the slot's new frames into the row on -- and back in (out and back are two launches: a kept part and its
// destination overlap).
template <class Q>
struct RingMoves {
  Q& q() { return static_cast<Q&>(*this); }
  void append(char* state, const Ring& r, const void* src) {
    q().fresh(state + r.off + r.keep, (size_t)(r.keep + r.hopb), src, (size_t)r.hopb, (size_t)r.hopb / q().hop, (size_t)r.rows);
  }
  void slide_out(char* state, char* ws, const Rings& R, const int64_t* tmp, int count) {
    for (const Ring* r = R.r; r < R.r + count; ++r, ++tmp)
      q().slid(ws + *tmp, (size_t)r->keep, state + r->off, (size_t)(r->keep + r->hopb), (size_t)r->keep, (size_t)r->hopb / q().hop, (size_t)r->rows);
  }
  void slide_back(char* state, char* ws, const Rings& R, const int64_t* tmp, int count) {
    for (const Ring* r = R.r; r < R.r + count; ++r, ++tmp)
      q().kept(state + r->off, (size_t)(r->keep + r->hopb), ws + *tmp, (size_t)r->keep, (size_t)r->keep, (size_t)r->rows);
  }
};

struct StreamPos { const int32_t* pos; const int32_t* lens; };   // what open() returns

// The mover of a step: the queue in front of the backend's  int copy_batch(const CopyDesc* d, int n)  -- n independent
// strided copies / zero fills in one launch (qvc_kernels.h).  The descriptors between two flushes run as ONE launch and
// must be independent of each other; st is the first error.  Every slot moves by hop frames and every buffer is
// batch-major, so a verb's rows per slot become B * rows rows of one descriptor.
template <class Backend_>
struct CopyQueue : RingMoves<CopyQueue<Backend_>> {
  using Backend = Backend_;
  using Pos = const int32_t;                     // the caller advances pos
  static constexpr bool kTick = false;           // the scratch to carve
  Backend& be;
  const size_t B, hop;
  int st = QVC_OK;
  CopyDesc cd[kCopyBatchMax];
  int n = 0;
  CopyQueue(Backend& b, int slots, int hop_frames) : be(b), B((size_t)slots), hop((size_t)hop_frames) {}
  void ok(int rc) { if (st == QVC_OK && rc != QVC_OK) st = rc; }
  void flush() { if (n) ok(be.copy_batch(cd, n)); n = 0; }
  // queue a strided copy of `rows` rows in all (src == nullptr: zero fill): the low-level call
  void add(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows) {
    if (n == kCopyBatchMax) flush();
    if ((dpitch | spitch | width | rows) >> 32) { ok(QVC_ERR_BAD_ARG); return; }
    cd[n++] = CopyDesc{dst, src, (uint32_t)dpitch, (uint32_t)spitch, (uint32_t)width, (uint32_t)rows};
  }
  // hop frames of `frame` bytes each from the front of a source row; `tail` zero bytes behind them (a descriptor of its own)
  void fresh(void* dst, size_t dpitch, const void* src, size_t spitch, size_t frame, size_t rows, size_t tail = 0, uint32_t = 0) {
    add(dst, dpitch, src, spitch, hop * frame, B * rows);
    if (tail) zeros(static_cast<char*>(dst) + hop * frame, dpitch, tail, rows);
  }
  void kept(void* dst, size_t dpitch, const void* src, size_t spitch, size_t bytes, size_t rows) { add(dst, dpitch, src, spitch, bytes, B * rows); }
  void slid(void* dst, size_t dpitch, const void* src, size_t spitch, size_t bytes, size_t frame, size_t rows) {
    kept(dst, dpitch, static_cast<const char*>(src) + hop * frame, spitch, bytes, rows);
  }
  void zeros(void* dst, size_t dpitch, size_t width, size_t rows) { add(dst, dpitch, nullptr, 0, width, B * rows); }
  StreamPos open(const int32_t* pos, const int32_t* lens, int, int32_t*, int32_t*, bool = false) { return {pos, lens}; }
  void advance(const int32_t*) {}
};

// The mover of a tick: CopyQueue's sibling in front of the backend's  int copy_counted(const CountedHead&, const
// CountedDesc*, int n)  (qvc_kernels.h).  `head` carries the counts -- slot b moves by n = clamp(n_new[b], 0, hop) frames,
// decided on the device -- and, for ONE launch each, the tick's bookkeeping: open() and advance() set it for the next
// flush, which clears it.
template <class Backend_>
struct CountedQueue : RingMoves<CountedQueue<Backend_>> {
  using Backend = Backend_;
  using Pos = int32_t;                           // advanced here
  static constexpr bool kTick = true;
  Backend& be;
  const size_t hop;
  CountedHead head;
  int st = QVC_OK;
  CountedDesc cd[kCopyBatchMax];
  int n = 0;
  CountedQueue(Backend& b, const int32_t* n_new, int slots, int hop_frames) : be(b), hop((size_t)hop_frames) {
    head.n_new = n_new; head.slots = slots; head.hop = hop_frames;
  }
  void ok(int rc) { if (st == QVC_OK && rc != QVC_OK) st = rc; }
  void flush() {
    if (n) ok(be.copy_counted(head, cd, n));
    n = 0;
    head.pos = head.lens = nullptr; head.pos_eff = head.len_eff = head.pos_add = nullptr; head.len_cap = false;
  }
  // per slot `rows` rows: `fixed + n * unit` bytes from src (read from byte n * shift of the row on), zeros up to width
  void add(void* dst, size_t dpitch, const void* src, size_t spitch, size_t fixed, size_t unit, size_t shift, size_t width, size_t rows,
           uint32_t flags = 0) {
    if (n == kCopyBatchMax) flush();
    if ((dpitch | spitch | fixed | unit | shift | width | rows) >> 32) { ok(QVC_ERR_BAD_ARG); return; }
    cd[n++] = CountedDesc{dst, src, (uint32_t)dpitch, (uint32_t)spitch, (uint32_t)fixed, (uint32_t)unit, (uint32_t)shift, (uint32_t)width,
                          (uint32_t)rows, flags};
  }
  // n frames of `frame` bytes each from the front of a source row, then zeros up to hop frames and `tail` bytes
  void fresh(void* dst, size_t dpitch, const void* src, size_t spitch, size_t frame, size_t rows, size_t tail = 0, uint32_t flags = 0) {
    add(dst, dpitch, src, spitch, 0, frame, 0, hop * frame + tail, rows, flags);
  }
  void kept(void* dst, size_t dpitch, const void* src, size_t spitch, size_t bytes, size_t rows) { add(dst, dpitch, src, spitch, bytes, 0, 0, bytes, rows); }
  void slid(void* dst, size_t dpitch, const void* src, size_t spitch, size_t bytes, size_t frame, size_t rows) {
    add(dst, dpitch, src, spitch, bytes, 0, frame, bytes, rows);
  }
  void zeros(void* dst, size_t dpitch, size_t width, size_t rows) { add(dst, dpitch, nullptr, 0, 0, 0, 0, width, rows); }
  // the next launch writes what the segments see: n > 0: pos[b], lens[b];  n == 0: idle_pos, 0 (an empty sequence).
  // prefix: the sequence ends behind the slot's new frames, min(lens[b], pos[b] + n) (the window: live_run)
  StreamPos open(const int32_t* pos, const int32_t* lens, int idle_pos, int32_t* pos_eff, int32_t* len_eff, bool prefix = false) {
    head.pos = pos; head.lens = lens; head.pos_eff = pos_eff; head.len_eff = len_eff; head.idle_pos = idle_pos; head.len_cap = prefix;
    return {pos_eff, len_eff};
  }
  void advance(int32_t* pos) { head.pos_add = pos; }   // the next launch: pos[b] += n
};

// Export and import of slots, reset_slot's siblings: the copies between the state of `batch` slots (pos, lens beside it) and
// n snapshots back to back in `snap`, snapshot i <-> slot slots[i] (host array; every slot in [0, batch), distinct for an
// import), queued through CopyQueue in front of the backend's copy_batch -- nothing else is launched.  A ring of several
// rows per slot (the unit ring) is one strided descriptor per slot: rows x keep out of rows of keep + hopb.  A ring of one
// row per slot is one contiguous run per slot, so a run of consecutive slots is ONE descriptor whose rows are the slots
// (pitch: a slot's row in the state, a snapshot in `snap`); pos and len travel the same way as 4-byte copies.  All
// descriptors of a call are independent, so it does not matter where the queue flushes.
// Import writes the kept part of the named slots' rows, pos[slot] and lens[slot]; the hop parts and the other slots are
// left as they are.  Export only reads the state.
template <class Backend>
int move_slots(bool import, Backend& be, const Rings& R, char* state, const int32_t* slots, int n, int32_t* pos, int32_t* lens, char* snap) {
  const SnapLayout L = snap_layout(R);
  CopyQueue<Backend> q(be, 1, 1);
  auto mv = [&](char* st, int64_t st_pitch, char* sn, int64_t sn_pitch, int64_t width, int64_t rows) {
    if (import) q.add(st, (size_t)st_pitch, sn, (size_t)sn_pitch, (size_t)width, (size_t)rows);
    else q.add(sn, (size_t)sn_pitch, st, (size_t)st_pitch, (size_t)width, (size_t)rows);
  };
  int64_t widest = L.bytes;                                        // the widest pitch of a run descriptor
  for (int k = 0; k < R.n; ++k) widest = std::max(widest, R.r[k].keep + R.r[k].hopb);
  const int64_t max_run = std::max<int64_t>(1, ((int64_t)1 << 31) / widest);   // copy_batch: 32-bit offsets inside a descriptor
  for (int i = 0; i < n;) {
    int run = 1;
    while (i + run < n && run < max_run && slots[i + run] == slots[i] + run) ++run;
    char* sn = snap + (int64_t)i * L.bytes;
    for (int k = 0; k < R.n; ++k) {
      const Ring& r = R.r[k];
      const int64_t pitch = r.keep + r.hopb;
      if (r.rows == 1) { mv(state + slot_range(r, slots[i]).off, pitch, sn + L.ring[k], L.bytes, r.keep, run); continue; }
      for (int j = 0; j < run; ++j) mv(state + slot_range(r, slots[i] + j).off, pitch, sn + j * L.bytes + L.ring[k], r.keep, r.keep, r.rows);
    }
    mv(reinterpret_cast<char*>(pos + slots[i]), 4, sn + L.pos, L.bytes, 4, run);
    mv(reinterpret_cast<char*>(lens + slots[i]), 4, sn + L.pos + 4, L.bytes, 4, run);
    i += run;
  }
  q.flush();
  return q.st;
}
template <class Backend>
int export_slots(Backend& be, const Rings& R, const char* state, const int32_t* slots, int n, const int32_t* pos, const int32_t* lens, char* snap) {
  return move_slots(false, be, R, const_cast<char*>(state), slots, n, const_cast<int32_t*>(pos), const_cast<int32_t*>(lens), snap);
}
template <class Backend>
int import_slots(Backend& be, const Rings& R, char* state, const int32_t* slots, int n, int32_t* pos, int32_t* lens, const char* snap) {
  return move_slots(true, be, R, state, slots, n, pos, lens, const_cast<char*>(snap));
}

// A step's segments: make(T, lag_before) is a Path over the last T rows of a window whose newest `hop` rows are this
// step's frames -- buffer row lag_before + T - hop is absolute frame pos[b].
template <class Backend>
struct Segments {
  const Plan& P; const char* blob; char* ws; int B, hop; const int32_t* pos; const int32_t* lens; Backend& be;
  Path<Backend> make(int T, int lag_before = 0) const {
    Path<Backend> p{P, blob, ws, carve_workspace(P, B, T), B, T, be};
    p.lens = lens; p.pos = pos; p.off = lag_before + (T - hop);
    p.wn_wide = false;
    return p;
  }
};

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
  const int mrf = mrf_reach(c);
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

// The segment rings: each keeps 2*H frames and takes hop new ones per step.
//   unit    fp32 (B, unit_channels, 2*He + hop), the reference's (B, C, T) layout
//   zf[k]   fp32 [B][2*Hf + hop][C]: z in front of coupling layer k
//   zd      fp32 [B][2*Hd1 + hop][C]: z after the flow
//   s0[j]   operand type [B][(2*Hd2 + hop) * r0][ch0]: stage-0 ResBlock outputs
inline Rings stream_rings(const Plan& P, const StreamGeom& G, int B) {
  Rings R;
  const int64_t h = G.hop, zrow = (int64_t)P.cfg.inter_channels * 4, srow = (int64_t)G.r0 * P.stages[0].ch * 2;
  R.add(B, P.cfg.unit_channels, 2 * G.He * 4, h * 4);
  for (int k = 0; k < G.nf; ++k) R.add(B, 1, 2 * G.Hf * zrow, h * zrow);
  R.add(B, 1, 2 * G.Hd1 * zrow, h * zrow);
  for (int j = 0; j < 3; ++j) R.add(B, 1, 2 * G.Hd2 * srow, h * srow);
  return R;
}

// The snapshot of one slot of the segment rings: its layout (sized on the plan alone: any batch, any hop) and the tag
// that fingerprints it -- FNV-1a over a format version, the operand type (the stage-0 rings are stored in it), the
// decoder kind, the channel counts and r0, the five reaches and every ring's (rows, keep).  Neither depends on the batch,
// the hop or the weights: snapshots of one checkpoint are interchangeable exactly when their tags are equal.
constexpr uint64_t kSnapshotFormat = 1;
inline int stream_snapshot(const qvc_config* cfg, SnapLayout& L, uint64_t* tag = nullptr) {
  Plan P; StreamGeom G;
  const int gs = stream_plan(cfg, 1, P, G);
  if (gs != QVC_OK) return gs;
  const Rings R = stream_rings(P, G, 1);
  L = snap_layout(R);
  if (tag) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto word = [&](uint64_t v) { for (int i = 0; i < 8; ++i) { h ^= (v >> (8 * i)) & 0xff; h *= 0x100000001b3ull; } };
    const qvc_config& c = P.cfg;
    for (int64_t v : {(int64_t)kSnapshotFormat, (int64_t)c.operand_dtype, (int64_t)c.decoder, (int64_t)c.unit_channels, (int64_t)c.inter_channels,
                      (int64_t)P.stages[0].ch, (int64_t)G.r0, (int64_t)G.He, (int64_t)G.Hf, (int64_t)G.nf, (int64_t)G.Hd1, (int64_t)G.Hd2, (int64_t)R.n})
      word((uint64_t)v);
    for (int i = 0; i < R.n; ++i) { word((uint64_t)R.r[i].rows); word((uint64_t)R.r[i].keep); }
    *tag = h;
  }
  return QVC_OK;
}

// What qvc_stream_export_slots / qvc_stream_import_slots (and the CPU twin's) do on backend `be`: the checks in the order
// the status codes are pinned to -- pointers, counts and slots; the plan; the two sizes (stream_checks, the snapshots in
// the workspace's place); the alignments -- and then the copies.  A refused call launches nothing.
template <class Backend>
int snapshot_slots(bool import, Backend& be, const qvc_config* cfg, void* state, int64_t state_bytes, int batch, int hop, const int32_t* slots,
                   int n_slots, int32_t* pos, int32_t* lens, void* snap, int64_t snap_bytes) {
  bool args_ok = cfg && state && pos && lens && snap && slots && n_slots >= 1;
  for (int i = 0; args_ok && i < n_slots; ++i) args_ok = slots[i] >= 0 && slots[i] < batch;
  Rings R;
  const int st = stream_checks(args_ok, batch, state_bytes, snap_bytes, [&](StreamBytes& b) {
    Plan P; StreamGeom G;
    const int gs = stream_plan(cfg, hop, P, G);
    if (gs != QVC_OK) return gs;
    R = stream_rings(P, G, batch);
    b = {R.bytes(), (int64_t)n_slots * snap_layout(R).bytes};
    return gs;
  });
  if (st != QVC_OK) return st;
  if ((reinterpret_cast<uintptr_t>(state) & 255) || (reinterpret_cast<uintptr_t>(snap) & 255)) return QVC_ERR_BAD_ARG;
  return move_slots(import, be, R, static_cast<char*>(state), slots, n_slots, pos, lens, static_cast<char*>(snap));
}

struct StreamState {     // the ring table and, by name, the byte offsets of its rings in the caller-owned state buffer
  Rings rings;
  int64_t unit = 0, zf[16] = {}, zd = 0, s0[3] = {};
  int64_t bytes = 0;
};

inline StreamState carve_stream_state(const Plan& P, const StreamGeom& G, int B) {
  StreamState S;
  S.rings = stream_rings(P, G, B);
  const Ring* r = S.rings.r;
  S.unit = (r++)->off;
  for (int k = 0; k < G.nf; ++k) S.zf[k] = (r++)->off;
  S.zd = (r++)->off;
  for (int j = 0; j < 3; ++j) S.s0[j] = (r++)->off;
  S.bytes = S.rings.bytes();
  return S;
}

struct StreamScratch {   // carved from the END of the step's workspace, after the path's own workspace
  int64_t path_bytes = 0;   // workspace of the widest segment
  int64_t noise = 0;        // fp32 (B, C, 2*He + hop): the step's noise placed at the frames enc_p really outputs
  int64_t zwork[2] = {};    // fp32 [B][2*Hf + hop][C]: the coupling layer updates z in place on a copy of its ring
                            // (two of them: layer k's result feeds the copy for layer k+1 in the same launch)
  int64_t wave = 0;         // fp32 (B, spf * (2*Hd2 + hop))
  int64_t tmp[kMaxRings] = {};   // slide buffers, one per ring of the table
  int64_t pos_eff = 0, len_eff = 0;   // int32 [B] each: a tick's effective positions and lengths (tick = true only)
  int64_t bytes = 0;
};

inline int samples_per_frame(const Plan& P) { return P.total_up * P.cfg.hop * P.cfg.subbands; }

inline StreamScratch carve_stream_scratch(const Plan& P, const StreamGeom& G, int B, bool tick = false) {
  StreamScratch X;
  const qvc_config& c = P.cfg;
  X.path_bytes = carve_workspace(P, B, G.max_window()).bytes;
  Carver cv{X.path_bytes};
  X.noise = cv.take((int64_t)B * c.inter_channels * (2 * G.He + G.hop) * 4);
  for (int k = 0; k < 2; ++k) X.zwork[k] = cv.take((int64_t)B * (2 * G.Hf + G.hop) * c.inter_channels * 4);
  X.wave = cv.take((int64_t)B * samples_per_frame(P) * (2 * G.Hd2 + G.hop) * 4);
  stream_rings(P, G, B).carve_tmp(cv, B, X.tmp);
  if (tick) { X.pos_eff = cv.take((int64_t)B * 4); X.len_eff = cv.take((int64_t)B * 4); }
  X.bytes = cv.off;
  return X;
}

// One call of the segment rings, step or tick: what moves per slot is the mover's business (Moves: CopyQueue or
// CountedQueue), everything else -- the segments, their windows and workspace offsets, the hand-offs, the delivery, the
// two slide launches -- is written here once.  All data movement goes through the mover: 5 + n_flows launches (9 at the
// shipped config) where one memcpy per hand-off / slide would be ~35.  Arguments for a step (stream_tick states what a
// tick changes):
//   unit_new  (B, unit_channels, hop) fp32: unit frames [pos, pos + hop) of every stream
//   noise_new (B, inter, hop) fp32:         the N(0,1) draw of models.py:94 for frames [pos - He, pos - He + hop)
//                                           (the frames enc_p finishes in this step)
//   out       (B, hop * samples_per_frame): waveform of frames [pos - lag, pos - lag + hop); zeros where that is
//                                           outside [0, lens[b])
//   pos, lens (B,) int32 in the backend's memory: first new frame of this step / sequence length (large if unknown)
//   rng       with noise_new == nullptr: the draw is computed in enc_p's draw site for key rng->keys[slot] at the absolute
//             frame of every window row (Path::rng) -- no noise staging, X.noise stays untouched
template <class Moves>
int stream_run(Moves& q, const Plan& P, const char* blob, char* state, char* ws, const float* unit_new, const float* g,
               const float* noise_new, float* out, int B, int hop, typename Moves::Pos* pos, const int32_t* lens, const NoiseRng* rng) {
  using Backend = typename Moves::Backend;
  const StreamGeom G = stream_geom(P, hop);
  if (G.status != QVC_OK) return G.status;
  const StreamState S = carve_stream_state(P, G, B);
  const StreamScratch X = carve_stream_scratch(P, G, B, Moves::kTick);
  const size_t C = (size_t)P.cfg.inter_channels;
  const int h = hop, He = G.He, Hf = G.Hf, Hd1 = G.Hd1, Hd2 = G.Hd2;
  // the positions and lengths every segment's launch reads; a tick's are written by the first launch queued below, in
  // front of every launch that reads them (the conditioning table reads neither)
  const StreamPos at = q.open(pos, lens, G.lag() + G.max_window(), reinterpret_cast<int32_t*>(ws + X.pos_eff), reinterpret_cast<int32_t*>(ws + X.len_eff));
  const Segments<Backend> seg{P, blob, ws, B, h, at.pos, at.lens, q.be};
  // the rings slide at the END of the call, all of them in two launches.  A ring is read by exactly one segment per
  // call, so nothing needs it slid earlier.
  const size_t zrow = C * 4;                                       // one frame of z
  const int Tf = 2 * Hf + h;
  // hand the central frames of a segment's result (from `src` on, frame pitch zrow, `srcT` frames per stream) to coupling
  // layer k: into its ring's tail AND -- together with the ring's kept part -- into the work copy the layer updates
  auto feed_flow = [&](int k, const char* src, int srcT) {
    char* ring = state + S.zf[k];
    char* zw = ws + X.zwork[k & 1];
    q.fresh(ring + (size_t)2 * Hf * zrow, (size_t)Tf * zrow, src, (size_t)srcT * zrow, zrow, 1);
    q.kept(zw, (size_t)Tf * zrow, ring, (size_t)Tf * zrow, (size_t)2 * Hf * zrow, 1);
    q.fresh(zw + (size_t)2 * Hf * zrow, (size_t)Tf * zrow, src, (size_t)srcT * zrow, zrow, 1);
    q.flush();
  };
  // ... or, behind the last coupling layer, into the tail of the decoder's ring
  auto feed_dec = [&](const char* src, int srcT) {
    q.fresh(state + S.zd + (size_t)2 * Hd1 * zrow, (size_t)(2 * Hd1 + h) * zrow, src, (size_t)srcT * zrow, zrow, 1);
    q.flush();
  };

  {   // the conditioning table (cond rows x g) once per call: every segment's workspace keeps it at the same place
    Path<Backend> p = seg.make(Tf);
    p.cond_table(g);
    q.ok(p.status);
  }
  // ---- E: enc_p over the unit ring
  {
    const int T = 2 * He + h;
    char* ring = state + S.unit;
    char* nz = ws + X.noise;                                       // zeros either side of the call's noise
    q.append(state, S.rings.r[0], unit_new);
    if (noise_new) {
      q.zeros(nz, (size_t)T * 4, (size_t)He * 4, C);
      q.fresh(nz + (size_t)He * 4, (size_t)T * 4, noise_new, (size_t)h * 4, 4, C, (size_t)He * 4);
    }
    q.flush();
    Path<Backend> p = seg.make(T);
    if (!noise_new && rng) p.rng = *rng;     // (neither: enc_p refuses)
    p.enc_p(reinterpret_cast<const float*>(ring), noise_new ? reinterpret_cast<const float*>(nz) : nullptr, p.template wsp<float>(p.W.z));
    q.ok(p.status);
    feed_flow(0, ws + p.W.z + (size_t)He * zrow, T);               // (validate(): at least one coupling layer)
  }
  // ---- F_k: one coupling layer per segment, in place on a copy of its ring (its edge rows come out wrong and
  //      must not be written back: the ring has to keep the untouched values for the next step's context)
  for (int k = 0; k < G.nf; ++k) {
    char* zw = ws + X.zwork[k & 1];
    Path<Backend> p = seg.make(Tf, He + k * Hf);
    p.flow_step(P.flow[(size_t)k], reinterpret_cast<float*>(zw), -1.f);
    q.ok(p.status);
    if (k + 1 < G.nf) feed_flow(k + 1, zw + (size_t)Hf * zrow, Tf);
    else feed_dec(zw + (size_t)Hf * zrow, Tf);
  }
  // ---- D1: conv_pre + stage 0; its three ResBlock outputs feed the stage-0 rings
  const int ch0 = P.stages[0].ch, r0 = G.r0;
  {
    const int T = 2 * Hd1 + h;
    Path<Backend> p = seg.make(T, He + G.nf * Hf);
    p.dec_front(reinterpret_cast<const float*>(state + S.zd));
    q.ok(p.status);
    const size_t row = (size_t)ch0 * 2 * r0;                         // one unit frame of a stage-0 stream
    for (int j = 0; j < 3; ++j)                                    // (validate(): three ResBlocks)
      q.fresh(state + S.s0[j] + (size_t)2 * Hd2 * row, (size_t)(2 * Hd2 + h) * row, ws + p.W.ra[0][(size_t)j] + (size_t)Hd1 * row,
              (size_t)T * row, row, 1);
    q.flush();
  }
  // ---- D2: remaining stages + conv_post + iSTFT / band synthesis; the central frames are the call's output (an idle
  //      slot of a tick gets a row of zeros)
  {
    const int T = 2 * Hd2 + h;
    const size_t spf = (size_t)samples_per_frame(P);
    Path<Backend> p = seg.make(T, He + G.nf * Hf + Hd1);
    for (int j = 0; j < 3; ++j) p.s0_override[j] = state + S.s0[j];
    p.dec_back_wave(p.template wsp<float>(p.W.post), reinterpret_cast<float*>(ws + X.wave));
    q.ok(p.status);
    q.fresh(out, (size_t)h * spf * 4, ws + X.wave + (size_t)Hd2 * spf * 4, (size_t)T * spf * 4, spf * 4, 1, 0, kCountedIdleZero);
  }
  // ---- slide every ring by the slot's new frames: kept parts out (in the launch that also delivers the output and
  //      moves the positions on: no launch reads pos after the first), then back in
  q.advance(pos);
  q.slide_out(state, ws, S.rings, X.tmp, S.rings.n);
  q.flush();
  q.slide_back(state, ws, S.rings, X.tmp, S.rings.n);
  q.flush();
  return q.st;
}

// One step: every slot moves by hop frames (arguments: stream_run).  pos is only read; the caller advances it.
template <class Backend>
int stream_step(const Plan& P, const char* blob, char* state, char* ws, const float* unit_new, const float* g,
                const float* noise_new, float* out, int B, int hop, const int32_t* pos, const int32_t* lens, Backend& be,
                const NoiseRng* rng = nullptr) {
  CopyQueue<Backend> q(be, B, hop);
  return stream_run(q, P, blob, state, ws, unit_new, g, noise_new, out, B, hop, pos, lens, rng);
}

// ---------------------------------------------------------------- the tick form of the segment rings (stream_tick)
// stream_step moves every slot by exactly `hop` frames.  A tick lets slot b bring n = clamp(n_new[b], 0, hop) frames, the
// counts in device memory (a late packet, a client catching up, a short last chunk), on the SAME state:
//
//     INVARIANT  between calls every ring is left-aligned, exactly as stream_step leaves it: row r of a ring whose
//                segment runs at lag_before holds frame pos[b] - lag_before - 2*H + r, for r in [0, 2*H).
//     SHARED     stream_step keeps that invariant too, so a server may switch between the two calls on one state.
//
// A tick writes a slot's n new frames behind the kept 2*H, zero-fills rows [2*H + n, 2*H + hop) and runs every segment
// over its usual window of 2*H + hop rows with the usual pos.  Row H + i of a segment's result depends on window rows
// <= 2*H + i only, so rows [H, H + n) are exact; the rows behind them are computed from zeros -- finite, whatever the
// scratch held -- and never handed on.  A hand-off appends those n rows (and the zero fill) to the next ring, the slides
// move a slot's kept part by n rows, the delivery takes the FIRST n of the hop central rows, and pos[b] += n.  A
// sequence is never shortened through lens to skip the unused rows: a conv zero-pads at a sequence end, which would
// change the rows within H of it.  The one legitimate empty sequence is an idle slot's: with n == 0 the segments see
// len_eff = 0 and pos_eff >= every segment's off, so its tiles return at once, and no copy touches its rings, its scratch
// rows or its pos; only its row of `out` is written (zeros).
// With every n == hop: pos_eff = pos, len_eff = lens, every copy moves what stream_step's moves, and out and the bytes
// of the rings a later call can read are stream_step's bit for bit.
// All data movement is the backend's copy_counted (qvc_kernels.h: CountedDesc / CountedHead), queued by CountedQueue
// under the ONE body stream_step runs (stream_run): the same 5 + n_flows launches, hand-offs, appends, delivery and two
// slide launches as a step by construction; what differs is what a verb of the mover queues.
// Backend adds:  static constexpr bool kStreamTick = true  with  int copy_counted(const CountedHead&, const CountedDesc*, int n);
//                -- one that does not say so gets QVC_ERR_BAD_CONFIG.
template <class B, class = void> constexpr bool stream_tick_backend = false;
template <class B> constexpr bool stream_tick_backend<B, std::void_t<decltype(B::kStreamTick)>> = B::kStreamTick;

// One tick.  State as stream_step's; scratch carved with tick = true.  Arguments as stream_step's, except:
//   unit_new  columns [0, n) of row b are frames [pos[b], pos[b] + n); columns [n, hop) are never read
//   noise_new the same rule: the draw for frames [pos - He, pos - He + n)
//   out       the first n * spf samples of row b: frames [pos - lag, pos - lag + n), zeros outside [0, lens[b]); then zeros
//   n_new     (B,) int32 in the backend's memory, clamped to [0, hop] there; pos is advanced by n there too
template <class Backend>
int stream_tick(const Plan& P, const char* blob, char* state, char* ws, const float* unit_new, const float* g,
                const float* noise_new, float* out, int B, int hop, const int32_t* n_new, int32_t* pos, const int32_t* lens,
                Backend& be, const NoiseRng* rng = nullptr) {
  if constexpr (stream_tick_backend<Backend>) {
    CountedQueue<Backend> q(be, n_new, B, hop);
    return stream_run(q, P, blob, state, ws, unit_new, g, noise_new, out, B, hop, pos, lens, rng);
  } else {
    return QVC_ERR_BAD_CONFIG;
  }
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
  // what live_step / live_tick refuse: a geometry live_plan refused, or one it never saw
  int usable() const { return status != QVC_OK ? status : W < 2 ? QVC_ERR_BAD_ARG : QVC_OK; }
};

inline LiveGeom live_geom(const Plan& P) {
  LiveGeom G;
  if (P.status != QVC_OK) { G.status = P.status; return G; }
  const qvc_config& c = P.cfg;
  const int K2 = (c.wn_kernel_size - 1) / 2;
  G.He = c.enc_layers * K2; G.Hf = c.flow_layers * K2; G.nf = c.n_flows;
  const int mrf = mrf_reach(c);
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

// The window's rings, live_step's and live_tick's alike:
//   unit    fp32 (B, unit_channels, W), the reference's (B, C, T) layout
//   noise   fp32 (B, inter_channels, W): the noise of the same frames (pointer form only)
//     INVARIANT  between calls both are left-aligned: row r of slot b holds frame pos[b] - (W - hop) + r, for r in
//                [0, W - hop); the hop rows behind are rewritten before they are read.
//     SHARED     live_step and live_tick both keep it, so a server may switch between the two calls on one state.
inline Rings live_rings(const Plan& P, const LiveGeom& G, int B) {
  Rings R;
  const int64_t keep = (int64_t)(G.W - G.hop) * 4, hopb = (int64_t)G.hop * 4;
  R.add(B, P.cfg.unit_channels, keep, hopb);
  R.add(B, P.cfg.inter_channels, keep, hopb);
  return R;
}

struct LiveState {       // the ring table; unit / noise: the byte offsets of its two rings in the caller-owned state buffer
  Rings rings;
  int64_t unit = 0, noise = 0;
  int64_t bytes = 0;
};

inline LiveState carve_live_state(const Plan& P, const LiveGeom& G, int B) {
  LiveState S;
  S.rings = live_rings(P, G, B);
  S.unit = S.rings.r[0].off; S.noise = S.rings.r[1].off;
  S.bytes = S.rings.bytes();
  return S;
}

struct LiveScratch {     // carved from the END of the step's workspace, after the path's own workspace
  int64_t path_bytes = 0;   // carve_workspace(P, B, W): the widest segment
  int64_t zf = 0;           // fp32 [B][W - He][C]: z handed to the flow, updated in place (trimmed form)
  int64_t zd = 0;           // fp32 [B][W - He - nf * Hf][C]: z handed to the decoder (trimmed form)
  int64_t wave = 0;         // fp32 (B, spf * W): the window's waveform (trimmed form: of the decoder's rows)
  int64_t tmp[2] = {};      // slide buffers: the kept W - hop frames of the unit / noise ring
  int64_t pos_eff = 0, len_eff = 0;   // int32 [B] each: a tick's effective positions and lengths (tick = true only)
  int64_t bytes = 0;
};

inline LiveScratch carve_live_scratch(const Plan& P, const LiveGeom& G, int B, bool tick = false) {
  LiveScratch X;
  X.path_bytes = carve_workspace(P, B, G.W).bytes;
  Carver cv{X.path_bytes};
  X.zf = cv.take((int64_t)B * (G.W - G.He) * P.cfg.inter_channels * 4);
  X.zd = cv.take((int64_t)B * (G.W - G.He - G.nf * G.Hf) * P.cfg.inter_channels * 4);
  X.wave = cv.take((int64_t)B * samples_per_frame(P) * G.W * 4);
  live_rings(P, G, B).carve_tmp(cv, B, X.tmp);
  if (tick) { X.pos_eff = cv.take((int64_t)B * 4); X.len_eff = cv.take((int64_t)B * 4); }
  X.bytes = cv.off;
  return X;
}

// The path over the window held in the rings -- what a step runs between appending the new frames and delivering:
// the plain form or the three trimmed segments.  `unit` / `noise`: the rings (noise == nullptr: the generator form, rng).
// pos / lens: buffer row T - hop of a segment over the window's last T rows is absolute frame pos[b].  The window's
// waveform ends up in X.wave: wave_rows rows per stream, the hop delivered ones from row `first` on.
// unit_fm: the window's unit frames are [B][W][unit_channels] (infer_windows gathers them as they are on disk) instead of
// the rings' (B, unit_channels, W).
template <class Backend>
int live_window(const Plan& P, const LiveGeom& G, const LiveScratch& X, const char* blob, char* ws, const float* unit, const float* g,
                const float* noise, int B, const int32_t* pos, const int32_t* lens, Backend& be, const NoiseRng* rng, bool trim,
                size_t& wave_rows, size_t& first, bool unit_fm = false) {
  const qvc_config& c = P.cfg;
  const size_t W = (size_t)G.W;
  CopyQueue<Backend> q(be, B, G.hop);        // one strided copy per hand-off, each a launch of its own
  const Segments<Backend> seg{P, blob, ws, B, G.hop, pos, lens, be};
  float* wave = reinterpret_cast<float*>(ws + X.wave);
  wave_rows = W; first = (size_t)G.C();
  if (!trim) {
    Path<Backend> p = seg.make(G.W);
    if (!noise && rng) p.rng = *rng;         // (neither: enc_p refuses)
    p.unit_fm = unit_fm;
    p.infer(unit, g, noise, wave);
    q.ok(p.status);
  } else {
    const size_t zrow = (size_t)c.inter_channels * 4;              // one frame of z
    const int Tf = G.W - G.He, Td = Tf - G.nf * G.Hf;
    {   // E: the conditioning table (every segment's workspace keeps it at the same place) and enc_p
      Path<Backend> p = seg.make(G.W);
      if (!noise && rng) p.rng = *rng;
      p.unit_fm = unit_fm;
      p.cond_table(g);
      p.enc_p(unit, noise, p.template wsp<float>(p.W.z));
      q.ok(p.status);
      q.add(ws + X.zf, (size_t)Tf * zrow, ws + p.W.z + (size_t)G.He * zrow, W * zrow, (size_t)Tf * zrow, (size_t)B);
      q.flush();
    }
    {   // F: the flow, in place on its rows
      Path<Backend> p = seg.make(Tf);
      p.flow(reinterpret_cast<float*>(ws + X.zf));
      q.ok(p.status);
      q.add(ws + X.zd, (size_t)Td * zrow, ws + X.zf + (size_t)(Tf - Td) * zrow, (size_t)Tf * zrow, (size_t)Td * zrow, (size_t)B);
      q.flush();
    }
    {   // D: the decoder and the tail
      Path<Backend> p = seg.make(Td);
      p.dec_trunk_wave(reinterpret_cast<const float*>(ws + X.zd), p.template wsp<float>(p.W.post), wave);
      q.ok(p.status);
    }
    wave_rows = (size_t)Td; first = (size_t)G.Hdec;
  }
  return q.st;
}

// One call of the window, step or tick (G from live_plan): as in stream_run, what moves per slot is the mover's business
// and everything else is written here once -- the new frames behind the kept ones, the path over the window, the delivery
// and the two slide launches.  Arguments for a step (live_tick states what a tick changes):
//   unit_new  (B, unit_channels, hop) fp32: unit frames [pos, pos + hop) of every stream
//   noise_new (B, inter, hop) fp32:         the N(0,1) draw of models.py:94 for the SAME frames (no noise lag)
//   out       (B, hop * samples_per_frame): waveform of frames [pos - L, pos - L + hop); zeros where that is outside
//                                           [0, lens[b])
//   pos, lens, rng: as stream_run (rng: the draw at the absolute frame of every window row; the noise ring stays untouched)
//   trim      false: the plain form (one Path over the window)
template <class Moves>
int live_run(Moves& q, const Plan& P, const LiveGeom& G, const char* blob, char* state, char* ws, const float* unit_new, const float* g,
             const float* noise_new, float* out, int B, typename Moves::Pos* pos, const int32_t* lens, const NoiseRng* rng, bool trim) {
  if (G.usable() != QVC_OK) return G.usable();
  const LiveState S = carve_live_state(P, G, B);
  const LiveScratch X = carve_live_scratch(P, G, B, Moves::kTick);
  const size_t h = (size_t)G.hop, spf = (size_t)samples_per_frame(P);
  const int nrings = noise_new ? 2 : 1;                            // the generator form leaves the noise ring alone
  // the positions and lengths the window's launches read; a tick's are written by the launch that appends (an idle slot:
  // an empty sequence at W, past every segment's off) and end the sequence behind the slot's new frames
  const StreamPos at = q.open(pos, lens, G.W, reinterpret_cast<int32_t*>(ws + X.pos_eff), reinterpret_cast<int32_t*>(ws + X.len_eff), true);
  // ---- append the new frames behind the kept ones
  q.append(state, S.rings.r[0], unit_new);
  if (noise_new) q.append(state, S.rings.r[1], noise_new);
  q.flush();
  const float* unit = reinterpret_cast<const float*>(state + S.unit);
  const float* noise = noise_new ? reinterpret_cast<const float*>(state + S.noise) : nullptr;
  size_t wave_rows = 0, first = 0;                                 // rows of X.wave, and the first delivered one
  q.ok(live_window(P, G, X, blob, ws, unit, g, noise, B, at.pos, at.lens, q.be, rng, trim, wave_rows, first));
  // ---- deliver the slot's new frames of rows [first, first + hop) (an idle slot of a tick gets a row of zeros), move the
  //      positions on and slide the rings: kept parts out, then back in
  q.fresh(out, h * spf * 4, ws + X.wave + first * spf * 4, wave_rows * spf * 4, spf * 4, 1, 0, kCountedIdleZero);
  q.advance(pos);
  q.slide_out(state, ws, S.rings, X.tmp, nrings);
  q.flush();
  q.slide_back(state, ws, S.rings, X.tmp, nrings);
  q.flush();
  return q.st;
}

// One step: every slot moves by hop frames (arguments: live_run).  pos is only read; the caller advances it.
template <class Backend>
int live_step(const Plan& P, const LiveGeom& G, const char* blob, char* state, char* ws, const float* unit_new, const float* g,
              const float* noise_new, float* out, int B, const int32_t* pos, const int32_t* lens, Backend& be,
              const NoiseRng* rng = nullptr, bool trim = true) {
  CopyQueue<Backend> q(be, B, G.hop);
  return live_run(q, P, G, blob, state, ws, unit_new, g, noise_new, out, B, pos, lens, rng, trim);
}

// ---------------------------------------------------------------- the tick form of the window (live_tick)
// live_step moves every slot by exactly `hop` frames.  A tick lets slot b bring n = clamp(n_new[b], 0, hop) frames, the
// counts in device memory: a late packet (n = 0), a client catching up, a last chunk shorter than hop -- on the SAME state
// (live_rings: INVARIANT, SHARED), through the same body on CountedQueue, as stream_tick does for the segment rings.
// A tick writes a slot's n new frames behind the kept W - hop and zero-fills rows [W - hop + n, W).  The window's launches
// see pos_eff = pos -- buffer row W - hop is that absolute frame, as in a step -- and len_eff = min(lens, pos + n): a
// sequence that ends behind the newest frame, which is what the window is (the zero-filled rows are past its end, not
// frames of it).  So the delivered frames [pos - L, pos - L + n), the FIRST n of the hop central rows, are those of the
// offline conversion of the prefix [0, min(lens, pos + n)); the rows behind them are never handed on.  The slides move a
// slot's kept part by n rows and pos[b] += n.  A slot with n == 0 gets an empty sequence (len_eff = 0, pos_eff = W: hi = 0
// in every segment), so its tiles return at once, and no copy touches its rings, its scratch rows or its pos; only its
// row of `out` is written (zeros).
// With every n == hop: pos_eff = pos, len_eff = min(lens, pos + hop) -- the buffer end, where a step's sequence ends
// anyway -- every copy moves what live_step's moves, and out and the kept ring bytes are live_step's bit for bit.
// Delivered frame f was computed with the frames up to pos + n - 1 in the window: L + n - 1 - (f - (pos - L)) frames of
// look-ahead, between L and L + n - 1.  With L = C every frame has its whole receptive field whatever n was, so the
// output does not depend on how the stream was cut into ticks; with L < C it legitimately does.
// Backend: as stream_tick (kStreamTick with copy_counted) -- one that does not say so gets QVC_ERR_BAD_CONFIG.
//
// One tick.  State as live_step's; scratch carved with tick = true.  Arguments as live_step's, except:
//   unit_new  columns [0, n) of row b are frames [pos[b], pos[b] + n); columns [n, hop) are never read
//   noise_new the same rule, the draw for the same frames
//   out       the first n * spf samples of row b: frames [pos - L, pos - L + n) of the prefix conversion; then zeros
//   n_new     (B,) int32 in the backend's memory, clamped to [0, hop] there; pos is advanced by n there too
template <class Backend>
int live_tick(const Plan& P, const LiveGeom& G, const char* blob, char* state, char* ws, const float* unit_new, const float* g,
              const float* noise_new, float* out, int B, const int32_t* n_new, int32_t* pos, const int32_t* lens, Backend& be,
              const NoiseRng* rng = nullptr, bool trim = true) {
  if constexpr (stream_tick_backend<Backend>) {
    CountedQueue<Backend> q(be, n_new, B, G.hop);
    return live_run(q, P, G, blob, state, ws, unit_new, g, noise_new, out, B, pos, lens, rng, trim);
  } else {
    return QVC_ERR_BAD_CONFIG;
  }
}

// ---------------------------------------------------------------- exact windows over packed utterances (infer_windows)
// The offline form of the window.  Every other whole-path call sizes its buffers by rows x longest utterance; here the
// rows of a call are WINDOWS, cut from utterances of any lengths that lie back to back in packed buffers and named by a
// table in device memory (qvc_window: base, length, start, count), so the memory is rows x window whatever the lengths,
// one long recording runs at batch rate, and every row has its own g row.  With n = window_frames it is live_window at
// hop = n and L = C, over the W = 2C + n frames [start - C, start + n + C) of the row's utterance:
//
//     row:   0 ............. C ........... C+n ............ W = 2C+n
//            |  left context  |  delivered  |  right context  |
//     frame: start-C        start        start+n          start+n+C        pos = start + C sits at buffer row W - n
//
// Property P2 of the window (L = C: the conversion of the prefix that ends with the window and the whole-utterance
// conversion agree on the delivered rows, for every decoder validate() accepts) makes the delivered frames those of the
// whole-utterance conversion; the sequence's own two ends inside a window are exact through pos / lens as everywhere, and
// the generator draws at the absolute frame of every row.  Four steps: the plan -- live_plan(cfg, n, C) --, ONE gather
// launch (units, the noise in the pointer form, the rows' pos / len), live_window as it is (trimmed, or plain), ONE
// deliver launch.  The decoder still runs over the C rows of right context: trimming them on the right as the trimmed
// form trims on the left is the obvious follow-up and not done here.
// Per delivered frame a row costs (2C + n) / n of the offline cost in enc_p, (2C + n - He) / n in the flow and
// (Hdec + C + n) / n in the decoder (trimmed form).
// Backend adds:  static constexpr bool kWindows = true  with  int window_gather(const WindowArgs&)  and
//                int window_deliver(const WindowArgs&)  (qvc_kernels.h) -- one that does not say so gets QVC_ERR_BAD_CONFIG.
template <class B, class = void> constexpr bool windows_backend = false;
template <class B> constexpr bool windows_backend<B, std::void_t<decltype(B::kWindows)>> = B::kWindows;

// The plan and the window for (cfg, n): live_plan(cfg, n, C), C read off the first geometry instead of a second plan.
inline int window_plan(const qvc_config* cfg, int n, Plan& P, LiveGeom& G) {
  const int st = live_plan(cfg, n, 0, P, G);
  if (st != QVC_OK) return st;
  const int C = G.C();
  if ((int64_t)2 * C + n > (1 << 24)) return G.status = QVC_ERR_BAD_ARG;
  G.L = C; G.W = 2 * C + n;
  return QVC_OK;
}

struct WindowScratch {   // the window's own scratch (a tick's: pos_eff / len_eff are the rows' pos / len), then the gathered windows
  LiveScratch X;
  int64_t unit = 0;         // fp32 [B][W][unit_channels]
  int64_t noise = 0;        // fp32 (B, inter_channels, W): the pointer form only (carved always: the size query has no form)
  int64_t bytes = 0;
};

inline WindowScratch carve_window_scratch(const Plan& P, const LiveGeom& G, int B) {
  WindowScratch S;
  S.X = carve_live_scratch(P, G, B, true);
  Carver cv{S.X.bytes};
  S.unit = cv.take((int64_t)B * G.W * P.cfg.unit_channels * 4);
  S.noise = cv.take((int64_t)B * P.cfg.inter_channels * G.W * 4);
  S.bytes = cv.off;
  return S;
}

// What qvc_infer_windows_fm / _rng_fm (and the CPU twin's) do on backend `be`: the checks in the order the status codes are
// pinned to -- pointers, counts and the draw; the plan; the workspace size (stream_checks, no state); the alignments --
// and then the four steps.  Exactly one of noise_packed / rng.  A refused call launches nothing.
template <class Backend>
int infer_windows(Backend& be, const qvc_config* cfg, const void* blob_, const float* unit_packed, const float* noise_packed, const NoiseRng* rng,
                  const qvc_window* win, const float* g, float* out_packed, int rows, int n, int total, void* ws_, int64_t ws_bytes, bool trim) {
  Plan P; LiveGeom G;
  const bool draw = rng ? (!noise_packed && rng->keys) : noise_packed != nullptr;
  const bool args_ok = blob_ && unit_packed && draw && win && g && out_packed && ws_ && rows <= 65535 && n >= 1 && total >= 1 && total <= kWindowMaxTotal;
  const int st = stream_checks(args_ok, rows, 0, ws_bytes, [&](StreamBytes& b) {
    const int gs = window_plan(cfg, n, P, G);
    if (gs != QVC_OK) return gs;
    if (!windows_backend<Backend>) return (int)QVC_ERR_BAD_CONFIG;
    b = {0, carve_window_scratch(P, G, rows).bytes};
    return gs;
  });
  if (st != QVC_OK) return st;
  if ((reinterpret_cast<uintptr_t>(ws_) & 255) || (reinterpret_cast<uintptr_t>(blob_) & 255)) return QVC_ERR_BAD_ARG;
  if constexpr (windows_backend<Backend>) {
    const char* blob = static_cast<const char*>(blob_);
    char* ws = static_cast<char*>(ws_);
    const WindowScratch S = carve_window_scratch(P, G, rows);
    WindowArgs a;
    a.win = win; a.rows = rows; a.n = n; a.C = G.C(); a.W = G.W; a.total = total;
    a.unit_packed = unit_packed; a.unit_win = reinterpret_cast<float*>(ws + S.unit); a.unit_channels = P.cfg.unit_channels;
    a.noise_packed = noise_packed; a.noise_win = reinterpret_cast<float*>(ws + S.noise); a.inter = P.cfg.inter_channels;
    a.pos_eff = reinterpret_cast<int32_t*>(ws + S.X.pos_eff); a.len_eff = reinterpret_cast<int32_t*>(ws + S.X.len_eff);
    a.out_packed = out_packed; a.spf = samples_per_frame(P);
    int rc = be.window_gather(a);
    if (rc != QVC_OK) return rc;
    size_t wave_rows = 0, first = 0;
    rc = live_window(P, G, S.X, blob, ws, a.unit_win, g, noise_packed ? a.noise_win : nullptr, rows, a.pos_eff, a.len_eff, be, rng, trim, wave_rows,
                     first, /*unit_fm=*/true);
    if (rc != QVC_OK) return rc;
    a.wave = reinterpret_cast<const float*>(ws + S.X.wave); a.wave_rows = (int32_t)wave_rows; a.first = (int32_t)first;
    return be.window_deliver(a);
  } else {
    return QVC_ERR_BAD_CONFIG;
  }
}

}  // namespace qvc
