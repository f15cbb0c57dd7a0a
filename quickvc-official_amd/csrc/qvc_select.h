// qvc_select.h -- which kernel a launch gets: one pure host function per kernel family, returning data.
//
// A launcher (qvc_kernels.h: launch_conv, launch_pair3, ...) is  choose_*  ->  LaunchChoice  ->  dispatch_*:
//   * choose_* (here) checks the call and picks the kernel instantiation, the tile, the grid and the LDS size.  Host
//     code only -- nothing of HIP is included, any C++17 compiler reads this header -- so a host test can ask which
//     kernel a shape gets (tools/emu_twin.cpp: qvc_emu_launch_trace; tests/golden/launch_trace.json pins the answers).
//   * dispatch_* (the device translation units) lifts the choice's integers to template arguments and launches.  It
//     decides nothing.
//   * *_built(...) states once per family which template tuples the library instantiates.  The chooser skips what is not
//     built, the dispatcher instantiates exactly what is: the two cannot disagree.
// Adding a variant: one line in the family's *_built, one in its chooser, one case in the golden file.
#pragma once
#include "qvc_kernels.h"

namespace qvc {

enum LaunchFamily : int32_t {
  LF_CONV = 0,      // conv_mfma_kernel<T, MF, NF, WM, EPI, CL>
  LF_PAIR,          // rbpair_kernel<T, MF, NF, WM, NWV, TS>
  LF_CHAIN,         // rbchain_kernel<T, MF, NF, NWV, TS>
  LF_WN_LAYER,      // wn_layer_kernel<T, NF, LAST, WV>
  LF_WN_STACK,      // wn_stack_kernel<T, NF, PM, WV>: the generic whole-stack kernel
  LF_WN_STACK2,     // wn_stack2_kernel<T, 6, 5, PM, NF, RING>: the continuous-stream kernel, NF 3 = 32-frame, NF 5 = 64-frame tile
  LF_POST_TAIL      // post_tail_kernel<T, NF, NB>
};

// One launch, decided.  Template integers a family does not have stay 0.
struct LaunchChoice {
  int32_t status = QVC_OK;              // QVC_ERR_BAD_ARG / QVC_ERR_BAD_CONFIG: nothing is launched, the rest is unspecified
  int32_t family = LF_CONV;
  int32_t op = QVC_F16, ts = QVC_F16;   // T: MFMA operand type; TS: type of the pairs' residual stream (QVC_F16 / QVC_BF16)
  int32_t MF = 0, NF = 0, WM = 0;
  int32_t waves = 0;                    // NWV (pair, chain) / WV (WaveNet: the bucket the kernel is built for, >= block / 64)
  int32_t epi = 0;                      // conv: the kernel's EPI (EPI_SAMPLE_RNG where the draw is computed in the epilogue)
  int32_t cl = 0;                       // conv: chunk loop
  int32_t last = 0;                     // WaveNet layer: LAST
  int32_t pm = 0;                       // WaveNet stacks: PM (fused post 1x1)
  int32_t bands = 0;                    // post_tail: NB
  int32_t ring = 0;                     // continuous-stream kernel: RING
  int32_t halo = 0, margin = 0, NT = 0; // chain: what the launch writes into ChainArgs (chain_geom)
  uint32_t grid[3] = {1, 1, 1};
  uint32_t block = 0;
  int64_t lds = 0;                      // dynamic LDS bytes
  int64_t optin_above = 0;              // the opt-in for large dynamic LDS is taken when lds exceeds this
};
inline LaunchChoice choice_error(LaunchChoice c, int status) { c.status = status; return c; }

// ------------------------------------------------------------------ what is instantiated
// Kernel-side variant of EPI_SAMPLE, chosen by choose_conv when the launch carries a generator instead of a noise
// tensor (ConvArgs::rng); callers and backends only ever name EPI_SAMPLE.
constexpr int EPI_SAMPLE_RNG = 16;

constexpr bool one_of(int v, int a, int b, int c = -1, int d = -1, int e = -1) { return v == a || v == b || (c >= 0 && v == c) || (d >= 0 && v == d) || (e >= 0 && v == e); }

// The accumulators of a tile must fit the registers (MF * NF quads); the generator epilogue is not built at NF 10 (at
// MF 4 its 160 accumulators plus the generator's temporaries spill, 656 B of scratch per lane; the tile changes no bit of
// the result); the chunk loop is built for the 4 x 4-fragment layout.  8-wave layouts exist for the fused pair kernel only.
constexpr bool conv_layout_built(int epi, int MF, int WM) {
  return epi == EPI_STD ? (WM == 4 && MF >= 1 && MF <= 4) || (WM == 2 && (MF == 3 || MF == 4)) || (WM == 1 && MF == 4)
                        : (epi == EPI_GAU || epi == EPI_SAMPLE || epi == EPI_SAMPLE_RNG || epi == EPI_STATS) && WM == 4 && one_of(MF, 2, 4, 6);
}
constexpr bool conv_built(int epi, int MF, int NF, int WM, int cl) {
  const bool tile = one_of(NF, 2, 4, 5, 8, 10) && MF * NF * 4 <= 160 && !(NF == 10 && epi == EPI_SAMPLE_RNG);
  return conv_layout_built(epi, MF, WM) && tile && (cl == 0 || (cl == 1 && epi == EPI_STD && MF == 4 && WM == 4 && NF <= 5));
}
// pair: NF + 1 column fragments of the intermediate per wave
constexpr bool pair_built(int MF, int NF, int WM, int NWV) {
  const bool layout = NWV == 4 ? (WM == 4 && MF >= 1 && MF <= 4) || (WM == 2 && (MF == 3 || MF == 4)) || (WM == 1 && MF == 4)
                               : NWV == 8 && WM == 8 && MF >= 2 && MF <= 4;
  return layout && one_of(NF, 2, 4, 5, 8, 10) && MF * (NF + 1) * 4 <= 160 && !(NF == 10 && MF > 2);
}
// chain: accumulator registers (+ as many for the B double buffer)
constexpr bool chain_built(int MF, int NF, int NWV) {
  return one_of(MF, 2, 4) && one_of(NWV, 4, 8) && one_of(NF, 9, 8, 6, 5, 4) && MF * NF * 4 <= (MF > 2 ? 80 : 96);
}
constexpr bool wn_layer_built(int NF, int WV) { return one_of(NF, 2, 4) && one_of(WV, 4, 8, 12, 16); }
constexpr bool wn_stack_built(int NF, int PM, int WV) { return one_of(NF, 2, 3, 6) && (PM == 0 || PM == 1) && one_of(WV, 4, 8, 12, 16); }
// register ring depth (k-steps) of the 64-frame tile; must divide a layer's 36 k-steps
#ifndef QVC_WN2_WIDE_RING
#define QVC_WN2_WIDE_RING 4
#endif
constexpr bool wn_stack2_built(int PM, int NF, int RING) { return (PM == 0 || PM == 1) && ((NF == 3 && RING == 6) || (NF == 5 && RING == QVC_WN2_WIDE_RING)); }
constexpr bool post_tail_built(int NF, int NB) { return (NB == 1 && NF == 2) || (NB == 4 && (NF == 2 || NF == 4)); }

inline bool choice_built(const LaunchChoice& c) {
  switch (c.family) {
    case LF_CONV: return conv_built(c.epi, c.MF, c.NF, c.WM, c.cl);
    case LF_PAIR: return pair_built(c.MF, c.NF, c.WM, c.waves);
    case LF_CHAIN: return chain_built(c.MF, c.NF, c.waves);
    case LF_WN_LAYER: return wn_layer_built(c.NF, c.waves);
    case LF_WN_STACK: return wn_stack_built(c.NF, c.pm, c.waves);
    case LF_WN_STACK2: return wn_stack2_built(c.pm, c.NF, c.ring);
    case LF_POST_TAIL: return post_tail_built(c.NF, c.bands);
    default: return false;
  }
}

// ------------------------------------------------------------------ conv
struct TileChoice { int NF; int blocks; size_t lds; };

inline TileChoice choose_tile(const ConvDesc& d, int Nq, int batch, int epi) {
  static const int nfs[] = {2, 4, 5, 8, 10};
  const int halo = (d.taps - 1) * d.dil;
  const int rowbytes = d.CinP * 2;
  const int WN = kWaves / d.WM;
  TileChoice best{0, 0, 0};
  double best_cost = 1e300;
  for (int i = 0; i < 5; ++i) {
    const int NF = nfs[i];
#ifdef QVC_FORCE_NF
    if (NF != QVC_FORCE_NF) continue;                           // developer sweep (tools/conv_bench)
#endif
    if (!conv_built(epi, d.MF, NF, d.WM, 0)) continue;
    // polyphase up-samplers have s * Cout rows = many row chunks, and every workgroup streams its chunk's whole K:
    // with 32-frame tiles up-sampler 0 pulls 4.9 MB of weights into every CU (45 us at the ~50 B/clk a CU takes in) --
    // 64-frame tiles halve that while the launch still has two workgroups per CU (57.9 -> 50.3 us, bit-identical)
    if (d.up_s > 1 && NF < 4 && (long)ceil_div(Nq, WN * 4 * 16) * batch * d.nchunk >= 512) continue;
    const int NT = WN * NF * 16;
    const size_t lds = (size_t)(NT + halo) * rowbytes;
    if (lds > 160 * 1024) continue;
    const int tiles = ceil_div(Nq, NT);
    const long blocks = (long)tiles * batch * d.nchunk;
    // workgroups that can share a CU (LDS, and the ~512 registers/lane of a SIMD): with >= 2 the
    // staging / epilogue of one overlaps the MFMA phase of another
    const int regs = d.MF * NF * 4 + 16 * d.MF + 8 * NF + 40;
    const int bpc = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(3, (160 * 1024) / lds), (size_t)(512 / regs)));
    const long rounds = (blocks + 256L * bpc - 1) / (256L * bpc);
    // work per block ~ frames computed + a fixed overhead (staging, launch, epilogue), in frame units
    const double work = NT + 0.35 * halo + 24.0;
    const double cost = (double)rounds * bpc * work * (bpc == 1 ? 1.3 : 1.0);
    if (cost < best_cost) { best_cost = cost; best = TileChoice{NF, (int)blocks, lds}; }
#ifndef QVC_FORCE_NF
    // latency-sized launch: even the smallest tile gives every workgroup a CU of its own -- take it (each workgroup
    // streams the same weights whatever its tile, so fewer frames per workgroup is less serial MFMA work behind them;
    // batch 1, up-sampler 0: 35 -> 22 us)
    if (i == 0 && blocks <= 256) return best;
#endif
  }
  return best;
}

// `a` as the caller fills it: the geometry fields launch_conv copies from `d` (conv_geometry) are read from `d`
inline LaunchChoice choose_conv(const ConvDesc& d, const ConvArgs& a, int batch, int epi, int dtype) {
  LaunchChoice c;
  c.family = LF_CONV; c.MF = d.MF; c.WM = d.WM; c.block = 256;
  if (d.lp && (epi != EPI_STD || !a.y16 || a.y32 || a.y32b || a.res || a.res16 || d.MF % 2)) return choice_error(c, QVC_ERR_BAD_CONFIG);
  if (dtype != QVC_F16 && dtype != QVC_BF16) return choice_error(c, QVC_ERR_BAD_ARG);
  c.op = c.ts = dtype;
  c.epi = EPI_STD;
  if (epi == EPI_GAU) {
    c.epi = EPI_GAU;
  } else if (epi == EPI_SAMPLE && !a.noise && a.rng.keys) {   // the draw computed in the epilogue (ConvArgs::rng)
    if (d.WM != 4 || !d.gau || !a.y32 || !a.bias || a.rg.mul != 1) return choice_error(c, QVC_ERR_BAD_CONFIG);
    c.epi = EPI_SAMPLE_RNG;
  } else if (epi == EPI_SAMPLE) {
    if (d.WM != 4 || !d.gau || !a.noise || !a.y32 || !a.bias) return choice_error(c, QVC_ERR_BAD_CONFIG);
    c.epi = EPI_SAMPLE;
  } else if (epi == EPI_STATS) {
    if (d.WM != 4 || !d.gau || !a.y32 || !a.bias) return choice_error(c, QVC_ERR_BAD_CONFIG);
    c.epi = EPI_STATS;
  }
  if (!conv_layout_built(c.epi, d.MF, d.WM)) return choice_error(c, QVC_ERR_BAD_CONFIG);
  const TileChoice tc = choose_tile(d, a.Nq, batch, c.epi);
  if (tc.NF == 0) return choice_error(c, QVC_ERR_BAD_CONFIG);   // no tile fits LDS / registers
  c.NF = tc.NF; c.lds = (int64_t)tc.lds;
  const int NT = (kWaves / d.WM) * c.NF * 16;
  // chunk loop: built for the 4 x 4-fragment layout; taken when the tile is the mean of three streams (expensive to
  // stage) and the launch still has two workgroups for every CU without the chunk dimension
  c.cl = conv_built(c.epi, c.MF, c.NF, c.WM, 1) && debug_get(DBG_CONV_CL) && d.nchunk >= 2 && a.x2 && (long)ceil_div(a.Nq, NT) * batch >= 512;
  c.grid[0] = (unsigned)ceil_div(a.Nq, NT); c.grid[1] = (unsigned)batch; c.grid[2] = (unsigned)(c.cl ? 1 : d.nchunk);
  return c;
}

// ------------------------------------------------------------------ fused pair
inline TileChoice choose_pair_tile(const ConvDesc* ds, int n, int T, int batch) {
  static const int nfs[] = {2, 4, 5, 8, 10}; // measured at B=32, MF 4: NF 5 (2 workgroups/CU) beats 4 and 8 by 7-35 %
  const ConvDesc& d = ds[0];
  const int NWV = block_waves(d);
  const int WN = NWV / d.WM;
  int halo1 = 0;                              // the chains of a launch share one tile shape: size it for the widest halo
  for (int i = 0; i < n; ++i) halo1 = std::max(halo1, (ds[i].taps - 1) * ds[i].dil);
  const int rowbytes = d.CinP * 2;
  TileChoice best{0, 0, 0};
  double best_cost = 1e300;
  for (int NF : nfs) {
#ifdef QVC_FORCE_NF
    if (NF != QVC_FORCE_NF) continue;
#endif
    if (!pair_built(d.MF, NF, d.WM, NWV)) continue;
    const size_t lds = (size_t)(WN * (NF + 1) * 16 + halo1) * rowbytes;
    if (lds > 160 * 1024) continue;
    const int NT = WN * NF * 16;
    const long blocks = (long)ceil_div(T, NT) * batch * n;
    // workgroups that can share a CU: 2 x 4 waves or 1 x 8 waves (two waves per SIMD either way)
    const int bpc = NWV == 8 ? 1 : (int)std::min<size_t>(2, (160 * 1024) / lds);
    const long rounds = (blocks + 256L * bpc - 1) / (256L * bpc);
    // per-workgroup work in frame units: both GEMMs + staging/epilogue; a single 4-wave workgroup per CU
    // cannot overlap its memory phases with another one's MFMA phases
    const double work = WN * (NF + 1) * 16 + NT + 0.35 * halo1 + 32.0;
    const double cost = rounds * bpc * work * ((bpc == 1 && NWV == 4) ? 1.3 : 1.0);
    if (cost < best_cost) { best_cost = cost; best = TileChoice{NF, (int)blocks, lds}; }
  }
  return best;
}

// operand and stream type of the pair / chain kernels: QVC_BF16X = bf16 operands, f16 stream
inline bool pair_types(int dtype, LaunchChoice& c) {
  if (dtype != QVC_F16 && dtype != QVC_BF16 && dtype != QVC_BF16X) return false;
  c.op = dtype == QVC_F16 ? QVC_F16 : QVC_BF16;
  c.ts = dtype == QVC_BF16 ? QVC_BF16 : QVC_F16;
  return true;
}

// n pairs (1..3) of equal shape class in one launch; d1[i] / d2[i] are chain i's convs
inline LaunchChoice choose_pair(const ConvDesc* d1, const ConvDesc* d2, const PairArgs3& a, int batch, int dtype) {
  LaunchChoice c;
  c.family = LF_PAIR;
  if (a.n < 1 || a.n > 3) return choice_error(c, QVC_ERR_BAD_ARG);
  for (int i = 0; i < a.n; ++i) {
    if (!pair_supported(d1[i], d2[i]) || !d1[i].lp || !d2[i].lp) return choice_error(c, QVC_ERR_BAD_CONFIG);
    if (d1[i].MF != d1[0].MF || d1[i].WM != d1[0].WM || d1[i].CinP != d1[0].CinP) return choice_error(c, QVC_ERR_BAD_CONFIG);
    if (a.p[i].T != a.p[0].T || a.p[i].C != a.p[0].C || a.p[i].CP != a.p[0].CP) return choice_error(c, QVC_ERR_BAD_ARG);
  }
  if (!pair_types(dtype, c)) return choice_error(c, QVC_ERR_BAD_ARG);
  c.MF = d1[0].MF; c.WM = d1[0].WM; c.waves = block_waves(d1[0]); c.block = (unsigned)c.waves * 64;
  const TileChoice tc = choose_pair_tile(d1, a.n, a.p[0].T, batch);
  if (tc.NF == 0) return choice_error(c, QVC_ERR_BAD_CONFIG);
  c.NF = tc.NF; c.lds = (int64_t)tc.lds;
  const unsigned tiles = (unsigned)ceil_div(a.p[0].T, (c.waves / c.WM) * c.NF * 16);
  if (a.chain_major) { c.grid[0] = tiles; c.grid[1] = (unsigned)batch; c.grid[2] = (unsigned)a.n; }
  else { c.grid[0] = tiles * (unsigned)a.n; c.grid[1] = (unsigned)batch; }
  return c;
}

// ------------------------------------------------------------------ chained ResBlock
struct ChainGeom { int halo, margin, NT; size_t lds; };
// tile of NF fragments (NF * 16 rows): halo rows per side are recomputed, NT = rows - 2 * halo frames come out
inline ChainGeom chain_geom(const ConvDesc* d1, int n, int NF) {
  ChainGeom g{0, 0, 0, 0};
  for (int q = 0; q < n; ++q) {
    const int h = (d1[q].taps - 1) / 2;
    g.halo += h * (d1[q].dil + 1);
    g.margin = std::max(g.margin, h * d1[q].dil);
  }
  g.NT = NF * 16 - 2 * g.halo;
  g.lds = (size_t)(NF * 16 + 2 * g.margin + NF * 16) * d1[0].CinP * 2;
  return g;
}

// Tile choice: the largest tile (fewest recomputed halo frames per produced frame) whose LDS fits the occupancy the
// layout's pair kernel has -- two 4-wave workgroups or one 8-wave workgroup per CU.
inline int chain_pick_nf(const ConvDesc* d1, int n, ChainGeom* out) {
  const int nwv = block_waves(d1[0]);
  const size_t budget = nwv == 8 ? 160 * 1024 : 80 * 1024;
  static const int nfs[] = {9, 8, 6, 5, 4};
  for (int NF : nfs) {
    if (!chain_built(d1[0].MF, NF, nwv)) continue;
    const ChainGeom g = chain_geom(d1, n, NF);
    if (g.lds <= budget && g.NT >= 64 && 4 * 2 * g.halo <= NF * 16) { *out = g; return NF; }   // <= 25 % of the tile recomputed ...
  }
  return 0;
}

inline bool chain_supported(const ConvDesc* d1, const ConvDesc* d2, int n) {
  if (n < 2 || n > 3) return false;
  for (int q = 0; q < n; ++q) {
    if (!pair_supported(d1[q], d2[q]) || !d1[q].lp || !d2[q].lp) return false;
    if (d1[q].MF != d1[0].MF || d1[q].WM != d1[0].WM || d1[q].CinP != d1[0].CinP || d1[q].taps != d1[0].taps || d1[q].M != d1[0].M) return false;
  }
  const int nwv = block_waves(d1[0]);
  if (d1[0].MF % 2 || nwv != d1[0].WM) return false;             // all waves along the rows, 16-byte epilogue pieces
  ChainGeom g;
  return chain_pick_nf(d1, n, &g) != 0;
}

// the n pairs of one ResBlock chained in one launch; d1[q] / d2[q] are pair q's convs
inline LaunchChoice choose_chain(const ConvDesc* d1, const ConvDesc* d2, const ChainArgs& a, int batch, int dtype) {
  LaunchChoice c;
  c.family = LF_CHAIN;
  if (!chain_supported(d1, d2, a.n)) return choice_error(c, QVC_ERR_BAD_CONFIG);
  for (int q = 1; q < a.n; ++q)
    if (a.p[q].T != a.p[0].T || a.p[q].C != a.p[0].C || a.p[q].CP != a.p[0].CP || a.p[q].bs != a.p[0].bs) return choice_error(c, QVC_ERR_BAD_ARG);
  if (!pair_types(dtype, c)) return choice_error(c, QVC_ERR_BAD_ARG);
  ChainGeom g;
  c.NF = chain_pick_nf(d1, a.n, &g);
  c.MF = d1[0].MF; c.WM = d1[0].WM; c.waves = block_waves(d1[0]); c.block = (unsigned)c.waves * 64;
  c.halo = g.halo; c.margin = g.margin; c.NT = g.NT; c.lds = (int64_t)g.lds;
  c.grid[0] = (unsigned)ceil_div(a.p[0].T, g.NT); c.grid[1] = (unsigned)batch;
  return c;
}

// ------------------------------------------------------------------ WaveNet layer and stacks
// the kernels are built for 4 / 8 / 12 / 16 waves: a launch of `waves` waves runs the next bucket's
inline int wn_wave_bucket(int waves) { return waves <= 4 ? 4 : (waves <= 8 ? 8 : (waves <= 12 ? 12 : 16)); }

inline LaunchChoice choose_wn(const ConvDesc& din, const WnArgs& a, int batch, int dtype) {
  LaunchChoice c;
  c.family = LF_WN_LAYER;
  if (dtype != QVC_F16 && dtype != QVC_BF16) return choice_error(c, QVC_ERR_BAD_ARG);
  c.op = c.ts = dtype;
  // 32-frame tiles unless that leaves most CUs without a workgroup anyway and 64 halves the weight traffic
  const long blocks32 = (long)ceil_div(a.T, 32) * batch;
  c.NF = blocks32 >= 512 ? 4 : 2;
  if (!wn_layout_ok(din)) return choice_error(c, QVC_ERR_BAD_CONFIG);
  c.waves = wn_wave_bucket(din.WM); c.last = a.last ? 1 : 0;
  c.lds = (int64_t)((size_t)(c.NF * 16 + a.taps - 1 + c.NF * 16) * a.HP * 2);
  c.grid[0] = (unsigned)ceil_div(a.T, c.NF * 16); c.grid[1] = (unsigned)batch; c.block = (unsigned)din.WM * 64;
  // hidden = 256 with 64-frame tiles needs (64 + taps-1 + 64) * 512 B > 64 KiB of dynamic LDS: only then the opt-in
  c.optin_above = 64 * 1024;
  return c;
}

// the shapes the continuous-stream kernel (qvc_wn2_impl.h) is built for
inline bool wn2_supported(const ConvDesc& din, const WnStackArgs& a) {
  return wn_layout_ok(din) && din.CinP == 192 && din.taps == 5 && a.layers >= 1 && a.layers <= 4 && wn_stack_nf(din.taps, a.layers) == 3 &&
         a.HP == 192 && a.H <= 192 && a.KS == 6 && a.nIt1 == 30 && (!a.w_post || a.post_mf == 1) && (!a.w_pre || a.pre_KS <= 6);
}
// x (+ gated) tile, fp32 residual + skip slots; the 64-frame tile writes the gated activations over the x tile
constexpr size_t wn2_lds_bytes(int KS, int TAPS, int NF) {
  return (size_t)(NF > 3 ? NF * 16 + TAPS - 1 : NF * 16 + TAPS - 1 + NF * 16) * (KS * 64) + (size_t)2 * NF * (KS * 2 * 64) * 16;
}
constexpr long kWnWideMinTiles = 256;        // 32-frame workgroups (one per CU) from which the 64-frame tile is used

// The continuous-stream kernel for the shipped shape, in a 32- and a 64-frame tile, else the generic stack kernel.  The
// 64-frame tile where the caller allows it (a.wide: not the streaming windows) and the 32-frame grid would fill the chip:
// there it takes the same time per layer on half the CUs.  Smaller grids keep the 32-frame tile: their CUs are
// free anyway, and a tile twice as wide takes longer per layer.  Debug switch "wn_kernel": 1 = the generic kernel,
// 2 = always the 32-frame tile, 3 = always the 64-frame tile (where the kernel applies).
inline LaunchChoice choose_wn_stack(const ConvDesc& din, const WnStackArgs& a, int batch, int dtype) {
  LaunchChoice c;
  const int sw = debug_get(DBG_WN_KERNEL);
  const bool stream = sw != 1 && wn2_supported(din, a);
  c.family = stream ? LF_WN_STACK2 : LF_WN_STACK;
  if (dtype != QVC_F16 && dtype != QVC_BF16) return choice_error(c, QVC_ERR_BAD_ARG);
  c.op = c.ts = dtype;
  c.grid[1] = (unsigned)batch;
  if (stream) {
    const bool wide = sw == 2 ? false : (sw == 3 ? true : a.wide && (long)batch * ceil_div(a.T, kWnOutFrames) >= kWnWideMinTiles);
    constexpr int KS = 6, TAPS = 5;
    c.NF = wide ? 5 : 3; c.ring = wide ? QVC_WN2_WIDE_RING : 6; c.pm = a.w_post ? 1 : 0;
    c.waves = KS * 2; c.block = KS * 2 * 64;
    c.lds = (int64_t)wn2_lds_bytes(KS, TAPS, c.NF);
    c.grid[0] = (unsigned)ceil_div(a.T, c.NF * 16 - 16);
    return c;
  }
  if (!wn_stack_ok(din, a.layers)) return choice_error(c, QVC_ERR_BAD_CONFIG);
  c.NF = wn_stack_nf(a.taps, a.layers);
  c.pm = a.w_post ? a.post_mf : 0;
  if (c.pm > 1) return choice_error(c, QVC_ERR_BAD_CONFIG);
  // tiny batches (<= 64 of the 32-frame tiles: a quarter of the CUs): 16-frame tiles, when the halo fits a 32-column window
  if (c.NF == 3 && 16 + (a.taps - 1) * a.layers <= 32 && (long)batch * ceil_div(a.T, kWnOutFrames) <= 64) c.NF = 2;
  else if (c.NF != 3) c.NF = 6;
  c.waves = wn_wave_bucket(din.WM); c.block = (unsigned)din.WM * 64;
  c.lds = (int64_t)((size_t)(c.NF * 16 + a.taps - 1 + c.NF * 16) * a.HP * 2);
  c.grid[0] = (unsigned)ceil_div(a.T, c.NF == 2 ? 16 : kWnOutFrames);
  return c;
}

// ------------------------------------------------------------------ conv_post + tail
template <int NF, int NB = kBands> struct PostTailGeom {
  static constexpr int MF = NB == 1 ? 2 : 3;    // row fragments per wave in conv_post's packed stream
  static constexpr int WM = NB == 1 ? 1 : 2;    // waves of this kernel along the rows (the other 4/WM split the frames);
                                                // one band: every wave reads the packing's wave-0 stream (rows 0..31)
  static constexpr int NT = (4 / WM) * NF * 16; // post-conv frames of the tile
  static constexpr int HL = NB == 1 ? 2 : 3;    // post-conv frames in front of the first output frame
  static constexpr int OF = NT - (NB == 1 ? 4 : 7);   // output frames owned
  static constexpr int SPF = NB == 1 ? 4 : 16;  // output samples per frame
  static constexpr int OT = OF * SPF;           // output samples owned
  static constexpr int NY = NB == 1 ? 0 : OT / 4 + 15;   // band samples needed (band synthesis only)
  static constexpr int PC = NB * 2 * kBins;     // post-conv channels
  static constexpr int PS = NB == 1 ? 20 : PC;  // LDS floats per post-conv frame (one band: 16-byte rows)
};
template <int NF, int NB = kBands>
inline size_t post_tail_lds(int taps, int CinP) {
  using G = PostTailGeom<NF, NB>;
  const size_t tile = std::max<size_t>((size_t)(G::NT + taps - 1) * CinP * 2, (size_t)G::NT * G::PS * 4);
  return align_up((int64_t)tile, 16) + (size_t)NB * (G::NY + 1) * 4 * (NB > 1 ? 1 : 0);
}
template <int NF, int NB>
inline LaunchChoice post_tail_tile(LaunchChoice c, const ConvDesc& d, const PostTailArgs& a, int batch) {
  static_assert(post_tail_built(NF, NB), "not instantiated");
  c.NF = NF; c.bands = NB;
  c.lds = (int64_t)post_tail_lds<NF, NB>(d.taps, d.CinP);
  if (c.lds > 160 * 1024) return choice_error(c, QVC_ERR_BAD_CONFIG);
  const int n_out = NB * 4 * (a.F - 1);
  c.grid[0] = (unsigned)ceil_div(n_out, PostTailGeom<NF, NB>::OT); c.grid[1] = (unsigned)batch;
  return c;
}

inline LaunchChoice choose_post_tail(const ConvDesc& d, const PostTailArgs& a, int batch, int dtype) {
  LaunchChoice c;
  c.family = LF_POST_TAIL; c.block = 256;
  if (dtype != QVC_F16 && dtype != QVC_BF16) return choice_error(c, QVC_ERR_BAD_ARG);
  c.op = c.ts = dtype;
  const int nb = post_tail_bands(d);
  if (!nb || a.F < 2 || !a.c.x2 || !a.c.x3 || a.c.x_kind != XK_OP_FM) return choice_error(c, QVC_ERR_BAD_CONFIG);
  // one band: 4 waves along the frames at NF 2 = the same 128-frame tile as the four-band default
  if (nb == 1) return post_tail_tile<2, 1>(c, d, a, batch);
  if (!a.fir) return choice_error(c, QVC_ERR_BAD_CONFIG);
  if (debug_get(DBG_POST_TAIL_NF) == 2) return post_tail_tile<2, kBands>(c, d, a, batch);
  return post_tail_tile<4, kBands>(c, d, a, batch);
}

// ------------------------------------------------------------------ the two halves of a launcher
// launch_* (qvc_kernels.h) = choose_* + dispatch_*; these overloads hand the choice back (the timed backend names its
// records from it).  dispatch_* launches `c` as it stands; `stream` is a hipStream_t.
int launch_conv(const ConvDesc& d, ConvArgs a, int batch, int epi, int dtype, void* stream, LaunchChoice& chosen);
int launch_pair3(const ConvDesc* d1, const ConvDesc* d2, const PairArgs3& a, int batch, int dtype, void* stream, LaunchChoice& chosen);
int launch_chain(const ConvDesc* d1, const ConvDesc* d2, ChainArgs a, int batch, int dtype, void* stream, LaunchChoice& chosen);
int launch_wn(const ConvDesc& din, const WnArgs& a, int batch, int dtype, void* stream, LaunchChoice& chosen);
int launch_wn_stack(const ConvDesc& din, const WnStackArgs& a, int batch, int dtype, void* stream, LaunchChoice& chosen);
int launch_post_tail(const ConvDesc& d, PostTailArgs a, int batch, int dtype, void* stream, LaunchChoice& chosen);

// Instantiation entries (one translation unit per operand dtype; the continuous-stream and the chain kernel have their own).
template <typename T> int dispatch_conv(const LaunchChoice& c, const ConvArgs& a, void* stream);
template <typename T, typename TS> int dispatch_pair(const LaunchChoice& c, const PairArgs3& a, void* stream);
template <typename T, typename TS> int dispatch_chain(const LaunchChoice& c, const ChainArgs& a, void* stream);
template <typename T> int dispatch_wn(const LaunchChoice& c, const WnArgs& a, void* stream);
template <typename T> int dispatch_wn_stack(const LaunchChoice& c, const WnStackArgs& a, void* stream);
template <typename T> int dispatch_wn_stack2(const LaunchChoice& c, const WnStackArgs& a, void* stream);
template <typename T> int dispatch_post_tail(const LaunchChoice& c, const PostTailArgs& a, void* stream);

}  // namespace qvc
