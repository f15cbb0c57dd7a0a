/*
 * qvc.h -- C ABI of the MI355X-native QuickVC inference hot path (libqvc_hip.so).
 *
 * This is the drop-in boundary for the path SynthesizerTrn.infer =
 *   enc_p (WN) -> reverse ResidualCouplingBlock -> multi-stream iSTFT generator
 * of tarepan/QuickVC-official.  The reference has no native code; its "FFI" for
 * this path is the Python surface of models.py.  Each entry point below names the
 * reference interface (file:line under the reference checkout) it replaces.  The
 * Python host (quickvc-official_amd/engine.py) binds these with ctypes; see
 * INTEGRATION.md for the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no torch / C++ types.
 *   - every function returns an int status: 0 = QVC_OK, negative = error
 *     (qvc_status_string() names it).  Nothing throws, aborts or prints.
 *   - device pointers are raw HIP device addresses owned by the caller
 *     (tensor.data_ptr()); the library allocates nothing and keeps no global state
 *     (two exceptions, neither reachable from the environment: a per-device flag that
 *     remembers the one-time opt-in to > 64 KiB of LDS, and the developer switches of
 *     qvc_debug_set(), which start at their production values).
 *   - all device work is enqueued asynchronously on the caller's hipStream_t
 *     (passed as void*); no host sync, no allocation, no host read inside, so
 *     every call is hipGraph-capturable.  Thread-safe by statelessness.
 *     Calls on DIFFERENT streams may overlap as long as each has its own workspace, state
 *     and output buffers (the packed weights are read-only and may be shared): bench.py
 *     and convert.py keep two batches in flight that way.
 *   - every entry point that needs scratch has a *_workspace_bytes() query.
 *
 * Layouts
 *   External tensors keep the reference's (B, C, T) contiguous fp32 layout.
 *   Internal activations are "frame-major": [B][T][C] (channel innermost), so that
 *   the 8 consecutive channels one MFMA lane consumes are one 16-byte access.
 */
#ifndef QVC_H
#define QVC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QVC_ABI_VERSION 8

/* ---- status codes ------------------------------------------------------- */
enum {
  QVC_OK = 0,
  QVC_ERR_BAD_ARG = -1,        /* null pointer, non-positive size, bad enum          */
  QVC_ERR_BAD_CONFIG = -2,     /* unsupported hyper-parameters                        */
  QVC_ERR_MISSING_TENSOR = -3, /* a state-dict entry the path needs is absent         */
  QVC_ERR_BAD_SHAPE = -4,      /* a tensor has an unexpected shape                    */
  QVC_ERR_SMALL_BUFFER = -5,   /* blob / workspace smaller than *_bytes() says        */
  QVC_ERR_LAUNCH = -6,         /* hipLaunchKernel / hipGetLastError reported failure  */
  QVC_ERR_NO_DEVICE = -7       /* no HIP device / wrong architecture                  */
};

/* ---- decoder variants (models.py:588) ----------------------------------- */
enum {
  QVC_DEC_ISTFT = 0,       /* iSTFT_Generator            models.py:98-192  (subbands = 1, no band synthesis) */
  QVC_DEC_MULTIBAND = 1,   /* Multiband_iSTFT_Generator  models.py:195-301 (fixed PQMF, pqmf.py:106-117)     */
  QVC_DEC_MULTISTREAM = 2  /* Multistream_iSTFT_Generator models.py:304-415 (learned 63-tap FIR) -- shipped  */
};

/* ---- MFMA operand types -------------------------------------------------- */
enum {
  QVC_BF16 = 0,  /* bf16 operands, fp32 accumulate (BASELINE.json configs 2-5) */
  QVC_F16 = 1,   /* fp16 operands, fp32 accumulate (same MFMA rate, 3 more mantissa bits) */
  QVC_BF16X = 2  /* mixed: bf16 MFMA operands in the fused ResBlock pairs (80 % of the path's FLOPs) with their residual
                    stream kept in fp16 (same bytes; the identity path of 18 chained pairs keeps 11 mantissa bits), fp16
                    everywhere else.  All-bf16 misses the 40 dB waveform bar (34 dB measured); this mode meets it */
};

#define QVC_MAX_UPS 4
#define QVC_MAX_RESBLOCKS 4

/*
 * Hyper-parameters of SynthesizerTrn (models.py:551-591) that shape the path.
 * Filled by the host from the reference's JSON "model" section.
 */
typedef struct qvc_config {
  int32_t unit_channels;            /* 256, hard-coded at models.py:579                 */
  int32_t inter_channels;           /* latent z channels                                 */
  int32_t hidden_channels;          /* WN width                                          */
  int32_t gin_channels;             /* speaker embedding size                            */
  int32_t wn_kernel_size;           /* 5  (models.py:582-584)                            */
  int32_t enc_layers;               /* 16 (models.py:583)                                */
  int32_t flow_layers;              /* 4  WN layers per coupling layer (models.py:584)   */
  int32_t n_flows;                  /* 4                                                  */
  int32_t upsample_initial_channel; /* 512                                               */
  int32_t n_ups;                    /* len(upsample_rates)                               */
  int32_t upsample_rates[QVC_MAX_UPS];
  int32_t upsample_kernel_sizes[QVC_MAX_UPS];
  int32_t n_resblocks;              /* len(resblock_kernel_sizes)                        */
  int32_t resblock_kernel_sizes[QVC_MAX_RESBLOCKS];
  int32_t resblock_dilations[QVC_MAX_RESBLOCKS][3];
  int32_t n_fft;                    /* gen_istft_n_fft  (16)                             */
  int32_t hop;                      /* gen_istft_hop_size (4)                            */
  int32_t subbands;                 /* 4 (1 for QVC_DEC_ISTFT)                           */
  int32_t decoder;                  /* QVC_DEC_*                                         */
  int32_t fir_taps;                 /* 63: multistream_conv_post / PQMF taps+1           */
  int32_t operand_dtype;            /* QVC_BF16 / QVC_F16                                */
  int32_t n_mel_channels;           /* SpeakerEncoder input size (models.py:508); 0 = 80  */
  int32_t spec_channels;            /* enc_q input size = filter_length/2+1 (convert.py:35); 0 = 641 */
} qvc_config;

/* One named fp32 tensor of the reference checkpoint's state_dict (utils.py:183-193). */
typedef struct qvc_tensor {
  const char* name;    /* e.g. "enc_p.enc.in_layers.3.weight_v"  */
  const float* data;   /* host pointer, contiguous fp32           */
  int32_t ndim;
  int64_t shape[4];
} qvc_tensor;

/* ---- library info ---------------------------------------------------------- */
int qvc_abi_version(void);
const char* qvc_status_string(int status);
/* 0 when a gfx950 device is visible to this process, QVC_ERR_NO_DEVICE otherwise. */
int qvc_device_check(void);

/* Developer / test switches (launch-shape and kernel-selection variants that must give identical results; the GPU
 * tests flip them in-process).  The library never reads environment variables: a switch changes only through this
 * call.  Names: "post_tail", "post_tail_nf", "pair_wide_launch", "pair_cm4", "conv_cl", "wn_chunk", "pair_chain3",
 * "wn_kernel", "live_trim" (1: qvc_live_step trims each stage's window, 0: every stage over the whole window), "launch_stop" (-1 = off; n >= 0: the whole-path entry points -- qvc_infer_batch[_ex|_timed|_ragged[_fm]],
 * qvc_infer_fanout_ragged[_fm], qvc_enc_q, qvc_flow_forward -- issue only their first n launches).  qvc_debug_get also reads "launch_steps" (read-only:
 * the launches the last such call would have issued without a stop).  Unknown name: QVC_ERR_BAD_ARG.  No reference
 * counterpart. */
int qvc_debug_set(const char* name, int32_t value);
int qvc_debug_get(const char* name, int32_t* value);
/* fp32 -> f16 conversions that SATURATED (|x| > 65504) since the last reset, summed over all kernels.  Counted only
 * by the debug build libqvc_hip_sat.so (-DQVC_SATCOUNT; synchronises the device): an activation range the f16
 * streams cannot carry becomes a number instead of passing silently.  The product library spends no instruction on
 * it and returns QVC_ERR_BAD_CONFIG with *count = -1. */
int qvc_debug_saturations(int64_t* count, int32_t reset);

/* ---- weights: replaces nn.Module.load_state_dict + per-forward weight_norm ----
 * Reference: utils.py:148-180 (load), modules.py:54,64,67,134-143 and
 * models.py:327,333,346,357 (weight_norm recomputed every forward).  Folds
 * w = g*v/||v|| once, folds the four channel Flips (modules.py:165-170) into the
 * coupling layers' weight layout, rewrites ConvTranspose1d as polyphase filters,
 * converts to the MFMA operand type and lays everything out as per-wave
 * fragment streams.  Pure host code.
 */
int64_t qvc_blob_bytes(const qvc_config* cfg);
int qvc_pack_weights(const qvc_config* cfg, const qvc_tensor* tensors, int32_t n_tensors,
                     void* blob_host, int64_t blob_bytes);

/* ---- whole path: replaces SynthesizerTrn.infer after the speaker encoder ------
 * Reference: models.py:638-642 (z_p = enc_p(unit); z = flow(z_p, g, reverse);
 * o = dec(z, g)), generalised to a batch of utterances with per-utterance g.
 *   unit  (B, unit_channels, T) fp32   HuBERT-soft units          (convert.py:79)
 *   g     (B, gin_channels)     fp32   speaker embeddings          (models.py:635)
 *   noise (B, inter_channels, T) fp32  the N(0,1) draw of models.py:94
 *   out   (B, T*prod(ups)*hop*subbands) fp32 waveform = (B,1,320*T)
 */
int64_t qvc_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t frames);
/* Layout decisions the plan takes for `cfg` (diagnostics; no reference counterpart): info[0] enc_p.proj rows paired
 * [mu | log sigma] (sampling in the conv epilogue), [1] its fragments per wave, [2..3] up-samplers 0 / 1 lane-packed,
 * [4] conv_post + iSTFT / band synthesis can run as one launch, [5..6] waves per workgroup of the stage 0 / 1 ResBlock
 * pairs, [7] every ResBlock pair runs fused, three chains per launch (then qvc_aux branches are never taken). */
int qvc_plan_info(const qvc_config* cfg, int32_t info[8]);
int qvc_infer_batch(const qvc_config* cfg, const void* blob_dev,
                    const float* unit, const float* g, const float* noise, float* out,
                    int32_t batch, int32_t frames,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the same for a RAGGED batch: utterances of different lengths in one launch sequence ------------------
 * The reference converts one utterance of any length per call (convert.py:58-86, models.py:625-642); a batched
 * drop-in therefore has to take utterances of different lengths.  unit / noise are padded to max_frames
 * ((B, C, max_frames), the padding's content is ignored), frames_dev is a DEVICE array of `batch` int32 lengths
 * (1 < frames_dev[b] <= max_frames; not validated on the host: the call is asynchronous; values are clamped
 * to [0, max_frames] on the device), and every conv / WaveNet layer / iSTFT frame sees utterance b end at
 * frames_dev[b] (zero padding at ITS end, as in the reference).  out is (B, 320*max_frames): the first
 * 320*frames_dev[b] samples of row b equal the waveform of utterance b converted alone, the rest are zeros.
 * Same workspace as qvc_infer_batch(cfg, batch, max_frames).
 */
int qvc_infer_batch_ragged(const qvc_config* cfg, const void* blob_dev,
                           const float* unit, const float* g, const float* noise, float* out,
                           int32_t batch, int32_t max_frames, const int32_t* frames_dev,
                           void* workspace, int64_t workspace_bytes, void* stream);
/* The same with the units as they are ON DISK: dataset/encode.py:33-38 saves each utterance's HuBERT-soft units as a
 * (frames, 256) float32 .npy, data_utils_new_new.py:121-122 transposes after loading.  unit_fm is [B][max_frames][256]
 * (frame-major, row b padded to max_frames; padding content ignored), so a batch of files can be read straight into
 * the upload buffer (include/qvc_io.h) with no host-side transpose. */
int qvc_infer_batch_ragged_fm(const qvc_config* cfg, const void* blob_dev,
                              const float* unit_fm, const float* g, const float* noise, float* out,
                              int32_t batch, int32_t max_frames, const int32_t* frames_dev,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* ---- fan-out: R output rows from U <= R distinct sources (any-to-many conversion) -------------------------------
 * The usual list for the reference's convert.py:58-86 names one source once per target speaker.  Nothing ahead of the
 * draw z_p = mu + eps * exp(log sigma) (models.py:93-94) depends on the speaker -- in models.py:638-640 only the flow
 * and the decoder see g -- so the sources are encoded ONCE each (enc_p at batch `sources`, as far as the projection's
 * statistics), one small launch draws z_p for every row from its source's statistics with the row's own noise, and
 * flow + decoder run at batch `rows`.
 *   unit            (U, unit_channels, max_frames) fp32, padded (_fm: [U][max_frames][unit_channels], as on disk)
 *   frames_dev      DEVICE int32 [U]: the sources' lengths (as qvc_infer_batch_ragged's; clamped on the device)
 *   src_of_row_dev  DEVICE int32 [R]: the source of every output row; clamped to [0, U-1] on the device
 *   g (R, gin), noise (R, inter_channels, max_frames), out (R, 320*max_frames): per output row
 * Row r of `out` follows qvc_infer_batch_ragged's contract: its first 320*frames_dev[src[r]] samples are the waveform
 * of source src[r] converted with g[r] and noise[r] -- what qvc_infer_batch_ragged gives for the expanded batch --, the
 * rest are zeros.  1 <= sources <= rows (else QVC_ERR_BAD_ARG).  A source that no row refers to costs its share of
 * enc_p time and nothing else.  Asynchronous, allocation-free and without a host read of any device array (map and
 * lengths included), so a captured call can be replayed with other maps and lengths.  The workspace is
 * qvc_workspace_bytes(cfg, rows, max_frames) plus the per-row length array: qvc_fanout_workspace_bytes (a negative
 * QVC_ERR_* for bad arguments / configs, as the other size queries).  Offline only: no streaming form. */
int64_t qvc_fanout_workspace_bytes(const qvc_config* cfg, int32_t sources, int32_t rows, int32_t max_frames);
int qvc_infer_fanout_ragged(const qvc_config* cfg, const void* blob_dev,
                            const float* unit, const int32_t* frames_dev, const int32_t* src_of_row_dev,
                            const float* g, const float* noise, float* out,
                            int32_t sources, int32_t rows, int32_t max_frames,
                            void* workspace, int64_t workspace_bytes, void* stream);
int qvc_infer_fanout_ragged_fm(const qvc_config* cfg, const void* blob_dev,
                               const float* unit_fm, const int32_t* frames_dev, const int32_t* src_of_row_dev,
                               const float* g, const float* noise, float* out,
                               int32_t sources, int32_t rows, int32_t max_frames,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* ---- streaming: one hop of new unit frames per call, state in a caller-owned buffer (BASELINE configs[4]) -----
 * The reference converts whole utterances; every op of the path is a bounded, symmetric
 * convolution, so the path also runs as a pipeline of segments (enc_p | each coupling layer | conv_pre+stage 0 |
 * stage 1+conv_post+iSTFT), each fed from a ring that keeps the last 2*H frames of its input: a frame costs
 * (2*H + hop)/hop of its offline cost per segment (1.08x at hop 320) and the output lags the input by
 * qvc_stream_lag_frames() frames -- the look-ahead a non-causal network needs.  Sequence starts and ends are
 * exact: every kernel masks rows by the window's absolute position.  csrc/qvc_stream.h has the details.
 *   state      caller-owned device buffer of qvc_stream_state_bytes(), ZEROED before a stream's first step
 *   unit_new   (B, unit_channels, hop) fp32: unit frames [pos[b], pos[b] + hop) (anything past the sequence end)
 *   noise_new  (B, inter_channels, hop) fp32: the N(0,1) draw of models.py:94 for frames
 *              [pos[b] - qvc_stream_noise_lag_frames(), ... + hop)  (the frames enc_p completes in this step)
 *   out        (B, hop * samples_per_frame) fp32: frames [pos[b] - lag, pos[b] - lag + hop); zeros outside [0, len[b])
 *   pos_dev, len_dev  device int32 [B]: first new frame of this step / sequence length (a large number while unknown).
 *              The caller advances pos by hop between steps (device arrays: a captured graph replays unchanged).
 * To flush a stream of length L keep stepping (inputs ignored) until pos - lag >= L.
 */
int64_t qvc_stream_state_bytes(const qvc_config* cfg, int32_t batch, int32_t hop);
int64_t qvc_stream_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t hop);
int32_t qvc_stream_lag_frames(const qvc_config* cfg);
int32_t qvc_stream_noise_lag_frames(const qvc_config* cfg);
int qvc_stream_step(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes,
                    const float* unit_new, const float* g, const float* noise_new, float* out,
                    int32_t batch, int32_t hop, const int32_t* pos_dev, const int32_t* len_dev,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* Admit a NEW stream into slot `slot` of a running batch (a server whose streams start and end at different times):
 * zeroes that slot's rows of every ring in `state` and sets pos_dev[slot] = 0, len_dev[slot] = length (a large number
 * while unknown) on `stream`.  The other slots are untouched, a captured step graph is replayed unchanged (it only
 * holds pointers), and the caller copies the new stream's g row itself.  Ending a stream = writing its length into
 * len_dev[slot]; the slot is free again once pos - lag >= length.  No reference counterpart. */
int qvc_stream_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop,
                          int32_t slot, int32_t length, int32_t* pos_dev, int32_t* len_dev, void* stream);

/* ---- the noise drawn on the device: a counter-based generator instead of a noise tensor ---------------------------
 * The N(0,1) draw of models.py:94 as a pure function of (seed, utterance key, channel, absolute frame), computed where
 * it is consumed: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (frame, channel / 4,
 * key & 0xffffffff, key >> 32); the four outputs give the normals of channels 4g .. 4g+3 by Box-Muller from 24-bit
 * uniforms (DESIGN.md has the exact recipe).  What an utterance gets depends on ITS key alone -- not on the batch it
 * rides in, its row, the padding, the shard, or the streaming window -- so an utterance converted alone, in any batch,
 * as a fan-out row or streamed under the same (seed, key) draws the same noise.  Rows with equal keys draw equal noise.
 * Each _rng entry point is its twin above with `rng` in place of the noise pointer: same arguments, same workspace
 * query, asynchronous, allocation-free, graph-capturable; nothing of a noise tensor is allocated, staged or read.
 *   keys_dev   DEVICE uint64, one key per row (fan-out: per OUTPUT row; streaming: per slot); read in [0, rows) only.
 *              Streaming: the caller writes keys_dev[slot] when it admits a stream, as it does with the slot's g row;
 *              the frame of the counter is the stream's absolute frame, so there is no noise lag to align.
 *   scale      noise_scale: multiplies the normal; 1.0f = the reference's draw, 0.0f = the deterministic mean conversion
 * The descriptor itself is read on the host during the call (its fields are baked into the launches). */
typedef struct qvc_noise_rng {
  uint64_t seed;
  const uint64_t* keys_dev;   /* DEVICE, one key per row / stream slot; read in [0, rows) only */
  float scale;                /* noise_scale; 1.0f = the reference's draw */
} qvc_noise_rng;
int qvc_infer_batch_ragged_rng(const qvc_config* cfg, const void* blob_dev,
                               const float* unit, const float* g, const qvc_noise_rng* rng, float* out,
                               int32_t batch, int32_t max_frames, const int32_t* frames_dev,
                               void* workspace, int64_t workspace_bytes, void* stream);
int qvc_infer_batch_ragged_rng_fm(const qvc_config* cfg, const void* blob_dev,
                                  const float* unit_fm, const float* g, const qvc_noise_rng* rng, float* out,
                                  int32_t batch, int32_t max_frames, const int32_t* frames_dev,
                                  void* workspace, int64_t workspace_bytes, void* stream);
int qvc_infer_fanout_ragged_rng(const qvc_config* cfg, const void* blob_dev,
                                const float* unit, const int32_t* frames_dev, const int32_t* src_of_row_dev,
                                const float* g, const qvc_noise_rng* rng, float* out,
                                int32_t sources, int32_t rows, int32_t max_frames,
                                void* workspace, int64_t workspace_bytes, void* stream);
int qvc_infer_fanout_ragged_rng_fm(const qvc_config* cfg, const void* blob_dev,
                                   const float* unit_fm, const int32_t* frames_dev, const int32_t* src_of_row_dev,
                                   const float* g, const qvc_noise_rng* rng, float* out,
                                   int32_t sources, int32_t rows, int32_t max_frames,
                                   void* workspace, int64_t workspace_bytes, void* stream);
int qvc_stream_step_rng(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes,
                        const float* unit_new, const float* g, const qvc_noise_rng* rng, float* out,
                        int32_t batch, int32_t hop, const int32_t* pos_dev, const int32_t* len_dev,
                        void* workspace, int64_t workspace_bytes, void* stream);
/* The generator's draw written out: noise_out (rows, channels, frames) fp32 in the reference's layout holds the normals
 * of frames [frame0, frame0 + frames) for keys_dev[0 .. rows) -- the tensor that, handed to a pointer entry point, gives
 * the bits of its _rng twin (the bridge between the two forms, and the way to inspect a draw).  channels % 4 == 0. */
int qvc_noise_fill(uint64_t seed, const uint64_t* keys_dev, float scale, int32_t rows, int32_t channels, int32_t frames,
                   int32_t frame0, float* noise_out, void* stream);

/* ---- streaming with a bounded look-ahead: a windowed step for EVERY decoder ---------------------------------------
 * qvc_stream_step is exact and cheap, but its output lags the input by the whole receptive field (90 frames = 1.8 s at
 * the shipped config) and it takes the band-synthesis decoders with two up-samplers only.  qvc_live_step lets the
 * caller choose the lag, L = look_ahead in [0, C], C = qvc_live_context_frames(cfg), and takes every configuration the
 * offline path takes.  The state is ONE ring per stream: the last W = C + L + hop unit frames (and their noise frames).
 * A step appends the new frames, runs the whole path over the W-row window -- whose last row is the newest frame, so
 * the kernels see a sequence that ends there -- and delivers rows [C, C + hop):
 *   out = frames [pos[b] - L, pos[b] - L + hop) of qvc_infer_batch_ragged on the stream's first min(len, pos + hop)
 *   frames (same g, same noise or (seed, key)); zeros outside [0, len[b]).
 * That is the prefix conversion, defined exactly, not an approximation of the whole-utterance result; with L = C the
 * two agree and the concatenated outputs ARE the whole-utterance conversion (exact streaming -- for the single-band
 * decoder and one-up-sampler decoders the only streaming form).  A frame costs (C + L + hop) / hop of its offline cost
 * in enc_p, less in the stages after it: rows a stage can no longer use are dropped before the next stage runs.
 *   state      caller-owned device buffer of qvc_live_state_bytes(); a slot is started with qvc_live_reset_slot
 *              (or the whole buffer zeroed and pos = 0)
 *   unit_new   (B, unit_channels, hop) fp32: unit frames [pos[b], pos[b] + hop) (anything past the sequence end)
 *   noise_new  (B, inter_channels, hop) fp32: the N(0,1) draw for the SAME frames -- no noise lag.  The _rng twin
 *              draws at the absolute frame of every window row instead (keys_dev: one key per slot)
 *   out        (B, hop * samples_per_frame) fp32
 *   pos_dev, len_dev  as qvc_stream_step: the caller advances pos by hop between steps; a stream of length n is
 *              flushed once pos - L >= n.
 * hop < 1, batch < 1 or look_ahead outside [0, C]: QVC_ERR_BAD_ARG (the size queries return the code as their value).
 * Asynchronous, allocation-free, capturable on one stream.  csrc/qvc_stream.h (live_step) has the details. */
int32_t qvc_live_context_frames(const qvc_config* cfg);
int64_t qvc_live_state_bytes(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead);
int64_t qvc_live_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead);
int qvc_live_step(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes,
                  const float* unit_new, const float* g, const float* noise_new, float* out,
                  int32_t batch, int32_t hop, int32_t look_ahead, const int32_t* pos_dev, const int32_t* len_dev,
                  void* workspace, int64_t workspace_bytes, void* stream);
int qvc_live_step_rng(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes,
                      const float* unit_new, const float* g, const qvc_noise_rng* rng, float* out,
                      int32_t batch, int32_t hop, int32_t look_ahead, const int32_t* pos_dev, const int32_t* len_dev,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* Admit a new stream into slot `slot`: zeroes that slot's ring rows and sets pos_dev[slot] = 0, len_dev[slot] = length
 * on `stream` (as qvc_stream_reset_slot; the caller copies the slot's g row and generator key itself). */
int qvc_live_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop,
                        int32_t look_ahead, int32_t slot, int32_t length, int32_t* pos_dev, int32_t* len_dev, void* stream);

/* ---- the tick form of the windowed step: per-slot frame counts per call ------------------------------------------
 * qvc_live_step moves every slot by exactly `hop` frames.  A real audio front end does not deliver like that: a packet
 * is late (nothing at this tick), a client catches up (less or more than usual), the last chunk is short.  In a tick
 * slot b brings n = clamp(n_new_dev[b], 0, hop) frames -- the counts live in device memory, are clamped there and never
 * read on the host; `hop` is the MOST a slot may bring and sizes the buffers and the window W = C + L + hop.
 *   unit_new   (B, unit_channels, hop) fp32: columns [0, n) of row b are frames [pos[b], pos[b] + n); columns [n, hop)
 *              -- the whole row of a slot with n = 0 -- are never read
 *   noise_new  (B, inter_channels, hop) fp32, the same rule: the draw for the same frames.  The _rng twin draws at the
 *              absolute frame of every window row with the slot's key instead
 *   out        (B, hop * samples_per_frame) fp32: the first n * samples_per_frame samples of row b are frames
 *              [pos[b] - L, pos[b] - L + n) of qvc_infer_batch_ragged on the stream's first min(len[b], pos[b] + n)
 *              frames (zeros outside [0, len[b])); the rest of the row is written as 0.0
 *   pos_dev    advanced on the device by the call: pos[b] += n (hence not const)
 * A slot with n = 0 leaves no trace: ring rows and pos bit for bit as they were, a row of zeros in `out`, its tiles
 * return at once.  One captured graph of the call replays for any tick pattern: only the contents of n_new_dev,
 * pos_dev, len_dev, unit_new and noise_new change between replays.  With every n = hop the outputs, and the ring bytes
 * a later call can read, are bit for bit qvc_live_step's.  With L = C the concatenated output of a stream is its whole-utterance conversion however the
 * stream was cut into ticks; with L < C a frame is delivered with between L and L + n - 1 frames of look-ahead, so the
 * output legitimately depends on the cut.
 *   state      the state of qvc_live_step: qvc_live_state_bytes(), started per slot with qvc_live_reset_slot
 *              (qvc_live_tick_state_bytes and qvc_live_tick_reset_slot are other names for the same two calls).  Between
 *              calls, ring row r of slot b holds frame pos[b] - (W - hop) + r for r in [0, W - hop): the last W - hop
 *              frames, left-aligned; the hop rows behind them are rewritten before they are read.  Both calls leave the
 *              rings like that, so a server may switch between qvc_live_step and qvc_live_tick on one state at any call
 *              (the caller advances pos after a step; a tick advances it itself).
 *   workspace  qvc_live_tick_workspace_bytes() (more than qvc_live_workspace_bytes())
 * Errors as qvc_live_step; n_new_dev == NULL: QVC_ERR_BAD_ARG.  The segment rings have a tick form of their own:
 * qvc_stream_tick, below. */
int64_t qvc_live_tick_state_bytes(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead);
int64_t qvc_live_tick_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t hop, int32_t look_ahead);
int qvc_live_tick(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes,
                  const float* unit_new, const float* g, const float* noise_new, float* out,
                  int32_t batch, int32_t hop, int32_t look_ahead, const int32_t* n_new_dev, int32_t* pos_dev,
                  const int32_t* len_dev, void* workspace, int64_t workspace_bytes, void* stream);
int qvc_live_tick_rng(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes,
                      const float* unit_new, const float* g, const qvc_noise_rng* rng, float* out,
                      int32_t batch, int32_t hop, int32_t look_ahead, const int32_t* n_new_dev, int32_t* pos_dev,
                      const int32_t* len_dev, void* workspace, int64_t workspace_bytes, void* stream);
int qvc_live_tick_reset_slot(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop,
                             int32_t look_ahead, int32_t slot, int32_t length, int32_t* pos_dev, int32_t* len_dev, void* stream);

/* ---- the tick form of the segment rings: per-slot frame counts per call ------------------------------------------------
 * qvc_stream_step moves every slot by exactly `hop` frames, so one late packet stalls every other stream of the batch.  In
 * a tick slot b brings n = clamp(n_new_dev[b], 0, hop) frames.  The counts live in device memory, are read and clamped
 * there and never on the host; `hop` is the MOST a slot may bring and sizes every buffer and launch.
 *   unit_new   (B, unit_channels, hop) fp32: columns [0, n) of row b are frames [pos[b], pos[b] + n); columns [n, hop) --
 *              the whole row of a slot with n = 0 -- are never read
 *   noise_new  (B, inter_channels, hop) fp32, the same rule: the draw for frames [pos[b] - noise_lag, pos[b] - noise_lag
 *              + n), noise_lag = qvc_stream_noise_lag_frames().  The _rng twin draws at the absolute frame with the
 *              slot's key instead
 *   out        (B, hop * samples_per_frame) fp32: the first n * samples_per_frame samples of row b are frames
 *              [pos[b] - lag, pos[b] - lag + n) of the stream's whole-utterance conversion (qvc_infer_batch_ragged with the
 *              same g and the same noise or (seed, key)), zeros outside [0, len[b]); the rest of the row is written as 0.0
 *   pos_dev    advanced on the device by the call: pos[b] += n (hence not const)
 * A slot with n = 0 leaves no trace: its rows of every ring and its pos bit for bit as they were, a row of zeros in
 * `out`, its workgroups return at once.  One captured graph of the call replays for any tick pattern: only the contents
 * of n_new_dev, pos_dev, len_dev, unit_new and noise_new change between replays.
 * With every n = hop, `out` is bit for bit qvc_stream_step's, and so is every ring byte a later call can read (the kept
 * 2*H frames of every ring; the hop frames behind them are rewritten before they are read and may differ).
 * The segment rings are exact, so a stream's concatenated output is its whole-utterance conversion HOWEVER the stream
 * was cut into ticks -- stronger than qvc_live_tick, which has that at L = C only.
 *   state      the state of qvc_stream_step: qvc_stream_state_bytes(), started per slot with qvc_stream_reset_slot (or
 *              zeroed with pos = 0).  Both calls leave the rings in the same layout, so a server may switch between
 *              qvc_stream_step and qvc_stream_tick on one state at any call.
 *   workspace  qvc_stream_tick_workspace_bytes() (more than qvc_stream_workspace_bytes())
 * Errors as qvc_stream_step's, in the same order; n_new_dev == NULL: QVC_ERR_BAD_ARG.  The configurations
 * qvc_stream_step refuses (the single-band decoder, decoders without exactly two up-samplers) get QVC_ERR_BAD_CONFIG
 * here too, from the size query as well.  Asynchronous, allocation-free, capturable on one stream.
 * csrc/qvc_stream.h (stream_tick) has the details. */
int64_t qvc_stream_tick_workspace_bytes(const qvc_config* cfg, int32_t batch, int32_t hop);
int qvc_stream_tick(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes,
                    const float* unit_new, const float* g, const float* noise_new, float* out,
                    int32_t batch, int32_t hop, const int32_t* n_new_dev, int32_t* pos_dev, const int32_t* len_dev,
                    void* workspace, int64_t workspace_bytes, void* stream);
int qvc_stream_tick_rng(const qvc_config* cfg, const void* blob_dev, void* state, int64_t state_bytes,
                        const float* unit_new, const float* g, const qvc_noise_rng* rng, float* out,
                        int32_t batch, int32_t hop, const int32_t* n_new_dev, int32_t* pos_dev, const int32_t* len_dev,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---- slot snapshots: move a running segment-ring stream between slots, batch sizes, hops, devices and processes ---
 * Between two calls of qvc_stream_step / qvc_stream_tick a stream IS the kept 2*H frames of its rows of every ring plus
 * pos[slot] and len[slot] (the hop frames behind the kept ones are rewritten before they are read).  None of that
 * depends on the batch size, the slot or the hop, so a snapshot cut from one state continues in any slot of any other
 * state of the same model: another converter, a larger or smaller batch, another hop, after a trip through host
 * memory.  A snapshot of one slot is qvc_stream_snapshot_bytes() bytes (a multiple of 256; a function of the
 * configuration alone): per ring, in the order the rings lie in the state, the kept part of the slot's rows, each ring
 * 256-byte aligned; then pos and len as two int32.
 *   qvc_stream_snapshot_tag   a 64-bit fingerprint of that layout: a format version, cfg.operand_dtype (the stage-0
 *              rings are stored in the operand type), the decoder kind, the channel counts, the reaches of the five
 *              kinds of segment and every ring's rows and kept bytes.  It does not depend on batch, hop or the weights:
 *              two snapshots are interchangeable when their tags are equal AND they come from the same checkpoint.  The
 *              caller stores the tag beside the bytes; the library does not.
 *   qvc_stream_export_slots   snapshot i (at snap_dev + i * qvc_stream_snapshot_bytes()) <- slot slots_host[i].  Reads only.
 *   qvc_stream_import_slots   slot slots_host[i] <- snapshot i: writes the kept part of that slot's rows of every ring,
 *              pos_dev[slot] and len_dev[slot], and NOTHING else -- not the hop part of the rows, not another slot.
 *              The slots of one import must be distinct.
 *   state, batch, hop   the state the slots live in, as passed to qvc_stream_step / _tick for it
 *   slots_host HOST int32 [n_slots], each in [0, batch); read during the call (baked into the launches)
 *   snap_dev   DEVICE, 256-byte aligned, n_slots snapshots back to back; snap_bytes >= n_slots * qvc_stream_snapshot_bytes()
 * As with qvc_stream_reset_slot the caller moves the slot's g row and generator key itself.  Both calls only enqueue
 * batched strided copies on `stream`: asynchronous, allocation-free, graph-capturable.  Checks, in this order:
 * QVC_ERR_BAD_ARG for a null cfg / state / pos_dev / len_dev / snap_dev / slots_host, batch < 1, n_slots < 1 or a slot
 * outside [0, batch); the plan -- QVC_ERR_BAD_ARG for hop < 1, QVC_ERR_BAD_CONFIG for what qvc_stream_step refuses (the
 * single-band decoder, decoders without exactly two up-samplers; from the two queries too); QVC_ERR_SMALL_BUFFER for
 * state_bytes or snap_bytes too small; QVC_ERR_BAD_ARG for a state or snap_dev that is not 256-byte aligned.  A refused
 * call launches nothing.  The windowed step (qvc_live_*) is not covered: its state is the caller's own last C + L input
 * frames.  csrc/qvc_stream.h (SnapLayout, move_slots) has the details. */
int64_t qvc_stream_snapshot_bytes(const qvc_config* cfg);
int qvc_stream_snapshot_tag(const qvc_config* cfg, uint64_t* tag);
int qvc_stream_export_slots(const qvc_config* cfg, const void* state, int64_t state_bytes, int32_t batch, int32_t hop,
                            const int32_t* slots_host, int32_t n_slots, const int32_t* pos_dev, const int32_t* len_dev,
                            void* snap_dev, int64_t snap_bytes, void* stream);
int qvc_stream_import_slots(const qvc_config* cfg, void* state, int64_t state_bytes, int32_t batch, int32_t hop,
                            const int32_t* slots_host, int32_t n_slots, int32_t* pos_dev, int32_t* len_dev,
                            const void* snap_dev, int64_t snap_bytes, void* stream);

/* ---- exact windows over packed utterances: recordings of any length, offline -----------------------------------------
 * Every whole-path call above sizes its buffers by rows x longest utterance, so one hour-long recording in a batch makes
 * the batch unallocatable.  Here many WINDOWS ride one call as its rows, cut from utterances of any lengths that lie back
 * to back in packed buffers and addressed through a table in device memory: memory is bounded by rows x window whatever
 * the lengths, one long recording converts at batch rate, and every row has its own g row (a target speaker per region).
 *   unit_fm_packed  [total_frames][unit_channels] fp32: the utterances as they are on disk (dataset/encode.py:38), back to back
 *   noise_packed    (inter_channels, total_frames) fp32: frame f of an utterance is column base + f.  The _rng twin draws
 *                   at the absolute frame of every window row instead; keys_dev holds one key per ROW (rows of one
 *                   utterance carry that utterance's key)
 *   win_dev         DEVICE qvc_window [rows], never read on the host
 *   g               (rows, gin_channels)
 *   out_packed      [total_frames * samples_per_frame] fp32, laid out as the units are
 * With n = window_frames and C = qvc_live_context_frames(cfg), a row's window is the W = 2C + n frames
 * [start - C, start + n + C) of its utterance (zeros outside [0, length)); the row delivers frames [start, start + count)
 * to out_packed[(base + start) * samples_per_frame ...] and NOTHING else of out_packed is written.  The delivered frames
 * are those of qvc_infer_batch_ragged[_rng] on the whole utterance with the same g and the same noise or (seed, key):
 * the windowed step at look_ahead = C (qvc_live_step above), where prefix and whole-utterance conversion agree.  A frame
 * costs (2C + n) / n of its offline cost in enc_p, less in the stages behind it.
 * The table is clamped on the device: base and length to total_frames, start to [0, length], count to
 * [0, min(n, length - start)]; no table content makes a launch touch memory outside the caller's buffers.  A row with
 * count = 0 is idle: an empty sequence, nothing of it is read or delivered.  Rows that deliver overlapping ranges race.
 * Asynchronous, allocation-free, no host read of any device array: a captured call replays with another table, other
 * lengths and other packed contents.  Checks, in the order of qvc_live_step's: QVC_ERR_BAD_ARG for a null pointer,
 * rows < 1 (or > 65535), window_frames < 1, total_frames < 1 or 2C + n > 1 << 24; QVC_ERR_BAD_CONFIG for a bad plan;
 * QVC_ERR_SMALL_BUFFER for a small workspace; QVC_ERR_BAD_ARG for a workspace or blob that is not 256-byte aligned.  A
 * refused call launches nothing; the size query returns the code as its value.  csrc/qvc_stream.h (infer_windows). */
typedef struct qvc_window {   /* one row of a call; DEVICE memory; never read on the host */
  int32_t base;    /* first frame of the row's utterance in the packed buffers          */
  int32_t length;  /* that utterance's length in frames                                  */
  int32_t start;   /* first delivered frame, relative to the utterance                   */
  int32_t count;   /* delivered frames; 0 = idle row                                      */
} qvc_window;
int64_t qvc_windows_workspace_bytes(const qvc_config* cfg, int32_t rows, int32_t window_frames);
int qvc_infer_windows_fm(const qvc_config* cfg, const void* blob_dev, const float* unit_fm_packed, const float* noise_packed,
                         const qvc_window* win_dev, const float* g, float* out_packed,
                         int32_t rows, int32_t window_frames, int32_t total_frames,
                         void* workspace, int64_t workspace_bytes, void* stream);
int qvc_infer_windows_rng_fm(const qvc_config* cfg, const void* blob_dev, const float* unit_fm_packed, const qvc_noise_rng* rng,
                             const qvc_window* win_dev, const float* g, float* out_packed,
                             int32_t rows, int32_t window_frames, int32_t total_frames,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---- optional fork/join resources: lets the three independent ResBlocks of an MRF stage
 * (models.py:378-384) run as parallel branches (two auxiliary non-blocking streams + events), so a
 * memory-bound k=3 launch overlaps a compute-bound k=11 launch.  Created/destroyed by the caller
 * outside the hot call; with aux == NULL everything runs on `stream` in the same order.  Works under
 * hipGraph capture of `stream` (the branches become parallel graph nodes).
 */
typedef struct qvc_aux qvc_aux;
int qvc_aux_create(qvc_aux** out);
int qvc_aux_destroy(qvc_aux* aux);
int qvc_infer_batch_ex(const qvc_config* cfg, const void* blob_dev,
                       const float* unit, const float* g, const float* noise, float* out,
                       int32_t batch, int32_t frames,
                       void* workspace, int64_t workspace_bytes, void* stream, qvc_aux* aux);

/* ---- the same call with per-launch timing (diagnostics for bench.py's roofline leg) ----
 * Runs the identical launch sequence but brackets every launch with HIP events recorded on
 * `stream`, synchronises the stream at the end and fills `records` (at most max_records;
 * *n_records receives the number of launches).  Creates/destroys events, so unlike
 * qvc_infer_batch it is NOT hipGraph-capturable and must not be used in the timed region.
 */
typedef struct qvc_launch_record {
  char name[48];        /* e.g. "conv<f16,MF4,NF2,WM4,std>", "rbpair<bf16x,MF2,NF10,WM4>", "post_tail<f16>", "cond_gemv" */
  float ms;             /* device time of this launch (HIP events on the stream)                */
  double flops;         /* algorithmic FLOPs (2*MAC) of the launch, 0 for byte movers           */
  double bytes;         /* algorithmic bytes: activations in + out + weights, each counted once */
} qvc_launch_record;

int qvc_infer_batch_timed(const qvc_config* cfg, const void* blob_dev,
                          const float* unit, const float* g, const float* noise, float* out,
                          int32_t batch, int32_t frames,
                          void* workspace, int64_t workspace_bytes, void* stream,
                          qvc_launch_record* records, int32_t max_records, int32_t* n_records);

/* ---- stages (same workspace; for stage-level parity tests and profiling) ------
 * Frame-major fp32 tensors: z_p / z are [B][T][inter_channels].
 */
/* CondNormalWN.forward (enc_p), models.py:75-95: unit, noise -> z_p. */
int qvc_enc_p(const qvc_config* cfg, const void* blob_dev, const float* unit, const float* noise,
              float* z_p_fm, int32_t batch, int32_t frames,
              void* workspace, int64_t workspace_bytes, void* stream);
/* WN.forward, modules.py:69-114: one of the path's WaveNet stacks on its own.
 *   which = 0: enc_p.enc (enc_layers layers, g = NULL: no conditioning, modules.py:98)
 *   which = 1 + i: flow.flows[2*i].enc (flow_layers layers, conditioned on g through cond_layer, modules.py:83-96)
 *   x_fm [B][T][hidden] fp32 (the stack's input, i.e. the output of the `pre` 1x1)  ->  out_fm [B][T][hidden] fp32
 *   (the sum of the skip paths = WN's return value).  x_fm and out_fm must not overlap. */
int qvc_wn_stack(const qvc_config* cfg, const void* blob_dev, int32_t which, const float* x_fm, const float* g,
                 float* out_fm, int32_t batch, int32_t frames,
                 void* workspace, int64_t workspace_bytes, void* stream);
/* ResidualCouplingBlock.forward(reverse=True), models.py:39-51: in place on z. */
int qvc_flow_reverse(const qvc_config* cfg, const void* blob_dev, float* z_fm, const float* g,
                     int32_t batch, int32_t frames,
                     void* workspace, int64_t workspace_bytes, void* stream);
/* Generator trunk, models.py:372-390: z -> subband_conv_post output [B][F][subbands*2*(n_fft/2+1)],
 * F = frames*prod(ups)+1 (the ReflectionPad1d((1,0)) adds one frame). */
int qvc_dec_trunk(const qvc_config* cfg, const void* blob_dev, const float* z_fm, const float* g,
                  float* post_fm, int32_t batch, int32_t frames,
                  void* workspace, int64_t workspace_bytes, void* stream);
/* exp / pi*sin / per-band iSTFT / zero-stuff / synthesis FIR, models.py:394-406 and
 * pqmf.py:106-117: post_fm [B][F][...] -> out (B, subbands*hop*(F-1)); y_mb (optional,
 * may be NULL) receives the sub-band signals (B, subbands, hop*(F-1)). */
int qvc_istft_synth(const qvc_config* cfg, const void* blob_dev, const float* post_fm,
                    float* out, float* y_mb, int32_t batch, int32_t post_frames, void* stream);

/* ---- one conv through the MFMA kernel (unit tests of the kernel itself) ---------
 * y[b,co,t] = bias[co] + sum_{ci,j} w[co,ci,j] * lrelu(x[b,ci,t+(j-(k-1)/2)*dil], slope_in)
 * x, y are (B,C,T) fp32; w is (Cout,Cin,k) fp32 on the HOST (packed internally into
 * w_scratch_host, then copied to w_scratch_dev on the stream).  Replaces
 * torch.nn.functional.conv1d as used at modules.py:91,104,150-153.
 */
int64_t qvc_conv1d_scratch_bytes(int32_t cout, int32_t cin, int32_t k);
int64_t qvc_conv1d_workspace_bytes(int32_t batch, int32_t cout, int32_t cin, int32_t frames);
int qvc_conv1d(const float* x, const float* w_host, const float* bias_host, float* y,
               int32_t batch, int32_t cin, int32_t cout, int32_t frames,
               int32_t k, int32_t dilation, float slope_in, int32_t operand_dtype,
               void* w_scratch_host, void* w_scratch_dev, int64_t scratch_bytes,
               void* workspace, int64_t workspace_bytes, void* stream);

/* ---- speaker encoder: replaces SpeakerEncoder.embed_utterance (models.py:507-546) -------
 * The step of SynthesizerTrn.infer in front of the path (models.py:635):
 * 3-layer LSTM n_mel -> gin over 128-frame partials at hop 64 (plus the last 128 frames),
 * Linear + ReLU + L2 normalisation per partial, mean over the partials (not re-normalised).
 * All partials of all utterances run in one persistent-recurrence launch per layer.
 *   mel (U, n_mel, mel_frames) fp32 -- the layout convert.py:77 hands to infer()
 *   g   (U, gin_channels)     fp32
 * Own blob (state-dict keys enc_spk.lstm.{weight,bias}_{ih,hh}_l{0,1,2}, enc_spk.linear.*),
 * so a host may pack it only when it embeds speakers.  Needs gin_channels % 8 == 0 and
 * gin_channels <= 256 (QVC_ERR_BAD_CONFIG otherwise).
 */
int64_t qvc_spk_blob_bytes(const qvc_config* cfg);
int qvc_spk_pack_weights(const qvc_config* cfg, const qvc_tensor* tensors, int32_t n_tensors,
                         void* blob_host, int64_t blob_bytes);
int64_t qvc_spk_workspace_bytes(const qvc_config* cfg, int32_t utterances, int32_t mel_frames);
int qvc_speaker_embed(const qvc_config* cfg, const void* spk_blob_dev, const float* mel, float* g,
                      int32_t utterances, int32_t mel_frames,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* The same for a RAGGED batch -- target recordings never have one length:
 *   mel (U, n_mel, max_frames) fp32 padded, frames_dev[U] int32 ON THE DEVICE: valid frames per row
 *   (clamped to [0, max_frames] on the device; the padding is never read, it may hold anything).
 * Row u of g is bit-identical to qvc_speaker_embed on that row alone (utterances = 1, mel_frames =
 * frames_dev[u]); a row of 0 frames gives a zero row.  One small launch builds a partial map on the
 * device ({row, first frame, steps} per partial, exclusive scan of the rows' partial counts); the
 * launches after it are sized from the cap utterances * partials(max_frames), and recurrence columns
 * whose own steps are over keep their state -- no length is read on the host, so the call can be
 * captured in a graph and replayed with other lengths.  Workspace: qvc_spk_ragged_workspace_bytes. */
int64_t qvc_spk_ragged_workspace_bytes(const qvc_config* cfg, int32_t utterances, int32_t max_frames);
int qvc_speaker_embed_ragged(const qvc_config* cfg, const void* spk_blob_dev, const float* mel,
                             const int32_t* frames_dev, float* g, int32_t utterances, int32_t max_frames,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---- mel front-end: replaces mel_processing.wave_to_mel (mel_processing.py:15-98) ---------
 * The step in front of the speaker encoder on the target side (convert.py:75-77):
 * reflect pad (n_fft-hop)/2, Hann STFT (center=False, win = n_fft), sqrt(re^2+im^2+1e-6),
 * mel-basis matmul, log(clamp(., 1e-5)).  All fp32: the STFT is a GEMM against a windowed DFT table
 * on the f32 MFMA (bitwise an fmaf chain), so it needs no FFT plan and no complex temporaries.
 *   wave (U, samples) fp32 in [-1, 1]   ->   mel (U, n_mels, frames) fp32,
 *   frames = (samples + 2*((n_fft-hop)/2) - n_fft) / hop + 1.
 * The mel filter bank itself is the caller's (n_mels x (n_fft/2+1), librosa.filters.mel in the
 * reference): qvc_mel_pack_tables turns it and the windowed DFT matrix into the device table.
 * Needs n_fft % 16 == 0, hop % 4 == 0, n_fft >= hop, samples > (n_fft-hop)/2.
 */
int64_t qvc_mel_table_bytes(int32_t n_fft, int32_t n_mels);
int qvc_mel_pack_tables(int32_t n_fft, int32_t hop, int32_t n_mels, const float* mel_basis_host,
                        void* table_host, int64_t table_bytes);
int64_t qvc_mel_workspace_bytes(int32_t n_fft, int32_t hop, int32_t utterances, int32_t samples);
int qvc_wave_to_mel(const void* table_dev, int32_t n_fft, int32_t hop, int32_t n_mels,
                    const float* wave, float* mel, int32_t utterances, int32_t samples,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* The same for a RAGGED batch: wave (U, max_samples) fp32 padded; row u is the samples_dev[u] samples
 * from start_dev[u] on (device int32 arrays, clamped to the row on the device; start_dev may be null
 * = 0), reflect-padded at ITS two ends.  mel (U, n_mels, max_frames) with max_frames = the frame
 * count of max_samples; frames_dev[U] receives each row's own count, frames at or past it are
 * written as 0.0, a row no longer than the reflect pad (n_fft-hop)/2 gets 0 frames.  A valid frame
 * is bit-identical to qvc_wave_to_mel on that row alone. */
int64_t qvc_mel_ragged_workspace_bytes(int32_t n_fft, int32_t hop, int32_t utterances, int32_t max_samples);
int qvc_wave_to_mel_ragged(const void* table_dev, int32_t n_fft, int32_t hop, int32_t n_mels,
                           const float* wave, const int32_t* start_dev, const int32_t* samples_dev,
                           float* mel, int32_t* frames_dev, int32_t utterances, int32_t max_samples,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* ---- silence trim in front of the mel (librosa.effects.trim in the reference, convert.py:65) ----
 * For every row of wave (U, max_samples) with samples_dev[u] samples (clamped on the device): frames
 * of frame_length samples at hop_length over the row zero-padded by frame_length/2 on both sides;
 * a frame is kept when its RMS is less than top_db below the row's loudest frame;
 *   start = first kept * hop_length, end = min(samples, (last kept + 1) * hop_length),
 * written to start_dev[u] / len_dev[u] (= end - start).  A row shorter than frame_length is left
 * whole.  Needs frame_length % (2 * hop_length) == 0 (QVC_ERR_BAD_CONFIG otherwise) and top_db > 0.
 * The outputs feed qvc_wave_to_mel_ragged as they are. */
int64_t qvc_trim_workspace_bytes(int32_t utterances, int32_t max_samples, int32_t frame_length, int32_t hop_length);
int qvc_trim_bounds(const float* wave, const int32_t* samples_dev, int32_t* start_dev, int32_t* len_dev,
                    int32_t utterances, int32_t max_samples, float top_db, int32_t frame_length, int32_t hop_length,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ---- sample formats either side of the float path: wav payloads in, 16-bit PCM out ----------
 * qvc_pcm_to_wave_ragged is frontend.load_wav's int -> float conversion and channel mean for a batch
 * of RAW wav payloads (what qvc_io_load_wavs of qvc_io.h puts into byte slots), in front of
 * qvc_trim_bounds: slot u of pcm (utterances slots of slot_bytes bytes each; pcm 16-byte aligned and
 * slot_bytes a multiple of 16, else QVC_ERR_BAD_ARG) holds interleaved little-endian frames in the
 * format rows_dev[u] names.  rows_dev is a DEVICE array and is never read on the host:
 *   code      1 u8, 2 s16, 3 s24 (packed), 4 s32, 5 f32   (QVC_PCM_* of qvc_io.h)
 *   channels  1 or 2
 *   frames    frames in the slot
 * Row u of wave (utterances, max_samples) fp32 receives n = clamp(frames, 0, min(max_samples,
 * slot_bytes / (bytes per sample * channels))) samples, samples [n, max_samples) are written as 0.0f
 * and samples_dev[u] = n; a row with another code or channel count gets n = 0.  Arithmetic, bit for
 * bit load_wav's: s16 (float)v / 32768, s24 (float)v / 8388608, s32 (float)v / 2147483648 (the
 * conversion rounds to nearest even), u8 ((float)v - 128) / 128, f32 the bits as they are; two
 * channels: (a + b) * 0.5f of the converted values.  One streaming launch sized by max_samples: the
 * payload is read once, the floats are written once, no workspace.  utterances <= 65535.
 *
 * qvc_wave_to_pcm16 is the 16-bit writer's conversion, element-wise over n floats:
 *   q = clamp(rint(x * 32768), -32768, 32767), halves to even, NaN -> 0
 * (numpy: np.clip(np.rint(x * np.float32(32768)), -32768, 32767).astype(np.int16)).  The scale is a
 * power of two, so nothing rounds twice, and it inverts the s16 reader above: a signal that came from
 * a 16-bit file survives write -> read unchanged. */
typedef struct { int32_t code, channels, frames; } qvc_pcm_row;
int qvc_pcm_to_wave_ragged(const void* pcm, int64_t slot_bytes, const qvc_pcm_row* rows_dev,
                           float* wave, int32_t* samples_dev, int32_t utterances, int32_t max_samples, void* stream);
int qvc_wave_to_pcm16(const float* wave, int16_t* pcm, int64_t n, void* stream);

/* ---- posterior direction: enc_q and the forward flow (models.py:617-618) -------
 * z ~ enc_q(spec | g) = CondNormalWN with speaker conditioning (models.py:75-95,582), then
 * z_p = flow(z, g) = ResidualCouplingBlock.forward(reverse=False) (models.py:39-51; x1 <- m + x1,
 * modules.py:217).  Not used by convert.py; it is the analysis half of the model (reconstruction /
 * evaluation) and runs on the same WaveNet kernels.  enc_q has its own blob (state-dict keys enc_q.*);
 * the forward flow reuses the path's blob: every coupling layer sees the same channel flip in both
 * directions, so the flip-folded pre / post weights serve both.
 *   spec  (B, spec_channels, T) fp32   linear spectrogram        (mel_processing.py:15-58)
 *   g     (B, gin_channels)     fp32
 *   noise (B, inter_channels, T) fp32  the N(0,1) draw of models.py:94
 *   z_fm / z: frame-major [B][T][inter_channels] fp32 (as the stage entry points above)
 * Both use the workspace of qvc_workspace_bytes(cfg, batch, frames).
 */
int64_t qvc_encq_blob_bytes(const qvc_config* cfg);
int qvc_encq_pack_weights(const qvc_config* cfg, const qvc_tensor* tensors, int32_t n_tensors,
                          void* blob_host, int64_t blob_bytes);
int qvc_enc_q(const qvc_config* cfg, const void* encq_blob_dev, const float* spec, const float* g,
              const float* noise, float* z_fm, int32_t batch, int32_t frames,
              void* workspace, int64_t workspace_bytes, void* stream);
int qvc_flow_forward(const qvc_config* cfg, const void* blob_dev, float* z_fm, const float* g,
                     int32_t batch, int32_t frames,
                     void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QVC_H */
