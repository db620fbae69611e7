/* rvcx.h -- C ABI of librvcx.so: the MI355X-native RVC v2 inference hot path.
 *
 * The reference (Bebra777228/PolGen-RVC) is pure Python; it has no FFI of its own.  Each
 * entry point below names the reference interface (file:line under /root/reference) whose
 * work it replaces; the Python mirror in polgen-rvc_amd/infer/{infer,pipeline}.py binds
 * them with ctypes behind the reference's own call signatures.
 *
 * Conventions: return 0 on success, negative on error (message via rvcx_last_error);
 * nothing throws across the ABI.  One context per GPU.  Every entry point takes the
 * context's own (recursive) mutex: threads that share a context QUEUE -- the reference
 * builds fresh model objects per request (rvc/scripts/voice_conversion.py:71-100), so
 * its concurrent requests are safe, and they stay safe here -- while different contexts
 * are fully concurrent.  Throughput comes from one rvcx_convert_batch call over many
 * utterances, not from threads.  rvcx_destroy must not race with any other call.  "hd" pointers may
 * be host or device memory (copied with hipMemcpyDefault); everything else is host.
 * All tensors are dense row-major float32 unless stated.
 */
#ifndef RVCX_H
#define RVCX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rvcx_ctx rvcx_ctx;

/* one checkpoint tensor, borrowed for the duration of the load call only */
typedef struct {
  const char* name;
  const void* data;
  int32_t dtype; /* 0 = float32, 1 = float16, 2 = int64 */
  int32_t ndim;
  int64_t shape[4];
} rvcx_tensor;

/* Synthesizer(*cpt["config"]) hyper-parameters -- rvc/infer/infer.py:86-97,
 * rvc/lib/algorithm/synthesizers.py:14-36 */
typedef struct {
  int32_t inter_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size;
  int32_t n_resblocks;          /* len(resblock_kernel_sizes) (<= 4) */
  int32_t res_kernels[4];
  int32_t res_dilations[4][3];
  int32_t n_ups;                /* len(upsample_rates) (<= 6) */
  int32_t up_rates[6], up_kernels[6];
  int32_t up_initial_channel, spk_embed_dim, gin_channels, sr, input_dim;
} rvcx_synth_cfg;

/* E2E(n_blocks, n_gru, kernel_size=(2,2), en_de_layers, inter_layers, in_channels,
 * en_out_channels) -- rvc/lib/predictors/RMVPE.py:340-352,452 */
typedef struct {
  int32_t n_blocks, en_de_layers, inter_layers, en_out_channels;
} rvcx_rmvpe_cfg;

/* FCPE(input_channel, out_dims, n_layers, n_chans) -- rvc/lib/predictors/FCPE.py:551-627, built from fcpe.pt's
 * "config" block at FCPE.py:715-733; heads / dim_head / nb_features / dw_kernel are the module defaults
 * (FCPE.py:445-446, 435, 315), read off the tensor shapes; mel_fmin / mel_fmax from config["mel"] */
typedef struct {
  int32_t n_layers, n_chans, input_channel, out_dims;
  int32_t heads, dim_head, nb_features, dw_kernel;
  float mel_fmin, mel_fmax;
} rvcx_fcpe_cfg;

/* fairseq HubertModel (hubert_base) geometry -- loaded at rvc/infer/infer.py:67-74 */
typedef struct {
  int32_t conv_dim, n_conv;
  int32_t conv_kernels[8], conv_strides[8];
  int32_t embed_dim, ffn_dim, heads, layers, pos_kernel, pos_groups;
} rvcx_hubert_cfg;

/* per-call conversion parameters -- the keyword set of VC.pipeline / rvc_infer
 * (rvc/infer/pipeline.py:289-311, rvc/infer/infer.py:109-128) plus Config's chunk geometry
 * (rvc/infer/infer.py:36-43) */
typedef struct {
  float pitch;            /* semitones */
  float f0_min, f0_max;
  float index_rate;
  float protect;
  float volume_envelope;
  int32_t sid;
  int32_t x_pad, x_query, x_center, x_max; /* seconds */
  uint64_t seed;          /* Philox seed for the two Gaussian draws when noise == NULL */
  int32_t f0_method;      /* RVCX_F0_RMVPE ("rmvpe" / "rmvpe+", pipeline.py:142-167) or RVCX_F0_FCPE ("fcpe", :169-181) */
  int32_t resample_sr;    /* VC.pipeline's resample_sr (pipeline.py:453-454): >= 16000 and != tgt_sr resamples the output
                             before the peak normalisation; 0 (what rvc_infer passes, infer.py:144) = off */
  int32_t hop_length;     /* VC.get_f0's hop_length: frame step of "mangio-crepe" in 16 kHz samples (pipeline.py:151-152);
                             <= 0: 128, the reference's default */
  int32_t reserved;
} rvcx_params;
enum { RVCX_F0_RMVPE = 0, RVCX_F0_FCPE = 1, RVCX_F0_CREPE = 2 /* "mangio-crepe", pipeline.py:86-117, 151-152 */ };

/* per-utterance extras of rvcx_convert_batch_ex */
typedef struct {
  /* VC.pipeline's f0_file (rvc/infer/pipeline.py:349-360): the parsed rows "time [s], f0 [Hz]" as float32 pairs in HOST
   * memory, or NULL.  VC.get_f0 turns them into a 100 Hz track with np.interp and overwrites the estimate from frame
   * x_pad * 100 on (pipeline.py:185-191); the library does exactly that (float32 / float64 steps as numpy takes them). */
  const float* inp_f0;
  int32_t inp_f0_rows;
  int32_t reserved;
  /* "mangio-crepe" only: the +-20 cent triangular dither torchcrepe adds to every decoded frame
   * (convert.bins_to_cents -> dither: scipy.stats.triang.rvs on the GLOBAL numpy RNG), one float32 per frame in HOST
   * memory (rvcx_crepe_frames(n_padded, hop) of them), or NULL: drawn from the call's Philox stream */
  const float* crepe_dither;
  int64_t crepe_dither_n;
} rvcx_utt_extra;

/* ---- lifecycle ------------------------------------------------------------------------ */
int rvcx_create(int device, rvcx_ctx** out);
void rvcx_destroy(rvcx_ctx* ctx);
const char* rvcx_last_error(rvcx_ctx* ctx); /* ctx may be NULL: last error of this thread */
const char* rvcx_version(void);

/* ---- model loading (host tensors in checkpoint layout; folded + packed + uploaded) ---- */
/* replaces load_hubert -- rvc/infer/infer.py:67-74 */
int rvcx_load_hubert(rvcx_ctx*, const rvcx_hubert_cfg*, const rvcx_tensor* tbl, int n);
/* replaces RMVPE0Predictor.__init__ -- rvc/lib/predictors/RMVPE.py:442-459 */
int rvcx_load_rmvpe(rvcx_ctx*, const rvcx_rmvpe_cfg*, const rvcx_tensor* tbl, int n);
/* replaces FCPEF0Predictor.__init__ / FCPEInfer.__init__ -- rvc/lib/predictors/FCPE.py:708-736, 806-826
 * (tbl: the checkpoint's "model" state_dict) */
int rvcx_load_fcpe(rvcx_ctx*, const rvcx_fcpe_cfg*, const rvcx_tensor* tbl, int n);
/* replaces torchcrepe.load.model (called by torchcrepe.predict, rvc/infer/pipeline.py:96): the state dict of
 * torchcrepe's model.Crepe -- conv{1..6}.weight (Cout, Cin, K, 1) / .bias, conv{1..6}_BN.*, classifier.*; the capacity
 * ("full" / "tiny" / ...) is read off the shapes.  torchcrepe is not vendored with the reference: parity unpinned */
int rvcx_load_crepe(rvcx_ctx*, const rvcx_tensor* tbl, int n);
/* replaces get_vc's Synthesizer construction -- rvc/infer/infer.py:78-105 */
int rvcx_load_synth(rvcx_ctx*, const rvcx_synth_cfg*, const rvcx_tensor* tbl, int n, int* model_id);
int rvcx_unload_synth(rvcx_ctx*, int model_id);
/* replaces faiss.read_index + reconstruct_n -- rvc/infer/pipeline.py:322-323.
 * big_npy is the (n, dim) float32 matrix of stored vectors; NULL/0 drops the index. */
int rvcx_load_index(rvcx_ctx*, const float* big_npy, int64_t n, int dim);
/* the same for a faiss "IVF{nlist},Flat" index, which is what RVC training writes: index.search then scans only
 * the inverted list of the query's nearest centroid (nprobe = 1, stored in the file; pipeline.py:242 uses it as
 * read).  centroids (nlist, dim): the coarse quantiser; assign (n): list id of every stored vector (row = id).
 * Lists with fewer than 8 vectors pad with id -1 / infinite distance, exactly as faiss does. */
int rvcx_load_index_ivf(rvcx_ctx*, const float* big_npy, int64_t n, int dim, const float* centroids, int nlist,
                        const int32_t* assign, int nprobe);

/* Folded weights live in per-model regions (freed by rvcx_unload_synth / rvcx_load_index(NULL) / a reload).
 * rvcx_weights_regions lists the device chunks of everything loaded, in a fixed order (HuBERT, RMVPE, voice
 * models by id, index): up to `cap` (pointer, used bytes) pairs are written, the total chunk count is returned.
 * Chunk sizes, offsets and *layout_hash depend on tensor SHAPES only, so ranks that loaded placeholder values
 * (zeros) with the same configurations report the same layout; rank 0's chunks can then be RCCL-broadcast into
 * them (polgen-rvc_amd/dist.py) instead of parsing / folding the checkpoints once per GPU.  New in rvcx -- the
 * reference is single-device.  After the chunks were overwritten, rvcx_weights_adopt re-reads
 * the value-dependent layer flags that travel in each region's header. */
int rvcx_weights_regions(rvcx_ctx*, int cap, void** dev_ptrs, int64_t* nbytes, uint64_t* layout_hash);
int rvcx_weights_adopt(rvcx_ctx*);
/* Same-device counterpart of the broadcast: copy the folded weights of `src` into this context, which must have
 * loaded the same configurations (placeholder values allowed) -- a second or third context per GPU (several
 * conversions in flight) then costs a device copy instead of parsing and folding again. */
int rvcx_weights_clone(rvcx_ctx*, rvcx_ctx* src);

/* ---- stage-level entry points (parity tests bind these) ------------------------------- */
/* RMVPE0Predictor.infer_from_audio_with_pitch -- rvc/lib/predictors/RMVPE.py:487-496.
 * audio (B, n) -> f0 (B, 1 + n/160) Hz; hidden (B, frames, 360) optional. */
int rvcx_rmvpe_f0(rvcx_ctx*, int B, const float* audio_hd, int64_t n, float thred, float f0_min,
                  float f0_max, float* f0_hd, float* hidden_hd);
int rvcx_rmvpe_frames(int64_t n);
/* MelSpectrogram.forward -- rvc/lib/predictors/RMVPE.py:412-439: audio (B, n) -> log-mel (B, 128, 1 + n/160) */
int rvcx_rmvpe_mel(rvcx_ctx*, int B, const float* audio_hd, int64_t n, float* mel_hd);
/* FCPEInfer.__call__(audio, sr=16000, threshold) -- rvc/lib/predictors/FCPE.py:739-745 (return_hz_f0, local_argmax
 * decoder): audio (B, n) -> f0 (B, n/160 + 1) Hz, 0 where the salience maximum is <= threshold.
 * salience (B, frames, 360) = the sigmoid output of FCPE.forward (FCPE.py:646), mel (B, 128, frames) =
 * Wav2Mel.__call__ transposed (FCPE.py:768-788); both optional. */
int rvcx_fcpe_f0(rvcx_ctx*, int B, const float* audio_hd, int64_t n, float threshold, float* f0_hd,
                 float* salience_hd, float* mel_hd);
int rvcx_fcpe_frames(int64_t n);
/* FCPEF0Predictor.compute_f0(x, p_len) as VC.get_f0 calls it (threshold 0.03, pipeline.py:169-179; FCPE.py:869-877)
 * followed by get_f0's own tail (pitch shift, coarse; pipeline.py:183-201): x (n samples) -> p_len frames. */
int rvcx_get_f0_fcpe_x(rvcx_ctx*, const float* x_hd, int64_t n, int64_t p_len, const rvcx_params* p, int32_t* coarse,
                       float* f0);
/* HubertModel.extract_features(source, padding_mask=False, output_layer=L)[0] --
 * call site rvc/infer/pipeline.py:228-236.  wav (B, n) -> feats (B, T', embed_dim). */
int rvcx_hubert_features(rvcx_ctx*, int B, const float* wav_hd, int64_t n, int output_layer,
                         float* feats_hd);
int rvcx_hubert_frames(rvcx_ctx*, int64_t n);
/* Synthesizer.infer -- rvc/lib/algorithm/synthesizers.py:163-188.
 * phone (B,T,input_dim), pitch (B,T) int32 coarse, pitchf (B,T) Hz, lens (B) valid frames,
 * sid (B).  z_noise (B,inter,T) / src_noise (B,T*upp) replace the two randn_like draws when
 * non-NULL (parity mode), otherwise Philox(seed).  out (B, T*upp). */
int rvcx_synth_infer(rvcx_ctx*, int model_id, int B, int T, const int32_t* lens,
                     const float* phone_hd, const int32_t* pitch_hd, const float* pitchf_hd,
                     const int32_t* sid, const float* z_noise_hd, const float* src_noise_hd,
                     uint64_t seed, float* out_hd);
/* the same with the NSF decoder evaluated on frames [dec_skip, len - dec_skip) of every item only (TextEncoder, flow and the
 * harmonic source stay whole); out samples outside that window read 0.  What VC.pipeline does with the result --
 * audio1[t_pad_tgt:-t_pad_tgt], rvc/infer/pipeline.py:432-447 -- makes the discarded ends dead work: with
 * dec_skip <= t_pad frames - rvcx_synth_dec_rf(model) the kept samples are those of the full evaluation (the decoder is
 * convolutional, nsf.py:100-144; rvcx_synth_dec_rf = its receptive field in frames, each side, + 2).  rvcx_convert_batch
 * uses this internally (RVCX_DEC_WINDOW=0 turns it off); no reference counterpart. */
int rvcx_synth_infer_window(rvcx_ctx*, int model_id, int B, int T, const int32_t* lens,
                            const float* phone_hd, const int32_t* pitch_hd, const float* pitchf_hd,
                            const int32_t* sid, const float* z_noise_hd, const float* src_noise_hd,
                            uint64_t seed, int dec_skip, float* out_hd);
int rvcx_synth_dec_rf(rvcx_ctx*, int model_id);
/* the same with the intermediates the reference returns beside the waveform (synthesizers.py:186-188):
 * stats (B, 2*inter, T) = [m_p ; logs_p] of the TextEncoder, zflow (B, inter, T) = z after the reverse flow */
int rvcx_synth_infer_taps(rvcx_ctx*, int model_id, int B, int T, const int32_t* lens,
                          const float* phone_hd, const int32_t* pitch_hd, const float* pitchf_hd,
                          const int32_t* sid, const float* z_noise_hd, const float* src_noise_hd,
                          uint64_t seed, float* out_hd, float* stats_hd, float* zflow_hd);
/* Synthesizer.infer(..., rate) -- synthesizers.py:170-181 -- with the head given in FRAMES: the TextEncoder and the z_p draw
 * run over all T frames, then z_p, the mask and nsff0 are sliced to [skip_head:] and the four coupling layers, the harmonic
 * source (whose phase accumulation starts at the slice) and the whole decoder run at T - skip_head frames.  This is not the
 * decoder window above: the flow and the source see the slice, not the whole, and the result differs from the tail of a
 * full evaluation.  The reference computes head = int(T * (1.0 - rate)) with rate a float32 tensor (the Python mirror's
 * head_from_rate restates it).  z_noise (B, inter, T); src_noise and out (B, (T - skip_head) * upp); zflow optional
 * (B, inter, T - skip_head).  Errors: skip_head outside [0, T); lens that are not all T together with skip_head > 0.
 * skip_head = 0 takes the launches of the plain call and returns its bits. */
int rvcx_synth_infer_head(rvcx_ctx*, int model_id, int B, int T, const int32_t* lens, const float* phone_hd,
                          const int32_t* pitch_hd, const float* pitchf_hd, const int32_t* sid,
                          const float* z_noise_hd, const float* src_noise_hd, uint64_t seed, int skip_head,
                          float* out_hd, float* zflow_hd);
int rvcx_synth_upp(rvcx_ctx*, int model_id);
/* index.search(k=8) + weighted blend -- rvc/infer/pipeline.py:239-250.
 * feats (T, dim) in/out; ids (T,8) int64 and dist (T,8) optional. */
int rvcx_index_blend(rvcx_ctx*, float* feats_hd, int T, float index_rate, int64_t* ids_hd,
                     float* dist_hd);

/* ---- whole path ------------------------------------------------------------------------ */
/* capacity (in samples) the caller must provide per output buffer for an n-sample 16 kHz input;
 * the exact count VC.pipeline produces depends on the silence-aligned cut points (and is exactly
 * (n/160)*upp - 2*upp... for single-chunk clips); rvcx_convert_batch reports it in out_n */
int64_t rvcx_out_len(rvcx_ctx*, int model_id, int64_t n, const rvcx_params* p);
/* VC.pipeline for a batch of utterances -- rvc/infer/pipeline.py:289-467 with
 * f0_method = p->f0_method ("rmvpe+" or "fcpe"; that model must be loaded), pitch_guidance=1, resample_sr=0,
 * f0_file=None.
 * wav16k[i] (n[i] samples, 16 kHz mono f32, host or device); out[i] caller-allocated int16
 * buffers of rvcx_out_len samples (host or device); out_f32[i] optional (same capacity) float
 * waveform before int16 quantisation; out_n[i] receives the number of samples produced; noise[i] optional
 * packed parity noise (see rvcx_noise_len).
 * Utterances of one length class (rvcx_bucket_length: padded lengths within RVCX_BUCKET_FRAMES 10 ms frames, default
 * 128; clips long enough to be cut into chunks: equal lengths) are converted together as ragged micro-batches (B > 1
 * through HuBERT, RMVPE, TextEncoder and flow with per-item lengths; rvcx_micro_batch tells how many at a time;
 * rvcx_last_micro_batches what the last call did); every utterance's result is bit-identical to converting it alone.  Without parity noise utterance i draws its Gaussians from Philox(seed + i).
 * Batch conversion is listed as not done in the reference (TODO.md:11). */
int rvcx_convert_batch(rvcx_ctx*, int model_id, int B, const float* const* wav16k_hd,
                       const int64_t* n, const rvcx_params* p, const float* const* noise_hd,
                       int16_t* const* out_hd, float* const* out_f32_hd, int64_t* out_n);
/* the same with float64 input, the dtype rvc_infer hands to VC.pipeline (load_audio -> float64,
 * rvc/lib/my_utils.py:5-16): the float64 zero-phase high-pass (pipeline.py:329) then sees the reference's input */
int rvcx_convert_batch_f64(rvcx_ctx*, int model_id, int B, const double* const* wav16k_hd,
                           const int64_t* n, const rvcx_params* p, const float* const* noise_hd,
                           int16_t* const* out_hd, float* const* out_f32_hd, int64_t* out_n);
/* the same with per-utterance extras (`extra`: B entries or NULL); wav16k_hd[i] is float64 when wav_is_f64 != 0 */
int rvcx_convert_batch_ex(rvcx_ctx*, int model_id, int B, const void* const* wav16k_hd, int wav_is_f64,
                          const int64_t* n, const rvcx_params* p, const float* const* noise_hd,
                          const rvcx_utt_extra* extra, int16_t* const* out_hd, float* const* out_f32_hd, int64_t* out_n);

/* ---- conversion tickets: two requests in flight per context ----------------------------------------------------------
 * rvcx_convert_submit takes the arguments of rvcx_convert_batch_ex, enqueues the conversion on the calling thread and
 * returns a ticket without waiting for the device; rvcx_convert_wait blocks until the ticket's outputs and out_n are
 * final.  What a ticket writes is byte for byte what rvcx_convert_batch_ex writes for the same arguments (utterance i of a
 * ticket draws from Philox(seed + i)).  While one ticket is in its synthesizer on the main stream, the front end (upload,
 * high-pass, F0 model, HuBERT) of the next one runs on the front / HuBERT streams, as consecutive micro-batches of one
 * call do; tickets of different voice models or parameters take the same path.
 *
 * Borrowing.  submit copies n, *p, the pointer tables, `extra` and the f0-file rows it points to.  The audio, noise,
 * crepe-dither and output buffers (and out_n) are BORROWED until rvcx_convert_wait has returned for the ticket: they must
 * stay valid and untouched until then.  Outputs in plain host memory are written during the wait (or whenever the ticket
 * is completed internally, see below), outputs in device or pinned memory by the device.
 *
 * Two in flight.  At most two tickets are in flight per context.  A third submit first completes the oldest one (that
 * ticket stays waitable, its results are in the caller's buffers) and then proceeds.
 *
 * Order and threads.  Tickets may be waited for in any order and from any thread; completions are processed in submit
 * order (waiting for the younger ticket settles the older one first).  wait does not hold the context's mutex while it
 * blocks on the device.  Waiting twice for a ticket, or for a ticket of another context, returns -1 with a message.
 *
 * Other entry points.  Every other entry point of the context (synchronous conversions, F0 / HuBERT calls, loading or
 * unloading a model or index, rvcx_destroy) first completes the tickets in flight; so does a submit that needs more of
 * the memory consecutive tickets share than the context holds.  Completed tickets stay waitable.  The exception is
 * rvcx_resample_f64 / rvcx_resample_f64_kind (what a caller decodes the NEXT request with): it runs beside the tickets
 * in flight, in memory of its own.
 *
 * Range guard, BiGRU fallback.  The observable outcome equals that of the same requests issued as synchronous calls in
 * submit order (rvcx_fp32_pinned and rvcx_gru_fallbacks included): each ticket has its own device error word; a ticket
 * that met an activation beyond fp16 range is repeated as a synchronous call, and so is every ticket enqueued behind it
 * before the layer was pinned; a BiGRU cluster time-out repeats that ticket alone.
 *
 * After rvcx_convert_wait(t), rvcx_last_micro_batches, rvcx_last_cuts and rvcx_last_timing describe ticket t. */
typedef int64_t rvcx_ticket; /* > 0; never reused within a context */
int rvcx_convert_submit(rvcx_ctx*, int model_id, int B, const void* const* wav16k_hd, int wav_is_f64,
                        const int64_t* n, const rvcx_params* p, const float* const* noise_hd,
                        const rvcx_utt_extra* extra, int16_t* const* out_hd, float* const* out_f32_hd,
                        int64_t* out_n, rvcx_ticket* ticket);
int rvcx_convert_wait(rvcx_ctx*, rvcx_ticket); /* blocks; 0 = the outputs and out_n are final */
int rvcx_convert_poll(rvcx_ctx*, rvcx_ticket); /* 1 done (wait will not block on the device), 0 in flight, < 0 error */
int rvcx_convert_inflight(rvcx_ctx*);          /* tickets submitted and not yet completed on the device */
/* Valid after the wait: device time (HIP events) from the first front-end work of the ticket to the completion of the
 * ticket submitted before it.  Positive: its front end started that many ms before its predecessor finished; 0 for a
 * ticket submitted into an idle context.  The context remembers the figure of the last 256 tickets waited for; for
 * any other ticket (older, never waited for, unknown, of another context) the result is NaN. */
float rvcx_ticket_lead_ms(rvcx_ctx*, rvcx_ticket);

/* utterances of n samples converted per launch sequence (memory-bounded; RVCX_MAX_BATCH, RVCX_ARENA_GB) */
int rvcx_micro_batch(rvcx_ctx*, int model_id, int64_t n, const rvcx_params* p);
/* The sample count whose launch geometry an n-sample utterance is converted with (>= n): utterances with equal values
 * share micro-batches.  An uncut rmvpe / mangio-crepe clip: the longest clip of its length class; otherwise n itself. */
int64_t rvcx_bucket_length(rvcx_ctx*, int model_id, int64_t n, const rvcx_params* p);
/* Member counts of the micro-batches the last rvcx_convert_batch* call of this context formed (in launch order);
 * returns their number (counts receives at most cap of them). */
int rvcx_last_micro_batches(rvcx_ctx*, int32_t* counts, int cap);
/* The cut points (the reference's opt_ts, pipeline.py:329-344: sample indices of the filtered clip) the last
 * rvcx_convert_batch* call of this context cut each utterance at, in the caller's order: for every utterance its count,
 * then that many points (an uncut clip: 0 and nothing).  Returns the number of values of the whole list (out receives at
 * most cap of them), -1 without a context. */
int64_t rvcx_last_cuts(rvcx_ctx*, int64_t* out, int64_t cap);
/* floats of parity noise rvcx_convert_batch consumes for one n-sample utterance: for each
 * chunk in order, z_noise (inter*T) then src_noise (T*upp) -- the draw order of the reference */
int64_t rvcx_noise_len(rvcx_ctx*, int model_id, int64_t n, const rvcx_params* p);
/* VC.get_f0 -- rvc/infer/pipeline.py:132-201 on the reflect-padded, high-passed signal (the F0 model is chosen by
 * p->f0_method): returns coarse (int32) and f0 (Hz) of p_len frames for one utterance */
int rvcx_get_f0(rvcx_ctx*, const float* wav16k_hd, int64_t n, const rvcx_params* p,
                int32_t* coarse, float* f0, int64_t* p_len);
/* VC.get_f0(input_audio_path, x, p_len, pitch, "rmvpe+", ...) -- rvc/infer/pipeline.py:132-201 with the
 * reference's meaning of x: the ALREADY reflect-padded, high-passed signal (n samples).  Writes 1 + n/160 frames
 * of coarse (1..255) and f0 (Hz, shifted by p->pitch semitones), un-truncated like the reference's return. */
int rvcx_get_f0_x(rvcx_ctx*, const float* x_hd, int64_t n, const rvcx_params* p, int32_t* coarse, float* f0);
/* VC.get_f0 with everything the reference's does (pipeline.py:132-201): the F0 model p->f0_method names on the padded
 * signal x, pitch shift, the optional f0-file table inp_f0 (rows of (time, f0) float32 pairs in host memory, see
 * rvcx_utt_extra), coarse quantisation.  rmvpe+ returns 1 + n/160 frames, fcpe p_len frames (*frames). */
int rvcx_get_f0_x_ex(rvcx_ctx*, const float* x_hd, int64_t n, int64_t p_len, const rvcx_params* p, const float* inp_f0,
                     int inp_f0_rows, int32_t* coarse, float* f0, int64_t* frames);
/* frames torchcrepe.predict(..., pad=True) returns for n samples at frame step hop: 1 + n / hop */
int64_t rvcx_crepe_frames(int64_t n, int hop);
/* VC.get_f0_crepe up to the resize (rvc/infer/pipeline.py:90-106): x / quantile(|x|, 0.999), then
 * torchcrepe.predict(x, 16000, hop, fmin, fmax, model, batch_size = 2 * hop, pad = True) with its default Viterbi decoder.
 * dither: rvcx_crepe_frames(n, hop) floats (see rvcx_utt_extra) or NULL (Philox, `seed`).  Writes the pitch track (Hz) and,
 * when non-NULL, the network's sigmoid outputs (360, frames) and the decoded bins. */
int rvcx_crepe_predict(rvcx_ctx*, const float* x_hd, int64_t n, int hop, float fmin, float fmax, const float* dither_hd,
                       uint64_t seed, float* pitch_hd, float* probs_hd, int32_t* bins_hd);
/* op level: core.postprocess + decode.viterbi + convert.bins_to_frequency on given sigmoid outputs (360, F), one Viterbi
 * pass per `batch` frames */
int rvcx_op_crepe_decode(rvcx_ctx*, const float* probs_hd, int64_t F, int batch, float fmin, float fmax,
                         const float* dither_hd, float* pitch_hd, int32_t* bins_hd);
/* VC.get_f0(..., f0_method="mangio-crepe", hop_length = p->hop_length) on the padded signal x: get_f0_crepe incl. the
 * resize to p_len frames, pitch shift, f0-file table, coarse quantisation (pipeline.py:86-117, 151-152, 183-201) */
int rvcx_get_f0_crepe_x(rvcx_ctx*, const float* x_hd, int64_t n, int64_t p_len, const rvcx_params* p, const float* inp_f0,
                        int inp_f0_rows, const float* dither_hd, int64_t dither_n, int32_t* coarse, float* f0);
/* host only (no GPU needed): the 100 Hz track VC.get_f0 builds from an f0 file's rows (pipeline.py:186-189: delta_t in
 * float32, np.interp in float64).  Writes min(count, cap) values, returns count. */
int rvcx_f0_file_track(const float* inp_f0, int rows, double* track, int cap);
/* librosa.resample(librosa.to_mono(audio.T), orig_sr=sr_in, target_sr=sr_out) of load_audio (rvc/lib/my_utils.py:9-13):
 * x = (frames, channels) interleaved float64 (host or device), y = rvcx_resample_len(frames, ...) mono float64 samples.
 * Band-limited sinc interpolation (csrc/audio.hip).  librosa's default res_type is "soxr_hq": libsoxr is not vendored and
 * its coefficients are unpublished, its design targets are (pass-band flat to 0.9136 x Nyquist, -120.4 dB from 1.0 x
 * Nyquist, linear phase).  kind 0 (the default; -1 = default / RVCX_RESAMPLER): "kaiser_hq", a Kaiser-windowed sinc
 * designed to those targets (measured +-0.001 dB / -127 dB); kind 1: resampy's published "kaiser_best" (librosa's default
 * before 0.10) in its published arithmetic. */
int64_t rvcx_resample_len(int64_t n, int sr_in, int sr_out);
int rvcx_resample_f64(rvcx_ctx*, const double* x_hd, int64_t frames, int channels, int sr_in, int sr_out, double* y_hd);
int rvcx_resample_f64_kind(rvcx_ctx*, const double* x_hd, int64_t frames, int channels, int sr_in, int sr_out, int kind,
                           double* y_hd);
/* VC.vc(model, net_g, sid, audio0, pitch, pitchf, index, big_npy, index_rate, version="v2", protect) --
 * rvc/infer/pipeline.py:203-287: HuBERT -> (retrieval blend with the resident index when index_rate != 0) ->
 * x2 upsample / protect mix -> Synthesizer.infer.  audio0 (n samples of audio_pad); pitch / pitchf (n_pitch
 * frames, n_pitch >= rvcx_vc_frames(n)); out receives rvcx_vc_frames(n) * upp float32 samples (*out_n), the
 * un-trimmed audio1 of the reference.  z_noise / src_noise as in rvcx_synth_infer. */
int rvcx_vc(rvcx_ctx*, int model_id, const float* audio0_hd, int64_t n, const int32_t* pitch_hd,
            const float* pitchf_hd, int n_pitch, int sid, float index_rate, float protect,
            const float* z_noise_hd, const float* src_noise_hd, uint64_t seed, float* out_hd, int64_t* out_n);
int rvcx_vc_frames(rvcx_ctx*, int64_t n);

/* ---- live streams ---------------------------------------------------------------------------------------------------
 * A session is S lock-step streams of one geometry on one voice model: every step takes one block of 16 kHz mono float32
 * per stream and returns the converted block at the model's rate before the next one arrives.  All lengths are 10 ms frames:
 * block Fb, context Fc, cross-fade Fx, search Fs.  Per stream the session owns (device memory of its own, not arena scratch)
 * a ring of N = Fc + Fx + Fs + Fb frames (zeros at open), the SOLA carry (Fx * upp samples, zeros) and a step counter.
 *
 * One step: (1) every ring moves left by one block and the new block is appended; (2) the F0 model p->f0_method names
 * ("rmvpe" / "rmvpe+" or "fcpe") runs on the whole ring with B = S, then the pitch shift and coarse quantisation of VC.get_f0
 * (pipeline.py:183-201) per stream with that stream's `pitch`; (3) what VC.vc does (pipeline.py:203-287) with B = S: HuBERT
 * (v1 / v2 by the model's input_dim), the retrieval blend when an index is resident and p->index_rate != 0, x2 upsample and
 * protect mix, T = min(N, 2 * HuBERT frames); (4) the synthesizer with skip_head = T - (Fb + Fx + Fs) and per-stream sid: only
 * the tail is synthesized; (5) SOLA per stream on the device (below), then the block is copied out.  The chosen offset never
 * travels to the host inside a step unless `offsets` asks for it.
 *
 * p_len clamp: with HuBERT-base 2 * frames = N - 1, so T = N - 1 and the newest frame of the ring has no synthesized
 * counterpart -- one frame (10 ms) of added latency, the clamp of pipeline.py:257-262.
 *
 * Deliberately absent, because they are whole-clip operations of VC.pipeline (pipeline.py:329, 450-461): the 48 Hz zero-phase
 * high-pass, the volume envelope, resample_sr and the peak normalisation.  A session opened with rvcx_stream_open takes 16 kHz
 * mono float32 and returns the model's rate; rvcx_stream_open_io (below) puts a stateful resampler at either edge.
 *
 * Noise.  noise_hd[s] (parity): z_noise (inter * T) then src_noise ((Fb + Fx + Fs) * upp) for this step.  NULL: stream s draws
 * from Philox(p->seed + s) at counter offsets that no two steps share.  A reset zeroes ring, carry and step counter: a reset
 * session replays a fresh one bit for bit.  Every stream's output equals that of the same stream stepped alone in a session
 * of its own, bit for bit.
 *
 * Rules.  Fb, Fx >= 1, Fs >= 0, n_streams >= 1, and Fb + Fx + Fs <= T, else open fails.  "mangio-crepe" is refused at open (its
 * Viterbi pass and host dither have no place in a per-block loop).  Open fails when a resident index's width differs from the
 * model's input_dim, and when the activation budget cannot hold one step at this S (the message names the largest S that
 * fits).  A step completes the tickets in flight first, like every other entry point, and holds the context's mutex.  A step
 * on a session whose voice model was unloaded returns -1 with a message.  rvcx_destroy closes open sessions. */
typedef struct {
  int32_t n_streams, block_frames, context_frames, crossfade_frames, search_frames; /* 10 ms frames */
} rvcx_stream_cfg;
/* sid (S) speaker ids, pitch (S) semitones; of *p the fields f0_method, f0_min, f0_max, index_rate, protect and seed are used */
int rvcx_stream_open(rvcx_ctx*, int model_id, const rvcx_stream_cfg*, const rvcx_params* p, const int32_t* sid,
                     const float* pitch, int* stream_id);
/* block16k_hd: S pointers to Fb * 160 samples; out_hd: S pointers to Fb * upp samples; pre_sola_hd (optional): S pointers to
 * (Fb + Fx + Fs) * upp samples, the synthesized tail before SOLA; offsets (optional, host): the S chosen SOLA offsets.
 * Sessions opened with rvcx_stream_open_io: block16k_hd[s] holds rvcx_stream_in_len x in_channels floats and out_hd[s]
 * rvcx_stream_out_len floats (see "live streams at the sound card's rate" below) */
int rvcx_stream_step(rvcx_ctx*, int stream_id, const float* const* block16k_hd, const float* const* noise_hd,
                     float* const* out_hd, float* const* pre_sola_hd, int32_t* offsets);
int rvcx_stream_reset(rvcx_ctx*, int stream_id);
int rvcx_stream_close(rvcx_ctx*, int stream_id);
int64_t rvcx_stream_out_len(rvcx_ctx*, int stream_id);   /* Fb * out_rate / 100 when the output is resampled, Fb * upp otherwise */
int64_t rvcx_stream_noise_len(rvcx_ctx*, int stream_id); /* inter * T + (Fb + Fx + Fs) * upp per stream and step */
int rvcx_stream_frames(rvcx_ctx*, int stream_id);        /* T, the frames the TextEncoder sees per step */
/* SOLA (synchronised overlap-add) of one synthesized tail y (Lb + Lx + Ls samples) against the carry b_in (Lx samples):
 *   for d = 0 .. Ls inclusive: nom[d] = sum_{i<Lx} y[d+i] b[i], den[d] = sqrt(sum_{i<Lx} y[d+i]^2 + 1e-8);
 *   d* = the FIRST index of max(nom / den);  out[i] = y[d*+i] (i < Lb), cross-faded with the carry over its first
 *   min(Lx, Lb) samples: out[i] = y[d*+i] fin[i] + b[i] (1 - fin[i]), fin[i] = sin^2(pi/2 i / (Lx - 1));
 *   new carry b_out[i] = y[d* + Lb + i].
 * float32 on the device, one wave per offset, every energy sum formed directly (silence ties exactly, no drift).
 * scores (optional): the Ls + 1 values nom / den.  Pointers may be host or device; b_out may be b_in. */
int rvcx_op_sola(rvcx_ctx*, const float* y_hd, const float* b_in_hd, int Lb, int Lx, int Ls, float* out_hd,
                 float* b_out_hd, int32_t* offset, float* scores_hd);

/* ---- live streams at the sound card's rate ----------------------------------------------------------------------------
 * rvcx_stream_open_io puts a stateful resampler in front of the ring (in_rate, in_channels -> 16 kHz mono) and one behind SOLA
 * (the model's rate sr -> out_rate), both inside the step, on the device.
 *
 * Filter.  Always kaiser_hq (kind 0 of rvcx_resample_f64_kind: 96 zero crossings per wing, taps at exact table positions, left
 * wing then right wing, the running sum in double, one rounding to float32).  RVCX_RESAMPLER does not apply to sessions.  The
 * one-shot kernel and the session's kernel share one tap loop.
 *
 * Delay.  delay(sr_in, sr_out) = 0 for equal rates, else ceil(96 max(1, sr_out / sr_in)) output samples: with it every sample
 * a step emits has all its taps inside the input received so far, so it equals the one-shot result on the complete signal
 * bit for bit.  6.0 ms on the way in (96 samples at 16 kHz), 2.2 - 3.0 ms on the way out (96 samples at 44.1 kHz; 116 at 48 kHz
 * from a 40 k model, 144 from a 32 k model).
 *
 * Input.  x = the mono mix (mean over channels, in double) of everything a stream has received since open or reset, u = the
 * one-shot kaiser_hq resample of x to 16 kHz, u[t] = 0 for t < 0.  Step k = 0, 1, .. appends u[k Fb 160 - d_in + i], i = 0 ..
 * Fb 160 - 1, to the ring, d_in = delay(in_rate, 16000).  Every sample is computed from its global index t (int64, restarting
 * at 0 on reset) at position (double)t * (in_rate / 16000): the result does not depend on how the signal was cut into blocks.
 * Output.  v = the concatenated SOLA blocks at the model's rate, w = its one-shot resample to out_rate; step k returns
 * w[k Fb out_rate / 100 - d_out + i], i = 0 .. Fb out_rate / 100 - 1, d_out = delay(sr, out_rate); negative indices give 0.
 *
 * Rates.  in_rate and out_rate are multiples of 100 Hz within 8000 .. 192000 (a 10 ms frame is a whole number of samples);
 * a rate below 8000 is accepted only beside a partner below 8000 (reduced-size voice models: 4800 Hz -> 6000 Hz).  Anything
 * else -- 22050, 11025, 7900 in front of 16 kHz -- is refused at open.  in_rate 0 or 16000 with one channel, and out_rate 0 or
 * sr, mean "none": that side is rvcx_stream_open's, launch for launch and bit for bit, delay 0.  Equal rates with several
 * channels: the mono mix alone (rounded once to float32), delay 0.  The two sides are independent.
 *
 * State.  Per stream and side a FIFO of past samples at the side's input rate (mono-mixed on the way in; SOLA output on the way
 * out), held in double, of ceil(d sr_in / sr_out) + ceil(96 / min(1, sr_out / sr_in)) + 2 frames of history plus the newest
 * block; the global index is the session's step counter times the block.  FIFOs, the staged blocks and the filter tables are
 * allocations of the session's own; FIFOs exist twice and change places with ring and carry once a step has succeeded.
 * rvcx_stream_reset zeroes them.
 *
 * rvcx_stream_step keeps its signature: block16k_hd[s] holds rvcx_stream_in_len x in_channels floats (interleaved), out_hd[s]
 * rvcx_stream_out_len floats; pre_sola_hd and offsets keep their meaning at the model's rate.  rvcx_last_timing keeps nine
 * slots: the input resampler is counted in the first interval (with F0), the output resampler in the last ("SOLA + copies"). */
typedef struct {
  int32_t in_rate;      /* Hz; 0 or 16000 with in_channels 1: blocks are 16 kHz mono, today's path */
  int32_t in_channels;  /* >= 1, interleaved (frames, channels); averaged like librosa.to_mono */
  int32_t out_rate;     /* Hz; 0 or the voice model's rate: none */
  int32_t reserved;
} rvcx_stream_io;
/* io == NULL: rvcx_stream_open */
int rvcx_stream_open_io(rvcx_ctx*, int model_id, const rvcx_stream_cfg*, const rvcx_stream_io*, const rvcx_params* p,
                        const int32_t* sid, const float* pitch, int* stream_id);
int64_t rvcx_stream_in_len(rvcx_ctx*, int stream_id);   /* frames per block and stream: Fb * in_rate / 100 (x in_channels floats) */
/* in_delay_16k: samples at 16 kHz; out_delay: samples at out_rate; either may be NULL */
int rvcx_stream_delays(rvcx_ctx*, int stream_id, int32_t* in_delay_16k, int32_t* out_delay);
/* host only, no GPU: the definition above; -1 for rates open refuses */
int rvcx_stream_resample_delay(int sr_in, int sr_out);
/* taps of the LAST successful step (zeros before the first): in16k_hd, S pointers to the Fb * 160 samples that entered the
 * rings; native_hd, S pointers to the Fb * upp samples of SOLA output in front of the output resampler -- kept only by sessions
 * whose output is resampled (otherwise out_hd of the step is that block, and asking fails).  Either table may be NULL */
int rvcx_stream_last_taps(rvcx_ctx*, int stream_id, float* const* in16k_hd, float* const* native_hd);
/* live controls, applied from the next step on; pitch / sid: S values or NULL, index_rate / protect: NaN keeps the current
 * value.  Ring, FIFOs, carry and the noise counters are untouched.  sid out of range, or index_rate != 0 with a resident index
 * of the wrong width: -1, nothing changed */
int rvcx_stream_set(rvcx_ctx*, int stream_id, const float* pitch, const int32_t* sid, float index_rate, float protect);
/* the session's resampler without a session: S rows of `frames` input frames (x_hd: S x frames x channels, interleaved), cut
 * into blocks of block_frames 10 ms frames (frames must be a multiple of block_frames * sr_in / 100), through the same FIFO +
 * kernel code a session runs per step; y_hd receives S rows of frames * sr_out / sr_in samples, delayed as defined */
int rvcx_op_stream_resample(rvcx_ctx*, const float* x_hd, int S, int64_t frames, int channels, int sr_in, int sr_out,
                            int block_frames, float* y_hd);

/* ---- post-production -------------------------------------------------------------------------------------------------
 * The reference's second workflow (rvc/scripts/audio_processing.py: convert_to_stereo -> add_effects -> combine_audio) on the
 * device.  add_effects is a pedalboard board and combine_audio is pydub; neither package nor its source is part of the
 * reference tree, so the stages are DEFINED here.  Parity with pedalboard's JUCE classes is unpinned (as for torchcrepe);
 * what is pinned is this arithmetic, against float64 and scipy.signal.lfilter.
 *
 * Signal: float32, B items of C in {1, 2} channels and n[b] frames each, interleaved (frames, channels) at the ABI, planar on
 * the device.  sr: any multiple of 100 Hz in 8000 .. 192000.  Coefficients are formed on the host in double and rounded once to
 * float32.  All state is zero at sample 0.  No parameter smoothing.  Stage order = the board's (audio_processing.py:76-102).  A
 * stage whose parameters make it the identity ("skip") is not launched: its output is its input bit for bit.
 *
 *  1 high-pass, first order, fc = 50 Hz: k = tan(pi fc / sr), b0 = 1 / (k + 1), b1 = -b0, a1 = (k - 1) / (k + 1);
 *    y[n] = b0 x[n] + b1 x[n-1] - a1 y[n-1].
 *  2 compressor (ratio, threshold_db; attack 1 ms, release 100 ms), per channel.  cte(ms) = ms < 1e-3 ? 0 :
 *    exp(-2 pi 1000 / (ms sr)).  Envelope e[n] = |x[n]| + c (e[n-1] - |x[n]|), c = cte(attack) when |x[n]| > e[n-1], else
 *    cte(release).  thr = 10^(dB / 20); g = e < thr ? 1 : pow(e / thr, 1 / ratio - 1); y = x g.  Skip when ratio == 1.
 *  3 noise gate (threshold_db, ratio, attack_ms, release_ms), per channel: two followers in series.  r[n] follows x^2 with
 *    attack 0 ms and release 50 ms and outputs sqrt(r[n]); e[n] is the follower of stage 2 on that output with the caller's
 *    attack and release.  g = e > thr ? 1 : pow(e / thr, ratio - 1).  Skip when ratio == 1.
 *  4 reverb: Freeverb (room_size, damping, wet, dry, width), stereo only, never skipped.  in = 0.015 (L + R);
 *    fb = 0.28 room_size + 0.7; d = 0.4 damping.  Eight parallel combs per side, delays {1116, 1188, 1277, 1356, 1422, 1491,
 *    1557, 1617}, then four all-passes in series, delays {556, 441, 341, 225}; the right side adds 23 to every delay; a delay
 *    of D becomes (int64) sr D / 44100 samples.  Comb: o = buf[i]; last = o (1 - d) + last d; buf[i] = in + last fb; the comb
 *    outputs o are summed in the listed order.  All-pass: v = buf[i]; buf[i] = in + 0.5 v; out = v - in.
 *    w1 = 1.5 wet (1 + width), w2 = 1.5 wet (1 - width); L' = oL w1 + oR w2 + 2 dry L, mirrored for R' (2 dry is ONE
 *    float32 coefficient).
 *  5 low shelf, 6 high shelf (gain_db; fc = 440 Hz, Q = 1 / sqrt 2): the audio-EQ-cookbook shelving biquads with
 *    A = 10^(dB / 40), w = 2 pi fc / sr, beta = sin w sqrt(A) / Q, normalised by a0, transposed direct form II
 *    (y = b0 x + s1; s1 = b1 x - a1 y + s2; s2 = b2 x - a2 y).  Skip at 0 dB.
 *  7 chorus (rate_hz, depth, centre_delay_ms, feedback, mix), per channel -- the project's own definition:
 *    tau(n) = sr / 1000 max(1, centre_ms + 10 depth sin(2 pi rate n / sr)) samples (evaluated in double);
 *    w[n] = the line d at n - tau(n), linear interpolation d[i] + frac (d[i+1] - d[i]), zero in front of sample 0;
 *    d[n] = x[n] + feedback w[n]; y = (1 - mix) x + mix w.  |feedback| < 1.  Skip at mix == 0 (the UI's default).
 *  8 mix (combine_audio, :29-40), pydub's int16 arithmetic: both inputs stereo int16 at the vocal's rate; every sample s
 *    becomes clip(floor(s 10^(gain_db / 20))) (the product in double), then a saturating add.  The result has the vocal's
 *    length: a longer instrumental is cut, a shorter one padded with zeros.
 *
 * How the recurrences run wide (csrc/effects.hip): linear stages as a chunked scan of affine 2 x 2 maps;
 * followers by relaxation over chunks of rvcx_fx_chunk() samples -- every chunk from a guessed state, re-run while its
 * initial state differs from its predecessor's final state, at most as many passes as the longest row has chunks -- which
 * ends in the sequential result bit for bit (every rounding of a step is explicit and the same on host and device); combs,
 * all-passes and the chorus in blocks of their shortest delay.
 *
 * Errors: a rate or channel count out of range, ratio < 1, |feedback| >= 1, a value that is not finite, and reverb on mono
 * return -1 with a message and write nothing.  Entry points with a context hold its mutex and complete the tickets in flight first.
 * Scratch is the activation arena: when B items do not fit its budget (or exceed RVCX_MAX_BATCH, when set), rvcx_fx_chain
 * runs them in groups; an item's result does not depend on the grouping, bit for bit. */
typedef struct {
  /* the eighteen values of add_effects (audio_processing.py:54-75), in its order */
  float reverb_rm_size, reverb_wet, reverb_dry, reverb_damping, reverb_width;
  float low_shelf_gain, high_shelf_gain;
  float compressor_ratio, compressor_threshold;
  float noise_gate_threshold, noise_gate_ratio, noise_gate_attack, noise_gate_release;
  float chorus_rate_hz, chorus_depth, chorus_centre_delay_ms, chorus_feedback, chorus_mix;
  int32_t sample_rate, channels;
} rvcx_fx_params;
/* the whole board on B items: x_hd[b] / y_hd[b] hold n[b] x channels floats (channels must be 2: the reverb is in it).
 * rvcx_last_timing afterwards: {high-pass, compressor, gate, reverb, low shelf, high shelf, chorus, copies + layout, total} */
int rvcx_fx_chain(rvcx_ctx*, int B, const float* const* x_hd, const int64_t* n, const rvcx_fx_params*, float* const* y_hd);
/* one stage on one item, x and y (n, channels) interleaved; the chain's fixed values are arguments here.  env_hd (optional,
 * (n, channels)): the envelope e[n] the gain was computed from. */
int rvcx_op_fx_highpass(rvcx_ctx*, const float* x_hd, int64_t n, int channels, int sr, float fc, float* y_hd);
int rvcx_op_fx_compressor(rvcx_ctx*, const float* x_hd, int64_t n, int channels, int sr, float ratio, float threshold_db,
                          float attack_ms, float release_ms, float* y_hd, float* env_hd);
int rvcx_op_fx_gate(rvcx_ctx*, const float* x_hd, int64_t n, int channels, int sr, float threshold_db, float ratio,
                    float attack_ms, float release_ms, float* y_hd, float* env_hd);
int rvcx_op_fx_reverb(rvcx_ctx*, const float* x_hd, int64_t n, int channels, int sr, float room_size, float damping, float wet,
                      float dry, float width, float* y_hd);
int rvcx_op_fx_shelf(rvcx_ctx*, const float* x_hd, int64_t n, int channels, int sr, int high, float gain_db, float fc, float Q,
                     float* y_hd);
int rvcx_op_fx_chorus(rvcx_ctx*, const float* x_hd, int64_t n, int channels, int sr, float rate_hz, float depth,
                      float centre_delay_ms, float feedback, float mix, float* y_hd);
/* stage 8: vocal (n_v, 2) and instrumental (n_i, 2) int16 -> out (n_v, 2) int16 */
int rvcx_op_fx_mix(rvcx_ctx*, const int16_t* vocal_hd, int64_t n_v, const int16_t* inst_hd, int64_t n_i, float vocal_gain_db,
                   float inst_gain_db, int16_t* out_hd);
/* samples per chunk of the scan and follower kernels */
int rvcx_fx_chunk(void);
/* relaxation passes of the last rvcx_fx_chain / compressor / gate call that ran at least one chunk: {compressor, gate's
 * x^2 follower, gate's peak follower} (0: stage not run; the largest over the groups of a chain); returns the number of
 * groups that call ran in, -1 without a context */
int rvcx_fx_last_passes(rvcx_ctx*, int32_t* passes3);
/* Host only, no context, no GPU: the pieces of the definitions above and each stage run sequentially in float32 in the
 * defined order (one channel).  -1 (message via rvcx_last_error(NULL)) and nothing written for arguments out of range. */
float rvcx_fx_cte(double ms, int sr);
int rvcx_fx_delay(int sr, int D);
/* kind 0: stage 1 (Q, gain_db unused; coef5[2] = coef5[4] = 0), 1: low shelf, 2: high shelf -> {b0, b1, b2, a1, a2} */
int rvcx_fx_coeffs(int kind, int sr, double fc, double Q, double gain_db, float* coef5);
int rvcx_fx_highpass_host(const float* x, int64_t n, int sr, float fc, float* y);
int rvcx_fx_biquad_host(const float* x, int64_t n, const float* coef5, float* y);
/* env[n] = follower of |x| (square = 0) or x^2 (square = 1) with the constants c_attack / c_release (rvcx_fx_cte values);
 * sqrt_out != 0 writes sqrt(e[n]) */
int rvcx_fx_follower_host(const float* x, int64_t n, int square, int sqrt_out, float c_attack, float c_release, float* env);
/* stages 2 and 3 whole on one channel (followers + gain); env optional */
int rvcx_fx_compressor_host(const float* x, int64_t n, int sr, float ratio, float threshold_db, float attack_ms,
                            float release_ms, float* y, float* env);
int rvcx_fx_gate_host(const float* x, int64_t n, int sr, float threshold_db, float ratio, float attack_ms, float release_ms,
                      float* y, float* env);
/* one comb (delay D samples, feedback fb, damping d = 0.4 damping) / one all-pass on a given input */
int rvcx_fx_comb_host(const float* in, int64_t n, int D, float fb, float d, float* out);
int rvcx_fx_allpass_host(const float* in, int64_t n, int D, float* out);
int rvcx_fx_chorus_host(const float* x, int64_t n, int sr, float rate_hz, float depth, float centre_delay_ms, float feedback,
                        float mix, float* y);
int rvcx_fx_mix_host(const int16_t* vocal, int64_t n_v, const int16_t* inst, int64_t n_i, float vocal_gain_db,
                     float inst_gain_db, int16_t* out);

/* ---- loudness, true peak, limiter, master ------------------------------------------------------------------------------
 * Stages 9 - 12 continue "post-production": the signal, the rates and the error rules are that section's.  The loudness
 * measure is ITU-R BS.1770-4 / EBU R 128 (Tech 3341 for the conformance signals); the limiter and the master are this
 * project's own definitions.  Tested against float64 (tests/loudness_reference.py).
 *
 *  9 programme loudness L(x) in LUFS.  Per channel two biquads in series (transposed direct form II as stage 5), their
 *    coefficients formed in double:
 *      shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / sr), Vh = 10^(G/20),
 *        Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2; b = {Vh + Vb K/Q + K^2, 2 (K^2 - Vh), Vh - Vb K/Q + K^2} / a0;
 *        a1 = 2 (K^2 - 1) / a0, a2 = (1 - K/Q + K^2) / a0
 *      high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773; b = {1, -2, 1} (not normalised), a1, a2 as above
 *    (at 48 kHz the Recommendation's table to every printed digit).  The filter KEEPS double coefficients and double state
 *    on the device and on the host, unlike stages 1, 5 and 6: 1 + a1 + a2 of the high-pass is 1.6e-6 at 192 kHz, below what
 *    float32 coefficients resolve.  The float32 samples are widened, nothing else is rounded to float32.
 *    h = sr / 10.  Hop sums s_c[k]: the squared filtered samples of [k h, (k+1) h) summed in double; only whole hops count.
 *    Blocks j = 0 .. nb-1, nb = floor(n / h) - 3 (400 ms, 75 % overlap): z[j] = sum over channels of ((s_c[j] + s_c[j+1]) +
 *    s_c[j+2]) + s_c[j+3], divided by 4 h; channel weights are 1.  l[j] = -0.691 + 10 log10 z[j] (the momentary values).
 *    Absolute gate: l[j] > -70.  Gamma = -0.691 + 10 log10(mean of z over those blocks) - 10.  L = -0.691 + 10 log10(mean of
 *    z over the blocks with l[j] > -70 and l[j] > Gamma); -infinity when nb < 1 or no block passes.
 *    On the device the recurrence runs as the biquad scan does, on four states, and a hop's sum is put together from the
 *    partial sums of the chunks it touches, in chunk order; the gated means are summed in an order fixed by nb alone.  A
 *    result therefore depends on the item only -- not on B or the grouping -- and differs from the sequential host twin by
 *    the association of double sums.
 * 10 true peak TP(x) in dBTP: 4x oversampling by an interpolating Kaiser-windowed sinc, h(t) = sinc(t) I0(9 sqrt(1 - (t/12)^2))
 *    / I0(9) for |t| < 12, else 0.  y[4n + p] = sum over m of x[n - m] h(m + p/4); x is zero outside the signal.  Phase 0 is
 *    the sample itself.  Phases 1 - 3 have 24 taps each (m = -12 .. 11), formed in double and rounded once to float32, and are
 *    accumulated from zero with fmaf in the order m = -12, -11, ..., 11 on both sides.  p[n] = max over channels and the four
 *    phases of |y[4n + p]|, n = 0 .. len-1; TP = 20 log10 max p[n] (-infinity for silence).  Device = host twin bit for bit.
 * 11 limiter (ceiling_db <= 0, lookahead_ms in 0 .. 10, release_ms in 0 .. 10000), channels linked.  c = fl(10^(ceiling_db/20));
 *    r[n] = min(1, c / p[n]); W = floor(lookahead_ms sr / 1000); g[n] = min r[n .. n + W] (r = 1 past the end); e = the
 *    follower of stage 2 on u = 1 - g with attack constant 0 and release cte(release_ms), where u is 1 - g rounded UP (the
 *    smallest float32 with 1 - u <= g: to nearest, 1 - u could exceed g by 2^-25 once g < 0.5); q = 1 - e; s[n] = (q[n - W] + ... +
 *    q[n], in double, an index below 0 taking q[0]) / (W + 1), rounded to float32; y = x s.  s[n] <= r[n] for every n, hence
 *    |y[n]| <= c up to the last rounding; the true peak of y is not bounded by construction (measured: tests).  Skip: when
 *    max p <= c nothing is launched and the output is the input bit for bit.  Device = host twin bit for bit (min is exact,
 *    the follower is stage 2's, and q is a multiple of 2^-24, so the box sum is exact in double).
 * 12 master: vocal (n_v, 2) and instrumental (n_i, 2) float32 at one rate; target_lufs <= 0, vocal_offset_lu, ceiling_dbtp <= 0.
 *    The instrumental is cut or zero-padded to n_v first.  Lv, Li = stage 9 of the two.  gi = 10^((target - Li) / 20),
 *    gv = 10^((target + offset - Lv) / 20), each formed in double and rounded once; a stem at -infinity keeps gain 1.
 *    m = fl(gv V) + fl(gi I).  Lm = stage 9 of m; m is scaled by fl(10^((target - Lm) / 20)).  Stage 11 at the ceiling with
 *    lookahead 2 ms and release 100 ms.  int16 = clip(rint(32768 y)).  report7 per item, in double: {Lv, Li, Lm, loudness of
 *    y, TP in front of the limiter, TP of y, min s[n]} (y: the float result in front of the int16 rounding).
 *    The three gains are formed on the host from the device's loudness values (one synchronisation each), so that the host
 *    twin forms them with the same libm.
 *
 * Errors: a rate or channel count out of range, a value that is not finite, target or ceiling above 0, lookahead or release
 * out of range return -1 with a message and write nothing. */
/* blocks of stage 9 for n frames: max(0, floor(n / (sr / 10)) - 3) */
int64_t rvcx_fx_momentary_len(int64_t n, int sr);
/* stage 9 (and 10 when tp_db is given) on B items of `channels` channels.  lufs, tp_db: B doubles; momentary_hd (optional):
 * per item rvcx_fx_momentary_len floats (an item without a block is not touched).  Groups as rvcx_fx_chain. */
int rvcx_fx_loudness(rvcx_ctx*, int B, const float* const* x_hd, const int64_t* n, int channels, int sr, double* lufs,
                     double* tp_db, float* const* momentary_hd);
/* stage 10 on one item; p_hd (optional): the n values p[n] */
int rvcx_op_fx_truepeak(rvcx_ctx*, const float* x_hd, int64_t n, int channels, float* p_hd, double* tp_db);
/* stage 11 on one item; gain_hd (optional): the n values s[n] (all 1 when the stage is skipped) */
int rvcx_op_fx_limit(rvcx_ctx*, const float* x_hd, int64_t n, int channels, int sr, float ceiling_db, float lookahead_ms,
                     float release_ms, float* y_hd, float* gain_hd);
/* stage 12 on B covers: out_hd[b] receives (n_v[b], 2) int16; report7 (optional): B x 7 doubles.  n_i[b] may be 0 */
int rvcx_fx_master(rvcx_ctx*, int B, const float* const* vocal_hd, const int64_t* n_v, const float* const* inst_hd,
                   const int64_t* n_i, int sr, double target_lufs, double vocal_offset_lu, double ceiling_dbtp,
                   int16_t* const* out_hd, double* report7);
/* Host only, no context, no GPU.  coef10: {shelf b0, b1, b2, a1, a2, high-pass b0, b1, b2, a1, a2}; taps72: phases 1 - 3, 24 taps
 * each, tap j of a phase multiplying x[n + 12 - j] */
int rvcx_fx_kweight_coeffs(int sr, double* coef10);
int rvcx_fx_truepeak_taps(float* taps72);
int rvcx_fx_loudness_host(const float* x, int64_t n, int channels, int sr, double* lufs, float* momentary);
int rvcx_fx_truepeak_host(const float* x, int64_t n, int channels, float* p, double* tp_db);
int rvcx_fx_limit_host(const float* x, int64_t n, int channels, int sr, float ceiling_db, float lookahead_ms, float release_ms,
                       float* y, float* gain);
int rvcx_fx_master_host(const float* vocal, int64_t n_v, const float* inst, int64_t n_i, int sr, double target_lufs,
                        double vocal_offset_lu, double ceiling_dbtp, int16_t* out, double* report7);

/* ---- time stretch and pitch shift ---------------------------------------------------------------------------------------
 * Stages 13 and 14 continue "post-production" (signal, rates, error rules): the key change for a backing track.  A
 * phase-locked vocoder (identity phase locking) whose phases are integers in units of 2^-32 turn, so that its frame-to-frame
 * recurrence is an exact, associative scan: chunk length, segment length, batch and grouping change no bit.  The definition
 * is this project's own; tested against float64 (tests/stretch_reference.py).
 *
 * 13 time stretch by P / Q, per channel; 1 <= Q <= 2^20, Q / 2 <= P <= 2 Q.  n_s = floor((n P + floor(Q / 2)) / Q) samples.
 *    Geometry: N = the smallest power of two with 24 N >= sr (512 at 8 kHz .. 8192 at 192 kHz), H = N / 4, nb = N / 2 + 1,
 *    w[i] = 0.5 - 0.5 cos(2 pi i / N) formed in double and rounded once.  Analysis frames t = 0 .. T - 1, T = floor(n / H) + 1:
 *    D[t][k] = sum_i w[i] x[t H - N / 2 + i] e^(-2 pi i k i / N), x zero outside the signal, stored as float32 pairs; frames T
 *    and T + 1 are all zero.
 *    Per frame, from the float32 D: A2[k] = fl(fl(re re) + fl(im im)) (float32, no fma), A = sqrtf(A2), TH[k] =
 *    rint((double) atan2f(im, re) 2^31 / pi) mod 2^32, 0 when A2 == 0.  k is a peak when A2[k] > 0, A2[k] > A2[k - 1],
 *    A2[k] > A2[k - 2], A2[k] >= A2[k + 1], A2[k] >= A2[k + 2], a neighbour outside 0 .. nb - 1 counting as smaller.
 *    own[k] = the peak nearest to k, the lower one at equal distance; own[k] = k in a frame without a peak.
 *    Output frames j = 0 .. J - 1, J = ceil(T P / Q): t_j = floor(j Q / P), f_j = (j Q mod P) / P, M_j[k] = (1 - f_j) A[t_j][k]
 *    + f_j A[t_j + 1][k], phase PHI_j = R_j + TH[t_j] mod 2^32 with R_0 = 0 and, p = own[t_{j+1}][k],
 *      R_{j+1}[k] = R_j[own[t_j][p]] + TH[t_j + 1][p] - TH[t_{j+1}][p]  mod 2^32
 *    (a map R -> R o par + off; such maps compose exactly).  At P = Q every offset is 0 and the stage returns its input to
 *    rounding.  Synthesis: angle = (int32) PHI pi / 2^31, fr_j = w irfft(M_j e^(i PHI_j)) (scaling 1 / N),
 *    y[m] = sum_j fr_j[m + N / 2 - j H] / sum_j w^2[m + N / 2 - j H] over the frames 0 <= j < J that cover m, in ascending j,
 *    the divisor in double; 0 where the divisor is <= 1e-8.
 *    On the device the transforms, M, the angle and the numerator are float32; the host twin transforms and synthesises in
 *    double and rounds D, and y, once.  own is equal on both sides whenever D is, R whenever own and TH are (TH comes from
 *    each side's own atan2f).
 * 14 pitch shift by s semitones, |s| <= 12: P = floor(sr 2^(s / 12) + 0.5) formed in double, Q = sr; stage 13, then kaiser_hq
 *    (rvcx_resample_f64_kind's kind 0, the same tap loop, float32 samples and a double sum) from rate P to rate sr per channel
 *    plane, cut or zero-padded to n frames.  P == sr: the stage is skipped, nothing is launched, the output is the input bit
 *    for bit.
 *
 * Errors: |s| > 12, P / Q out of range, a value that is not finite, a rate or channel count out of range return -1 with a
 * message and write nothing. */
int64_t rvcx_fx_stretch_len(int64_t n, int64_t P, int64_t Q);              /* n_s; -1 for a refused ratio */
int rvcx_fx_stretch_frames(int64_t n, int sr, int64_t P, int64_t Q, int64_t* T, int64_t* J, int32_t* N);
int64_t rvcx_fx_pitch_ratio(int sr, double semitones);                     /* P of stage 14; -1 when refused */
int rvcx_fx_stretch_chunk(void);                                           /* output frames per chunk of the scan */
/* stage 13 on B items of `channels` channels: y_hd[b] receives (rvcx_fx_stretch_len(n[b], P, Q), channels).  Groups as
 * rvcx_fx_chain; long items run in segments of output frames with R and the overlap carried. */
int rvcx_fx_stretch(rvcx_ctx*, int B, const float* const* x_hd, const int64_t* n, int channels, int sr, int64_t P, int64_t Q,
                    float* const* y_hd);
/* stage 14 on B items: y_hd[b] receives (n[b], channels) */
int rvcx_fx_pitch_shift(rvcx_ctx*, int B, const float* const* x_hd, const int64_t* n, int channels, int sr, double semitones,
                        float* const* y_hd);
/* stage 13 on one channel of one item with its intermediates (each optional): D_hd (T + 2, nb, 2) float32, own_hd and TH_hd
 * (T + 2, nb), R_hd (J, nb) */
int rvcx_op_fx_stretch_taps(rvcx_ctx*, const float* x_hd, int64_t n, int sr, int64_t P, int64_t Q, float* y_hd, float* D_hd,
                            int32_t* own_hd, uint32_t* TH_hd, uint32_t* R_hd);
/* Host only, no context, no GPU.  The taps (optional) as above and for one channel only.  rvcx_fx_stretch_own_host: own of
 * one frame from its nb float32 pairs D */
int rvcx_fx_stretch_host(const float* x, int64_t n, int channels, int sr, int64_t P, int64_t Q, float* y, float* D, int32_t* own,
                         uint32_t* TH, uint32_t* R);
int rvcx_fx_pitch_shift_host(const float* x, int64_t n, int channels, int sr, double semitones, float* y, float* D, int32_t* own,
                             uint32_t* TH, uint32_t* R);
int rvcx_fx_stretch_own_host(const float* D, int nb, int32_t* own);

/* ---- noise reduction -----------------------------------------------------------------------------------------------------
 * Stage 15 continues "post-production" (signal, rates, error rules): a soft spectral gate that takes room noise, hiss or the
 * bleed of a separated stem out from under the voice, from a noise profile (mode 0) or adaptively (mode 1).  The gate decision
 * is a sigmoid on a smoothed level, so it is continuous in the spectrum: no threshold flips a bin between float32 and float64.
 * The definition is this project's own (noisereduce is the model for its two modes; parity with it is unpinned); tested
 * against float64 (tests/denoise_reference.py).
 *
 * 15 noise reduction, per channel.  N, H = N / 4, nb = N / 2 + 1 and w are stage 13's.  Frames t = 0 .. T - 1, T = floor(n / H)
 *    + 1; D[t][k] as in stage 13 (frame centred at t H, x zero outside the signal, float32 pairs); A2[t][k] = fl(fl(re re) +
 *    fl(im im)), no fma.
 *    Smoothed power S.  nf = floor(freq_smooth_hz N / (2 sr)) bins, nt = floor(time_smooth_ms sr / (2000 H)) frames; triangles
 *    wf[i] = nf + 1 - |i|, |i| <= nf, and wt likewise.  S[t][k] = (sum_dt wt[dt] (sum_dk wf[dk] A2[t + dt][k + dk])) / ((sum_dt
 *    wt[dt]) (sum_dk wf[dk])), every sum over the indices inside 0 .. T - 1 and 0 .. nb - 1 only (renormalised at the edges), in
 *    float32 from zero, each in ascending index order, every product and sum rounded (no fma); the divisor is an integer below
 *    2^24.  nf = 0 or nt = 0 leaves that axis alone.  nf > 64 or nt > 16 is refused.  Device = host twin bit for bit on a given A2.
 *    mode 0, profile: l[t][k] = fl(10 log10f(fl(S + 1e-20f))).  The profile frames are those of a noise clip of the same rate and
 *    channel count, through the same analysis and smoothing on its own grid, channel c of the clip serving channel c of the
 *    item.  WITHOUT a clip the profile frames are the item's own: everything stationary in the item is then treated as noise.
 *    mu[k], sd[k]: mean and population standard deviation of l over the Tp profile frames, two passes in double (sum of l, then
 *    sum of (l - mu)^2), each as partial sums over 64 consecutive frames added in ascending order.  thr = mu + n_std sd (double);
 *    m = 1 / (1 + expf(-z)), z = (float)((l - thr) / knee_db) formed in double.
 *    mode 1, adaptive: A = sqrtf(S), c = exp(-H / (sr time_constant_s)) in double.  f[t] = (1 - c) A[t] + c f[t - 1], f[-1] =
 *    A[0]; b[t] = (1 - c) f[t] + c b[t + 1], b[T] = f[T - 1]; both in double, per bin, two products and one sum each.  r = (A - b)
 *    / (b + 1e-10); m = 1 / (1 + expf(-z)), z = (float)((r - thresh_mult) slope) formed in double.  A tone that holds steady
 *    becomes the floor and is removed with it: that is the mode's documented property (a noise gate for speech and song
 *    between pauses, not for drones).
 *    Gain and synthesis: g = fl(1 - fl(strength fl(1 - m))), Y = g D (the imaginary parts of bins 0 and N / 2 dropped), fr_t =
 *    w irfft(Y_t) (scaling 1 / N), y[i] = sum_t fr_t[i + N / 2 - t H] / sum_t w^2[i + N / 2 - t H] over the frames that cover i in
 *    ascending t, the divisor in double; 0 where the divisor is <= 1e-8.  The output has n frames.
 *    On the device the transforms and the numerator are float32; the host twin transforms and synthesises in double and rounds
 *    D, and y, once, and applies the float32 roundings of A2, S, l and m as defined.
 *    Skip: strength == 0 launches nothing, the output is the input bit for bit.
 *    A result depends on the item and its noise clip alone: B, the grouping, RVCX_MAX_BATCH and the other members change no bit.
 *
 * Errors: a value out of the ranges below or not finite, a rate or channel count out of range, a noise clip in mode 1, n < 1
 * return -1 with a message and write nothing.  An item that does not fit the arena budget on its own is refused with a
 * message that names its size (one item is not cut into segments). */
typedef struct {
  int32_t sample_rate, channels;
  int32_t mode;                 /* 0 profile, 1 adaptive (default 1) */
  float strength;               /* 0 .. 1 (0.7) */
  float n_std;                  /* mode 0: 0 .. 10 (3) */
  float knee_db;                /* mode 0: 0.1 .. 20 (1) */
  float thresh_mult;            /* mode 1: 0 .. 20 (1) */
  float slope;                  /* mode 1: 0.1 .. 100 (5) */
  float time_constant_s;        /* mode 1: 0.05 .. 30 (2) */
  float freq_smooth_hz;         /* >= 0 (500) */
  float time_smooth_ms;         /* >= 0 (50) */
} rvcx_fx_denoise_params;
/* T and N of an item of n frames, and the half-widths nf, nt of the default smoothing (500 Hz, 50 ms) at this rate */
int rvcx_fx_denoise_frames(int64_t n, int sr, int64_t* T, int32_t* N, int32_t* nf, int32_t* nt);
/* frames and bins of a smoothing tile and profile frames per partial sum: the lengths at which the kernels take another path */
int rvcx_fx_denoise_tiles(int32_t* tile_t, int32_t* tile_k, int32_t* stat_chunk);
/* stage 15 on B items of params->channels channels: y_hd[b] receives (n[b], channels).  noise_hd may be NULL, and so may any
 * entry of it; noise_hd[b] holds (n_noise[b], channels).  Items that name the same clip share its analysis.  Groups as
 * rvcx_fx_chain. */
int rvcx_fx_denoise(rvcx_ctx*, int B, const float* const* x_hd, const int64_t* n, const float* const* noise_hd,
                    const int64_t* n_noise, const rvcx_fx_denoise_params*, float* const* y_hd);
/* stage 15 on one channel of one item with its intermediates (each optional): D_hd (T, nb, 2) float32, S_hd (T, nb), mu_hd and
 * sd_hd (nb doubles, mode 0), b_hd (T, nb) doubles (mode 1), m_hd (T, nb) */
int rvcx_op_fx_denoise_taps(rvcx_ctx*, const float* x_hd, int64_t n, const float* noise_hd, int64_t n_noise,
                            const rvcx_fx_denoise_params*, float* y_hd, float* D_hd, float* S_hd, double* mu_hd, double* sd_hd,
                            double* b_hd, float* m_hd);
/* Host only, no context, no GPU.  The taps (optional) as above and for one channel only.  rvcx_fx_denoise_smooth_host: S of a
 * given (T, nb) array A2 */
int rvcx_fx_denoise_host(const float* x, int64_t n, const float* noise, int64_t n_noise, const rvcx_fx_denoise_params*, float* y,
                         float* D, float* S, double* mu, double* sd, double* b, float* m);
int rvcx_fx_denoise_smooth_host(const float* A2, int64_t T, int nb, int nf, int nt, float* S);

/* ---- live post-production ---------------------------------------------------------------------------------------------
 * The board of "post-production" inside a live-stream session: rvcx_stream_open_fx puts stages 1 - 7 behind the output
 * resampler, inside the step, on the device, with all state carried from block to block.
 *
 * Signal.  For stream s, v = everything the session has emitted since open or reset at the delivery rate sr (out_rate when the
 * output is resampled, else the voice model's rate), the zeros of the output resampler's delay included, duplicated to stereo
 * (L = R, as convert_to_stereo does).  Output.  A session with effects returns stages 1 - 7 (the definitions above, in the
 * board's order) applied to v from zero state at sample 0 of the session, stereo interleaved (frames, 2); step k returns
 * samples [k Bout, (k + 1) Bout) of that result.  The board adds no delay.  Identity stages follow the rule above (ratio == 1,
 * 0 dB and mix == 0 are skipped; the high-pass and the reverb never are).  The chorus' tau(n) takes the global sample index n =
 * step counter x block (int64, restarting at 0 on reset); there is no device counter.
 *
 * Arithmetic -- what makes the result independent of the cut.  Every stage runs in sample order, every rounding is one IEEE
 * operation (contraction off), and the step functions are those of the one-shot kernels and host twins (csrc/effects_device.h):
 *  - high-pass, low shelf, high shelf: the float32 transposed-direct-form-II recurrence sample by sample, (s1, s2) carried.
 *    Equal to rvcx_fx_highpass_host / rvcx_fx_biquad_host on the whole signal BIT FOR BIT.  Deliberately not the one-shot
 *    kernels' bits: their chunked scan carries the state in double and associates by the row's length.
 *  - compressor, gate: the followers in sample order with e (and the gate's r) carried, the one-shot device gain.  Equal to
 *    rvcx_op_fx_compressor / rvcx_op_fx_gate on the whole signal bit for bit (the envelopes thereby to rvcx_fx_follower_host).
 *  - reverb: per comb o = buf[i]; last = fma(last, d, o (1 - d)); buf[i] = fma(last, fb, in); the comb outputs summed in the
 *    listed order; the four all-passes in series; the mix FMAs of stage 4.  1 - d is (float)(1 - (double)(float)d), the comb
 *    twin's.  Equal to rvcx_fx_reverb_host (below) on the whole signal bit for bit; not to rvcx_op_fx_reverb, whose 64-lane
 *    scan re-associates the damping one-pole.
 *  - chorus: the one-shot tap (fx_chorus_tap) at the global index.  Equal to rvcx_op_fx_chorus on the whole signal bit for
 *    bit, for feedback == 0 and != 0.
 * So live and one-shot results differ in the last bits for the linear stages and the reverb, and only there.
 *
 * Rates.  sr a multiple of 100 Hz in 8000 .. 192000; 3200 .. 7900 too, but only when the voice model's own rate is below 8000
 * (the reduced test models' 4800 / 6000 Hz; the concession rvcx_stream_open_io makes -- at 4800 Hz the comb delays are 121 ..,
 * the shortest all-pass 24, the chorus block 20).  Anything else is refused at open, with a message.
 *
 * State.  Per stream: the biquad and follower states, 16 comb lines with their one-pole states, 8 all-pass lines, and per
 * channel a chorus ring of sr + 2 samples (the 1000 ms the board accepts) + two blocks.  Lines and rings are indexed by the
 * global sample index mod their length; there are no stored positions, and a block may be shorter than every delay.  All of
 * it is the session's own memory and exists twice: a step reads set cur and writes the other one, and the sets change places
 * only when the step has succeeded (ring, carry, FIFOs).  The board adds no host synchronisation to a step.  rvcx_last_timing
 * counts it in the last interval ("SOLA + copies").  rvcx_stream_reset zeroes it; rvcx_stream_close and rvcx_destroy free it. */
/* fx == NULL: rvcx_stream_open_io, launch for launch.  fx->sample_rate must be 0 or the delivery rate, fx->channels 0 or 2; the
 * refusals of rvcx_fx_chain (ratio < 1, |feedback| >= 1, a value that is not finite, ...) are made here, and nothing is opened */
int rvcx_stream_open_fx(rvcx_ctx*, int model_id, const rvcx_stream_cfg*, const rvcx_stream_io*, const rvcx_fx_params* fx,
                        const rvcx_params* p, const int32_t* sid, const float* pitch, int* stream_id);
/* 1, or 2 for a session with effects: out_hd[s] of a step holds rvcx_stream_out_len x channels floats.  pre_sola_hd, offsets
 * and rvcx_stream_last_taps keep their meaning: mono, in front of the board */
int rvcx_stream_out_channels(rvcx_ctx*, int stream_id);
/* new parameters from the next step on.  All state is kept (a reverb tail rings on), except that the state of a stage the new
 * values make an identity is zeroed once, in both sets: it starts clean when it comes back.  A refused value: -1, nothing
 * changed.  Refused on a session opened without effects (its channel count is fixed at open).  No parameter smoothing. */
int rvcx_stream_set_fx(rvcx_ctx*, int stream_id, const rvcx_fx_params*);
/* device ms of the board in the last step: {high-pass (with the load), compressor, gate, reverb, low shelf, high shelf,
 * chorus (with the interleave), total} */
int rvcx_stream_last_fx_ms(rvcx_ctx*, int stream_id, float* ms8);
/* the session's board without a session and without a model: S rows of `frames` input frames (x_hd: S x frames x channels,
 * channels 1 or 2, interleaved), cut into blocks of block_frames 10 ms frames (frames must be a multiple of block_frames * sr /
 * 100), through the same state and kernel code a session runs per step; y_hd receives S x frames x 2.  stage_mask bit i enables
 * stage i + 1; a disabled stage is skipped like an identity.  sr: the rule above, 3200 .. 7900 allowed */
int rvcx_op_stream_fx(rvcx_ctx*, const float* x_hd, int S, int64_t frames, int channels, int sr, int block_frames,
                      const rvcx_fx_params* fx, uint32_t stage_mask, float* y_hd);
/* host only, no context: stage 4 on one stereo item, x (n, 2) -> y (n, 2), sequentially in float32 from rvcx_fx_comb_host /
 * rvcx_fx_allpass_host and the mix FMAs; sr as the other host twins.  -1 and nothing written for arguments out of range */
int rvcx_fx_reverb_host(const float* x, int64_t n, int sr, float room_size, float damping, float wet, float dry, float width,
                        float* y);

/* ---- live noise reduction -------------------------------------------------------------------------------------------------
 * Stage 16 is stage 15 made causal, so that a live-stream session can run it inside a step, at either edge: on the 16 kHz mono
 * block in front of the ring (a microphone in a room feeds HuBERT and the F0 model directly) and on what leaves, behind the
 * output resampler and in front of the board.  Stage 15 cannot run there: its adaptive floor runs backward from the end of the
 * item and its time triangle reads frames that have not arrived.  The definition is this project's own; tested against float64
 * (tests/denoise_live_reference.py).
 *
 * 16 live noise reduction, one channel, defined on x[0 .. ): everything the stream has received since open or reset.  There is
 *    no last frame.  sr a multiple of 100 Hz in 3200 .. 192000.
 *    Geometry: N = the smallest power of two with 48 N >= sr, and never below 512 (512 up to 24 kHz, 1024 at 44.1 and 48 kHz,
 *    2048 at 96 kHz, 4096 at 192 kHz), H = N / 4, nb = N / 2 + 1, w[i] = 0.5 - 0.5 cos(2 pi i / N) formed in double and rounded
 *    once (stage 13's formula at this N).
 *    Frames t = 0, 1, ..: D[t][k] = sum_i w[i] x[t H - N / 2 + i] e^(-2 pi i k i / N), x = 0 in front of sample 0, float32 pairs;
 *    A2[t][k] = fl(fl(re re) + fl(im im)), no fma.  Frame t is complete once sample t H + N / 2 - 1 has arrived: n samples
 *    complete T(n) = floor((n - N / 2) / H) + 1 frames, none while n < N / 2.
 *    Smoothed power S.  nf = floor(freq_smooth_hz N / (2 sr)) bins, wf[i] = nf + 1 - |i|, |i| <= nf: F[t][k] = sum_dk wf[dk]
 *    A2[t][k + dk] over the bins inside 0 .. nb - 1, in float32 from zero in ascending k + dk, every product and sum rounded.
 *    nt = floor(time_smooth_ms sr / (1000 H)) frames ON THE PAST SIDE ONLY, wt[dt] = nt + 1 - |dt|, dt = -nt .. 0: S[t][k] =
 *    (sum_dt wt[dt] F[t + dt][k]) / ((sum_dt wt[dt]) (sum_dk wf[dk])), the sum over the frames t + dt >= 0 in float32 from zero
 *    in ascending t + dt, the weight sums over the same indices; the divisor is an integer below 2^24, converted to float32,
 *    and the quotient is one float32 division.  nf = 0 or nt = 0 leaves that axis alone.  nf > 64 or nt > 32 is refused.
 *    mode 1, adaptive floor, forward only, per bin, in double: A = sqrtf(S), c_up = exp(-H / (sr time_constant_s)), c_dn =
 *    exp(-H / (sr fall_time_s)); f[-1] = A[0]; f[t] = (1 - c) A[t] + c f[t - 1] with c = c_up when A[t] >= f[t - 1] and c_dn
 *    otherwise (two products and one sum; 1 - c is formed in double).  The floor rises slowly under a voice and falls fast
 *    into a pause; both branches give f[t - 1] at A[t] == f[t - 1], so f is continuous in the spectrum.  r = (A - f) / (f +
 *    1e-10); m = 1 / (1 + expf(-z)), z = (float)((r - thresh_mult) slope) formed in double (stage 15's rule with f for b).
 *    mode 0, profile: mu[k], sd[k] from a noise clip given at open (same rate, one channel, N / 2 .. 2^22 samples): the frames
 *    of the clip are the Tp = T(n_noise) frames complete inside it, through this analysis and this smoothing from sample 0 of
 *    the clip; l = fl(10 log10f(fl(S + 1e-20f))); mean and population standard deviation of l over the Tp frames as in stage 15
 *    (two passes in double, partial sums over 64 consecutive frames added in ascending order); thr = mu + n_std sd; m = 1 /
 *    (1 + expf(-z)), z = (float)((l - thr) / knee_db) formed in double.  Mode 0 without a clip is refused, and so is a clip
 *    in mode 1.
 *    Gain and synthesis: g = fl(1 - fl(strength fl(1 - m))), Y = g D (the imaginary parts of bins 0 and N / 2 dropped), fr_t =
 *    w irfft(Y_t) (scaling 1 / N); y[i] = (sum_t fr_t[i + N / 2 - t H]) / (sum_t w^2[i + N / 2 - t H]) over all frames t >= 0
 *    that cover i, each sum in ascending t; the numerator in float32 from zero, the divisor in double (it is never below 1 and
 *    has period H from sample N / 2 on), the quotient formed in double and rounded once.
 *    Delay: d = N samples.  A step that has received the samples below (k + 1) Bn emits y[k Bn - N + i], i < Bn, and 0 where
 *    that index is negative: every frame that covers an emitted sample is complete.
 *    strength == 0: the stage stays in the path with its delay and emits x[k Bn - N + i], the delayed input bit for bit.
 *    Analysis, floor and the sums of the synthesis keep running, so the floor is learned when strength comes back.
 *    On the device the transforms and the numerator are float32; the host twin transforms and synthesises in double and rounds
 *    D, and y, once, and applies the float32 roundings of A2, F, S, l and m as defined.
 *    The result depends on the samples received alone: the block length (shorter than H, so that a step completes no frame, or
 *    longer than N), the other streams of a group and a repeated step change no bit.
 *
 * State, per stream and side: the last N samples, the N overlap-add sums behind the last sample emitted, the last nt rows of
 * F, f (nb doubles); mu and sd once per side.  It is the session's own memory and exists twice: a step reads set cur and
 * writes the other one whole, and the sets change places only when the step has succeeded (ring, carry, FIFOs, the board).
 * Nothing in it is a stored position: the frames a step completes follow from the step counter x block.  One launch of one
 * 256-lane workgroup per stream, per side and step; no atomics, no host synchronisation.
 *
 * Errors: a value out of the ranges below or not finite, a rate that is not the side's (or 0) or out of range, channels other
 * than 0 or 1, mode 0 without a clip, a clip in mode 1 or of a length out of range return -1 with a message and write or
 * open nothing. */
typedef struct {
  int32_t sample_rate, channels; /* 0 or the rate of the side; 0 or 1 */
  int32_t mode;                 /* 0 profile, 1 adaptive (default 1) */
  float strength;               /* 0 .. 1 (0.9; stage 15's 0.7 leaves the pauses 10 dB down, 0.9 gives 18 dB) */
  float n_std;                  /* mode 0: 0 .. 10 (3) */
  float knee_db;                /* mode 0: 0.1 .. 20 (1) */
  float thresh_mult;            /* mode 1: 0 .. 20 (1) */
  float slope;                  /* mode 1: 0.1 .. 100 (5) */
  float time_constant_s;        /* mode 1, rising: 0.05 .. 30 (2) */
  float fall_time_s;            /* mode 1, falling: 0.01 .. time_constant_s (0.2) */
  float freq_smooth_hz;         /* >= 0 (500) */
  float time_smooth_ms;         /* >= 0 (50) */
} rvcx_live_denoise_params;
/* one side of a session: params == NULL, the side is absent.  noise_hd: the clip of mode 0 (host or device), n_noise samples */
typedef struct {
  const rvcx_live_denoise_params* params;
  const float* noise_hd;
  int64_t n_noise;
} rvcx_stream_dn_side;
typedef struct {
  rvcx_stream_dn_side in;       /* behind the input resampler (or on the 16 kHz mono block), in front of the ring, at 16 kHz */
  rvcx_stream_dn_side out;      /* behind the output resampler, in front of the board, mono, at the delivery rate */
} rvcx_stream_dn;
/* N of stage 16 at this rate: the delay a side adds, in samples of its rate; -1 for a refused rate (host only) */
int rvcx_stream_denoise_delay(int sr);
/* T(n), N and the half-widths nf, nt of the given widths at this rate, before any refusal of their size (host only) */
int rvcx_stream_denoise_frames(int64_t n, int sr, float freq_smooth_hz, float time_smooth_ms, int64_t* T, int32_t* N, int32_t* nf,
                               int32_t* nt);
/* dn == NULL or both sides absent: rvcx_stream_open_fx, launch for launch and bit for bit.  Every refusal of both sides is made
 * first, and nothing is opened.  pre_sola_hd, offsets and the native tap of rvcx_stream_last_taps stay in front of the output
 * side; its in16k tap returns what entered the ring, behind the input side. */
int rvcx_stream_open_dn(rvcx_ctx*, int model_id, const rvcx_stream_cfg*, const rvcx_stream_io*, const rvcx_fx_params* fx,
                        const rvcx_stream_dn* dn, const rvcx_params* p, const int32_t* sid, const float* pitch, int* stream_id);
/* new values for side 0 (input) or 1 (output) from the next step on.  Geometry, delay and the state's layout are fixed at
 * open: a time_smooth_ms that changes nt is refused, and so is mode 0 on a side opened without a clip.  All state is kept (the
 * floor stays learned).  A refused value: -1, nothing changed.  Refused for a side that was absent at open. */
int rvcx_stream_set_denoise(rvcx_ctx*, int stream_id, int side, const rvcx_live_denoise_params*);
/* device ms of the two sides in the last step ({input, output}; 0 for an absent side).  rvcx_last_timing keeps nine slots: the
 * input side is counted in the first interval ("F0"), the output side in the last ("SOLA + copies").  rvcx_stream_delays adds
 * N of each present side to the delay it reports. */
int rvcx_stream_last_dn_ms(rvcx_ctx*, int stream_id, float* ms2);
/* a side without a session and without a model: S mono rows of `frames` samples (x_hd: S x frames) at rate sr, cut into blocks
 * of block_frames 10 ms frames (frames must be a multiple of block_frames * sr / 100), through the same state and kernel code
 * a session runs per step; y_hd receives S x frames, delayed by N.  noise_hd / n_noise: the clip of mode 0, shared by the rows.
 * Optional taps for the T(frames) frames completed: S_hd and m_hd (S, T, nb) float32, f_hd (S, T, nb) doubles (mode 1) */
int rvcx_op_stream_denoise(rvcx_ctx*, const float* x_hd, int S, int64_t frames, int sr, int block_frames,
                           const rvcx_live_denoise_params*, const float* noise_hd, int64_t n_noise, float* y_hd, float* S_hd,
                           double* f_hd, float* m_hd);
/* host only, no context: stage 16 on the whole signal x[0 .. n) -> y (n samples, delayed by N).  Optional taps for the T(n)
 * frames: D (T, nb, 2) float32, S and m (T, nb), f (T, nb) doubles (mode 1) */
int rvcx_fx_denoise_live_host(const float* x, int64_t n, int sr, const float* noise, int64_t n_noise,
                              const rvcx_live_denoise_params*, float* y, float* D, float* S, double* f, float* m);

/* ---- formant shift and formant-preserving pitch shift ------------------------------------------------------------------
 * Stages 17 and 18 continue "post-production" (signal, rates, error rules): the timbre control.  Per frame a spectral envelope
 * is estimated (the "true envelope": cepstral smoothing iterated under the maximum with the log spectrum, so that it rides the
 * harmonic peaks) and replaced by a warped copy of an envelope: the frame's own, warped in frequency (a formant shift), or the
 * envelope of a second signal at the same frame (stage 18: the untransposed signal's, which keeps the formants of a vocal in
 * place through a key change).  Maximum, linear warp and clamp are continuous in the spectrum: nothing flips a bin between
 * float32 and float64.  The definition is this project's own; tested against float64 (tests/formant_reference.py).
 *
 * 17 envelope transfer, per channel.  N, H = N / 4, nb = N / 2 + 1 and w are stage 13's.  Frames t = 0 .. T - 1, T = floor(n / H)
 *    + 1; D[t][k] as in stage 13 (float32 pairs); A2[k] = fl(fl(re re) + fl(im im)), no fma.
 *    Log spectrum: top = max_k A2[k] (exact), eps = fl(fl(1e-10f top) + 1e-20f), L[k] = fl(0.5f logf(fl(A2[k] + eps))).
 *    True envelope: nc = floor(quefrency_ms sr / 1000) formed in double, 1 <= nc <= N / 8.  lift(V): the length-N real even
 *    extension of V[0 .. nb) (V[N - k] = V[k]), its inverse transform c[q] (real, even), c[q] kept for q <= nc, c[N - q] = c[q]
 *    set from it, the rest zero; the forward transform, its real part on 0 .. nb - 1.  V_0 = L; for i = 0 .. iterations: E =
 *    lift(V_i), V_{i+1} = max(L, E): iterations + 1 lifts.  E is float32 after every lift.
 *    Target: Es = the item's own E, or, with a source (a second signal of the same rate, channel count and length n, channel c
 *    serving channel c), the E of frame t of the source through the same steps.  Warp, in double: u = k / ratio, i = floor(u),
 *    f = u - i, W[k] = (float)((1 - f) Es[i] + f Es[i + 1]), W[k] = Es[nb - 1] when i >= nb - 1.
 *    Gain: d = amount (W[k] - E[k]) in double, clamped to +- max_gain_db ln(10) / 20, g = expf((float) d).
 *    Energy (keep_energy == 1): e0 = sum_k c_k A2[k], e1 = sum_k c_k ((g g) A2[k]), c_k = 1 at k = 0 and k = nb - 1, else 2, in
 *    double, every product rounded: 256 partial sums, partial p over the bins k = p mod 256 in ascending k, then the partials
 *    added in ascending p.  s = (float) sqrt(e0 / e1), 1 when e1 == 0; s = 1 with keep_energy == 0.
 *    Synthesis is stage 15's: Y = fl(g s) D (the imaginary parts of bins 0 and N / 2 dropped), fr_t = w irfft(Y_t) (scaling
 *    1 / N), y[i] = sum_t fr_t[i + N / 2 - t H] / sum_t w^2[i + N / 2 - t H] over the frames that cover i in ascending t, the
 *    divisor in double; 0 where the divisor is <= 1e-8.  The output has n frames.
 *    On the device the transforms (those of the lifts too), E and the numerator are float32; the envelope of the frame and of
 *    its source frame pass through the lifts as the real and the imaginary part of one complex sequence.  The host twin
 *    transforms and synthesises in double and rounds D, E (after every lift), W, g, s and y as defined.  Given the same A2
 *    and g, s is equal on both sides bit for bit.
 *    Skip: amount == 0 launches nothing; an item without a source at ratio == 1 is its own target and is not run.  In both cases
 *    the output is the input bit for bit.
 *    A result depends on the item and its source alone: B, the grouping, RVCX_MAX_BATCH and the other members change no bit.
 * 18 formant-preserving pitch shift by s semitones: stage 14, then stage 17 on its output with src = the stage's own input and
 *    ratio = 1 (both have n frames on one grid).  P == sr: everything is skipped, the output is the input bit for bit.
 *
 * Errors: a value out of the ranges below or not finite, a rate or channel count out of range, nc outside 1 .. N / 8, n < 1
 * return -1 with a message and write nothing.  An item that does not fit the arena budget on its own is refused with a
 * message that names its size (one item is not cut into segments).  A source has its item's length by definition: the ABI
 * takes no second length, the Python layer refuses a source of another length. */
typedef struct {
  int32_t sample_rate, channels;
  float ratio;                  /* 0.5 .. 2 (1): formants move up by this factor */
  float amount;                 /* 0 .. 1 (1) */
  float quefrency_ms;           /* > 0 with 1 <= nc <= N / 8 (1.5) */
  int32_t iterations;           /* 0 .. 16 (8) */
  float max_gain_db;            /* 0 .. 48 (24) */
  int32_t keep_energy;          /* 0 or 1 (1) */
} rvcx_fx_formant_params;
/* T, N and nc of an item of n frames at this rate and quefrency (host only) */
int rvcx_fx_formant_frames(int64_t n, int sr, float quefrency_ms, int64_t* T, int32_t* N, int32_t* nc);
/* stage 17 on B items of params->channels channels: y_hd[b] receives (n[b], channels).  src_hd may be NULL, and so may any
 * entry of it; src_hd[b] holds (n[b], channels).  Groups as rvcx_fx_chain. */
int rvcx_fx_formant(rvcx_ctx*, int B, const float* const* x_hd, const int64_t* n, const float* const* src_hd,
                    const rvcx_fx_formant_params*, float* const* y_hd);
/* stage 18 on B items: y_hd[b] receives (n[b], channels); no output may overlap any input of the call, in whole or in part
 * (refused: stage 14 writes the outputs while the inputs are still the sources).  params may be NULL (the defaults);
 * its sample_rate, channels and ratio are not read. */
int rvcx_fx_pitch_shift_formant(rvcx_ctx*, int B, const float* const* x_hd, const int64_t* n, int channels, int sr,
                                double semitones, const rvcx_fx_formant_params*, float* const* y_hd);
/* stage 17 on one channel of one item with its intermediates (each optional): D_hd (T, nb, 2) float32, E_hd, Es_hd and g_hd
 * (T, nb), s_hd (T) */
int rvcx_op_fx_formant_taps(rvcx_ctx*, const float* x_hd, int64_t n, const float* src_hd, const rvcx_fx_formant_params*,
                            float* y_hd, float* D_hd, float* E_hd, float* Es_hd, float* g_hd, float* s_hd);
/* Host only, no context, no GPU.  The taps (optional) as above and for one channel only.  rvcx_fx_formant_envelope_host: E of
 * one frame from its nb = N / 2 + 1 values L */
int rvcx_fx_formant_host(const float* x, int64_t n, const float* src, const rvcx_fx_formant_params*, float* y, float* D,
                         float* E, float* Es, float* g, float* s);
int rvcx_fx_pitch_shift_formant_host(const float* x, int64_t n, int channels, int sr, double semitones,
                                     const rvcx_fx_formant_params*, float* y);
int rvcx_fx_formant_envelope_host(const float* L, int N, int nc, int iterations, float* E);

/* ---- live formant shift ---------------------------------------------------------------------------------------------------
 * Stage 19 is stage 17 without a source, made causal on stage 16's grid, so that a live-stream session can run it inside a
 * step, at either edge: on the 16 kHz mono block in front of the ring (behind stage 16 when the side has one), where it moves
 * the formants of the microphone signal before HuBERT and the F0 model see it, and on what leaves, behind the output resampler
 * and stage 16 and in front of the board.  Stage 17 cannot run there: its grid has a last frame, its transform at 16 kHz is
 * 1024 points (64 ms), and cut into blocks it leaves a seam at every block edge.  The definition is this project's own; tested
 * against float64 (tests/formant_live_reference.py).
 *
 * 19 live formant shift, one channel, defined on x[0 .. ): everything the stream has received since open or reset.  There is no
 *    last frame.  sr: stage 16's rule (a multiple of 100 Hz in 3200 .. 192000).
 *    Geometry: stage 16's, not stage 13's.  N = the smallest power of two with 48 N >= sr, never below 512; H = N / 4, nb = N / 2
 *    + 1, w stage 13's formula at this N.  Frame t is complete once sample t H + N / 2 - 1 has arrived; x = 0 in front of
 *    sample 0; n samples complete T(n) frames as in stage 16.
 *    Per frame, stage 17's rules from its own text: D, A2, top, eps and L; the true envelope (iterations + 1 lifts, E in float32
 *    after each) with nc = floor(quefrency_ms sr / 1000), 1 <= nc <= N / 8 at THIS N (refused otherwise; the default 1.5 ms fits
 *    at every admitted rate, since N >= sr / 48 > 0.012 sr); Es = E (there is no source); the warp in double; the gain with its
 *    clamp; the energy scale with stage 17's summation order; Y = fl(g s) D with the imaginary parts of bins 0 and N / 2
 *    dropped; fr_t = w irfft(Y_t) (scaling 1 / N).
 *    Synthesis and delay are stage 16's: y[i] = (sum_t fr_t[i + N / 2 - t H]) / (sum_t w^2[i + N / 2 - t H]) over all frames t >=
 *    0 that cover i, each sum in ascending t; the numerator in float32 from zero, the divisor in double, the quotient formed in
 *    double and rounded once.  Delay: d = N samples.  A step that has received the samples below (k + 1) Bn emits y[k Bn - N +
 *    i], i < Bn, and 0 where that index is negative.
 *    Off: amount == 0 or ratio == 1 keeps the stage in the path with its delay; it emits x[k Bn - N + i], the delayed input bit
 *    for bit.  Frames and sums keep running (every gain is then 1), so switching it on in mid-session starts from correct
 *    overlap-add sums, and the latency never changes.
 *    Parameter changes: frame t uses the values in force in the step that completes it, and a step emits by the values in force
 *    in it.
 *    On the device the transforms (those of the lifts too), E and the numerator are float32.  The host twin transforms and
 *    synthesises in double and rounds D, E (after every lift), W, g, s and y as stage 17's twin does.
 *    The result depends on the samples received and the parameter history alone: the block length (shorter than H, so that a
 *    step completes no frame, or longer than N), the other streams of a group and a repeated step change no bit.
 *
 * State, per stream and side: the last N samples and the N overlap-add sums behind the last sample emitted -- a frame has no
 * recurrence across frames.  It is the session's own memory and exists twice, like stage 16's: a step reads set cur and writes
 * the other one whole.  Nothing in it is a stored position.  Two launches per side and step: the frames the step completes side
 * by side, one 256-lane workgroup each (skipped when the step completes none), then one workgroup per stream that adds them to
 * the sums in ascending t, emits the block and writes the new state; no atomics, no host synchronisation.
 *
 * Errors: a value out of the ranges below or not finite, a rate that is not the side's (or 0) or out of range, channels other
 * than 0 or 1, nc outside 1 .. N / 8 return -1 with a message and write or open nothing. */
typedef struct {
  int32_t sample_rate, channels; /* 0 or the rate of the side; 0 or 1 */
  float ratio;                  /* 0.5 .. 2 (1): formants move up by this factor */
  float amount;                 /* 0 .. 1 (1) */
  float quefrency_ms;           /* > 0 with 1 <= nc <= N / 8 (1.5) */
  int32_t iterations;           /* 0 .. 16 (8) */
  float max_gain_db;            /* 0 .. 48 (24) */
  int32_t keep_energy;          /* 0 or 1 (1) */
} rvcx_live_formant_params;
/* one side of a session: params == NULL, the side is absent */
typedef struct {
  const rvcx_live_formant_params* params;
} rvcx_stream_fm_side;
typedef struct {
  rvcx_stream_fm_side in;       /* behind the input resampler and stage 16, in front of the ring, at 16 kHz */
  rvcx_stream_fm_side out;      /* behind the output resampler and stage 16, in front of the board, mono, at the delivery rate */
} rvcx_stream_fm;
/* N of stage 19 at this rate: the delay a side adds, in samples of its rate; -1 for a refused rate (host only) */
int rvcx_stream_formant_delay(int sr);
/* T(n), N and nc at this rate and quefrency; nc outside 1 .. N / 8 is refused (host only) */
int rvcx_stream_formant_frames(int64_t n, int sr, float quefrency_ms, int64_t* T, int32_t* N, int32_t* nc);
/* fm == NULL or both sides absent: rvcx_stream_open_dn, launch for launch and bit for bit.  Every refusal of both sides is made
 * first, and nothing is opened.  Order in the step: input resampler, stage 16 in, stage 19 in, ring; output resampler, stage 16
 * out, stage 19 out, board.  The in16k tap of rvcx_stream_last_taps returns what entered the ring, behind both. */
int rvcx_stream_open_fm(rvcx_ctx*, int model_id, const rvcx_stream_cfg*, const rvcx_stream_io*, const rvcx_fx_params* fx,
                        const rvcx_stream_dn* dn, const rvcx_stream_fm* fm, const rvcx_params* p, const int32_t* sid,
                        const float* pitch, int* stream_id);
/* new values for side 0 (input) or 1 (output) from the next step on; every value may change (geometry and delay depend on the
 * rate alone).  A refused value (a quefrency_ms outside the bound among them): -1, nothing changed.  Refused for a side that
 * was absent at open. */
int rvcx_stream_set_formant(rvcx_ctx*, int stream_id, int side, const rvcx_live_formant_params*);
/* device ms of the two sides in the last step ({input, output}; 0 for an absent side).  In rvcx_last_timing the input side is
 * counted in the "F0" interval, the output side in "SOLA + copies".  rvcx_stream_delays adds N of each present side. */
int rvcx_stream_last_fm_ms(rvcx_ctx*, int stream_id, float* ms2);
/* a side without a session and without a model: S mono rows of `frames` samples (x_hd: S x frames) at rate sr, cut into blocks
 * of block_frames 10 ms frames (frames must be a multiple of block_frames * sr / 100), through the same state and kernel code
 * a session runs per step; y_hd receives S x frames, delayed by N.  Optional taps for the T(frames) frames completed: E_hd and
 * g_hd (S, T, nb), s_hd (S, T) */
int rvcx_op_stream_formant(rvcx_ctx*, const float* x_hd, int S, int64_t frames, int sr, int block_frames,
                           const rvcx_live_formant_params*, float* y_hd, float* E_hd, float* g_hd, float* s_hd);
/* an op-level entry for verification, like the other rvcx_op_*: the same with a parameter history, as rvcx_stream_set_formant
 * writes one in a session, so that a session under set_formant can be held to the op bit for bit.  params[i] (n_params >= 1 of
 * them) is in force from block from_block[i] on; from_block[0] == 0, ascending.  An application has no use for it */
int rvcx_op_stream_formant_history(rvcx_ctx*, const float* x_hd, int S, int64_t frames, int sr, int block_frames, int n_params,
                                   const rvcx_live_formant_params* params, const int64_t* from_block, float* y_hd, float* E_hd,
                                   float* g_hd, float* s_hd);
/* host only, no context: stage 19 on the whole signal x[0 .. n) -> y (n samples, delayed by N).  Optional taps for the T(n)
 * frames: D (T, nb, 2) float32, E and g (T, nb), s (T) */
int rvcx_fx_formant_live_host(const float* x, int64_t n, int sr, const rvcx_live_formant_params*, float* y, float* D, float* E,
                              float* g, float* s);

/* ---- instrumentation ------------------------------------------------------------------- */
/* per-stage GPU milliseconds (HIP events on the library's stream) of the last
 * rvcx_convert_batch: {highpass, rmvpe, hubert, index, enc_p, flow, decoder, post, total}; of the last rvcx_stream_step:
 * {0, F0, HuBERT, blend + mix, enc_p, flow, decoder, SOLA + copies, total} -- a session's input resampler is counted in the
 * F0 interval, its output resampler in "SOLA + copies", and so are the input and the output side of stages 16 and 19; of the last
 * rvcx_fx_chain: {high-pass, compressor, gate, reverb, low
 * shelf, high shelf, chorus, copies + layout, total} (summed over the call's groups); of the last rvcx_fx_loudness: {copies +
 * layout, chunk states, carry, K-weighting + energy, hop sums + gates, true peak, copies back, 0, total}; of the last
 * rvcx_fx_master: {stem loudness, mix, mix loudness, scale + true peak, limiter gain, gain + int16, result meters, copies +
 * layout, total}; of the last rvcx_fx_stretch / rvcx_fx_pitch_shift: {copies + layout, transforms, owners, scan, inverse
 * transforms, overlap-add, resampler, layout + copies back, total} (all zero when stage 14 was skipped); of the last
 * rvcx_fx_denoise: {copies in + layout, analysis, smoothing, statistics (mode 0) or floor + mask (mode 1), mask (mode 0),
 * synthesis, overlap-add, copies back, total} (all zero when stage 15 was skipped); of the last rvcx_fx_formant /
 * rvcx_fx_pitch_shift_formant: {copies in + layout, frames, overlap-add, copies back, 0, 0, 0, stage 14 (stage 18 only), total}
 * (all zero when everything was skipped) */
int rvcx_last_timing(rvcx_ctx*, float* ms9);
/* HIP-event profile of the MFMA conv kernel family: begin=1 starts recording an event pair around
 * every conv launch on the library stream; begin=0 stops and returns, per tile configuration
 * (kind: -1 generic strided kernel, halo*10 for the stride-1
 * family, 100000/100001 its Linear variants), the launch count, algorithmic FLOPs (2*M*N*K of the unpadded problem) and the
 * summed kernel milliseconds, plus the tile shape (bm x bn).
 * The profile is PROCESS-wide: the two hooks serialise against each other, but launches of any other context of the
 * process that run while a profile is open are recorded into it -- profile with one context active. */
int rvcx_conv_profile(rvcx_ctx*, int begin, int64_t* launches, double* flops, double* ms, int32_t* bm,
                      int32_t* bn, int32_t* kind, int cap);
/* per-launch table (CSV text: tile,B,cin,cout,k,stride,nout,gflop,ms,tflops) of the last profile */
const char* rvcx_conv_profile_csv(rvcx_ctx*);
/* name and memory size of GPU `device` (no context needed) -- what Config._configure_gpu reads through
 * torch.cuda.get_device_name / get_device_properties, rvc/infer/infer.py:49-63.  -1 without a visible device. */
int rvcx_device_info(int device, char* name, int name_cap, int64_t* total_bytes);
/* free / total bytes of the context's GPU (hipMemGetInfo): what is left for further voice models and indices */
int rvcx_mem_info(rvcx_ctx*, int64_t* free_bytes, int64_t* total_bytes);
/* calls this context repeated because a split-fp16 kernel met an activation beyond
 * fp16 range (|x| >= 6e4; attention K / V >= 234): the default kernels form fp32-grade products from fp16 hi/lo
 * halves, which have fp16's exponent range.  The repeat is automatic and transparent; this counter reports it. */
int64_t rvcx_fp32_reruns(rvcx_ctx*);
/* layers (and attention calls) pinned to the exact-fp32 kernels since their models were loaded: a split-fp16 kernel that
 * meets an activation beyond fp16 range stamps its layer; the entry point pins the first offender of the call (launch
 * order) for the life of the model and repeats the call once -- later requests pay nothing. */
int64_t rvcx_fp32_layers(rvcx_ctx*);
/* which ones: one text line per layer the range guard pinned at run time since its model was loaded ("voice model 0: layer
 * 17 of 142 (conv 128 <- 128 x 7)"), in the order they were pinned; returns the length of the full text (buf receives at
 * most cap - 1 bytes + NUL).  Diagnostics for checkpoints with outlier channels; no reference counterpart. */
int rvcx_fp32_pinned(rvcx_ctx*, char* buf, int cap);
/* calls repeated with the single-workgroup BiGRU kernel because the cluster kernel's workgroups were not co-resident */
int64_t rvcx_gru_fallbacks(rvcx_ctx*);
/* the cluster BiGRU publishes h_t inside one XCD with a plain store and relies on the partners' sc1 polls seeing it (a
 * hardware observation, INTEGRATION.md "hardware assumptions").  The library checks that once per device when RMVPE is loaded
 * (or at the first BiGRU call); this runs the check if it has not run and reports it: 1 holds (plain publish in use), 0 does
 * not (the device uses the write-through publish), -1 undecided (no co-located pair ran side by side), -2 error. */
int rvcx_gru_publish_probe(rvcx_ctx*);
/* retrieval: queries whose 8 neighbours could not be certified from the split-fp16 pre-filter and were searched
 * exhaustively instead (csrc/index.hip) since the last call of this function; waits for the device.  -1: no index */
int64_t rvcx_index_exhaustive(rvcx_ctx*);

/* ---- index building ("train index" of the RVC UIs; csrc/kmeans.hip) --------------------------------------------------------
 * The reference ships no index trainer: the UIs call faiss (IVF{n},Flat trained on the stacked HuBERT features) and, above
 * 200 000 rows, scikit-learn's MiniBatchKMeans first.  Neither is restated here (parity with their clustering is unpinned);
 * the stages are DEFINED below and checked against a float64 restatement (tests/kmeans_reference.py).
 *
 * rvcx_kmeans: `iters` >= 1 Lloyd iterations on x (n, dim) from C_0 = init (k, dim).  Iteration i:
 *  - assign.  a_i[r] = the centroid c with the smallest EXACT fp32 pair distance e(x, c) = |c|^2 - 2 dot(x, c); ties go to
 *    the smaller id.  One fp32 routine computes e for a pair, whatever path reached the pair (kmeans.hip: pair_dot; its
 *    error is below 2^-18 (|x||c| + |c|^2)).  The split-fp16 GEMM pre-filters: the pick of a row is used only when it is
 *    certified against the filter's error bound; other rows -- and rows or centroids with values beyond fp16 range -- are
 *    scanned over all k centroids.  The result does not depend on the filter, the tiling or the row chunks:
 *    RVCX_KMEANS_PREFILTER=0 (read once per process; every row takes the scan) gives the same bits.
 *  - objective[i] = sum_r (|x_r|^2 + e(x_r, C_i[a_i[r]])), |x|^2 and the sum in double in a fixed order.
 *  - update.  C_{i+1}[c] = the mean of c's members, added in double in ascending row order, rounded once to float32; no
 *    floating-point atomics, the same bits in every run.  A cluster without members keeps its centroid for the next step.
 *  - empty clusters, after the update, in ascending id: an empty c takes the centroid of the cluster j that is largest by the
 *    running counts (ties: smaller id); float32 products: c's even dimensions x (1 + 2^-10), odd x (1 - 2^-10), j's the other
 *    way round; for the remaining empties c then counts count[j] / 2 (integer division) and j the rest.  splits[i] = the
 *    number of clusters treated.
 * Outputs: centroids = C_iters (k, dim); assign = a_{iters-1} (n); counts = the histogram of assign (k), before any split
 * bookkeeping; objective, splits: `iters` values each in HOST memory.  Every output pointer may be NULL.
 * Refused: k > n, k < 1, iters < 1, dim % 16 != 0, dim > 1024 (the limit of csrc/index.hip), n >= 2^31. */
int rvcx_kmeans(rvcx_ctx*, const float* x_hd, int64_t n, int dim, const float* init_hd, int k, int iters,
                float* centroids_hd, int32_t* assign_hd, int32_t* counts_hd, double* objective, int32_t* splits);
/* the inverted list of every stored row of an IVF{nlist},Flat index: the search's own coarse quantiser (rvcx_index_blend on an
 * IVF index: nearest centroid by |q|^2 + |c|^2 - 2 q.c on exact-fp32 dots, the first minimum on ties), so a stored vector
 * used as a query probes the list it was filed under -- outside fp32 rounding of the coarse distance: the fp32 dots of a chunk
 * of thousands of rows and of a few queries may be summed in another order (tile and split-K follow the row count), so two
 * centroids closer than that rounding can change places.  Refused: dim > 1024, nlist < 1, n < 1 */
int rvcx_ivf_assign(rvcx_ctx*, const float* x_hd, int64_t n, int dim, const float* centroids_hd, int nlist,
                    int32_t* assign_hd);
/* the rows an index is built from: what VC.vc hands the retrieval blend (pipeline.py:228-236) for B clips of n samples --
 * out_dim = the HuBERT's embed_dim: the output of layer 12 (RVC v2); out_dim = its final_proj width: final_proj of the
 * output of layer 9 (RVC v1).  feats (B, rvcx_hubert_frames(n), out_dim) */
int rvcx_index_features(rvcx_ctx*, int B, const float* wav_hd, int64_t n, int out_dim, float* feats_hd);
/* rows of the last rvcx_kmeans call (summed over its iterations) that took the exact scan; -1 without a context */
int64_t rvcx_kmeans_exhaustive(rvcx_ctx*);

/* DEBUG HOOKS -- rvcx_debug_inject, rvcx_bench_resblock_pair, rvcx_bench_conv1d, rvcx_bench_gemm, rvcx_conv_override are
 * process-wide tuning / fault-injection levers.  They return -2 ("refused") unless the process was started with
 * RVCX_DEBUG=1 in its environment (read once); the product path never calls them. */
/* test hook: what = 1 makes the next call behave as if the BiGRU cluster kernel had timed out; what = 3 makes the next BiGRU
 * cluster launch of the calling thread lose one workgroup, so that its partners really run into the device-side time-out
 * (~1.5 s) and the call is repeated on the single-workgroup kernel; what = 2 reads and clears the raw device error word */
int rvcx_debug_inject(rvcx_ctx*, int what);
/* algorithmic FLOPs issued by conv/GEMM/attention launches since the last reset */
double rvcx_flop_counter(rvcx_ctx*, int reset);
void* rvcx_stream(rvcx_ctx*); /* hipStream_t the library launches on */

/* ---- kernel-level entry points (unit parity tests of the HIP kernels) ------------------ */
/* FCPEF0Predictor.post_process()[0] (FCPE.py:841-867) + the tail of VC.get_f0 (pipeline.py:183-201) on a given raw
 * track: raw (F_in) Hz with 0 = unvoiced -> f0 (p_len, float32 of the float64 result) and coarse (p_len) */
int rvcx_op_fcpe_post(rvcx_ctx*, const float* raw_hd, int F_in, int p_len, double pitch, double f0_min, double f0_max,
                      int32_t* coarse, float* f0);
/* y = act(conv1d(pre(x), w) + bias) + res ; x (B,Cin,Tin) w (Cout,Cin/groups,K) host f32 */
int rvcx_op_conv1d(rvcx_ctx*, const float* x, const float* w, const float* bias, const float* res,
                   float* y, int B, int Cin, int Tin, int Cout, int K, int stride, int dil,
                   int pad_left, int Tout, int groups, int pre_lrelu, float pre_slope, int act,
                   float act_slope, const int32_t* lens_in, const int32_t* lens_out);
/* one ResBlock1 step, y = x + c2(lrelu(c1(lrelu(x)) + b1)) + b2 -- rvc/lib/algorithm/residuals.py:45-53.
 * w1 / w2 (C, C, K); c1 has dilation dil, c2 dilation 1.  fused = 1: the single-kernel form (resblock.hip);
 * fused = 0: the two conv launches it replaces.  lens (B) optional per-item valid lengths. */
int rvcx_op_resblock_pair(rvcx_ctx*, const float* x, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* y, int B, int C, int T, int K, int dil, float slope, int fused,
                          const int32_t* lens);
/* a whole ResBlock1 with kernel size 3 -- three steps x = x + c2_s(lrelu(c1_s(lrelu(x)) + b1_s)) + b2_s, c1_s dilated by
 * dils[s] (1, 3, 5 in every RVC v2 decoder), rvc/lib/algorithm/residuals.py:15-62 -- in ONE kernel (csrc/resblock3.hip; C = 32 /
 * 64, T a multiple of 4).  w1 / w2 (3, C, C, 3), b1 / b2 (3, C) or NULL.  Bit-identical to three rvcx_op_resblock_pair calls. */
int rvcx_op_resblock3(rvcx_ctx*, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                      float* y, int B, int C, int T, const int32_t* dils, float slope, const int32_t* lens);
/* micro-benchmark of one ResBlock1 step on device-resident random data (fused kernel or the two launches) */
int rvcx_bench_resblock_pair(rvcx_ctx*, int B, int C, int T, int K, int dil, int fused, int iters,
                             float* ms_per_launch);
/* micro-benchmark of the conv kernel on device-resident random data: `iters` back-to-back launches of
 * y = conv1d(lrelu(x)) + bias + res, average milliseconds per launch (HIP events on the library stream) */
int rvcx_bench_conv1d(rvcx_ctx*, int B, int Cin, int Tin, int Cout, int K, int stride, int dil, int groups,
                      int iters, float* ms_per_launch);
/* tuning hook for the tile-selection sweeps (tools/sweep_tiles_1d.py, sweep_unet.py, bench_conv.py): force the conv_fast tile index, the
 * staging variant (ignored: the LDS-DMA variant was removed in round 2) and the split-K factor; -1 = heuristic.
 * Process-wide; never set by the product path. */
int rvcx_conv_override(int tile, int variant, int splitk);
/* test hook for stage 13: output frames per chunk of the scan and per segment, 0 = the default (refused like the hooks
 * above).  No length changes a bit of any result. */
int rvcx_fx_stretch_override(int chunk_frames, int segment_frames);
/* ConvTranspose1d: w (Cin,Cout,K), padding p; Tout = (Tin-1)*s - 2p + K */
int rvcx_op_convtranspose1d(rvcx_ctx*, const float* x, const float* w, const float* bias, float* y,
                            int B, int Cin, int Tin, int Cout, int K, int stride, int pad,
                            int pre_lrelu, float pre_slope);
/* Conv2d 3x3 pad 1 (+bias, act, res) on (B,Cin,H,W) */
int rvcx_op_conv2d3x3(rvcx_ctx*, const float* x, const float* w, const float* bias, const float* res,
                      float* y, int B, int Cin, int H, int W, int Cout, int act);
/* One ConvBlockRes of the F0 model's U-Net (RMVPE.py:140-175, BatchNorm already folded into w / b by the caller):
 * y = relu(conv3x3(relu(conv3x3(x, w1) + b1), w2) + b2) + (wsc ? conv1x1(x, wsc) + bsc : x), through the model's own block
 * path (split hand-off between the two convs on large maps).  rows (B ints or NULL): valid rows of each item -- the rows
 * below are zero in x and come back zero (what a shorter member of a ragged batch sees). */
int rvcx_op_convblock2d(rvcx_ctx*, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* wsc, const float* bsc, float* y, int B, int Cin, int Cout, int H, int W,
                        const int32_t* rows);
/* ConvTranspose2d 3x3 stride 2 pad 1 output_padding 1: (B,Cin,H,W) -> (B,Cout,2H,2W), w (Cin,Cout,3,3) */
int rvcx_op_convtranspose2d(rvcx_ctx*, const float* x, const float* w, const float* bias, float* y,
                            int B, int Cin, int H, int W, int Cout, int act);
/* softmax(q k^T [+ rel-pos bias]) v on (B, H*D, T) channel-first tensors; emb_rel_k/v (2w+1, D) or NULL */
int rvcx_op_attention(rvcx_ctx*, const float* q, const float* k, const float* v, float* out, int B,
                      int H, int D, int T, float scale, const float* emb_rel_k,
                      const float* emb_rel_v, int window, const int32_t* lens);
/* The time-major Linear kernel of the transformer sections (csrc/gemm.hip): x_cf (B, Cin, T) is turned into rows
 * r = b T + t (split form, or fp32 when exact_fp32), y = act(x W^T + bias) + res.  w (Cout, Cin); res_tm (B T, Cout) or
 * NULL; act as in rvcx_op_conv1d (0 none, 2 relu, 3 gelu).  Outputs, each (B T, Cout) unless noted: y_tm; y_cf
 * (B, Cout, T) or NULL; y_split = the split-form output decoded to fp32 (hi + lo) or NULL. */
int rvcx_op_gemm_tm(rvcx_ctx*, const float* x_cf, const float* w, const float* bias, const float* res_tm, int B, int T,
                    int Cin, int Cout, int act, int exact_fp32, float* y_tm, float* y_cf, float* y_split);
/* micro-benchmark of the time-major Linear kernel on device-resident random rows (split form in, fp32 rows out) */
int rvcx_bench_gemm(rvcx_ctx*, int64_t rows, int Cin, int Cout, int iters, float* ms_per_launch);
/* LayerNorm of time-major rows (rows, C): fp32 result and the decoded split-form result (NULL to skip) */
int rvcx_op_layernorm_tm(rvcx_ctx*, const float* x, const float* gamma, const float* beta, float* y, float* y_split,
                         int64_t rows, int C, float eps);
/* LayerNorm over channels of (B,C,T) */
int rvcx_op_layernorm_c(rvcx_ctx*, const float* x, const float* gamma, const float* beta, float* y,
                        int B, int C, int T, float eps);
/* GroupNorm(C, C) + GELU (erf) over time of x (B, C, T); lens (B) or NULL: statistics over an item's first lens[b] frames,
 * zeros behind them.  y (B, C, T).  stats (B, C, 2) = {mean, rstd} and y_split (B, C, T: the split-fp16 image the next
 * conv reads, decoded to fp32 = hi + lo / 256) come from the statistics + split-store pair; both or neither, C % 16 == 0. */
int rvcx_op_groupnorm_gelu(rvcx_ctx*, const float* x, const float* gamma, const float* beta, int B, int C, int T, float eps,
                           const int32_t* lens, float* y, float* stats, float* y_split);
/* HuBERT's first extractor layer: conv1d(wav (B, n), w (C, 1, K), stride, no bias) -> GroupNorm(C, C) -> GELU -> split image,
 * T0 = (n - K) / stride + 1 frames, lens (B) or NULL as above.  fused = 1: the form that never stores the fp32 map; fused = 0:
 * conv, statistics, split store.  stats (B, C, 2); y_split (B, C, T0) decoded; raw_split (B C T0 2 halves, or NULL): the
 * image's own bytes.  C % 16 == 0, K <= 16. */
int rvcx_op_hubert_conv0(rvcx_ctx*, const float* wav, const float* w, const float* gamma, const float* beta, int B, int C,
                         int n, int K, int stride, float eps, const int32_t* lens, int fused, float* stats, float* y_split,
                         uint16_t* raw_split);
/* NSF harmonic source: f0 (B, T) Hz, noise (B, T upp), lin_wb = {w, b} of the 1 -> 1 Linear -> har (B, T upp); frames behind
 * lens[b] (or NULL) are zero */
int rvcx_op_sine_source(rvcx_ctx*, const float* f0, const float* noise, const float* lin_wb, int B, int T, int upp, float sr,
                        const int32_t* lens, float* har);
/* n standard normal values: Philox4x32-10, counter (offset + i / 4, 0x52564358, 0), key = seed, Box-Muller on word pairs */
int rvcx_op_randn(rvcx_ctx*, int64_t n, uint64_t seed, uint64_t offset, float* out);
/* np.pad(x[b, :ns[b]], p, "reflect") for any p: x (B, n) -> y (B, n + 2 p), zeros behind ns[b] + 2 p; ns (B) or NULL */
int rvcx_op_reflect_pad(rvcx_ctx*, const float* x, int B, int n, int p, const int32_t* ns, float* y);
/* log(max(mel, 1e-5)) * bn[0] + bn[1]: mel (B, nmel, F) -> out (B, Tp, nmel + 2) with zero pad columns; item b has fs[b]
 * frames reflected up to tps[b] rows, zero rows behind them (fs / tps (B) or NULL: F / Tp) */
int rvcx_op_mel_post(rvcx_ctx*, const float* mel, int B, int nmel, int F, int Tp, const float* bn, const int32_t* fs,
                     const int32_t* tps, float* out);
/* salience (B, T, 360) in rows of ld floats -> f0 (B, T) Hz: local average of cents around the first maximum, 0 at or
 * below thred and outside [f0_min, f0_max] */
int rvcx_op_decode_f0(rvcx_ctx*, const float* sal, int B, int T, int ld, float thred, float f0_min, float f0_max, float* f0);
/* 2 x 2 average pool of row-padded planes (H, Wp), x_ps floats apart -> (H / 2, (Wp - 2) / 2 + 2), y_ps apart; x holds
 * planes * x_ps floats, y planes * y_ps (what the kernel leaves unwritten comes back NaN) */
int rvcx_op_avgpool2(rvcx_ctx*, const float* x, int planes, int H, int Wp, int64_t x_ps, int64_t y_ps, float* y);
/* row-padded (B, C, T, Wp) -> (B, C (Wp - 2), T) */
int rvcx_op_gru_input(rvcx_ctx*, const float* x, int B, int C, int T, int Wp, float* y);
/* nearest x2 upsampling of feats (C rows of ld_in floats, Th used) cropped to p_len, mixed with feats0 where pitchf < 1
 * (use_protect) -> out (C rows of ld_out floats; what the kernel leaves unwritten comes back NaN) */
int rvcx_op_upsample_protect(rvcx_ctx*, const float* feats, const float* feats0, const float* pitchf, int C, int Th, int p_len,
                             float protect, int use_protect, int ld_in, int ld_out, float* out);
/* bidirectional GRU: x (B,T,I) -> y (B,T,2H); weights in torch layout */
int rvcx_op_bigru(rvcx_ctx*, const float* x, const float* w_ih, const float* w_hh, const float* b_ih,
                  const float* b_hh, const float* w_ih_r, const float* w_hh_r, const float* b_ih_r,
                  const float* b_hh_r, float* y, int B, int T, int I, int H);
/* scipy.signal.filtfilt(bh, ah, x) of pipeline.py:19-22,329 (float64) */
int rvcx_op_highpass(rvcx_ctx*, const double* x, double* y, int64_t n);
/* The same filter on the host, serial in scipy's own operation order: bit for bit what scipy.signal.filtfilt returns.
 * The cut search of rvcx_convert_batch runs on it.  No GPU, no context; n > 18 samples; x and y may alias. */
int rvcx_highpass_exact(const double* x, double* y, int64_t n);

/* ---- FLAC on the host (csrc/flac.hip; no GPU, no context) -------------------------------------------------------
 * rvc/infer/infer.py:153 writes WAV bytes whatever the extension of output_path; the mirror writes a real FLAC stream when
 * the path ends in ".flac"  and reads FLAC input where soundfile (rvc/lib/my_utils.py:9) is absent.
 * Encoder: 16-bit PCM, interleaved, 1-8 channels, block size 4096, CONSTANT / VERBATIM / FIXED 0-4 + partitioned Rice,
 * STREAMINFO with MD5.  Decoder: the whole format (LPC, wasted bits, Rice2 / escape partitions, stereo decorrelation,
 * 4-32 bits), CRC-8 / CRC-16 / MD5 checked.  Errors: negative return, text via rvcx_flac_last_error (per thread). */
int64_t rvcx_flac_encode_bound(int64_t frames, int channels);
int64_t rvcx_flac_encode_s16(const int16_t* pcm, int64_t frames, int channels, int sample_rate, uint8_t* out, int64_t cap);
int rvcx_flac_info(const uint8_t* data, int64_t n, int64_t* frames, int32_t* channels, int32_t* sample_rate, int32_t* bits);
/* decoded samples, interleaved, right-justified at the stream's sample size; returns frames decoded */
int64_t rvcx_flac_decode_s32(const uint8_t* data, int64_t n, int32_t* out, int64_t cap_samples);
const char* rvcx_flac_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RVCX_H */
