// VC.pipeline orchestration (rvc/infer/pipeline.py:289-467).
#pragma once
#include <functional>
#include <memory>
#include "models.h"

namespace rvcx {

struct Geometry {
  long t_pad = 0, t_pad_tgt = 0, t_query = 0, t_center = 0, t_max = 0;
};
struct Chunk {
  long s, e;      // sample range of audio_pad handed to vc()
  long f0_off;    // first pitch frame
};

Geometry make_geometry(const rvcx_params& p, int tgt_sr);
std::vector<Chunk> plan_chunks(long n, const std::vector<long>& opt_ts, const Geometry& g);
long out_capacity(const SynthModel& m, long n, const rvcx_params& p);
long noise_len_for(const Ctx& c, const SynthModel& m, long n, const rvcx_params& p);

size_t highpass_ext_doubles(long n);   // scratch per signal the caller provides as `ext`
// B signals (element stride xs, 0 = n); y64 / y32 are written densely (B, n).  ns (device, B ints or null): item b holds
// ns[b] <= n samples -- it is filtered as a signal of exactly that length, the rest of its output row is zero
void launch_highpass(const float* x32, const double* x64, double* ext, double* y64, float* y32, long n,
                     hipStream_t s, int B = 1, long xs = 0, const int* ns = nullptr);
// scipy.signal.filtfilt(BH, AH, x) on the host, serial and bit for bit (n > 18; x and y may alias)
void highpass_exact_host(const double* x, long n, double* y);
// VC.pipeline's opt_ts (pipeline.py:329-344) of an n-sample clip (float32 input: its float64 values), from
// highpass_exact_host's arithmetic: cut_count(n) values
template <typename T>
std::vector<long> exact_cut_points(const T* x, long n, const Geometry& g);

// one utterance of a rvcx_convert_batch call.  wav / wav64 / noise / out / out_f32 may be host or device memory.
struct UttIO {
  const float* wav = nullptr;      // 16 kHz mono float32 ...
  const double* wav64 = nullptr;   // ... or float64 (what load_audio returns in the reference, my_utils.py:16)
  long n = 0;
  const float* noise = nullptr;    // packed parity noise (rvcx_noise_len floats) or null (Philox)
  short* out = nullptr;            // capacity out_capacity()
  float* out_f32 = nullptr;        // optional, same capacity
  long out_n = 0;                  // produced samples (result)
  int seed_offset = 0;             // Philox stream of this utterance = params.seed + seed_offset
  const float* inp_f0 = nullptr;   // f0 file table, rows of (time [s], f0 [Hz]) float32 in HOST memory (pipeline.py:349-360)
  int inp_f0_rows = 0;
  const float* crepe_dither = nullptr;   // "mangio-crepe": per-frame dither in HOST memory or null (rvcx_utt_extra)
  long crepe_dither_n = 0;
};
// per batch item of get_f0_device: the crepe dither (host) and the item's Philox stream offset
struct F0Extra {
  const float* dither = nullptr;
  long dither_n = 0;
  int seed_offset = 0;
};
// what get_f0_device takes beyond VC.get_f0's own arguments (all optional)
struct F0Opts {
  long frames = 0;                              // frames written per item; 0: n / 160
  const float* pitch = nullptr;                 // host, B: a semitone shift per item instead of params.pitch
  const std::vector<double>* track = nullptr;   // f0-file track (f0_file_track), applied to every item
  const F0Extra* extra = nullptr;               // B
  const int* ns_host = nullptr;                 // B, rmvpe / crepe: ragged batch -- item b holds ns_host[b] <= n samples in its row
  const std::function<void()>* mid = nullptr;   // called once the model's first launches are enqueued
};
// A conversion in two halves.  convert_enqueue plans the call and enqueues ALL of its device work; convert_finish runs once
// the device has completed it and resolves the stage times.  convert_batch (the synchronous call) is one after the other
// with the stream synchronisations in between; a ticket (rvcx_convert_submit) returns to its caller between the two.
struct ConvertState;      // what the enqueue half leaves for the finish half (pipeline.hip)
struct ConvertStateDeleter {
  void operator()(ConvertState*) const;
};
using ConvertStatePtr = std::unique_ptr<ConvertState, ConvertStateDeleter>;
// The ticket a conversion is enqueued for.  Its ticket-long buffers and front sets come from Ctx::slot[slot].arena (the
// main arena keeps the work area only, reused from ticket to ticket in stream order), outputs bound for plain host memory
// leave into the slot's pinned staging (`staged`: copied to the caller's buffers once the device is done -- an
// asynchronous copy into pageable memory would hold the enqueueing thread until the ticket has finished), ev_first /
// ev_done bracket the ticket on the device, and nothing in the enqueue half waits for the device except `drain`.
struct TicketIO {
  int slot = 0;
  hipEvent_t ev_first = nullptr;    // front stream, ahead of the ticket's first front-end work
  hipEvent_t ev_done = nullptr;     // main stream, behind its last copy
  bool beside_predecessor = false;  // another ticket is in flight: this front end runs beside that ticket's decoder
  std::function<void()> drain;      // completes every ticket in flight; called before memory they may use is freed or moved
  struct Staged {
    void* dst;
    size_t off, bytes;              // offset into the slot's staging
  };
  std::vector<Staged> staged;
};
ConvertStatePtr convert_enqueue(Ctx& c, int model_id, std::vector<UttIO>& utts, const rvcx_params& p, bool timing,
                                TicketIO* ticket /*null: a synchronous call*/);
void convert_finish(Ctx& c, ConvertState& st, float* stage_ms /*9 or null*/);
// the micro-batch sizes and cut points of the conversion (what rvcx_last_micro_batches / rvcx_last_cuts report)
const std::vector<int>& convert_state_mbs(const ConvertState& st);
const std::vector<std::vector<long>>& convert_state_cuts(const ConvertState& st);
// VC.pipeline for a list of utterances: equal-length utterances run as micro-batches (B > 1 through every network).
void convert_batch(Ctx& c, int model_id, std::vector<UttIO>& utts, const rvcx_params& p, float* stage_ms /*9 or null*/);
int convert_micro_batch(Ctx& c, int model_id, long n, const rvcx_params& p);   // utterances per micro-batch at this length
size_t arena_budget(Ctx& c);   // activation bytes the context may plan with (probed once per context state, on its own device)

// F0 back-end selected by params.f0_method: throws unless its model is resident; workspace for B signals of n_pad samples
void check_f0_backend(const Ctx& c, const rvcx_params& p);
size_t f0_arena_bytes(const Ctx& c, const rvcx_params& p, int B, long n_pad);
int crepe_hop(const rvcx_params& p);
void crepe_f0_device(Ctx& c, const float* x, long n, const rvcx_params& p, long p_len, const F0Extra* ex, float* f0raw,
                     hipStream_t s);   // VC.get_f0_crepe for one padded signal on the device          // "mangio-crepe" frame step: params.hop_length, 128 when unset
// VC.get_f0 on device for B equal-length reflect-padded signals (B, n): coarse / f0 rows `stride` elements apart
void get_f0_device(Ctx& c, const float* x, int B, long n, const rvcx_params& p, int* coarse, float* f0, long stride,
                   hipStream_t s, const F0Opts& o = {});
// VC.vc's front for S items of one geometry: HuBERT -> retrieval blend -> upsample + protect mix into phone (S, E, T)
void vc_front(Ctx& c, int E, int S, const float* wav, long n, int Th, int T, const float* pitchf, float index_rate,
              float protect, float* phone, hipStream_t s, hipEvent_t after_hubert = nullptr);
int bucket_frames();                                                   // class width of the ragged micro-batches (frames)
long bucket_length(long n, const rvcx_params& p, const Geometry& g);   // length whose geometry an n-sample utterance runs with

}  // namespace rvcx
