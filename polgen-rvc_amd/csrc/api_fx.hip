// C ABI of librvcx.so (include/rvcx.h): post-production -- the effects chain, its stages one by one, the mix, the host twins.
#include "api_fx_common.h"

using namespace rvcx;
using namespace rvcx::api;

namespace rvcx {
namespace api {

// every refusal of a plan, before anything is written
void fx_validate(const char* who, const FxPlan& P) {
  if (!P.low_rate) check_rate(who, P.sr);
  else if (!fx_live_rate_ok(P.sr, true))         // a live session's board: the same text with its rider
    fail(std::string(who) + ": the sample rate must be a multiple of 100 Hz within 8000 .. 192000" +
         " (or 3200 .. 7900 for a reduced-size voice model)");
  check_channels(who, P.C);
  auto finite = [&](double v, const char* what) { check_finite(who, {v}, what); };   // the chain names the value
  if (P.hp) {
    finite(P.hp_fc, "fc");
    if (!(P.hp_fc > 0.0 && P.hp_fc < 0.5 * P.sr)) fail(std::string(who) + ": fc must lie inside (0, sr / 2)");
  }
  for (int k = 0; k < 2; ++k) {
    if (!(k ? P.gate : P.comp)) continue;
    const double ratio = k ? P.gate_ratio : P.comp_ratio, att = k ? P.gate_att : P.comp_att, rel = k ? P.gate_rel : P.comp_rel;
    finite(ratio, "ratio"), finite(k ? P.gate_thr_db : P.comp_thr_db, "threshold_db"), finite(att, "attack_ms"), finite(rel, "release_ms");
    if (ratio < 1.0) fail(std::string(who) + ": ratio must be >= 1");
    if (att < 0.0 || rel < 0.0) fail(std::string(who) + ": attack_ms and release_ms must be >= 0");
  }
  if (P.reverb) {
    if (P.C != 2) fail(std::string(who) + ": the reverb is stereo only (channels = 2)");
    finite(P.room, "room_size"), finite(P.damp, "damping"), finite(P.wet, "wet"), finite(P.dry, "dry"), finite(P.width, "width");
    if (0.28 * P.room + 0.7 >= 1.0 || 0.28 * P.room + 0.7 < 0.0) fail(std::string(who) + ": room_size outside [-2.5, 1.07): the combs would not decay");
    if (0.4 * P.damp < 0.0 || 0.4 * P.damp >= 1.0) fail(std::string(who) + ": damping outside [0, 2.5)");
  }
  for (int k = 0; k < 2; ++k) {
    if (!(k ? P.hi : P.lo)) continue;
    const double fc = k ? P.hi_fc : P.lo_fc, q = k ? P.hi_q : P.lo_q;
    finite(k ? P.hi_db : P.lo_db, "gain_db"), finite(fc, "fc"), finite(q, "Q");
    if (!(fc > 0.0 && fc < 0.5 * P.sr) || !(q > 0.0)) fail(std::string(who) + ": fc must lie inside (0, sr / 2) and Q be positive");
  }
  if (P.chorus) {
    finite(P.rate, "rate_hz"), finite(P.depth, "depth"), finite(P.centre, "centre_delay_ms"), finite(P.fb, "feedback"), finite(P.mix, "mix");
    if (std::fabs(P.fb) >= 1.0) fail(std::string(who) + ": |feedback| must be < 1");
    if (P.centre < 0.0 || P.centre + 10.0 * std::fabs(P.depth) > 1000.0) fail(std::string(who) + ": the chorus delay must stay inside 0 .. 1000 ms");
  }
}

FxPlan fx_board_plan(const char* who, const rvcx_fx_params& p, int sr, int channels, bool low_rate) {
  FxPlan P;
  P.sr = sr, P.C = channels, P.low_rate = low_rate;
  P.hp = true;
  P.comp_ratio = p.compressor_ratio, P.comp_thr_db = p.compressor_threshold, P.comp = true;
  P.gate_thr_db = p.noise_gate_threshold, P.gate_ratio = p.noise_gate_ratio, P.gate_att = p.noise_gate_attack;
  P.gate_rel = p.noise_gate_release, P.gate = true;
  P.reverb = true, P.room = p.reverb_rm_size, P.damp = p.reverb_damping, P.wet = p.reverb_wet, P.dry = p.reverb_dry;
  P.width = p.reverb_width;
  P.lo_db = p.low_shelf_gain, P.hi_db = p.high_shelf_gain, P.lo = P.hi = true;
  P.rate = p.chorus_rate_hz, P.depth = p.chorus_depth, P.centre = p.chorus_centre_delay_ms, P.fb = p.chorus_feedback;
  P.mix = p.chorus_mix, P.chorus = true;
  fx_validate(who, P);                  // with every stage on: a refused value is refused whether or not its stage would run
  P.comp = P.comp_ratio != 1.0, P.gate = P.gate_ratio != 1.0, P.lo = P.lo_db != 0.0, P.hi = P.hi_db != 0.0, P.chorus = P.mix != 0.0;
  return P;
}

}  // namespace api
}  // namespace rvcx

namespace {

size_t fx_item_bytes(const FxPlan& P, long ld) {
  const size_t nch = (size_t)(ld / kFxChunk);
  return (size_t)ld * 4 * ((size_t)P.C * 5 + (P.reverb ? 16 : 0)) + (size_t)P.C * nch * 4 * 7 + 4096;
}

// B items through the stages of P.  env (optional): per item the envelope of the LAST dynamics stage of the plan.
void fx_run(rvcx_ctx* h, Ctx* C, const char* who, int B, const float* const* x, const int64_t* n, const FxPlan& P,
            float* const* y, float* const* env) {
  check_items(who, B, x, n, y);
  fx_validate(who, P);
  const size_t worst = fx_item_bytes(P, fx_ld(*std::max_element(n, n + B)));
  const int G = fx_group_size(*C, B, worst, 0);
  Arena& A = C->arena;
  A.reset();
  A.reserve(worst * G + ((size_t)1 << 20));
  hipStream_t s = C->stream;
  FxTimer T(*C);
  int passes[3] = {0, 0, 0}, groups = 0;
  const int Cc = P.C;
  for (int g0 = 0; g0 < B; g0 += G, ++groups) {
    const int Bg = std::min(G, B - g0), R = Bg * Cc;
    const long ld = fx_ld(*std::max_element(n + g0, n + g0 + Bg));
    const size_t nch = (size_t)(ld / kFxChunk), plane = (size_t)R * ld;
    A.reset();
    float* stage = A.alloc<float>(plane);
    float* buf[4];
    for (float*& q : buf) q = A.alloc<float>(plane);
    float* combs = P.reverb ? A.alloc<float>((size_t)Bg * 16 * ld) : nullptr;
    float* scan = A.alloc<float>(4 * (size_t)R * nch);
    float* fstate = A.alloc<float>(3 * (size_t)R * nch + 64);
    const std::vector<int> len = row_lengths(n + g0, Bg, Cc);
    T.mark(0);
    const int* dlen = to_dev(*C, len.data(), len.size());
    RVCX_HIP(hipMemsetAsync(buf[0], 0, 4 * plane * sizeof(float), s));       // the four planes are one after the other
    float *cur = buf[0], *nxt = buf[1], *e1 = buf[2], *e2 = buf[3];
    const float* env_dev = nullptr;
    stage_in([&](int b) { return std::make_pair(x[g0 + b], n[g0 + b]); }, Bg, Cc, ld, stage, cur, dlen, s);
    T.mark(1);
    if (P.hp) {
      launch_fx_biquad(fx_coeffs(0, P.sr, P.hp_fc, 0.0, 0.0), cur, nxt, dlen, R, ld, scan, s);
      std::swap(cur, nxt);
    }
    T.mark(2);
    if (P.comp) {
      const int p = launch_fx_follower(cur, e2, dlen, len.data(), R, ld, 0, 0, fx_cte(P.comp_att, P.sr), fx_cte(P.comp_rel, P.sr),
                                       fstate, s);
      passes[0] = std::max(passes[0], p);
      launch_fx_gain(cur, e2, nxt, R, ld, 0, (float)std::pow(10.0, P.comp_thr_db / 20.0), (float)(1.0 / P.comp_ratio - 1.0), s);
      std::swap(cur, nxt);
      env_dev = e2;
    }
    T.mark(3);
    if (P.gate) {
      int p = launch_fx_follower(cur, e1, dlen, len.data(), R, ld, 1, 1, fx_cte(0.0, P.sr), fx_cte(50.0, P.sr), fstate, s);
      passes[1] = std::max(passes[1], p);
      p = launch_fx_follower(e1, e2, dlen, len.data(), R, ld, 0, 0, fx_cte(P.gate_att, P.sr), fx_cte(P.gate_rel, P.sr), fstate, s);
      passes[2] = std::max(passes[2], p);
      launch_fx_gain(cur, e2, nxt, R, ld, 1, (float)std::pow(10.0, P.gate_thr_db / 20.0), (float)(P.gate_ratio - 1.0), s);
      std::swap(cur, nxt);
      env_dev = e2;
    }
    T.mark(4);
    if (P.reverb) {
      launch_fx_reverb(fx_reverb_setup(P.sr, P.room, P.damp, P.wet, P.dry, P.width), cur, combs, e1, nxt, dlen, Bg, ld, s);
      std::swap(cur, nxt);
    }
    T.mark(5);
    if (P.lo) {
      launch_fx_biquad(fx_coeffs(1, P.sr, P.lo_fc, P.lo_q, P.lo_db), cur, nxt, dlen, R, ld, scan, s);
      std::swap(cur, nxt);
    }
    T.mark(6);
    if (P.hi) {
      launch_fx_biquad(fx_coeffs(2, P.sr, P.hi_fc, P.hi_q, P.hi_db), cur, nxt, dlen, R, ld, scan, s);
      std::swap(cur, nxt);
    }
    T.mark(7);
    if (P.chorus) {
      launch_fx_chorus(fx_chorus_setup(P.sr, P.rate, P.depth, P.centre, P.fb, P.mix), cur, e1, nxt, dlen, R, ld, s);
      std::swap(cur, nxt);
    }
    T.mark(8);
    stage_out(cur, dlen, Bg, Cc, ld, stage, s, [&](int b) { return std::make_pair(y[g0 + b], n[g0 + b]); });
    if (env && env_dev) stage_out(env_dev, dlen, Bg, Cc, ld, stage, s, [&](int b) { return std::make_pair(env[g0 + b], n[g0 + b]); });
    T.mark(9);
    RVCX_HIP(hipStreamSynchronize(s));
    // {the seven stages, copies + layout at either end, total}
    T.add_each(0, 1, 7), T.add(7, 0, 1), T.add(7, 8, 9), T.add(8, 0, 9);
  }
  A.reset();
  T.store(*C);
  std::copy(passes, passes + 3, h->fx_passes);
  h->fx_groups = groups;
}

void fx_host_args(const char* who, const void* x, int64_t n, const void* y) {
  if (!x || !y) fail(std::string(who) + ": null pointer");
  if (n < 0) fail(std::string(who) + ": n < 0");
}

}  // namespace

extern "C" {

int rvcx_fx_chain(rvcx_ctx* ctx, int B, const float* const* x, const int64_t* n, const rvcx_fx_params* p, float* const* y) {
  API_BEGIN(ctx)
  if (!p) fail("fx_chain: null parameters");
  const FxPlan P = fx_board_plan("fx_chain", *p, p->sample_rate, p->channels, false);
  fx_run(ctx, C, "fx_chain", B, x, n, P, y, nullptr);
  API_END
}

int rvcx_op_fx_highpass(rvcx_ctx* ctx, const float* x, int64_t n, int channels, int sr, float fc, float* y) {
  API_BEGIN(ctx)
  FxPlan P;
  P.sr = sr, P.C = channels, P.hp = true, P.hp_fc = fc;
  fx_run(ctx, C, "op_fx_highpass", 1, &x, &n, P, &y, nullptr);
  API_END
}

int rvcx_op_fx_compressor(rvcx_ctx* ctx, const float* x, int64_t n, int channels, int sr, float ratio, float threshold_db,
                          float attack_ms, float release_ms, float* y, float* env) {
  API_BEGIN(ctx)
  FxPlan P;
  P.sr = sr, P.C = channels, P.comp = true, P.comp_ratio = ratio, P.comp_thr_db = threshold_db, P.comp_att = attack_ms;
  P.comp_rel = release_ms;
  fx_validate("op_fx_compressor", P);
  P.comp = ratio != 1.f;
  fx_run(ctx, C, "op_fx_compressor", 1, &x, &n, P, &y, env ? &env : nullptr);
  API_END
}

int rvcx_op_fx_gate(rvcx_ctx* ctx, const float* x, int64_t n, int channels, int sr, float threshold_db, float ratio,
                    float attack_ms, float release_ms, float* y, float* env) {
  API_BEGIN(ctx)
  FxPlan P;
  P.sr = sr, P.C = channels, P.gate = true, P.gate_ratio = ratio, P.gate_thr_db = threshold_db, P.gate_att = attack_ms;
  P.gate_rel = release_ms;
  fx_validate("op_fx_gate", P);
  P.gate = ratio != 1.f;
  fx_run(ctx, C, "op_fx_gate", 1, &x, &n, P, &y, env ? &env : nullptr);
  API_END
}

int rvcx_op_fx_reverb(rvcx_ctx* ctx, const float* x, int64_t n, int channels, int sr, float room_size, float damping, float wet,
                      float dry, float width, float* y) {
  API_BEGIN(ctx)
  FxPlan P;
  P.sr = sr, P.C = channels, P.reverb = true, P.room = room_size, P.damp = damping, P.wet = wet, P.dry = dry, P.width = width;
  fx_run(ctx, C, "op_fx_reverb", 1, &x, &n, P, &y, nullptr);
  API_END
}

int rvcx_op_fx_shelf(rvcx_ctx* ctx, const float* x, int64_t n, int channels, int sr, int high, float gain_db, float fc, float Q,
                     float* y) {
  API_BEGIN(ctx)
  FxPlan P;
  P.sr = sr, P.C = channels;
  if (high) P.hi = true, P.hi_db = gain_db, P.hi_fc = fc, P.hi_q = Q;
  else P.lo = true, P.lo_db = gain_db, P.lo_fc = fc, P.lo_q = Q;
  fx_validate("op_fx_shelf", P);
  if (gain_db == 0.f) P.lo = P.hi = false;
  fx_run(ctx, C, "op_fx_shelf", 1, &x, &n, P, &y, nullptr);
  API_END
}

int rvcx_op_fx_chorus(rvcx_ctx* ctx, const float* x, int64_t n, int channels, int sr, float rate_hz, float depth,
                      float centre_delay_ms, float feedback, float mix, float* y) {
  API_BEGIN(ctx)
  FxPlan P;
  P.sr = sr, P.C = channels, P.chorus = true, P.rate = rate_hz, P.depth = depth, P.centre = centre_delay_ms, P.fb = feedback;
  P.mix = mix;
  fx_validate("op_fx_chorus", P);
  P.chorus = mix != 0.f;
  fx_run(ctx, C, "op_fx_chorus", 1, &x, &n, P, &y, nullptr);
  API_END
}

int rvcx_op_fx_mix(rvcx_ctx* ctx, const int16_t* vocal, int64_t n_v, const int16_t* inst, int64_t n_i, float vocal_gain_db,
                   float inst_gain_db, int16_t* out) {
  API_BEGIN(ctx)
  if (n_v < 0 || n_i < 0 || n_v > (int64_t)1 << 30 || n_i > (int64_t)1 << 30) fail("op_fx_mix: frame counts must lie in 0 .. 2^30");
  if ((n_v && (!vocal || !out)) || (n_i && !inst)) fail("op_fx_mix: null argument");
  check_finite("op_fx_mix", {vocal_gain_db, inst_gain_db}, "a gain");
  if (n_v == 0) return;
  const size_t nv = (size_t)n_v * 2, ni = (size_t)std::min(n_i, n_v) * 2;
  C->arena.reset();
  C->arena.reserve((2 * nv + ni) * 2 + (1 << 20));
  hipStream_t s = C->stream;
  int16_t* dv = to_dev(*C, vocal, nv);
  int16_t* di = ni ? to_dev(*C, inst, ni) : nullptr;
  int16_t* dout = C->arena.alloc<int16_t>(nv);
  launch_fx_mix(dv, (long)nv, di, (long)ni, std::pow(10.0, (double)vocal_gain_db / 20.0), std::pow(10.0, (double)inst_gain_db / 20.0),
                dout, s);
  RVCX_HIP(hipMemcpyAsync(out, dout, nv * 2, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  C->arena.reset();
  API_END
}

int rvcx_fx_chunk(void) { return kFxChunk; }

int rvcx_fx_last_passes(rvcx_ctx* ctx, int32_t* passes3) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  if (!ctx) return -1;
  if (passes3)
    for (int k = 0; k < 3; ++k) passes3[k] = ctx->fx_passes[k];
  return ctx->fx_groups;
}

// ---- host only ---------------------------------------------------------------------------------------------------------------
float rvcx_fx_cte(double ms, int sr) { return fx_cte(ms, sr); }
int rvcx_fx_delay(int sr, int D) { return fx_delay(sr, D); }

int rvcx_fx_coeffs(int kind, int sr, double fc, double Q, double gain_db, float* coef5) {
  return host_call([&] {
    if (!coef5) fail("fx_coeffs: null pointer");
    if (kind < 0 || kind > 2) fail("fx_coeffs: kind must be 0, 1 or 2");
    check_rate("fx_coeffs", sr);
    if (!(fc > 0.0 && fc < 0.5 * sr) || (kind && !(Q > 0.0)) || !std::isfinite(gain_db)) fail("fx_coeffs: fc inside (0, sr / 2), Q > 0, finite gain");
    const FxBiquad q = fx_coeffs(kind, sr, fc, Q, gain_db);
    coef5[0] = q.b0, coef5[1] = q.b1, coef5[2] = q.b2, coef5[3] = q.a1, coef5[4] = q.a2;
  });
}

int rvcx_fx_highpass_host(const float* x, int64_t n, int sr, float fc, float* y) {
  return host_call([&] {
    fx_host_args("fx_highpass_host", x, n, y);
    check_rate("fx_highpass_host", sr);
    if (!(fc > 0.f && fc < 0.5f * sr)) fail("fx_highpass_host: fc must lie inside (0, sr / 2)");
    fx_highpass_host(fx_coeffs(0, sr, fc, 0.0, 0.0), x, (long)n, y);
  });
}

int rvcx_fx_biquad_host(const float* x, int64_t n, const float* c, float* y) {
  return host_call([&] {
    fx_host_args("fx_biquad_host", x, n, y);
    if (!c) fail("fx_biquad_host: null coefficients");
    fx_biquad_host(FxBiquad{c[0], c[1], c[2], c[3], c[4]}, x, (long)n, y);
  });
}

int rvcx_fx_follower_host(const float* x, int64_t n, int square, int sqrt_out, float c_attack, float c_release, float* env) {
  return host_call([&] {
    fx_host_args("fx_follower_host", x, n, env);
    if (!(c_attack >= 0.f && c_attack < 1.f && c_release >= 0.f && c_release < 1.f)) fail("fx_follower_host: constants must lie in [0, 1)");
    fx_follower_host(x, (long)n, square, sqrt_out, c_attack, c_release, env);
  });
}

static void fx_dynamics_host(const char* who, int gate, const float* x, int64_t n, int sr, float ratio, float thr_db, float att,
                             float rel, float* y, float* env) {
  fx_host_args(who, x, n, y);
  FxPlan P;
  P.sr = sr, P.C = 1;
  if (gate) P.gate = true, P.gate_ratio = ratio, P.gate_thr_db = thr_db, P.gate_att = att, P.gate_rel = rel;
  else P.comp = true, P.comp_ratio = ratio, P.comp_thr_db = thr_db, P.comp_att = att, P.comp_rel = rel;
  fx_validate(who, P);
  if (ratio == 1.f) {                       // skip: the input, bit for bit
    if (y != x) std::copy(x, x + n, y);
    return;
  }
  std::vector<float> e((size_t)n), r;
  if (gate) {
    r.resize((size_t)n);
    fx_follower_host(x, (long)n, 1, 1, fx_cte(0.0, sr), fx_cte(50.0, sr), r.data());
    fx_follower_host(r.data(), (long)n, 0, 0, fx_cte(att, sr), fx_cte(rel, sr), e.data());
  } else {
    fx_follower_host(x, (long)n, 0, 0, fx_cte(att, sr), fx_cte(rel, sr), e.data());
  }
  const float thr = (float)std::pow(10.0, (double)thr_db / 20.0);
  fx_gain_host(x, e.data(), (long)n, gate, thr, gate ? (float)((double)ratio - 1.0) : (float)(1.0 / (double)ratio - 1.0), y);
  if (env) std::copy(e.begin(), e.end(), env);
}

int rvcx_fx_compressor_host(const float* x, int64_t n, int sr, float ratio, float threshold_db, float attack_ms,
                            float release_ms, float* y, float* env) {
  return host_call([&] { fx_dynamics_host("fx_compressor_host", 0, x, n, sr, ratio, threshold_db, attack_ms, release_ms, y, env); });
}

int rvcx_fx_gate_host(const float* x, int64_t n, int sr, float threshold_db, float ratio, float attack_ms, float release_ms,
                      float* y, float* env) {
  return host_call([&] { fx_dynamics_host("fx_gate_host", 1, x, n, sr, ratio, threshold_db, attack_ms, release_ms, y, env); });
}

int rvcx_fx_comb_host(const float* in, int64_t n, int D, float fb, float d, float* out) {
  return host_call([&] {
    fx_host_args("fx_comb_host", in, n, out);
    if (D < 1 || !(std::fabs(fb) < 1.f) || !(d >= 0.f && d < 1.f)) fail("fx_comb_host: D >= 1, |fb| < 1 and d in [0, 1)");
    fx_comb_host(in, (long)n, D, fb, d, out);
  });
}

int rvcx_fx_allpass_host(const float* in, int64_t n, int D, float* out) {
  return host_call([&] {
    fx_host_args("fx_allpass_host", in, n, out);
    if (D < 1) fail("fx_allpass_host: D >= 1");
    fx_allpass_host(in, (long)n, D, out);
  });
}

int rvcx_fx_chorus_host(const float* x, int64_t n, int sr, float rate_hz, float depth, float centre_delay_ms, float feedback,
                        float mix, float* y) {
  return host_call([&] {
    fx_host_args("fx_chorus_host", x, n, y);
    FxPlan P;
    P.sr = sr, P.C = 1, P.chorus = true, P.rate = rate_hz, P.depth = depth, P.centre = centre_delay_ms, P.fb = feedback, P.mix = mix;
    fx_validate("fx_chorus_host", P);
    if (mix == 0.f) {
      if (y != x) std::copy(x, x + n, y);
      return;
    }
    if (x == y) fail("fx_chorus_host: x and y must not alias");
    fx_chorus_host(fx_chorus_setup(sr, rate_hz, depth, centre_delay_ms, feedback, mix), x, (long)n, y);
  });
}

int rvcx_fx_mix_host(const int16_t* vocal, int64_t n_v, const int16_t* inst, int64_t n_i, float vocal_gain_db,
                     float inst_gain_db, int16_t* out) {
  return host_call([&] {
    if (n_v < 0 || n_i < 0) fail("fx_mix_host: negative frame count");
    if ((n_v && (!vocal || !out)) || (n_i && !inst)) fail("fx_mix_host: null pointer");
    check_finite("fx_mix_host", {vocal_gain_db, inst_gain_db}, "a gain");
    fx_mix_host(vocal, (long)n_v * 2, inst, (long)std::min(n_i, n_v) * 2, std::pow(10.0, (double)vocal_gain_db / 20.0),
                std::pow(10.0, (double)inst_gain_db / 20.0), out);
  });
}

}  // extern "C"
