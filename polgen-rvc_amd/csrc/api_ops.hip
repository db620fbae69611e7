// C ABI of librvcx.so (include/rvcx.h): kernel-level entry points of the tests and the tuning tools (rvcx_op_*, rvcx_bench_*).
#include "api_internal.h"
#include "h3_device.h"

using namespace rvcx;
using namespace rvcx::api;

// ------------------------------------------------------------------------------------------
// kernel-level entry points: host in, host out.  Weights are packed into the slab on each
// call (test-only path), activations live in the arena.
// ------------------------------------------------------------------------------------------
static void to_host(Ctx& c, float* h, const float* d, size_t n) {
  RVCX_HIP(hipMemcpyAsync(h, d, n * sizeof(float), hipMemcpyDeviceToHost, c.stream));
  RVCX_HIP(hipStreamSynchronize(c.stream));
}
// kernel-level entry points pack their weights into a region that lives for the call only
#define TEMP_REGION(C) WeightRegion tmp_region_; RegionScope tmp_scope_(*(C), tmp_region_)

extern "C" {

int rvcx_op_conv1d(rvcx_ctx* ctx, const float* x, const float* w, const float* bias, const float* res,
                   float* y, int B, int Cin, int Tin, int Cout, int K, int stride, int dil,
                   int pad_left, int Tout, int groups, int pre_lrelu, float pre_slope, int act,
                   float act_slope, const int32_t* lens_in, const int32_t* lens_out) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  size_t nx = (size_t)B * Cin * Tin, ny = (size_t)B * Cout * Tout;
  C->arena.reserve((nx + 2 * ny) * 4 + (64 << 20));
  C->arena.reset();
  ConvW L = make_conv(*C, w, bias, Cout, Cin / groups, K, groups, true);
  float* dx = to_dev(*C, x, nx);
  float* dy = C->arena.alloc<float>(ny);
  ConvArgs a = conv1d_args(L, dx, dy, B, Tin, Tout, stride, dil, pad_left);
  if (res) conv_set_res(a, to_dev(*C, res, ny), Cout, Tout);
  if (pre_lrelu) {
    a.pre_act = ACT_LRELU;
    a.pre_slope = pre_slope;
  }
  a.act = act;
  a.act_slope = act_slope;
  a.lens_in = (lens_in ? to_dev(*C, lens_in, B) : nullptr);
  a.lens_out = (lens_out ? to_dev(*C, lens_out, B) : nullptr);
  C->conv(a);
  to_host(*C, y, dy, ny);
  C->arena.reset();
  API_END
}

int rvcx_op_resblock_pair(rvcx_ctx* ctx, const float* x, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* y, int B, int Cc, int T, int K, int dil, float slope, int fused,
                          const int32_t* lens) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  const size_t n = (size_t)B * Cc * T;
  C->arena.reserve(n * 4 * 4 + (64 << 20));
  C->arena.reset();
  ConvW L1 = make_conv(*C, w1, b1, Cc, Cc, K, 1, true);
  ConvW L2 = make_conv(*C, w2, b2, Cc, Cc, K, 1, true);
  float* dx = to_dev(*C, x, n);
  float* dt = C->arena.alloc<float>(n);
  float* dy = C->arena.alloc<float>(n);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, n * 4, C->stream));      // NaN fill: every element must be written
  const int* dl = (lens ? to_dev(*C, lens, B) : nullptr);
  if (fused) {
    PairArgs pa;
    pa.x = dx;
    pa.y = dy;
    pa.w1 = (L1.w_h3 && *L1.h3_ok) ? L1.w_h3 : nullptr;
    pa.w2 = (L2.w_h3 && *L2.h3_ok) ? L2.w_h3 : nullptr;
    pa.b1 = L1.bias;
    pa.b2 = L2.bias;
    pa.lens = dl;
    pa.B = B;
    pa.C = Cc;
    pa.T = T;
    pa.bs = (long)Cc * T;
    pa.cs = T;
    pa.k = K;
    pa.dil = dil;
    pa.slope = slope;
    if (!resblock_pair_ok(pa) && !g_force_fp32) fail("resblock pair: shape not supported by the fused kernel");
  }
  if (fused && !g_force_fp32) {
    PairArgs pa;
    pa.x = dx;
    pa.y = dy;
    pa.w1 = L1.w_h3;
    pa.w2 = L2.w_h3;
    pa.b1 = L1.bias;
    pa.b2 = L2.bias;
    pa.lens = dl;
    pa.B = B;
    pa.C = Cc;
    pa.T = T;
    pa.bs = (long)Cc * T;
    pa.cs = T;
    pa.k = K;
    pa.dil = dil;
    pa.slope = slope;
    C->pair_on(pa, C->stream);
  } else {   // the two launches the fused kernel replaces (synth.hip's fallback path; also the exact-fp32 rerun)
    ConvArgs a = conv1d_args(L1, dx, dt, B, T, T, 1, dil, (K * dil - dil) / 2);
    a.pre_act = ACT_LRELU;
    a.pre_slope = slope;
    a.act = ACT_LRELU;
    a.act_slope = slope;
    a.lens_in = dl;
    a.lens_out = dl;
    ConvArgs a2 = conv1d_args(L2, dt, dy, B, T, T, 1, 1, (K - 1) / 2);
    const bool split = conv_h3_split_ok(a) && conv_h3_split_ok(a2);
    if (split) {
      a.y_split = dt;
      a.y = nullptr;
    }
    C->conv(a);
    if (split) a2.x_split = dt;
    conv_set_res(a2, dx, Cc, T);
    a2.lens_in = dl;
    a2.lens_out = dl;
    C->conv(a2);
  }
  to_host(*C, y, dy, n);
  C->arena.reset();
  API_END
}

int rvcx_op_resblock3(rvcx_ctx* ctx, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                      float* y, int B, int Cc, int T, const int32_t* dils, float slope, const int32_t* lens) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  const size_t n = (size_t)B * Cc * T, wn = (size_t)Cc * Cc * 3;
  C->arena.reserve(n * 4 * 3 + (64 << 20));
  C->arena.reset();
  ConvW L1[3], L2[3];
  for (int s = 0; s < 3; ++s) {
    L1[s] = make_conv(*C, w1 + s * wn, b1 ? b1 + (size_t)s * Cc : nullptr, Cc, Cc, 3, 1, true);
    L2[s] = make_conv(*C, w2 + s * wn, b2 ? b2 + (size_t)s * Cc : nullptr, Cc, Cc, 3, 1, true);
  }
  float* dx = to_dev(*C, x, n);
  float* dy = C->arena.alloc<float>(n);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, n * 4, C->stream));      // NaN fill: every element must be written
  const int* dl = (lens ? to_dev(*C, lens, B) : nullptr);
  Block3Args a;
  a.x = dx;
  a.y = dy;
  for (int s = 0; s < 3; ++s) {
    a.w1[s] = (L1[s].w_h3 && *L1[s].h3_ok) ? L1[s].w_h3 : nullptr;
    a.w2[s] = (L2[s].w_h3 && *L2[s].h3_ok) ? L2[s].w_h3 : nullptr;
    a.b1[s] = L1[s].bias;
    a.b2[s] = L2[s].bias;
    a.dil[s] = dils ? dils[s] : 2 * s + 1;       // NULL: ResBlock1's own dilations (1, 3, 5), residuals.py:15-62
  }
  a.ovf_layer = L1[0].ovf_word;
  a.lens = dl;
  a.B = B;
  a.C = Cc;
  a.T = T;
  a.bs = (long)Cc * T;
  a.cs = T;
  a.slope = slope;
  a.any_shape = true;
  if (!resblock3_ok(a)) fail("resblock3: shape not supported by the whole-block kernel");
  C->block3_on(a, C->stream);
  to_host(*C, y, dy, n);
  C->arena.reset();
  API_END
}

int rvcx_bench_resblock_pair(rvcx_ctx* ctx, int B, int Cc, int T, int K, int dil, int fused, int iters,
                             float* ms_per_launch) {
  REQUIRE_DEBUG(ctx, "rvcx_bench_resblock_pair")
  API_BEGIN(ctx)
  TEMP_REGION(C);
  const size_t n = (size_t)B * Cc * T;
  C->arena.reserve(n * 4 * 4 + (64 << 20));
  C->arena.reset();
  std::vector<float> w((size_t)Cc * Cc * K), bias((size_t)Cc, 0.1f);
  for (size_t i = 0; i < w.size(); ++i) w[i] = ((float)((i * 2654435761u) % 2001) / 1000.f - 1.f) / std::sqrt((float)Cc * K);
  ConvW L1 = make_conv(*C, w.data(), bias.data(), Cc, Cc, K, 1, true);
  ConvW L2 = make_conv(*C, w.data(), bias.data(), Cc, Cc, K, 1, true);
  float* dx = C->arena.alloc<float>(n);
  float* dt = C->arena.alloc<float>(n);
  float* dy = C->arena.alloc<float>(n);
  launch_randn(dx, n, 1, 0, C->stream);
  if (getenv("RVCX_BENCH_ZERO")) RVCX_HIP(hipMemsetAsync(dx, 0, n * 4, C->stream));   // power / clock experiments only
  PairArgs pa;
  pa.x = dx;
  pa.y = dy;
  pa.w1 = L1.w_h3;
  pa.w2 = L2.w_h3;
  pa.b1 = L1.bias;
  pa.b2 = L2.bias;
  pa.B = B;
  pa.C = Cc;
  pa.T = T;
  pa.bs = (long)Cc * T;
  pa.cs = T;
  pa.k = K;
  pa.dil = dil;
  ConvArgs a = conv1d_args(L1, dx, dt, B, T, T, 1, dil, (K * dil - dil) / 2);
  a.pre_act = ACT_LRELU;
  a.pre_slope = 0.1f;
  a.act = ACT_LRELU;
  a.act_slope = 0.1f;
  ConvArgs a2 = conv1d_args(L2, dt, dy, B, T, T, 1, 1, (K - 1) / 2);
  const bool split = conv_h3_split_ok(a) && conv_h3_split_ok(a2);
  if (split) {
    a.y_split = dt;
    a.y = nullptr;
    a2.x_split = dt;
  }
  conv_set_res(a2, dx, Cc, T);
  auto once = [&]() {
    if (fused) {
      C->pair_on(pa, C->stream);
    } else {
      C->conv(a);
      C->conv(a2);
    }
  };
  if (fused && !resblock_pair_ok(pa)) fail("resblock pair: shape not supported by the fused kernel");
  once();
  if (fused && getenv("RVCX_PAIR_TRACE")) {     // one traced launch: per-workgroup phase stamps -> CSV (tools/pair_trace.py)
    const size_t cap = (size_t)B * (T / 32 + 64) * 8;
    long long* tr = C->arena.alloc<long long>(cap);
    RVCX_HIP(hipMemsetAsync(tr, 0, cap * 8, C->stream));
    pa.trace = tr;
    once();
    pa.trace = nullptr;
    std::vector<long long> h(cap);
    RVCX_HIP(hipMemcpyAsync(h.data(), tr, cap * 8, hipMemcpyDeviceToHost, C->stream));
    RVCX_HIP(hipStreamSynchronize(C->stream));
    if (FILE* f = fopen(getenv("RVCX_PAIR_TRACE"), "a")) {
      fprintf(f, "# C %d T %d K %d dil %d\n", Cc, T, K, dil);
      for (size_t w = 0; w * 8 < cap; ++w)
        if (h[w * 8]) {
          for (int k = 0; k < 8; ++k) fprintf(f, "%lld%c", h[w * 8 + k], k == 7 ? '\n' : ',');
        }
      fclose(f);
    }
  }
  hipEvent_t e0, e1;
  RVCX_HIP(hipEventCreate(&e0));
  RVCX_HIP(hipEventCreate(&e1));
  RVCX_HIP(hipEventRecord(e0, C->stream));
  for (int i = 0; i < iters; ++i) once();
  RVCX_HIP(hipEventRecord(e1, C->stream));
  RVCX_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  RVCX_HIP(hipEventElapsedTime(&ms, e0, e1));
  *ms_per_launch = ms / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  C->arena.reset();
  API_END
}

int rvcx_conv_override(int tile, int variant, int splitk) {
  REQUIRE_DEBUG(nullptr, "rvcx_conv_override")
  rvcx::g_conv_override.tile = tile;
  rvcx::g_conv_override.variant = variant;
  rvcx::g_conv_override.splitk = splitk;
  return 0;
}

int rvcx_bench_conv1d(rvcx_ctx* ctx, int B, int Cin, int Tin, int Cout, int K, int stride, int dil, int groups,
                      int iters, float* ms_per_launch) {
  REQUIRE_DEBUG(ctx, "rvcx_bench_conv1d")
  API_BEGIN(ctx)
  TEMP_REGION(C);
  const int pad = (K * dil - dil) / 2;
  const int Tout = (Tin + 2 * pad - dil * (K - 1) - 1) / stride + 1;
  size_t nx = (size_t)B * Cin * Tin, ny = (size_t)B * Cout * Tout;
  C->arena.reserve((nx + 2 * ny) * 4 + (64 << 20));
  C->arena.reset();
  std::vector<float> w((size_t)Cout * (Cin / groups) * K), bias((size_t)Cout, 0.1f);
  for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((i * 2654435761u) % 2001) / 1000.f - 1.f;
  ConvW L = make_conv(*C, w.data(), bias.data(), Cout, Cin / groups, K, groups, true);
  float* dx = C->arena.alloc<float>(nx);
  float* dy = C->arena.alloc<float>(ny);
  float* dr = C->arena.alloc<float>(ny);
  launch_randn(dx, nx, 1, 0, C->stream);
  launch_randn(dr, ny, 2, 0, C->stream);
  ConvArgs a = conv1d_args(L, dx, dy, B, Tin, Tout, stride, dil, pad);
  conv_set_res(a, dr, Cout, Tout);
  a.pre_act = ACT_LRELU;
  a.pre_slope = 0.1f;
  C->conv(a);
  long long* dtrace = nullptr;
  const long ntrace = 1L << 16;
  if (getenv("RVCX_TRACE")) {
    RVCX_HIP(hipMalloc(&dtrace, ntrace * 6 * sizeof(long long)));
    RVCX_HIP(hipMemset(dtrace, 0, ntrace * 6 * sizeof(long long)));
    a.trace = dtrace;
  }
  hipEvent_t e0, e1;
  RVCX_HIP(hipEventCreate(&e0));
  RVCX_HIP(hipEventCreate(&e1));
  RVCX_HIP(hipEventRecord(e0, C->stream));
  for (int i = 0; i < iters; ++i) C->conv(a);
  RVCX_HIP(hipEventRecord(e1, C->stream));
  RVCX_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  RVCX_HIP(hipEventElapsedTime(&ms, e0, e1));
  *ms_per_launch = ms / iters;
  if (dtrace) {
    std::vector<long long> ht((size_t)ntrace * 6);
    RVCX_HIP(hipMemcpy(ht.data(), dtrace, ht.size() * sizeof(long long), hipMemcpyDeviceToHost));
    FILE* f = fopen(getenv("RVCX_TRACE"), "w");
    for (long i = 0; i < ntrace; ++i)
      if (ht[i * 6 + 5]) fprintf(f, "%ld,%lld,%lld,%lld,%lld,%lld,%lld\n", i, ht[i*6], ht[i*6+1], ht[i*6+2], ht[i*6+3], ht[i*6+4], ht[i*6+5]);
    fclose(f);
    (void)hipFree(dtrace);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  C->arena.reset();
  API_END
}

int rvcx_op_convtranspose1d(rvcx_ctx* ctx, const float* x, const float* w, const float* bias, float* y,
                            int B, int Cin, int Tin, int Cout, int K, int stride, int pad,
                            int pre_lrelu, float pre_slope) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  const int Tout = (Tin - 1) * stride - 2 * pad + K;
  size_t nx = (size_t)B * Cin * Tin, ny = (size_t)B * Cout * Tout;
  C->arena.reserve((nx + ny) * 4 + (64 << 20));
  C->arena.reset();
  ConvT1dW L = make_convT1d(*C, w, bias, Cin, Cout, K, stride, pad);
  float* dx = to_dev(*C, x, nx);
  float* dy = C->arena.alloc<float>(ny);
  ConvArgs a = convT1d_args(L, dx, dy, B, Tin, Tout);
  if (pre_lrelu) {
    a.pre_act = ACT_LRELU;
    a.pre_slope = pre_slope;
  }
  C->conv(a);
  to_host(*C, y, dy, ny);
  C->arena.reset();
  API_END
}

// host helpers: dense (B,C,H,W) <-> row-padded (B,C,H,W+2)
static std::vector<float> pad_rows(const float* x, size_t planes, int H, int W) {
  const int Wp = W + 2;
  std::vector<float> o(planes * H * Wp, 0.f);
  for (size_t p = 0; p < planes; ++p)
    for (int h = 0; h < H; ++h)
      std::memcpy(&o[(p * H + h) * Wp + 1], &x[(p * H + h) * W], (size_t)W * 4);
  return o;
}
static void unpad_rows(const std::vector<float>& xp, float* y, size_t planes, int H, int W) {
  const int Wp = W + 2;
  for (size_t p = 0; p < planes; ++p)
    for (int h = 0; h < H; ++h)
      std::memcpy(&y[(p * H + h) * W], &xp[(p * H + h) * Wp + 1], (size_t)W * 4);
}

int rvcx_op_conv2d3x3(rvcx_ctx* ctx, const float* x, const float* w, const float* bias, const float* res,
                      float* y, int B, int Cin, int H, int W, int Cout, int act) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  const int Wp = W + 2;
  size_t nx = (size_t)B * Cin * H * Wp, ny = (size_t)B * Cout * H * Wp;
  C->arena.reserve((nx + 2 * ny) * 4 + (64 << 20));
  C->arena.reset();
  ConvW L = make_conv(*C, w, bias, Cout, Cin, 9, 1);
  std::vector<float> xp = pad_rows(x, (size_t)B * Cin, H, W);
  float* dx = to_dev(*C, xp.data(), nx);
  float* dy = C->arena.alloc<float>(ny);
  ConvArgs a = conv2d_args(L, dx, dy, B, H, Wp);
  std::vector<float> rp;
  if (res) {
    rp = pad_rows(res, (size_t)B * Cout, H, W);
    conv_set_res(a, to_dev(*C, rp.data(), ny), Cout, H * Wp);
  }
  a.act = act;
  C->conv(a);
  std::vector<float> yp(ny);
  to_host(*C, yp.data(), dy, ny);
  // the kernel must keep the pad columns at exactly zero
  for (size_t r = 0; r < (size_t)B * Cout * H; ++r)
    if (yp[r * Wp] != 0.f || yp[r * Wp + Wp - 1] != 0.f) fail("conv2d: pad column not zero");
  unpad_rows(yp, y, (size_t)B * Cout, H, W);
  C->arena.reset();
  API_END
}

int rvcx_op_convblock2d(rvcx_ctx* ctx, const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* wsc, const float* bsc, float* y, int B, int Cin, int Cout, int H, int W,
                        const int32_t* rows) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  RVCX_CHECK(wsc || Cin == Cout, "op_convblock2d: Cin != Cout needs the 1x1 shortcut");
  const int Wp = W + 2;
  const size_t nx = (size_t)B * Cin * H * Wp, ny = (size_t)B * Cout * H * Wp;
  C->arena.reserve((nx + 3 * ny) * 4 + (64 << 20));
  C->arena.reset();
  ConvW c1 = make_conv(*C, w1, b1, Cout, Cin, 9, 1), c2 = make_conv(*C, w2, b2, Cout, Cout, 9, 1), sc;
  if (wsc) sc = make_conv(*C, wsc, bsc, Cout, Cin, 1, 1);
  std::vector<float> xp = pad_rows(x, (size_t)B * Cin, H, W);
  if (rows)                                       // what the model guarantees: nothing but zeros below an item's last row
    for (int b = 0; b < B; ++b) {
      RVCX_CHECK(rows[b] >= 0 && rows[b] <= H, "op_convblock2d: rows outside [0, H]");
      for (int c = 0; c < Cin; ++c)
        std::fill(xp.begin() + (((size_t)b * Cin + c) * H + rows[b]) * Wp, xp.begin() + (((size_t)b * Cin + c) + 1) * H * Wp, 0.f);
    }
  float* dx = to_dev(*C, xp.data(), nx);
  float* dy = C->arena.alloc<float>(ny);
  float* t1 = C->arena.alloc<float>(ny);
  float* t2 = C->arena.alloc<float>(ny);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, ny * 4, C->stream));  // NaN fill: every element must be written
  RVCX_HIP(hipMemsetAsync(t1, 0xff, ny * 4, C->stream));
  rvcx::rmvpe_block_op(*C, c1, c2, wsc ? &sc : nullptr, dx, dy, t1, t2, B, H, Wp, rows, C->stream);
  std::vector<float> yp(ny);
  to_host(*C, yp.data(), dy, ny);
  for (size_t r = 0; r < (size_t)B * Cout * H; ++r)
    if (yp[r * Wp] != 0.f || yp[r * Wp + Wp - 1] != 0.f) fail("convblock2d: pad column not zero");
  unpad_rows(yp, y, (size_t)B * Cout, H, W);
  C->arena.reset();
  API_END
}

int rvcx_op_convtranspose2d(rvcx_ctx* ctx, const float* x, const float* w, const float* bias, float* y,
                            int B, int Cin, int H, int W, int Cout, int act) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  const int Wp = W + 2, Wpo = 2 * W + 2;
  size_t nx = (size_t)B * Cin * H * Wp, ny = (size_t)B * Cout * 2 * H * Wpo;
  C->arena.reserve((nx + ny) * 4 + (64 << 20));
  C->arena.reset();
  ConvT2dW L = make_convT2d(*C, w, nullptr, bias, Cin, Cout);
  std::vector<float> xp = pad_rows(x, (size_t)B * Cin, H, W);
  float* dx = to_dev(*C, xp.data(), nx);
  float* dy = C->arena.alloc<float>(ny);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, ny * 4, C->stream));  // NaN fill: every element must be written
  ConvArgs a = convT2d_args(L, dx, dy, B, H, Wp);
  a.act = act;
  C->conv(a);
  std::vector<float> yp(ny);
  to_host(*C, yp.data(), dy, ny);
  for (size_t r = 0; r < (size_t)B * Cout * 2 * H; ++r)
    if (yp[r * Wpo] != 0.f || yp[r * Wpo + Wpo - 1] != 0.f) fail("convT2d: pad column not zero");
  unpad_rows(yp, y, (size_t)B * Cout, 2 * H, 2 * W);
  C->arena.reset();
  API_END
}

int rvcx_op_attention(rvcx_ctx* ctx, const float* q, const float* k, const float* v, float* out, int B, int H,
                      int D, int T, float scale, const float* emb_rel_k, const float* emb_rel_v, int window,
                      const int32_t* lens) {
  API_BEGIN(ctx)
  const size_t n = (size_t)B * H * D * T;
  C->arena.reserve(n * 16 + (attention_scratch_floats(B, H, T, window) + attention_split_floats(B, H, T)) * 4 + (64 << 20));
  C->arena.reset();
  float *dq = to_dev(*C, q, n), *dk = to_dev(*C, k, n), *dv = to_dev(*C, v, n);
  float* dout = C->arena.alloc<float>(n);
  float *ek = nullptr, *ev = nullptr, *scratch = nullptr;
  if (emb_rel_k) {
    ek = to_dev(*C, emb_rel_k, (size_t)(2 * window + 1) * D);
    ev = to_dev(*C, emb_rel_v, (size_t)(2 * window + 1) * D);
    scratch = C->arena.alloc<float>(attention_scratch_floats(B, H, T, window));
  }
  launch_attention(dq, dk, dv, dout, B, H, D, T, T, (long)H * D * T, (long)H * D * T, scale, ek, ev, window,
                   (lens ? to_dev(*C, lens, B) : nullptr), scratch, C->arena.alloc<float>(attention_split_floats(B, H, T)), C->stream);
  to_host(*C, out, dout, n);
  C->arena.reset();
  API_END
}

// host view of split rows: hi + (S lo) / S
static void decode_xs(const std::vector<uint16_t>& raw, long rows, int Cc, float* out) {
  for (long r = 0; r < rows; ++r)
    for (int c = 0; c < Cc; ++c) {
      const size_t e = ((size_t)r * Cc * 2) + (size_t)(c >> 4) * 32 + ((c >> 3) & 1) * 8 + (c & 7);
      out[(size_t)r * Cc + c] = half_to_float(raw[e]) + half_to_float(raw[e + 16]) / 256.f;
    }
}

// host view of a channel-first split image (ops.hip, groupnorm_gelu_split_kernel): per item XS[c/16][op][(c%16)/8][t][8]
// halves, op 0 = hi, op 1 = lo * kH3Scale (h3_device.h)
static void decode_split_cf(const std::vector<uint16_t>& raw, int B, int Cc, int T, float* out) {
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < Cc; ++c)
      for (int t = 0; t < T; ++t) {
        const size_t item = (size_t)b * Cc * T * 2;
        const size_t hi = item + ((size_t)(((c >> 4) * 2 + 0) * 2 + ((c >> 3) & 1)) * T + t) * 8 + (c & 7);
        const size_t lo = item + ((size_t)(((c >> 4) * 2 + 1) * 2 + ((c >> 3) & 1)) * T + t) * 8 + (c & 7);
        out[((size_t)b * Cc + c) * T + t] = half_to_float(raw[hi]) + half_to_float(raw[lo]) / kH3Scale;
      }
}

int rvcx_op_gemm_tm(rvcx_ctx* ctx, const float* x_cf, const float* w, const float* bias, const float* res_tm, int B,
                    int T, int Cin, int Cout, int act, int exact_fp32, float* y_tm, float* y_cf, float* y_split) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  const long R = (long)B * T;
  C->arena.reserve(((size_t)R * (3 * (size_t)Cin + 4 * (size_t)Cout)) * 4 + (64 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  ConvW L = make_conv(*C, w, bias, Cout, Cin, 1, 1, true);
  float* dx = to_dev(*C, x_cf, (size_t)R * Cin);
  float* xf = C->arena.alloc<float>((size_t)R * Cin);
  float* xs = C->arena.alloc<float>((size_t)R * L.cin_gp);
  RVCX_HIP(hipMemsetAsync(xs, 0, (size_t)R * L.cin_gp * 4, s));
  const bool h3 = !exact_fp32 && conv_h3_ok(L) && gemm_h3_enabled() && Cin % 4 == 0;
  launch_cf_to_tm(dx, (long)Cin * T, xf, Cin, h3 ? xs : nullptr, (long)L.cin_gp * 4, B, Cin, T, C->dev_err, nullptr, 0, s);
  GemmArgs g = gemm_args(L, R, T);
  if (h3) g.xs = xs, g.ld_xs = (long)L.cin_gp * 4;
  else g.w_h3 = nullptr, g.x = xf, g.ld_x = Cin;
  g.act = act;
  if (res_tm) g.res = to_dev(*C, res_tm, (size_t)R * Cout), g.ld_res = Cout;
  float* dy = C->arena.alloc<float>((size_t)R * Cout);
  float* dc = C->arena.alloc<float>((size_t)R * Cout);
  float* ds = C->arena.alloc<float>((size_t)R * Cout);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, (size_t)R * Cout * 4, s));
  RVCX_HIP(hipMemsetAsync(dc, 0xff, (size_t)R * Cout * 4, s));
  g.y = dy, g.ld_y = Cout;
  if (y_cf) g.y_cf = dc, g.cf_bs = (long)Cout * T;
  if (y_split && Cout % 16 == 0) g.ys = ds, g.ld_ys = (long)Cout * 4;
  C->gemm_on(g, s);
  to_host(*C, y_tm, dy, (size_t)R * Cout);
  if (y_cf) to_host(*C, y_cf, dc, (size_t)R * Cout);
  if (g.ys) {
    std::vector<uint16_t> raw((size_t)R * Cout * 2);
    RVCX_HIP(hipMemcpy(raw.data(), ds, raw.size() * 2, hipMemcpyDeviceToHost));
    decode_xs(raw, R, Cout, y_split);
  }
  C->arena.reset();
  API_END
}

int rvcx_bench_gemm(rvcx_ctx* ctx, int64_t rows, int Cin, int Cout, int iters, float* ms_per_launch) {
  REQUIRE_DEBUG(ctx, "rvcx_bench_gemm")
  API_BEGIN(ctx)
  TEMP_REGION(C);
  C->arena.reserve(((size_t)rows * ((size_t)Cin + 2 * (size_t)Cout)) * 4 + (64 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  std::vector<float> w((size_t)Cout * Cin), bias((size_t)Cout, 0.1f);
  for (size_t i = 0; i < w.size(); ++i) w[i] = ((float)((i * 2654435761u) % 2001) / 1000.f - 1.f) / std::sqrt((float)Cin);
  ConvW L = make_conv(*C, w.data(), bias.data(), Cout, Cin, 1, 1, true);
  float* xf = C->arena.alloc<float>((size_t)rows * Cin);
  float* xs = C->arena.alloc<float>((size_t)rows * L.cin_gp);
  float* dy = C->arena.alloc<float>((size_t)rows * Cout);
  launch_randn(xf, (size_t)rows * Cin, 1, 0, s);
  // N(0,1) data read as a channel-first (1, Cin, rows) map -> split rows
  launch_cf_to_tm(xf, (long)Cin * rows, nullptr, 0, xs, (long)L.cin_gp * 4, 1, Cin, (int)rows, nullptr, nullptr, 0, s);
  GemmArgs g = gemm_args(L, rows, (int)rows);
  g.xs = xs, g.ld_xs = (long)L.cin_gp * 4;
  g.y = dy, g.ld_y = Cout;
  C->gemm_on(g, s);
  hipEvent_t e0, e1;
  RVCX_HIP(hipEventCreate(&e0));
  RVCX_HIP(hipEventCreate(&e1));
  RVCX_HIP(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) C->gemm_on(g, s);
  RVCX_HIP(hipEventRecord(e1, s));
  RVCX_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  RVCX_HIP(hipEventElapsedTime(&ms, e0, e1));
  *ms_per_launch = ms / iters;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  C->arena.reset();
  API_END
}

int rvcx_op_layernorm_tm(rvcx_ctx* ctx, const float* x, const float* gamma, const float* beta, float* y, float* y_split,
                         int64_t rows, int Cc, float eps) {
  API_BEGIN(ctx)
  const size_t n = (size_t)rows * Cc;
  C->arena.reserve(n * 16 + (64 << 20));
  C->arena.reset();
  float* dx = to_dev(*C, x, n);
  float* dy = C->arena.alloc<float>(n);
  float* ds = C->arena.alloc<float>(n);
  launch_layernorm_tm(dx, Cc, to_dev(*C, gamma, Cc), to_dev(*C, beta, Cc), dy, Cc, (y_split && Cc % 16 == 0) ? ds : nullptr,
                      (long)Cc * 4, rows, Cc, eps, C->dev_err, nullptr, 0, C->stream);
  to_host(*C, y, dy, n);
  if (y_split && Cc % 16 == 0) {
    std::vector<uint16_t> raw(n * 2);
    RVCX_HIP(hipMemcpy(raw.data(), ds, raw.size() * 2, hipMemcpyDeviceToHost));
    decode_xs(raw, rows, Cc, y_split);
  }
  C->arena.reset();
  API_END
}

int rvcx_op_layernorm_c(rvcx_ctx* ctx, const float* x, const float* gamma, const float* beta, float* y, int B,
                        int Cc, int T, float eps) {
  API_BEGIN(ctx)
  const size_t n = (size_t)B * Cc * T;
  C->arena.reserve(n * 8 + (64 << 20));
  C->arena.reset();
  float* dx = to_dev(*C, x, n);
  float* dy = C->arena.alloc<float>(n);
  launch_layernorm_c(dx, to_dev(*C, gamma, Cc), to_dev(*C, beta, Cc), dy, B, Cc, T, eps, nullptr, C->stream);
  to_host(*C, y, dy, n);
  C->arena.reset();
  API_END
}

int rvcx_op_groupnorm_gelu(rvcx_ctx* ctx, const float* x, const float* gamma, const float* beta, int B, int Cc, int T, float eps,
                           const int32_t* lens, float* y, float* stats, float* y_split) {
  API_BEGIN(ctx)
  if (!x || !gamma || !beta || !y || B <= 0 || Cc <= 0 || T <= 0) fail("op_groupnorm_gelu: bad argument");
  if ((stats == nullptr) != (y_split == nullptr)) fail("op_groupnorm_gelu: stats and y_split come together");
  if (lens)
    for (int b = 0; b < B; ++b)
      if (lens[b] < 1 || lens[b] > T) fail("op_groupnorm_gelu: lens outside [1, T]");
  const size_t n = (size_t)B * Cc * T;
  C->arena.reserve(n * 4 * 3 + (size_t)B * Cc * 8 + (64 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  float* dx = to_dev(*C, x, n);
  const float *dg = to_dev(*C, gamma, Cc), *db = to_dev(*C, beta, Cc);
  const int* dl = (lens ? to_dev(*C, lens, B) : nullptr);
  float* dy = C->arena.alloc<float>(n);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, n * 4, s));      // NaN fill: every element must be written
  launch_groupnorm_gelu(dx, dg, db, dy, B, Cc, T, eps, s, dl);
  float *dst = nullptr, *ds = nullptr;
  if (stats) {
    dst = C->arena.alloc<float>((size_t)B * Cc * 2);
    ds = C->arena.alloc<float>(n);
    RVCX_HIP(hipMemsetAsync(dst, 0xff, (size_t)B * Cc * 8, s));
    RVCX_HIP(hipMemsetAsync(ds, 0xff, n * 4, s));
    launch_groupnorm_gelu_split(dx, dg, db, dst, ds, B, Cc, T, eps, s, dl, C->dev_err, nullptr, 0);
  }
  RVCX_HIP(hipGetLastError());
  to_host(*C, y, dy, n);
  if (stats) {
    to_host(*C, stats, dst, (size_t)B * Cc * 2);
    std::vector<uint16_t> raw(n * 2);
    RVCX_HIP(hipMemcpy(raw.data(), ds, raw.size() * 2, hipMemcpyDeviceToHost));
    decode_split_cf(raw, B, Cc, T, y_split);
  }
  C->arena.reset();
  API_END
}

int rvcx_op_hubert_conv0(rvcx_ctx* ctx, const float* wav, const float* w, const float* gamma, const float* beta, int B, int Cc,
                         int n, int K, int stride, float eps, const int32_t* lens, int fused, float* stats, float* y_split,
                         uint16_t* raw_split) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  if (!wav || !w || !gamma || !beta || !stats || !y_split || B <= 0 || Cc <= 0 || K <= 0 || stride <= 0 || n < K)
    fail("op_hubert_conv0: bad argument");
  const int T0 = (n - K) / stride + 1;
  if (lens)
    for (int b = 0; b < B; ++b)
      if (lens[b] < 1 || lens[b] > T0) fail("op_hubert_conv0: lens outside [1, T0]");
  const size_t ny = (size_t)B * Cc * T0;
  C->arena.reserve(((size_t)B * n + 2 * ny + (size_t)B * Cc * 2) * 4 + (64 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  ConvW L = make_conv(*C, w, nullptr, Cc, 1, K, 1);
  float* dw = to_dev(*C, wav, (size_t)B * n);
  const float *dg = to_dev(*C, gamma, Cc), *db = to_dev(*C, beta, Cc);
  const int* dl = (lens ? to_dev(*C, lens, B) : nullptr);
  float* dst = C->arena.alloc<float>((size_t)B * Cc * 2);
  float* ds = C->arena.alloc<float>(ny);
  RVCX_HIP(hipMemsetAsync(dst, 0xff, (size_t)B * Cc * 8, s));      // NaN fill: every element must be written
  RVCX_HIP(hipMemsetAsync(ds, 0xff, ny * 4, s));
  if (fused) {
    launch_hubert_conv0_gn_gelu_split(dw, (long)n, L.w, K, stride, L.cin_gp * L.cout_gp, dg, db, nullptr, dst, ds, B, Cc, T0, eps,
                                      s, dl, C->dev_err, nullptr, 0);
  } else {      // hubert.hip's three passes: the conv stores the fp32 map, statistics, split store
    float* dm = C->arena.alloc<float>(ny);
    RVCX_HIP(hipMemsetAsync(dm, 0xff, ny * 4, s));
    ConvArgs a = conv1d_args(L, dw, dm, B, n, T0, stride, 1, 0);
    a.lens_out = dl;
    C->conv(a);
    launch_groupnorm_gelu_split(dm, dg, db, dst, ds, B, Cc, T0, eps, s, dl, C->dev_err, nullptr, 0);
  }
  RVCX_HIP(hipGetLastError());
  to_host(*C, stats, dst, (size_t)B * Cc * 2);
  std::vector<uint16_t> raw(ny * 2);
  RVCX_HIP(hipMemcpy(raw.data(), ds, raw.size() * 2, hipMemcpyDeviceToHost));
  decode_split_cf(raw, B, Cc, T0, y_split);
  if (raw_split) std::memcpy(raw_split, raw.data(), raw.size() * 2);
  C->arena.reset();
  API_END
}

int rvcx_op_sine_source(rvcx_ctx* ctx, const float* f0, const float* noise, const float* lin_wb, int B, int T, int upp, float sr,
                        const int32_t* lens, float* har) {
  API_BEGIN(ctx)
  if (!f0 || !noise || !lin_wb || !har || B <= 0 || T <= 0 || upp <= 0) fail("op_sine_source: bad argument");
  const size_t n = (size_t)B * T * upp;
  C->arena.reserve(n * 8 + (size_t)B * T * 24 + (64 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  const float* df = to_dev(*C, f0, (size_t)B * T);
  const float* dn = to_dev(*C, noise, n);
  const float* dwb = to_dev(*C, lin_wb, 2);
  const int* dl = (lens ? to_dev(*C, lens, B) : nullptr);
  double* sc = C->arena.alloc<double>((size_t)B * T * 2);      // prefixes (fp64) + rad (fp32), as synth.hip sizes it
  float* dh = C->arena.alloc<float>(n);
  RVCX_HIP(hipMemsetAsync(dh, 0xff, n * 4, s));      // NaN fill: every element must be written
  launch_sine_source(df, dn, dh, B, T, upp, sr, dwb, dl, sc, s);
  RVCX_HIP(hipGetLastError());
  to_host(*C, har, dh, n);
  C->arena.reset();
  API_END
}

int rvcx_op_randn(rvcx_ctx* ctx, int64_t n, uint64_t seed, uint64_t offset, float* out) {
  API_BEGIN(ctx)
  if (!out || n <= 0) fail("op_randn: bad argument");
  C->arena.reserve((size_t)n * 4 + (64 << 20));
  C->arena.reset();
  float* d = C->arena.alloc<float>((size_t)n + 4);
  RVCX_HIP(hipMemsetAsync(d, 0xff, ((size_t)n + 4) * 4, C->stream));      // NaN fill, and four guard words behind the tail
  launch_randn(d, (size_t)n, seed, offset, C->stream);
  RVCX_HIP(hipGetLastError());
  std::vector<float> h((size_t)n + 4);
  to_host(*C, h.data(), d, h.size());
  for (size_t i = (size_t)n; i < h.size(); ++i)
    if (!std::isnan(h[i])) fail("op_randn: wrote behind the last value");
  std::memcpy(out, h.data(), (size_t)n * 4);
  C->arena.reset();
  API_END
}

int rvcx_op_reflect_pad(rvcx_ctx* ctx, const float* x, int B, int n, int p, const int32_t* ns, float* y) {
  API_BEGIN(ctx)
  if (!x || !y || B <= 0 || n <= 0 || p < 0) fail("op_reflect_pad: bad argument");
  if (ns)
    for (int b = 0; b < B; ++b)
      if (ns[b] < 1 || ns[b] > n) fail("op_reflect_pad: ns outside [1, n]");
  const size_t ny = (size_t)B * (n + 2 * p);
  C->arena.reserve(((size_t)B * n + ny) * 4 + (64 << 20));
  C->arena.reset();
  const float* dx = to_dev(*C, x, (size_t)B * n);
  const int* dn = (ns ? to_dev(*C, ns, B) : nullptr);
  float* dy = C->arena.alloc<float>(ny);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, ny * 4, C->stream));      // NaN fill: every element must be written
  launch_reflect_pad(dx, dy, B, n, p, (long)n + 2 * p, C->stream, dn);
  RVCX_HIP(hipGetLastError());
  to_host(*C, y, dy, ny);
  C->arena.reset();
  API_END
}

int rvcx_op_mel_post(rvcx_ctx* ctx, const float* mel, int B, int nmel, int F, int Tp, const float* bn, const int32_t* fs,
                     const int32_t* tps, float* out) {
  API_BEGIN(ctx)
  if (!mel || !bn || !out || B <= 0 || nmel <= 0 || F <= 0 || Tp <= 0) fail("op_mel_post: bad argument");
  for (int b = 0; b < B; ++b) {
    const int Fb = fs ? fs[b] : F, Tb = tps ? tps[b] : Tp;
    if (Fb < 1 || Fb > F || Tb < 0 || Tb > Tp || Tb > 2 * Fb - 1) fail("op_mel_post: rows cannot be reflected from the item's frames");
  }
  const size_t nx = (size_t)B * nmel * F, ny = (size_t)B * Tp * (nmel + 2);
  C->arena.reserve((nx + ny) * 4 + (64 << 20));
  C->arena.reset();
  const float* dm = to_dev(*C, mel, nx);
  const float* dbn = to_dev(*C, bn, 2);
  const int* dfs = (fs ? to_dev(*C, fs, B) : nullptr);
  const int* dtp = (tps ? to_dev(*C, tps, B) : nullptr);
  float* dy = C->arena.alloc<float>(ny);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, ny * 4, C->stream));      // NaN fill: every element must be written
  launch_mel_post(dm, dy, B, nmel, F, Tp, dbn, C->stream, dfs, dtp);
  RVCX_HIP(hipGetLastError());
  to_host(*C, out, dy, ny);
  C->arena.reset();
  API_END
}

int rvcx_op_decode_f0(rvcx_ctx* ctx, const float* sal, int B, int T, int ld, float thred, float f0_min, float f0_max, float* f0) {
  API_BEGIN(ctx)
  if (!sal || !f0 || B <= 0 || T <= 0 || ld < 360) fail("op_decode_f0: bad argument");
  const size_t nx = (size_t)B * T * ld, ny = (size_t)B * T;
  C->arena.reserve((nx + ny) * 4 + (64 << 20));
  C->arena.reset();
  const float* dsal = to_dev(*C, sal, nx);
  float* dy = C->arena.alloc<float>(ny);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, ny * 4, C->stream));      // NaN fill: every element must be written
  launch_decode_f0(dsal, dy, B, T, ld, thred, f0_min, f0_max, C->stream);
  RVCX_HIP(hipGetLastError());
  to_host(*C, f0, dy, ny);
  C->arena.reset();
  API_END
}

int rvcx_op_avgpool2(rvcx_ctx* ctx, const float* x, int planes, int H, int Wp, int64_t x_ps, int64_t y_ps, float* y) {
  API_BEGIN(ctx)
  if (!x || !y || planes <= 0 || H < 2 || Wp < 4 || Wp % 2) fail("op_avgpool2: bad argument");
  if (x_ps < (int64_t)H * Wp || y_ps < (int64_t)(H / 2) * ((Wp - 2) / 2 + 2)) fail("op_avgpool2: plane stride smaller than the plane");
  const size_t nx = (size_t)planes * x_ps, ny = (size_t)planes * y_ps;
  C->arena.reserve((nx + ny) * 4 + (64 << 20));
  C->arena.reset();
  const float* dx = to_dev(*C, x, nx);
  float* dy = C->arena.alloc<float>(ny);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, ny * 4, C->stream));      // NaN fill: what the kernel does not own stays NaN
  launch_avgpool2(dx, dy, planes, H, Wp, (long)x_ps, (long)y_ps, C->stream);
  RVCX_HIP(hipGetLastError());
  to_host(*C, y, dy, ny);
  C->arena.reset();
  API_END
}

int rvcx_op_gru_input(rvcx_ctx* ctx, const float* x, int B, int Cc, int T, int Wp, float* y) {
  API_BEGIN(ctx)
  if (!x || !y || B <= 0 || Cc <= 0 || T <= 0 || Wp < 3) fail("op_gru_input: bad argument");
  const size_t nx = (size_t)B * Cc * T * Wp, ny = (size_t)B * Cc * (Wp - 2) * T;
  C->arena.reserve((nx + ny) * 4 + (64 << 20));
  C->arena.reset();
  const float* dx = to_dev(*C, x, nx);
  float* dy = C->arena.alloc<float>(ny);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, ny * 4, C->stream));      // NaN fill: every element must be written
  launch_gru_input(dx, dy, B, Cc, T, Wp, C->stream);
  RVCX_HIP(hipGetLastError());
  to_host(*C, y, dy, ny);
  C->arena.reset();
  API_END
}

int rvcx_op_upsample_protect(rvcx_ctx* ctx, const float* feats, const float* feats0, const float* pitchf, int Cc, int Th, int p_len,
                             float protect, int use_protect, int ld_in, int ld_out, float* out) {
  API_BEGIN(ctx)
  if (!feats || !out || Cc <= 0 || Th <= 0 || p_len <= 0 || p_len > 2 * Th) fail("op_upsample_protect: bad argument");
  if (use_protect && (!feats0 || !pitchf)) fail("op_upsample_protect: protect needs feats0 and pitchf");
  const int li = ld_in > 0 ? ld_in : Th, lo = ld_out > 0 ? ld_out : p_len;
  if (li < Th || lo < p_len) fail("op_upsample_protect: row stride smaller than the row");
  const size_t nx = (size_t)Cc * li, ny = (size_t)Cc * lo;
  C->arena.reserve((2 * nx + ny + (size_t)p_len) * 4 + (64 << 20));
  C->arena.reset();
  const float* df = to_dev(*C, feats, nx);
  const float* df0 = (use_protect ? to_dev(*C, feats0, nx) : nullptr);
  const float* dp = (use_protect ? to_dev(*C, pitchf, (size_t)p_len) : nullptr);
  float* dy = C->arena.alloc<float>(ny);
  RVCX_HIP(hipMemsetAsync(dy, 0xff, ny * 4, C->stream));      // NaN fill: what the kernel does not own stays NaN
  launch_upsample_protect(df, df0, dp, dy, Cc, Th, p_len, protect, use_protect, C->stream, ld_in, ld_out);
  RVCX_HIP(hipGetLastError());
  to_host(*C, out, dy, ny);
  C->arena.reset();
  API_END
}

int rvcx_op_crepe_decode(rvcx_ctx* ctx, const float* probs, int64_t F, int batch, float fmin, float fmax, const float* dither,
                         float* pitch, int32_t* bins) {
  API_BEGIN(ctx)
  if (!C->crepe) fail("crepe not loaded");
  if (!probs || !dither || !pitch || F <= 0 || batch <= 0) fail("crepe_decode: bad argument");
  C->arena.reserve((size_t)F * (2 * 360 * 4 + 360 * 2 + 64) + (64 << 20));
  C->arena.reset();
  hipStream_t s = C->stream;
  float* dpr = to_dev(*C, probs, (size_t)F * 360);
  float* dd = to_dev(*C, dither, (size_t)F);
  float* dp = C->arena.alloc<float>((size_t)F);
  int* db = C->arena.alloc<int>((size_t)F);
  crepe_decode(*C, *C->crepe, dpr, (long)F, batch, fmin, fmax, dd, dp, db, s);
  RVCX_HIP(hipMemcpyAsync(pitch, dp, (size_t)F * 4, hipMemcpyDefault, s));
  if (bins) RVCX_HIP(hipMemcpyAsync(bins, db, (size_t)F * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipStreamSynchronize(s));
  C->arena.reset();
  API_END
}

int rvcx_op_fcpe_post(rvcx_ctx* ctx, const float* raw, int F_in, int p_len, double pitch, double f0_min, double f0_max,
                      int32_t* coarse, float* f0) {
  API_BEGIN(ctx)
  if (F_in <= 0 || p_len <= 0) fail("fcpe_post: empty track");
  C->arena.reserve((size_t)(F_in + 5L * p_len) * 4 + (64 << 20));
  C->arena.reset();
  float* dr = to_dev(*C, raw, (size_t)F_in);
  int* dc = C->arena.alloc<int>((size_t)p_len);
  float* df = C->arena.alloc<float>((size_t)p_len);
  fcpe_post_coarse(*C, dr, 1, F_in, p_len, df, dc, p_len, pitch, f0_min, f0_max, C->stream);
  RVCX_HIP(hipMemcpyAsync(coarse, dc, (size_t)p_len * 4, hipMemcpyDefault, C->stream));
  RVCX_HIP(hipMemcpyAsync(f0, df, (size_t)p_len * 4, hipMemcpyDefault, C->stream));
  RVCX_HIP(hipStreamSynchronize(C->stream));
  C->arena.reset();
  API_END
}

int rvcx_op_bigru(rvcx_ctx* ctx, const float* x, const float* w_ih, const float* w_hh, const float* b_ih,
                  const float* b_hh, const float* w_ih_r, const float* w_hh_r, const float* b_ih_r,
                  const float* b_hh_r, float* y, int B, int T, int I, int H) {
  API_BEGIN(ctx)
  TEMP_REGION(C);
  const int H3 = 3 * H;
  C->arena.reserve(((size_t)B * T * (2 * I + 2 * H3 + 4 * H)) * 4 + (64 << 20));
  C->arena.reset();
  std::vector<float> wih((size_t)2 * H3 * I), bih((size_t)2 * H3), whh_t((size_t)2 * H * H3), bhh((size_t)2 * H3);
  const float* wi[2] = {w_ih, w_ih_r};
  const float* wh[2] = {w_hh, w_hh_r};
  const float* bi[2] = {b_ih, b_ih_r};
  const float* bh[2] = {b_hh, b_hh_r};
  for (int d = 0; d < 2; ++d) {
    std::memcpy(&wih[(size_t)d * H3 * I], wi[d], (size_t)H3 * I * 4);
    std::memcpy(&bih[(size_t)d * H3], bi[d], (size_t)H3 * 4);
    std::memcpy(&bhh[(size_t)d * H3], bh[d], (size_t)H3 * 4);
    for (int j = 0; j < H3; ++j)
      for (int k = 0; k < H; ++k) whh_t[((size_t)d * H + k) * H3 + j] = wh[d][(size_t)j * H + k];
  }
  ConvW Wih = make_conv(*C, wih.data(), bih.data(), 2 * H3, I, 1, 1);
  const float* dwhh = C->slab.upload(whh_t);
  const float* dbhh = C->slab.upload(bhh);
  float* dx = to_dev(*C, x, (size_t)B * T * I);
  float* dxt = C->arena.alloc<float>((size_t)B * T * I);
  launch_transpose(dx, dxt, B, T, I, C->stream);   // (B,T,I) -> (B,I,T)
  float* gi = C->arena.alloc<float>((size_t)B * T * 2 * H3);
  ConvArgs a = conv1d_args(Wih, dxt, gi, B, T, T);
  a.out_mode = OUT_TRANSPOSED;
  a.y_bs = (long)T * 2 * H3;
  a.y_cs = 2 * H3;
  C->conv(a);
  float* gy = C->arena.alloc<float>((size_t)B * 2 * H * T);
  void* gscr = C->arena.alloc<unsigned long long>(bigru_scratch_bytes(B) / 8);
  launch_bigru(gi, dwhh, dbhh, gy, B, T, H, gscr, C->dev_err, C->stream);
  float* gyt = C->arena.alloc<float>((size_t)B * 2 * H * T);
  launch_transpose(gy, gyt, B, 2 * H, T, C->stream);  // (B,2H,T) -> (B,T,2H)
  to_host(*C, y, gyt, (size_t)B * T * 2 * H);
  C->check_dev_err();
  C->arena.reset();
  API_END
}

int rvcx_op_highpass(rvcx_ctx* ctx, const double* x, double* y, int64_t n) {
  API_BEGIN(ctx)
  C->arena.reserve((size_t)n * 32 + (64 << 20));
  C->arena.reset();
  double* dx = C->arena.alloc<double>((size_t)n);
  RVCX_HIP(hipMemcpyAsync(dx, x, (size_t)n * 8, hipMemcpyHostToDevice, C->stream));
  double* ext = C->arena.alloc<double>(highpass_ext_doubles(n));
  double* dy = C->arena.alloc<double>((size_t)n);
  launch_highpass(nullptr, dx, ext, dy, nullptr, n, C->stream);
  RVCX_HIP(hipMemcpyAsync(y, dy, (size_t)n * 8, hipMemcpyDeviceToHost, C->stream));
  RVCX_HIP(hipStreamSynchronize(C->stream));
  C->arena.reset();
  API_END
}

}  // extern "C"
