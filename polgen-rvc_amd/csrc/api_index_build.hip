// C ABI of index building (include/rvcx.h "index building"): the refusals, then kmeans.hip.
#include "api_internal.h"

using namespace rvcx;
using namespace rvcx::api;

// Both calls run once (no range-guard repeat): a value beyond fp16 range demotes its rows to the exact scan inside the call.
int rvcx_kmeans(rvcx_ctx* ctx, const float* x, int64_t n, int dim, const float* init, int k, int iters, float* centroids,
                int32_t* assign, int32_t* counts, double* objective, int32_t* splits) {
  API_BEGIN_ONCE(ctx)
  if (!x || !init) fail("kmeans: null argument");
  if (dim < 16 || dim % 16 != 0) fail("kmeans: dim must be a multiple of 16, got " + std::to_string(dim));
  if (dim > 1024) fail("kmeans: dim above 1024 (" + std::to_string(dim) + ")");
  if (k < 1) fail("kmeans: k must be at least 1, got " + std::to_string(k));
  if (k > n) fail("kmeans: k = " + std::to_string(k) + " exceeds the " + std::to_string(n) + " rows");
  if (iters < 1) fail("kmeans: iters must be at least 1");
  if (n >= ((int64_t)1 << 31)) fail("kmeans: 2^31 rows or more");
  C->kmeans_exhaustive = 0;
  C->kmeans_exhaustive = kmeans_run(*C, x, n, dim, init, k, iters, centroids, assign, counts, objective, splits).exhaustive;
  API_END
}

int rvcx_ivf_assign(rvcx_ctx* ctx, const float* x, int64_t n, int dim, const float* centroids, int nlist, int32_t* assign) {
  API_BEGIN_ONCE(ctx)
  if (!x || !centroids || !assign) fail("ivf_assign: null argument");
  if (dim < 1 || dim > 1024) fail("ivf_assign: dim must be 1 .. 1024, got " + std::to_string(dim));
  if (nlist < 1 || n < 1) fail("ivf_assign: no centroids or no rows");
  if (n >= ((int64_t)1 << 31)) fail("ivf_assign: 2^31 rows or more");
  ivf_assign_run(*C, x, n, dim, centroids, nlist, assign);
  API_END
}

int rvcx_index_features(rvcx_ctx* ctx, int B, const float* wav, int64_t n, int out_dim, float* feats) {
  API_BEGIN(ctx)
  if (!C->hubert) fail("hubert not loaded");
  if (!wav || !feats || B < 1) fail("index_features: null argument");
  const int T = hubert_frames(*C->hubert, n), E = C->hubert->cfg.embed_dim;
  if (T <= 0) fail("hubert: input too short");
  if (out_dim < 1 || out_dim > E) fail("index_features: no such feature width");
  C->ensure_splitk(B);
  C->arena.reserve(hubert_arena_bytes(*C->hubert, B, n) + (size_t)B * (n + (size_t)3 * T * E) * 4 + (1 << 20));
  C->arena.reset();
  hipStream_t st = C->stream;
  float* dw = to_dev(*C, wav, (size_t)B * n);
  float* fct = C->arena.alloc<float>((size_t)B * out_dim * T);
  float* ftc = C->arena.alloc<float>((size_t)B * out_dim * T);
  hubert_features_for(*C, *C->hubert, out_dim, B, dw, n, fct, st);
  launch_transpose(fct, ftc, B, out_dim, T, st);   // (B, out_dim, T) -> (B, T, out_dim)
  RVCX_HIP(hipMemcpyAsync(feats, ftc, (size_t)B * out_dim * T * 4, hipMemcpyDefault, st));
  RVCX_HIP(hipStreamSynchronize(st));
  C->arena.reset();
  API_END
}

int64_t rvcx_kmeans_exhaustive(rvcx_ctx* ctx) {
  CtxLock ctx_guard_ = lock_ctx(ctx);
  return ctx ? ctx->c.kmeans_exhaustive : -1;
}
