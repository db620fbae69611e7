// Index building (include/rvcx.h "index building"): Lloyd's k-means with a deterministic split of empty clusters, and the
// filing of stored rows into the inverted lists of an "IVF{n},Flat" index.  The reference ships no index trainer (RVC's
// "train index" step calls faiss / scikit-learn); the stages are defined in the header and restated in float64 in
// tests/kmeans_reference.py.
//
// One iteration: ASSIGN every row to the centroid with the smallest exact fp32 pair distance e(x, c) = |c|^2 - 2 x.c,
// OBJECTIVE = sum (|x|^2 + e) in double, UPDATE = double mean of the members in ascending row order, SPLIT of the empty
// clusters.  The n x k dot products are a PRE-FILTER on the split-fp16 GEMM (gemm.hip), as in index.hip: per row the best
// two centroids by approximate distance are kept, the best one is re-scored exactly, and it is the answer only when it is
// CERTIFIED -- every other centroid has an approximate distance >= the second one, so if the exact distance of the first is
// below that minus the error bound nobody else can win or tie.  A row that fails the test (near-ties, duplicated centroids,
// values beyond fp16 range) is scanned over all k centroids with the same dot routine.  The assignment therefore does not
// depend on the pre-filter, the tiling or the row chunks (RVCX_KMEANS_PREFILTER=0: every row takes the scan; same bits).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "gemm.h"
#include "h3_device.h"
#include "layers.h"
#include "models.h"
#include "ops.h"

namespace rvcx {

namespace {

constexpr int kMaxDim = 1024;       // index.hip's limit: a row fits the LDS of the scan
constexpr int kSplits = 32;         // centroid ranges of the best-two reduction
constexpr int kObjBlock = 4096;     // rows per partial sum of the objective (a function of the row index only)

struct DevBuf {                     // device memory for the length of one call
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  template <typename T>
  T* get(size_t n) {
    RVCX_HIP(hipMalloc(&p, std::max<size_t>(n * sizeof(T), 256)));
    return static_cast<T*>(p);
  }
};

// THE dot product of a (row, centroid) pair, by 16 lanes: lane l takes the dimensions 4 l .. 4 l + 3 of every block of 64
// in four independent fma chains, (s0 + s1) + (s2 + s3), then a fixed xor tree.  Every exact path goes through it, so a
// pair has ONE distance.  Error: a chain has dim / 64 <= 16 terms, six additions follow -- |dot - x.c| <= 22 u sum |x_i c_i|
// <= 22 * 2^-24 |x||c|; e = cn - 2 dot with cn from the same routine: |e - exact| <= 2^-24 (45 |x||c| + 23 |c|^2)
// < 2^-18 (|x||c| + |c|^2), inside the 2^-17 the header allows.
__device__ __forceinline__ float pair_dot(const float* a, const float* b, int dim, int l) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int d = 4 * l; d < dim; d += 64) {
    const float4 u = *reinterpret_cast<const float4*>(a + d), v = *reinterpret_cast<const float4*>(b + d);
    s0 = fmaf(u.x, v.x, s0);
    s1 = fmaf(u.y, v.y, s1);
    s2 = fmaf(u.z, v.z, s2);
    s3 = fmaf(u.w, v.w, s3);
  }
  float s = (s0 + s1) + (s2 + s3);
  s += __shfl_xor(s, 8);
  s += __shfl_xor(s, 4);
  s += __shfl_xor(s, 2);
  s += __shfl_xor(s, 1);
  return s;
}

// |c|^2 per centroid through pair_dot: 16 centroids per workgroup
__global__ __launch_bounds__(256) void cent_norm_kernel(const float* __restrict__ cent, float* cn, int k, int dim) {
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int c = blockIdx.x * 16 + g;
  const float* row = cent + (long)min(c, k - 1) * dim;
  const float s = pair_dot(row, row, dim, l);
  if (l == 0 && c < k) cn[c] = s;
}

// |x|^2 per row in double: one wavefront per row, lane l sums the dimensions l, l + 64, .. in order, xor tree
__global__ __launch_bounds__(256) void row_norm2_kernel(const float* __restrict__ x, double* xn2, long n, int dim) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const float* row = x + (r < n ? r : n - 1) * dim;
  double s = 0.0;
  for (int d = lane; d < dim; d += 64) s += (double)row[d] * (double)row[d];
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
  if (lane == 0 && r < n) xn2[r] = s;
}

// rows (n, dim) fp32 -> the fp16 hi/lo split rows the GEMM stages (gemm.h: 64 bytes per 16 channels).  A value the split
// cannot hold marks its ROW: that row never trusts the pre-filter.
__global__ __launch_bounds__(256) void split_rows_kernel(const float* __restrict__ x, void* xs, long ld_xs, long n, int dim,
                                                         int* bad) {
  typedef _Float16 half4 __attribute__((ext_vector_type(4)));
  const int per = dim >> 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * per) return;
  const long row = idx / per;
  const int c = (int)(idx % per) * 4;
  const float4 v4 = *reinterpret_cast<const float4*>(x + row * dim + c);
  const float v[4] = {v4.x, v4.y, v4.z, v4.w};
  half4 hi, lo;
  bool ovf = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    ovf |= !(fabsf(v[q]) < kH3ActLimit);
    const _Float16 vh = (_Float16)v[q];
    hi[q] = vh;
    lo[q] = (_Float16)((v[q] - (float)vh) * kH3Scale);
  }
  char* e = static_cast<char*>(xs) + row * ld_xs + (c >> 4) * 64 + ((c >> 3) & 1) * 16 + (c & 7) * 2;
  *reinterpret_cast<half4*>(e) = hi;
  *reinterpret_cast<half4*>(e + 32) = lo;
  if (ovf) bad[row] = 1;
}

// best two of (b1, i1, b2) and a later range's (c1, j1, c2); ids of the later range are larger, so a tie keeps i1 -- and
// leaves b2 == b1, which no certificate survives
__device__ __forceinline__ void best2_merge(float& b1, int& i1, float& b2, float c1, int j1, float c2) {
  if (c1 < b1) {
    b2 = fminf(b1, c2);
    b1 = c1;
    i1 = j1;
  } else {
    b2 = fminf(b2, c1);
  }
}

// dots (kp, T) channel-first from the GEMM: block = 64 rows x 4 centroid slices, grid.y = centroid ranges.  Per (range,
// row): the smallest approximate distance cn - 2 dot, its centroid, and the second smallest.
__global__ __launch_bounds__(256) void best2_partial_kernel(const float* __restrict__ dots, const float* __restrict__ cn,
                                                            int k, int T, int splits, float* p1, int* pi, float* p2) {
  __shared__ float s1[4][64], s2[4][64];
  __shared__ int si[4][64];
  const int tx = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + tx;
  const int per = (k + splits - 1) / splits;
  const int c0 = blockIdx.y * per, c1 = min(k, c0 + per);
  const int sub = (per + 3) / 4;                         // contiguous sub-range per slice: ids ascend with `part`
  float b1 = INFINITY, b2 = INFINITY;
  int i1 = 0;
  if (t < T)
    for (int c = c0 + part * sub; c < min(c1, c0 + (part + 1) * sub); ++c) {
      const float d = cn[c] - 2.f * dots[(long)c * T + t];
      if (d < b1) {
        b2 = b1;
        b1 = d;
        i1 = c;
      } else if (d < b2) {
        b2 = d;
      }
    }
  s1[part][tx] = b1;
  s2[part][tx] = b2;
  si[part][tx] = i1;
  __syncthreads();
  if (part == 0 && t < T) {
    for (int p = 1; p < 4; ++p) best2_merge(b1, i1, b2, s1[p][tx], si[p][tx], s2[p][tx]);
    const long o = (long)blockIdx.y * T + t;
    p1[o] = b1;
    pi[o] = i1;
    p2[o] = b2;
  }
}

// 16 lanes per row: merge the ranges, re-score the best centroid with pair_dot and certify it.  E bounds |approx - e|, where
// approx = cn - 2 dot_h3 carries TWICE the GEMM's dot error.  That error, by the structure of gemm_h3_kernel: per chunk of 16
// channels three 32x32x16 MFMAs (hi.hi, hi.lo, lo.hi) add a 16-term block each to ONE fp32 accumulator, so a dot is a chain
// of 3 dim / 16 <= 192 accumulator roundings (not dim sequential ones) plus the rounding inside a block -- at most
// ~(192 + 16) 2^-24 |x||c| = 2^-16.3 |x||c| in the worst case at dim = 1024, plus the split's own 2^-20 |x||c|; doubled and
// with pair_dot's 2^-18 (|x||c| + |c|^2) that stays below 2^-15 |x||c| + 2^-18 |c|^2.  E = 2^-16 (|x| + |c|max)^2 >=
// 2^-14 |x||c| + 2^-16 |c|^2 is twice that.  (A GEMM that summed dim terms one by one would NOT be covered at dim = 1024:
// the bound leans on the blocked accumulation.)  Every other centroid c has e(c) >= approx(c) - E >= b2 - E, so e1 < b2 - E
// makes i1 the unique minimum.  *ovf, the context's device error word, is belt and braces: nothing on this path raises it
// today (the GEMM converts no activation when it stores y_cf, and split_rows_kernel marks its rows in `bad` itself); a
// split kernel that did raise it would decertify every row until the iteration's end.
__global__ __launch_bounds__(256) void rescore_kernel(const float* p1, const int* pi, const float* p2, int splits, int T,
                                                      const float* __restrict__ x, const double* __restrict__ xn2,
                                                      const int* __restrict__ bad, const float* __restrict__ cent,
                                                      const float* __restrict__ cn, int dim, float cmax, const int* ovf,
                                                      int* assign, float* e_out, int* flag) {
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int t = blockIdx.x * 16 + g;
  const int tc = min(t, T - 1);
  float b1 = p1[tc], b2 = p2[tc];
  int i1 = pi[tc];
  for (int s = 1; s < splits; ++s) best2_merge(b1, i1, b2, p1[(long)s * T + tc], pi[(long)s * T + tc], p2[(long)s * T + tc]);
  const float dot = pair_dot(x + (long)tc * dim, cent + (long)i1 * dim, dim, l);
  if (l != 0 || t >= T) return;
  const float e1 = cn[i1] - 2.f * dot;
  const float sq = sqrtf((float)xn2[t]) + cmax;
  const float E = 1.52587890625e-5f * sq * sq;
  const bool certified = !bad[t] && !(*ovf & kErrH3Overflow) && b1 < INFINITY && e1 < b2 - E;
  assign[t] = i1;
  e_out[t] = e1;
  flag[t] = certified ? 0 : 1;
}

// The exact scan of the rows nobody certified (one workgroup per row; returns at once for the others): every centroid
// through pair_dot, the smallest e, the smaller id on ties.
__global__ __launch_bounds__(256) void exact_scan_kernel(const int* __restrict__ flag, const float* __restrict__ x,
                                                         const float* __restrict__ cent, const float* __restrict__ cn,
                                                         int k, int dim, int* assign, float* e_out,
                                                         unsigned long long* counter) {
  const int t = blockIdx.x, tid = threadIdx.x;
  if (!flag[t]) return;
  __shared__ __align__(16) float qs[kMaxDim];
  __shared__ float sd[16];
  __shared__ int si[16];
  for (int c = tid; c < dim; c += 256) qs[c] = x[(long)t * dim + c];
  __syncthreads();
  const int g = tid >> 4, l = tid & 15;
  float be = INFINITY;
  int bi = 0;
  for (int c0 = 0; c0 < k; c0 += 16) {                   // whole groups iterate together: the shuffles of pair_dot stay converged
    const int c = min(c0 + g, k - 1);
    const float e = cn[c] - 2.f * pair_dot(qs, cent + (long)c * dim, dim, l);
    if (c0 + g < k && e < be) {
      be = e;
      bi = c;
    }
  }
  if (l == 0) {
    sd[g] = be;
    si[g] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int p = 1; p < 16; ++p)
      if (sd[p] < be || (sd[p] == be && si[p] < bi)) {
        be = sd[p];
        bi = si[p];
      }
    assign[t] = bi;
    e_out[t] = be;
    atomicAdd(counter, 1ull);
  }
}

// objective: sum over rows of |x|^2 + e in double.  Rows in blocks of kObjBlock: thread t adds its rows t, t + 256, .. in
// order, the 256 sums meet in a fixed tree; the block sums are added the same way by one workgroup.
__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
    __syncthreads();
  }
  return sh[0];
}
__global__ __launch_bounds__(256) void objective_partial_kernel(const double* __restrict__ xn2, const float* __restrict__ e,
                                                                long n, double* part) {
  __shared__ double sh[256];
  const long r0 = (long)blockIdx.x * kObjBlock;
  double s = 0.0;
  for (long r = r0 + threadIdx.x; r < min(n, r0 + kObjBlock); r += 256) s += xn2[r] + (double)e[r];
  const double tot = block_tree_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ __launch_bounds__(256) void objective_final_kernel(const double* __restrict__ part, long nb, double* out) {
  __shared__ double sh[256];
  double s = 0.0;
  for (long b = threadIdx.x; b < nb; b += 256) s += part[b];
  const double tot = block_tree_sum(s, sh);
  if (threadIdx.x == 0) *out = tot;
}

// update: one workgroup per cluster, threads across the dimensions, the members (ascending row ids) added one after the
// other in double, one division, one rounding to float.  No atomics: the sum does not depend on anything but the list.
__global__ __launch_bounds__(256) void segmented_mean_kernel(const float* __restrict__ x, const int* __restrict__ members,
                                                             const int* __restrict__ offsets, int dim, float* cent) {
  const int c = blockIdx.x;
  const int m0 = offsets[c], m1 = offsets[c + 1];
  if (m1 == m0) return;                                  // empty: keeps its centroid until the split treats it
  for (int d = threadIdx.x; d < dim; d += 256) {
    double acc = 0.0;
    int m = m0;
    for (; m + 3 < m1; m += 4) {                         // four loads in flight, added in list order
      const float v0 = x[(long)members[m] * dim + d], v1 = x[(long)members[m + 1] * dim + d];
      const float v2 = x[(long)members[m + 2] * dim + d], v3 = x[(long)members[m + 3] * dim + d];
      acc += (double)v0;
      acc += (double)v1;
      acc += (double)v2;
      acc += (double)v3;
    }
    for (; m < m1; ++m) acc += (double)x[(long)members[m] * dim + d];
    cent[(long)c * dim + d] = (float)(acc / (double)(m1 - m0));
  }
}

// split of the empty clusters, in the order the host lists them: pairs[2 p] = the empty cluster, pairs[2 p + 1] = the
// cluster it halves.  A thread owns its dimensions across all pairs, so the pairs need no barrier between them.
__global__ __launch_bounds__(256) void split_kernel(float* cent, const int* __restrict__ pairs, int npairs, int dim) {
  const float up = 1.f + 0.0009765625f, dn = 1.f - 0.0009765625f;
  for (int p = 0; p < npairs; ++p) {
    const long c = pairs[2 * p], j = pairs[2 * p + 1];
    for (int d = threadIdx.x; d < dim; d += 256) {
      const float v = cent[j * dim + d];
      const bool even = (d & 1) == 0;
      cent[c * dim + d] = v * (even ? up : dn);
      cent[j * dim + d] = v * (even ? dn : up);
    }
  }
}

bool prefilter_wanted() {
  static const bool on = !getenv("RVCX_KMEANS_PREFILTER") || atoi(getenv("RVCX_KMEANS_PREFILTER")) != 0;
  return on;
}

// rows per chunk: what keeps the (kp, rows) dots near 384 MB -- at k = 10 000, 8 192 rows = 82 M dots
long chunk_rows(long n, int kp) {
  long rows = 65536;
  while (rows > 256 && rows * kp > (96L << 20)) rows >>= 1;
  return std::min(n, rows);
}

}  // namespace

KmeansResult kmeans_run(Ctx& c, const float* x_in, int64_t n, int dim, const float* init, int k, int iters, float* centroids,
                        int32_t* assign_out, int32_t* counts_out, double* objective, int32_t* splits) {
  RVCX_CHECK(dim % 16 == 0 && dim <= kMaxDim && k >= 1 && k <= n && iters >= 1 && n < (1L << 31), "kmeans: bad shape");
  hipStream_t s = c.stream;
  KmeansResult res;
  const int kp = round_up(k, 4);                         // the GEMM stores channels in fours: zero rows pad the centroids
  const long ld_xs = (long)conv_cin_pad(dim) * 4;
  const bool want_pre = prefilter_wanted() && conv_h3_configured();
  const long chunk = chunk_rows(n, kp);
  const int splits_k = std::min(kSplits, cdiv(k, 64));
  const long nb = cdiv64(n, kObjBlock);

  DevBuf bx, bxs, bxn, be, bas, bmem, bbad, bcent, bcn, boff, bpairs, bpart, bcnt;
  float* x = bx.get<float>((size_t)n * dim);
  double* xn2 = bxn.get<double>((size_t)n);
  float* e = be.get<float>((size_t)n);
  int* assign = bas.get<int>((size_t)n);
  int* members = bmem.get<int>((size_t)n);
  int* bad = bbad.get<int>((size_t)n);
  float* cent = bcent.get<float>((size_t)k * dim);
  float* cn = bcn.get<float>((size_t)k);
  int* offsets = boff.get<int>((size_t)k + 1);
  int* pairs = bpairs.get<int>((size_t)2 * k);
  double* part = bpart.get<double>((size_t)nb + 1);
  unsigned long long* counter = bcnt.get<unsigned long long>(1);
  RVCX_HIP(hipMemcpyAsync(x, x_in, (size_t)n * dim * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipMemcpyAsync(cent, init, (size_t)k * dim * 4, hipMemcpyDefault, s));
  RVCX_HIP(hipMemsetAsync(bad, 0, (size_t)n * 4, s));
  RVCX_HIP(hipMemsetAsync(counter, 0, 8, s));
  hipLaunchKernelGGL(row_norm2_kernel, dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, s, x, xn2, (long)n, dim);
  void* xs = nullptr;
  if (want_pre) {                                        // the data matrix is split ONCE; the centroids change per iteration
    xs = bxs.get<char>((size_t)n * ld_xs);
    hipLaunchKernelGGL(split_rows_kernel, dim3((unsigned)cdiv64(n * (dim / 4), 256)), dim3(256), 0, s, x, xs, ld_xs, (long)n,
                       dim, bad);
  }
  RVCX_HIP(hipGetLastError());

  c.arena.reset();
  c.arena.reserve((size_t)kp * chunk * 4 + (size_t)chunk * (3 * kSplits + 1) * 4 + (1 << 20));
  std::vector<float> hcent((size_t)kp * dim, 0.f), hcn((size_t)k);
  std::vector<int32_t> hassign((size_t)n), hcounts((size_t)k), book((size_t)k), hoff((size_t)k + 1), hmem((size_t)n), hpairs;

  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(cent_norm_kernel, dim3(cdiv(k, 16)), dim3(256), 0, s, cent, cn, k, dim);
    RVCX_HIP(hipMemcpyAsync(hcent.data(), cent, (size_t)k * dim * 4, hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipMemcpyAsync(hcn.data(), cn, (size_t)k * 4, hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipStreamSynchronize(s));
    float cmax2 = 0.f;
    for (float v : hcn) {
      if (!std::isfinite(v)) fail("kmeans: a centroid is not finite");
      cmax2 = std::max(cmax2, v);
    }
    const float cmax = std::sqrt(cmax2);

    // this iteration's centroids as a Linear layer with its split image: a weight region of its own, freed below
    WeightRegion region;
    ConvW L;
    bool pre = want_pre;
    if (pre) {
      RegionScope scope(c, region);
      L = make_conv(c, hcent.data(), nullptr, kp, dim, 1, 1, true);
      region.seal();
      pre = conv_h3_ok(L) && gemm_h3_enabled() && (long)L.cin_gp * L.cout_gp * 4 < kH3Oob;   // centroids beyond fp16: no filter
    }
    for (long r0 = 0; r0 < n; r0 += chunk) {
      const int T = (int)std::min<long>(chunk, n - r0);
      c.arena.reset();
      int* flag = c.arena.alloc<int>((size_t)T);
      if (pre) {
        float* dots = c.arena.alloc<float>((size_t)kp * T);
        float* p1 = c.arena.alloc<float>((size_t)splits_k * T);
        float* p2 = c.arena.alloc<float>((size_t)splits_k * T);
        int* pi = c.arena.alloc<int>((size_t)splits_k * T);
        GemmArgs g = gemm_args(L, T, T);
        g.xs = static_cast<const char*>(xs) + r0 * ld_xs;
        g.ld_xs = ld_xs;
        g.y_cf = dots;
        g.cf_bs = (long)kp * T;
        c.gemm_on(g, s);
        hipLaunchKernelGGL(best2_partial_kernel, dim3(cdiv(T, 64), splits_k), dim3(256), 0, s, dots, cn, k, T, splits_k, p1,
                           pi, p2);
        hipLaunchKernelGGL(rescore_kernel, dim3(cdiv(T, 16)), dim3(256), 0, s, p1, pi, p2, splits_k, T, x + r0 * dim,
                           xn2 + r0, bad + r0, cent, cn, dim, cmax, c.dev_err, assign + r0, e + r0, flag);
      } else {
        RVCX_HIP(hipMemsetAsync(flag, 1, (size_t)T * 4, s));
      }
      hipLaunchKernelGGL(exact_scan_kernel, dim3(T), dim3(256), 0, s, flag, x + r0 * dim, cent, cn, k, dim, assign + r0,
                         e + r0, counter);
      RVCX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(objective_partial_kernel, dim3((unsigned)nb), dim3(256), 0, s, xn2, e, (long)n, part);
    hipLaunchKernelGGL(objective_final_kernel, dim3(1), dim3(256), 0, s, part, nb, part + nb);
    double obj = 0.0;
    RVCX_HIP(hipMemcpyAsync(&obj, part + nb, 8, hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipMemcpyAsync(hassign.data(), assign, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    RVCX_HIP(hipStreamSynchronize(s));                   // the region's weights are no longer in use either
    (void)c.take_overflow();                             // a range overflow demoted its rows; it is not an error of the call
    if (objective) objective[it] = obj;

    // the host pass over the n list ids: histogram, counting sort into member lists (ascending rows inside a list)
    std::fill(hcounts.begin(), hcounts.end(), 0);
    for (int64_t r = 0; r < n; ++r) {
      const int32_t a = hassign[(size_t)r];
      if (a < 0 || a >= k) fail("kmeans: internal: list id out of range");
      ++hcounts[(size_t)a];
    }
    hoff[0] = 0;
    for (int cc = 0; cc < k; ++cc) hoff[(size_t)cc + 1] = hoff[(size_t)cc] + hcounts[(size_t)cc];
    {
      std::vector<int32_t> cur(hoff.begin(), hoff.end() - 1);
      for (int64_t r = 0; r < n; ++r) hmem[(size_t)cur[(size_t)hassign[(size_t)r]]++] = (int32_t)r;
    }
    RVCX_HIP(hipMemcpyAsync(members, hmem.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    RVCX_HIP(hipMemcpyAsync(offsets, hoff.data(), ((size_t)k + 1) * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(segmented_mean_kernel, dim3(k), dim3(256), 0, s, x, members, offsets, dim, cent);

    // empty clusters in ascending id: each halves the cluster that is largest by the running bookkeeping
    book = hcounts;
    hpairs.clear();
    for (int cc = 0; cc < k; ++cc) {
      if (hcounts[(size_t)cc] != 0) continue;
      int j = 0;
      for (int q = 1; q < k; ++q)
        if (book[(size_t)q] > book[(size_t)j]) j = q;
      hpairs.push_back(cc);
      hpairs.push_back(j);
      book[(size_t)cc] = book[(size_t)j] / 2;
      book[(size_t)j] -= book[(size_t)cc];
    }
    const int npairs = (int)hpairs.size() / 2;
    if (npairs) {
      RVCX_HIP(hipMemcpyAsync(pairs, hpairs.data(), hpairs.size() * 4, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(split_kernel, dim3(1), dim3(256), 0, s, cent, pairs, npairs, dim);
    }
    if (splits) splits[it] = npairs;
    RVCX_HIP(hipGetLastError());
    RVCX_HIP(hipStreamSynchronize(s));                   // hmem / hpairs are reused by the next iteration
  }
  if (centroids) RVCX_HIP(hipMemcpyAsync(centroids, cent, (size_t)k * dim * 4, hipMemcpyDefault, s));
  if (assign_out) RVCX_HIP(hipMemcpyAsync(assign_out, assign, (size_t)n * 4, hipMemcpyDefault, s));
  if (counts_out) RVCX_HIP(hipMemcpyAsync(counts_out, hcounts.data(), (size_t)k * 4, hipMemcpyDefault, s));
  unsigned long long cnt = 0;
  RVCX_HIP(hipMemcpyAsync(&cnt, counter, 8, hipMemcpyDeviceToHost, s));
  RVCX_HIP(hipStreamSynchronize(s));
  c.arena.reset();
  res.exhaustive = (int64_t)cnt;
  return res;
}

// The inverted list of every stored row: literally the search's coarse quantiser (index.hip: coarse_assign_kernel on the
// exact-fp32 dots of conv_on), in row chunks.
void ivf_assign_run(Ctx& c, const float* x_in, int64_t n, int dim, const float* centroids, int nlist, int32_t* assign_out) {
  RVCX_CHECK(dim <= kMaxDim && nlist >= 1 && n >= 1, "ivf_assign: bad shape");
  hipStream_t s = c.stream;
  std::vector<float> hc((size_t)nlist * dim);
  RVCX_HIP(hipMemcpy(hc.data(), centroids, hc.size() * 4, hipMemcpyDefault));
  WeightRegion region;
  RegionScope scope(c, region);
  const ConvW cent = make_conv(c, hc.data(), nullptr, nlist, dim, 1, 1, false);
  const float* cent_norms = c.slab.upload(index_sq_norms(hc.data(), nlist, dim));
  region.seal();
  const long chunk = chunk_rows(n, nlist);
  c.arena.reset();
  c.arena.reserve(index_coarse_arena_bytes(nlist, (int)chunk) + (size_t)chunk * (2 * dim + 1) * 4 + (1 << 20));
  for (long r0 = 0; r0 < n; r0 += chunk) {
    const int T = (int)std::min<long>(chunk, n - r0);
    c.arena.reset();
    float* rows = c.arena.alloc<float>((size_t)T * dim);
    float* fct = c.arena.alloc<float>((size_t)T * dim);
    int* qlist = c.arena.alloc<int>((size_t)T);
    RVCX_HIP(hipMemcpyAsync(rows, x_in + r0 * dim, (size_t)T * dim * 4, hipMemcpyDefault, s));
    launch_transpose(rows, fct, 1, T, dim, s);           // (T, dim) -> channel-first (dim, T): what the search hands the quantiser
    index_coarse_assign(c, cent, cent_norms, fct, T, qlist, s);
    RVCX_HIP(hipMemcpyAsync(assign_out + r0, qlist, (size_t)T * 4, hipMemcpyDefault, s));
    RVCX_HIP(hipStreamSynchronize(s));
  }
  c.arena.reset();
}

}  // namespace rvcx
