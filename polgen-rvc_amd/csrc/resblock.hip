// One step of ResBlock1 (rvc/lib/algorithm/residuals.py:45-53) as ONE kernel:
//     xt = c1(leaky_relu(x));  xt = c2(leaky_relu(xt));  x = xt + x
// c1: k taps, dilation d; c2: k taps, dilation 1; both C -> C channels, "same" zero padding.
//
// Unfused, the pair moves five activation tensors through HBM (read x, write xt, read xt, read x again as the
// residual, write y) and re-stages the same input tile once per 32-channel output block.  Here a workgroup owns
// ALL C channels of a tile of positions: the c1 output tile never leaves the CU -- it is written, already in the
// fp16 hi/lo split form and element order the MFMA B operand wants, into LDS and consumed from there by c2; the
// residual is re-read from the (L2-hot) x tile the workgroup just staged.  HBM traffic per pair: read x, write y.
//
// Arithmetic is exactly conv_h3_kernel's (same split, same MFMA order: chunks of 16 input channels ascending, taps
// ascending, three MFMAs {S wh . xh, wh . S xl, S wl . xh} per block), so the fused step is bit-identical to the two
// launches it replaces (tests/test_gpu_conv.py::test_fused_resblock_pair_equals_two_launches).
//
// Tile: N1 = 32 NT positions of the c1 output (= the c2 input tile incl. its (k-1)/2 halo on both sides); the
// workgroup stores BN = N1 - (k-1) output positions.  LDS: Y1[C/16][op][h][N1 + 16] + As[KKT][op][h][C] +
// Bs[op][h][N1 + 64], 16-byte elements (8 halves = the k-slice one lane feeds to one MFMA).
//
// Two kernels, 20 instantiations (kPair at the end of the file):
//   resblock_pair_persist_kernel  rows 16-byte aligned, C <= 128: a workgroup per CU walks a range of tiles, wide epilogue
//   resblock_pair_kernel          one workgroup per tile: C = 256 with the wide epilogue (aligned rows), and every (C, k)
//                                 with the dword epilogue for rows that are not aligned
// The forms that were measured against these and lost are in LABNOTES.md and in the history of this file.
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <type_traits>

#include "conv.h"
#include "conv_device.h"
#include "h3_device.h"

namespace rvcx {

namespace {

constexpr int kPairHalo = 64;    // (k - 1) d <= 50 for k <= 11, d <= 5
constexpr int kPairPadY = 16;    // c2 reads up to k - 1 <= 10 columns past N1 (for output columns that are discarded)

// ====================================================================================================================
// The PER-TILE form: one workgroup per tile of positions.
//
// K: taps (compile time: the k-loop is straight-line code, fragment reads of slot s+1 are issued ahead of the MFMAs
// of slot s).  A stage = NCS chunks of 16 input channels x a group of <= KKT taps ("slots"); NCS > 1 only with
// KKT == K (small kernels: more MFMA work between two barriers).
// RESPF: when the residual x of the output tile is fetched.  1: all of a wave's values in one go right behind the c2
// loop; 2: ahead of the c2 loop, so that the loads fly under its MFMAs (where 16 WM WN more registers fit); fetched
// inside the epilogue, eight values at a time, they cost four dependent load -> store round trips per wave: ~5 us of
// every workgroup, 3 ms of a 30 s clip.  3: the WIDE epilogue -- every 32 x 32 accumulator tile goes through a 4.5 KB LDS
// tile of its wave and comes back transposed, a lane then owns 4 consecutive positions of one channel: residual loads and
// output stores are 16 bytes per lane, a quarter of the memory instructions (the dword stores were store-ISSUE bound).
// Needs 16-byte aligned rows (cs, T multiples of 4); the tile keeps a multiple of 4 output positions.
// tools/mfma_peak.hip: ds_read_b128 delivers ~115 B/clk/CU, so at one fragment read per MFMA the LDS, not the
// matrix pipe, bounds the k-loop (measured: 1.9 us per stage against 1.2 us of MFMA time).
template <int C, int NT, int WR, int WC, int K, int KKT, int NCS, int RESPF>
__global__ __launch_bounds__(64 * WR * WC) void resblock_pair_kernel(const PairArgs a) {
  constexpr int THREADS = 64 * WR * WC;
  constexpr int N1 = 32 * NT, N1P = N1 + kPairPadY, WROW = N1 + kPairHalo;
  constexpr int WM = (C / 32) / WR, WN = NT / WC;
  constexpr int NCHUNK = C / 16;
  constexpr int NG = (K + KKT - 1) / KKT;                 // tap groups per chunk set
  constexpr int SL = NCS * KKT;                           // weight slots resident per stage
  constexpr int A_ELEMS = SL * 4 * C, NA = (A_ELEMS + THREADS - 1) / THREADS;
  constexpr int B_TASKS = NCS * 2 * WROW, NBT = (B_TASKS + THREADS - 1) / THREADS;
  constexpr int BN_OUT = RESPF == 3 ? ((N1 - (K - 1)) & ~3) : N1 - (K - 1), H2 = (K - 1) / 2;
  static_assert(RESPF >= 1 && RESPF <= 3, "residual fetch: 1 behind the c2 loop, 2 ahead of it, 3 wide epilogue");
  static_assert(WM >= 1 && WN >= 1 && WM * WR * 32 == C && WN * WC == NT, "bad tile");
  static_assert(NCS == 1 || KKT == K, "several chunks per stage only with all taps resident");
  static_assert(NCHUNK % NCS == 0, "chunk sets must tile the channels");
  extern __shared__ uint4 lds[];
  constexpr int Y1_ELEMS = NCHUNK * 4 * N1P;
  uint4* Y1 = lds;                              // [chunk][op][h][N1P]
  uint4* As = Y1 + Y1_ELEMS;                    // [slot][op][h][C]
  uint4* Bs = As + A_ELEMS;                     // [cl][op][h][WROW]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int i = lane & 31, h = lane >> 5;
  const int b = blockIdx.z;
  const int pad1 = (K - 1) * a.dil / 2;
  // XCD-aware tile order.  Workgroups are dealt round-robin to the 8 XCDs (block b -> XCD b % 8), each with its own L2:
  // with tile = blockIdx.x neighbouring tiles always sit on DIFFERENT L2s, so the halo columns two tiles share are
  // fetched from HBM twice and the cache line that straddles a tile boundary (BN_OUT is not a multiple of 32
  // positions) is written back half-filled by two L2s.  Here XCD x works through a contiguous range of tiles.
  int tile = blockIdx.x;
  if (a.xcd_order) {
    const int nt = gridDim.x, xcd = tile & 7, idx = tile >> 3, q = nt >> 3, r = nt & 7;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int n0 = tile * BN_OUT;
  const int len = a.lens ? a.lens[b] : a.T;
  const int wuse = N1 + (K - 1) * a.dil;        // input columns the tile really needs
  const int in_base = n0 - H2 - pad1;           // position of input-tile column 0
  const float slope = a.slope;
  const H3Rsrc xr = h3_rsrc(a.x + (long)b * a.bs, C * a.cs * 4);
  const H3Rsrc w1r = h3_rsrc(a.w1, K * NCHUNK * 4 * C * 16);
  const H3Rsrc w2r = h3_rsrc(a.w2, K * NCHUNK * 4 * C * 16);
  const int xrow = a.cs * 4;
  constexpr int slab = 4 * C * 16;              // bytes of one (tap, chunk) weight slab

  // phase stamps of this workgroup (100 MHz real-time counter): 0 start, 1 first stage committed (inputs arrived),
  // 2 c1 loop done, 3 Y1 written, 4 c2 loop done, 5 end; 6 = tile, 7 = XCC id
  auto stamp = [&](int k) {
    if (a.trace && tid == 0) a.trace[((long)b * gridDim.x + blockIdx.x) * 8 + k] = (long long)wall_clock64();
  };
  stamp(0);
  if (a.trace && tid == 0) {
    a.trace[((long)b * gridDim.x + blockIdx.x) * 8 + 6] = tile;
    unsigned xcc = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
#endif
    a.trace[((long)b * gridDim.x + blockIdx.x) * 8 + 7] = xcc & 0xf;
  }
  f32x16 acc[WM][WN];
  auto zero_acc = [&]() {
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
      for (int n = 0; n < WN; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
  };

  // stage-invariant addressing: weight element e = tid + THREADS j -> (slot = cl * KKT + kkl, op, h, co)
  int a_cl[NA], a_kkl[NA], a_off[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int e = tid + THREADS * j;
    const int co = e % C, rest = e / C;          // rest = (slot*2 + op)*2 + h
    const int slot = rest / 4;
    a_cl[j] = slot / KKT;
    a_kkl[j] = slot % KKT;
    a_off[j] = e < A_ELEMS ? ((rest % 4) * C + co) * 16 : kH3Oob;
  }
  int b_off[NBT], b_row[NBT];                    // input task t -> (cl, h, p): 8 channels at one position
#pragma unroll
  for (int j = 0; j < NBT; ++j) {
    const int t = tid + THREADS * j;
    const int ch2 = t / WROW, p = t - ch2 * WROW;   // ch2 = cl*2 + h
    const int pos = in_base + p;
    b_row[j] = (ch2 >> 1) * 16 + (ch2 & 1) * 8;
    b_off[j] = (t < B_TASKS && p < wuse && pos >= 0 && pos < len) ? pos * 4 : kH3Oob;
  }

  uint4 ra[NA];
  float rb[NBT][8];
  bool ovf = false;
  auto fetch_b = [&](int chunk0) {
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
      const int row0 = (chunk0 * 16 + b_row[j]) * xrow;
#pragma unroll
      for (int q = 0; q < 8; ++q) rb[j][q] = h3_load1(xr, b_off[j] == kH3Oob ? kH3Oob : row0 + q * xrow + b_off[j]);
    }
  };
  auto fetch_a = [&](const H3Rsrc& wr_, int chunk0, int kk0) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int kk = kk0 + a_kkl[j];
      const bool ok = a_off[j] != kH3Oob && kk < K;
      ra[j] = h3_load4(wr_, ok ? (kk * NCHUNK + chunk0 + a_cl[j]) * slab + a_off[j] : kH3Oob);
    }
  };
  auto commit_a = [&]() {
#pragma unroll
    for (int j = 0; j < NA; ++j)
      if (NA * THREADS == A_ELEMS || tid + THREADS * j < A_ELEMS) As[tid + THREADS * j] = ra[j];
  };
  auto commit_b = [&]() {
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
      const int t = tid + THREADS * j;
      if (NBT * THREADS == B_TASKS || t < B_TASKS) {
        half8 hi, lo;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float v = rb[j][q];
          v = v > 0.f ? v : v * slope;                 // leaky_relu ahead of c1
          ovf |= !(fabsf(v) < kH3ActLimit);
          const _Float16 vh = (_Float16)v;
          hi[q] = vh;
          lo[q] = (_Float16)((v - (float)vh) * kH3Scale);
        }
        const int ch2 = t / WROW, p = t - ch2 * WROW;
        const int cl = ch2 >> 1, hh = ch2 & 1;
        Bs[((cl * 2 + 0) * 2 + hh) * WROW + p] = __builtin_bit_cast(uint4, hi);
        Bs[((cl * 2 + 1) * 2 + hh) * WROW + p] = __builtin_bit_cast(uint4, lo);
      }
    }
  };
  // The k-steps of one stage: slots (cl, kkl), TAPS taps per chunk.  Bt: tile of chunk cl at Bt + cl * cl_pitch,
  // [op][h][pitch]; tap kk of the group starting at kk0 reads column + (kk0 + kkl) * tap_step.  Fragments of the
  // next slot are read before the MFMAs of the current one are issued.
  auto compute = [&](auto taps_tag, const uint4* Bt, int pitch, int cl_pitch, int kk0, int tap_step) {
    constexpr int TAPS = decltype(taps_tag)::value;
    constexpr int NS = NCS * TAPS;
    half8 af[2][2][WM], bf[2][2][WN];
    auto load = [&](int buf, int s) {
      const int cl = s / TAPS, kkl = s % TAPS;
      const int tp = (kk0 + kkl) * tap_step;
      const uint4* Bc = Bt + cl * cl_pitch;
#pragma unroll
      for (int m = 0; m < WM; ++m) {
        af[buf][0][m] = __builtin_bit_cast(half8, As[(((cl * KKT + kkl) * 2 + 0) * 2 + h) * C + wr * (WM * 32) + m * 32 + i]);
        af[buf][1][m] = __builtin_bit_cast(half8, As[(((cl * KKT + kkl) * 2 + 1) * 2 + h) * C + wr * (WM * 32) + m * 32 + i]);
      }
#pragma unroll
      for (int op = 0; op < 2; ++op)
#pragma unroll
        for (int n = 0; n < WN; ++n)
          bf[buf][op][n] = __builtin_bit_cast(half8, Bc[(op * 2 + h) * pitch + wc * (WN * 32) + n * 32 + i + tp]);
    };
    load(0, 0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int cur = s & 1;
      if (s + 1 < NS) load(cur ^ 1, s + 1);
#pragma unroll
      for (int m = 0; m < WM; ++m) {
        const half8 wh = af[cur][0][m] * (_Float16)(1.f / kH3Scale);
#pragma unroll
        for (int n = 0; n < WN; ++n) {
          acc[m][n] = h3_mfma(af[cur][0][m], bf[cur][0][n], acc[m][n]);   // (S wh) xh
          acc[m][n] = h3_mfma(wh, bf[cur][1][n], acc[m][n]);              // wh (S xl)
          acc[m][n] = h3_mfma(af[cur][1][m], bf[cur][0][n], acc[m][n]);   // (S wl) xh
        }
      }
    }
    // The software pipeline above, PINNED.  Left alone the scheduler sinks every ds_read next to its first use
    // -- the ISA was {ds_read, s_waitcnt lgkmcnt(0), v_mfma} per MFMA: each wave pays the LDS latency per matrix
    // instruction, the matrix pipe idled more than half of the k-loop.  The groups below order the block as: the first
    // slot's fragment reads, then per slot one MFMA / one read of the NEXT slot alternating; the compiler's counted
    // lgkmcnt waits then find the data already there.  Same instructions, same arithmetic order per accumulator.
    {
      constexpr int R = 2 * WM + 2 * WN, M = 3 * WM * WN;
      __builtin_amdgcn_sched_group_barrier(0x100, R, 0);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          if (s + 1 < NS && j < R) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        if (s + 1 < NS && R > M) __builtin_amdgcn_sched_group_barrier(0x100, R - M, 0);
      }
    }
  };
  using Full = std::integral_constant<int, KKT>;
  using Last = std::integral_constant<int, K - (NG - 1) * KKT>;
  constexpr float inv = 1.f / kH3Scale;

  // ================================================================ phase 1: Y1 = lrelu(c1(lrelu(x)) + b1)
  zero_acc();
  fetch_b(0);
  fetch_a(w1r, 0, 0);
  // The tap groups of a chunk set are unrolled at compile time: one loop body holds the Full and the Last form of the
  // k-steps, so the accumulators keep their registers across the loop (as a runtime choice inside one loop the two forms
  // were joined by 32 v_mov_b64 per stage behind an s_nop that drained the matrix pipe).
  for (int chunk = 0; chunk < NCHUNK; chunk += NCS) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const bool last_stage = chunk + NCS >= NCHUNK && g == NG - 1;
      __syncthreads();
      if (g == 0) commit_b();
      commit_a();
      __syncthreads();
      if (chunk == 0 && g == 0) stamp(1);
      if (!last_stage) fetch_a(w1r, g + 1 == NG ? chunk + NCS : chunk, g + 1 == NG ? 0 : (g + 1) * KKT);
      else fetch_a(w2r, 0, 0);                       // first weights of c2 fly during the c1 epilogue
      if (g == 0 && chunk + NCS < NCHUNK) fetch_b(chunk + NCS);
      if (NG > 1 && g == NG - 1) compute(Last{}, Bs, WROW, 4 * WROW, g * KKT, a.dil);
      else compute(Full{}, Bs, WROW, 4 * WROW, g * KKT, a.dil);
    }
  }
  stamp(2);
  // c1 epilogue: bias, leaky_relu (the one ahead of c2), zero outside the sequence, split, into LDS
#pragma unroll
  for (int m = 0; m < WM; ++m)
#pragma unroll
    for (int n = 0; n < WN; ++n) {
      const int c_t = wr * (WM * 32) + m * 32;
      const int j = wc * (WN * 32) + n * 32 + i;
      const int pos1 = n0 - H2 + j;
      const bool live = pos1 >= 0 && pos1 < len;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        typedef _Float16 half4 __attribute__((ext_vector_type(4)));
        const int cg = c_t + 8 * g;
        half4 hi, lo;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v = acc[m][n][4 * g + q] * inv + (a.b1 ? a.b1[cg + 4 * h + q] : 0.f);
          v = fmaxf(v, v * slope);
          v = live ? v : 0.f;
          ovf |= !(fabsf(v) < kH3ActLimit);
          const _Float16 vh = (_Float16)v;
          hi[q] = vh;
          lo[q] = (_Float16)((v - (float)vh) * kH3Scale);
        }
        char* e_hi = reinterpret_cast<char*>(Y1 + (((cg >> 4) * 2 + 0) * 2 + (g & 1)) * N1P + j) + 8 * h;
        char* e_lo = reinterpret_cast<char*>(Y1 + (((cg >> 4) * 2 + 1) * 2 + (g & 1)) * N1P + j) + 8 * h;
        *reinterpret_cast<half4*>(e_hi) = hi;
        *reinterpret_cast<half4*>(e_lo) = lo;
      }
    }

  if (ovf) report_h3_overflow(a.ovf, a.ovf_layer, a.seq);

  // ================================================================ phase 2: y = c2(Y1) + b2 + x
  float resv[WM][WN][16];
  auto load_res = [&]() {
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
      for (int n = 0; n < WN; ++n) {
        const int col = wc * (WN * 32) + n * 32 + i;
        const int pos = n0 + col;
        const bool ok = col < BN_OUT && pos < a.T;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int co = wr * (WM * 32) + m * 32 + 4 * h + (r & 3) + 8 * (r >> 2);
          if (RESPF == 2) {
            // Issued HERE, not where the compiler would like them (it sinks a plain load across the whole c2 loop to its
            // first use): inline asm stays put.  The compiler does not count these loads; they are older than every
            // load of the c2 loop, loads return in order, so its counted waits stay correct (they only wait longer),
            // and the epilogue waits vmcnt(0) by hand before the first use.
            const float* p = a.x + (long)b * a.bs + (ok ? (long)co * a.cs + pos : 0);
            float v;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(p) : "memory");
#else
            v = *p;
#endif
            resv[m][n][r] = v;
          } else {
            resv[m][n][r] = h3_load1(xr, ok ? (co * a.cs + pos) * 4 : kH3Oob);
          }
        }
      }
  };
  if (RESPF == 2) load_res();
  zero_acc();
  stamp(3);
  for (int chunk = 0; chunk < NCHUNK; chunk += NCS) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const bool last_stage = chunk + NCS >= NCHUNK && g == NG - 1;
      __syncthreads();
      commit_a();
      __syncthreads();
      if (!last_stage) fetch_a(w2r, g + 1 == NG ? chunk + NCS : chunk, g + 1 == NG ? 0 : (g + 1) * KKT);
      if (NG > 1 && g == NG - 1) compute(Last{}, Y1 + chunk * 4 * N1P, N1P, 4 * N1P, g * KKT, 1);
      else compute(Full{}, Y1 + chunk * 4 * N1P, N1P, 4 * N1P, g * KKT, 1);
    }
  }
  stamp(4);
  if constexpr (RESPF == 3) {
    constexpr int P = 36;                              // floats per staged row: 16-byte aligned, rows 4 banks apart
    static_assert(THREADS / 64 * 32 * P * 4 <= NCHUNK * 4 * N1P * 16, "staging tiles must fit the Y1 region");
    __syncthreads();                                   // every wave is done reading Y1: the staging tiles overlay it
    float* stg = reinterpret_cast<float*>(lds) + wave * (32 * P);
    const int lr = lane >> 3, lc = (lane & 7) * 4;
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
      for (int n = 0; n < WN; ++n) {
#pragma unroll
        for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * h) * P + i] = acc[m][n][r] * inv;
        __builtin_amdgcn_wave_barrier();               // same wave, in-order LDS queue: ordering for the compiler only
        const int col0 = wc * (WN * 32) + n * 32 + lc;
        const int pos0 = n0 + col0;
        const bool ok = col0 < BN_OUT && pos0 < a.T;
        float4 v[4], rv[4], pv[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int co = wr * (WM * 32) + m * 32 + lr + 8 * p;
          const long off = (long)b * a.bs + (long)co * a.cs + pos0;
          v[p] = *reinterpret_cast<const float4*>(stg + (lr + 8 * p) * P + lc);
          rv[p] = ok ? *reinterpret_cast<const float4*>(a.x + off) : make_float4(0.f, 0.f, 0.f, 0.f);
          pv[p] = (ok && a.acc2_mode != ACC2_NONE && a.acc2_mode != ACC2_SET) ? *reinterpret_cast<const float4*>(a.y2 + off)
                                                                              : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __builtin_amdgcn_wave_barrier();
        if (ok) {
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const int co = wr * (WM * 32) + m * 32 + lr + 8 * p;
            const long off = (long)b * a.bs + (long)co * a.cs + pos0;
            const float bb = a.b2 ? a.b2[co] : 0.f;
            float o[4] = {v[p].x + bb + rv[p].x, v[p].y + bb + rv[p].y, v[p].z + bb + rv[p].z, v[p].w + bb + rv[p].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = pos0 + q < len ? o[q] : 0.f;
            if (a.y) *reinterpret_cast<float4*>(a.y + off) = make_float4(o[0], o[1], o[2], o[3]);
            if (a.acc2_mode != ACC2_NONE) {
              const float pp[4] = {pv[p].x, pv[p].y, pv[p].z, pv[p].w};
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                if (a.acc2_mode == ACC2_ADD) o[q] = pp[q] + o[q];
                else if (a.acc2_mode == ACC2_ADD_DIV) o[q] = (pp[q] + o[q]) / a.acc2_div;
              }
              *reinterpret_cast<float4*>(a.y2 + off) = make_float4(o[0], o[1], o[2], o[3]);
            }
          }
        }
      }
    stamp(5);
    return;
  }
  // c2 epilogue: bias, residual (x itself: L2-hot, this workgroup staged it a moment ago), length mask, store
  if (RESPF == 1) load_res();
#if defined(__HIP_DEVICE_COMPILE__)
  if (RESPF == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
#pragma unroll
  for (int m = 0; m < WM; ++m)
#pragma unroll
    for (int n = 0; n < WN; ++n) {
      const int col = wc * (WN * 32) + n * 32 + i;
      const int pos = n0 + col;
      if (col >= BN_OUT || pos >= a.T) continue;
      const bool live = pos < len;
      const int co_base = wr * (WM * 32) + m * 32 + 4 * h;
      float* yb = a.y ? a.y + (long)b * a.bs + pos : nullptr;
      float* y2b = a.acc2_mode != ACC2_NONE ? a.y2 + (long)b * a.bs + pos : nullptr;
#pragma unroll
      for (int r0 = 0; r0 < 16; r0 += 8) {
        float bv[8], rv[8], pv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int co = co_base + ((r0 + q) & 3) + 8 * ((r0 + q) >> 2);
          bv[q] = a.b2 ? a.b2[co] : 0.f;
          rv[q] = resv[m][n][r0 + q];
          pv[q] = (y2b && a.acc2_mode != ACC2_SET) ? y2b[(long)co * a.cs] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int co = co_base + ((r0 + q) & 3) + 8 * ((r0 + q) >> 2);
          float v = acc[m][n][r0 + q] * inv + bv[q];
          v = v + rv[q];
          v = live ? v : 0.f;
          if (yb) yb[(long)co * a.cs] = v;
          if (y2b) {
            float* p2 = y2b + (long)co * a.cs;
            if (a.acc2_mode == ACC2_SET) *p2 = v;
            else if (a.acc2_mode == ACC2_ADD) *p2 = pv[q] + v;
            else *p2 = (pv[q] + v) / a.acc2_div;
          }
        }
      }
    }
}

// ====================================================================================================================
// The PERSISTENT form of the fused step: the default where it is instantiated (aligned rows, C <= 128).
//
// Per-workgroup phase stamps of the kernel at the top of this file (tools/pair_trace.py) show how much of a
// tile's life is NOT in the two k-loops:   C = 128, k = 11: 9.5 of 94 us    C = 64, k = 3: 10.8 of 18.9 us
// C = 32, k = 3: 12.7 of 15.5 us -- launch + address set-up + the input tile's trip from HBM (2.2 - 5.7 us), the bias
// loads inside the c1 epilogue, and the residual's round trip inside the final epilogue (4.5 - 6.6 us).  None of it is
// work; all of it is latency that a workgroup with the CU to itself cannot hide.  Here a workgroup stays on its CU and
// walks a CONTIGUOUS range of tiles (XCD x owns a contiguous eighth of the tiles, its workgroups contiguous parts of
// that: neighbouring tiles share their halo in one L2, as before):
//   * the input tile of tile t + 1 is requested when tile t's c1 loop ends, converted and committed to LDS in the last
//     stage of tile t's c2 loop (the input staging area is idle in phase 2); its first weights are requested in that
//     stage too: the prologue of every tile but the first is a weight commit, not a round trip to HBM;
//   * the residual (the 16-byte-per-lane words of the wide epilogue) is requested in that same last stage and is there
//     when the epilogue asks for it;
//   * biases are read once per launch (into LDS; as registers they would cost 20 per lane and spill);
//   * no launch, no dispatch, no resource set-up per tile.
// The arithmetic is the first kernel's, instruction for instruction (same split, same k-order, same epilogues): the
// results are bit-identical to it and to the two conv launches (tests/test_gpu_conv.py: fused vs unfused, both forms).
// Tile t + 1's input is requested at the c1 epilogue and the first residual block in the last c2 stage, no earlier: vector
// memory loads return IN ORDER, so behind an earlier request the weight fetch of the next stage waits out the ~5 us HBM round
// trip of the input tile (measured slower on every multi-stage shape).
template <int C, int NT, int WR, int WC, int K, int KKT, int NCS>
__global__ __launch_bounds__(64 * WR * WC) void resblock_pair_persist_kernel(const PairArgs a) {
  constexpr int THREADS = 64 * WR * WC;
  constexpr int N1 = 32 * NT, N1P = N1 + kPairPadY, WROW = N1 + kPairHalo;
  constexpr int WM = (C / 32) / WR, WN = NT / WC;
  constexpr int NCHUNK = C / 16;
  constexpr int NG = (K + KKT - 1) / KKT;
  constexpr int SL = NCS * KKT;
  constexpr int A_ELEMS = SL * 4 * C, NA = (A_ELEMS + THREADS - 1) / THREADS;
  constexpr int B_TASKS = NCS * 2 * WROW, NBT = (B_TASKS + THREADS - 1) / THREADS;
  constexpr int BN_OUT = (N1 - (K - 1)) & ~3, H2 = (K - 1) / 2;
  static_assert(WM >= 1 && WN >= 1 && WM * WR * 32 == C && WN * WC == NT, "bad tile");
  static_assert(NCS == 1 || KKT == K, "several chunks per stage only with all taps resident");
  static_assert(NCHUNK % NCS == 0, "chunk sets must tile the channels");
  extern __shared__ uint4 lds[];
  constexpr int Y1_ELEMS = NCHUNK * 4 * N1P;
  uint4* Y1 = lds;                              // [chunk][op][h][N1P]
  uint4* As = Y1 + Y1_ELEMS;                    // [slot][op][h][C]
  uint4* Bs = As + A_ELEMS;                     // [cl][op][h][WROW]
  float* bias_s = reinterpret_cast<float*>(Bs + NCS * 4 * WROW);   // b1[C], b2[C]: read once per launch, 16-byte reads after

  // per-thread coordinates: NOT const -- they are re-derived at the top of every tile from an opaque copy of the thread id,
  // so that the hundred address terms built from them are recomputed per tile (a few dozen VALU instructions) instead of
  // being hoisted out of the tile loop and kept in registers for the whole launch (first build: 256 VGPRs + 28-154 spilled)
  int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int wr = wave / WC, wc = wave % WC;
  int i = lane & 31, h = lane >> 5;
  const int b = blockIdx.z;
  const int pad1 = (K - 1) * a.dil / 2;
  const int len = a.lens ? a.lens[b] : a.T;
  const int wuse = N1 + (K - 1) * a.dil;
  const float slope = a.slope;
  const H3Rsrc xr = h3_rsrc(a.x + (long)b * a.bs, C * a.cs * 4);
  const H3Rsrc w1r = h3_rsrc(a.w1, K * NCHUNK * 4 * C * 16);
  const H3Rsrc w2r = h3_rsrc(a.w2, K * NCHUNK * 4 * C * 16);
  const int xrow = a.cs * 4;
  constexpr int slab = 4 * C * 16;

  // ---- this workgroup's tiles: XCD (blockIdx.x & 7) owns a contiguous range, its workgroups contiguous parts of it
  int first, count;
  {
    const int nt = (a.T + BN_OUT - 1) / BN_OUT, nwg = gridDim.x, w = blockIdx.x;
    if (a.xcd_order && nwg >= 8) {
      const int x = w & 7, j = w >> 3;
      const int q = nt >> 3, r = nt & 7;
      const int x0 = x * q + (x < r ? x : r), xn = q + (x < r ? 1 : 0);          // tiles of this XCD
      const int m = (nwg >> 3) + (x < (nwg & 7) ? 1 : 0);                        // its workgroups
      const int q2 = xn / m, r2 = xn % m;
      first = x0 + j * q2 + (j < r2 ? j : r2);
      count = q2 + (j < r2 ? 1 : 0);
    } else {
      const int q = nt / nwg, r = nt % nwg;
      first = w * q + (w < r ? w : r);
      count = q + (w < r ? 1 : 0);
    }
  }
  if (count <= 0) return;
  const int ntiles_all = (a.T + BN_OUT - 1) / BN_OUT;
  int cur_tile = first;
  auto stamp = [&](int k) {
    if (a.trace && tid == 0) a.trace[((long)b * ntiles_all + cur_tile) * 8 + k] = (long long)wall_clock64();
  };

  f32x16 acc[WM][WN];
  auto zero_acc = [&]() {
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
      for (int n = 0; n < WN; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
  };

  int a_cl[NA], a_kkl[NA], a_off[NA];
  int b_off[NBT], b_row[NBT];
  int lr = 0, lc = 0;
  auto derive_thread = [&]() {
    int t0 = threadIdx.x;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(t0));                   // opaque: nothing derived from it is loop-invariant to the compiler
#endif
    tid = t0;
    lane = tid & 63;
    wave = tid >> 6;
    wr = wave / WC;
    wc = wave % WC;
    i = lane & 31;
    h = lane >> 5;
    lr = lane >> 3;
    lc = (lane & 7) * 4;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int e = tid + THREADS * j;
      const int co = e % C, rest = e / C;
      const int slot = rest / 4;
      a_cl[j] = slot / KKT;
      a_kkl[j] = slot % KKT;
      a_off[j] = e < A_ELEMS ? ((rest % 4) * C + co) * 16 : kH3Oob;
    }
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
      const int t = tid + THREADS * j;
      const int ch2 = t / WROW;
      b_row[j] = (ch2 >> 1) * 16 + (ch2 & 1) * 8;
    }
  };
  derive_thread();
  auto set_input_tile = [&](int tile) {           // where the input tasks of this thread read for `tile`
    const int in_base = tile * BN_OUT - H2 - pad1;
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
      const int t = tid + THREADS * j;
      const int ch2 = t / WROW, p = t - ch2 * WROW;
      const int pos = in_base + p;
      b_off[j] = (t < B_TASKS && p < wuse && pos >= 0 && pos < len) ? pos * 4 : kH3Oob;
    }
  };

  uint4 ra[NA];
  float rb[NBT][8];
  bool ovf = false;
  auto fetch_b = [&](int chunk0) {
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
      const int row0 = (chunk0 * 16 + b_row[j]) * xrow;
#pragma unroll
      for (int q = 0; q < 8; ++q) rb[j][q] = h3_load1(xr, b_off[j] == kH3Oob ? kH3Oob : row0 + q * xrow + b_off[j]);
    }
  };
  auto fetch_a = [&](const H3Rsrc& wr_, int chunk0, int kk0) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int kk = kk0 + a_kkl[j];
      const bool ok = a_off[j] != kH3Oob && kk < K;
      ra[j] = h3_load4(wr_, ok ? (kk * NCHUNK + chunk0 + a_cl[j]) * slab + a_off[j] : kH3Oob);
    }
  };
  auto commit_a = [&]() {
#pragma unroll
    for (int j = 0; j < NA; ++j)
      if (NA * THREADS == A_ELEMS || tid + THREADS * j < A_ELEMS) As[tid + THREADS * j] = ra[j];
  };
  auto commit_b = [&]() {
#pragma unroll
    for (int j = 0; j < NBT; ++j) {
      const int t = tid + THREADS * j;
      if (NBT * THREADS == B_TASKS || t < B_TASKS) {
        half8 hi, lo;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float v = rb[j][q];
          v = v > 0.f ? v : v * slope;                 // leaky_relu ahead of c1
          ovf |= !(fabsf(v) < kH3ActLimit);
          const _Float16 vh = (_Float16)v;
          hi[q] = vh;
          lo[q] = (_Float16)((v - (float)vh) * kH3Scale);
        }
        const int ch2 = t / WROW, p = t - ch2 * WROW;
        const int cl = ch2 >> 1, hh = ch2 & 1;
        Bs[((cl * 2 + 0) * 2 + hh) * WROW + p] = __builtin_bit_cast(uint4, hi);
        Bs[((cl * 2 + 1) * 2 + hh) * WROW + p] = __builtin_bit_cast(uint4, lo);
      }
    }
  };
  auto compute = [&](auto taps_tag, const uint4* Bt, int pitch, int cl_pitch, int kk0, int tap_step) {
    constexpr int TAPS = decltype(taps_tag)::value;
    constexpr int NS = NCS * TAPS;
    half8 af[2][2][WM], bf[2][2][WN];
    auto load = [&](int buf, int s) {
      const int cl = s / TAPS, kkl = s % TAPS;
      const int tp = (kk0 + kkl) * tap_step;
      const uint4* Bc = Bt + cl * cl_pitch;
#pragma unroll
      for (int m = 0; m < WM; ++m) {
        af[buf][0][m] = __builtin_bit_cast(half8, As[(((cl * KKT + kkl) * 2 + 0) * 2 + h) * C + wr * (WM * 32) + m * 32 + i]);
        af[buf][1][m] = __builtin_bit_cast(half8, As[(((cl * KKT + kkl) * 2 + 1) * 2 + h) * C + wr * (WM * 32) + m * 32 + i]);
      }
#pragma unroll
      for (int op = 0; op < 2; ++op)
#pragma unroll
        for (int n = 0; n < WN; ++n)
          bf[buf][op][n] = __builtin_bit_cast(half8, Bc[(op * 2 + h) * pitch + wc * (WN * 32) + n * 32 + i + tp]);
    };
    load(0, 0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int cur = s & 1;
      if (s + 1 < NS) load(cur ^ 1, s + 1);
#pragma unroll
      for (int m = 0; m < WM; ++m) {
        const half8 wh = af[cur][0][m] * (_Float16)(1.f / kH3Scale);
#pragma unroll
        for (int n = 0; n < WN; ++n) {
          acc[m][n] = h3_mfma(af[cur][0][m], bf[cur][0][n], acc[m][n]);   // (S wh) xh
          acc[m][n] = h3_mfma(wh, bf[cur][1][n], acc[m][n]);              // wh (S xl)
          acc[m][n] = h3_mfma(af[cur][1][m], bf[cur][0][n], acc[m][n]);   // (S wl) xh
        }
      }
    }
    {
      constexpr int R = 2 * WM + 2 * WN, M = 3 * WM * WN;
      __builtin_amdgcn_sched_group_barrier(0x100, R, 0);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          if (s + 1 < NS && j < R) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        if (s + 1 < NS && R > M) __builtin_amdgcn_sched_group_barrier(0x100, R - M, 0);
      }
    }
  };
  using Full = std::integral_constant<int, KKT>;
  using Last = std::integral_constant<int, K - (NG - 1) * KKT>;
  constexpr float inv = 1.f / kH3Scale;

  // biases, once per launch, into LDS (as registers they cost 20 per lane for the whole launch: spills)
  for (int c = tid; c < C; c += THREADS) {
    bias_s[c] = a.b1 ? a.b1[c] : 0.f;
    bias_s[C + c] = a.b2 ? a.b2[c] : 0.f;
  }

  // ---- first tile: its input chunk set 0 into Bs, its first weights into registers.  Loop invariant from here on:
  // at the top of a tile Bs holds the tile's chunk set 0 (converted), ra its first weight stage.
  set_input_tile(first);
  fetch_b(0);
  fetch_a(w1r, 0, 0);
  commit_b();

  for (int ti = 0; ti < count; ++ti) {
    const int tile = first + ti;
    cur_tile = tile;
    const int n0 = tile * BN_OUT;
    const bool has_next = ti + 1 < count;
    if (ti > 0) derive_thread();
    stamp(0);
    // ================================================================ phase 1: Y1 = lrelu(c1(lrelu(x)) + b1)
    zero_acc();
    for (int chunk = 0; chunk < NCHUNK; chunk += NCS) {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const bool last_stage = chunk + NCS >= NCHUNK && g == NG - 1;
        __syncthreads();
        if (g == 0 && chunk > 0) commit_b();           // chunk set 0 was committed by the previous tile (or the preamble)
        commit_a();
        __syncthreads();
        if (chunk == 0 && g == 0) stamp(1);
        if (!last_stage) fetch_a(w1r, g + 1 == NG ? chunk + NCS : chunk, g + 1 == NG ? 0 : (g + 1) * KKT);
        else fetch_a(w2r, 0, 0);                       // first weights of c2 fly during the c1 epilogue
        if (g == 0 && chunk + NCS < NCHUNK) fetch_b(chunk + NCS);
        if (NG > 1 && g == NG - 1) compute(Last{}, Bs, WROW, 4 * WROW, g * KKT, a.dil);
        else compute(Full{}, Bs, WROW, 4 * WROW, g * KKT, a.dil);
      }
    }
    stamp(2);
    if (has_next) {                                  // the staging registers are free: tile t + 1's input leaves HBM now
      set_input_tile(tile + 1);
      fetch_b(0);
    }
    // c1 epilogue: bias, leaky_relu (the one ahead of c2), zero outside the sequence, split, into LDS
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
      for (int n = 0; n < WN; ++n) {
        const int c_t = wr * (WM * 32) + m * 32;
        const int j = wc * (WN * 32) + n * 32 + i;
        const int pos1 = n0 - H2 + j;
        const bool live = pos1 >= 0 && pos1 < len;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          typedef _Float16 half4 __attribute__((ext_vector_type(4)));
          const int cg = c_t + 8 * g;
          half4 hi, lo;
          const float4 bq = *reinterpret_cast<const float4*>(bias_s + cg + 4 * h);
          const float b4[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float v = acc[m][n][4 * g + q] * inv + b4[q];
            v = fmaxf(v, v * slope);
            v = live ? v : 0.f;
            ovf |= !(fabsf(v) < kH3ActLimit);
            const _Float16 vh = (_Float16)v;
            hi[q] = vh;
            lo[q] = (_Float16)((v - (float)vh) * kH3Scale);
          }
          char* e_hi = reinterpret_cast<char*>(Y1 + (((cg >> 4) * 2 + 0) * 2 + (g & 1)) * N1P + j) + 8 * h;
          char* e_lo = reinterpret_cast<char*>(Y1 + (((cg >> 4) * 2 + 1) * 2 + (g & 1)) * N1P + j) + 8 * h;
          *reinterpret_cast<half4*>(e_hi) = hi;
          *reinterpret_cast<half4*>(e_lo) = lo;
        }
      }

    // ================================================================ phase 2: y = c2(Y1) + b2 + x
    zero_acc();
    stamp(3);
    // The residual words of the wide epilogue.  Column block n = 0 is requested in the last stage of the c2 loop, blocks
    // n >= 1 when the epilogue starts -- they land while block 0 is transposed and stored.  Half the registers of
    // requesting everything ahead.
    uint4 rv[WM][WN][4];
    auto request_res = [&](int n) {
#pragma unroll
      for (int m = 0; m < WM; ++m) {
        const int col0 = wc * (WN * 32) + n * 32 + lc;
        const int pos0 = n0 + col0;
        const bool ok = col0 < BN_OUT && pos0 < a.T;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int co = wr * (WM * 32) + m * 32 + lr + 8 * p;
          rv[m][n][p] = h3_load4(xr, ok ? (co * a.cs + pos0) * 4 : kH3Oob);
        }
      }
    };
    for (int chunk = 0; chunk < NCHUNK; chunk += NCS) {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const bool last_stage = chunk + NCS >= NCHUNK && g == NG - 1;
        __syncthreads();
        commit_a();
        if (last_stage && has_next) commit_b();        // Bs is idle in phase 2: tile t + 1's chunk set 0 is ready before its tile starts
        __syncthreads();
        if (!last_stage) fetch_a(w2r, g + 1 == NG ? chunk + NCS : chunk, g + 1 == NG ? 0 : (g + 1) * KKT);
        else if (has_next) fetch_a(w1r, 0, 0);       // tile t + 1's first weights
        if (last_stage) request_res(0);
        if (NG > 1 && g == NG - 1) compute(Last{}, Y1 + chunk * 4 * N1P, N1P, 4 * N1P, g * KKT, 1);
        else compute(Full{}, Y1 + chunk * 4 * N1P, N1P, 4 * N1P, g * KKT, 1);
      }
    }
    stamp(4);
    {
      constexpr int P = 36;                              // floats per staged row: 16-byte aligned, rows 4 banks apart
      static_assert(THREADS / 64 * 32 * P * 4 <= NCHUNK * 4 * N1P * 16, "staging tiles must fit the Y1 region");
      __syncthreads();                                   // every wave is done reading Y1: the staging tiles overlay it
      float* stg = reinterpret_cast<float*>(lds) + wave * (32 * P);
#pragma unroll
      for (int n = 1; n < WN; ++n) request_res(n);
#pragma unroll
      for (int n = 0; n < WN; ++n)
#pragma unroll
        for (int m = 0; m < WM; ++m) {
#pragma unroll
          for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * h) * P + i] = acc[m][n][r] * inv;
          __builtin_amdgcn_wave_barrier();
          const int col0 = wc * (WN * 32) + n * 32 + lc;
          const int pos0 = n0 + col0;
          const bool ok = col0 < BN_OUT && pos0 < a.T;
          float4 v[4], pv[4];
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const int co = wr * (WM * 32) + m * 32 + lr + 8 * p;
            const long off = (long)b * a.bs + (long)co * a.cs + pos0;
            v[p] = *reinterpret_cast<const float4*>(stg + (lr + 8 * p) * P + lc);
            pv[p] = (ok && a.acc2_mode != ACC2_NONE && a.acc2_mode != ACC2_SET) ? *reinterpret_cast<const float4*>(a.y2 + off)
                                                                                : make_float4(0.f, 0.f, 0.f, 0.f);
          }
          __builtin_amdgcn_wave_barrier();
          if (ok) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              const int co = wr * (WM * 32) + m * 32 + lr + 8 * p;
              const long off = (long)b * a.bs + (long)co * a.cs + pos0;
              const float bb = bias_s[C + co];
              const float4 rr = __builtin_bit_cast(float4, rv[m][n][p]);
              float o[4] = {v[p].x + bb + rr.x, v[p].y + bb + rr.y, v[p].z + bb + rr.z, v[p].w + bb + rr.w};
#pragma unroll
              for (int q = 0; q < 4; ++q) o[q] = pos0 + q < len ? o[q] : 0.f;
              if (a.y) *reinterpret_cast<float4*>(a.y + off) = make_float4(o[0], o[1], o[2], o[3]);
              if (a.acc2_mode != ACC2_NONE) {
                const float pp[4] = {pv[p].x, pv[p].y, pv[p].z, pv[p].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  if (a.acc2_mode == ACC2_ADD) o[q] = pp[q] + o[q];
                  else if (a.acc2_mode == ACC2_ADD_DIV) o[q] = (pp[q] + o[q]) / a.acc2_div;
                }
                *reinterpret_cast<float4*>(a.y2 + off) = make_float4(o[0], o[1], o[2], o[3]);
              }
            }
          }
        }
    }
    stamp(5);
  }
  if (ovf) report_h3_overflow(a.ovf, a.ovf_layer, a.seq);
}

enum PairForm { kPersist, kWide, kDword };
struct PairCfg {
  PairForm form;                 // kPersist / kWide: wide epilogue, rows must be 16-byte aligned
  int C, K, n1, threads, bn_out;
  size_t lds;
  void (*kern)(const PairArgs);
};
template <int C, int NT, int WR, int WC, int K, int KKT, int NCS, int RESPF>
constexpr PairCfg make_cfg() {
  constexpr size_t y1 = (size_t)(C / 16) * 4 * (32 * NT + kPairPadY), as = (size_t)NCS * KKT * 4 * C,
                   bs = (size_t)NCS * 4 * (32 * NT + kPairHalo);
  return {RESPF == 3 ? kWide : kDword, C, K, 32 * NT, 64 * WR * WC,
          RESPF == 3 ? ((32 * NT - (K - 1)) & ~3) : 32 * NT - (K - 1), (y1 + as + bs) * 16,
          resblock_pair_kernel<C, NT, WR, WC, K, KKT, NCS, RESPF>};
}
template <int C, int NT, int WR, int WC, int K, int KKT, int NCS>
constexpr PairCfg make_persist() {
  constexpr size_t y1 = (size_t)(C / 16) * 4 * (32 * NT + kPairPadY), as = (size_t)NCS * KKT * 4 * C,
                   bs = (size_t)NCS * 4 * (32 * NT + kPairHalo);
  return {kPersist, C, K, 32 * NT, 64 * WR * WC, (32 * NT - (K - 1)) & ~3, (y1 + as + bs) * 16 + 2 * C * 4,
          resblock_pair_persist_kernel<C, NT, WR, WC, K, KKT, NCS>};
}
// (C, K) instantiations of the RVC v2 decoders (resblock kernels 3 / 7 / 11); every tile fills a CU (one workgroup each)
const PairCfg kPair[] = {
    // ---- rows that are not 16-byte aligned: one workgroup per tile, dword epilogue; 512 threads at C <= 64
    make_cfg<32, 16, 1, 8, 3, 3, 2, 2>(),  make_cfg<32, 16, 1, 8, 7, 7, 1, 2>(),  make_cfg<32, 16, 1, 8, 11, 11, 1, 2>(),
    make_cfg<64, 8, 2, 4, 3, 3, 2, 2>(),   make_cfg<64, 8, 2, 4, 7, 7, 1, 2>(),   make_cfg<64, 8, 2, 4, 11, 11, 1, 2>(),
    // C = 128: k = 3 and k = 11 run 768 threads on N1 = 192 (three waves per SIMD: +12 % / +6 % in tools/bench_pair.py),
    // k = 7 keeps 512 threads with all 7 taps resident (the 768-thread form would spill)
    make_cfg<128, 6, 4, 3, 3, 3, 1, 2>(),  make_cfg<128, 4, 4, 2, 7, 7, 1, 2>(),  make_cfg<128, 6, 4, 3, 11, 4, 1, 1>(),
    // C = 256 (NSF stage 0): the c1 tile of all 256 channels is 1 KB per position, N1 = 96 fills the LDS (154 KB with two
    // weight taps resident); 12 waves of 64 x 32.  Only k = 3: at k = 7 / 11 the two conv_h3 launches are faster
    // (tools/bench_pair.py), find_cfg sends them there
    make_cfg<256, 3, 4, 3, 3, 2, 1, 1>(),
    // ---- aligned rows, C = 256: the same tile with the wide (LDS-transposed, 16 bytes per lane) epilogue
    make_cfg<256, 3, 4, 3, 3, 2, 1, 3>(),
    // ---- aligned rows, C <= 128: PERSISTENT workgroups on the tiles above, wide epilogue.  Measured per shape against one
    // workgroup per tile with the wide epilogue (tools/bench_pair.py, same box; profiles/pair_persist_r05.txt): k = 3
    // -11 ... -15 %, C = 32 -8 ... -12 %, C = 64 / 128 at k = 7 -4 ... -6 %, C = 64 k = 11 -3 %.
    make_persist<32, 16, 1, 8, 3, 3, 2>(),  make_persist<32, 16, 1, 8, 7, 7, 1>(),  make_persist<32, 16, 1, 8, 11, 11, 1>(),
    make_persist<64, 8, 2, 4, 3, 3, 2>(),   make_persist<64, 8, 2, 4, 7, 7, 1>(),   make_persist<64, 8, 2, 4, 11, 11, 1>(),
    // C = 128: k = 3 on 768 threads (12 waves of 32 x 64); k = 7 and k = 11 on 512 threads with N1 = 192 -- eight waves of 32 x 96
    // (WN = 3: eight fragment reads per nine product blocks), 220-235 registers: k = 7 -6 ... -10 % against N1 = 128 on 512
    // threads, k = 11 -3.5 % against 768 threads (168 registers: the persistent form spills inside its k-loops there)
    make_persist<128, 6, 4, 3, 3, 3, 1>(),  make_persist<128, 6, 4, 2, 7, 4, 1>(),  make_persist<128, 6, 4, 2, 11, 4, 1>(),
};
// rows 16-byte aligned: what the wide epilogue needs
bool pair_aligned(const PairArgs& a) {
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return a.cs % 4 == 0 && a.T % 4 == 0 && a.bs % 4 == 0 && al(a.x) && al(a.y) && al(a.y2);
}

const PairCfg* find_cfg(const PairArgs& a) {
  if (a.C == 256 && a.k != 3) return nullptr;            // k = 7 / 11 at C = 256: the two launches are faster (bench_pair)
  const PairForm form = !pair_aligned(a) ? kDword : (a.C <= 128 ? kPersist : kWide);
  for (const auto& c : kPair)
    if (c.form == form && c.C == a.C && c.K == a.k) return &c;
  return nullptr;
}

}  // namespace

bool resblock_pair_enabled() {
  static const int mode = getenv("RVCX_FUSE") ? atoi(getenv("RVCX_FUSE")) : 1;
  return mode != 0 && conv_h3_enabled();
}

bool resblock_pair_ok(const PairArgs& a) {
  if (!resblock_pair_enabled() || !a.w1 || !a.w2) return false;
  if (a.dil < 1 || a.dil > 5 || (a.k - 1) * a.dil > kPairHalo - 14) return false;
  if ((long)a.C * a.cs * 4 >= kH3Oob || (long)a.k * a.C * a.C * 4 >= kH3Oob) return false;
  return find_cfg(a) != nullptr;
}

int resblock_pair_slot(int C) { return C == 32 ? 50 : (C == 64 ? 51 : (C == 128 ? 52 : 58)); }

void resblock_pair_describe(ConvProfile* p) {
  for (const auto& c : kPair) {
    if (c.form != kDword) continue;            // one report per slot: the tile of the last dword row of that C
    const int s = resblock_pair_slot(c.C);
    p->bm[s] = c.C;
    p->bn[s] = c.n1;
    p->halo[s] = 500000 + c.C;
  }
}

void resblock_pair_init() {      // once per device, also when several contexts start on different threads
  static std::mutex mu;
  static uint64_t done = 0;
  int dev = 0;
  RVCX_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  if ((done >> (dev & 63)) & 1) return;
  for (const auto& c : kPair)
    RVCX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(c.kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)c.lds));
  done |= 1ull << (dev & 63);
}

void launch_resblock_pair(const PairArgs& a, hipStream_t stream) {
  RVCX_CHECK(resblock_pair_ok(a), "resblock pair: unsupported shape");
  RVCX_CHECK(a.y != a.x && a.y2 != a.x, "resblock pair: in-place operation is a race (halo reads vs neighbours' stores)");
  resblock_pair_init();
  const PairCfg& c = *find_cfg(a);
  const int bn_out = c.bn_out;
  dim3 grid(cdiv(a.T, bn_out), 1, a.B);
  if (c.form == kPersist) {                  // at most one workgroup per CU, each walks a range of tiles
    static const int ncu = [] {
      int dev = 0, n = 256;
      if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
      return std::max(8, n);
    }();
    grid.x = std::min<unsigned>(grid.x, (unsigned)ncu);
  }
  static const int xcd = getenv("RVCX_PAIR_XCD") ? atoi(getenv("RVCX_PAIR_XCD")) : 1;
  PairArgs b = a;
  b.xcd_order = xcd;
  hipLaunchKernelGGL(c.kern, grid, dim3(c.threads), c.lds, stream, b);
  RVCX_HIP(hipGetLastError());
}

}  // namespace rvcx
