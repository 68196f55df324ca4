// wgrad.hip -- the weight gradients of the LSTM nets: C[M,N] += A[K,M]^T . B[K,N] with K = T*B (40,960 at the bench shape,
// 81,920 at the f32 parity mode's configs[4]), M = 4H gate columns, N = H or I input columns; f32 accumulation.  (No reference
// counterpart: the reference's model is FC and its autograd computes `dy^T x` with ATen, simple_fhvae.py:127-134,
// train_model.py:452.)  One kernel template over an element-traits struct: bf16 operands (WgBf16) or f32 operands (WgF32).
//
// Why a kernel of its own: both operands are K-MAJOR (the contraction index is the row of dgates / of the saved states), the
// outputs are small (1 MB) and the contraction is long, so the GEMM is bound by how many operand bytes a CU pulls from L2 per
// FLOP and by the split-K partial sums.  The generic engine (gemm_core.h: 4 waves, 128x64 tiles, register staging, padded LDS
// image) ran it at 445 TFLOP/s with 512 workgroups x 32 KB of f32 atomics per GEMM, one launch per weight matrix.  Here:
//   * 256 x 256 (or 256 x 128 for N <= 128) output tile per 512-thread workgroup: 8 waves as 2 (m) x 4 (n), 128 x 64 per wave,
//     128 accumulator registers -- a quarter of the L2 -> LDS bytes per FLOP of the 128x64 tiles;
//   * operands go global -> LDS by LDS-DMA (buffer_load ... lds, 16 B per lane, 1 KiB per wave-instruction), two stages of BK
//     k-rows; the loads of stage s+1 stay in flight under the MFMAs of stage s behind a COUNTED s_waitcnt vmcnt(n) and raw
//     s_barriers (guide: "Pipelining across barriers"); buffer range checking zero-fills the k rows past K, so any K works;
//   * the LDS image keeps the memory layout [k][column] (the DMA cannot transpose); the k-rows that one fragment read touches
//     are spread over the banks by an XOR of the row's chunk index with the low bits of k -- applied to the per-lane SOURCE
//     address of the DMA and to the read address (guide rule 21): conflict-free;
//   * ALL weight matrices of ALL nets of a step go out as ONE launch (fhvae_lstm_param_grads_multi): 36 tiles x split-K 7 = 252
//     workgroups at the bench shape instead of 12 launches x 512 workgroups; the f32 atomics (the chip adds ~1.3 TB/s) drop
//     from 12 x 16.8 MB to 63 MB per step.
// What the element decides (the traits below, nothing else):
//   * bf16: 64-k stages, v_mfma_f32_16x16x32_bf16; rows are 512 B = two bank rows, the 32-byte segment index of a row is
//     XOR-ed with (k & 7), so the 8 k-rows a 32-lane half touches land on 8 different 32-byte slots of the 256-byte bank row;
//     fragments by ds_read_b64_tr_b16 (hardware transpose, guide T10); s_setprio around each MFMA block;
//   * f32: 32-k stages, v_mfma_f32_16x16x4_f32 (every product and every accumulation step an f32 fma, like the autograd
//     contraction it replaces); an operand is ONE float per lane (A[m = lane & 15][k = lane >> 4]), i.e. 16 consecutive floats
//     of each of 4 consecutive k-rows: the 64-byte group index of a row is XOR-ed with (k & 3), so the four rows fall into four
//     different 16-bank ranges; per 4-k block a wave reads 8 + 4 scalars (ds_read_b32) for 32 MFMAs of 32 cycles, so the LDS
//     is idle next to the matrix pipe (the generic engine's 64 x 64 tiles read one scalar per MFMA).
#include "wgrad.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "gemm_core.h"

namespace fh {

constexpr int kWgThreads = 512, kWgBM = 256, kMaxWgProblems = FHVAE_WGRAD_MAX_PROBLEMS;

struct WgBf16 {
  using T = u16;
  using Frag = bf16x8;
  static constexpr int BK = 64, KB = 32;         // k-rows per stage / per MFMA block
  static constexpr bool kSetprio = true;         // s_setprio around the MFMA block
  static constexpr unsigned kOob = 0x40000000u;  // a buffer offset >= num_records: operands stay below kMaxBytes
  static constexpr int64_t kMaxBytes = 1LL << 30;
  static constexpr double kRate = 1.0e15;        // FLOP/s of the chip in the split-K model
  // the logical 16-byte chunk whose bytes fill physical chunk pc of k-row `row`
  static __device__ __forceinline__ int swizzle(int pc, int row) { return (((pc >> 1) ^ (row & 7)) << 1) | (pc & 1); }
  // a lane reads k-row 4g + (i >> 2) of the 32-k block, 32-byte segment (col0 / 16) ^ (k & 7), 8 bytes per lane
  static constexpr int kXor = 7, kSegShift = 5;
  static __device__ __forceinline__ int krow(int gq, int i) { return 4 * gq + (i >> 2); }
  static __device__ __forceinline__ int sub(int i) { return 8 * (i & 3); }
  // 8 k-values of one column: k rows 4g..4g+3 and 16+4g..16+4g+3 of the 32-k block (the same permutation of k for A and B)
  template <int RB>
  static __device__ __forceinline__ Frag read(const char* a0) {
    typedef s16x4 __attribute__((address_space(3))) * lds_p;
    union {
      struct {
        s16x4 lo, hi;
      } s;
      bf16x8 v;
    } u;
    u.s.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a0));
    u.s.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a0 + 16 * RB));
    return u.v;
  }
  static __device__ __forceinline__ f32x4 mfma(Frag a, Frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

struct WgF32 {
  using T = float;
  using Frag = float;
  static constexpr int BK = 32, KB = 4;
  static constexpr bool kSetprio = false;
  static constexpr unsigned kOob = 0x7ffffff0u;
  static constexpr int64_t kMaxBytes = 0x7ffffff0LL;
  static constexpr double kRate = 140.0e12;  // the f32 MFMA rate
  static __device__ __forceinline__ int swizzle(int pc, int row) { return (((pc >> 2) ^ (row & 3)) << 2) | (pc & 3); }
  // k-row gq of the 4-k block (k & 3 == gq: the blocks start at multiples of 4), 16-float group = the 16-wide tile
  static constexpr int kXor = 3, kSegShift = 6;
  static __device__ __forceinline__ int krow(int gq, int i) { return gq; }
  static __device__ __forceinline__ int sub(int i) { return i * 4; }
  template <int RB>
  static __device__ __forceinline__ Frag read(const char* a0) {
    return *(const float*)a0;
  }
  static __device__ __forceinline__ f32x4 mfma(Frag a, Frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};
template <class T>
using WgElem = std::conditional_t<std::is_same<T, u16>::value, WgBf16, WgF32>;

template <class E>
struct WgGroupT {
  int n;
  int base[kMaxWgProblems + 1];  // problem i owns the logical workgroups [base[i], base[i+1])
  WgProblemT<typename E::T> p[kMaxWgProblems];
};

template <class E, int W>  // operand tile width in elements
struct WgImg {
  static constexpr int RB = W * (int)sizeof(typename E::T);  // bytes per k-row of the image
  static constexpr int BYTES = E::BK * RB;                   // one stage
  static constexpr int CPR = RB / 16;                        // 16-byte chunks per row
  static constexpr int RPI = 1024 / RB;                      // k-rows written by one wave-instruction
  static constexpr int NI = BYTES / 1024 / 8;                // wave-instructions per wave and stage
};

typedef void __attribute__((address_space(3))) * lds_void_p;

// per-lane byte offsets (relative to the stage's first k-row) of this wave's DMA pieces: row * ld + swizzled chunk
template <class E, int W, int NI>
__device__ __forceinline__ void wg_dma_offsets(unsigned (&voff)[NI], unsigned ld_bytes, int wave, int lane) {
  using I = WgImg<E, W>;
#pragma unroll
  for (int q = 0; q < I::NI; ++q) {
    const int row = (wave * I::NI + q) * I::RPI + lane / I::CPR;
    const int pc = lane % I::CPR;  // physical 16-byte chunk of the LDS row this lane fills
    voff[q] = (unsigned)row * ld_bytes + (unsigned)E::swizzle(pc, row) * 16u;
  }
}

template <class E, int W, int NI>
__device__ __forceinline__ void wg_issue(char* stage, __amdgpu_buffer_rsrc_t rs, const unsigned (&voff)[NI], unsigned kbase, int wave) {
  using I = WgImg<E, W>;
#pragma unroll
  for (int q = 0; q < I::NI; ++q)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_p)(stage + (wave * I::NI + q) * 1024), 16, voff[q] + kbase, 0, 0, 0);
}

// The DMA pieces of the next stage are issued in two halves (A behind the first MFMA block's fragment reads, B behind the middle
// one's: their issue cost then overlaps the LDS latency), plain vmcnt(0) at the top of the next step (they have had a whole step
// to land).  Measured at 4096^3 bf16 (64 steps per workgroup + 67 MB of epilogue): 159-164 us; all pieces at the top of a step
// behind a counted wait: 173 us; no DMA in the loop at all: 141 us; DMA only: 98 us -- the fragment-read + MFMA phases between
// the two barriers of a step bound the loop (~970 TFLOP/s with no DMA); a software pipeline over the (32-k block, m-tile) groups
// pinned with sched_group_barrier was no faster (173 us).
template <class E, int BN>
__global__ __launch_bounds__(kWgThreads) void wgrad_kernel(WgGroupT<E> g) {
  using T = typename E::T;
  using IA = WgImg<E, kWgBM>;
  using IB = WgImg<E, BN>;
  constexpr int STAGE = IA::BYTES + IB::BYTES;
  constexpr int TM = 8, TN = BN / 64;
  constexpr int BK = E::BK, NJ = BK / E::KB;
  // TWO LDS objects, one per stage, and the K loop written out for both: hipcc then knows (alias scopes of the two
  // variables) that the fragment reads of one stage cannot alias the DMA in flight into the other and emits a COUNTED
  // s_waitcnt vmcnt(n) in front of them; with one array (or a runtime stage index) it drains every LDS-DMA (vmcnt(0)) before
  // the first ds_read of each step and the loads never overlap the MFMAs
  __shared__ __attribute__((aligned(1024))) char stage0[STAGE];
  __shared__ __attribute__((aligned(1024))) char stage1[STAGE];

  // XCD-aware order (guide T1, bijective form): each XCD gets a contiguous range of logical workgroups; the m-tiles of one
  // (problem, K slice, n-tile) are adjacent, so the B panel they share is fetched into one L2 (speed only)
  int wg = blockIdx.x;
  {
    const int nb = gridDim.x;
    if (nb >= 16) {
      const int q = nb >> 3, r = nb & 7, xcd = wg & 7;
      wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (wg >> 3);
    }
  }
  int pi = 0;
  while (pi + 1 < g.n && wg >= g.base[pi + 1]) ++pi;
  const WgProblemT<T>& p = g.p[pi];
  const int local = wg - g.base[pi];
  const int mt = local % p.m_tiles, nt = (local / p.m_tiles) % p.n_tiles, sp = local / (p.m_tiles * p.n_tiles);
  const int ks_total = (p.K + BK - 1) / BK;
  const int ks0 = sp * p.ksteps_per, ks1 = min(ks_total, ks0 + p.ksteps_per);
  if (ks0 >= ks1) return;
  const int m0 = mt * kWgBM, n0 = nt * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int gq = lane >> 4, i = lane & 15;

  // buffer descriptors from the tile's first column: offsets past the last valid k-row read as zero (K tail); columns past
  // M / N inside a row read the neighbouring bytes (in bounds) and only feed output columns that are never stored
  constexpr unsigned ES = sizeof(T);
  const unsigned lda_b = (unsigned)p.lda * ES, ldb_b = (unsigned)p.ldb * ES;
  const __amdgpu_buffer_rsrc_t rsa =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p.A + m0), 0, (int)(((int64_t)p.K * p.lda - p.a_col0 - m0) * ES), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsb =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p.B + n0), 0, (int)(((int64_t)p.K * p.ldb - n0) * ES), 0x00020000);
  unsigned va[IA::NI], vb[IB::NI];
  wg_dma_offsets<E, kWgBM>(va, lda_b, wave, lane);
  wg_dma_offsets<E, BN>(vb, ldb_b, wave, lane);

  // fragment read offsets: the lane's k-row, the segment of its 16-column tile XOR-ed with the row's key
  const int kr = E::krow(gq, i), x = kr & E::kXor;
  int offa[TM], offb[TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm) offa[tm] = kr * IA::RB + (((wm * 8 + tm) ^ x) << E::kSegShift) + E::sub(i);
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) offb[tn] = kr * IB::RB + (((wn * TN + tn) ^ x) << E::kSegShift) + E::sub(i);

  f32x4 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

  // (always_inline: the f32 body of `compute` is 256 MFMAs; left as a call, its closure -- and with it the accumulators -- lived
  // in scratch)
  // byte offset of k-step ks (uniform)
  auto kofs = [&](int ks, unsigned ld_b) __attribute__((always_inline)) -> unsigned { return (unsigned)(ks * BK) * ld_b; };
  auto compute = [&](const char* As, char* nxt, int ks_next) __attribute__((always_inline)) {
    const char* Bs = As + IA::BYTES;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      typename E::Frag a[TM], b[TN];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) b[tn] = E::template read<IB::RB>(Bs + offb[tn] + j * E::KB * IB::RB);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) a[tm] = E::template read<IA::RB>(As + offa[tm] + j * E::KB * IA::RB);
      if (j == 0 || j == NJ / 2) {  // this half of the next stage's DMA pieces: issued while the fragment reads are in flight
        // k-steps past this workgroup's slice load from an offset beyond the descriptors' range: zeros
        const bool in = ks_next < ks1;
        if (j == 0)
          wg_issue<E, kWgBM>(nxt, rsa, va, in ? kofs(ks_next, lda_b) : E::kOob, wave);
        else
          wg_issue<E, BN>(nxt + IA::BYTES, rsb, vb, in ? kofs(ks_next, ldb_b) : E::kOob, wave);
      }
      if (E::kSetprio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = E::mfma(a[tm], b[tn], acc[tm][tn]);
      if (E::kSetprio) __builtin_amdgcn_s_setprio(0);
    }
  };
  // One K-step: the next stage's DMA stays in flight under this stage's MFMAs (its buffer was released by the barrier that ended
  // the previous step).  The loop body is branch-free and handles two steps (one per LDS object): an odd slice gets one padding
  // step whose operands are the zeros of out-of-range loads, and the look-ahead DMA of the last step is such a zero fill too.
  auto step = [&](const char* cur, char* nxt, int ks_next) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's pieces of the current stage have landed
    compute(cur, nxt, ks_next);
    __builtin_amdgcn_s_barrier();  // every wave is done reading it: the next step may refill it
  };
  wg_issue<E, kWgBM>(stage0, rsa, va, kofs(ks0, lda_b), wave);
  wg_issue<E, BN>(stage0 + IA::BYTES, rsb, vb, kofs(ks0, ldb_b), wave);
  for (int ks = ks0; ks < ks1; ks += 2) {
    step(stage0, stage1, ks + 1);
    step(stage1, stage0, ks + 2);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last look-ahead DMA (zeros) must land before the LDS is released

  // split-K partial tile -> f32 atomics: a 16-lane group adds 64 contiguous bytes of one output row per instruction
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int n = n0 + wn * (BN / 4) + tn * 16 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 128 + tm * 16 + 4 * gq + r;
        if (m < p.M && n < p.N) {
          float* c = p.C + (int64_t)m * p.ldc + n;
          if (p.splitk == 1 && !p.shared_c)
            *c += acc[tm][tn][r];  // the only workgroup on this tile: plain read-modify-write (the atomic path adds ~1.3 TB/s)
          else
            atomicAdd(c, acc[tm][tn][r]);
        }
      }
    }
}

template __global__ void wgrad_kernel<WgBf16, 256>(WgGroupT<WgBf16>);
template __global__ void wgrad_kernel<WgBf16, 128>(WgGroupT<WgBf16>);
template __global__ void wgrad_kernel<WgF32, 256>(WgGroupT<WgF32>);
template __global__ void wgrad_kernel<WgF32, 128>(WgGroupT<WgF32>);

template <class T>
bool wgrad_eligible(const WgProblemT<T>& p) {
  using E = WgElem<T>;
  constexpr int64_t ES = sizeof(T);
  if (p.M <= 0 || p.N <= 0 || p.K <= 0 || !p.A || !p.B || !p.C) return false;
  if ((((uintptr_t)p.A) | ((uintptr_t)p.B)) & 15) return false;
  if ((p.lda % (16 / ES)) || (p.ldb % (16 / ES)) || p.lda < p.a_col0 + p.M || p.ldb < p.N || p.a_col0 < 0) return false;
  // 32-bit buffer offsets / num_records
  if ((int64_t)p.K * p.lda * ES >= E::kMaxBytes || (int64_t)p.K * p.ldb * ES >= E::kMaxBytes) return false;
  return true;
}

// One launch of the plan: the K slices of its problems (all of the tile class l.BN) and the grid.
// One launch is about one workgroup per CU: the K slices are what is left after the tiles.
template <class T>
static void plan_launch(const WgProblemT<T>* ps, fhvae_wgrad_plan& l) {
  using E = WgElem<T>;
  int64_t tiles = 0, ks_max = 1;
  for (int k = 0; k < l.n; ++k) {
    const WgProblemT<T>& p = ps[l.p[k].which];
    tiles += fh_cdiv(p.M, kWgBM) * fh_cdiv(p.N, l.BN);
    ks_max = std::max<int64_t>(ks_max, fh_cdiv(p.K, E::BK));
  }
  // K slices: every extra slice adds a tile of f32 atomics per output tile (the chip adds ~1.3 TB/s, guide: global float
  // atomics) and shortens the slices; pick the count that minimises  waves x steps x t_step + atomic bytes / rate
  // (t_step: one BK-k step of a workgroup at the element's MFMA rate over 256 CUs)
  const double t_step = 2.0 * kWgBM * l.BN * E::BK / (E::kRate / 256), tile_bytes = 4.0 * kWgBM * l.BN;
  int64_t sk = 1;
  double best = 1e30;
  for (int64_t c = 1; c <= 64 && c * 2 <= ks_max; ++c) {
    const double waves = (double)fh_cdiv(tiles * c, 256), steps = (double)fh_cdiv(ks_max, c) + 2.0;
    const double t = waves * steps * t_step + (c > 1 ? tiles * c * tile_bytes / 1.3e12 : 0.0);
    if (t < best) best = t, sk = c;
  }
  l.sk = (int)sk;
  for (int k = 0; k < l.n; ++k) {
    auto& q = l.p[k];
    const WgProblemT<T>& p = ps[q.which];
    q.m_tiles = (int)fh_cdiv(p.M, kWgBM);
    q.n_tiles = (int)fh_cdiv(p.N, l.BN);
    const int64_t ks_total = fh_cdiv(p.K, E::BK);
    int64_t s = sk;
    if (s > ks_total / 2) s = ks_total / 2;
    if (s < 1) s = 1;
    q.ksteps_per = (int)fh_cdiv(ks_total, s);
    q.splitk = (int)fh_cdiv(ks_total, q.ksteps_per);
    l.grid += q.m_tiles * q.n_tiles * q.splitk;
    // two problems of one launch that accumulate into the same matrix (a net queued twice: gradient accumulation over two
    // backward passes before one optimizer step) must not take the plain read-modify-write path
    for (int b = 0; b < l.n; ++b)
      if (b != k && ps[l.p[b].which].C == p.C) q.shared_c = 1;
  }
}

// The launch plan of a call: its launches in launch order -- the problems with N > 128 (BN = 256) in chunks of kMaxWgProblems,
// then the others (BN = 128) -- into out[cap]; returns their number.  Host arithmetic on sizes, alignments and the equality of
// the C pointers; fhvae_plan_wgrad hands it to a caller, launch_wgrad launches it.
template <class T>
static int plan_wgrad(const WgProblemT<T>* ps, int n, fhvae_wgrad_plan* out, int cap) {
  if (n > 256) return FHVAE_ERR_LIMIT;
  for (int k = 0; k < n; ++k)
    if (!wgrad_eligible(ps[k])) return FHVAE_ERR_ALIGN;
  int launches = 0;
  for (const int BN : {256, 128}) {
    fhvae_wgrad_plan* l = nullptr;
    for (int k = 0; k < n; ++k) {
      if ((ps[k].N > 128) != (BN == 256)) continue;
      if (!l || l->n == kMaxWgProblems) {
        if (launches == cap) return FHVAE_ERR_LIMIT;
        l = &out[launches++];
        *l = {};
        l->BN = BN;
      }
      l->p[l->n++].which = k;
    }
  }
  for (int i = 0; i < launches; ++i) plan_launch(ps, out[i]);
  return launches;
}

template <class T, int BN>
static int launch_class(const WgProblemT<T>* ps, const fhvae_wgrad_plan& l, hipStream_t st) {
  WgGroupT<WgElem<T>> g = {};
  g.n = l.n;
  for (int k = 0; k < l.n; ++k) {
    const auto& q = l.p[k];
    WgProblemT<T>& p = g.p[k] = ps[q.which];
    p.m_tiles = q.m_tiles, p.n_tiles = q.n_tiles, p.ksteps_per = q.ksteps_per, p.splitk = q.splitk;
    if (q.shared_c) p.shared_c = 1;
    g.base[k + 1] = g.base[k] + q.m_tiles * q.n_tiles * q.splitk;
  }
  hipLaunchKernelGGL((wgrad_kernel<WgElem<T>, BN>), dim3((unsigned)l.grid), dim3(kWgThreads), 0, st, g);
  return fh_launch_status();
}

template <class T>
int launch_wgrad(const WgProblemT<T>* ps, int n, hipStream_t st) {
  if (n <= 0) return FHVAE_OK;
  constexpr int kMaxLaunches = 256 / kMaxWgProblems + 1;  // of 256 problems in two tile classes
  fhvae_wgrad_plan pl[kMaxLaunches];
  const int launches = plan_wgrad(ps, n, pl, kMaxLaunches);
  for (int i = 0; i < launches; ++i) {
    const int e = pl[i].BN == 256 ? launch_class<T, 256>(ps, pl[i], st) : launch_class<T, 128>(ps, pl[i], st);
    if (e) return e;
  }
  return launches < 0 ? launches : FHVAE_OK;
}

template bool wgrad_eligible<u16>(const WgProblem&);
template bool wgrad_eligible<float>(const WgProblem32&);
template int launch_wgrad<u16>(const WgProblem*, int, hipStream_t);
template int launch_wgrad<float>(const WgProblem32*, int, hipStream_t);

}  // namespace fh

using namespace fh;

template <class T>
static int wgrad_entry(const T* a, int64_t lda, const T* b, int64_t ldb, float* c, int64_t ldc, int64_t M, int64_t N, int64_t K, void* stream) {
  FH_CHECK_PTR(a);
  FH_CHECK_PTR(b);
  FH_CHECK_PTR(c);
  FH_CHECK_POS(M);
  FH_CHECK_POS(N);
  FH_CHECK_POS(K);
  FH_CHECK_I32(M);
  FH_CHECK_I32(N);
  FH_CHECK_I32(K);
  WgProblemT<T> p = {};
  p.A = a, p.B = b, p.C = c;
  p.lda = lda, p.ldb = ldb, p.ldc = ldc;
  p.M = (int)M, p.N = (int)N, p.K = (int)K;
  if (!wgrad_eligible(p)) return FHVAE_ERR_ALIGN;
  return launch_wgrad(&p, 1, (hipStream_t)stream);
}

template <class T>
static int plan_descs(const fhvae_wgrad_desc* x, int n, fhvae_wgrad_plan* out, int cap) {
  std::vector<WgProblemT<T>> ps(n, WgProblemT<T>{});
  for (int i = 0; i < n; ++i) {
    for (const int64_t v : {x[i].M, x[i].N, x[i].K, x[i].a_col0})
      if (v != (int)v) return FHVAE_ERR_LIMIT;
    ps[i].A = (const T*)x[i].a, ps[i].B = (const T*)x[i].b, ps[i].C = x[i].c;
    ps[i].lda = x[i].lda, ps[i].ldb = x[i].ldb, ps[i].ldc = x[i].ldc;
    ps[i].M = (int)x[i].M, ps[i].N = (int)x[i].N, ps[i].K = (int)x[i].K, ps[i].a_col0 = (int)x[i].a_col0;
  }
  return plan_wgrad(ps.data(), n, out, cap);
}

extern "C" int fhvae_plan_wgrad(const fhvae_wgrad_desc* x, int n, int dtype, fhvae_wgrad_plan* out, int cap) {
  if (n <= 0) return 0;
  FH_CHECK_PTR(x);
  FH_CHECK_PTR(out);
  if (dtype != FHVAE_F32 && dtype != FHVAE_BF16) return FHVAE_ERR_DTYPE;
  return dtype == FHVAE_BF16 ? plan_descs<u16>(x, n, out, cap) : plan_descs<float>(x, n, out, cap);
}

// C[M,N] (f32, ldc) += A[K,M]^T . B[K,N]: operands with the contraction index as the ROW of both (lda, ldb in elements, multiples
// of 16 bytes; 16-byte aligned bases).  The weight-gradient contraction of a linear / LSTM layer over K = batch x time rows
// (dW += dY^T X; nn.Linear's backward at simple_fhvae.py:127-134, torch.nn.LSTM's for the stub fhvae.py:14, autograd's at
// train_model.py:452).  bf16 operands ...
extern "C" int fhvae_wgrad_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, float* c, int64_t ldc, int64_t M, int64_t N,
                                int64_t K, void* stream) {
  return wgrad_entry((const u16*)a, lda, (const u16*)b, ldb, c, ldc, M, N, K, stream);
}

// ... and f32 operands on the exact-f32 MFMA
extern "C" int fhvae_wgrad_f32(const float* a, int64_t lda, const float* b, int64_t ldb, float* c, int64_t ldc, int64_t M, int64_t N,
                               int64_t K, void* stream) {
  return wgrad_entry(a, lda, b, ldb, c, ldc, M, N, K, stream);
}
