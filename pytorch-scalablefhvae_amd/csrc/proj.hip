// proj.hip -- C[M,N] = A[M,K] . B[N,K]^T (+ bias): bf16 operands with the contraction index CONTIGUOUS in both (activations
// times a weight matrix as torch.nn.Linear / torch.nn.LSTM store it), f32 accumulate, f32 output.  M = T*B rows (40,960 at
// the bench shape), N and K a few hundred: the projections around the recurrences --
//   * the from-above term of the LSTM backward, dh^{l}_t += dg^{l+1}_t . W_ih[l+1] for all t at once (M = T*B, K = 4H, N = H;
//     operand B = the transposed bf16 weight copy [H,4H] of the workspace), between the two per-layer launches of a net
//     (lstm_bwd_rs.hip; the body the reference never wrote, fhvae.py:14);
// Why a kernel of its own: the generic engine (gemm_core.h: 4 waves, 64x64 tiles, one workgroup-wide barrier pair per 32 k)
// ran this shape at 325 TFLOP/s (66 us); a prologue of the persistent launch that computed it per cluster member re-read the
// operand four times and took 70 us.  Here:
//   * ONE tile per CU: the row tile BM is chosen so that ceil(M / BM) is about the CU count (BM = 160 at M = 40,960: 256 tiles;
//     256-row tiles would leave 96 CUs idle), all N columns per tile (BN = 256 or 128): A is read exactly once;
//   * 512 threads = 8 waves as 2 (m) x 4 (n); operands go global -> LDS by LDS-DMA (8 rows x 128 B per wave-instruction, whole
//     lines) into two rings of 64-k slots, one per operand and one LDS object per slot (PjRing: (3,3) at the bench tile), with
//     counted waits and ONE raw barrier per k-step: a step waits for the stage it is about to read only, every younger stage
//     stays in flight, and the slots freed one step earlier are refilled behind the fragment reads;
//   * LDS image [row][8 chunks] with the 16-byte chunk XOR-ed by (row & 7) on the DMA's per-lane source and on the ds_read_b128
//     (conflict-free for 128-byte rows: the two rows of a bank row take opposite halves);
//   * MFMA roles swapped (weight fragment first): a lane holds 4 consecutive columns of one row -> 16-byte f32 stores.
#include "proj.h"

#include <cstdlib>
#include <type_traits>

#include "gemm_core.h"

namespace fh {

constexpr int kPjThreads = 512;
typedef void __attribute__((address_space(3))) * lds_void_p;

struct ProjArgs {
  const u16* A;
  const u16* B;
  float* C;
  const float* bias;   // [N] or NULL
  const float* bias2;  // columns >= bias_split take bias2[n - bias_split] (two heads side by side); NULL: one vector
  int bias_split;
  int64_t lda, ldb, ldc;
  int M, N, K;
  // Non-temporal stores of C: set for a launch of one round of tiles (at most one per CU), the c3 step's five launches among
  // them.  Measured: the c3 step is faster with it in every round of two runs of five alternating rounds, by 0.2 - 0.5 % (the five
  // launches 134 -> 129 us per step; the readers' times do not move: the lower layer's recurrence loads the from-above term with nt
  // hints too).  Back to back, 40,960 x 256 x 1024 28.6 -> 28.0 us, x 160 x 256 12.9 -> 11.6 us; of two four-round shapes
  // 81,920 x 512 x 2048 gains (239 -> 211 us) and 40,960 x 1024 x 256 (168 MB of output for 21 MB of input) loses (53 -> 66 - 81 us),
  // so launches of more rounds than one keep their plain stores.
  int nt;
};

constexpr unsigned kPjOob = 0x80000000u;  // a byte offset no buffer of proj_eligible reaches (num_records < 2^31): reads as zeros

// The ring depths of a tile shape: the deepest of (4,3), (3,3), (3,2), (2,2) 64-k slots (A, B) that fits the CU's 160 KB of LDS.
//   * NSB <= NSA <= NSB + 1: vmcnt retires in issue order, so the wait that covers this step's B slot also covers every A piece
//     issued before it, and an A ring more than one slot deeper than the B ring buys no latency.  Measured at <160,256> (M =
//     40,960, N = 256, K = 1024, HIP events, back to back; the two-stage form this replaces: 31.9 us): (3,3) = 159,744 B + the
//     1-KB dump 29.2 us, (4,2) = 147,456 B 30.2 us -- the same A stage in flight across the wait, and B one step ahead, not two.
//     (Waves 0-3 loading A and waves 4-7 loading B, each with a vmcnt of its own, so that (4,2) does keep three A stages in
//     flight: 33.7 us, and 31.4 us at (3,3).  The loop is no longer bound by the latency of A alone.)
//   * at most 4 + 3 slots + the dump = 8 LDS objects, as far as this was tried: the compiler keeps its own LDS-DMA scoreboard per
//     object, and where it loses track of one its waits in front of the fragment reads become vmcnt(0) (read the ISA after
//     changing the depths: the loop of <160,256> must show s_waitcnt vmcnt(7) and nothing lower).
//   * per wave LA PA + LB PB DMA instructions are outstanding at most (14 at <160,256> and <128,256>): far from vmcnt's 63.
constexpr int kPjLds = 160 * 1024;
template <int BM, int BN>
struct PjRing {
  static constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128;
  static constexpr int DUMP = (BM / 8) % 8 ? 1024 : 0;  // where the padding pieces of an uneven A stage land (below)
  static constexpr bool fits(int nsa, int nsb) { return nsa * A_BYTES + nsb * B_BYTES + DUMP <= kPjLds; }
  static constexpr int NSA = fits(4, 3) ? 4 : fits(3, 2) ? 3 : 2;
  static constexpr int NSB = fits(4, 3) || fits(3, 3) ? 3 : 2;
  static_assert(fits(NSA, NSB) && NSB <= NSA && NSA <= NSB + 1, "ring depths");
};

// NP 1-KB pieces (8 rows x 128 B) of one operand stage, piece wave + 8 i by this wave.  Every wave issues the SAME number of
// instructions per stage, so one counted wait is right for all of them: where NP % 8 != 0 (BM = 160: 20 pieces, BM = 96: 12) the
// waves without a last piece send an out-of-range one (zeros, no memory traffic) into `dump`, which nobody reads.
// (A __device__ function, not a lambda of the kernel: with the address-space cast inside a lambda the HOST pass silently dropped
// the kernel's instantiation.)
template <int NP>
__device__ __forceinline__ void pj_issue(char* st, char* dump, __amdgpu_buffer_rsrc_t rs, const unsigned (&voff)[(NP + 7) / 8],
                                         unsigned kbytes, int wave) {
#pragma unroll
  for (int i = 0; i < (NP + 7) / 8; ++i) {
    const bool real = 8 * i + 8 <= NP || wave + 8 * i < NP;  // (uniform; voff[i] = kPjOob where not)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_p)(real ? st + (wave + 8 * i) * 1024 : dump), 16,
                                             voff[i] + (real ? kbytes : 0u), 0, 0, 0);
  }
}

template <int BM, int BN>
__global__ __launch_bounds__(kPjThreads) void proj_kernel(ProjArgs p) {
  constexpr int TM = BM / 32, TN = BN / 64;       // 16x16 tiles per wave: (BM/2 rows) x (BN/4 columns)
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128;
  constexpr int NA = BM / 8, NB = BN / 8;         // 1-KB DMA pieces (8 rows x 128 B) per stage
  constexpr int PA = (NA + 7) / 8, PB = NB / 8;   // DMA instructions per wave and stage (A: padded to equal counts, pj_issue)
  constexpr int NSA = PjRing<BM, BN>::NSA, NSB = PjRing<BM, BN>::NSB, LA = NSA - 1, LB = NSB - 1;  // slots; stages of look-ahead
  constexpr int PERIOD = NSA == NSB ? NSA : NSA * NSB / (NSA % 2 == 0 && NSB % 2 == 0 ? 2 : 1);    // lcm: the slot pattern repeats
  static_assert(BM % 32 == 0 && BN % 64 == 0, "tile shape");
  // one LDS object per slot and the k-loop written out over them: the compiler's own waits in front of the fragment reads stay
  // counted per object (a run-time slot index makes every one of them vmcnt(0))
  __shared__ __attribute__((aligned(1024))) char sa0[A_BYTES];
  __shared__ __attribute__((aligned(1024))) char sa1[A_BYTES];
  __shared__ __attribute__((aligned(1024))) char sa2[NSA > 2 ? A_BYTES : 1024];
  __shared__ __attribute__((aligned(1024))) char sa3[NSA > 3 ? A_BYTES : 1024];
  __shared__ __attribute__((aligned(1024))) char sb0[B_BYTES];
  __shared__ __attribute__((aligned(1024))) char sb1[B_BYTES];
  __shared__ __attribute__((aligned(1024))) char sb2[NSB > 2 ? B_BYTES : 1024];
  __shared__ __attribute__((aligned(1024))) char dump[1024];
  auto slot_a = [&](int i) -> char* { return i == 0 ? sa0 : i == 1 ? sa1 : i == 2 ? sa2 : sa3; };  // (i: a constant after unrolling)
  auto slot_b = [&](int i) -> char* { return i == 0 ? sb0 : i == 1 ? sb1 : sb2; };

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int swave = __builtin_amdgcn_readfirstlane(wave);  // (scalar: the DMA's LDS base goes through M0)
  const int wm = wave >> 2, wn = wave & 3;
  const int r = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

  // rows past M / N read as zeros (buffer range check); K % 64 == 0 (host-checked), so no chunk straddles a row end
  const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc(const_cast<u16*>(p.A + (int64_t)m0 * p.lda), 0,
                                                                     (int)(((int64_t)(p.M - m0) * p.lda) * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<u16*>(p.B + (int64_t)n0 * p.ldb), 0,
                                                                     (int)(((int64_t)(p.N - n0) * p.ldb) * 2), 0x00020000);
  unsigned va[PA], vb[PB];
#pragma unroll
  for (int i = 0; i < PA; ++i) {
    const int piece = wave + 8 * i, row = piece * 8 + (lane >> 3);
    va[i] = piece < NA ? (unsigned)row * (unsigned)(p.lda * 2) + (unsigned)(((lane & 7) ^ (row & 7)) << 4) : kPjOob;
  }
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    const int piece = wave + 8 * i, row = piece * 8 + (lane >> 3);
    vb[i] = (unsigned)row * (unsigned)(p.ldb * 2) + (unsigned)(((lane & 7) ^ (row & 7)) << 4);
  }
  const int nk = p.K / 64;
  // stage ks of an operand into a slot; a stage past the end is requested out of range: zeros (no memory traffic) into a slot
  // that nobody reads any more, so that every step issues the same PA + PB instructions and the waits below stay counted
  auto issue_a = [&](char* st, int ks) { pj_issue<NA>(st, dump, rsa, va, ks < nk ? (unsigned)ks * 128u : kPjOob, swave); };
  auto issue_b = [&](char* st, int ks) { pj_issue<NB>(st, dump, rsb, vb, ks < nk ? (unsigned)ks * 128u : kPjOob, swave); };
  // fragment reads: row (tile * 16 + r), chunk (4 j + q) ^ (r & 7): two bases (j), the tile is an immediate
  int offj[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) offj[j] = r * 128 + (((j * 4 + q) ^ (r & 7)) << 4);

  f32x4 acc[TM][TN];
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Issue order and waits.  Step s computes stage s and, behind its fragment reads, requests A stage s + LA and B stage s + LB
  // into the slots that step s - 1 read (every wave is past them: it has passed this step's barrier).  The prologue is the
  // steps -LA .. -1 of the same pattern without their compute, so the counts hold from step 0 on.  vmcnt retires in order:
  //   * NSA == NSB (L = LA = LB): A then B per step.  After stage s's last instruction come the L - 1 steps s - L + 1 .. s - 1:
  //     WAIT = (L - 1) (PA + PB) keeps all of them in flight ((3,3) at <160,256>: 3 + 4 = 7; (2,2): 0, the two-stage form).
  //   * NSA == NSB + 1: B then A per step, so that B stage s (step s - LB) is not behind an A stage that step s does not need.
  //     After it come that step's A (PA) and the LB - 1 steps up to s - 1: WAIT = PA + (LB - 1) (PA + PB); A stage s is older.
  constexpr bool A_FIRST = NSA == NSB;
  constexpr int WAIT = A_FIRST ? (LA - 1) * (PA + PB) : PA + (LB - 1) * (PA + PB);
  auto compute = [&](const char* ca, const char* cb, char* na, char* nb, int ks) {
    const char* As = ca + wm * (BM / 2) * 128;
    const char* Bs = cb + wn * (BN / 4) * 128;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bf16x8 a[TM], b[TN];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) b[tn] = __builtin_bit_cast(bf16x8, *(const uint4*)(Bs + offj[j] + tn * 2048));
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) a[tm] = __builtin_bit_cast(bf16x8, *(const uint4*)(As + offj[j] + tm * 2048));
      if ((j == 0) == A_FIRST)
        issue_a(na, ks + LA);
      else
        issue_b(nb, ks + LB);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[tn], a[tm], acc[tm][tn], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  };
#pragma unroll
  for (int v = -LA; v < 0; ++v) {
    if (!A_FIRST && v + LB >= 0) issue_b(slot_b(v + LB), v + LB);
    issue_a(slot_a(v + LA), v + LA);
    if (A_FIRST) issue_b(slot_b(v + LB), v + LB);
  }
  auto step = [&](int i, int ks) {  // (i = ks % PERIOD: a constant after unrolling)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT) : "memory");  // this wave's pieces of stage ks; younger ones stay in flight
    // ... and every other wave's; and every wave is done reading stage ks - 1, whose slots this step refills
    __builtin_amdgcn_s_barrier();
    compute(slot_a(i % NSA), slot_b(i % NSB), slot_a((i + LA) % NSA), slot_b((i + LB) % NSB), ks);
  };
  // whole periods, then the up to PERIOD - 1 steps that remain.  (One loop whose steps each test ks < nk gives the compiler
  // paths from a skipped step back to the loop's head, and its waits in front of the first step's fragment reads drain.)
  int ks = 0;
  for (; ks + PERIOD <= nk; ks += PERIOD)
#pragma unroll
    for (int i = 0; i < PERIOD; ++i) step(i, ks + i);
#pragma unroll
  for (int i = 0; i < PERIOD - 1; ++i) {
    if (ks + i >= nk) break;
    step(i, ks + i);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the look-ahead DMAs past the end (zeros) must land before the LDS is released

  // (two copies of the store loop under one uniform branch: as an if / else around the store itself the compiler merges the two
  // stores into one and drops the hint)
  auto store = [&](auto nt) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
      const int n = n0 + wn * (BN / 4) + tn * 16 + 4 * q;
      if (n >= p.N) continue;  // (N % 4 == 0, host-checked)
      f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p.bias) bv = (p.bias2 && n >= p.bias_split) ? *(const f32x4*)(p.bias2 + (n - p.bias_split)) : *(const f32x4*)(p.bias + n);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const int m = m0 + wm * (BM / 2) + tm * 16 + r;
        if (m >= p.M) continue;
        f32x4* dst = (f32x4*)(p.C + (int64_t)m * p.ldc + n);
        if constexpr (decltype(nt)::value)
          __builtin_nontemporal_store(acc[tm][tn] + bv, dst);
        else
          *dst = acc[tm][tn] + bv;
      }
    }
  };
  if (p.nt)
    store(std::true_type{});
  else
    store(std::false_type{});
}

// (explicit instantiations: left implicit, the host stubs of kernels with static LDS objects were not emitted)
template __global__ void proj_kernel<64, 256>(ProjArgs);
template __global__ void proj_kernel<96, 256>(ProjArgs);
template __global__ void proj_kernel<128, 256>(ProjArgs);
template __global__ void proj_kernel<160, 256>(ProjArgs);
template __global__ void proj_kernel<192, 256>(ProjArgs);
template __global__ void proj_kernel<224, 256>(ProjArgs);
template __global__ void proj_kernel<256, 256>(ProjArgs);
template __global__ void proj_kernel<64, 128>(ProjArgs);
template __global__ void proj_kernel<96, 128>(ProjArgs);
template __global__ void proj_kernel<128, 128>(ProjArgs);
template __global__ void proj_kernel<160, 128>(ProjArgs);
template __global__ void proj_kernel<192, 128>(ProjArgs);
template __global__ void proj_kernel<224, 128>(ProjArgs);
template __global__ void proj_kernel<256, 128>(ProjArgs);

template <int BM, int BN>
static int launch_one(const ProjArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)fh_cdiv(a.M, BM), (unsigned)fh_cdiv(a.N, BN));
  hipLaunchKernelGGL((proj_kernel<BM, BN>), grid, dim3(kPjThreads), 0, st, a);
  return fh_launch_status();
}

template <int BN>
static int launch_bn(const ProjArgs& a, int bm, hipStream_t st) {
  switch (bm) {
    case 64: return launch_one<64, BN>(a, st);
    case 96: return launch_one<96, BN>(a, st);
    case 128: return launch_one<128, BN>(a, st);
    case 160: return launch_one<160, BN>(a, st);
    case 192: return launch_one<192, BN>(a, st);
    case 224: return launch_one<224, BN>(a, st);
    default: return launch_one<256, BN>(a, st);
  }
}

// The launch plan: all N columns per tile where they fit (BN = 256 or 128), and the row tile that fills the chip's 256 CUs in
// the fewest rounds with the least padding: one round if it can.  fhvae_plan_proj hands it to a caller, launch_proj launches it.
static fhvae_proj_plan plan_proj(int64_t M, int64_t N) {
  fhvae_proj_plan pl = {256, N > 128 ? 256 : 128, 0};
  const int64_t ncol = fh_cdiv(N, pl.BN);
  double best_t = 1e30;
  for (int bm = 64; bm <= 256; bm += 32) {
    const int64_t tiles = fh_cdiv(M, bm) * ncol;
    const double t = (double)fh_cdiv(tiles, 256) * (bm + 24);  // per-tile time ~ rows + a fixed cost (weights, fill, drain)
    if (t < best_t) best_t = t, pl.BM = bm, pl.tiles = (int)tiles;
  }
  return pl;
}

bool proj_eligible(const void* a, int64_t lda, const void* b, int64_t ldb, const float* c, int64_t ldc, int64_t M, int64_t N,
                   int64_t K) {
  if (!a || !b || !c || M <= 0 || N <= 0 || K <= 0) return false;
  if ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) return false;
  if ((K % 64) || (N % 4) || (lda % 8) || (ldb % 8) || (ldc % 4) || lda < K || ldb < K || ldc < N) return false;
  if (M * lda * 2 >= (1LL << 31) || N * ldb * 2 >= (1LL << 30)) return false;  // 32-bit buffer offsets / num_records
  return true;
}

int launch_proj(const void* a, int64_t lda, const void* b, int64_t ldb, float* c, int64_t ldc, const float* bias, int64_t M,
                int64_t N, int64_t K, hipStream_t st, const float* bias2, int bias_split) {
  if (!proj_eligible(a, lda, b, ldb, c, ldc, M, N, K) || (bias2 && (bias_split % 4))) return FHVAE_ERR_ALIGN;
  const fhvae_proj_plan pl = plan_proj(M, N);
  ProjArgs p = {(const u16*)a, (const u16*)b, c, bias, bias2, bias_split, lda, ldb, ldc, (int)M, (int)N, (int)K, pl.tiles <= 256};
  return pl.BN == 256 ? launch_bn<256>(p, pl.BM, st) : launch_bn<128>(p, pl.BM, st);
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_plan_proj(int64_t M, int64_t N, fhvae_proj_plan* out) {
  FH_CHECK_PTR(out);
  FH_CHECK_POS(M);
  FH_CHECK_POS(N);
  *out = plan_proj(M, N);
  return 1;
}

extern "C" int fhvae_proj_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, const float* bias, float* c, int64_t ldc,
                               int64_t M, int64_t N, int64_t K, void* stream) {
  FH_CHECK_PTR(a);
  FH_CHECK_PTR(b);
  FH_CHECK_PTR(c);
  FH_CHECK_POS(M);
  FH_CHECK_POS(N);
  FH_CHECK_POS(K);
  FH_CHECK_I32(M);
  return launch_proj(a, lda, b, ldb, c, ldc, bias, M, N, K, (hipStream_t)stream, nullptr, 0);
}
