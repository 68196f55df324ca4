// segment.hip -- duration-penalised segmentation over a codebook (include/fhvae_segment.h):
//   fhvae_seg_scores : for every (last row n, length l) the best unit of the segment and its score;
//   fhvae_seg_dp     : per utterance the cut that minimises the scores plus lambda per segment, and its back-trace.
//
// PHASE 1 is kmeans.hip's assignment on other rows: a cell's "row" is the f32 segment sum Sf(n, l), its score for unit k is
// fmaf(-2, Sf . c_k, l cn[k]).  The sums are built FHVAE_SEG_CHUNK_ROWS rows (chunk_rows Lmax cells) at a time into the workspace
// by seg_sum_kernel -- one thread per (row, 16-byte column chunk) that runs over l with a float64 accumulator and reads each x
// row from cache -- and seg_min_kernel is allpairs_f32.h's pass over them with the arg-min epilogue: 256 cells stationary per
// workgroup, ALL K centroids streamed through LDS in tiles of 64, a running (best, k) per cell, the four lanes of a cell merged
// by two xor shuffles (smaller score, then smaller k).  The length of a lane's four cells scales cn in the epilogue.  A cell
// whose segment would begin before its utterance (l > room[n], seg_room_kernel) has zeros as its sum and gets +inf / -1.
//
// PHASE 2 is one wavefront per utterance and a lane per length.  The last 64 alphas are a ring along the lanes (alpha[t] goes to
// lane t & 63 and stays there), so at step t lane p stands for the length ((t - 1 - p) & 63) + 1 and loads that entry of the
// row's 256 bytes, eight rows ahead: nothing moves between the lanes but the minimum.  That is four DPP levels inside the rows of
// 16 lanes and four v_readlane across them (a minimum of values that are not NaN: commutative, every lane ends with the same
// bits); the smallest l among the lanes that hold the minimum is read off their ballot.  (A first form with an xor butterfly of
// __shfl_xor on (value, l) and a __shfl_up of the alphas took 0.9 us a step)  back goes to the workspace as
// one byte per frame, 64 at a time.  The back-trace brings 2048 of those bytes into LDS, one lane walks them and marks every
// frame with its segment's end, then the wave fills seg_unit and seg_start of those frames side by side.
//
// Arithmetic: exactly the header's.  No contraction (the pragma below and -ffp-contract=off); the fmaf of the norms and of the
// score are explicit.  No atomics except the atomicOr of the status word.
#pragma clang fp contract(off)

#include <math.h>

#include "allpairs_f32.h"
#include "trellis.h"

#include "../../include/fhvae_segment.h"

namespace fh {

namespace {

constexpr int kSegYT = ap::kYT;
constexpr int kSegMaxLen = FHVAE_SEG_MAX_LEN;
constexpr int64_t kSegChunkRows = FHVAE_SEG_CHUNK_ROWS;
constexpr int kSegWin = 2048;  // back-pointer bytes of a trace-back window

static_assert(kSegYT == 64, "side() fills one cn per streamed row of a tile with the first 64 threads");
static_assert(kSegMaxLen == 64, "a lane per length");
static_assert(kSegWin + kSegMaxLen < 65536, "a segment's end within the window is a uint16");

// ---- workspace of fhvae_seg_scores: cn (K) f32 | room (n_frames) int32 | segment sums (chunk rows, Lmax, D) f32.
// fhvae_seg_dp uses the first n_frames bytes as back-pointers.
struct SegWs {
  int64_t cn, room, sums, total, chunk_rows;
};
inline int64_t seg_pad(int64_t b) { return fh_cdiv(b, 256) * 256; }
inline SegWs seg_ws(int64_t n_frames, int64_t K, int64_t D, int64_t Lmax) {
  SegWs w;
  w.chunk_rows = n_frames < kSegChunkRows ? n_frames : kSegChunkRows;
  w.cn = 0;
  w.room = w.cn + seg_pad(K * 4);
  w.sums = w.room + seg_pad(n_frames * 4);
  w.total = w.sums + seg_pad(w.chunk_rows * Lmax * D * 4);
  return w;
}

// out[k] = sum_d c[k][d]^2: km_sqnorm_kernel of kmeans.hip (one thread per row, one fma chain in d order)
__global__ void seg_sqnorm_kernel(const float* __restrict__ m, int64_t ld, int64_t rows, int D, float* __restrict__ out,
                                  const int32_t* status) {
  if (*status & FHVAE_SEG_BAD_PTR) return;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const float* p = m + r * ld;
  float ss = 0.f;
  for (int d = 0; d < D; d += 4) {
    const float4 v = *(const float4*)(p + d);
    ss = __builtin_fmaf(v.x, v.x, ss);
    ss = __builtin_fmaf(v.y, v.y, ss);
    ss = __builtin_fmaf(v.z, v.z, ss);
    ss = __builtin_fmaf(v.w, v.w, ss);
  }
  out[r] = ss;
}

// room[n] = the lengths row n can end: min(n - first row of its utterance + 1, Lmax); one thread per row finds its utterance by
// a binary search in utt_ptr (integer comparisons only) and checks what it found
__global__ void seg_room_kernel(const int64_t* __restrict__ utt_ptr, int64_t U, int64_t n_frames, int Lmax, int32_t* __restrict__ room,
                                const int32_t* status) {
  if (*status & FHVAE_SEG_BAD_PTR) return;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_frames) return;
  int64_t lo = 0, hi = U - 1;  // the last u with utt_ptr[u] <= n
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (utt_ptr[mid] <= n) lo = mid; else hi = mid - 1;
  }
  const int64_t a = utt_ptr[lo], b = utt_ptr[lo + 1];
  int64_t rm = 0;
  if (a >= 0 && a <= n && n < b) rm = n - a + 1 < Lmax ? n - a + 1 : Lmax;
  room[n] = (int32_t)rm;
}

// one thread per (row of the chunk, 16-byte column chunk): the float64 sums over l = 1 .. room, each rounded once to f32;
// zeros for the lengths past room
__global__ void __launch_bounds__(256) seg_sum_kernel(const float* __restrict__ x, int64_t ldx, int64_t n_frames, int D, int Lmax,
                                                      const int32_t* __restrict__ room, int64_t row0, int rows, float* __restrict__ sums,
                                                      const int32_t* status) {
  if (*status & FHVAE_SEG_BAD_PTR) return;
  const int CH = D >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t r = idx / CH;
  const int ch = (int)(idx - r * CH);
  const int64_t n = row0 + r;
  if (r >= rows || n >= n_frames) return;
  int64_t rm = room[n];
  if (rm > Lmax) rm = Lmax;
  if (rm > n + 1) rm = n + 1;  // (never below row 0, whatever room holds)
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  float* out = sums + r * Lmax * D + ch * 4;
  const float* in = x + n * ldx + ch * 4;
  for (int l = 1; l <= Lmax; ++l) {
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (l <= rm) {
      const float4 v = *(const float4*)(in - (int64_t)(l - 1) * ldx);
      a0 = a0 + (double)v.x, a1 = a1 + (double)v.y, a2 = a2 + (double)v.z, a3 = a3 + (double)v.w;
      w = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
    }
    *(float4*)(out + (int64_t)(l - 1) * D) = w;
  }
}

struct SegMinArgs {
  const float* sums;  // (cells, D), dense
  const float* cent;
  const float* cn;       // (K)
  const int32_t* room;   // (n_frames)
  float* score;          // (n_frames, Lmax)
  int32_t* unit;
  const int32_t* status;
  int64_t ldc, row0, n_frames;
  int cells, K, Lmax;
};

// (D > 96: 128 and more registers of stationary fragments; two workgroups per CU would spill, as in kmeans.hip)
template <int D>
__global__ __launch_bounds__(256, D > 96 ? 1 : 2) void seg_min_kernel(SegMinArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                            // [64][D] f32, swizzled
  float* cnl = (float*)(smem + kSegYT * D * 4);  // [64]
  if (*a.status & FHVAE_SEG_BAD_PTR) return;     // (the same in every thread)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int x0 = (int)blockIdx.x * 256 + wave * 64;  // (cells <= 4096 * 64)
  const int K = a.K;

  uint4 xf[4][D / 16];
  ap::load_stationary<D>(a.sums, D, a.cells, x0, xf);
  float best[4], lf[4];
  int bk[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) best[t] = INFINITY, bk[t] = 0, lf[t] = (float)((x0 + t * 16 + i) % a.Lmax + 1);

  ap::stream<D>(
      a.cent, a.ldc, 0, K, ytile, xf,
      [&](int y0) {
        if (tid < kSegYT) cnl[tid] = y0 + tid < K ? a.cn[y0 + tid] : INFINITY;
      },
      ap::EveryBlock(),
      [&](int y0, int yb, const f32x4(&acc)[4]) {
        const float4 cv = *(const float4*)(cnl + yb * 16 + 4 * g);
        const float cr[4] = {cv.x, cv.y, cv.z, cv.w};
        const int kb = y0 + yb * 16 + 4 * g;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float s = __builtin_fmaf(-2.f, acc[t][r], lf[t] * cr[r]);
            if (s < best[t]) best[t] = s, bk[t] = kb + r;
          }
        }
      });

  // ---- the four lanes of a cell: smaller score, then smaller k
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float ob = __shfl_xor(best[t], o, 64);
      const int ok = __shfl_xor(bk[t], o, 64);
      if (ob < best[t] || (ob == best[t] && ok < bk[t])) best[t] = ob, bk[t] = ok;
    }
    const int c = x0 + t * 16 + i;
    const int64_t n = a.row0 + c / a.Lmax;
    if (g == 0 && c < a.cells && n < a.n_frames) {
      const bool inside = c % a.Lmax < a.room[n];
      const int64_t o = a.row0 * a.Lmax + c;
      a.score[o] = inside ? best[t] : INFINITY;
      a.unit[o] = inside ? bk[t] : -1;
    }
  }
}

template <int D>
int seg_min_launch(const SegMinArgs& a, hipStream_t st) {
  const int smem = kSegYT * D * 4 + kSegYT * 4;
  hipLaunchKernelGGL(seg_min_kernel<D>, dim3((unsigned)fh_cdiv(a.cells, 256)), dim3(256), (size_t)smem, st, a);
  return fh_launch_status();
}

// the l a back-pointer byte stands for at segment end t (1 <= t): inside [1, min(Lmax, t)] whatever the byte holds
__device__ __forceinline__ int seg_len(int b, int t, int Lmax) {
  int l = b < 1 ? 1 : b;
  l = l > Lmax ? Lmax : l;
  return l > t ? t : l;
}

// the smaller of two values that are not NaN
__device__ __forceinline__ double seg_min2(double a, double b) { return b < a ? b : a; }

// min(v, v of the lane the DPP control names): the two halves of the double move separately
template <int CTRL>
__device__ __forceinline__ double seg_min_dpp(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return seg_min2(v, __hiloint2double(ohi, olo));
}

__device__ __forceinline__ double seg_readlane(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

__global__ void __launch_bounds__(64)
    seg_dp_kernel(const float* __restrict__ score, const int32_t* __restrict__ unit, int64_t n_frames, int Lmax,
                  const int64_t* __restrict__ utt_ptr, int64_t U, double lambda, uint8_t* back, int32_t* __restrict__ seg_unit,
                  uint8_t* __restrict__ seg_start, int32_t* __restrict__ n_seg, double* __restrict__ cost, int32_t* status) {
  __shared__ uint8_t bw[kSegWin];                  // back[lo + 1 .. hi] of the window: bw[i] is the byte of segment end lo + i + 1
  __shared__ uint16_t ew[kSegWin + kSegMaxLen];    // frame f: its segment's end minus lo, at ew[f - lo + 64]
  __shared__ int walk[2];                          // where the walk stopped, the segments it met
  if (*status & FHVAE_SEG_BAD_PTR) return;  // (set by the check kernel)
  const int lane = threadIdx.x;
  const int64_t u = blockIdx.x;
  if (u >= U || Lmax < 1 || Lmax > kSegMaxLen) return;
  const int64_t u0 = utt_ptr[u], u1 = utt_ptr[u + 1];
  if (!tr_utt_ok(u0, u1, n_frames)) return;
  const int T = (int)(u1 - u0);
  if (T == 0) {
    if (lane == 0) n_seg[u] = 0, cost[u] = 0.0;
    return;
  }
  // ---- forward.  The last 64 alphas stay where they are: lane p holds alpha[t'] of the latest t' < t with t' = p (mod 64), so
  // at step t it stands for the length l = t - t' = ((t - 1 - p) & 63) + 1 and loads score[row t - 1][l - 1]: the row's 256 bytes,
  // rotated.  cur / nxt: this lane's scores of eight rows, loaded eight rows ahead
  const float* sc = score + u0 * Lmax;
  uint8_t* bk = back + u0;  // back[t] at bk[t - 1]
  double h = lane == 0 ? 0.0 : INFINITY, alpha = 0.0;
  int keep = 0;
  float cur[8], nxt[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int col = (i - lane) & 63;
    nxt[i] = (col < Lmax && 1 + i <= T) ? sc[(int64_t)i * Lmax + col] : INFINITY;
  }
  for (int t0 = 1; t0 <= T; t0 += 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      cur[i] = nxt[i];
      const int64_t tn = (int64_t)t0 + 8 + i;
      const int col = (int)((tn - 1 - lane) & 63);
      nxt[i] = (col < Lmax && tn <= T) ? sc[(tn - 1) * Lmax + col] : INFINITY;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t = t0 + i;
      if (t > T) break;  // (the same in all lanes)
      const int top = (t - 1) & 63, col = (top - lane) & 63;  // the lane of alpha[t - 1]; this lane's l - 1
      double v = h + (double)cur[i];
      if (col >= t || !(v < INFINITY)) v = INFINITY;  // no such segment (cur is +inf past Lmax), +inf or NaN: never wins
      // the minimum: four DPP levels inside each row of 16 lanes, then the four rows; the smallest l of the lanes that hold it is
      // the first of them below `top`, cyclically: the leading zeros of their ballot rotated so that `top` is bit 63
      double m = seg_min_dpp<0xB1>(v);  // quad_perm [1, 0, 3, 2]
      m = seg_min_dpp<0x4E>(m);         // quad_perm [2, 3, 0, 1]
      m = seg_min_dpp<0x141>(m);        // row_half_mirror
      m = seg_min_dpp<0x140>(m);        // row_mirror
      m = seg_min2(seg_min2(seg_readlane(m, 0), seg_readlane(m, 16)), seg_min2(seg_readlane(m, 32), seg_readlane(m, 48)));
      const uint64_t hit = __ballot(v == m);
      const uint64_t rot = top == 63 ? hit : ((hit << (63 - top)) | (hit >> (top + 1)));
      const int l = __clzll(rot) + 1;
      alpha = m + lambda;
      if (lane == top) keep = l;
      if ((t & 63) == 0 || t == T) {
        const int base = (t - 1) & ~63;
        if (base + lane < t) bk[base + lane] = (uint8_t)keep;
      }
      if (lane == (t & 63)) h = alpha;
    }
  }
  if (!(alpha > -INFINITY && alpha < INFINITY)) {  // (the same bits in all lanes)
    if (lane == 0) atomicOr(status, FHVAE_SEG_NOT_FINITE);
    return;
  }
  if (lane == 0) cost[u] = alpha;

  // ---- back-trace, a window of back-pointer bytes at a time from the end
  int t = T, count = 0;
  while (t > 0) {
    const int hi = t, lo = hi > kSegWin ? hi - kSegWin : 0;
    __syncthreads();  // the forward's stores are visible to the wave; the window before is consumed
    for (int i = lane; i < hi - lo; i += 64) bw[i] = bk[lo + i];
    __syncthreads();
    if (lane == 0) {
      int tt = hi, c = 0;
      while (tt > lo) {
        const int l = seg_len(bw[tt - 1 - lo], tt, Lmax);
        for (int f = tt - l; f < tt; ++f) ew[f - lo + kSegMaxLen] = (uint16_t)(tt - lo);
        tt -= l;
        ++c;
      }
      walk[0] = tt, walk[1] = c;
    }
    __syncthreads();
    const int tn = walk[0];  // (lo - 64 < tn <= lo)
    count += walk[1];
    for (int f = tn + lane; f < hi; f += 64) {
      const int e = lo + ew[f - lo + kSegMaxLen];  // lo < e <= hi
      const int l = seg_len(bw[e - 1 - lo], e, Lmax);
      seg_unit[u0 + f] = unit[(u0 + e - 1) * Lmax + (l - 1)];
      seg_start[u0 + f] = (uint8_t)(f == e - l);
    }
    t = tn;
  }
  if (lane == 0) n_seg[u] = count;
}

int seg_check_common(int64_t n_frames, int64_t Lmax, const int64_t* utt_ptr, int64_t U, const void* ws, const int32_t* status) {
  FH_CHECK_PTR(utt_ptr);
  FH_CHECK_PTR(ws);
  FH_CHECK_PTR(status);
  FH_CHECK_POS(U);
  if (((uintptr_t)ws & 15) != 0 || ((uintptr_t)utt_ptr & 7) != 0 || ((uintptr_t)status & 3) != 0) return FHVAE_ERR_ALIGN;
  if (n_frames > FHVAE_KM_MAX_ROWS || Lmax < 1 || Lmax > FHVAE_SEG_MAX_LEN) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(U);
  return FHVAE_OK;
}

}  // namespace

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_seg_ws_bytes(int64_t n_frames, int64_t K, int64_t D, int64_t Lmax) {
  if (n_frames < 1 || K < 1 || n_frames > FHVAE_KM_MAX_ROWS || K > FHVAE_KM_MAX_CENT) return 0;
  if (D < 16 || D > 128 || D % 16 != 0 || Lmax < 1 || Lmax > FHVAE_SEG_MAX_LEN) return 0;
  return seg_ws(n_frames, K, D, Lmax).total;
}

extern "C" int fhvae_seg_scores(const float* x, int64_t ldx, int64_t n_frames, int64_t D, const float* cent, int64_t ldc, int64_t K,
                                int64_t Lmax, const int64_t* utt_ptr, int64_t U, void* ws, int64_t ws_bytes, float* score, int32_t* unit,
                                int32_t* status, void* stream) {
  FH_CHECK_PTR(x);
  FH_CHECK_PTR(cent);
  FH_CHECK_PTR(score);
  FH_CHECK_PTR(unit);
  FH_CHECK_POS(n_frames);
  FH_CHECK_POS(K);
  int rc = fh_allpairs_check(x, ldx, D);
  if (rc != FHVAE_OK) return rc;
  rc = fh_allpairs_check(cent, ldc, D);
  if (rc != FHVAE_OK) return rc;
  rc = seg_check_common(n_frames, Lmax, utt_ptr, U, ws, status);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)score & 3) != 0 || ((uintptr_t)unit & 3) != 0) return FHVAE_ERR_ALIGN;
  if (K > FHVAE_KM_MAX_CENT) return FHVAE_ERR_LIMIT;
  const SegWs w = seg_ws(n_frames, K, D, Lmax);
  if (ws_bytes < w.total) return FHVAE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  float* cn = (float*)((char*)ws + w.cn);
  int32_t* room = (int32_t*)((char*)ws + w.room);
  float* sums = (float*)((char*)ws + w.sums);
  hipLaunchKernelGGL(tr_check_kernel<FHVAE_SEG_BAD_PTR>, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, st, utt_ptr, U, n_frames, status);
  hipLaunchKernelGGL(seg_sqnorm_kernel, dim3((unsigned)fh_cdiv(K, 256)), dim3(256), 0, st, cent, ldc, K, (int)D, cn, status);
  hipLaunchKernelGGL(seg_room_kernel, dim3((unsigned)fh_cdiv(n_frames, 256)), dim3(256), 0, st, utt_ptr, U, n_frames, (int)Lmax, room,
                     status);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  SegMinArgs a = {};
  a.sums = sums;
  a.cent = cent;
  a.cn = cn;
  a.room = room;
  a.score = score;
  a.unit = unit;
  a.status = status;
  a.ldc = ldc;
  a.n_frames = n_frames;
  a.K = (int)K;
  a.Lmax = (int)Lmax;
  for (int64_t row0 = 0; row0 < n_frames; row0 += w.chunk_rows) {
    const int64_t rows = n_frames - row0 < w.chunk_rows ? n_frames - row0 : w.chunk_rows;
    hipLaunchKernelGGL(seg_sum_kernel, dim3((unsigned)fh_cdiv(rows * (D / 4), 256)), dim3(256), 0, st, x, ldx, n_frames, (int)D, (int)Lmax,
                       room, row0, (int)rows, sums, status);
    a.row0 = row0;
    a.cells = (int)(rows * Lmax);
    rc = fh_allpairs_dispatch(D, [&](auto d) { return seg_min_launch<decltype(d)::value>(a, st); });
    if (rc != FHVAE_OK) return rc;
  }
  return FHVAE_OK;
}

extern "C" int fhvae_seg_dp(const float* score, const int32_t* unit, int64_t n_frames, int64_t Lmax, const int64_t* utt_ptr, int64_t U,
                            double lambda, void* ws, int64_t ws_bytes, int32_t* seg_unit, uint8_t* seg_start, int32_t* n_seg,
                            double* cost, int32_t* status, void* stream) {
  FH_CHECK_PTR(score);
  FH_CHECK_PTR(unit);
  FH_CHECK_PTR(seg_unit);
  FH_CHECK_PTR(seg_start);
  FH_CHECK_PTR(n_seg);
  FH_CHECK_PTR(cost);
  if (n_frames < 0 || !(lambda >= 0.0)) return FHVAE_ERR_SHAPE;
  int rc = seg_check_common(n_frames, Lmax, utt_ptr, U, ws, status);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)score & 3) != 0 || ((uintptr_t)unit & 3) != 0 || ((uintptr_t)seg_unit & 3) != 0 || ((uintptr_t)n_seg & 3) != 0 ||
      ((uintptr_t)cost & 7) != 0)
    return FHVAE_ERR_ALIGN;
  if (ws_bytes < n_frames) return FHVAE_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tr_check_kernel<FHVAE_SEG_BAD_PTR>, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, st, utt_ptr, U, n_frames, status);
  hipLaunchKernelGGL(seg_dp_kernel, dim3((unsigned)U), dim3(64), 0, st, score, unit, n_frames, (int)Lmax, utt_ptr, U, lambda, (uint8_t*)ws,
                     seg_unit, seg_start, n_seg, cost, status);
  return fh_launch_status();
}
