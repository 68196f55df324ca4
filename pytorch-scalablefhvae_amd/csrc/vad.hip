// vad.hip -- energy voice-activity detection (include/fhvae_vad.h):
//   fhvae_vad_energy : one energy per frame of a batch of waveforms, in the reference's framing (librosa's centred RMS) or
//                      Kaldi's (snip-edges raw log energy);
//   fhvae_vad_decide : per-utterance threshold from the mean energy, the context vote of every frame, and the exclusive
//                      prefix count of the decisions over the whole batch (every voiced row's destination);
//   fhvae_vad_select : the voiced rows of a feature matrix, packed.
//
// Energy.  A workgroup takes a tile of consecutive frames of the batch (at most kVadTileFrames, fewer when frame_len and
// frame_shift make their samples exceed kVadLdsSamples).  A tile may span utterances: it is walked utterance by utterance,
// and for each the samples its frames cover -- (frames - 1) * shift + frame_len padded positions, the overlap of neighbouring
// frames included once -- are staged in LDS: the part inside the utterance by 16-byte loads where wave + offset is aligned,
// with a scalar head and tail; the reflected edge of the centred framing by scalar loads.  Every sample comes from HBM once
// per tile (neighbouring tiles share frame_len - shift samples).  16 lanes then sum a frame from LDS in float64, lane j the
// positions j, j + 16, ... in increasing order, and a fixed butterfly adds the 16 sums: the order is a function of the frame
// alone.
//
// Decision.  The mean of an utterance must not depend on the batch and must not serialise a long utterance on one
// workgroup: utterance u owns the slots frame_ptr[u] / C + u + k, k < ceil(T_u / C), of a partial-sum array (C =
// FHVAE_VAD_CHUNK; distinct utterances get distinct slots because floor(a / C) + ceil(T / C) <= floor((a + T) / C) + 1, and
// there are at most n_frames / C + U of them).  One workgroup per slot sums its chunk (fixed order), one thread per
// utterance adds the utterance's chunks in order and forms the threshold, one thread per frame votes; the vote kernel
// counts the voiced frames per tile of FHVAE_VAD_TILE frames, one workgroup scans the tile counts, and the apply kernel
// writes every frame's rank.  Integer counts apart there is no atomic; the one atomicOr sets the status word.
//
// Pointer errors: a check kernel validates the pointers and sets FHVAE_VAD_BAD_PTR; the kernels behind it then write
// nothing.  They also re-check the utterance of every frame they touch, so no input makes them read or write out of bounds.
#pragma clang fp contract(off)

#include <float.h>

#include "common.h"

#include "../../include/fhvae_vad.h"

namespace fh {

constexpr int kVadThreads = 256;
constexpr int kVadTileFrames = 32;      // frames per workgroup of the energy kernel, at most (21 KB of LDS at 400 / 160: 7 per CU)
constexpr int kVadLdsSamples = 12288;   // samples a tile may stage (48 KB)
constexpr int kVadPerThread = FHVAE_VAD_TILE / kVadThreads;  // frames per thread of the vote and apply kernels

static_assert(FHVAE_VAD_CHUNK % kVadThreads == 0 && FHVAE_VAD_TILE % kVadThreads == 0, "chunk and tile are whole passes");
static_assert(FHVAE_VAD_MAX_FRAME <= kVadLdsSamples, "one frame fits the staging buffer");

__host__ __device__ inline int64_t vad_frames(int64_t n, int64_t L, int64_t hop, int mode) {
  if (mode == FHVAE_VAD_RMS_CENTER) return n < L / 2 + 1 ? 0 : 1 + (n + 2 * (L / 2) - L) / hop;
  return n < L ? 0 : 1 + (n - L) / hop;
}

// the last u in [0, U) with ptr[u] <= x (0 when there is none); reads ptr[0 .. U - 1] only
__device__ __forceinline__ int64_t vad_find(const int64_t* __restrict__ ptr, int64_t U, int64_t x) {
  int64_t lo = 0, hi = U - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ptr[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the 16 lanes of a frame: every lane gets the same sum (a + b == b + a bitwise)
__device__ __forceinline__ double vad_sum16(double v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------- energy
// one thread per utterance: offsets inside the buffers, at least one frame, frame counts by the framing rule
__global__ void vad_energy_check_kernel(const int64_t* __restrict__ wave_ptr, const int64_t* __restrict__ frame_ptr, int64_t U,
                                        int64_t n_samples, int64_t n_frames, int64_t L, int64_t hop, int mode, int32_t* status) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t w0 = wave_ptr[u], w1 = wave_ptr[u + 1], f0 = frame_ptr[u], f1 = frame_ptr[u + 1];
  bool ok = w0 >= 0 && w1 <= n_samples && w1 > w0;
  const int64_t T = ok ? vad_frames(w1 - w0, L, hop, mode) : 0;
  ok = ok && T >= 1 && f0 >= 0 && f1 <= n_frames && f1 > f0 && f1 - f0 == T;
  if (u == 0) ok = ok && f0 == 0;
  if (u == U - 1) ok = ok && f1 == n_frames;
  if (!ok) atomicOr(status, FHVAE_VAD_BAD_PTR);
}

__global__ void __launch_bounds__(kVadThreads) vad_energy_kernel(const float* __restrict__ wave, int64_t n_samples,
                                                                 const int64_t* __restrict__ wave_ptr,
                                                                 const int64_t* __restrict__ frame_ptr, int64_t U, int64_t n_frames,
                                                                 int L, int64_t hop, int tile_frames, int mode, int flags, int vec,
                                                                 float* __restrict__ energy, const int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  if (*status & FHVAE_VAD_BAD_PTR) return;  // (set by the check kernel)
  const int tid = threadIdx.x, j = tid & 15;
  const int64_t g0 = (int64_t)blockIdx.x * tile_frames;
  const int64_t g1 = g0 + tile_frames < n_frames ? g0 + tile_frames : n_frames;
  const int64_t off = mode == FHVAE_VAD_RMS_CENTER ? L / 2 : 0;
  const bool dc = mode == FHVAE_VAD_LOGE_SNIP && (flags & FHVAE_VAD_REMOVE_DC);
  int64_t g = g0, u = vad_find(frame_ptr, U, g0);
  // (every value that steers this loop is the same in all threads: the barriers are reached by all or none)
  while (g < g1 && u < U) {
    const int64_t fa = frame_ptr[u], fe = frame_ptr[u + 1], wa = wave_ptr[u], we = wave_ptr[u + 1];
    if (!(wa >= 0 && we <= n_samples && we > wa && fa >= 0 && fe <= n_frames && fa <= g && g < fe)) break;
    const int64_t n = we - wa;
    if (fe - fa != vad_frames(n, L, hop, mode)) break;
    const int64_t f0 = g - fa;
    const int nf = (int)((g1 < fe ? g1 : fe) - g);          // frames of this utterance in the tile
    const int cnt = (int)((nf - 1) * hop) + L;              // padded positions they cover: <= kVadLdsSamples
    const int64_t i_lo = f0 * hop - off, i_hi = i_lo + cnt;  // xs[k] is sample i_lo + k of the utterance
    const int64_t ia = i_lo > 0 ? i_lo : 0, ib = i_hi < n ? i_hi : n;
    // the part inside the utterance: samples [ia, ib) = wave[wa + ia, wa + ib)
    if (vec) {
      const int64_t ga = wa + ia, gb = wa + ib, qa = ga & ~(int64_t)3, qt = gb & ~(int64_t)3;
      const float* src = wave + qa;              // 16-byte aligned
      float* dst = xs + (qa - wa - i_lo);        // (xs index of sample qa; below 0 by up to 3 when the head is cut)
      const int qf0 = qa < ga ? 1 : 0, qf1 = (int)((gb - qa) >> 2);  // the quads [qf0, qf1) lie whole inside [ga, gb)
      // whole quads, four loads in flight per thread (a load past the end re-reads the last whole quad and is dropped: no
      // branch around a load)
      for (int q0 = qf0 + tid; q0 < qf1; q0 += 4 * kVadThreads) {
        float4 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = q0 + r * kVadThreads;
          v[r] = *(const float4*)(src + 4 * (q < qf1 ? q : qf1 - 1));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q = q0 + r * kVadThreads;
          if (q < qf1) {
            float* d = dst + 4 * q;
            d[0] = v[r].x, d[1] = v[r].y, d[2] = v[r].z, d[3] = v[r].w;
          }
        }
      }
      // the scalar head and tail: the samples of [ga, gb) in the first and in the last quad (again, if those were whole)
      if (tid < 8) {
        const int64_t idx = (tid < 4 ? qa : qt) + (tid & 3);
        if (idx >= ga && idx < gb) xs[idx - wa - i_lo] = wave[idx];
      }
    } else {
      for (int64_t i = ia + tid; i < ib; i += kVadThreads) xs[i - i_lo] = wave[wa + i];
    }
    // what lies in front of and behind the utterance: reflection, the edge not repeated (centred framing only; the clamp
    // never acts on a checked utterance)
    const int left = (int)(ia - i_lo), right = (int)(ib - i_lo);
    for (int k = tid; k < left + (cnt - right); k += kVadThreads) {
      const int kk = k < left ? k : right + (k - left);
      const int64_t i = i_lo + kk;
      int64_t r = i < 0 ? -i : 2 * (n - 1) - i;
      r = r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
      xs[kk] = wave[wa + r];
    }
    __syncthreads();
    for (int fl = tid >> 4; fl < nf; fl += kVadThreads / 16) {
      const float* p = xs + (int64_t)fl * hop;
      double mean = 0.0;
      if (dc) {
        double m = 0.0;
        for (int k = j; k < L; k += 16) m = m + (double)p[k];
        mean = vad_sum16(m) / (double)L;
      }
      double s = 0.0;
      for (int k = j; k < L; k += 16) {
        const double d = (double)p[k] - mean;
        s = s + d * d;
      }
      s = vad_sum16(s);
      const double e = mode == FHVAE_VAD_RMS_CENTER ? sqrt(s / (double)L) : log(s > (double)FLT_EPSILON ? s : (double)FLT_EPSILON);
      if (j == 0) energy[g + fl] = (float)e;
    }
    __syncthreads();
    g += nf;
    ++u;
  }
}

// ---------------------------------------------------------------------------------------------------------------- decide
struct VadWs {  // the workspace of fhvae_vad_decide
  int64_t slots, tiles;
  double* partial;    // (slots) the chunk sums
  double* th;         // (U) the thresholds
  int64_t* tile_off;  // (tiles + 1) the voiced frames per tile, then their exclusive scan and the total
};

__host__ __device__ inline int64_t vad_slots(int64_t n_frames, int64_t U) { return n_frames / FHVAE_VAD_CHUNK + U; }

static inline VadWs vad_ws(void* ws, int64_t n_frames, int64_t U) {
  VadWs w;
  w.slots = vad_slots(n_frames, U);
  w.tiles = fh_cdiv(n_frames, FHVAE_VAD_TILE);
  w.partial = (double*)ws;
  w.th = w.partial + w.slots;
  w.tile_off = (int64_t*)(w.th + U);
  return w;
}

// one thread per utterance: frame_ptr starts at 0, ends at n_frames and rises strictly
__global__ void vad_decide_check_kernel(const int64_t* __restrict__ frame_ptr, int64_t U, int64_t n_frames, int32_t* status) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t f0 = frame_ptr[u], f1 = frame_ptr[u + 1];
  bool ok = f0 >= 0 && f1 <= n_frames && f1 > f0;
  if (u == 0) ok = ok && f0 == 0;
  if (u == U - 1) ok = ok && f1 == n_frames;
  if (!ok) atomicOr(status, FHVAE_VAD_BAD_PTR);
}

// one workgroup per slot: the sum of one chunk of one utterance
__global__ void __launch_bounds__(kVadThreads) vad_partial_kernel(const float* __restrict__ energy,
                                                                  const int64_t* __restrict__ frame_ptr, int64_t U, int64_t n_frames,
                                                                  double* __restrict__ partial, const int32_t* status) {
  __shared__ double sh[kVadThreads];
  if (*status & FHVAE_VAD_BAD_PTR) return;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  // the last u with frame_ptr[u] / C + u <= b (that key rises strictly with u)
  int64_t lo = 0, hi = U - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (frame_ptr[mid] / FHVAE_VAD_CHUNK + mid <= b) lo = mid; else hi = mid - 1;
  }
  const int64_t a = frame_ptr[lo], e = frame_ptr[lo + 1];
  if (!(a >= 0 && e <= n_frames && e > a)) return;
  const int64_t k = b - (a / FHVAE_VAD_CHUNK + lo);
  if (k < 0 || k * FHVAE_VAD_CHUNK >= e - a) return;  // (a slot no utterance owns)
  const int64_t c0 = a + k * FHVAE_VAD_CHUNK;
  const int len = (int)(e - c0 < FHVAE_VAD_CHUNK ? e - c0 : FHVAE_VAD_CHUNK);
  double s = 0.0;
  for (int i = tid; i < len; i += kVadThreads) s = s + (double)energy[c0 + i];
  sh[tid] = s;
  __syncthreads();
  for (int o = kVadThreads / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] = sh[tid] + sh[tid + o];
    __syncthreads();
  }
  if (tid == 0) partial[b] = sh[0];
}

// one thread per utterance: its chunks in order, then the threshold
__global__ void vad_threshold_kernel(const int64_t* __restrict__ frame_ptr, int64_t U, int64_t n_frames, int64_t slots,
                                     const double* __restrict__ partial, double thr_abs, double mean_scale, double* __restrict__ th,
                                     const int32_t* status) {
  if (*status & FHVAE_VAD_BAD_PTR) return;
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int64_t a = frame_ptr[u], e = frame_ptr[u + 1];
  if (!(a >= 0 && e <= n_frames && e > a)) return;
  const int64_t T = e - a, s0 = a / FHVAE_VAD_CHUNK + u, chunks = (T + FHVAE_VAD_CHUNK - 1) / FHVAE_VAD_CHUNK;
  double s = 0.0;
  for (int64_t k = 0; k < chunks && s0 + k < slots; ++k) s = s + partial[s0 + k];
  th[u] = thr_abs + mean_scale * (s / (double)T);
}

// exclusive scan of one value per thread over the workgroup; *total: the sum.  sh: kVadThreads values
__device__ __forceinline__ int64_t vad_block_scan(int64_t v, int64_t* sh, int tid, int64_t* total) {
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < kVadThreads; o <<= 1) {
    const int64_t add = tid >= o ? sh[tid - o] : 0;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  const int64_t incl = sh[tid];
  *total = sh[kVadThreads - 1];
  __syncthreads();
  return incl - v;
}

// one thread per kVadPerThread consecutive frames: the vote of each, and the voiced frames of the tile
__global__ void __launch_bounds__(kVadThreads) vad_vote_kernel(const float* __restrict__ energy, const int64_t* __restrict__ frame_ptr,
                                                               int64_t U, int64_t n_frames, const double* __restrict__ th, int64_t ctx,
                                                               float proportion, uint8_t* __restrict__ vad,
                                                               int64_t* __restrict__ tile_cnt, const int32_t* status) {
  __shared__ int64_t sh[kVadThreads];
  if (*status & FHVAE_VAD_BAD_PTR) return;
  const int tid = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * FHVAE_VAD_TILE + (int64_t)tid * kVadPerThread;
  int64_t u = first < n_frames ? vad_find(frame_ptr, U, first) : 0;
  int64_t count = 0;
  for (int e = 0; e < kVadPerThread; ++e) {
    const int64_t g = first + e;
    if (g >= n_frames) break;
    while (u + 1 < U && frame_ptr[u + 1] <= g) ++u;
    const int64_t a = frame_ptr[u], b = frame_ptr[u + 1];
    uint8_t v = 0;
    if (a >= 0 && a <= g && g < b && b <= n_frames) {
      const int64_t t = g - a, T = b - a;
      const int64_t lo = t - ctx > 0 ? t - ctx : 0, hi = t + ctx < T - 1 ? t + ctx : T - 1;
      const double thu = th[u];
      int64_t num = 0;
      for (int64_t t2 = lo; t2 <= hi; ++t2) num += (double)energy[a + t2] > thu ? 1 : 0;
      const float need = (float)(hi - lo + 1) * proportion;
      v = (float)num >= need ? 1 : 0;
    }
    vad[g] = v;
    count += v;
  }
  int64_t total;
  vad_block_scan(count, sh, tid, &total);
  if (tid == 0) tile_cnt[blockIdx.x] = total;
}

// one workgroup: tile_off (tiles) counts -> their exclusive scan, tile_off[tiles] = the total
__global__ void __launch_bounds__(kVadThreads) vad_scan_kernel(int64_t* __restrict__ tile_off, int64_t tiles, const int32_t* status) {
  __shared__ int64_t sh[kVadThreads];
  if (*status & FHVAE_VAD_BAD_PTR) return;
  const int tid = threadIdx.x;
  int64_t carry = 0;
  for (int64_t base = 0; base < tiles; base += kVadThreads) {
    const int64_t i = base + tid;
    const int64_t v = i < tiles ? tile_off[i] : 0;
    int64_t total;
    const int64_t ex = vad_block_scan(v, sh, tid, &total);
    if (i < tiles) tile_off[i] = carry + ex;
    carry += total;
  }
  if (tid == 0) tile_off[tiles] = carry;
}

// one thread per kVadPerThread consecutive frames: rank = the tile's offset + the voiced frames of the tile in front
__global__ void __launch_bounds__(kVadThreads) vad_rank_kernel(const uint8_t* __restrict__ vad, int64_t n_frames,
                                                               const int64_t* __restrict__ tile_off, int64_t tiles,
                                                               int64_t* __restrict__ rank, const int32_t* status) {
  __shared__ int64_t sh[kVadThreads];
  if (*status & FHVAE_VAD_BAD_PTR) return;
  const int tid = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * FHVAE_VAD_TILE + (int64_t)tid * kVadPerThread;
  uint8_t v[kVadPerThread];
  int64_t count = 0;
#pragma unroll
  for (int e = 0; e < kVadPerThread; ++e) {
    v[e] = first + e < n_frames ? vad[first + e] : 0;
    count += v[e];
  }
  int64_t total;
  int64_t r = tile_off[blockIdx.x] + vad_block_scan(count, sh, tid, &total);
#pragma unroll
  for (int e = 0; e < kVadPerThread; ++e) {
    if (first + e < n_frames) rank[first + e] = r;
    r += v[e];
  }
  if (blockIdx.x == 0 && tid == 0) rank[n_frames] = tile_off[tiles];
}

// ---------------------------------------------------------------------------------------------------------------- select
// 16 lanes per output row: they search together (every lane the same loads) and copy the row.
template <int V>
__global__ void __launch_bounds__(kVadThreads) vad_select_kernel(const float* __restrict__ rows, const uint8_t* __restrict__ vad,
                                                                 const int64_t* __restrict__ rank, int64_t n_frames, int F,
                                                                 int64_t n_out, float* __restrict__ out, int32_t* status) {
  const int l = threadIdx.x & 15;
  const int64_t jrow = (int64_t)blockIdx.x * (kVadThreads / 16) + (threadIdx.x >> 4);
  if (jrow >= n_out) return;
  const int64_t r = vad_find(rank, n_frames, jrow);  // the last r in [0, n_frames) with rank[r] <= jrow
  const bool ok = rank[r] == jrow && vad[r] == 1;
  if (!ok && l == 0) atomicOr(status, FHVAE_VAD_BAD_RANK);
  const float* src = rows + r * F;
  float* dst = out + jrow * F;
  if constexpr (V == 4) {
    for (int c = l * 4; c < F; c += 64) *(float4*)(dst + c) = ok ? *(const float4*)(src + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int c = l; c < F; c += 16) dst[c] = ok ? src[c] : 0.f;
  }
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_vad_energy(const float* wave, int64_t n_samples, const int64_t* wave_ptr, const int64_t* frame_ptr, int64_t U,
                                int64_t n_frames, int64_t frame_len, int64_t frame_shift, int mode, int flags, float* energy,
                                int32_t* status, void* stream) {
  FH_CHECK_PTR(wave);
  FH_CHECK_PTR(wave_ptr);
  FH_CHECK_PTR(frame_ptr);
  FH_CHECK_PTR(status);
  if (mode != FHVAE_VAD_RMS_CENTER && mode != FHVAE_VAD_LOGE_SNIP) return FHVAE_ERR_SHAPE;
  if ((flags & ~FHVAE_VAD_REMOVE_DC) != 0 || (flags != 0 && mode != FHVAE_VAD_LOGE_SNIP)) return FHVAE_ERR_SHAPE;
  if (frame_len < 2 || frame_shift < 1 || n_frames < 0) return FHVAE_ERR_SHAPE;
  if (frame_len > FHVAE_VAD_MAX_FRAME) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(frame_shift);
  if (n_frames == 0) return FHVAE_OK;
  FH_CHECK_PTR(energy);
  FH_CHECK_POS(U);
  FH_CHECK_POS(n_samples);
  int64_t tile = (kVadLdsSamples - frame_len) / frame_shift + 1;  // (tile - 1) * shift + len <= kVadLdsSamples
  tile = tile > kVadTileFrames ? kVadTileFrames : tile;
  const int64_t blocks = fh_cdiv(n_frames, tile), ublocks = fh_cdiv(U, kVadThreads);
  FH_CHECK_I32(blocks);
  FH_CHECK_I32(ublocks);
  const size_t lds = (size_t)((tile - 1) * frame_shift + frame_len) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(vad_energy_check_kernel, dim3((unsigned)ublocks), dim3(kVadThreads), 0, st, wave_ptr, frame_ptr, U, n_samples,
                     n_frames, frame_len, frame_shift, mode, status);
  const int vec = ((uintptr_t)wave & 15) == 0 ? 1 : 0;
  hipLaunchKernelGGL(vad_energy_kernel, dim3((unsigned)blocks), dim3(kVadThreads), lds, st, wave, n_samples, wave_ptr, frame_ptr, U,
                     n_frames, (int)frame_len, frame_shift, (int)tile, mode, flags, vec, energy, status);
  return fh_launch_status();
}

extern "C" int64_t fhvae_vad_ws_bytes(int64_t n_frames, int64_t U) {
  if (n_frames < 0 || U < 0) return FHVAE_ERR_SHAPE;
  return 8 * (vad_slots(n_frames, U) + U + fh_cdiv(n_frames, FHVAE_VAD_TILE) + 1);
}

extern "C" int fhvae_vad_decide(const float* energy, const int64_t* frame_ptr, int64_t U, int64_t n_frames, double thr_abs,
                                double mean_scale, int64_t ctx, float proportion, void* ws, int64_t ws_bytes, uint8_t* vad,
                                int64_t* rank, int32_t* status, void* stream) {
  FH_CHECK_PTR(frame_ptr);
  FH_CHECK_PTR(status);
  if (n_frames < 0 || ctx < 0) return FHVAE_ERR_SHAPE;
  if (!(proportion > 0.f && proportion <= 1.f)) return FHVAE_ERR_SHAPE;
  if (!(thr_abs - thr_abs == 0.0) || !(mean_scale - mean_scale == 0.0)) return FHVAE_ERR_SHAPE;  // (NaN or infinite)
  if (ctx > FHVAE_VAD_MAX_CTX) return FHVAE_ERR_LIMIT;
  if (n_frames == 0) return FHVAE_OK;
  FH_CHECK_PTR(energy);
  FH_CHECK_PTR(ws);
  FH_CHECK_PTR(vad);
  FH_CHECK_PTR(rank);
  FH_CHECK_POS(U);
  if (ws_bytes < fhvae_vad_ws_bytes(n_frames, U)) return FHVAE_ERR_SHAPE;
  if (((uintptr_t)ws & 7) != 0) return FHVAE_ERR_ALIGN;
  const VadWs w = vad_ws(ws, n_frames, U);
  const int64_t ublocks = fh_cdiv(U, kVadThreads);
  FH_CHECK_I32(w.slots);
  FH_CHECK_I32(w.tiles);
  FH_CHECK_I32(ublocks);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(vad_decide_check_kernel, dim3((unsigned)ublocks), dim3(kVadThreads), 0, st, frame_ptr, U, n_frames, status);
  hipLaunchKernelGGL(vad_partial_kernel, dim3((unsigned)w.slots), dim3(kVadThreads), 0, st, energy, frame_ptr, U, n_frames, w.partial,
                     status);
  hipLaunchKernelGGL(vad_threshold_kernel, dim3((unsigned)ublocks), dim3(kVadThreads), 0, st, frame_ptr, U, n_frames, w.slots,
                     w.partial, thr_abs, mean_scale, w.th, status);
  hipLaunchKernelGGL(vad_vote_kernel, dim3((unsigned)w.tiles), dim3(kVadThreads), 0, st, energy, frame_ptr, U, n_frames, w.th, ctx,
                     proportion, vad, w.tile_off, status);
  hipLaunchKernelGGL(vad_scan_kernel, dim3(1), dim3(kVadThreads), 0, st, w.tile_off, w.tiles, status);
  hipLaunchKernelGGL(vad_rank_kernel, dim3((unsigned)w.tiles), dim3(kVadThreads), 0, st, vad, n_frames, w.tile_off, w.tiles, rank,
                     status);
  return fh_launch_status();
}

extern "C" int fhvae_vad_select(const float* rows, const uint8_t* vad, const int64_t* rank, int64_t n_frames, int64_t F,
                                int64_t n_out, float* out, int32_t* status, void* stream) {
  FH_CHECK_PTR(status);
  if (n_frames < 0 || n_out < 0 || n_out > n_frames) return FHVAE_ERR_SHAPE;
  FH_CHECK_POS(F);
  FH_CHECK_I32(F);
  if (n_out == 0) return FHVAE_OK;
  FH_CHECK_PTR(rows);
  FH_CHECK_PTR(vad);
  FH_CHECK_PTR(rank);
  FH_CHECK_PTR(out);
  const bool vec = F % 4 == 0 && ((((uintptr_t)rows | (uintptr_t)out) & 15) == 0);
  const int64_t blocks = fh_cdiv(n_out, kVadThreads / 16);  // 16 lanes per output row
  FH_CHECK_I32(blocks);
  hipLaunchKernelGGL(vec ? vad_select_kernel<4> : vad_select_kernel<1>, dim3((unsigned)blocks), dim3(kVadThreads), 0,
                     (hipStream_t)stream, rows, vad, rank, n_frames, (int)F, n_out, out, status);
  return fh_launch_status();
}
