// hs.hip -- hierarchical sampling (Hsu & Glass 2018): the device work that runs before every block of K sequences.
//   fhvae_hs_select            : the block's segments in CSR order (block order, then segment order) + their local index
//   fhvae_mu2_accumulate_sorted: per-sequence sums of z2_mu over rows whose local index is non-decreasing, with no float
//                                atomics: each destination row is summed by ONE workgroup in a fixed order, so the result is
//                                bitwise reproducible for a fixed chunking
//   fhvae_mu2_load_table       : table rows = zsum / (count + ratio) written in place, their Adam moment rows zeroed and the
//                                accumulators cleared, in one launch
// Across ranks (the row-sharded K-row table of dist_shard): every rank accumulates a contiguous range of the block's segments,
//   fhvae_hs_pack_partials     : [zsum | count] into one (K, D+1) buffer (one all-gather moves it) and the accumulators cleared
//   fhvae_mu2_merge_load_shard : the W gathered partials of the rank's own rows summed in rank order, then loaded like
//                                fhvae_mu2_load_table: the order is fixed, so every rank loads the same bits for a given W
// Data-dependent errors (a bad sequence id, a total above cap, unsorted or out-of-range local indices) set bits of a
// device status word (FHVAE_HS_*) that the host reads once per block; no input makes a kernel read or write out of bounds.
#include "common.h"

namespace fh {

constexpr int kSelThreads = 1024;  // sequences per select tile (one workgroup each)
constexpr int kAccThreads = 256;   // 4 waves per accumulating workgroup
constexpr int kAccRows = 256;      // rows whose run starts a workgroup owns
constexpr int kAccPiece = 32;      // rows per piece of a long run; pieces go round-robin over the workgroup's row groups
constexpr int kAccShort = 256;     // longest run one row group sums alone
constexpr int kAccProbe = 64;      // rows a start slot scans linearly before it binary-searches for its run's end

// segment count of block sequence s (0 and a status bit for an id outside [0, S) or a decreasing seq_ptr)
__device__ __forceinline__ int64_t hs_count(const int64_t* __restrict__ seq_ptr, int64_t S, int64_t s, int32_t* status) {
  if (s < 0 || s >= S) {
    atomicOr(status, FHVAE_HS_BAD_SEQ);
    return 0;
  }
  const int64_t c = seq_ptr[s + 1] - seq_ptr[s];
  if (c < 0) {
    atomicOr(status, FHVAE_HS_BAD_SEQ);
    return 0;
  }
  return c;
}

__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  int64_t t = 0;
  for (int w = 0; w < nw; ++w) t += red[w];
  return t;
}

// One workgroup per tile of kSelThreads block sequences.  The tile's base offset is the sum of the counts of every
// earlier sequence (each workgroup reduces them itself: O(K^2 / 1024) reads of an L2-resident seq_ptr, no second launch
// and no workspace); an LDS scan over the tile; then the tile's segments are written with one thread per output position
// (binary search over the tile's offsets), coalesced.
__global__ void __launch_bounds__(kSelThreads) hs_select_kernel(const int64_t* __restrict__ seq_ptr, int64_t S,
                                                                 const int64_t* __restrict__ block_seqs, int64_t K,
                                                                 int64_t* __restrict__ seg_ids, int64_t* __restrict__ local_idx,
                                                                 int64_t* __restrict__ n_out, int64_t cap, int32_t* status) {
  __shared__ int64_t off[kSelThreads + 1];
  __shared__ int64_t red[kSelThreads / 64];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kSelThreads;
  int64_t pre = 0;
  for (int64_t i = t; i < i0; i += kSelThreads) pre += hs_count(seq_ptr, S, block_seqs[i], status);
  const int64_t base = block_sum_i64(pre, red);
  const int64_t i = i0 + t;
  const int64_t s = i < K ? block_seqs[i] : -1;
  const int64_t c = i < K ? hs_count(seq_ptr, S, s, status) : 0;
  // Hillis-Steele inclusive scan in LDS (10 steps)
  off[t + 1] = c;
  if (t == 0) off[0] = 0;
  __syncthreads();
  for (int d = 1; d < kSelThreads; d <<= 1) {
    const int64_t v = t + 1 - d >= 1 ? off[t + 1 - d] : 0;
    __syncthreads();
    off[t + 1] += v;
    __syncthreads();
  }
  const int64_t tile_n = off[kSelThreads];
  if (blockIdx.x == gridDim.x - 1 && t == 0) {
    const int64_t total = base + tile_n;
    *n_out = total;
    if (total > cap) atomicOr(status, FHVAE_HS_CAP);
  }
  const int64_t nt = K - i0 < kSelThreads ? K - i0 : kSelThreads;
  for (int64_t p = t; p < tile_n; p += kSelThreads) {
    const int64_t o = base + p;
    if (o >= cap) break;
    int lo = 0, hi = (int)nt - 1;  // last tile sequence j with off[j] <= p
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int64_t sj = block_seqs[i0 + lo];  // valid: a bad id has count 0 and owns no position
    seg_ids[o] = seq_ptr[sj] + (p - off[lo]);
    local_idx[o] = i0 + lo;
  }
}

// pre-pass of the sorted accumulation: every local index in [0, K), non-decreasing
__global__ void hs_check_sorted_kernel(const int64_t* __restrict__ idx, int64_t N, int64_t K, int32_t* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int64_t k = idx[i];
  if (k < 0 || k >= K) atomicOr(status, FHVAE_HS_BAD_IDX);
  if (i > 0 && idx[i - 1] > k) atomicOr(status, FHVAE_HS_UNSORTED);
}

// Owner-computes segmented sum.  Workgroup b owns the runs (maximal stretches of equal local index) that START in rows
// [b*kAccRows, (b+1)*kAccRows) and sums each of them whole, wherever it ends: every destination row has exactly one owner per
// call, which adds its sum to zsum / count with plain stores.
//   * each start slot finds its run's end itself (a short linear probe, then a binary search over the sorted rows);
//   * a run of at most kAccShort rows is summed by one row group (D lanes) in row order; slot j goes to group j % G;
//   * a longer run (Appendix B's skewed case) is spread over the whole workgroup: cut into pieces of kAccPiece rows from its
//     first row, piece q summed in row order by group q % G, and the G partial sums added in group order through LDS.
// The order depends only on the run's bounds inside this call: bitwise reproducible for a fixed chunking.
__global__ void __launch_bounds__(kAccThreads) mu2_acc_sorted_kernel(const float* __restrict__ z, const int64_t* __restrict__ idx,
                                                                      float* __restrict__ zsum, float* __restrict__ cnt, int64_t N,
                                                                      int64_t K, int64_t D, const int32_t* status) {
  __shared__ float part[kAccThreads];
  __shared__ int64_t runlen[kAccRows];  // 0: no run starts at this slot
  if (*status & (FHVAE_HS_BAD_IDX | FHVAE_HS_UNSORTED)) return;  // (set by the pre-pass: runs would not be unique)
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kAccRows;
  {
    const int64_t a = r0 + t;
    int64_t n = 0;
    if (a < N && (a == 0 || idx[a - 1] != idx[a])) {
      const int64_t k = idx[a];
      int64_t e = a + 1;
      while (e < N && e - a < kAccProbe && idx[e] == k) ++e;
      if (e < N && e - a == kAccProbe && idx[e] == k) {  // long run: binary search for its end in (e, N]
        int64_t lo = e + 1, hi = N;
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (idx[mid] == k) lo = mid + 1; else hi = mid;
        }
        e = lo;
      }
      n = e - a;
    }
    runlen[t] = n;
  }
  __syncthreads();
  const int G = (int)(kAccThreads / D);
  const int g = t / (int)D, d = t % (int)D;
  if (g < G) {
    for (int j = g; j < kAccRows; j += G) {
      const int64_t n = runlen[j];
      if (n == 0 || n > kAccShort) continue;
      const int64_t a = r0 + j, k = idx[a];
      const float* zr = z + a * D + d;
      float s = 0.f;
      for (int64_t r = 0; r < n; ++r, zr += D) s += *zr;
      if (k >= 0 && k < K) {
        zsum[k * D + d] = zsum[k * D + d] + s;
        if (d == 0) cnt[k] = cnt[k] + (float)n;
      }
    }
  }
  for (int j = 0; j < kAccRows; ++j) {
    const int64_t n = runlen[j];  // (uniform: LDS broadcast)
    if (n <= kAccShort) continue;
    const int64_t a = r0 + j, k = idx[a];
    float acc = 0.f;
    if (g < G) {
      for (int64_t q = g; q * kAccPiece < n; q += G) {
        const int64_t e = (q + 1) * kAccPiece < n ? (q + 1) * kAccPiece : n;
        const float* zr = z + (a + q * kAccPiece) * D + d;
        for (int64_t r = q * kAccPiece; r < e; ++r, zr += D) acc += *zr;
      }
    }
    part[t] = acc;
    __syncthreads();
    if (t < D && k >= 0 && k < K) {
      float s = part[t];
      for (int h = 1; h < G; ++h) s += part[h * D + t];
      zsum[k * D + t] = zsum[k * D + t] + s;
      if (t == 0) cnt[k] = cnt[k] + (float)n;
    }
    __syncthreads();
  }
}

// one wave per table row: lanes read the row's count, write the row and zero its moments; lane 0 clears the count last
// (its store follows the row stores that consumed the loaded count, so no lane reads a cleared count)
__global__ void mu2_load_table_kernel(float* __restrict__ zsum, float* __restrict__ cnt, float* __restrict__ table,
                                      float* __restrict__ m, float* __restrict__ v, int64_t K, int64_t D, float ratio) {
  const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (k >= K) return;
  const float n = cnt[k];
  for (int64_t d = lane; d < D; d += 64) {
    const int64_t e = k * D + d;
    table[e] = n > 0.f ? zsum[e] / (n + ratio) : 0.f;  // utils.py:57-59, as mu2_finalize_kernel
    m[e] = 0.f;
    v[e] = 0.f;
    zsum[e] = 0.f;
  }
  if (lane == 0) cnt[k] = n * 0.f;  // (a store whose value depends on the loaded count: issued after every lane read it)
}

// one thread per element of the (K, D+1) buffer: column D carries the count; each thread clears what it read
__global__ void hs_pack_partials_kernel(float* __restrict__ zsum, float* __restrict__ cnt, float* __restrict__ out, int64_t K,
                                        int64_t D) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= K * (D + 1)) return;
  const int64_t k = e / (D + 1), d = e - k * (D + 1);
  if (d < D) {
    out[e] = zsum[k * D + d];
    zsum[k * D + d] = 0.f;
  } else {
    out[e] = cnt[k];
    cnt[k] = 0.f;
  }
}

// one thread per element of the shard's rows [row0, row1): the W partials of its row are added one rank after the other
// (rank 0 first), the count the same way, so the result does not depend on the transport that gathered them
__global__ void mu2_merge_load_shard_kernel(const float* __restrict__ parts, int64_t W, int64_t K, int64_t row0, int64_t rows,
                                            float* __restrict__ shard, float* __restrict__ m, float* __restrict__ v, int64_t D,
                                            float ratio) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rows * D) return;
  const int64_t r = e / D, d = e - r * D;
  const float* p = parts + (row0 + r) * (D + 1);
  const int64_t step = K * (D + 1);
  float s = 0.f, n = 0.f;
  for (int64_t w = 0; w < W; ++w, p += step) {
    s += p[d];
    n += p[D];
  }
  shard[e] = n > 0.f ? s / (n + ratio) : 0.f;  // as mu2_load_table_kernel
  m[e] = 0.f;
  v[e] = 0.f;
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_hs_select(const int64_t* seq_ptr, int64_t S, const int64_t* block_seqs, int64_t K, int64_t* seg_ids,
                               int64_t* local_idx, int64_t* n_out, int64_t cap, int32_t* status, void* stream) {
  FH_CHECK_PTR(seq_ptr);
  FH_CHECK_PTR(block_seqs);
  FH_CHECK_PTR(n_out);
  FH_CHECK_PTR(status);
  FH_CHECK_POS(S);
  FH_CHECK_POS(K);
  if (cap < 0) return FHVAE_ERR_SHAPE;
  if (cap > 0 && (seg_ids == nullptr || local_idx == nullptr)) return FHVAE_ERR_NULL;
  FH_CHECK_I32(fh_cdiv(K, kSelThreads));
  hipLaunchKernelGGL(hs_select_kernel, dim3((unsigned)fh_cdiv(K, kSelThreads)), dim3(kSelThreads), 0, (hipStream_t)stream,
                     seq_ptr, S, block_seqs, K, seg_ids, local_idx, n_out, cap, status);
  return fh_launch_status();
}

extern "C" int fhvae_mu2_accumulate_sorted(const float* z2_mu, const int64_t* local_idx, float* zsum, float* count, int64_t N,
                                           int64_t K, int64_t D, int32_t* status, void* stream) {
  FH_CHECK_PTR(z2_mu);
  FH_CHECK_PTR(local_idx);
  FH_CHECK_PTR(zsum);
  FH_CHECK_PTR(count);
  FH_CHECK_PTR(status);
  FH_CHECK_POS(N);
  FH_CHECK_POS(K);
  FH_CHECK_POS(D);
  if (D > kAccThreads) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(fh_cdiv(N, 256));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(hs_check_sorted_kernel, dim3((unsigned)fh_cdiv(N, 256)), dim3(256), 0, s, local_idx, N, K, status);
  int rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  hipLaunchKernelGGL(mu2_acc_sorted_kernel, dim3((unsigned)fh_cdiv(N, kAccRows)), dim3(kAccThreads), 0, s, z2_mu, local_idx,
                     zsum, count, N, K, D, status);
  return fh_launch_status();
}

extern "C" int fhvae_mu2_load_table(float* zsum, float* count, float* table, float* m_rows, float* v_rows, int64_t K, int64_t D,
                                    float ratio, void* stream) {
  FH_CHECK_PTR(zsum);
  FH_CHECK_PTR(count);
  FH_CHECK_PTR(table);
  FH_CHECK_PTR(m_rows);
  FH_CHECK_PTR(v_rows);
  FH_CHECK_POS(K);
  FH_CHECK_POS(D);
  FH_CHECK_I32(fh_cdiv(K * 64, 256));
  hipLaunchKernelGGL(mu2_load_table_kernel, dim3((unsigned)fh_cdiv(K * 64, 256)), dim3(256), 0, (hipStream_t)stream, zsum, count,
                     table, m_rows, v_rows, K, D, ratio);
  return fh_launch_status();
}

extern "C" int fhvae_hs_pack_partials(float* zsum, float* count, float* out, int64_t K, int64_t D, void* stream) {
  FH_CHECK_PTR(zsum);
  FH_CHECK_PTR(count);
  FH_CHECK_PTR(out);
  FH_CHECK_POS(K);
  FH_CHECK_POS(D);
  FH_CHECK_I32(fh_cdiv(K * (D + 1), 256));
  hipLaunchKernelGGL(hs_pack_partials_kernel, dim3((unsigned)fh_cdiv(K * (D + 1), 256)), dim3(256), 0, (hipStream_t)stream, zsum,
                     count, out, K, D);
  return fh_launch_status();
}

extern "C" int fhvae_mu2_merge_load_shard(const float* parts, int64_t W, int64_t K, int64_t row0, int64_t row1, float* shard,
                                          float* m_rows, float* v_rows, int64_t D, float ratio, void* stream) {
  FH_CHECK_PTR(parts);
  FH_CHECK_POS(W);
  FH_CHECK_POS(K);
  FH_CHECK_POS(D);
  if (row0 < 0 || row1 < row0 || row1 > K) return FHVAE_ERR_SHAPE;
  if (row1 == row0) return FHVAE_OK;  // an empty shard (more ranks than rows): nothing to load
  FH_CHECK_PTR(shard);
  FH_CHECK_PTR(m_rows);
  FH_CHECK_PTR(v_rows);
  FH_CHECK_I32(fh_cdiv((row1 - row0) * D, 256));
  hipLaunchKernelGGL(mu2_merge_load_shard_kernel, dim3((unsigned)fh_cdiv((row1 - row0) * D, 256)), dim3(256), 0,
                     (hipStream_t)stream, parts, W, K, row0, row1 - row0, shard, m_rows, v_rows, D, ratio);
  return fh_launch_status();
}
