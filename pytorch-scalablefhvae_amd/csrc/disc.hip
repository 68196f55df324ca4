// disc.hip -- K5, the discriminative log-sum-exp cross-entropy over the mu2 table (simple_fhvae.py:119-122): everything that is
// not a matrix-core kernel body.  The engine choice (disc_engine: the VALU direct form here, the exact-f32 MFMA kernel of
// disc_mfma.hip, the bf16 split-operand MFMA kernel of disc_lp.hip), the grids and workspaces, the VALU kernels, the kernels every
// engine shares (combine, own-row backward, CE mean, the reductions of the one-pass backward, the merge of row shards' partials)
// and the exported entry points.
#include <algorithm>
#include <cstdlib>

#include "disc_tile.h"

namespace fh {

// ---------------------------------------------------------------------------------------------
// The VALU direct form (small problems, D not 16 / 32, FHVAE_DISC_VALU).
// Forward: thread = query b (q row in registers), table rows are wave-uniform -> scalar loads
// (s_load_dwordx*), so per (b,s) pair the VALU does only the 2*D sub/fma and the online-LSE
// update; nothing of size B*S is written.  grid = (query tiles of 256) x (row chunks).
// ---------------------------------------------------------------------------------------------
struct DiscPlan {
  int chunk;    // table rows per workgroup
  int nchunks;
  int btiles;
};
static inline DiscPlan disc_plan(int64_t B, int64_t S) {
  DiscPlan p;
  p.btiles = (int)fh_cdiv(B, 256);
  int64_t want = fh_cdiv(1024, p.btiles);  // aim at ~1024 workgroups
  int64_t chunk = fh_cdiv(S, want);
  chunk = fh_cdiv(chunk, 8) * 8;
  if (chunk < 8) chunk = 8;
  p.chunk = (int)chunk;
  p.nchunks = (int)fh_cdiv(S, chunk);
  return p;
}

template <int D>
__device__ __forceinline__ float sqdist(const float (&q)[D], const float* __restrict__ trow) {
  float a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int d = 0; d < D; d += 2) {
    const float d0 = q[d] - trow[d], d1 = q[d + 1] - trow[d + 1];
    a0 = fmaf(d0, d0, a0);
    a1 = fmaf(d1, d1, a1);
  }
  return a0 + a1;
}

template <int D>
__global__ __launch_bounds__(256) void disc_fwd_kernel(const float* __restrict__ q, const float* __restrict__ table,
                                                       float c, float2* __restrict__ part, int B, int S, int chunk) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  const int bb = b < B ? b : B - 1;
  float qr[D];
#pragma unroll
  for (int d = 0; d < D; ++d) qr[d] = q[(int64_t)bb * D + d];
  const int s0 = blockIdx.y * chunk;
  const int s1 = min(S, s0 + chunk);
  float m = -INFINITY, sum = 0.f;
  for (int s = s0; s < s1; s += 8) {
    float l[8];
    float gm = -INFINITY;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int su = s + u;
      // rows past the chunk end are clamped (uniform scalar address) and masked to -inf
      const float* trow = table + (int64_t)(su < s1 ? su : s1 - 1) * D;
      l[u] = su < s1 ? -c * sqdist<D>(qr, trow) : -INFINITY;
      gm = fmaxf(gm, l[u]);
    }
    if (gm > m) {
      sum *= __expf(m - gm);  // m = -inf on the first group: exp(-inf) = 0
      m = gm;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += __expf(l[u] - m);
  }
  if (b < B) part[(int64_t)blockIdx.y * B + b] = make_float2(m, sum);
}

// one WAVE per query: lanes stride over the chunk partials (a thread-per-query loop was a chain of nchunks
// dependent L2 loads: 165 us for 144 chunks), then a wave-level (max, sum) merge; lane 0 also evaluates the
// target logit.
template <int D>
__global__ __launch_bounds__(256) void disc_combine_kernel(const float* __restrict__ q, const float* __restrict__ table,
                                                           const int64_t* __restrict__ idx, int64_t row0, float c,
                                                           const float2* __restrict__ part, int nchunks,
                                                           float* __restrict__ row_max, float* __restrict__ row_sum,
                                                           float* __restrict__ tgt, int B, int S, int own_excluded) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  float m = -INFINITY, sum = 0.f;
  for (int k = lane; k < nchunks; k += 64) {
    const float2 p = part[(int64_t)k * B + b];
    if (p.x > m) {
      sum = sum * __expf(m - p.x) + p.y;
      m = p.x;
    } else {
      sum += p.y * __expf(p.x - m);
    }
  }
  const float gm = wave_max(m);
  sum = m == -INFINITY ? 0.f : sum * __expf(m - gm);
  sum = wave_sum(sum);
  // target logit with EXACTLY the arithmetic of disc_fwd_kernel (same sqdist order), so that a target that is the
  // row maximum gives (max - target) == 0 bit for bit
  const int64_t s = idx[b] - row0;
  if (lane == 0) {
    float t = 0.f;
    if (s >= 0 && s < S) {
      float qr[D];
#pragma unroll
      for (int d = 0; d < D; ++d) qr[d] = q[(int64_t)b * D + d];
      t = -c * sqdist<D>(qr, table + s * D);
      if (own_excluded) {
        // the MFMA kernels left the query's own row out of the partials (disc_tile.h): its exact logit joins here
        const float nm = fmaxf(gm, t);
        sum = (gm == -INFINITY ? 0.f : sum * __expf(gm - nm)) + __expf(t - nm);
        row_max[b] = nm;
        row_sum[b] = sum;
        tgt[b] = t;
        return;
      }
    }
    row_max[b] = gm;
    row_sum[b] = sum;
    tgt[b] = t;
  }
}

// Backward of the (query, own row) pairs the MFMA kernels leave out: w = g (p_own - 1), p_own = exp(target - max) / sum with the
// DIRECT-form target logit; dq[b] += -2c w (q_b - t_y), dtable[y] += +2c w (q_b - t_y).  One thread per (query, 4 dims).
template <int D>
__global__ __launch_bounds__(256) void disc_own_bwd_kernel(const float* __restrict__ q, const float* __restrict__ table,
                                                           const int64_t* __restrict__ idx, int64_t row0, float c,
                                                           const float* __restrict__ rmax, const float* __restrict__ rsum,
                                                           const float* __restrict__ gsc, float gmul, float* __restrict__ dq,
                                                           float* __restrict__ dtable, int B, int S) {
  constexpr int PER = D / 4;  // threads per query
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int b = tid / PER, part = tid % PER;
  if (b >= B) return;
  const int64_t s = idx[b] - row0;
  if (s < 0 || s >= S) return;
  float qr[D];
#pragma unroll
  for (int d = 0; d < D; ++d) qr[d] = q[(int64_t)b * D + d];
  const float t = -c * sqdist<D>(qr, table + s * D);
  const float w = (*gsc) * gmul * (__expf(t - rmax[b]) / rsum[b] - 1.f);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = part * 4 + k;
    const float diff = qr[d] - table[s * D + d];
    if (dq) atomicAdd(dq + (int64_t)b * D + d, -2.f * c * w * diff);
    if (dtable) atomicAdd(dtable + s * D + d, 2.f * c * w * diff);
  }
}

// single-workgroup deterministic mean of (max + log(sumexp) - target)
__global__ __launch_bounds__(256) void ce_mean_kernel(const float* __restrict__ row_max, const float* __restrict__ row_sum,
                                                      const float* __restrict__ tgt, float* __restrict__ out, int B, float scale) {
  __shared__ float red[4];
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) s += (row_max[b] - tgt[b]) + logf(row_sum[b]);  // exact 0 + log s when the target row is the max
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = scale * ((red[0] + red[1] + red[2] + red[3]) / (float)B);
}

// merge of the W ranks' K5 partials (dist_shard.py; parts[w] = [max | sumexp | target], N each): m = max_w, s = sum_w sumexp_w exp(max_w - m),
// t = sum_w target_w.  An empty shard's (-inf, 0, 0) contributes exp(-inf) * 0 = 0.
__global__ void disc_merge_kernel(const float* __restrict__ parts, float* __restrict__ m, float* __restrict__ s, float* __restrict__ t,
                                  int W, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float mx = -INFINITY;
  for (int w = 0; w < W; ++w) mx = fmaxf(mx, parts[((int64_t)w * 3 + 0) * N + i]);
  float ss = 0.f, tt = 0.f;
  for (int w = 0; w < W; ++w) {
    const float rm = parts[((int64_t)w * 3 + 0) * N + i], rs = parts[((int64_t)w * 3 + 1) * N + i];
    ss += rs > 0.f ? rs * __expf(rm - mx) : 0.f;
    tt += parts[((int64_t)w * 3 + 2) * N + i];
  }
  m[i] = mx, s[i] = ss, t[i] = tt;
}

// rows row0 .. row0 + 255 (those below nrows) of a [nrows][D] matrix from the transpose buffer, contiguous along the rows
// (MI355X_MICROARCH.md, float atomics), added with atomics
template <int D>
__device__ __forceinline__ void add_rows(float* __restrict__ dst, const float (*tr)[D + 1], int row0, int nrows) {
  for (int e = threadIdx.x; e < 256 * D; e += 256) {
    const int rr = e / D, d = e % D;
    const int x = row0 + rr;
    if (x < nrows)
      atomicAdd(dst + (int64_t)x * D + d, tr[rr][d]);
  }
}

// Backward, query side: dq[b,:] = -2c * sum_s w_bs (q_b - t_s), w = g (p - onehot)
template <int D>
__global__ __launch_bounds__(256) void disc_bwd_dq_kernel(const float* __restrict__ q, const float* __restrict__ table,
                                                          const int64_t* __restrict__ idx, int64_t row0, float c,
                                                          const float* __restrict__ rmax, const float* __restrict__ rsum,
                                                          const float* __restrict__ gsc, float gmul,
                                                          float* __restrict__ dq, int B, int S, int chunk) {
  __shared__ float tr[256][D + 1];
  const int b = blockIdx.x * 256 + threadIdx.x;
  const int bb = b < B ? b : B - 1;
  float qr[D], V[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    qr[d] = q[(int64_t)bb * D + d];
    V[d] = 0.f;
  }
  const float g = *gsc * gmul;
  // p = exp(logit - max) / sumexp: the max is one of the logits exactly, so the subtraction is exact for
  // the rows that matter (an lse = max + log(sum) would carry the ulp of |max| ~ 1e3 into every p)
  const float mb = rmax[bb], inv_s = 1.f / rsum[bb];
  const int64_t tg = idx[bb] - row0;
  const int s0 = blockIdx.y * chunk, s1 = min(S, s0 + chunk);
  for (int s = s0; s < s1; ++s) {
    const float* trow = table + (int64_t)s * D;
    float df[D];
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int d = 0; d < D; d += 2) {
      df[d] = qr[d] - trow[d];
      df[d + 1] = qr[d + 1] - trow[d + 1];
      a0 = fmaf(df[d], df[d], a0);
      a1 = fmaf(df[d + 1], df[d + 1], a1);
    }
    const float lg = -c * (a0 + a1);
    const float w = g * (__expf(lg - mb) * inv_s - (s == tg ? 1.f : 0.f));
#pragma unroll
    for (int d = 0; d < D; ++d) V[d] = fmaf(w, df[d], V[d]);
  }
  // transpose through LDS so the atomics go out as contiguous rows
#pragma unroll
  for (int d = 0; d < D; ++d) tr[threadIdx.x][d] = -2.f * c * V[d];
  __syncthreads();
  add_rows<D>(dq, tr, blockIdx.x * 256, B);
}

// Backward, table side: thread = table row s (row in registers), queries are wave-uniform.
// dtable[s,:] += 2c * sum_b w_bs (q_b - t_s)
template <int D>
__global__ __launch_bounds__(256) void disc_bwd_dt_kernel(const float* __restrict__ q, const float* __restrict__ table,
                                                          const int64_t* __restrict__ idx, int64_t row0, float c,
                                                          const float* __restrict__ rmax, const float* __restrict__ rsum,
                                                          const float* __restrict__ gsc, float gmul,
                                                          float* __restrict__ dtable, int B, int S, int bchunk) {
  __shared__ float tr[256][D + 1];
  const int s = blockIdx.x * 256 + threadIdx.x;
  const int ss = s < S ? s : S - 1;
  float t[D], U[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    t[d] = table[(int64_t)ss * D + d];
    U[d] = 0.f;
  }
  const float g = *gsc * gmul;
  const int b0 = blockIdx.y * bchunk, b1 = min(B, b0 + bchunk);
  for (int b = b0; b < b1; ++b) {
    const float* qrow = q + (int64_t)b * D;
    float df[D];
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int d = 0; d < D; d += 2) {
      df[d] = qrow[d] - t[d];
      df[d + 1] = qrow[d + 1] - t[d + 1];
      a0 = fmaf(df[d], df[d], a0);
      a1 = fmaf(df[d + 1], df[d + 1], a1);
    }
    const float lg = -c * (a0 + a1);
    const float w = g * (__expf(lg - rmax[b]) / rsum[b] - ((int64_t)s == idx[b] - row0 ? 1.f : 0.f));
#pragma unroll
    for (int d = 0; d < D; ++d) U[d] = fmaf(w, df[d], U[d]);
  }
#pragma unroll
  for (int d = 0; d < D; ++d) tr[threadIdx.x][d] = 2.f * c * U[d];
  __syncthreads();
  add_rows<D>(dtable, tr, blockIdx.x * 256, S);
}

// the reductions of the one-pass backward's partials (MODE 2 of both MFMA kernels; disc_lp.hip has the reasoning)
// dY[y][d] += 2c (sum_xt G2[xt][y][d] - Y[y][d] sum_xt WY[xt][y])
__global__ void disc_dt_finish_kernel(float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ g2,
                                      const float* __restrict__ wy, int nxt, float c2, int64_t NY, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= NY * D) return;
  const int64_t row = i / D;
  float sg = 0.f, sw = 0.f;
  for (int t = 0; t < nxt; ++t) {
    sg += g2[(int64_t)t * NY * D + i];
    sw += wy[(int64_t)t * NY + row];
  }
  dy[i] += c2 * (sg - y[i] * sw);
}
// dX[i] = sum_chunks G[chunk][i]
__global__ void disc_dq_reduce_kernel(float* __restrict__ dx, const float* __restrict__ g, int nchunks, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int c = 0;
  for (; c + 4 <= nchunks; c += 4) {
    a0 += g[(int64_t)c * n + i], a1 += g[(int64_t)(c + 1) * n + i], a2 += g[(int64_t)(c + 2) * n + i], a3 += g[(int64_t)(c + 3) * n + i];
  }
  for (; c < nchunks; ++c) a0 += g[(int64_t)c * n + i];
  dx[i] = (a0 + a1) + (a2 + a3);
}
// ---------------------------------------------------------------------------------------------
// Which engine runs a call.  The only reader of FHVAE_DISC_VALU, and the only place that knows: the matrix cores for D = 16 / 32
// and B S >= 2^16 (below that the VALU form's launch is the cost), the bf16 kernel only for D = 32 (otherwise the bf16 compute
// mode runs the f32 kernel).
// ---------------------------------------------------------------------------------------------
enum DiscEngine { kDiscValu, kDiscF32, kDiscBf16 };
static DiscEngine disc_engine(int64_t B, int64_t S, int64_t D, int dtype) {
  if (!((D == 32 || D == 16) && B * S >= (int64_t)1 << 16) || getenv("FHVAE_DISC_VALU")) return kDiscValu;
  return (dtype == FHVAE_BF16 && D == 32) ? kDiscBf16 : kDiscF32;
}
static int launch_mfma(DiscEngine engine, int64_t D, int mode, const DiscMfmaArgs& a, dim3 grid, hipStream_t st) {
  if (engine == kDiscBf16)
    disc_lp_launch(a, mode, grid, st);
  else
    disc_f32_launch(a, (int)D, mode, grid, st);
  return fh_launch_status();
}

// streamed vectors per workgroup for about `target` workgroups.  Forward (one partial per (chunk, x)): 1024.  Backward: every
// workgroup adds its whole 256 x D partial gradient with atomics, so fewer, longer chunks pay (c2, S = 4600: 0.103 -> 0.078 ms per
// step with 512; 384 and fewer lose on the large tables: S = 1M backward 6.4 ms with 512, 7.5 ms with 384)
static int mfma_chunk(int64_t nx, int64_t ny, int target) {
  const int64_t xt = fh_cdiv(nx, 256);
  return (int)fh_allpairs_chunk(ny, fh_cdiv(target, xt), 64);
}
// the stationary / streamed sets of a launch and its grid: queries stationary (forward, dq, one pass) or table rows (dtable)
static dim3 set_sides(DiscMfmaArgs& a, bool x_is_query, const float* q, int64_t B, const float* table, int64_t S, int target) {
  a.X = x_is_query ? q : table;
  a.Y = x_is_query ? table : q;
  a.NX = (int)(x_is_query ? B : S);
  a.NY = (int)(x_is_query ? S : B);
  a.x_is_query = x_is_query;
  a.chunk = mfma_chunk(a.NX, a.NY, target);
  return dim3((unsigned)fh_cdiv(a.NY, a.chunk), (unsigned)fh_cdiv(a.NX, 256));
}

// one-pass backward: the queries go in groups of `tiles` 256-query tiles; a group needs its chunks' partials of dq
// (nchunks x rows x D floats) and tiles x S x (D + 1) floats of the streamed side's partial sums
static int64_t onepass_group_bytes(int64_t tiles, int64_t B, int64_t S, int64_t D) {
  const int64_t rows = std::min<int64_t>(B, tiles * 256);
  const int64_t nchunks = fh_cdiv(S, mfma_chunk(rows, S, 512));
  return (nchunks * rows * D + tiles * S * (D + 1)) * (int64_t)sizeof(float);
}
// the most tiles per group (<= all of them) whose partials fit `bytes`; 0: not even one
static int64_t onepass_group_tiles(int64_t bytes, int64_t B, int64_t S, int64_t D) {
  const int64_t nxt = fh_cdiv(B, 256);
  int64_t lo = 0, hi = nxt;  // (the size grows with the tile count)
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if (onepass_group_bytes(mid, B, S, D) <= bytes) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

static int disc_mfma_fwd(DiscEngine engine, const float* q, const float* table, const int64_t* idx, int64_t row0, float c, float2* part,
                         int* nchunks, int64_t B, int64_t S, int64_t D, hipStream_t st) {
  DiscMfmaArgs a = {};
  a.c = c;
  a.idx = idx;
  a.row0 = row0;
  a.part = part;
  const dim3 grid = set_sides(a, true, q, B, table, S, 1024);
  *nchunks = (int)grid.x;
  return launch_mfma(engine, D, 0, a, grid, st);
}

// ws / ws_bytes: workspace (or NULL / 0): with it and dq AND dtable wanted, both gradients come from one recomputation of the
// logits, the queries in groups of as many 256-query tiles as the workspace holds the partial sums of; otherwise (or with less
// than one tile's worth) one pass per gradient.  fhvae_disc_lse_bwd_ws_bytes = the recommended size: the whole problem in one
// group up to kOnePassWsCap.
constexpr int64_t kOnePassWsCap = 3LL << 29;  // 1.5 GiB
static int disc_mfma_bwd(DiscEngine engine, const float* q, const float* table, const int64_t* idx, int64_t row0, float c,
                         const float* rmax, const float* rsum, const float* gsc, float gmul, float* dq, float* dtable, float* ws,
                         int64_t ws_bytes, int64_t B, int64_t S, int64_t D, hipStream_t st) {
  DiscMfmaArgs a = {};
  a.c = c;
  a.idx = idx;
  a.row0 = row0;
  a.rmax = rmax;
  a.rsum = rsum;
  a.gsc = gsc;
  a.gmul = gmul;
  const int64_t gtiles = (dq && dtable && ws) ? onepass_group_tiles(ws_bytes, B, S, D) : 0;
  if (gtiles > 0) {
    // one pass: stationary = queries, streamed = table rows; dq as in the two-pass form, dtable from the same weights.  Query
    // groups of gtiles tiles, one after the other on the same workspace (dtable accumulates over the groups)
    for (int64_t x0 = 0; x0 < B; x0 += gtiles * 256) {
      const int64_t nb = std::min<int64_t>(B - x0, gtiles * 256);
      a.idx = idx + x0;
      a.rmax = rmax + x0;
      a.rsum = rsum + x0;
      const dim3 grid = set_sides(a, true, q + x0 * D, nb, table, S, 512);
      const int64_t nchunks = grid.x, nxt = grid.y;
      a.G = ws;                       // [nchunks][nb, D]
      a.G2 = a.G + nchunks * nb * D;  // [nxt][S, D]
      a.WY = a.G2 + nxt * S * D;      // [nxt][S]
      int e = launch_mfma(engine, D, 2, a, grid, st);
      if (e) return e;
      hipLaunchKernelGGL(disc_dq_reduce_kernel, dim3((unsigned)fh_cdiv(nb * D, 256)), dim3(256), 0, st, dq + x0 * D, a.G, (int)nchunks, nb * D);
      hipLaunchKernelGGL(disc_dt_finish_kernel, dim3((unsigned)fh_cdiv(S * D, 256)), dim3(256), 0, st, dtable, table, a.G2, a.WY, (int)nxt,
                         2.f * c, S, (int)D);
      e = fh_launch_status();
      if (e) return e;
    }
    return FHVAE_OK;
  }
  if (dq) {  // stationary = queries, streamed = table rows; the workgroups ADD their partial gradients: zero first
    hipError_t he = hipMemsetAsync(dq, 0, (size_t)(B * D) * sizeof(float), st);
    if (he != hipSuccess) return (int)he;
    const dim3 grid = set_sides(a, true, q, B, table, S, 512);
    a.G = dq;
    int e = launch_mfma(engine, D, 1, a, grid, st);
    if (e) return e;
  }
  if (dtable) {  // stationary = table rows, streamed = queries
    const dim3 grid = set_sides(a, false, q, B, table, S, 512);
    a.G = dtable;
    int e = launch_mfma(engine, D, 1, a, grid, st);
    if (e) return e;
  }
  return FHVAE_OK;
}

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_disc_lse_bwd_ws_bytes(int64_t B, int64_t S, int64_t D) {
  if (B <= 0 || S <= 0 || D <= 0 || disc_engine(B, S, D, FHVAE_F32) == kDiscValu) return 0;  // (both MFMA engines: the same partials)
  const int64_t t = onepass_group_tiles(kOnePassWsCap, B, S, D);
  return t > 0 ? onepass_group_bytes(t, B, S, D) : 0;
}

// (max, sumexp) per (chunk, query).  The query has no D to ask disc_engine with: the larger of the VALU form's grid and the MFMA one's
extern "C" int64_t fhvae_disc_lse_ws_bytes(int64_t B, int64_t S) {
  if (B <= 0 || S <= 0) return 0;
  const int64_t nchunks = std::max<int64_t>(disc_plan(B, S).nchunks, fh_cdiv(S, mfma_chunk(B, S, 1024)));
  return nchunks * B * (int64_t)sizeof(float2);
}

#define DISC_DISPATCH(D_, CALL) \
  switch (D_) {                 \
    case 4: { constexpr int DD = 4; CALL; } break;   \
    case 8: { constexpr int DD = 8; CALL; } break;   \
    case 16: { constexpr int DD = 16; CALL; } break; \
    case 32: { constexpr int DD = 32; CALL; } break; \
    case 64: { constexpr int DD = 64; CALL; } break; \
    default: return FHVAE_ERR_SHAPE;                 \
  }

extern "C" int fhvae_disc_lse_fwd(const float* q, const float* table, const int64_t* idx, int64_t row0, float inv_two_var,
                                  float* row_max, float* row_sumexp, float* tgt_logit, float* ce_mean, float ce_scale, void* ws,
                                  int64_t B, int64_t S, int64_t D, int dtype, void* stream) {
  if (dtype != FHVAE_F32 && dtype != FHVAE_BF16) return FHVAE_ERR_DTYPE;
  FH_CHECK_PTR(q);
  FH_CHECK_PTR(table);
  FH_CHECK_PTR(idx);
  FH_CHECK_PTR(row_max);
  FH_CHECK_PTR(row_sumexp);
  FH_CHECK_PTR(tgt_logit);
  FH_CHECK_PTR(ws);
  FH_CHECK_POS(B);
  FH_CHECK_POS(S);
  FH_CHECK_I32(B);
  FH_CHECK_I32(S);
  hipStream_t st = (hipStream_t)stream;
  DiscPlan p = disc_plan(B, S);
  float2* part = (float2*)ws;
  int e, own_excluded = 0;
  const DiscEngine engine = disc_engine(B, S, D, dtype);
  if (engine != kDiscValu) {
    e = disc_mfma_fwd(engine, q, table, idx, row0, inv_two_var, part, &p.nchunks, B, S, D, st);
    own_excluded = 1;
  } else {
    dim3 grid((unsigned)p.btiles, (unsigned)p.nchunks);
    DISC_DISPATCH(D, hipLaunchKernelGGL((disc_fwd_kernel<DD>), grid, dim3(256), 0, st, q, table, inv_two_var, part, (int)B,
                                        (int)S, p.chunk));
    e = fh_launch_status();
  }
  if (e) return e;
  DISC_DISPATCH(D, hipLaunchKernelGGL((disc_combine_kernel<DD>), dim3((unsigned)fh_cdiv(B, 4)), dim3(256), 0, st, q, table, idx,
                                      row0, inv_two_var, part, p.nchunks, row_max, row_sumexp, tgt_logit, (int)B, (int)S,
                                      own_excluded));
  e = fh_launch_status();
  if (e) return e;
  if (ce_mean) {
    hipLaunchKernelGGL(ce_mean_kernel, dim3(1), dim3(256), 0, st, row_max, row_sumexp, tgt_logit, ce_mean, (int)B, ce_scale);
    e = fh_launch_status();
  }
  return e;
}

extern "C" int fhvae_disc_ce_mean(const float* row_max, const float* row_sumexp, const float* tgt_logit, float* ce_mean,
                                  float ce_scale, int64_t B, void* stream) {
  FH_CHECK_PTR(row_max);
  FH_CHECK_PTR(row_sumexp);
  FH_CHECK_PTR(tgt_logit);
  FH_CHECK_PTR(ce_mean);
  FH_CHECK_POS(B);
  FH_CHECK_I32(B);
  hipLaunchKernelGGL(ce_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_max, row_sumexp, tgt_logit, ce_mean,
                     (int)B, ce_scale);
  return fh_launch_status();
}

extern "C" int fhvae_disc_merge_partials(const float* parts, float* row_max, float* row_sumexp, float* tgt_logit, int64_t W, int64_t N,
                                         void* stream) {
  FH_CHECK_PTR(parts);
  FH_CHECK_PTR(row_max);
  FH_CHECK_PTR(row_sumexp);
  FH_CHECK_PTR(tgt_logit);
  FH_CHECK_POS(W);
  FH_CHECK_POS(N);
  FH_CHECK_I32(W);
  hipLaunchKernelGGL(disc_merge_kernel, dim3((unsigned)fh_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, parts, row_max, row_sumexp,
                     tgt_logit, (int)W, N);
  return fh_launch_status();
}

extern "C" int fhvae_disc_lse_bwd(const float* q, const float* table, const int64_t* idx, int64_t row0, float inv_two_var,
                                  const float* row_max, const float* row_sumexp, const float* g_scale, float g_mul,
                                  float* dq, float* dtable, void* ws, int64_t ws_bytes, int64_t B, int64_t S, int64_t D, int dtype,
                                  void* stream) {
  if (dtype != FHVAE_F32 && dtype != FHVAE_BF16) return FHVAE_ERR_DTYPE;
  FH_CHECK_PTR(q);
  FH_CHECK_PTR(table);
  FH_CHECK_PTR(idx);
  FH_CHECK_PTR(row_max);
  FH_CHECK_PTR(row_sumexp);
  FH_CHECK_PTR(g_scale);
  FH_CHECK_POS(B);
  FH_CHECK_POS(S);
  FH_CHECK_I32(B);
  FH_CHECK_I32(S);
  hipStream_t st = (hipStream_t)stream;
  const DiscEngine engine = disc_engine(B, S, D, dtype);
  if (engine != kDiscValu) {
    if (ws && (((uintptr_t)ws) & 15)) return FHVAE_ERR_ALIGN;
    int e = disc_mfma_bwd(engine, q, table, idx, row0, inv_two_var, row_max, row_sumexp, g_scale, g_mul, dq, dtable, (float*)ws,
                          ws ? ws_bytes : 0, B, S, D, st);
    if (e) return e;
    if (dq || dtable) {
      DISC_DISPATCH(D, hipLaunchKernelGGL((disc_own_bwd_kernel<DD>), dim3((unsigned)fh_cdiv(B * (DD / 4), 256)), dim3(256), 0, st, q,
                                          table, idx, row0, inv_two_var, row_max, row_sumexp, g_scale, g_mul, dq, dtable, (int)B,
                                          (int)S));
      e = fh_launch_status();
    }
    return e;
  }
  if (dq) {
    hipError_t he = hipMemsetAsync(dq, 0, (size_t)(B * D) * sizeof(float), st);
    if (he != hipSuccess) return (int)he;
    DiscPlan p = disc_plan(B, S);
    dim3 grid((unsigned)p.btiles, (unsigned)p.nchunks);
    DISC_DISPATCH(D, hipLaunchKernelGGL((disc_bwd_dq_kernel<DD>), grid, dim3(256), 0, st, q, table, idx, row0, inv_two_var,
                                        row_max, row_sumexp, g_scale, g_mul, dq, (int)B, (int)S, p.chunk));
    int e = fh_launch_status();
    if (e) return e;
  }
  if (dtable) {
    DiscPlan p = disc_plan(S, B);  // roles swapped: threads = rows, chunks over queries
    dim3 grid((unsigned)p.btiles, (unsigned)p.nchunks);
    DISC_DISPATCH(D, hipLaunchKernelGGL((disc_bwd_dt_kernel<DD>), grid, dim3(256), 0, st, q, table, idx, row0, inv_two_var,
                                        row_max, row_sumexp, g_scale, g_mul, dtable, (int)B, (int)S, p.chunk));
    int e = fh_launch_status();
    if (e) return e;
  }
  return FHVAE_OK;
}
