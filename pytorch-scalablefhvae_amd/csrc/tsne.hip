// tsne.hip -- exact t-SNE of N embeddings with no (N x N) array: the perplexity search and the gradient both recompute
// every squared distance, and the gradient recomputes every p_ij, inside a streaming all-pairs pass.
//
//   d2(i, j) = max(n_i + n_j - 2 x_i . x_j, 0)                 n_i = sum_d x_id^2 (tsne_norm_kernel), j != i everywhere
//   m_i = min_j d2(i, j)    e_ij = exp(-beta_i (d2(i, j) - m_i))    Z_i = sum_j e_ij    p_j|i = e_ij / Z_i
//   beta_i: bisection on log2 beta over [kTsneLo, kTsneHi], kTsneSteps steps, no exit that depends on the data: a step
//     moves the lower end up where log Z_i + beta_i sum_j e_ij (d2 - m_i) / Z_i > log(perplexity); beta_i = 2^(middle of
//     the last interval), and Z_i is summed at that beta_i.
//   p_ij = (p_j|i + p_i|j) / (2 N)    w_ij = 1 / (1 + |y_i - y_j|^2)
//   F_i = a sum_j p_ij w_ij (y_i - y_j)    R_i = sum_j w_ij^2 (y_i - y_j)    W_i = sum_j w_ij    Zq = sum_i W_i
//   grad_i = 4 (F_i - R_i / Zq)    KL = sum_{i != j} p_ij log(p_ij Zq / w_ij)   (a = 1; a term with p_ij < 1e-30 is 0)
//   update (scikit-learn's _gradient_descent): inc = V grad < 0; G = inc ? G + 0.2 : 0.8 G; G = max(G, 0.01);
//     V = momentum V - lr G grad; Y += V.
//
// The contraction is allpairs_f32.h's pass over the full N x N: a stationary row sums over every j != i, nothing is scattered to
// the streamed side.
//
//   tsne_affinity_kernel: one workgroup per stationary block, every pass (1 for m, kTsneSteps of the bisection, 1 for Z)
//     inside the launch; a wave owns its 64 rows over all j, so a pass ends in the wave's registers.
//   tsne_grad_kernel: the j range is split into chunks (grid.y); a workgroup writes per-row partials of F, R, W and the two
//     KL pieces  A_i = sum_j p_ij log(p_ij N^2 / w_ij),  B_i = sum_j p_ij  to the workspace, and the sums of W, A, B over
//     its rows.
//   tsne_update_kernel: every workgroup adds the workgroup sums in index order in double (Zq, KL = A + (log Zq - log N^2) B),
//     then adds its rows' chunks in index order and does the update.
// No floating-point atomic anywhere: two calls give equal bits.
//
// Symmetry, bit for bit: the dot is symmetric (allpairs_f32.h, THE ORDER), the norms come from one kernel and enter as the
// commutative sum n_i + n_j, and the same expression fma(-2, dot, n_i + n_j) is used by all three kernels: d2(i, j) ==
// d2(j, i), and d2(i, j) - m_i >= 0 holds exactly in every later pass.  The norm's fma chain runs in the MFMA chain's k
// order, so two equal rows are at distance exactly 0.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "allpairs_f32.h"

namespace fh {

namespace {

constexpr int kTsneYT = ap::kYT;
constexpr int kTsneMinChunk = 512;       // streamed rows per workgroup of the gradient pass, at least
constexpr int kTsneWorkgroups = 2048;    // workgroups the gradient pass aims at
constexpr float kTsneLo = -60.f, kTsneHi = 60.f;  // the interval of log2 beta
constexpr int kTsneSteps = 48;           // bisection steps (an f32 middle stops moving after about 30)
constexpr int kTsneParts = 7;            // per-row partials of a chunk: Fx, Fy, Rx, Ry, W, A, B
constexpr int64_t kTsneMaxN = (int64_t)1 << 22;
constexpr float kLog2e = 1.44269504088896340736f;

// n[s] = sum_d x[s][d]^2: one thread per row, one fma chain in the k order of the MFMA chain (16 jj + 4 g + c: c inside g
// inside jj is the order in which allpairs_f32.h's chain meets the columns)
__global__ void tsne_norm_kernel(const float* __restrict__ x, int64_t ld, int N, int D, float* __restrict__ nrm) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= N) return;
  const float* p = x + (int64_t)s * ld;
  float ss = 0.f;
  for (int d = 0; d < D; d += 16) {
    float q[4][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 v = *(const float4*)(p + d + 4 * g);
      q[g][0] = v.x, q[g][1] = v.y, q[g][2] = v.z, q[g][3] = v.w;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g = 0; g < 4; ++g) ss = __builtin_fmaf(q[g][c], q[g][c], ss);
  }
  nrm[s] = ss;
}

__device__ __forceinline__ float ts_d2(float dot, float nx, float ny) { return fmaxf(__builtin_fmaf(-2.f, dot, nx + ny), 0.f); }

struct TsneAffArgs {
  const float* x;    // (N, D), leading dimension ld
  const float* nrm;  // (N)
  float *beta, *m, *z;
  int64_t ld;
  int N;
  float log_perp;
};

// (the stationary fragments take D registers, the bisection's state 30 more: above D = 80 two workgroups per CU would spill)
template <int D>
__global__ __launch_bounds__(256, D > 80 ? 1 : 2) void tsne_affinity_kernel(TsneAffArgs a) {
  constexpr int YT = kTsneYT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                       // [YT][D] f32, swizzled
  float* yn = (float*)(smem + YT * D * 4);  // [YT]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int x0 = blockIdx.x * 256 + wave * 64;
  const int N = a.N;

  uint4 xf[4][D / 16];
  ap::load_stationary<D>(a.x, a.ld, N, x0, xf);
  float xn[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) xn[t] = (x0 + t * 16 + i < N) ? a.nrm[x0 + t * 16 + i] : 0.f;

  auto side = [&](int y0) {
    if (tid < YT) yn[tid] = (y0 + tid < N) ? a.nrm[y0 + tid] : 0.f;
  };

  // ---- m = the smallest distance to another row
  float mn[4] = {FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX};
  ap::stream<D>(a.x, a.ld, 0, N, ytile, xf, side, ap::EveryBlock(), [&](int y0, int yb, const f32x4(&acc)[4]) {
    const float4 ynv = *(const float4*)(yn + yb * 16 + 4 * g);
    const float ynr[4] = {ynv.x, ynv.y, ynv.z, ynv.w};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int y = y0 + yb * 16 + 4 * g + r;
        const float d2 = ts_d2(acc[t][r], xn[t], ynr[r]);
        mn[t] = (y < N && y != x0 + t * 16 + i) ? fminf(mn[t], d2) : mn[t];
      }
  });
#pragma unroll
  for (int t = 0; t < 4; ++t) mn[t] = ap::quad_min(mn[t]);

  // ---- the bisection; the pass after its last step sums Z at the final beta
  float lo[4], hi[4], mid[4], s0[4], s1[4], nbl[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) lo[t] = kTsneLo, hi[t] = kTsneHi;
#pragma unroll 1
  for (int step = 0; step <= kTsneSteps; ++step) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      mid[t] = 0.5f * (lo[t] + hi[t]);
      nbl[t] = -(exp2f(mid[t]) * kLog2e);  // exp(-beta u) = 2^(nbl u)
      s0[t] = 0.f, s1[t] = 0.f;
    }
    ap::stream<D>(a.x, a.ld, 0, N, ytile, xf, side, ap::EveryBlock(), [&](int y0, int yb, const f32x4(&acc)[4]) {
      const float4 ynv = *(const float4*)(yn + yb * 16 + 4 * g);
      const float ynr[4] = {ynv.x, ynv.y, ynv.z, ynv.w};
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int y = y0 + yb * 16 + 4 * g + r;
          const float u = ts_d2(acc[t][r], xn[t], ynr[r]) - mn[t];
          const float e = (y < N && y != x0 + t * 16 + i) ? __builtin_amdgcn_exp2f(nbl[t] * u) : 0.f;
          s0[t] += e;
          s1[t] = __builtin_fmaf(e, u, s1[t]);
        }
    });
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s0[t] = ap::quad_sum(s0[t]);
      s1[t] = ap::quad_sum(s1[t]);
      if (step < kTsneSteps) {  // (s0 >= 1: the nearest row's term is exactly 1)
        const float h = logf(s0[t]) + exp2f(mid[t]) * s1[t] / s0[t];
        const bool up = h > a.log_perp;
        lo[t] = up ? mid[t] : lo[t];
        hi[t] = up ? hi[t] : mid[t];
      }
    }
  }
  if (g == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = x0 + t * 16 + i;
      if (r < N) {
        a.beta[r] = exp2f(mid[t]);
        a.m[r] = mn[t];
        a.z[r] = s0[t];
      }
    }
  }
}

struct TsneGradArgs {
  const float* x;                // (N, D), leading dimension ld
  const float *nrm, *beta, *m, *z;  // (N)
  const float* y;                // (N, 2)
  float* part;                   // [nchunks][kTsneParts][npad]
  float* wg;                     // [nchunks][nxb][4]: W, A, B over the workgroup's rows
  int64_t ld;
  int N, npad, chunk, kl;
  float inv2n, nn;               // 1 / (2 N), N^2
};

// (D registers of stationary fragments, 52 of the rows' state and sums, 24 of the streamed rows' values: above D = 48 two
// workgroups per CU would spill)
template <int D>
__global__ __launch_bounds__(256, D > 48 ? 1 : 2) void tsne_grad_kernel(TsneGradArgs a) {
  constexpr int YT = kTsneYT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                       // [YT][D] f32, swizzled
  float* sy = (float*)(smem + YT * D * 4);  // [6][YT]: n, -beta log2(e), m, 1 / Z, y0, y1
  float* red = sy + 6 * YT;                 // [4 waves][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int x0 = blockIdx.x * 256 + wave * 64;
  const int N = a.N;
  const int y_begin = blockIdx.y * a.chunk, y_end = min(N, y_begin + a.chunk);  // (the host's grid leaves no empty chunk)

  uint4 xf[4][D / 16];
  ap::load_stationary<D>(a.x, a.ld, N, x0, xf);
  float xn[4], xb[4], xm[4], xz[4], xy0[4], xy1[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int r = x0 + t * 16 + i;
    const bool ok = r < N;
    xn[t] = ok ? a.nrm[r] : 0.f;
    xb[t] = ok ? -(a.beta[r] * kLog2e) : 0.f;
    xm[t] = ok ? a.m[r] : 0.f;
    xz[t] = ok ? 1.f / a.z[r] : 0.f;
    xy0[t] = ok ? a.y[2 * (int64_t)r] : 0.f;
    xy1[t] = ok ? a.y[2 * (int64_t)r + 1] : 0.f;
  }
  float f0[4], f1[4], r0[4], r1[4], ws[4], ka[4], kb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) f0[t] = f1[t] = r0[t] = r1[t] = ws[t] = ka[t] = kb[t] = 0.f;

  auto side = [&](int y0) {
    if (tid < YT) {
      const int y = y0 + tid;
      const bool ok = y < y_end;
      sy[tid] = ok ? a.nrm[y] : 0.f;
      sy[YT + tid] = ok ? -(a.beta[y] * kLog2e) : 0.f;
      sy[2 * YT + tid] = ok ? a.m[y] : 0.f;
      sy[3 * YT + tid] = ok ? 1.f / a.z[y] : 0.f;
    } else if (tid < 2 * YT) {
      const int y = y0 + tid - YT;
      const float2 v = (y < y_end) ? *(const float2*)(a.y + 2 * (int64_t)y) : make_float2(0.f, 0.f);
      sy[4 * YT + tid - YT] = v.x;
      sy[5 * YT + tid - YT] = v.y;
    }
  };
  ap::stream<D>(a.x, a.ld, y_begin, y_end, ytile, xf, side, ap::EveryBlock(), [&](int y0, int yb, const f32x4(&acc)[4]) {
    float sv[6][4];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const float4 v = *(const float4*)(sy + k * YT + yb * 16 + 4 * g);
      sv[k][0] = v.x, sv[k][1] = v.y, sv[k][2] = v.z, sv[k][3] = v.w;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int y = y0 + yb * 16 + 4 * g + r;
        const bool ok = y < y_end && y != x0 + t * 16 + i;
        const float d2 = ts_d2(acc[t][r], xn[t], sv[0][r]);
        const float pji = __builtin_amdgcn_exp2f(xb[t] * (d2 - xm[t])) * xz[t];
        const float pij = __builtin_amdgcn_exp2f(sv[1][r] * (d2 - sv[2][r])) * sv[3][r];
        const float p = ok ? (pji + pij) * a.inv2n : 0.f;
        const float dy0 = xy0[t] - sv[4][r], dy1 = xy1[t] - sv[5][r];
        const float q = __builtin_fmaf(dy1, dy1, __builtin_fmaf(dy0, dy0, 1.f));  // 1 / w
        const float w = ok ? __builtin_amdgcn_rcpf(q) : 0.f;
        const float pw = p * w, ww = w * w;
        f0[t] = __builtin_fmaf(pw, dy0, f0[t]);
        f1[t] = __builtin_fmaf(pw, dy1, f1[t]);
        r0[t] = __builtin_fmaf(ww, dy0, r0[t]);
        r1[t] = __builtin_fmaf(ww, dy1, r1[t]);
        ws[t] += w;
        if (a.kl) {  // (uniform)
          // p N^2 / w: of order 1 where it counts, so the two KL pieces stay small against the sum they cancel to
          const float term = (p > 1e-30f) ? p * __logf(p * a.nn * q) : 0.f;
          ka[t] += term;
          kb[t] += p;
        }
      }
  });

  // ---- the rows' partials of this chunk, and their sums over the workgroup's rows
  float tot[3] = {0.f, 0.f, 0.f};
  float* part = a.part + (int64_t)blockIdx.y * kTsneParts * a.npad;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float v[kTsneParts] = {ap::quad_sum(f0[t]), ap::quad_sum(f1[t]), ap::quad_sum(r0[t]), ap::quad_sum(r1[t]),
                                 ap::quad_sum(ws[t]), ap::quad_sum(ka[t]), ap::quad_sum(kb[t])};
    const int r = x0 + t * 16 + i;
    if (g == 0 && r < N) {
#pragma unroll
      for (int k = 0; k < kTsneParts; ++k) part[(int64_t)k * a.npad + r] = v[k];
      tot[0] += v[4], tot[1] += v[5], tot[2] += v[6];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) tot[k] = wave_sum(tot[k]);
  if (lane == 0) red[wave * 4 + 0] = tot[0], red[wave * 4 + 1] = tot[1], red[wave * 4 + 2] = tot[2];
  __syncthreads();
  if (tid < 3) {
    const float v = ((red[tid] + red[4 + tid]) + red[8 + tid]) + red[12 + tid];
    a.wg[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + tid] = v;
  }
}

struct TsneUpdArgs {
  const float* part;  // [nchunks][kTsneParts][npad]
  const float* wg;    // [nwg][4]
  float *y, *v, *g;   // (N, 2); v and g NULL: no update
  float* out;         // (N, 7) or NULL: F (with the exaggeration), R, W, grad
  float* scal;        // (2) or NULL: Zq, KL
  float* kl;          // (1) or NULL
  int N, npad, nchunks, nwg;
  float exaggeration, momentum, lr, nn;
};

__global__ __launch_bounds__(256) void tsne_update_kernel(TsneUpdArgs a) {
  __shared__ double red[3][256];
  const int tid = threadIdx.x;
  // ---- Zq and the KL pieces: every workgroup adds the same numbers in the same order
  double s[3] = {0.0, 0.0, 0.0};
  for (int e = tid; e < a.nwg; e += 256) {
    s[0] += (double)a.wg[4 * (int64_t)e];
    s[1] += (double)a.wg[4 * (int64_t)e + 1];
    s[2] += (double)a.wg[4 * (int64_t)e + 2];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) red[k][tid] = s[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + o];
    }
    __syncthreads();
  }
  const double zq = red[0][0];
  if (blockIdx.x == 0 && tid == 0) {
    const double klv = red[1][0] + (log(zq) - log((double)a.nn)) * red[2][0];
    if (a.kl) a.kl[0] = (float)klv;
    if (a.scal) a.scal[0] = (float)zq, a.scal[1] = (float)klv;
  }
  const int r = blockIdx.x * 256 + tid;
  if (r >= a.N) return;
  float p[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    float acc = 0.f;
    for (int c = 0; c < a.nchunks; ++c) acc += a.part[((int64_t)c * kTsneParts + k) * a.npad + r];
    p[k] = acc;
  }
  const float izq = (float)(1.0 / zq);
  const float fx = a.exaggeration * p[0], fy = a.exaggeration * p[1];
  const float gr[2] = {4.f * (fx - p[2] * izq), 4.f * (fy - p[3] * izq)};
  if (a.out) {
    float* o = a.out + 7 * (int64_t)r;
    o[0] = fx, o[1] = fy, o[2] = p[2], o[3] = p[3], o[4] = p[4], o[5] = gr[0], o[6] = gr[1];
  }
  if (a.v) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int64_t e = 2 * (int64_t)r + k;
      const float vel = a.v[e];
      float gain = a.g[e];
      gain = (vel * gr[k] < 0.f) ? gain + 0.2f : gain * 0.8f;
      gain = fmaxf(gain, 0.01f);
      const float nv = a.momentum * vel - a.lr * gain * gr[k];
      a.g[e] = gain;
      a.v[e] = nv;
      a.y[e] += nv;
    }
  }
}

struct TsnePlan {
  int64_t nxb, chunk, nchunks, npad;
  int64_t part_off, wg_off, floats;  // in floats from the workspace's start (the norms sit at 0)
};

TsnePlan tsne_plan(int64_t N) {
  TsnePlan p;
  p.nxb = fh_cdiv(N, 256);
  p.chunk = fh_allpairs_chunk(N, std::max<int64_t>(1, kTsneWorkgroups / p.nxb), kTsneMinChunk);
  p.nchunks = fh_cdiv(N, p.chunk);
  p.npad = fh_cdiv(N, 64) * 64;
  p.part_off = p.npad;
  p.wg_off = p.part_off + p.nchunks * kTsneParts * p.npad;
  p.floats = p.wg_off + p.nchunks * p.nxb * 4;
  return p;
}

int tsne_check(const float* x, int64_t ld, int64_t N, int64_t D, const void* ws, int64_t ws_bytes) {
  if (N < 8) return FHVAE_ERR_SHAPE;
  const int rc = fh_allpairs_check(x, ld, D);
  if (rc != FHVAE_OK) return rc;
  if (((uintptr_t)ws & 15) != 0) return FHVAE_ERR_ALIGN;
  if (N > kTsneMaxN) return FHVAE_ERR_LIMIT;
  if (ws_bytes < fhvae_tsne_ws_bytes(N, D)) return FHVAE_ERR_SHAPE;
  return FHVAE_OK;
}

int tsne_norms(const float* x, int64_t ld, int64_t N, int64_t D, float* nrm, hipStream_t st) {
  hipLaunchKernelGGL(tsne_norm_kernel, dim3((unsigned)fh_cdiv(N, 256)), dim3(256), 0, st, x, ld, (int)N, (int)D, nrm);
  return fh_launch_status();
}

int tsne_aff_launch(int64_t D, const TsneAffArgs& a, dim3 grid, hipStream_t st) {
  return fh_allpairs_dispatch(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    hipLaunchKernelGGL(tsne_affinity_kernel<DD>, grid, dim3(256), (size_t)(kTsneYT * DD * 4 + kTsneYT * 4), st, a);
    return fh_launch_status();
  });
}

int tsne_grad_launch(int64_t D, const TsneGradArgs& a, dim3 grid, hipStream_t st) {
  return fh_allpairs_dispatch(D, [&](auto d) {
    constexpr int DD = decltype(d)::value;
    hipLaunchKernelGGL(tsne_grad_kernel<DD>, grid, dim3(256), (size_t)(kTsneYT * DD * 4 + 6 * kTsneYT * 4 + 16 * 4), st, a);
    return fh_launch_status();
  });
}

// the norms, the gradient pass and the reduction / update: what fhvae_tsne_step and fhvae_tsne_grad share
int tsne_pass(const float* x, int64_t ld, int64_t N, int64_t D, const float* beta, const float* m, const float* z, float* y, float* v,
              float* g, float exaggeration, float momentum, float lr, int want_kl, float* kl, float* out, float* scal, void* ws,
              hipStream_t st) {
  const TsnePlan p = tsne_plan(N);
  float* base = (float*)ws;
  int rc = tsne_norms(x, ld, N, D, base, st);
  if (rc != FHVAE_OK) return rc;
  TsneGradArgs a = {};
  a.x = x, a.nrm = base, a.beta = beta, a.m = m, a.z = z, a.y = y;
  a.part = base + p.part_off, a.wg = base + p.wg_off;
  a.ld = ld, a.N = (int)N, a.npad = (int)p.npad, a.chunk = (int)p.chunk, a.kl = want_kl;
  a.inv2n = (float)(0.5 / (double)N);
  a.nn = (float)((double)N * (double)N);
  rc = tsne_grad_launch(D, a, dim3((unsigned)p.nxb, (unsigned)p.nchunks), st);
  if (rc != FHVAE_OK) return rc;
  TsneUpdArgs u = {};
  u.part = a.part, u.wg = a.wg, u.y = y, u.v = v, u.g = g, u.out = out, u.scal = scal, u.kl = kl;
  u.N = (int)N, u.npad = (int)p.npad, u.nchunks = (int)p.nchunks, u.nwg = (int)(p.nchunks * p.nxb);
  u.exaggeration = exaggeration, u.momentum = momentum, u.lr = lr, u.nn = a.nn;
  hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)p.nxb), dim3(256), 0, st, u);
  return fh_launch_status();
}

}  // namespace

}  // namespace fh

extern "C" int64_t fhvae_tsne_ws_bytes(int64_t N, int64_t D) {
  if (N < 1 || N > fh::kTsneMaxN || D < 1) return 0;
  return fh_cdiv(fh::tsne_plan(N).floats * (int64_t)sizeof(float), 256) * 256;
}

extern "C" int fhvae_tsne_affinity(const float* x, int64_t ld, int64_t N, int64_t D, float perplexity, float* beta, float* m, float* z,
                                   void* ws, int64_t ws_bytes, void* stream) {
  using namespace fh;
  FH_CHECK_PTR(x);
  FH_CHECK_PTR(beta);
  FH_CHECK_PTR(m);
  FH_CHECK_PTR(z);
  FH_CHECK_PTR(ws);
  int rc = tsne_check(x, ld, N, D, ws, ws_bytes);
  if (rc != FHVAE_OK) return rc;
  if (!(perplexity >= 1.f) || !((double)perplexity <= (double)(N - 1) / 3.0)) return FHVAE_ERR_SHAPE;
  if ((((uintptr_t)beta | (uintptr_t)m | (uintptr_t)z) & 3) != 0) return FHVAE_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  rc = tsne_norms(x, ld, N, D, (float*)ws, st);
  if (rc != FHVAE_OK) return rc;
  TsneAffArgs a = {};
  a.x = x, a.nrm = (const float*)ws, a.beta = beta, a.m = m, a.z = z;
  a.ld = ld, a.N = (int)N, a.log_perp = (float)std::log((double)perplexity);
  return tsne_aff_launch(D, a, dim3((unsigned)fh_cdiv(N, 256)), st);
}

extern "C" int fhvae_tsne_step(const float* x, int64_t ld, int64_t N, int64_t D, const float* beta, const float* m, const float* z, float* y,
                               float* v, float* g, float exaggeration, float momentum, float lr, float* kl, void* ws, int64_t ws_bytes,
                               void* stream) {
  using namespace fh;
  FH_CHECK_PTR(x);
  FH_CHECK_PTR(beta);
  FH_CHECK_PTR(m);
  FH_CHECK_PTR(z);
  FH_CHECK_PTR(y);
  FH_CHECK_PTR(v);
  FH_CHECK_PTR(g);
  FH_CHECK_PTR(ws);
  int rc = tsne_check(x, ld, N, D, ws, ws_bytes);
  if (rc != FHVAE_OK) return rc;
  if ((((uintptr_t)beta | (uintptr_t)m | (uintptr_t)z | (uintptr_t)v | (uintptr_t)g | (uintptr_t)kl) & 3) != 0 || ((uintptr_t)y & 7) != 0)
    return FHVAE_ERR_ALIGN;
  return tsne_pass(x, ld, N, D, beta, m, z, y, v, g, exaggeration, momentum, lr, kl != nullptr, kl, nullptr, nullptr, ws,
                   (hipStream_t)stream);
}

extern "C" int fhvae_tsne_grad(const float* x, int64_t ld, int64_t N, int64_t D, const float* beta, const float* m, const float* z,
                               const float* y, float exaggeration, float* out, float* scal, void* ws, int64_t ws_bytes, void* stream) {
  using namespace fh;
  FH_CHECK_PTR(x);
  FH_CHECK_PTR(beta);
  FH_CHECK_PTR(m);
  FH_CHECK_PTR(z);
  FH_CHECK_PTR(y);
  FH_CHECK_PTR(out);
  FH_CHECK_PTR(scal);
  FH_CHECK_PTR(ws);
  int rc = tsne_check(x, ld, N, D, ws, ws_bytes);
  if (rc != FHVAE_OK) return rc;
  if ((((uintptr_t)beta | (uintptr_t)m | (uintptr_t)z | (uintptr_t)out | (uintptr_t)scal) & 3) != 0 || ((uintptr_t)y & 7) != 0)
    return FHVAE_ERR_ALIGN;
  return tsne_pass(x, ld, N, D, beta, m, z, (float*)y, nullptr, nullptr, exaggeration, 0.f, 0.f, 1, nullptr, out, scal, ws,
                   (hipStream_t)stream);
}
