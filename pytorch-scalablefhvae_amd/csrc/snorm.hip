// snorm.hip -- the cohort statistics of score normalisation (include/fhvae_snorm.h): per evaluation row the K-th largest cohort
// score, and the mean and standard deviation of the K largest, in ONE launch with no (S x Nc) temporary.  (The normalised score
// of a pair is an epilogue of spk.hip's all-pairs kernel.)
//
// A workgroup keeps 256 stationary evaluation rows (allpairs_f32.h) and streams the WHOLE cohort seven times:
//   passes 0 .. 5   a radix select on the order-preserving 32-bit key of the score, 6 + 6 + 6 + 6 + 6 + 2 bits from the top.  A
//                   score whose bits above the digit equal its row's prefix counts into the row's 64-bin LDS histogram
//                   (ds_add_u32); after the pass one thread per row walks its bins from the top, takes the bin the rank falls
//                   in as the next digit and lowers the rank by the counts above it.  After pass 5 the prefix is the key of T_i.
//   pass 6          d = s - T_i of every score above T_i, summed with d * d per lane in float64 in increasing cohort row; the
//                   four lanes of a row merge through LDS as (g0 + g1) + (g2 + g3), one thread per row finishes.
// Counts are integers and the order of the sums is fixed by the cohort row alone (lane group g = (n mod 16) / 4): a row's result
// has the same bits wherever the row stands.  The score of a pass is recomputed, not kept: the same instructions on the same
// operands give the same bits in every pass.
// Built with -ffp-contract=off and correctly rounded f32 division (r = 1 / sd).
#include <cmath>

#include "allpairs_f32.h"

#include "../../include/fhvae_snorm.h"

namespace fh {

namespace {

constexpr int kSnYT = ap::kYT;
constexpr int kSnBins = 64;

// (spk.hip's key) f32 -> a 32-bit key whose unsigned order is the order of the floats, -0 below +0; and back
__device__ __forceinline__ unsigned sn_key(float f) {
  const unsigned b = __builtin_bit_cast(unsigned, f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sn_unkey(unsigned k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct SnArgs {
  const float* v;   // (S, D), leading dimension ld
  const float* a;   // (S)
  const float* z;   // (Nc, D), leading dimension ldz
  const float* az;  // (Nc)
  float *mu, *sd, *r, *thr;
  int32_t* status;
  int64_t ld, ldz;
  float c, sd_floor;
  int S, Nc, K;
};

// the row's bin b stands at another bank in every row (16 rows of a wave count at once, often into the same bin)
__device__ __forceinline__ int sn_bin(int row, int b) { return row * kSnBins + ((b + row) & (kSnBins - 1)); }

// LDS: the streamed tile, az of its rows, the histograms (pass 6: the lanes' sums), prefix, rank and the non-finite flag per row
template <int D>
constexpr int sn_smem() {
  return kSnYT * D * 4 + kSnYT * 4 + 256 * kSnBins * 4 + 3 * 256 * 4;
}

template <int D>
__global__ __launch_bounds__(256, 1) void sn_cohort_kernel(SnArgs a) {
  constexpr int YT = kSnYT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ytile = smem;                           // [YT][D] f32, swizzled
  float* yaz = (float*)(smem + YT * D * 4);     // [YT]
  unsigned* hist = (unsigned*)(yaz + YT);       // [256][64]
  unsigned* prefix = hist + 256 * kSnBins;      // [256] the key's bits found so far, in place
  unsigned* rank = prefix + 256;                // [256] the rank looked for among the scores that share the prefix, from 1
  int* bad = (int*)(rank + 256);                // [256]
  static_assert(256 * kSnBins * 4 >= 256 * 4 * 2 * 8, "the lanes' float64 sums reuse the histograms");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int xb0 = blockIdx.x * 256;
  const int x0 = xb0 + wave * 64;
  const float c = a.c;

  for (int e = tid; e < 256 * kSnBins; e += 256) hist[e] = 0u;
  prefix[tid] = 0u;
  rank[tid] = (unsigned)a.K;
  bad[tid] = 0;
  __syncthreads();

  uint4 xf[4][D / 16];
  ap::load_stationary<D>(a.v, a.ld, a.S, x0, xf);
  float xa[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = x0 + t * 16 + i;
    xa[t] = x < a.S ? a.a[x] : 0.f;
  }
  auto side = [&](int y0) {
    if (tid < YT) yaz[tid] = y0 + tid < a.Nc ? a.az[y0 + tid] : 0.f;
  };

  // ---- the radix select
#pragma unroll 1
  for (int pass = 0; pass < 6; ++pass) {
    const int shift = pass < 5 ? 26 - 6 * pass : 0;
    const unsigned digit = pass < 5 ? 63u : 3u;
    const unsigned above = pass == 0 ? 0u : ~0u << (shift + (pass < 5 ? 6 : 2));  // the bits found so far
    unsigned pre[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) pre[t] = prefix[wave * 64 + t * 16 + i];
    ap::stream<D>(a.z, a.ldz, 0, a.Nc, ytile, xf, side, ap::EveryBlock(), [&](int y0, int yb, const f32x4(&acc)[4]) {
      const float4 yav = *(const float4*)(yaz + yb * 16 + 4 * g);
      const float yar[4] = {yav.x, yav.y, yav.z, yav.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row = wave * 64 + t * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = (acc[t][r] + (xa[t] + yar[r])) + c;
          const unsigned key = sn_key(s);
          if (y0 + yb * 16 + 4 * g + r < a.Nc && ((key ^ pre[t]) & above) == 0u) atomicAdd(&hist[sn_bin(row, (int)((key >> shift) & digit))], 1u);
        }
      }
    });
    // (stream() ends on a barrier) one thread per row: the bin the rank falls in
    {
      unsigned want = rank[tid], seen = 0u;
      int b = (int)digit;
      for (; b > 0; --b) {
        const unsigned n = hist[sn_bin(tid, b)];
        if (seen + n >= want) break;
        seen += n;
      }
      rank[tid] = want - seen;
      prefix[tid] |= (unsigned)b << shift;
      for (int e = 0; e < kSnBins; ++e) hist[tid * kSnBins + e] = 0u;
    }
    __syncthreads();
  }

  // ---- the sums above the threshold
  unsigned tkey[4];
  double tv[4], s1[4], s2[4];
  bool nonfinite[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    tkey[t] = prefix[wave * 64 + t * 16 + i];
    tv[t] = (double)sn_unkey(tkey[t]);
    s1[t] = s2[t] = 0.0;
    nonfinite[t] = false;
  }
  ap::stream<D>(a.z, a.ldz, 0, a.Nc, ytile, xf, side, ap::EveryBlock(), [&](int y0, int yb, const f32x4(&acc)[4]) {
    const float4 yav = *(const float4*)(yaz + yb * 16 + 4 * g);
    const float yar[4] = {yav.x, yav.y, yav.z, yav.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = (acc[t][r] + (xa[t] + yar[r])) + c;
        if (y0 + yb * 16 + 4 * g + r < a.Nc) {
          if (!(fabsf(s) < INFINITY)) nonfinite[t] = true;
          if (sn_key(s) > tkey[t]) {
            const double d = (double)s - tv[t];
            s1[t] += d;
            s2[t] += d * d;
          }
        }
      }
    }
  });
  // (stream() ended on a barrier: the histograms are free) [row][g][S1, S2]
  double* sums = (double*)hist;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int row = wave * 64 + t * 16 + i;
    sums[(row * 4 + g) * 2] = s1[t];
    sums[(row * 4 + g) * 2 + 1] = s2[t];
    if (nonfinite[t]) atomicOr(&bad[row], 1);
  }
  __syncthreads();
  const int x = xb0 + tid;
  if (x >= a.S) return;
  const double* q = sums + tid * 8;
  const double S1 = (q[0] + q[2]) + (q[4] + q[6]);
  const double S2 = (q[1] + q[3]) + (q[5] + q[7]);
  const double K = (double)a.K;
  const float T = sn_unkey(prefix[tid]);
  const double m = S1 / K;
  const double mu64 = (double)T + m;
  double var64 = S2 / K - m * m;
  var64 = var64 > 0.0 ? var64 : 0.0;
  float thr = T, mu = (float)mu64, sd = fmaxf((float)sqrt(var64), a.sd_floor);
  float r = 1.0f / sd;
  if (bad[tid]) {
    thr = mu = sd = r = NAN;
    atomicOr(a.status, (int32_t)FHVAE_SN_NONFINITE);
  }
  a.thr[x] = thr;
  a.mu[x] = mu;
  a.sd[x] = sd;
  a.r[x] = r;
}

template <int D>
int sn_launch(const SnArgs& a, hipStream_t st) {
  constexpr int smem = sn_smem<D>();
  hipError_t e = hipFuncSetAttribute((const void*)sn_cohort_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((sn_cohort_kernel<D>), dim3((unsigned)fh_cdiv(a.S, 256)), dim3(256), (size_t)smem, st, a);
  return fh_launch_status();
}

}  // namespace

}  // namespace fh

extern "C" int fhvae_sn_cohort_stats(const float* v, int64_t ld, const float* a, int64_t S, const float* z, int64_t ldz, const float* az,
                                     int64_t Nc, int64_t D, float c, int64_t top, float sd_floor, float* mu, float* sd, float* r, float* thr,
                                     int32_t* status, void* stream) {
  using namespace fh;
  FH_CHECK_PTR(v);
  FH_CHECK_PTR(a);
  FH_CHECK_PTR(z);
  FH_CHECK_PTR(az);
  FH_CHECK_PTR(mu);
  FH_CHECK_PTR(sd);
  FH_CHECK_PTR(r);
  FH_CHECK_PTR(thr);
  FH_CHECK_PTR(status);
  FH_CHECK_POS(S);
  FH_CHECK_POS(Nc);
  int rc = fh_allpairs_check(v, ld, D);
  if (rc != FHVAE_OK) return rc;
  rc = fh_allpairs_check(z, ldz, D);
  if (rc != FHVAE_OK) return rc;
  if (!(sd_floor > 0.f) || !std::isfinite(sd_floor)) return FHVAE_ERR_SHAPE;
  if ((((uintptr_t)a | (uintptr_t)az | (uintptr_t)mu | (uintptr_t)sd | (uintptr_t)r | (uintptr_t)thr | (uintptr_t)status) & 3) != 0)
    return FHVAE_ERR_ALIGN;
  if (S > (int64_t)FHVAE_SN_MAX_ROWS || Nc > (int64_t)FHVAE_SN_MAX_COHORT) return FHVAE_ERR_LIMIT;
  SnArgs g = {};
  g.v = v;
  g.a = a;
  g.z = z;
  g.az = az;
  g.mu = mu;
  g.sd = sd;
  g.r = r;
  g.thr = thr;
  g.status = status;
  g.ld = ld;
  g.ldz = ldz;
  g.c = c;
  g.sd_floor = sd_floor;
  g.S = (int)S;
  g.Nc = (int)Nc;
  g.K = (int)((top <= 0 || top > Nc) ? Nc : top);
  return fh_allpairs_dispatch(D, [&](auto d) { return sn_launch<decltype(d)::value>(g, (hipStream_t)stream); });
}
