// disc_tile.h -- the device code that the two matrix-core K5 kernels share (disc_mfma.hip: exact-f32 MFMA; disc_lp.hip: bf16 MFMA
// with split operands): everything around the products.  Each kernel keeps its own operands (fragments, staging, products, 16-
// against 32-row blocks, the weight image of the one-pass backward); the per-pair arithmetic after the logits, the slot flush and
// the forward epilogue stand here once (the logits with their masks and the backward epilogue: see the notes in disc_lp.hip).  Inline pieces only, as in allpairs_f32.h.  `xq`: the stationary set is the queries (a run-time field in the
// f32 kernel, a template flag in the bf16 one).
//
// Layout both kernels agree on, lane = 16 g + i: a 16 x 16 logit tile comes out of the MFMA with the stationary vector
// x0 + 16 t + i on the lanes and four streamed vectors 4 g + r in the accumulator registers.
//
// The (query, own table row) pairs are NOT computed by these kernels.  The expanded form's absolute error ~1e-7 * 2c (|q|^2 + |t|^2)
// is harmless on far rows (their softmax weight is 0 either way) but it is the whole signal on the pair training drives together
// (q -> table[idx]).  That one logit per query is therefore masked out (logit = -inf: no contribution to the log-sum-exp, zero
// weight in both backward passes) and taken in the DIRECT form -c |q - t|^2 by the callers: the forward's combine kernel merges
// exp(target - max) into the row sum, the backward adds the pair's gradient in disc_own_bwd_kernel (disc.hip).  CE -> log(1 +
// sum_others) and p_target - 1 -> -sum_others then come out cleanly however large the norms are.
#pragma once
#include "disc_mfma.h"

namespace fh {
namespace dt {

// floats of the `red` buffer: the backward epilogue's tr[256][D + 1]; MODE 2, inside the loop: one [64 y][slot_ld] slot per wave
constexpr int red_floats(int D, int mode, int slot_ld) {
  return mode == 0 ? 1 : (mode == 2 && 4 * 64 * slot_ld > 256 * (D + 1) ? 4 * 64 * slot_ld : 256 * (D + 1));
}

// per stationary vector x (ok: x < NX): its target among the streamed rows and, backward, its (max, scale / sum)
template <bool BW>
__device__ __forceinline__ void x_scalars(const DiscMfmaArgs& a, bool xq, int x, bool ok, float gscale, float& xmax, float& xinv, int& xtgt) {
  xmax = 0.f;
  xinv = 0.f;
  xtgt = -1;
  if (xq) {
    if (ok) {
      const int64_t tg = a.idx[x] - a.row0;
      xtgt = (tg >= 0 && tg < a.NY) ? (int)tg : -1;
      if (BW) {
        xmax = a.rmax[x];
        xinv = gscale / a.rsum[x];  // (the upstream scale rides on the normaliser)
      }
    }
  } else {
    xtgt = ok ? x : -2;  // table row index: a streamed query hits it when its target == x
  }
}

// per streamed QUERY y (table rows stationary): its (max, scale / sum, target) into the tile's LDS arrays; returns whether its
// own row is among this workgroup's 256 stationary rows
template <int MODE>
__device__ __forceinline__ bool y_scalars(const DiscMfmaArgs& a, int y, int y_end, float gscale, float& ymax, float& yinv, int& ytgt) {
  const bool ok = y < y_end;
  ymax = ok && MODE == 1 ? a.rmax[y] : 0.f;
  yinv = ok && MODE == 1 ? gscale / a.rsum[y] : 0.f;  // (the upstream scale rides on the normaliser)
  int tg = -3;
  if (ok) {
    const int64_t v = a.idx[y] - a.row0;
    tg = (v >= 0 && v < a.NX) ? (int)v : -3;
  }
  ytgt = tg;
  return tg >= (int)blockIdx.y * 256 && tg < (int)blockIdx.y * 256 + 256;
}

// online log-sum-exp over four more logits
template <bool MASKED>
__device__ __forceinline__ void lse_update(const float (&lg)[4], float& m, float& ssum) {
  const float gm = fmaxf(fmaxf(lg[0], lg[1]), fmaxf(lg[2], lg[3]));
  if (gm > m) {
    ssum *= __expf(m - gm);
    m = gm;
  }
  if (!MASKED || m > -INFINITY) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ssum += __expf(lg[r] - m);
  }
}

// w = g (softmax - onehot) without the onehot: exp(logit - max) * scale / sum of the pair's QUERY (the stationary vector when xq,
// else the streamed one); masked pairs 0  (own pairs: masked by the kernels, added by disc_own_bwd_kernel)
template <bool MASKED>
__device__ __forceinline__ void weights(float (&w)[4], const float (&lg)[4], bool xq, float xmax, float xinv, const float (&ymx)[4],
                                        const float (&yiv)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float p;
    if (xq)
      p = __expf(lg[r] - xmax) * xinv;
    else
      p = __expf(lg[r] - ymx[r]) * yiv[r];
    w[r] = (!MASKED || lg[r] > -INFINITY) ? p : 0.f;
  }
}

// MODE 2, after the barrier behind a 64-row tile: the four waves' slots ([64 y][LD] each, in red) and weight sums summed into this
// x-tile's slice of the partial buffers: plain stores (every (x-tile, y) is written exactly once); the next tile's slot writes are
// behind its staging barrier
template <int D, int LD>
__device__ __forceinline__ void flush_slots(const DiscMfmaArgs& a, const float* red, const float (&wy_lds)[4][64], int y0, int y_end) {
  const int tid = threadIdx.x;
  for (int e = tid; e < 64 * D; e += 256) {
    const int row = e / D, d = e % D, o = row * LD + d;
    if (y0 + row < y_end)
      a.G2[((int64_t)blockIdx.y * a.NY + y0 + row) * D + d] = (red[o] + red[64 * LD + o]) + (red[2 * 64 * LD + o] + red[3 * 64 * LD + o]);
  }
  if (tid < 64 && y0 + tid < y_end)
    a.WY[(int64_t)blockIdx.y * a.NY + y0 + tid] = (wy_lds[0][tid] + wy_lds[1][tid]) + (wy_lds[2][tid] + wy_lds[3][tid]);
}

// forward epilogue: merge the 4 lane groups that share a stationary vector, then one partial per (chunk, x)
__device__ __forceinline__ void fwd_epilogue(const DiscMfmaArgs& a, const float (&m)[4], const float (&ssum)[4], int x0) {
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float mm = m[t], ss = ssum[t];
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float om = __shfl_xor(mm, o, 64), os = __shfl_xor(ss, o, 64);
      const float nm = fmaxf(mm, om);
      // (an explicit fma: left to -ffp-contract the compiler fuses whichever product the operand order it happens to see puts
      // first, and the sum then changes in its last bit with the inlining around it)
      ss = (nm == -INFINITY) ? 0.f : __builtin_fmaf(ss, __expf(mm - nm), os * __expf(om - nm));
      mm = nm;
    }
    const int x = x0 + t * 16 + i;
    if (g == 0 && x < a.NX) a.part[(int64_t)blockIdx.x * a.NX + x] = make_float2(mm, ss);
  }
}

}  // namespace dt
}  // namespace fh
