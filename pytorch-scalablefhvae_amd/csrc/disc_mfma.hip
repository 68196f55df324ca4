// disc_mfma.hip -- K5 on the matrix cores (large tables; simple_fhvae.py:119-122).
//
//   logit[b,s] = -c |q_b - t_s|^2 = 2c (q_b . t_s) - c |q_b|^2 - c |t_s|^2
//
// The cross term q.t is a (B x S x D) contraction: it runs on exact-f32 MFMA (v_mfma_f32_16x16x4_f32: every product
// and every accumulation step is an f32 fma, so the expanded form costs only the cancellation of the norms, ~1e-5
// absolute on logits of 10..1000), and the exp / online log-sum-exp runs on the VALU under it (separate pipes).
// The VALU kernels in disc.hip spend 2*D lane-instructions per (query,row) pair on the distance alone.
//
// One kernel template, three uses.  A workgroup keeps 256 STATIONARY vectors X (64 per wave, as MFMA B-operand
// fragments in registers) and streams the other set Y through LDS in tiles of 64 (the pieces of allpairs_f32.h, in a loop of
// its own: two barriers per tile with the norms taken from the LDS image in between, and a software pipeline over the tiles):
//   MODE 0  forward   X = queries,    Y = table rows : per-query online (max, sumexp) partials per row chunk
//   MODE 1  dq        X = queries,    Y = table rows : G_x = sum_y w[y,x] Y_y  on MFMA again -> dq = 2c (G - q W)
//   MODE 1  dtable    X = table rows, Y = queries    : same formula gives dt = 2c (G - t W)
// with w = g (softmax - onehot) recomputed from the per-query (max, sumexp) of the forward.  The logit tile comes out
// of the MFMA with the stationary index on the lanes (col = lane&15) and the streamed index in the 4 accumulator
// registers (row = 4*(lane>>4)+r): exactly the B-operand layout of the second product, so w never leaves registers.
// This file holds the kernel and its launch (disc_f32_launch); the arithmetic around the products is disc_tile.h's, shared with the
// bf16 kernel of disc_lp.hip; the engine choice, the grids, the workspaces and the reduce kernels are disc.hip's.
#include "allpairs_f32.h"
#include "disc_tile.h"

#include <type_traits>

namespace fh {

namespace {

using ap::yoff;

// (The (query, own table row) pairs are masked out here and taken in the direct form by the callers: disc_tile.h.)
template <int D, int MODE>
__global__ __launch_bounds__(256, 2) void disc_mfma_kernel(DiscMfmaArgs a) {
  constexpr int CHN = D / 4;   // 16-byte chunks per vector
  constexpr int NJ = D / 16;   // 16-k groups (also 16-wide d blocks)
  constexpr int YT = ap::kYT;  // streamed vectors per LDS tile
  __shared__ __attribute__((aligned(16))) char ytile[YT * D * 4];
  __shared__ __attribute__((aligned(16))) float yn[YT];
  __shared__ float ymax[YT], yinv[YT];
  __shared__ int ytgt[YT];
  __shared__ int yown[YT / 16];  // streamed queries: block b holds one whose own row is among this workgroup's stationary rows
  // MODE 2 (queries stationary only) = MODE 1 plus the STREAMED side's gradient from the same weights (disc_lp.hip has the
  // bf16 form and the reasoning): G2[y][d] = sum_x w[y,x] X[x][d] contracts over x, which sits on the lanes of the logit tile, so
  // each wave passes its weights through a private [16 y][64 x] f32 LDS image (4 ds_write_b32 per tile, one ds_read_b128 back:
  // lane (g, i) gets w[y = i][x = 16t + 4g .. + 3], the A operands of the 4 MFMAs of tile t); B = X[x0 + 16t + 4g + q][16dj + i].  WY[y] = sum_x w[y,x] is summed on the VALU from the same transposed registers.  Per-wave LDS slots,
  // partial buffers and the two reduce kernels of disc.hip instead of atomics.
  constexpr bool BW = MODE >= 1, BOTH = MODE == 2;
  constexpr int kWLd = 68;        // row stride of the weight image (floats): the 4 lane groups write different banks
  constexpr int kDtLd = D + 4;    // row stride of a slot
  __shared__ __attribute__((aligned(16))) float wimg[BOTH ? 4 : 1][BOTH ? 16 * kWLd : 4];
  __shared__ float wy_lds[BOTH ? 4 : 1][BOTH ? YT : 1];
  __shared__ __attribute__((aligned(16))) float red[dt::red_floats(D, MODE, kDtLd)];  // epilogue: tr; MODE 2, in the loop: 4 slots
  float (*tr)[D + 1] = (float (*)[D + 1]) red;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  // blockIdx.x = chunk of the STREAMED set: round-robin XCD placement then gives every XCD (private L2) 1/8 of the
  // streamed vectors (the table, 128 MB at 1M rows) instead of all of them
  const int x0 = blockIdx.y * 256 + wave * 64;
  const int y_begin = blockIdx.x * a.chunk;
  const int y_end = min(a.NY, y_begin + a.chunk);
  const float gscale = BW ? (*a.gsc) * a.gmul : 0.f;

  // ---- stationary fragments, as ap::load_stationary lays them out, with the norm summed next to the load (the shared load and
  // a norm loop after it cost disc_mfma_kernel<32, 2> one more spilled register)
  uint4 xf[4][NJ];
  float xn[4], xmax[4], xinv[4];
  int xtgt[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int x = x0 + t * 16 + i;
    const bool ok = x < a.NX;
    float nrm = 0.f;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      uint4 u = make_uint4(0, 0, 0, 0);
      if (ok) u = *(const uint4*)(a.X + (int64_t)x * D + 4 * g + 16 * jj);
      xf[t][jj] = u;
      const float f0 = __uint_as_float(u.x), f1 = __uint_as_float(u.y), f2 = __uint_as_float(u.z), f3 = __uint_as_float(u.w);
      nrm += f0 * f0 + f1 * f1 + f2 * f2 + f3 * f3;
    }
    nrm += __shfl_xor(nrm, 16, 64);
    nrm += __shfl_xor(nrm, 32, 64);
    xn[t] = nrm;
    dt::x_scalars<BW>(a, a.x_is_query, x, ok, gscale, xmax[t], xinv[t], xtgt[t]);
  }
  float m[4], ssum[4], wsum[4];
  f32x4 gacc[4][NJ];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    m[t] = -INFINITY;
    ssum[t] = 0.f;
    wsum[t] = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) gacc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- stream Y in tiles of 64 vectors
  ap::TileMover<D> mv(a.Y, D, y_end, ytile);
  if (y_begin < y_end) mv.issue(y_begin);
  for (int y0 = y_begin; y0 < y_end; y0 += YT) {
    mv.commit();
    __syncthreads();
    if (y0 + YT < y_end) mv.issue(y0 + YT);
    // per-y scalars: norm (4 lanes per vector), and for streamed queries their (max, 1/sum, target)
    {
      const int row = tid >> 2, part = tid & 3;  // 64 rows x 4 lanes
      float nrm = 0.f;
#pragma unroll
      for (int c4 = part; c4 < CHN; c4 += 4) {
        const uint4 u = *(const uint4*)(ytile + yoff<D>(row, c4));
        const float f0 = __uint_as_float(u.x), f1 = __uint_as_float(u.y), f2 = __uint_as_float(u.z), f3 = __uint_as_float(u.w);
        nrm += f0 * f0 + f1 * f1 + f2 * f2 + f3 * f3;
      }
      nrm += __shfl_xor(nrm, 1, 64);
      nrm += __shfl_xor(nrm, 2, 64);
      bool mine = false;
      if (part == 0) {
        yn[row] = nrm;
        if (!a.x_is_query) mine = dt::y_scalars<MODE>(a, y0 + row, y_end, gscale, ymax[row], yinv[row], ytgt[row]);
      }
      {  // wave w holds the 16 rows of block w
        const bool any = __any(mine);
        if (lane == 0) yown[wave] = any ? 1 : 0;
      }
    }
    __syncthreads();

#pragma unroll 1
    for (int yb = 0; yb < YT / 16; ++yb) {
      if (y0 + yb * 16 >= y_end) break;
      // A fragments of the logit product: Y[yb*16+i][4g+16jj .. +3]
      uint4 af[NJ];
      ap::read_a<D>(ytile, yb, af);
      const float4 ynv = *(const float4*)(yn + yb * 16 + 4 * g);
      const float ynr[4] = {ynv.x, ynv.y, ynv.z, ynv.w};
      float ymx[4], yiv[4];
      int ytg[4];
      if (MODE == 1 && !a.x_is_query) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ymx[r] = ymax[yb * 16 + 4 * g + r];
          yiv[r] = yinv[yb * 16 + 4 * g + r];
          ytg[r] = ytgt[yb * 16 + 4 * g + r];
        }
      }
      // interior blocks without a (query, own row) pair take the body without the validity / own-row selects (disc_lp.hip)
      const int ybase = y0 + yb * 16;
      const bool whole = ybase + 16 <= y_end && x0 + 64 <= a.NX;
      const bool own_blk = !a.x_is_query && yown[yb] != 0;
      const float c2 = 2.f * a.c;
      f32x4 oacc[BOTH ? NJ : 1];
      float wyp = 0.f;
      if constexpr (BOTH) {
#pragma unroll
        for (int dj = 0; dj < NJ; ++dj) oacc[dj] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      // the logit product of tile t: 8 dependent MFMAs
      auto logits = [&](int t) __attribute__((always_inline)) -> f32x4 { return ap::dot<D>(af, xf[t]); };
      auto tile = [&](int t, auto masked_c, const f32x4& acc) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_c)::value;
        // MODE 2: B operands of the streamed side's product, xb[q][dj] = X[x0 + 16t + 4g + q][16dj + i], fetched per tile (L1 /
        // L2 hits) rather than held: 32 more stationary registers would halve the occupancy.  Vectors past NX are clamped: their
        // weights are zero.
        const bool xok = x0 + t * 16 + i < a.NX;
        const float cxn = a.c * xn[t];
        float lg[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // (the same text as in disc_lp.hip, see there)
          lg[r] = c2 * acc[r] - (a.c * ynr[r] + cxn);
          if constexpr (MASKED) {
            const int y = ybase + 4 * g + r;
            if (!(xok && y < y_end)) lg[r] = -INFINITY;
            // the query's own row is handled exactly by the callers (disc_tile.h)
            const bool own = (MODE == 1 && !a.x_is_query) ? ytg[r] == xtgt[t] : xtgt[t] == y;
            if (own) lg[r] = -INFINITY;
          }
        }
        if constexpr (MODE == 0) {
          dt::lse_update<MASKED>(lg, m[t], ssum[t]);
        } else {
          float w[4];
          dt::weights<MASKED>(w, lg, a.x_is_query, xmax[t], xinv[t], ymx, yiv);
#pragma unroll
          for (int r = 0; r < 4; ++r) wsum[t] += w[r];
          float xb[BOTH ? 4 : 1][NJ];  // MODE 2: requested behind the exp arithmetic; their latency hides under the G product's MFMAs
          if constexpr (BOTH) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int x = min(x0 + 16 * t + 4 * g + q, a.NX - 1);
#pragma unroll
              for (int dj = 0; dj < NJ; ++dj) xb[q][dj] = a.X[(int64_t)x * D + 16 * dj + i];
            }
          }
          // G^T[d][x] += sum_y Y[y][d] * w[y][x]: A = Y^T from LDS (lane: d = 16*dj + i, y = 4g + r), B = w[r]
#pragma unroll
          for (int dj = 0; dj < NJ; ++dj) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = yb * 16 + 4 * g + r, d = dj * 16 + i;
              const float av = *(const float*)(ytile + yoff<D>(row, d >> 2) + (d & 3) * 4);
              gacc[t][dj] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[r], gacc[t][dj], 0, 0, 0);
            }
          }
          if constexpr (BOTH) {
            float* wi = wimg[wave];
#pragma unroll
            for (int r = 0; r < 4; ++r) wi[(4 * g + r) * kWLd + 16 * t + i] = w[r];
            asm volatile("" ::: "memory");  // (LDS operations of one wave complete in order; only the compiler must keep it)
            const float4 wt = *(const float4*)(wi + i * kWLd + 16 * t + 4 * g);  // w[y = i][x = 16t + 4g + q]
            asm volatile("" ::: "memory");
            const float wq[4] = {wt.x, wt.y, wt.z, wt.w};
            wyp += (wq[0] + wq[1]) + (wq[2] + wq[3]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int dj = 0; dj < NJ; ++dj) oacc[dj] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[q], xb[q][dj], oacc[dj], 0, 0, 0);
          }
        }
      };
      // Interior blocks with no masked tile (all but a few per cent): ONE basic block for the four tiles, tile t + 1's logit MFMAs
      // issued before tile t's exp / weight arithmetic, so that the matrix pipe works under the VALU of the same wave (with a
      // branch per tile the chains ran one after the other: MfmaUtil 46 % forward; S = 1M forward 1.81 -> 1.65 ms).
      bool any_masked = !whole || own_blk;
      if (a.x_is_query) {
#pragma unroll
        for (int t = 0; t < 4; ++t) any_masked = any_masked || __any((unsigned)(xtgt[t] - ybase) < 16u);
      }
      if (!BOTH && !any_masked) {  // (the one-pass backward has no registers for a second accumulator in flight: 101 spills)
        f32x4 nxt = logits(0);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 cur = nxt;
          if (t + 1 < 4) nxt = logits(t + 1);
          tile(t, std::false_type{}, cur);
        }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          bool masked = !whole || own_blk;
          if (a.x_is_query) masked = masked || __any((unsigned)(xtgt[t] - ybase) < 16u);
          const f32x4 acc = logits(t);
          if (masked)
            tile(t, std::true_type{}, acc);
          else
            tile(t, std::false_type{}, acc);
        }
      }
      if constexpr (BOTH) {  // lane holds out[y = 4g + r][d = 16dj + i] -> the wave's slot; wyp: the partial row sum of y = i
        float* slot = red + wave * (YT * kDtLd);
#pragma unroll
        for (int dj = 0; dj < NJ; ++dj)
#pragma unroll
          for (int r = 0; r < 4; ++r) slot[(yb * 16 + 4 * g + r) * kDtLd + 16 * dj + i] = oacc[dj][r];
        wyp += __shfl_xor(wyp, 16, 64);
        wyp += __shfl_xor(wyp, 32, 64);
        if (g == 0) wy_lds[wave][yb * 16 + i] = wyp;
      }
    }
    __syncthreads();
    if constexpr (BOTH) dt::flush_slots<D, kDtLd>(a, red, wy_lds, y0, y_end);
  }

  if constexpr (MODE == 0) {
    dt::fwd_epilogue(a, m, ssum, x0);
  } else {
    if constexpr (BOTH) __syncthreads();  // (tr shares its memory with the slots the last tile's sums were read from)
    // (the same text as in disc_lp.hip, see there)
    // grad_x = 2c (G - X W); lane holds G[x = 16t+i][d = 16dj + 4g + reg]; transpose through LDS -> row-contiguous atomics
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float ws = wsum[t];
      ws += __shfl_xor(ws, 16, 64);
      ws += __shfl_xor(ws, 32, 64);
#pragma unroll
      for (int dj = 0; dj < NJ; ++dj) {
        const int x = x0 + t * 16 + i;
        float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (x < a.NX) xv = *(const float4*)(a.X + (int64_t)x * D + dj * 16 + 4 * g);
        const float xr[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) tr[wave * 64 + t * 16 + i][dj * 16 + 4 * g + r] = 2.f * a.c * (gacc[t][dj][r] - xr[r] * ws);
      }
    }
    __syncthreads();
    for (int e = tid; e < 256 * D; e += 256) {
      const int rr = e / D, d = e % D;
      const int x = blockIdx.y * 256 + rr;
      if (x < a.NX) {
        if constexpr (BOTH)
          a.G[((int64_t)blockIdx.x * a.NX + x) * D + d] = tr[rr][d];  // this chunk's slice of the partial buffer
        else
          atomicAdd(a.G + (int64_t)x * D + d, tr[rr][d]);
      }
    }
  }
}

template <int D>
void launch_d(const DiscMfmaArgs& a, int mode, dim3 grid, hipStream_t st) {
  if (mode == 0)
    hipLaunchKernelGGL((disc_mfma_kernel<D, 0>), grid, dim3(256), 0, st, a);
  else if (mode == 1)
    hipLaunchKernelGGL((disc_mfma_kernel<D, 1>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((disc_mfma_kernel<D, 2>), grid, dim3(256), 0, st, a);
}

}  // namespace

void disc_f32_launch(const DiscMfmaArgs& a, int D, int mode, dim3 grid, hipStream_t st) {
  if (D == 32)
    launch_d<32>(a, mode, grid, st);
  else
    launch_d<16>(a, mode, grid, st);
}

}  // namespace fh
