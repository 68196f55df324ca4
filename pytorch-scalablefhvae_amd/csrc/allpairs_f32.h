// allpairs_f32.h -- the exact-f32 all-pairs pass that disc_mfma.hip (the f32 K5), sv.hip and tsne.hip share: device inline
// pieces only, compiled into each file under that file's own flags (no division and no square root in here: sv.hip is
// built with correctly rounded ones, the others are not, and the pieces must give the same bits in all three).
//
// A workgroup of 256 threads keeps 256 STATIONARY rows X (64 per wave, as MFMA B-operand fragments in registers) and
// streams the other rows Y through swizzled LDS in tiles of 64; the dots X . Y run on v_mfma_f32_16x16x4_f32 (every
// product and every accumulation step an f32 fma), the caller's epilogue on the VALU.  With lane = 16 g + i:
//   stationary   lane (g, i) of tile t holds X[x0 + 16 t + i][16 jj + 4 g .. + 3]                   (B operands)
//   streamed     lane (g, i) of block yb reads Y[y0 + 16 yb + i][16 jj + 4 g .. + 3] from LDS       (A operands)
//   dot tile     acc[t][r] = X[x0 + 16 t + i] . Y[y0 + 16 yb + 4 g + r]: the stationary row on the lanes' i, four streamed
//                rows per lane group g in the four accumulator registers; the four lanes (g = 0..3) of a stationary row
//                merge their sums by two xor shuffles (quad_sum / quad_min).
//
// THE ORDER.  Every accumulator, in the single chain (dot) and in the four interleaved ones of stream() alike, meets the columns in
// the order jj ascending, then x, y, z, w of the 16-byte chunk, and one MFMA adds its four g in the hardware's fixed order:
// the k order does not depend on which of the two rows is stationary (both operands use the same lane <-> column layout),
// and a product of two floats commutes.  So dot(i, j) == dot(j, i) bit for bit: the symmetry that sv.hip's scores and
// tsne.hip's distances rest on.
#pragma once
#include "common.h"

namespace fh {
namespace ap {

constexpr int kYT = 64;  // streamed rows per LDS tile

// byte offset of 16-byte chunk ch of LDS row `row` ([kYT][D] f32); the xor stays inside an aligned group of 8 / 4 chunks
template <int D>
__device__ __forceinline__ int yoff(int row, int ch) {
  static_assert(D % 16 == 0 && D >= 16 && D <= 128, "D = 16, 32 .. 128");
  constexpr int CHN = D / 4;
  return row * (D * 4) + ((ch ^ (row & (CHN % 8 == 0 ? 7 : 3))) << 4);
}

// the stationary fragments of a wave's 64 rows from x0 on; rows past nrows are zero
template <int D>
__device__ __forceinline__ void load_stationary(const float* __restrict__ x, int64_t ld, int nrows, int x0, uint4 (&xf)[4][D / 16]) {
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int r = x0 + t * 16 + i;
#pragma unroll
    for (int jj = 0; jj < D / 16; ++jj) {
      uint4 u = make_uint4(0, 0, 0, 0);
      if (r < nrows) u = *(const uint4*)(x + (int64_t)r * ld + 4 * g + 16 * jj);
      xf[t][jj] = u;
    }
  }
}

// (TileMover and read_a serve disc_mfma.hip's own loop; stream() below holds the same two spelled out, see there: a change to
// either copy goes into both.)
// A 64-row tile of Y on its way to LDS: issue(y0) loads rows y0 .. y0 + 63 into registers (rows from y_end on: zeros),
// commit() stores them swizzled.  The loads of the next tile fly while the workgroup computes on this one.
template <int D>
struct TileMover {
  static constexpr int CHN = D / 4, LOADS = kYT * CHN / 256;  // 16-byte chunks per row, per thread per tile
  const float* __restrict__ y;
  int64_t ld;
  int y_end;
  char* ytile;
  uint4 st[LOADS];
  __device__ __forceinline__ TileMover(const float* y_, int64_t ld_, int y_end_, char* ytile_) : y(y_), ld(ld_), y_end(y_end_), ytile(ytile_) {}
  __device__ __forceinline__ void issue(int y0) {
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int id = threadIdx.x + p * 256;
      const int row = y0 + id / CHN, ch = id % CHN;
      st[p] = (row < y_end) ? *(const uint4*)(y + (int64_t)row * ld + ch * 4) : make_uint4(0, 0, 0, 0);
    }
  }
  __device__ __forceinline__ void commit() {
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int id = threadIdx.x + p * 256;
      *(uint4*)(ytile + yoff<D>(id / CHN, id % CHN)) = st[p];
    }
  }
};

// the A fragments of block yb (16 streamed rows) of the tile in LDS
template <int D>
__device__ __forceinline__ void read_a(const char* ytile, int yb, uint4 (&af)[D / 16]) {
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
#pragma unroll
  for (int jj = 0; jj < D / 16; ++jj) af[jj] = *(const uint4*)(ytile + yoff<D>(yb * 16 + i, g + 4 * jj));
}

// one dot tile: D / 4 dependent MFMAs in THE ORDER
template <int D>
__device__ __forceinline__ f32x4 dot(const uint4 (&af)[D / 16], const uint4 (&xf)[D / 16]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int jj = 0; jj < D / 16; ++jj) {
    const uint4 ua = af[jj], ub = xf[jj];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.x), __uint_as_float(ub.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.y), __uint_as_float(ub.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.z), __uint_as_float(ub.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.w), __uint_as_float(ub.w), acc, 0, 0, 0);
  }
  return acc;
}

struct EveryBlock {
  __device__ __forceinline__ bool operator()(int) const { return true; }
};

// Stream rows y_begin .. y_end - 1 (y_begin < y_end) against the wave's stationary rows.  Per tile: side(y0) fills the
// caller's per-row LDS arrays (every thread calls it, before the barrier); per block of 16 streamed rows from ybase =
// y0 + 16 yb on, unless want(ybase) says no (uniform over the wave), pair(y0, yb, acc) gets the four dot tiles: four
// independent chains, interleaved (the 16x16x4 form needs two in flight to reach its issue rate), per accumulator THE ORDER, so
// acc[t] has the bits of dot(af, xf[t]).  The loop spells the mover, the A read and the chains out: written as calls of the
// pieces above the compiler schedules the t-SNE kernels differently, and their affinity pass measured 0.8 % slower.
template <int D, class Side, class Want, class Pair>
__device__ __forceinline__ void stream(const float* __restrict__ y, int64_t ld, int y_begin, int y_end, char* ytile,
                                       const uint4 (&xf)[4][D / 16], Side side, Want want, Pair pair) {
  constexpr int CHN = D / 4, LOADS = kYT * CHN / 256;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, i = lane & 15;
  uint4 st[LOADS];
  auto issue = [&](int y0) {
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int id = tid + p * 256;
      const int row = id / CHN, ch = id % CHN;
      st[p] = (y0 + row < y_end) ? *(const uint4*)(y + (int64_t)(y0 + row) * ld + ch * 4) : make_uint4(0, 0, 0, 0);
    }
  };
  issue(y_begin);
  for (int y0 = y_begin; y0 < y_end; y0 += kYT) {
#pragma unroll
    for (int p = 0; p < LOADS; ++p) {
      const int id = tid + p * 256;
      *(uint4*)(ytile + yoff<D>(id / CHN, id % CHN)) = st[p];
    }
    side(y0);
    __syncthreads();
    if (y0 + kYT < y_end) issue(y0 + kYT);
#pragma unroll 1
    for (int yb = 0; yb < kYT / 16; ++yb) {
      if (y0 + yb * 16 >= y_end) break;
      if (!want(y0 + yb * 16)) continue;
      uint4 af[D / 16];
#pragma unroll
      for (int jj = 0; jj < D / 16; ++jj) af[jj] = *(const uint4*)(ytile + yoff<D>(yb * 16 + i, g + 4 * jj));
      f32x4 acc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int jj = 0; jj < D / 16; ++jj) {
        const uint4 ua = af[jj];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.x), __uint_as_float(xf[t][jj].x), acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.y), __uint_as_float(xf[t][jj].y), acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.z), __uint_as_float(xf[t][jj].z), acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(ua.w), __uint_as_float(xf[t][jj].w), acc[t], 0, 0, 0);
      }
      pair(y0, yb, acc);
    }
    __syncthreads();
  }
}

// over the four lanes (g = 0..3) of a stationary row; commutative, so the four end with equal bits
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
__device__ __forceinline__ float quad_min(float v) {
  v = fminf(v, __shfl_xor(v, 16, 64));
  return fminf(v, __shfl_xor(v, 32, 64));
}

}  // namespace ap
}  // namespace fh
