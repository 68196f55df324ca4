// kaldi_cm.hip -- Kaldi's compressed feature matrices (matrix/compressed-matrix.{h,cc}: the tokens CM, CM2, CM3) decoded into
// and coded from the resident (frames, F) f32 matrix, a batch of utterances per launch.
//
// An utterance is a descriptor (FhvaeKaldiCmDesc: token, size, global header, byte offset of its payload in one uint8
// buffer, first row in the f32 matrix) and is cut into tiles of FHVAE_KALDI_CM_TILE_ROWS rows; a workgroup takes one tile
// (binary search of its index in the descriptors' tile0).  CM2 and CM3 are row-major like the matrix: element by element.
// CM stores a column's rows contiguously, the matrix a row's columns, so a tile goes through LDS, 128 columns at a time:
//   decode: aligned dwords along each column's rows -> LDS [column][33 dwords] (a column's bytes keep their offset within the
//           first dword, so global and LDS dwords line up whatever rows and the tile's first row are); then lanes run along a
//           row, pick their columns' bytes, decode with the column's four levels (LDS, decoded once per tile) and store 16 B.
//   encode: lanes along a row load 16 B, code with the column's levels, drop the bytes into the same LDS image; then whole
//           dwords go out along each column (bytes at the two ragged ends of a tile's column segment one by one).
// The LDS column stride of 33 dwords is odd: the dword phase walks a column (consecutive banks) and the byte phase walks
// columns (stride 33 banks); a lane that owns four adjacent columns meets 4-way conflicts on its byte accesses.  That is
// left as it is, and the kernels are NOT HBM-bound: one hour of 80-bin features decodes in 0.083 ms, 0.22 of the 8 TB/s peak
// (profiles/r11_bench_kaldi_compress.jsonl); whether the conflicts are what holds it there is not measured.
//
// Arithmetic: f32 with one rounding per operation (no contraction: the pragma below and -ffp-contract=off), correctly
// rounded division, in the order kaldi_io_lite.py uses, so the device and host codecs agree bit for bit and byte for byte.
//
// The encoder's statistics: per utterance min / max (atomics on the order-preserving uint32 image of the floats), then per
// (utterance, 8 columns) a workgroup finds s[0], s[rows/4], s[3 rows/4], s[rows-1] of every column exactly by a 4-pass
// radix select on that image with 256-bin LDS histograms (one histogram per rank once their prefixes part); the rows of any
// utterance length are streamed, never sorted or held.
//
// Every workgroup re-checks the descriptor it works on against the buffer sizes, so no table makes it read or write out
// of bounds; a check kernel also sets FHVAE_KALDI_CM_BAD_DESC in the status word and the launches behind it write nothing.
#pragma clang fp contract(off)

#include "common.h"

namespace fh {

using Desc = FhvaeKaldiCmDesc;
constexpr int kCmThreads = 256;
constexpr int kCmTR = FHVAE_KALDI_CM_TILE_ROWS;
constexpr int kCmCC = 128;            // columns per LDS pass
constexpr int kCmSD = kCmTR / 4 + 1;  // dwords per column in LDS: TR bytes and the 0..3 bytes in front of them
constexpr int kCmSelCols = 8;         // columns per select workgroup (32 B of a row)

__host__ __device__ inline int64_t cm_payload_size(int token, int64_t rows, int64_t cols) {
  return token == FHVAE_KALDI_CM ? cols * (8 + rows) : token == FHVAE_KALDI_CM2 ? 2 * rows * cols : rows * cols;
}

__device__ __forceinline__ int cm_tiles(int rows) { return (rows + kCmTR - 1) / kCmTR; }

// the descriptor's own fields against the buffers (tile0 is checked by the check kernel and, per tile, by cm_find)
__device__ __forceinline__ bool cm_desc_ok(int token, int rows, int cols, int64_t off, int64_t row0, int64_t n_bytes, int64_t n_frames,
                                           int64_t F) {
  if (token < FHVAE_KALDI_CM || token > FHVAE_KALDI_CM3 || rows <= 0 || cols <= 0 || cols != F) return false;
  if (off < 0 || (off & 3) != 0 || off > n_bytes || cm_payload_size(token, rows, cols) > n_bytes - off) return false;
  return row0 >= 0 && row0 <= n_frames && rows <= n_frames - row0;
}

// the utterance of tile b: the last u with tile0[u] <= b; -1 unless b is one of its tiles and its descriptor holds
__device__ __forceinline__ int64_t cm_find(const Desc* desc, int64_t U, int64_t b, int64_t n_bytes, int64_t n_frames, int64_t F) {
  int64_t lo = 0, hi = U - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (desc[mid].tile0 <= b) lo = mid; else hi = mid - 1;
  }
  const Desc& d = desc[lo];
  if (!cm_desc_ok(d.token, d.rows, d.cols, d.payload_off, d.row0, n_bytes, n_frames, F)) return -1;
  if (b < d.tile0 || b - d.tile0 >= cm_tiles(d.rows)) return -1;
  return lo;
}

// one thread per utterance: its descriptor, and tile0 as the running count of tiles
__global__ void cm_check_kernel(const Desc* __restrict__ desc, int64_t U, int64_t n_tiles, int64_t n_bytes, int64_t n_frames, int64_t F,
                                uint32_t* ws, int32_t* status) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const Desc& d = desc[u];
  bool ok = cm_desc_ok(d.token, d.rows, d.cols, d.payload_off, d.row0, n_bytes, n_frames, F);
  if (ok) {
    const int64_t next = (int64_t)d.tile0 + cm_tiles(d.rows);
    ok = d.tile0 >= 0 && (u == 0 ? d.tile0 == 0 : true) && (u == U - 1 ? next == n_tiles : next == desc[u + 1].tile0);
  }
  if (!ok) atomicOr(status, FHVAE_KALDI_CM_BAD_DESC);
  if (ws != nullptr) {
    ws[2 * u] = 0xFFFFFFFFu;  // min image
    ws[2 * u + 1] = 0u;       // max image
  }
}

// ---------------------------------------------------------------------------------------------------------------- decode
__device__ __forceinline__ float cm_u16(float mn, float rg, uint32_t w) { return mn + (rg * (float)w) / 65535.0f; }
__device__ __forceinline__ float cm_u8(float mn, float rg, uint32_t b) { return mn + (rg * (float)b) / 255.0f; }
__device__ __forceinline__ float cm_value(const float4 P, uint32_t b) {
  const float bf = (float)b;
  if (b <= 64) return P.x + ((P.y - P.x) * bf) * 0.015625f;
  if (b <= 192) return P.y + ((P.z - P.y) * (bf - 64.0f)) * 0.0078125f;
  return P.z + ((P.w - P.z) * (bf - 192.0f)) / 63.0f;
}

// the walk of a tile's (row, column group) items by 256 threads without a division per item
struct CmWalk {
  int r, g, dr, dg, ng;
  __device__ CmWalk(int tid, int ng_) : ng(ng_) {
    r = tid / ng; g = tid - r * ng; dr = kCmThreads / ng; dg = kCmThreads - dr * ng;
  }
  __device__ void next() {
    r += dr; g += dg;
    if (g >= ng) { g -= ng; ++r; }
  }
};

template <int V>
__global__ void __launch_bounds__(kCmThreads) cm_decompress_kernel(const uint8_t* __restrict__ payload, int64_t n_bytes,
                                                                   const Desc* __restrict__ desc, int64_t U, float* __restrict__ out,
                                                                   int64_t n_frames, int64_t F, const int32_t* status) {
  __shared__ uint32_t raw[kCmCC * kCmSD];
  __shared__ float4 lev[kCmCC];
  __shared__ int sh[kCmCC];
  if (*status & FHVAE_KALDI_CM_BAD_DESC) return;
  const int64_t u = cm_find(desc, U, blockIdx.x, n_bytes, n_frames, F);
  if (u < 0) return;
  const Desc d = desc[u];
  const int tid = threadIdx.x, C = d.cols, rows = d.rows;
  const int r0 = ((int)blockIdx.x - d.tile0) * kCmTR, nr = min(kCmTR, rows - r0);
  float* o = out + (d.row0 + r0) * F;
  const float mn = d.min_value, rg = d.range;
  if (d.token != FHVAE_KALDI_CM) {  // row-major: the tile's elements are contiguous on both sides
    const int64_t e0 = (int64_t)r0 * C;
    const int n = nr * C;
    if (d.token == FHVAE_KALDI_CM2) {
      const uint16_t* p = (const uint16_t*)(payload + d.payload_off) + e0;
      for (int i = tid; i < n; i += kCmThreads) o[i] = cm_u16(mn, rg, p[i]);
    } else {
      const uint8_t* p = payload + d.payload_off + e0;
      for (int i = tid; i < n; i += kCmThreads) o[i] = cm_u8(mn, rg, p[i]);
    }
    return;
  }
  const int64_t body = d.payload_off + 8 * (int64_t)C + r0;  // byte index of column 0's part of this tile
  for (int c0 = 0; c0 < C; c0 += kCmCC) {
    const int cc = min(kCmCC, C - c0);
    __syncthreads();
    if (tid < cc) {
      const uint32_t* h = (const uint32_t*)(payload + d.payload_off + 8 * (int64_t)(c0 + tid));
      const uint32_t a = h[0], b = h[1];
      lev[tid] = make_float4(cm_u16(mn, rg, a & 0xFFFFu), cm_u16(mn, rg, a >> 16), cm_u16(mn, rg, b & 0xFFFFu), cm_u16(mn, rg, b >> 16));
      sh[tid] = (int)((body + (int64_t)(c0 + tid) * rows) & 3);
    }
    for (int it = tid; it < cc * kCmSD; it += kCmThreads) {
      const int jl = it / kCmSD, k = it - jl * kCmSD;
      const int64_t g = body + (int64_t)(c0 + jl) * rows;
      const int64_t a = (g & ~(int64_t)3) + 4 * k;
      // (n_bytes is a multiple of 4: an aligned dword that starts inside the buffer ends inside it)
      raw[it] = (a < g + nr && a + 4 <= n_bytes) ? *(const uint32_t*)(payload + a) : 0u;
    }
    __syncthreads();
    const int ng = cc / V;
    const uint8_t* rb = (const uint8_t*)raw;
    for (CmWalk w(tid, ng); w.r < nr; w.next()) {
      float v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int jl = w.g * V + e;
        v[e] = cm_value(lev[jl], rb[jl * (kCmSD * 4) + sh[jl] + w.r]);
      }
      float* dst = o + (int64_t)w.r * F + c0 + w.g * V;
      if constexpr (V == 4) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
      else dst[0] = v[0];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- encode
__device__ __forceinline__ uint32_t cm_image(float v) {  // order-preserving: a < b as floats <=> image(a) < image(b)
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float cm_unimage(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// the global header of utterance u from the min / max images; false when a value is not finite.  The image orders -0.0
// below +0.0; a zero minimum is written as +0.0 (x + 0.0f is +0.0 for both zeros), as the host does
__device__ __forceinline__ bool cm_range(const uint32_t* ws, int64_t u, float& mn, float& rg) {
  mn = cm_unimage(ws[2 * u]) + 0.0f;
  float mx = cm_unimage(ws[2 * u + 1]);
  const bool finite = fabsf(mn) <= 3.402823466e38f && fabsf(mx) <= 3.402823466e38f;
  if (mx == mn) mx = mn + (1.0f + fabsf(mn));
  rg = mx - mn;
  return finite;
}

__device__ __forceinline__ int cm_quant(float v, float mn, float rg, float top) {
  float f = (v - mn) / rg;
  f = fminf(fmaxf(f, 0.0f), 1.0f);
  const float t = f * top;
  return (int)((double)t + 0.499);
}

__device__ __forceinline__ int cm_byte(float v, const float4 P) {
  if (v < P.y) {
    const float f = (v - P.x) / (P.y - P.x);
    const float t = f * 64.0f;
    return min(max((int)((double)t + 0.5), 0), 64);
  }
  if (v < P.z) {
    const float f = (v - P.y) / (P.z - P.y);
    const float t = f * 128.0f;
    return min(max(64 + (int)((double)t + 0.5), 64), 192);
  }
  const float f = (v - P.z) / (P.w - P.z);
  const float t = f * 63.0f;
  return min(max(192 + (int)((double)t + 0.5), 192), 255);
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

// (a) per-utterance min / max: a workgroup reduces its tile (contiguous in the matrix) and merges with two atomics per wave
__global__ void __launch_bounds__(kCmThreads) cm_minmax_kernel(const float* __restrict__ feats, int64_t n_frames, int64_t F,
                                                               const Desc* __restrict__ desc, int64_t U, int64_t n_bytes, uint32_t* ws,
                                                               const int32_t* status) {
  if (*status & FHVAE_KALDI_CM_BAD_DESC) return;
  const int64_t u = cm_find(desc, U, blockIdx.x, n_bytes, n_frames, F);
  if (u < 0) return;
  const int rows = desc[u].rows, C = desc[u].cols;
  const int r0 = ((int)blockIdx.x - desc[u].tile0) * kCmTR, nr = min(kCmTR, rows - r0);
  const float* x = feats + (desc[u].row0 + r0) * F;
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  for (int i = threadIdx.x; i < nr * C; i += kCmThreads) {
    const uint32_t k = cm_image(x[i]);
    lo = min(lo, k);
    hi = max(hi, k);
  }
  lo = wave_min_u32(lo);
  hi = wave_max_u32(hi);
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&ws[2 * u], lo);
    atomicMax(&ws[2 * u + 1], hi);
  }
}

// (b) the global header into the descriptor and, for CM, the column headers: workgroup (u, cg) selects the order statistics
// of columns 8 cg .. 8 cg + 7 of utterance u
__global__ void __launch_bounds__(kCmThreads) cm_select_kernel(const float* __restrict__ feats, int64_t n_frames, int64_t F, Desc* desc,
                                                               int64_t U, int64_t n_bytes, const uint32_t* __restrict__ ws,
                                                               uint8_t* __restrict__ payload, int32_t* status) {
  __shared__ uint32_t hist[kCmSelCols][2][256];
  __shared__ uint32_t pref[kCmSelCols][2], want[kCmSelCols][2], cmin[kCmSelCols], cmax[kCmSelCols];
  if (*status & FHVAE_KALDI_CM_BAD_DESC) return;
  const int ncg = (int)((F + kCmSelCols - 1) / kCmSelCols);
  const int64_t u = blockIdx.x / ncg;
  const int cg = blockIdx.x - (int)u * ncg, tid = threadIdx.x;
  if (u >= U) return;
  const int token = desc[u].token, rows = desc[u].rows, C = desc[u].cols;
  const int64_t off = desc[u].payload_off, row0 = desc[u].row0;
  if (!cm_desc_ok(token, rows, C, off, row0, n_bytes, n_frames, F)) return;
  float mn, rg;
  const bool finite = cm_range(ws, u, mn, rg);
  if (cg == 0 && tid == 0) {
    desc[u].min_value = mn;
    desc[u].range = rg;
    if (!finite) atomicOr(status, FHVAE_KALDI_CM_NONFINITE);
  }
  if (token != FHVAE_KALDI_CM) return;
  const int c0 = cg * kCmSelCols, nc = min(kCmSelCols, C - c0);
  const float* x0 = feats + row0 * F + c0;
  if (tid < kCmSelCols) {
    pref[tid][0] = pref[tid][1] = 0u;
    want[tid][0] = (uint32_t)(rows / 4);
    want[tid][1] = 3u * (uint32_t)(rows / 4);
    cmin[tid] = 0xFFFFFFFFu;
    cmax[tid] = 0u;
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t hi_mask = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);
    for (int i = tid; i < kCmSelCols * 2 * 256; i += kCmThreads) (&hist[0][0][0])[i] = 0u;
    __syncthreads();
    uint32_t p0[kCmSelCols], p1[kCmSelCols], lo[kCmSelCols], hi[kCmSelCols];
#pragma unroll
    for (int c = 0; c < kCmSelCols; ++c) {
      p0[c] = pref[c][0]; p1[c] = pref[c][1]; lo[c] = 0xFFFFFFFFu; hi[c] = 0u;
    }
    for (int r = tid; r < rows; r += kCmThreads) {
      const float* x = x0 + (int64_t)r * F;
#pragma unroll
      for (int c = 0; c < kCmSelCols; ++c) {
        if (c >= nc) break;
        const uint32_t k = cm_image(x[c]);
        const uint32_t top = k & hi_mask, dgt = (k >> shift) & 255u;
        if (top == p0[c]) atomicAdd(&hist[c][0][dgt], 1u);
        if (p1[c] != p0[c] && top == p1[c]) atomicAdd(&hist[c][1][dgt], 1u);
        if (pass == 0) { lo[c] = min(lo[c], k); hi[c] = max(hi[c], k); }
      }
    }
    if (pass == 0) {
#pragma unroll
      for (int c = 0; c < kCmSelCols; ++c) {
        if (c >= nc) break;
        atomicMin(&cmin[c], lo[c]);
        atomicMax(&cmax[c], hi[c]);
      }
    }
    __syncthreads();
    // one thread per (column, rank): the digit whose bin holds the wanted element of the current bucket
    uint32_t new_pref = 0u, new_want = 0u;
    const int c = tid >> 1, rk = tid & 1;
    const bool mine = tid < 2 * kCmSelCols && c < nc;
    if (mine) {
      const uint32_t* h = hist[c][pref[c][0] == pref[c][1] ? 0 : rk];
      uint32_t k = want[c][rk], cum = 0u, dgt = 0u;
      for (; dgt < 255u; ++dgt) {
        const uint32_t n = h[dgt];
        if (k < cum + n) break;
        cum += n;
      }
      new_pref = pref[c][rk] | (dgt << shift);
      new_want = k - cum;
    }
    __syncthreads();
    if (mine) {
      pref[c][rk] = new_pref;
      want[c][rk] = new_want;
    }
    __syncthreads();
  }
  if (tid < nc) {
    const int q0 = cm_quant(cm_unimage(cmin[tid]), mn, rg, 65535.0f), q25 = cm_quant(cm_unimage(pref[tid][0]), mn, rg, 65535.0f);
    const int q75 = cm_quant(cm_unimage(pref[tid][1]), mn, rg, 65535.0f), q100 = cm_quant(cm_unimage(cmax[tid]), mn, rg, 65535.0f);
    const int w0 = min(q0, 65532), w25 = min(max(q25, w0 + 1), 65533), w75 = min(max(q75, w25 + 1), 65534), w100 = max(q100, w75 + 1);
    uint32_t* h = (uint32_t*)(payload + off + 8 * (int64_t)(c0 + tid));
    h[0] = (uint32_t)w0 | ((uint32_t)w25 << 16);
    h[1] = (uint32_t)w75 | ((uint32_t)w100 << 16);
  }
}

// (c) the values: CM2 / CM3 element by element, CM through the LDS image of the tile
template <int V>
__global__ void __launch_bounds__(kCmThreads) cm_quantise_kernel(const float* __restrict__ feats, int64_t n_frames, int64_t F,
                                                                 const Desc* __restrict__ desc, int64_t U, int64_t n_bytes,
                                                                 uint8_t* payload, const int32_t* status) {
  __shared__ uint32_t raw[kCmCC * kCmSD];
  __shared__ float4 lev[kCmCC];
  __shared__ int sh[kCmCC];
  if (*status & FHVAE_KALDI_CM_BAD_DESC) return;
  const int64_t u = cm_find(desc, U, blockIdx.x, n_bytes, n_frames, F);
  if (u < 0) return;
  const Desc d = desc[u];
  const int tid = threadIdx.x, C = d.cols, rows = d.rows;
  const int r0 = ((int)blockIdx.x - d.tile0) * kCmTR, nr = min(kCmTR, rows - r0);
  const float* x = feats + (d.row0 + r0) * F;
  const float mn = d.min_value, rg = d.range;  // (written by cm_select_kernel, the launch before this one)
  if (d.token != FHVAE_KALDI_CM) {
    const int64_t e0 = (int64_t)r0 * C;
    const int n = nr * C;
    if (d.token == FHVAE_KALDI_CM2) {
      uint16_t* p = (uint16_t*)(payload + d.payload_off) + e0;
      for (int i = tid; i < n; i += kCmThreads) p[i] = (uint16_t)cm_quant(x[i], mn, rg, 65535.0f);
    } else {
      uint8_t* p = payload + d.payload_off + e0;
      for (int i = tid; i < n; i += kCmThreads) p[i] = (uint8_t)cm_quant(x[i], mn, rg, 255.0f);
    }
    return;
  }
  const int64_t body = d.payload_off + 8 * (int64_t)C + r0;
  const float step = rg * 1.52590218966964e-05f;
  for (int c0 = 0; c0 < C; c0 += kCmCC) {
    const int cc = min(kCmCC, C - c0);
    __syncthreads();
    if (tid < cc) {
      const uint32_t* h = (const uint32_t*)(payload + d.payload_off + 8 * (int64_t)(c0 + tid));
      const uint32_t a = h[0], b = h[1];
      lev[tid] = make_float4(mn + step * (float)(a & 0xFFFFu), mn + step * (float)(a >> 16), mn + step * (float)(b & 0xFFFFu),
                             mn + step * (float)(b >> 16));
      sh[tid] = (int)((body + (int64_t)(c0 + tid) * rows) & 3);
    }
    __syncthreads();
    const int ng = cc / V;
    uint8_t* rb = (uint8_t*)raw;
    for (CmWalk w(tid, ng); w.r < nr; w.next()) {
      const float* src = x + (int64_t)w.r * F + c0 + w.g * V;
      float v[V];
      if constexpr (V == 4) {
        const float4 t = *(const float4*)src;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
        v[0] = src[0];
      }
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int jl = w.g * V + e;
        rb[jl * (kCmSD * 4) + sh[jl] + w.r] = (uint8_t)cm_byte(v[e], lev[jl]);
      }
    }
    __syncthreads();
    for (int it = tid; it < cc * kCmSD; it += kCmThreads) {
      const int jl = it / kCmSD, k = it - jl * kCmSD;
      const int64_t g = body + (int64_t)(c0 + jl) * rows;  // the column segment is bytes [g, g + nr)
      const int64_t a = (g & ~(int64_t)3) + 4 * k;
      if (a + 4 <= g || a >= g + nr) continue;
      const uint32_t wv = raw[it];
      if (a >= g && a + 4 <= g + nr) {
        *(uint32_t*)(payload + a) = wv;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (a + e >= g && a + e < g + nr) payload[a + e] = (uint8_t)(wv >> (8 * e));
      }
    }
  }
}

static inline int cm_common_checks(int64_t n_bytes, int64_t U, int64_t n_tiles, int64_t n_frames, int64_t F) {
  FH_CHECK_POS(n_bytes);
  FH_CHECK_POS(U);
  FH_CHECK_POS(n_tiles);
  FH_CHECK_POS(n_frames);
  FH_CHECK_POS(F);
  if (n_bytes & 3) return FHVAE_ERR_ALIGN;
  FH_CHECK_I32(n_tiles);
  FH_CHECK_I32(F);
  FH_CHECK_I32(fh_cdiv(U, 256));
  return FHVAE_OK;
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_kaldi_decompress(const uint8_t* payload, int64_t n_bytes, const FhvaeKaldiCmDesc* desc, int64_t U, int64_t n_tiles,
                                      float* out, int64_t n_frames, int64_t F, int32_t* status, void* stream) {
  FH_CHECK_PTR(payload);
  FH_CHECK_PTR(desc);
  FH_CHECK_PTR(out);
  FH_CHECK_PTR(status);
  int rc = cm_common_checks(n_bytes, U, n_tiles, n_frames, F);
  if (rc != FHVAE_OK) return rc;
  if ((((uintptr_t)payload) & 3) != 0 || (((uintptr_t)out) & 3) != 0 || (((uintptr_t)desc) & 7) != 0) return FHVAE_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cm_check_kernel, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, s, desc, U, n_tiles, n_bytes, n_frames, F,
                     (uint32_t*)nullptr, status);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  const bool vec = (F & 3) == 0 && (((uintptr_t)out) & 15) == 0;  // rows of the matrix start on 16 B
  hipLaunchKernelGGL(vec ? cm_decompress_kernel<4> : cm_decompress_kernel<1>, dim3((unsigned)n_tiles), dim3(kCmThreads), 0, s, payload,
                     n_bytes, desc, U, out, n_frames, F, status);
  return fh_launch_status();
}

extern "C" int fhvae_kaldi_compress(const float* feats, int64_t n_frames, int64_t F, FhvaeKaldiCmDesc* desc, int64_t U, int64_t n_tiles,
                                    uint32_t* ws, uint8_t* payload, int64_t n_bytes, int32_t* status, void* stream) {
  FH_CHECK_PTR(feats);
  FH_CHECK_PTR(desc);
  FH_CHECK_PTR(ws);
  FH_CHECK_PTR(payload);
  FH_CHECK_PTR(status);
  int rc = cm_common_checks(n_bytes, U, n_tiles, n_frames, F);
  if (rc != FHVAE_OK) return rc;
  if ((((uintptr_t)payload) & 3) != 0 || (((uintptr_t)feats) & 3) != 0 || (((uintptr_t)desc) & 7) != 0 || (((uintptr_t)ws) & 3) != 0)
    return FHVAE_ERR_ALIGN;
  const int64_t ncg = fh_cdiv(F, kCmSelCols);
  FH_CHECK_I32(U * ncg);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cm_check_kernel, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, s, (const Desc*)desc, U, n_tiles, n_bytes, n_frames,
                     F, ws, status);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  hipLaunchKernelGGL(cm_minmax_kernel, dim3((unsigned)n_tiles), dim3(kCmThreads), 0, s, feats, n_frames, F, (const Desc*)desc, U, n_bytes,
                     ws, (const int32_t*)status);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  hipLaunchKernelGGL(cm_select_kernel, dim3((unsigned)(U * ncg)), dim3(kCmThreads), 0, s, feats, n_frames, F, desc, U, n_bytes,
                     (const uint32_t*)ws, payload, status);
  rc = fh_launch_status();
  if (rc != FHVAE_OK) return rc;
  const bool vec = (F & 3) == 0 && (((uintptr_t)feats) & 15) == 0;
  hipLaunchKernelGGL(vec ? cm_quantise_kernel<4> : cm_quantise_kernel<1>, dim3((unsigned)n_tiles), dim3(kCmThreads), 0, s, feats, n_frames,
                     F, (const Desc*)desc, U, n_bytes, payload, (const int32_t*)status);
  return fh_launch_status();
}
