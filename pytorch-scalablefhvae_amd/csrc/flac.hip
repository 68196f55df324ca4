// flac.hip -- FLAC (RFC 9639) frames decoded on the device, a batch of files per call.  The host (flac_lite.py) parses the
// container; everything behind a file's first frame is concatenated into one uint8 buffer and described by FhvaeFlacDesc.
//
// Stage 1, fhvae_flac_scan: one thread per byte position.  A position whose two bytes are the sync code goes on to the full
//   header test (flac_header: field rules, agreement with STREAMINFO, CRC-8) inside its file's byte range; the result is one
//   info word per position (0, or FHVAE_FLAC_CAND | block size << 8 | header bytes).  About one position in 2^15 passes the
//   first test, so the launch is a stream over the buffer: 1 B read and 4 B written per position.
// Stage 2, fhvae_flac_decode: one thread per candidate, 64 candidates per workgroup.  A frame is a serial code (each Rice
//   residual ends where the next begins, each sample needs the ones before it), so the parallelism is across frames: an hour
//   of 16 kHz speech is about 14 000 of them.  The stage is run twice ("parse twice" of DESIGN section 16):
//     out == NULL: every candidate is parsed to its end (subframes, padding, CRC-16) and nothing but its status, end and
//                  sample position is written.  No prediction is computed: whether a frame parses does not depend on it.
//     out != NULL: the candidates the host found to be the chain are parsed again, predicted and written to `out`.
//   A thread keeps the last 32 samples of its subframe and its LPC coefficients in LDS ([k][lane]: the 64 lanes of a row fall
//   into 64 consecutive banks), writes a sample to `out` once, and for the three stereo modes reads its block back at the end.
//
// Bounds: the bit reader holds the byte range of the candidate's file and returns zeros behind it, counting what it handed
// out; a parse that used a bit behind the range ends in FHVAE_FLAC_TRUNCATED, and the unary count stops at the range's end.
// Every write is inside [out_off, out_off + n_samples * channels) of the candidate's file, checked against n_out before the
// first one.  A descriptor that breaks the layout rules gives FHVAE_FLAC_BAD_DESC and the thread does nothing.
#include "common.h"

// the frame code is plain C++ that also compiles for the host, where a CPU build can be run under a debugger or sanitizer
#define FLAC_HD __host__ __device__

namespace fh {

using FDesc = FhvaeFlacDesc;
constexpr int kFlacThreads = 64;
constexpr int kFlacMaxOrder = 32;

FLAC_HD inline bool flac_desc_ok(const FDesc& d, int64_t n_bytes) {
  return d.byte_begin >= 0 && d.byte_begin <= d.byte_end && d.byte_end <= n_bytes && d.channels >= 1 && d.channels <= 8 && d.bps >= 4 &&
         d.bps <= 24 && d.rate >= 0 && d.min_block >= 0 && d.min_block <= 65535 && d.n_samples >= 0 && d.out_off >= 0;
}

// the file whose byte range holds pos (ranges ascend and do not overlap); -1 when there is none
FLAC_HD inline int64_t flac_find(const FDesc* desc, int64_t U, int64_t pos, int64_t n_bytes) {
  int64_t lo = 0, hi = U - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (desc[mid].byte_begin <= pos) lo = mid; else hi = mid - 1;
  }
  const FDesc& d = desc[lo];
  if (!flac_desc_ok(d, n_bytes) || pos < d.byte_begin || pos >= d.byte_end) return -1;
  return lo;
}

struct FlacHdr {
  int bs, hlen, assign, bps, strategy;
  uint64_t number;
};

// the frame header at pos, inside [pos, fend): every rule of the scan.  false: no frame starts here
FLAC_HD bool flac_header(const uint8_t* __restrict__ b, int64_t pos, int64_t fend, const FDesc& d, FlacHdr& h) {
  if (fend - pos < 6) return false;
  if (b[pos] != 0xFF || (b[pos + 1] & 0xFE) != 0xF8) return false;
  h.strategy = b[pos + 1] & 1;
  const int bsc = b[pos + 2] >> 4, rc = b[pos + 2] & 15;
  const int b3 = b[pos + 3];
  h.assign = b3 >> 4;
  const int ssc = (b3 >> 1) & 7;
  if (bsc == 0 || rc == 15 || h.assign > 10 || ssc == 3 || (b3 & 1)) return false;
  // the coded number: 0xxxxxxx, or 11..10 with that many bytes in all (2..7), each further one 10xxxxxx
  int k = 4;
  const int f = b[pos + k++];
  int extra = 0;
  if (f & 0x80) {
    extra = __builtin_clz((~(uint32_t)f << 24) | 0x00FFFFFFu) - 1;  // leading ones - 1
    if (extra < 1 || extra > 6) return false;
  }
  uint64_t num = extra == 0 ? (uint64_t)f : (uint64_t)(f & (0x7F >> (extra + 1)));
  if (fend - pos < 4 + 1 + extra + 1) return false;
  for (int i = 0; i < extra; ++i) {
    const int c = b[pos + k++];
    if ((c & 0xC0) != 0x80) return false;
    num = (num << 6) | (uint64_t)(c & 0x3F);
  }
  h.number = num;
  const int more = (bsc == 6 ? 1 : bsc == 7 ? 2 : 0) + (rc == 12 ? 1 : rc >= 13 ? 2 : 0);
  if (fend - pos < k + more + 1) return false;
  int bs;
  if (bsc == 1) bs = 192;
  else if (bsc <= 5) bs = 576 << (bsc - 2);
  else if (bsc == 6) bs = b[pos + k++] + 1;
  else if (bsc == 7) { bs = ((b[pos + k] << 8) | b[pos + k + 1]) + 1; k += 2; }
  else bs = 256 << (bsc - 8);
  if (bs > 65535) return false;
  h.bs = bs;
  int rate = 0;
  switch (rc) {
    case 1: rate = 88200; break;
    case 2: rate = 176400; break;
    case 3: rate = 192000; break;
    case 4: rate = 8000; break;
    case 5: rate = 16000; break;
    case 6: rate = 22050; break;
    case 7: rate = 24000; break;
    case 8: rate = 32000; break;
    case 9: rate = 44100; break;
    case 10: rate = 48000; break;
    case 11: rate = 96000; break;
    case 12: rate = b[pos + k++] * 1000; break;
    case 13: rate = (b[pos + k] << 8) | b[pos + k + 1]; k += 2; break;
    case 14: rate = ((b[pos + k] << 8) | b[pos + k + 1]) * 10; k += 2; break;
    default: break;
  }
  if (rc != 0 && rate != d.rate) return false;
  if ((h.assign < 8 ? h.assign + 1 : 2) != d.channels) return false;
  constexpr int kBits[8] = {0, 8, 12, 0, 16, 20, 24, 32};
  if (ssc != 0 && kBits[ssc] != d.bps) return false;
  h.bps = d.bps;
  uint32_t crc = 0;
  for (int i = 0; i < k; ++i) {
    crc ^= b[pos + i];
#pragma unroll
    for (int j = 0; j < 8; ++j) crc = (crc & 0x80) ? ((crc << 1) ^ 0x07) & 0xFF : (crc << 1);
  }
  if (crc != b[pos + k]) return false;
  h.hlen = k + 1;
  return true;
}

__global__ void __launch_bounds__(256) flac_scan_kernel(const uint8_t* __restrict__ buf, int64_t n_bytes, const FDesc* __restrict__ desc,
                                                        int64_t U, uint32_t* __restrict__ info) {
  const int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (pos >= n_bytes) return;
  uint32_t w = 0;
  if (pos + 1 < n_bytes && buf[pos] == 0xFF && (buf[pos + 1] & 0xFE) == 0xF8) {
    const int64_t u = flac_find(desc, U, pos, n_bytes);
    FlacHdr h;
    if (u >= 0 && flac_header(buf, pos, desc[u].byte_end, desc[u], h)) w = FHVAE_FLAC_CAND | ((uint32_t)h.bs << 8) | (uint32_t)h.hlen;
  }
  info[pos] = w;
}

// ---------------------------------------------------------------------------------------------------------------- bit reader
// Most significant bit first.  acc holds the next n bits at its top; bytes behind `end` read as zero, and used() > 8 * end
// afterwards says that the parse took some of them.
struct FlacBits {
  const uint8_t* __restrict__ p;
  int64_t pos, end;
  uint64_t acc;
  int n;
  uint32_t nxt;  // the four bytes at pos, loaded one refill ahead of their use so that the load's latency passes under the decoding
  FLAC_HD inline uint32_t load32(int64_t q) const {
    if (q + 4 <= end) {
      uint32_t w;
      __builtin_memcpy(&w, p + q, 4);
      return __builtin_bswap32(w);
    }
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) w = (w << 8) | (q + i < end ? (uint32_t)p[q + i] : 0u);
    return w;
  }
  FLAC_HD void init(const uint8_t* buf, int64_t start, int64_t e) { p = buf; pos = start; end = e; acc = 0; n = 0; nxt = load32(pos); }
  FLAC_HD inline void refill() {
    if (n <= 32) {
      acc |= (uint64_t)nxt << (32 - n);
      n += 32;
      pos += 4;
      nxt = load32(pos);
    }
  }
  FLAC_HD inline uint32_t get(int k) {  // 0 <= k <= 32
    refill();
    const uint32_t v = k == 0 ? 0u : (uint32_t)(acc >> (64 - k));
    acc <<= k;
    n -= k;
    return v;
  }
  FLAC_HD inline int32_t sget(int k) {  // signed, 0 <= k <= 32
    if (k == 0) return 0;
    const uint32_t v = get(k);
    return (int32_t)(v << (32 - k)) >> (32 - k);
  }
  FLAC_HD inline int64_t used() const { return pos * 8 - n; }
  // zeros up to the next 1 (which is taken too); -1 when the range ends first
  FLAC_HD int64_t unary() {
    int64_t q = 0;
    for (;;) {
      refill();
      if (acc != 0) {
        const int z = __builtin_clzll(acc);
        acc <<= z;  // z <= n - 1 <= 63; the 1 goes with one more shift
        acc <<= 1;
        n -= z + 1;
        return q + z;
      }
      q += n;
      n = 0;
      if (pos >= end) return -1;
    }
  }
};

FLAC_HD inline int flac_fixed_coef(int order, int i) {
  // x[n-1-i] coefficients of the fixed predictors of order 1..4
  constexpr int c[4][4] = {{1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
  return c[order - 1][i];
}

// one subframe of `bs` samples at `sbps` bits.  WRITE: sample i goes to o[i * stride].  Returns a FHVAE_FLAC_* status
template <bool WRITE>
FLAC_HD int flac_subframe(FlacBits& br, int bs, int sbps, int32_t* __restrict__ o, int stride, int32_t* hist, int32_t* coef) {
  if (br.get(1) != 0) return FHVAE_FLAC_BAD_SUBFRAME;
  const int type = (int)br.get(6);
  int wasted = 0;
  if (br.get(1)) {
    const int64_t u = br.unary();
    if (u < 0) return FHVAE_FLAC_TRUNCATED;
    if (u + 1 >= sbps) return FHVAE_FLAC_BAD_SUBFRAME;
    wasted = (int)u + 1;
    sbps -= wasted;
  }
  if (type == 0) {
    const int32_t v = br.sget(sbps);
    if constexpr (WRITE)
      for (int i = 0; i < bs; ++i) o[(int64_t)i * stride] = (int32_t)((uint32_t)v << wasted);
    return FHVAE_OK;
  }
  if (type == 1) {
    for (int i = 0; i < bs; ++i) {
      const int32_t v = br.sget(sbps);
      if constexpr (WRITE) o[(int64_t)i * stride] = (int32_t)((uint32_t)v << wasted);
      if ((i & 63) == 63 && br.used() > br.end * 8) return FHVAE_FLAC_TRUNCATED;  // (a cut file: no need to walk the rest)
    }
    return FHVAE_OK;
  }
  int order, shift = 0;
  const bool lpc = type >= 32;
  if (lpc) order = type - 31;
  else if (type >= 8 && type <= 12) order = type - 8;
  else return FHVAE_FLAC_BAD_SUBFRAME;
  if (order > bs) return FHVAE_FLAC_BAD_SUBFRAME;
  for (int i = 0; i < order; ++i) {
    const int32_t v = br.sget(sbps);
    if constexpr (WRITE) {
      hist[(i & (kFlacMaxOrder - 1)) * kFlacThreads] = v;
      o[(int64_t)i * stride] = (int32_t)((uint32_t)v << wasted);
    }
  }
  if (lpc) {
    const int prec = (int)br.get(4) + 1;
    if (prec == 16) return FHVAE_FLAC_BAD_LPC;
    shift = br.sget(5);
    if (shift < 0) return FHVAE_FLAC_BAD_LPC;
    for (int i = 0; i < order; ++i) {
      const int32_t c = br.sget(prec);
      if constexpr (WRITE) coef[i * kFlacThreads] = c;
    }
  } else if constexpr (WRITE) {
    for (int i = 0; i < order; ++i) coef[i * kFlacThreads] = flac_fixed_coef(order, i);
  }
  const int method = (int)br.get(2);
  if (method > 1) return FHVAE_FLAC_BAD_RESIDUAL;
  const int pbits = method == 0 ? 4 : 5, esc = (1 << pbits) - 1;
  const int po = (int)br.get(4);
  if ((bs & ((1 << po) - 1)) != 0 || (bs >> po) < order) return FHVAE_FLAC_BAD_RESIDUAL;
  const int psize = bs >> po;
  int i = order;
  for (int part = 0; part < (1 << po); ++part) {
    const int cnt = psize - (part == 0 ? order : 0);
    const int k = (int)br.get(pbits);
    const int raw = k == esc ? (int)br.get(5) : 0;
    for (int j = 0; j < cnt; ++j, ++i) {
      int32_t r;
      if (k == esc) {
        r = br.sget(raw);
      } else {
        const int64_t q = br.unary();
        if (q < 0) return FHVAE_FLAC_TRUNCATED;
        const uint64_t u = ((uint64_t)q << k) | (uint64_t)br.get(k);
        if (u > 0xFFFFFFFFull) return FHVAE_FLAC_BAD_RESIDUAL;  // (a residual has 32 bits)
        r = (int32_t)((uint32_t)(u >> 1) ^ (0u - (uint32_t)(u & 1)));
      }
      if constexpr (WRITE) {
        int64_t sum = 0;
        for (int t = 0; t < order; ++t)
          sum += (int64_t)coef[t * kFlacThreads] * (int64_t)hist[((i - 1 - t) & (kFlacMaxOrder - 1)) * kFlacThreads];
        const int32_t v = (int32_t)((sum >> shift) + (int64_t)r);
        hist[(i & (kFlacMaxOrder - 1)) * kFlacThreads] = v;
        o[(int64_t)i * stride] = (int32_t)((uint32_t)v << wasted);
      }
    }
    if (br.used() > br.end * 8) return FHVAE_FLAC_TRUNCATED;
  }
  return FHVAE_OK;
}

// one candidate: header, subframes, padding, CRC-16 (parse) or the stereo step (WRITE)
template <bool WRITE>
FLAC_HD void flac_frame(const uint8_t* __restrict__ buf, int64_t n_bytes, const FDesc* __restrict__ desc, int64_t U, int64_t pos,
                        int32_t* __restrict__ out, int64_t n_out, int32_t* hist, int32_t* coef, const uint16_t* crc_tab, int& st, int64_t& end,
                        int64_t& spos) {
  st = FHVAE_OK;
  end = -1;
  spos = -1;
  const int64_t u = pos >= 0 && pos < n_bytes ? flac_find(desc, U, pos, n_bytes) : -1;
  if (u < 0) { st = FHVAE_FLAC_BAD_DESC; return; }
  const FDesc d = desc[u];
  FlacHdr h;
  if (!flac_header(buf, pos, d.byte_end, d, h)) { st = FHVAE_FLAC_BAD_HEADER; return; }
  spos = h.strategy ? (int64_t)h.number : (int64_t)h.number * d.min_block;
  const int nch = d.channels;
  int32_t* o = nullptr;
  if constexpr (WRITE) {
    // the frame's samples must lie inside its file's part of `out`, and that inside `out`
    if (spos < 0 || spos > d.n_samples || h.bs > d.n_samples - spos || d.out_off > n_out || d.n_samples > (n_out - d.out_off) / nch) {
      st = FHVAE_FLAC_BAD_RANGE;
      return;
    }
    o = out + d.out_off + spos * nch;
  }
  FlacBits br;
  br.init(buf, pos + h.hlen, d.byte_end);
  for (int c = 0; c < nch; ++c) {
    const bool side = (h.assign == 8 && c == 1) || (h.assign == 9 && c == 0) || (h.assign == 10 && c == 1);
    st = flac_subframe<WRITE>(br, h.bs, h.bps + (side ? 1 : 0), WRITE ? o + c : nullptr, nch, hist, coef);
    if (st != FHVAE_OK) return;
  }
  const int pad = (int)((8 - (br.used() & 7)) & 7);
  if (br.get(pad) != 0) { st = FHVAE_FLAC_BAD_PADDING; return; }
  const uint32_t want = br.get(16);
  const int64_t e = br.used() >> 3;
  if (e > d.byte_end) { st = FHVAE_FLAC_TRUNCATED; return; }
  if constexpr (!WRITE) {
    uint32_t crc = 0;
    for (int64_t i = pos; i < e - 2; ++i) crc = ((crc << 8) & 0xFFFF) ^ crc_tab[(crc >> 8) ^ buf[i]];
    if (crc != want) { st = FHVAE_FLAC_BAD_CRC; return; }
  } else if (h.assign >= 8) {
    for (int i = 0; i < h.bs; ++i) {
      const int32_t a = o[(int64_t)i * 2], b = o[(int64_t)i * 2 + 1];
      if (h.assign == 8) {  // left, side
        o[(int64_t)i * 2 + 1] = a - b;
      } else if (h.assign == 9) {  // side, right
        o[(int64_t)i * 2] = a + b;
      } else {  // mid, side
        const int32_t m = (int32_t)(((uint32_t)a << 1) | ((uint32_t)b & 1u));
        o[(int64_t)i * 2] = (m + b) >> 1;
        o[(int64_t)i * 2 + 1] = (m - b) >> 1;
      }
    }
  }
  end = e;
}

FLAC_HD inline uint16_t flac_crc16_entry(int v) {
  uint32_t c = (uint32_t)v << 8;
  for (int j = 0; j < 8; ++j) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1);
  return (uint16_t)c;
}

template <bool WRITE>
__global__ void __launch_bounds__(kFlacThreads) flac_decode_kernel(const uint8_t* __restrict__ buf, int64_t n_bytes,
                                                                   const FDesc* __restrict__ desc, int64_t U,
                                                                   const int64_t* __restrict__ cand_pos, int64_t n_cand,
                                                                   int32_t* __restrict__ cand_status, int64_t* __restrict__ cand_end,
                                                                   int64_t* __restrict__ cand_spos, int32_t* __restrict__ out, int64_t n_out) {
  __shared__ int32_t hist_s[WRITE ? kFlacMaxOrder * kFlacThreads : 1];
  __shared__ int32_t coef_s[WRITE ? kFlacMaxOrder * kFlacThreads : 1];
  __shared__ uint16_t crc_tab[256];
  const int tid = threadIdx.x;
  if constexpr (!WRITE) {
    for (int v = tid; v < 256; v += kFlacThreads) crc_tab[v] = flac_crc16_entry(v);
    __syncthreads();
  }
  const int64_t ci = (int64_t)blockIdx.x * kFlacThreads + tid;
  if (ci >= n_cand) return;
  int st;
  int64_t end, spos;
  flac_frame<WRITE>(buf, n_bytes, desc, U, cand_pos[ci], out, n_out, hist_s + (WRITE ? tid : 0), coef_s + (WRITE ? tid : 0), crc_tab, st, end,
                    spos);
  cand_status[ci] = st;
  cand_end[ci] = end;
  cand_spos[ci] = spos;
}

}  // namespace fh

using namespace fh;

extern "C" int fhvae_flac_scan(const uint8_t* buf, int64_t n_bytes, const FhvaeFlacDesc* desc, int64_t U, uint32_t* info, void* stream) {
  FH_CHECK_PTR(buf);
  FH_CHECK_PTR(desc);
  FH_CHECK_PTR(info);
  FH_CHECK_POS(n_bytes);
  FH_CHECK_POS(U);
  FH_CHECK_I32(fh_cdiv(n_bytes, 256));
  if ((((uintptr_t)desc) & 7) != 0 || (((uintptr_t)info) & 3) != 0) return FHVAE_ERR_ALIGN;
  hipLaunchKernelGGL(flac_scan_kernel, dim3((unsigned)fh_cdiv(n_bytes, 256)), dim3(256), 0, (hipStream_t)stream, buf, n_bytes, desc, U, info);
  return fh_launch_status();
}

extern "C" int fhvae_flac_decode(const uint8_t* buf, int64_t n_bytes, const FhvaeFlacDesc* desc, int64_t U, const int64_t* cand_pos,
                                 int64_t n_cand, int32_t* cand_status, int64_t* cand_end, int64_t* cand_spos, int32_t* out, int64_t n_out,
                                 void* stream) {
  FH_CHECK_PTR(buf);
  FH_CHECK_PTR(desc);
  FH_CHECK_PTR(cand_pos);
  FH_CHECK_PTR(cand_status);
  FH_CHECK_PTR(cand_end);
  FH_CHECK_PTR(cand_spos);
  FH_CHECK_POS(n_bytes);
  FH_CHECK_POS(U);
  FH_CHECK_POS(n_cand);
  if (out != nullptr) FH_CHECK_POS(n_out);
  FH_CHECK_I32(fh_cdiv(n_cand, kFlacThreads));
  if ((((uintptr_t)desc) & 7) != 0 || (((uintptr_t)cand_pos) & 7) != 0 || (((uintptr_t)cand_end) & 7) != 0 ||
      (((uintptr_t)cand_spos) & 7) != 0 || (((uintptr_t)cand_status) & 3) != 0 || (((uintptr_t)out) & 3) != 0)
    return FHVAE_ERR_ALIGN;
  const dim3 grid((unsigned)fh_cdiv(n_cand, kFlacThreads)), block(kFlacThreads);
  if (out == nullptr)
    hipLaunchKernelGGL(flac_decode_kernel<false>, grid, block, 0, (hipStream_t)stream, buf, n_bytes, desc, U, cand_pos, n_cand, cand_status,
                       cand_end, cand_spos, out, n_out);
  else
    hipLaunchKernelGGL(flac_decode_kernel<true>, grid, block, 0, (hipStream_t)stream, buf, n_bytes, desc, U, cand_pos, n_cand, cand_status,
                       cand_end, cand_spos, out, n_out);
  return fh_launch_status();
}
