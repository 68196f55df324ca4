// ctcbeam.hip -- CTC prefix beam search with an optional label bigram (include/fhvae_ctcbeam.h):
//   fhvae_cb_decode : per utterance the best labelling among the prefixes a beam of W keeps, its length and its score
//
// One workgroup of four waves per utterance; the search is sequential in t and parallel over the at most W + W C candidates of a
// frame.  The beam (pb, pnb, lm, node, parent node, last label, length) lives in LDS in two halves, the frame's log-softmax too
// (every wave computes it with trellis.h's tr_log_softmax, as ctc.hip does, wave 0 parks it; the row is loaded a frame ahead).  A thread owns stay(tid) and the
// extensions tid + 256 r: at most 33 candidates, each an order-preserving 64-bit key of its score.
// Selection: the W best under (score, index) by a radix select over the digits of (key, 65535 - index), eight bits a pass with an
// LDS histogram, starting at the first byte in which the keys differ and stopping as soon as a bin holds exactly what is still
// needed; the survivors are ranked among themselves (W x W) and written to the other half in rank order.
// Prefix identity: one node per prefix in a per-utterance trie in the workspace (parent, label, first child, next sibling).
// Lane r of wave 0 walks the children of its parent for every kept extension and only makes a node when none is found; new
// nodes are numbered in beam order by a ballot.  The table is read through L2: a frame touches the at most W rows of the
// beam's last labels, every row C consecutive doubles, and the whole table does not fit LDS beside the rest at C = 128.
//
// Arithmetic: the header's expressions as written (the pragma below and -ffp-contract=off).
#pragma clang fp contract(off)

#include <math.h>

#include "common.h"
#include "trellis.h"

#include "../../include/fhvae_ctcbeam.h"

namespace fh {

constexpr int kCbW = FHVAE_CB_MAX_BEAM;
constexpr int kCbC = FHVAE_CB_MAX_CLASSES;
constexpr int kCbThreads = 256;
constexpr int kCbRounds = (kCbW + kCbW * kCbC + kCbThreads - 1) / kCbThreads;  // 33 candidates a thread at most

static_assert(FHVAE_CB_MAX_CLASSES == kTrMaxClasses, "a lane owns two classes (trellis.h)");
static_assert(FHVAE_CB_MAX_BEAM == 64, "a lane of wave 0 owns a beam position");
static_assert(kCbRounds <= 64, "a thread's candidates are one bit each of a 64-bit mask");
static_assert(kCbW + kCbW * kCbC <= 0xffff, "a candidate index is two digits");
static_assert(FHVAE_CB_NODE_BYTES == 16, "a node is an int4");

typedef unsigned long long cb_u64;

// larger score, larger key; -0 and +0 share a key; 0 is kept for "no candidate" (also a score of -inf)
__device__ __forceinline__ cb_u64 cb_key(double s) {
  if (!(s > -INFINITY)) return 0;
  const cb_u64 b = (cb_u64)__double_as_longlong(s + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

struct CbLds {
  double lp[kCbC + 1];  // the frame's log-softmax; entry C (the empty prefix's "last label") is -inf
  double pb[2][kCbW], pnb[2][kCbW], lm[2][kCbW];
  double tot[kCbW], spb[kCbW], spnb[kCbW], sscore[kCbW], fin[kCbW];
  cb_u64 excl[kCbW][2];  // the labels c for which prefix_i + c is in the beam
  cb_u64 open[2];
  cb_u64 skey[kCbW];     // the survivors, in arrival order
  cb_u64 rmax[4], rmin[4];
  int node[2][kCbW], par[2][kCbW], last[2][kCbW], len[2][kCbW];
  int parpos[kCbW];
  int sidx[kCbW];
  unsigned hist[256];
  int wsum[4], rcnt[4];
  int sel[3];
  int nsurv;
  int root_child;
};

// extend(i, c): its score and its (pnb', lm'); -inf if it is no candidate
__device__ __forceinline__ double cb_extend(const CbLds& sm, int cur, int n, int C, int blank, const double* __restrict__ lm, int i, int c,
                                            double& pnb, double& l) {
  if (i >= n || c == blank || !((sm.open[c >> 6] >> (c & 63)) & 1) || ((sm.excl[i][c >> 6] >> (c & 63)) & 1)) return -INFINITY;
  const int li = sm.last[cur][i];
  pnb = (c == li ? sm.pb[cur][i] : sm.tot[i]) + sm.lp[c];
  l = sm.lm[cur][i] + (lm != nullptr ? lm[(int64_t)li * (C + 1) + c] : 0.0);
  return pnb + l;
}

// A thread's candidates are its slots: slot 0 is stay(tid), slot s >= 1 is the extension e = tid + 256 (s - 1) = i C + c.  The
// keys are not kept: a slot's key is computed again wherever it is needed (a handful of LDS reads and one table entry), which
// costs less than 33 live 64-bit registers or an array the compiler puts into scratch.
struct CbSlots {
  int i, c, qi, qc;  // the extension of the slot at hand; the step of 256 extensions as (256 / C, 256 % C)
  __device__ __forceinline__ void start(int tid, int C) { i = tid / C, c = tid - i * C, qi = kCbThreads / C, qc = kCbThreads - qi * C; }
  __device__ __forceinline__ void rewind(int tid, int C) { i = tid / C, c = tid - i * C; }
  __device__ __forceinline__ void step(int C) {
    i += qi, c += qc;
    if (c >= C) c -= C, i += 1;
  }
};

__device__ __forceinline__ cb_u64 cb_slot_key(const CbLds& sm, int cur, int n, int C, int blank, const double* __restrict__ lm, int tid, int s,
                                              const CbSlots& sl) {
  if (s == 0) return tid < n ? cb_key(sm.sscore[tid]) : 0;
  double a, b;
  return cb_key(cb_extend(sm, cur, n, C, blank, lm, sl.i, sl.c, a, b));
}

__device__ __forceinline__ unsigned cb_digit(cb_u64 key, int k, int p) {
  return p < 8 ? (unsigned)(key >> (56 - 8 * p)) & 255u : ((unsigned)(0xffff - k) >> (8 * (9 - p))) & 255u;
}

__global__ void __launch_bounds__(kCbThreads)
    cb_decode_kernel(const float* __restrict__ logits, int64_t ldz, int64_t n_frames, int C, int blank, const int64_t* __restrict__ utt_ptr,
                     int64_t U, int W, double class_beam, const double* __restrict__ lm, int32_t* __restrict__ hyp,
                     int32_t* __restrict__ hyp_len, double* __restrict__ score, int32_t* status, int4* ws, int64_t ws_nodes) {
  __shared__ CbLds sm;
  if (*status & FHVAE_CB_BAD_PTR) return;  // (set by the check kernel)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- the utterance.  Everything up to the first barrier is the same in all threads: they return together or not at all
  const int64_t u = blockIdx.x;
  if (u >= U || C < 2 || C > kCbC || blank < 0 || blank >= C || W < 1 || W > kCbW) return;
  const int64_t u0 = utt_ptr[u], u1 = utt_ptr[u + 1];
  if (!tr_utt_ok(u0, u1, n_frames)) return;
  const int T = (int)(u1 - u0);
  if (u0 > ws_nodes / W || (int64_t)T > ws_nodes / W - u0) return;  // (the host has refused a workspace this small already)
  int4* nodes = ws + u0 * W;                                      // node id v >= 1 is nodes[v - 1]; node 0 is the empty prefix
  const int64_t cap = (int64_t)T * W;
  const float* z = logits + u0 * ldz;

  int cur = 0, n = 1, next_node = 1;
  CbSlots sl;
  sl.start(tid, C);
  if (tid == 0) {
    sm.pb[0][0] = 0.0, sm.pnb[0][0] = -INFINITY, sm.lm[0][0] = 0.0;
    sm.node[0][0] = 0, sm.par[0][0] = -1, sm.last[0][0] = C, sm.len[0][0] = 0;
    sm.root_child = 0;
    sm.lp[C] = -INFINITY;
  }
  sm.hist[tid] = 0;
  float n0 = 0.f, n1 = 0.f;
  if (T > 0) tr_load_row(z, C, lane, n0, n1);
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    // ---- the row's log-softmax (the one ctc.hip trains with: every lane of every wave ends with the same bits) and the open classes
    const float z0 = n0, z1 = n1;
    if (t + 1 < T) tr_load_row(z + (int64_t)(t + 1) * ldz, C, lane, n0, n1);
    {
      const TrLogSoftmax r = tr_log_softmax(z0, z1);
      const double thr = (0.0 - r.lg) - class_beam;  // (the largest lp is that of the row maximum: 0 - lg)
      const cb_u64 o0 = __ballot(lane < C && r.l0 >= thr), o1 = __ballot(lane + 64 < C && r.l1 >= thr);
      if (wave == 0) {
        if (lane < C) sm.lp[lane] = r.l0;
        if (lane + 64 < C) sm.lp[lane + 64] = r.l1;
        if (lane == 0) sm.open[0] = o0, sm.open[1] = o1;
      }
    }
    // ---- per entry: tot, where its parent sits, which of its children sit in the beam
    if (tid < n) {
      sm.tot[tid] = tr_lse2(sm.pb[cur][tid], sm.pnb[cur][tid]);
      const int me = sm.node[cur][tid], mypar = sm.par[cur][tid];
      int pp = -1;
      cb_u64 e0 = 0, e1 = 0;
      for (int j = 0; j < n; ++j) {
        if (sm.node[cur][j] == mypar) pp = j;
        if (sm.par[cur][j] == me) {
          const int c = sm.last[cur][j];
          if (c < 64) e0 |= 1ULL << c; else e1 |= 1ULL << (c - 64);
        }
      }
      sm.parpos[tid] = pp, sm.excl[tid][0] = e0, sm.excl[tid][1] = e1;
    }
    __syncthreads();
    // ---- stay(i)
    if (tid < n) {
      const int li = sm.last[cur][tid], j = sm.parpos[tid];
      const double pb = sm.tot[tid] + sm.lp[blank];
      double pnb = li < C ? sm.pnb[cur][tid] + sm.lp[li] : -INFINITY;
      if (j >= 0 && li < C && ((sm.open[li >> 6] >> (li & 63)) & 1)) {
        const double ext = (li == sm.last[cur][j] ? sm.pb[cur][j] : sm.tot[j]) + sm.lp[li];
        pnb = tr_lse2(pnb, ext);
      }
      sm.spb[tid] = pb, sm.spnb[tid] = pnb;
      sm.sscore[tid] = tr_lse2(pb, pnb) + sm.lm[cur][tid];
    }
    if (tid == 0) sm.nsurv = 0;
    __syncthreads();
    // ---- the candidates: how many, the largest and the smallest key
    const int nslot = 1 + (n * C + kCbThreads - 1) / kCbThreads;
    cb_u64 alive = 0, kept = 0, kmax = 0, kmin = ~0ULL;
    sl.rewind(tid, C);
    for (int s = 0; s < nslot; ++s) {
      const cb_u64 key = cb_slot_key(sm, cur, n, C, blank, lm, tid, s, sl);
      if (key != 0) {
        alive |= 1ULL << s;
        kmax = key > kmax ? key : kmax;
        kmin = key < kmin ? key : kmin;
      }
      if (s > 0) sl.step(C);
    }
    int cnt = __popcll(alive);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o, 64);
      const cb_u64 v = __shfl_xor(kmax, o, 64), w = __shfl_xor(kmin, o, 64);
      kmax = v > kmax ? v : kmax;
      kmin = w < kmin ? w : kmin;
    }
    if (lane == 0) sm.rcnt[wave] = cnt, sm.rmax[wave] = kmax, sm.rmin[wave] = kmin;
    __syncthreads();
    const int n_valid = sm.rcnt[0] + sm.rcnt[1] + sm.rcnt[2] + sm.rcnt[3];
    if (n_valid == 0) {  // the beam has emptied out (uniform)
      if (tid == 0) hyp_len[u] = 0, score[u] = -INFINITY, atomicOr(status, FHVAE_CB_EMPTY);
      return;
    }
    if (n_valid <= W) {
      kept = alive;
    } else {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        kmax = sm.rmax[w] > kmax ? sm.rmax[w] : kmax;
        kmin = sm.rmin[w] < kmin ? sm.rmin[w] : kmin;
      }
      const cb_u64 diff = kmax ^ kmin;  // every key lies between them, so it shares the digits they share
      int need = W, pp = -1;            // pp: the pass whose decision (digit dd) the slots have not seen yet
      unsigned dd = 0;
      for (int p = diff != 0 ? __clzll((long long)diff) >> 3 : 8; p < 10; ++p) {
        sl.rewind(tid, C);
        for (int s = 0; s < nslot; ++s) {
          if ((alive >> s) & 1) {
            const cb_u64 key = cb_slot_key(sm, cur, n, C, blank, lm, tid, s, sl);
            const int k = s == 0 ? tid : W + tid + (s - 1) * kCbThreads;
            bool on = true;
            if (pp >= 0) {
              const unsigned dg = cb_digit(key, k, pp);
              if (dg > dd) kept |= 1ULL << s;
              if (dg != dd) alive &= ~(1ULL << s), on = false;
            }
            if (on) atomicAdd(&sm.hist[cb_digit(key, k, p)], 1u);
          }
          if (s > 0) sl.step(C);
        }
        __syncthreads();
        const int h = (int)sm.hist[tid];
        sm.hist[tid] = 0;
        int sfx = h;  // the candidates whose digit is at least tid
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int v = __shfl_down(sfx, o, 64);
          if (lane + o < 64) sfx += v;
        }
        if (lane == 0) sm.wsum[wave] = sfx;
        __syncthreads();
        for (int w = wave + 1; w < 4; ++w) sfx += sm.wsum[w];
        if (sfx >= need && sfx - h < need) sm.sel[0] = tid, sm.sel[1] = sfx - h, sm.sel[2] = h;
        __syncthreads();
        pp = p, dd = (unsigned)sm.sel[0];
        need -= sm.sel[1];
        if (sm.sel[2] == need) break;  // (uniform) all that still match are kept; at p = 9 a bin holds one candidate at most
      }
      sl.rewind(tid, C);
      for (int s = 0; s < nslot; ++s) {  // the last decision
        if ((alive >> s) & 1) {
          const cb_u64 key = cb_slot_key(sm, cur, n, C, blank, lm, tid, s, sl);
          const unsigned dg = cb_digit(key, s == 0 ? tid : W + tid + (s - 1) * kCbThreads, pp);
          if (dg > dd) kept |= 1ULL << s;
          if (dg != dd) alive &= ~(1ULL << s);
        }
        if (s > 0) sl.step(C);
      }
      kept |= alive;
    }
    // ---- the survivors, in arrival order
    sl.rewind(tid, C);
    for (int s = 0; s < nslot; ++s) {
      if ((kept >> s) & 1) {
        const int at = atomicAdd(&sm.nsurv, 1);
        if (at < kCbW) sm.skey[at] = cb_slot_key(sm, cur, n, C, blank, lm, tid, s, sl), sm.sidx[at] = s == 0 ? tid : W + tid + (s - 1) * kCbThreads;
      }
      if (s > 0) sl.step(C);
    }
    __syncthreads();
    const int ns = sm.nsurv < W ? sm.nsurv : W;
    const int nxt = cur ^ 1;
    if (tid < ns) {  // rank among the survivors, then the entry at its place in the other half
      const cb_u64 mk = sm.skey[tid];
      const int k = sm.sidx[tid];
      int rank = 0;
      for (int j = 0; j < ns; ++j) {
        const cb_u64 ok = sm.skey[j];
        rank += (ok > mk || (ok == mk && sm.sidx[j] < k)) ? 1 : 0;
      }
      if (k < W) {
        sm.pb[nxt][rank] = sm.spb[k], sm.pnb[nxt][rank] = sm.spnb[k], sm.lm[nxt][rank] = sm.lm[cur][k];
        sm.node[nxt][rank] = sm.node[cur][k], sm.par[nxt][rank] = sm.par[cur][k];
        sm.last[nxt][rank] = sm.last[cur][k], sm.len[nxt][rank] = sm.len[cur][k];
      } else {
        const int e = k - W, i = e / C;
        double pnb = -INFINITY, l = -INFINITY;
        cb_extend(sm, cur, n, C, blank, lm, i, e - i * C, pnb, l);
        sm.pb[nxt][rank] = -INFINITY, sm.pnb[nxt][rank] = pnb, sm.lm[nxt][rank] = l;
        sm.node[nxt][rank] = -1, sm.par[nxt][rank] = sm.node[cur][i];
        sm.last[nxt][rank] = e - i * C, sm.len[nxt][rank] = sm.len[cur][i] + 1;
      }
    }
    __syncthreads();
    // ---- the trie: wave 0, lane r is beam position r
    if (wave == 0) {
      const bool ext = lane < ns && sm.node[nxt][lane] < 0;
      int found = 0, parent = 0, label = 0;
      if (ext) {
        parent = sm.par[nxt][lane], label = sm.last[nxt][lane];
        // (a node's first child is only ever exchanged atomically, in L2: it is read from there, past the vector L1)
        int v = parent == 0 ? sm.root_child
                            : (parent >= 1 && parent < next_node ? __hip_atomic_load(&nodes[parent - 1].z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0);
        for (int step = 0; step < C && v >= 1 && v < next_node; ++step) {
          const int4 nd = nodes[v - 1];
          if (nd.y == label) {
            found = v;
            break;
          }
          v = nd.w;
        }
      }
      const cb_u64 fresh = __ballot(ext && found == 0);
      if (ext && found == 0) {
        const int id = next_node + __popcll(fresh & ((1ULL << lane) - 1));
        if ((int64_t)id <= cap && parent >= 0 && parent < next_node) {
          const int sib = parent == 0 ? atomicExch(&sm.root_child, id) : atomicExch(&nodes[parent - 1].z, id);
          nodes[id - 1] = make_int4(parent, label, 0, sib);
          found = id;
        }
      }
      if (ext) sm.node[nxt][lane] = found;
    }
    __syncthreads();
    next_node += __popcll(__ballot(lane < ns && sm.node[nxt][lane] >= next_node));  // (every wave counts the same entries)
    cur = nxt, n = ns;
    __syncthreads();
  }

  // ---- the best final score, the first position that has it; its labels through the trie, written forward
  if (tid < n) {
    const int li = sm.last[cur][tid];
    sm.fin[tid] = (tr_lse2(sm.pb[cur][tid], sm.pnb[cur][tid]) + sm.lm[cur][tid]) + (lm != nullptr ? lm[(int64_t)li * (C + 1) + C] : 0.0);
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int i = 1; i < n; ++i)
      if (sm.fin[i] > sm.fin[best]) best = i;
    int L = sm.len[cur][best];
    if (L > T) L = 0;  // (cannot happen: a frame adds one label at most)
    int v = sm.node[cur][best];
    for (int k = L - 1; k >= 0 && v >= 1 && v < next_node; --k) {
      const int4 nd = nodes[v - 1];
      hyp[u0 + k] = nd.y;
      v = nd.x;
    }
    hyp_len[u] = L;
    score[u] = sm.fin[best];
  }
}

static inline int64_t cb_ws(int64_t n_frames, int64_t W) { return (n_frames * W * FHVAE_CB_NODE_BYTES + 255) / 256 * 256; }

}  // namespace fh

using namespace fh;

extern "C" int64_t fhvae_cb_ws_bytes(int64_t n_frames, int64_t W) {
  if (n_frames < 0 || n_frames > (1LL << 52) || W < 1 || W > FHVAE_CB_MAX_BEAM) return 0;
  return cb_ws(n_frames, W);
}

extern "C" int fhvae_cb_decode(const float* logits, int64_t ldz, int64_t n_frames, int64_t C, int64_t blank, const int64_t* utt_ptr,
                               int64_t U, int64_t W, double class_beam, const double* lm, int32_t* hyp, int32_t* hyp_len, double* score,
                               int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
  FH_CHECK_PTR(status);
  if (C < 2 || blank < 0 || blank >= C || n_frames < 0 || U < 0 || ldz < C || ws_bytes < 0) return FHVAE_ERR_SHAPE;
  if (!(class_beam >= 0.0)) return FHVAE_ERR_SHAPE;
  if (C > FHVAE_CB_MAX_CLASSES || W < 1 || W > FHVAE_CB_MAX_BEAM || n_frames > (1LL << 52)) return FHVAE_ERR_LIMIT;
  FH_CHECK_I32(U);
  if (ws_bytes < cb_ws(n_frames, W)) return FHVAE_ERR_SHAPE;
  if (U == 0) return FHVAE_OK;
  FH_CHECK_PTR(logits);
  FH_CHECK_PTR(utt_ptr);
  FH_CHECK_PTR(hyp);
  FH_CHECK_PTR(hyp_len);
  FH_CHECK_PTR(score);
  FH_CHECK_PTR(ws);
  if (ldz % 4 != 0 || ((uintptr_t)logits & 15) != 0 || ((uintptr_t)ws & 15) != 0) return FHVAE_ERR_ALIGN;
  if (((uintptr_t)utt_ptr & 7) != 0 || ((uintptr_t)lm & 7) != 0 || ((uintptr_t)hyp & 3) != 0 || ((uintptr_t)hyp_len & 3) != 0 ||
      ((uintptr_t)score & 7) != 0 || ((uintptr_t)status & 3) != 0)
    return FHVAE_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tr_check_kernel<FHVAE_CB_BAD_PTR>, dim3((unsigned)fh_cdiv(U, 256)), dim3(256), 0, st, utt_ptr, U, n_frames, status);
  hipLaunchKernelGGL(cb_decode_kernel, dim3((unsigned)U), dim3(kCbThreads), 0, st, logits, ldz, n_frames, (int)C, (int)blank, utt_ptr, U,
                     (int)W, class_beam, lm, hyp, hyp_len, score, status, (int4*)ws, ws_bytes / FHVAE_CB_NODE_BYTES);
  return fh_launch_status();
}
