// lstm_fwd_wr.hip -- K1 forward, two-layer H = 256 net, rows form, ONE persistent launch for all T + 1 wavefront steps, with the
// WEIGHTS REGISTER-STATIONARY (the lesson of lstm_bwd_rs.hip applied to the forward; the body the reference never wrote:
// fhvae.py:14, semantics of torch.nn.LSTM).
//
// lstm_fwd_cluster_kernel (rounds 1-2) keeps a member's 64 gate columns of W_hh^0, W_ih^1, W_hh^1 in LDS (96 KB) and lets each of
// its four waves multiply its own 32 batch rows: per k-step a wave re-reads 8 weight fragments for 16 MFMAs -- 900 KB of LDS reads
// per CU and step, 5.1 us of contraction for 1.7 us of MFMA issue -- and a wave alone on its SIMD exposes every latency.  Here:
//   * a cluster = 8 workgroups of ONE XCD (lstm_cluster_dev.h), 64 batch rows; member m owns hidden units [32m, 32m + 32) of both
//     layers; a workgroup = 512 threads = EIGHT waves, two per SIMD (256 registers each): wave w owns 4 units = one 16-column tile of
//     [4 units][i,f,g,o], for ALL 64 rows.  Its fragments of the three recurrent / inter-layer matrices (24) and of W_ih[0] (4) stay
//     in registers for the whole launch: the LDS holds activations only, and the SIMD's other wave issues MFMAs while this one
//     does gate math or waits for an LDS read;
//   * what the members exchange per step is h^0_t and h^1_{t-1} (bf16, the saved-for-backward tensors themselves), fetched by LDS-DMA
//     (L1-bypassing, whole 512-byte rows) into two LDS images; layer 0's input row [x_t | xc] (the time-constant input rides along,
//     so there is no per-row additive term) goes into a third.  Images are separate LDS objects, waits are counted;
//   * two chains with their own flags -- A: layer 0 (h^0_t needs h^0_{t-1} only), B: layer 1 -- so that a step's waits hide behind
//     the other chain's work (the step loop below); VMEM operations of a wave complete in order, so polls, image requests and stores
//     are dealt to different waves: waves 0-3 poll A and request the h^0 / x images, waves 4-7 poll B and request the h^1 image;
//   * MFMA roles swapped (weight fragment first) with the tile's 16 columns ordered [unit][gate]: a lane holds i,f,g,o of ONE unit of
//     ONE row per tile -- the gate math never leaves registers; its results are staged in LDS in the layout they leave in and
//     stored by the whole workgroup as 16-byte pieces of whole lines: h (bf16, what the other members wait for) at once, c (f32),
//     the activated gates (UNIT-MAJOR: [row][unit][i,f,g,o] bf16; ClFwd::gates_um / ClBwd::gates_um) and the f32 copies of h a
//     step later, when their acknowledgements can no longer hold up an image wait.
// Hand-off protocol, XCD placement, bounded spins: lstm_cluster_dev.h / lstm_cluster.hip.
#include <cstdlib>
#include <type_traits>

#include "lstm_cluster_dev.h"

#include "trace.h"

namespace fh {

constexpr int kFwH = 256, kFwG = 4 * kFwH, kFwHU = 32, kFwNU = 8, kFwThreads = 512;
typedef void __attribute__((address_space(3))) * fw_lds_p;

// LDS-DMA of an activation image, NP consecutive 1-KB pieces per requesting wave: buffer form, so that the per-lane part of the address
// is a 32-bit offset that does NOT change from step to step (one register per piece, computed once) while the step's slab is the
// scalar offset.  (With 64-bit per-lane pointers hipcc hoisted the step-invariant halves of 20 addresses out of the step loop,
// spilled them, and reloaded each behind an s_waitcnt vmcnt(0) between two DMA instructions.)
//   h image: [rows][32 chunks]: one piece = 2 rows x 512 B; the per-lane SOURCE chunk carries the XOR swizzle (chunk ^ (row & 15)) the
//   fragment reads undo (guide rule 21); rows past `rlast` are clamped (their results are never stored)
template <int NP>
__device__ __forceinline__ void fw_h_offsets(unsigned (&voff)[NP], int r0, int rlast, int piece0, int lane) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int rw = (piece0 + i) * 2 + (lane >> 5), rg = r0 + rw;
    voff[i] = (unsigned)(rg < rlast ? rg : rlast) * (kFwH * 2) + (unsigned)(((lane & 31) ^ (rw & 15)) << 4);
  }
}
// L1-bypassing (sc1): the rows were written by other CUs of this XCD
template <int NP>
__device__ __forceinline__ void fw_dma_h(char* img, __amdgpu_buffer_rsrc_t rs, const unsigned (&voff)[NP], unsigned slab_bytes, int piece0) {
#pragma unroll
  for (int i = 0; i < NP; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (fw_lds_p)(img + (piece0 + i) * 1024), 16, voff[i], slab_bytes, 0, kSc1);
}
//   layer 0's input image: row = [x_t (I) | xc (Ic) | padding] bf16 in 256 bytes (16 chunks), one piece = 4 rows.  The x_t chunks are
//   rewritten every step (lanes of other chunks are masked off: an LDS-DMA lane writes its own 16 bytes); the time-constant xc chunks
//   and the padding (finite data against zero weight fragments) are written once (fw_dma_xc)
template <int NP>
__device__ __forceinline__ void fw_x_offsets(unsigned (&voff)[NP], int I, int r0, int rlast, int piece0, int lane) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int rw = (piece0 + i) * 4 + (lane >> 4), rg = r0 + rw;
    voff[i] = (unsigned)(rg < rlast ? rg : rlast) * (unsigned)(I * 2) + (unsigned)(((lane & 15) ^ (rw & 15)) << 4);
  }
}
template <int NP>
__device__ __forceinline__ void fw_dma_x(char* img, __amdgpu_buffer_rsrc_t rs, const unsigned (&voff)[NP], unsigned slab_bytes, int nchx, int piece0,
                                         int lane) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int rw = (piece0 + i) * 4 + (lane >> 4);
    if (((lane & 15) ^ (rw & 15)) < nchx)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (fw_lds_p)(img + (piece0 + i) * 1024), 16, voff[i], slab_bytes, 0, 0);
  }
}
template <int NP>
__device__ __forceinline__ void fw_dma_xc(char* img, const u16* xc, int Ic, const u16* pad, int nchx, int r0, int rlast, int piece0, int lane) {
  const int nchc = Ic >> 3;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int rw = (piece0 + i) * 4 + (lane >> 4), rg = r0 + rw;
    const int64_t rc = rg < rlast ? rg : rlast;
    const int c = (lane & 15) ^ (rw & 15);
    if (c >= nchx) {
      const u16* src = c < nchx + nchc ? xc + rc * Ic + (c - nchx) * 8 : pad;
      __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (fw_lds_p)(img + (piece0 + i) * 1024), 16, 0, 0);
    }
  }
}

template <int RT, int PDT = 4>
__global__ __launch_bounds__(kFwThreads) void lstm_fwd_wr_kernel(ClFwd p) {
  constexpr bool kSave = true;
#include "lstm_fwd_wr_body.h"
}
template <int RT, int PDT = 4>
__global__ __launch_bounds__(kFwThreads) void lstm_fwd_wr_infer_kernel(ClFwd p) {
  constexpr bool kSave = false;
#include "lstm_fwd_wr_body.h"
}

template __global__ void lstm_fwd_wr_kernel<2>(ClFwd);
template __global__ void lstm_fwd_wr_kernel<4>(ClFwd);
template __global__ void lstm_fwd_wr_infer_kernel<2>(ClFwd);
template __global__ void lstm_fwd_wr_infer_kernel<4>(ClFwd);

int cluster_fwd_wr(const ClFwd& p, hipStream_t st) {
  if ((int64_t)2 * p.T * p.B * kFwH * 2 >= (1LL << 31) || (int64_t)p.T * p.B * p.I * 2 >= (1LL << 31)) return FHVAE_ERR_LIMIT;  // 32-bit buffer offsets
  if (p.NU != kFwNU || p.Mc > 64 || p.Mc % 16 != 0 || p.pre || p.K0 != p.I + p.Ic || p.K0 <= 0 || p.K0 > 128 || (p.I % 8) || (p.Ic % 8) ||
      (p.I > 0 && !p.x) || (p.Ic > 0 && !p.xcv))
    return FHVAE_ERR_SHAPE;
  const bool save = p.gates != nullptr;  // (NULL: fhvae_lstm_seq_infer)
  if (p.Mc <= 32 && save)
    hipLaunchKernelGGL((lstm_fwd_wr_kernel<2>), dim3(kGrid), dim3(kFwThreads), 0, st, p);
  else if (save)
    hipLaunchKernelGGL((lstm_fwd_wr_kernel<4>), dim3(kGrid), dim3(kFwThreads), 0, st, p);
  else if (p.Mc <= 32)
    hipLaunchKernelGGL((lstm_fwd_wr_infer_kernel<2>), dim3(kGrid), dim3(kFwThreads), 0, st, p);
  else
    hipLaunchKernelGGL((lstm_fwd_wr_infer_kernel<4>), dim3(kGrid), dim3(kFwThreads), 0, st, p);
  return fh_launch_status();
}

}  // namespace fh
