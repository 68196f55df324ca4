// lstm_cluster.h -- persistent "cluster" form of the bf16 LSTM recurrence (lstm_cluster.hip), used by lstm.hip.
#pragma once
#include "common.h"

namespace fh {

// The first FHVAE_LSTM_SYNC_BYTES of the bf16 workspace (fhvae_lstm_desc.lp) are the kernels' sync block (u32 words):
constexpr int kSyncStatus = 0;    // 0 = ok; bit 0: a bounded spin gave up, bit 1: a workgroup could not read its XCD
constexpr int kSyncSticky = 2;    // two words: address of fhvae_lstm_desc.sticky_status (0 = none), written when the block is armed
constexpr int kSyncFlags = 64;    // + cluster * 32: one word per workgroup of the cluster = the last step it has published
// 8 arrival counters, one per XCD, at kSyncXcdCnt + XCD * kSyncXcdStride (words 2112, 2144, .. 2336, behind the flags): ticket & 31 =
// a workgroup's slot on its XCD, ticket >> 5 = the launch.  ONE 128-byte line per counter: returning atomics on one line are
// serialised at the memory side, and a launch takes 256 tickets before its first step
constexpr int kSyncXcdCnt = kSyncFlags + 64 * 32;
constexpr int kSyncXcdStride = 32;
constexpr int kSyncWordsUsed = 3072;  // the words the operand cast re-arms: flags to word 2111, tickets to 2367, the rest unused; the last
                                      // quarter of the block (from byte 12288) is the phase-clock log of the profiling tools
// The block is zeroed once per forward (by the operand-cast launch that precedes every bf16 forward); the launches that then
// share it -- forward chunks, later the backward's, however often it runs -- number themselves: every launch takes 32 tickets
// of each XCD counter, so launch n holds the tickets [32 n, 32 n + 32) and uses the flag epochs (n * kSeqEpochs, (n + 1) *
// kSeqEpochs].  Nothing is re-armed between the launches (and nothing depends on the host counting them: graph replay repeats
// the same sequence from the same zeroed block).
constexpr int kSeqEpochs = 4096;

// bf16 elements of the exchange buffer the partial-dh backward (lstm_bwd_rs.hip) needs: 2 parities x 64 clusters x 4 sources x
// 3 destinations x 4 waves x 2 row tiles x 512 B (bf16 partials)
constexpr int64_t kRsXchElems = 2LL * 64 * 4 * 3 * 4 * 2 * 256;

struct ClusterWeights {  // bf16 operand copies in the workspace
  const u16* w_ih[FHVAE_MAX_LAYERS];    // [4H, H]   (l >= 1)
  const u16* w_hh[FHVAE_MAX_LAYERS];    // [4H, H]
  const u16* w_ih_t[FHVAE_MAX_LAYERS];  // [H, 4H]   (l >= 1)
  const u16* w_hh_t[FHVAE_MAX_LAYERS];  // [H, 4H]
  u16* xch;                             // exchange buffer: 2 * L * B * 4H bf16 (lstm_cluster.hip, xch_off)
  const u16* x_fold;                    // (T,B,I) bf16 when the forward kernels do the layer-0 input projection themselves
  const u16* xc_fold;                   // (B,Ic) bf16 when the rows-form forward kernel projects the time-constant input itself
};

// The schedule of a recurrence and its variants, decided ONCE per C call from the descriptor's scalar fields, `lp != NULL`, the
// (cached) device check and the environment: every schedule switch (FHVAE_NO_CLUSTER, _NO_FOLD, _NO_XC_FOLD, _NO_FWD_WR, _NO_RS,
// _NO_DXC_FOLD, _BIG_CELLS, _NO_WGRAD, _CLUSTER_TLOG) is read in lstm_plan and nowhere else, on every call (the tests flip them
// between calls).  Forward, backward and the size queries of the C ABI all read the same fields, so what a forward saves (gates unit-major or not,
// ws_below, pre) is what the backward of the same descriptor and environment expects.
struct LstmPlan {
  int form;  // 0: one launch per wavefront step (lstm.hip); persistent (bf16, gfx950 with 256 CUs, H in {128, 256}, L <= 2, ...):
             // 1: the waves of a workgroup split the cluster's rows, 2: they split the contraction (<= 32 rows per cluster)
  bool big, big_shape;  // form 0: the large-tile cells (lstm_cell.hip) are wanted (FHVAE_BIG_CELLS = 0 / 1, else from about a
                        // workgroup per CU), and the shape meets their preconditions (what remains is 16-byte alignment)
  bool fold;            // form > 0: the forward kernels multiply x_t by W_ih[0][:, :I] themselves (I a multiple of 8, at most 128)
  bool xc_in;           // form > 0: ... and project the time-constant input themselves (no GEMM, no (B,4H) f32 round trip)
  bool bwd_rs;          // rows form at H = 256: the per-layer backward exchanges partial dh (lstm_bwd_rs.hip)
  bool fwd_wr;          // ... two layers, the inputs folded: the forward with register-stationary weights (lstm_fwd_wr.hip); it
                        // saves the gates unit-major, which the partial-dh backward then reads (gates_um of ClFwd and ClBwd)
  bool bwd_zeroes_dxc;  // the backward recurrence leaves bd->d_xc zeroed: lstm.hip's split-K contraction into it needs no zeroing launch
  bool bwd_folds_dxc;   // ... and, partial-dh backward with Ic <= 64 and T >= 2, computes d_xc itself: that contraction is not launched
  bool needs_ws_below;  // rows form, L >= 2: the layer-by-layer backward hands the from-above gradient down through bd->ws_below
  bool wgrad;           // the long weight-gradient contractions go to wgrad.hip's grouped launch
  bool tlog;            // the persistent kernels log their phase clocks into the last quarter of the sync block
  struct Geo {
    int NU, NC;     // workgroups per cluster, clusters per launch
    int64_t chunk;  // batch rows per launch (larger batches run as consecutive launches)
  } fwd, bwd;       // form > 0
};
LstmPlan lstm_plan(const fhvae_lstm_desc* d);

// the recurrence of fhvae_lstm_seq_fwd after the layer-0 input projection (d->pre filled): all T steps, all layers
int cluster_fwd(const fhvae_lstm_desc* d, const LstmPlan& pl, const ClusterWeights& w, hipStream_t st);
// the recurrence of fhvae_lstm_seq_bwd: fills dgates (and dgsum when Ic > 0)
int cluster_bwd(const fhvae_lstm_bwd_desc* bd, const LstmPlan& pl, const ClusterWeights& w, hipStream_t st);

}  // namespace fh
