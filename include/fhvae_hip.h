/*
 * fhvae_hip.h -- C ABI of libfhvae_hip.so: the MI355X (gfx950) hot path of the ScalableFHVAE
 * training step.  The reference (BurnhamG/PyTorch-ScalableFHVAE) is pure Python on stock ATen
 * CPU ops and has no FFI; every entry point below names the reference lines it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; all buffers are caller-owned DEVICE memory, dense row-major
 *     unless a leading dimension (ld*, in ELEMENTS) is given; kernels never allocate or free.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream); no internal synchronisation, no global state, re-entrant -> graph-capturable.
 *   - return value: 0 on success; FHVAE_ERR_* (<0) for argument errors detected on the host
 *     before anything is launched; a positive hipError_t if a launch failed.
 *   - dtype: FHVAE_F32 computes with exact-f32 MFMA (v_mfma_f32_16x16x4_f32) -- the parity mode;
 *     FHVAE_BF16 uses bf16 MFMA operands with f32 accumulation and f32 cell state.
 *   - "time-major" activations are (T, B, X): row index t*B + b.
 */
#ifndef FHVAE_HIP_H
#define FHVAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHVAE_ABI_VERSION 12

enum { FHVAE_F32 = 0, FHVAE_BF16 = 1 };

enum {
  FHVAE_OK = 0,
  FHVAE_ERR_NULL = -1,   /* required pointer is NULL */
  FHVAE_ERR_SHAPE = -2,  /* non-positive / inconsistent dimension */
  FHVAE_ERR_DTYPE = -3,  /* unknown dtype code */
  FHVAE_ERR_ALIGN = -4,  /* pointer / leading dimension not aligned as required */
  FHVAE_ERR_LIMIT = -5   /* size beyond what the kernels index (int32 rows/cols) */
};

#define FHVAE_MAX_LAYERS 4
/* BF16 mode: the first bytes of fhvae_lstm_desc.lp are the sync block of the persistent (cluster) recurrence kernels;
   u32 word 0 = status of the last such launch on that workspace: 0 ok, non-zero = the launch gave up (outputs invalid). */
#define FHVAE_LSTM_SYNC_BYTES 16384

int fhvae_abi_version(void);
/* human-readable text for a return code (static storage) */
const char* fhvae_strerror(int code);

/* ------------------------------------------------------------------------------------------
 * Linear layer:  y[M,N] = act(x[M,K] . w[N,K]^T + b[N])        (act = ReLU if relu != 0)
 * replaces nn.Linear / VariableLinearLayer, simple_fhvae.py:127-134, :208-213.
 * dtype selects the MFMA operand type of x and w; y (and b) are f32; y_lp (optional, may be
 * NULL) receives a copy of y in the operand dtype (for chaining bf16 layers).
 * ------------------------------------------------------------------------------------------ */
int fhvae_linear_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* b,
                     float* y, int64_t ldy, void* y_lp, int64_t M, int64_t K, int64_t N, int relu,
                     int dtype, void* stream);

/* Backward of the above.  dy[M,N] f32 is the upstream gradient; if relu != 0, `y` (the forward
 * OUTPUT) masks it (dy *= y > 0) and the masked gradient is written to `dy_masked` (M*N f32
 * workspace, required iff relu).  Produces dx[M,K] f32 (may be NULL; += if dx_accumulate), and ACCUMULATES
 * dw[N,K] += dy^T x, db[N] += colsum(dy) (either may be NULL).  x, w are f32 here (the weight
 * gradient contraction runs on exact-f32 MFMA in both modes for round 1). */
int fhvae_linear_bwd(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* y,
                     int64_t ldy, const float* dy, int64_t lddy, float* dy_masked, float* dx,
                     int64_t lddx, float* dw, int64_t lddw, float* db, int64_t M, int64_t K,
                     int64_t N, int relu, int dx_accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gaussian head + reparameterisation (K2):  mu = h.Wmu^T + bmu, logvar = h.Wlv^T + blv,
 * sample = mu + eps * exp(0.5*logvar)   -- GaussianLayer.forward, simple_fhvae.py:211-216.
 * eps is supplied by the caller (the reference draws it with randn_like, :215); eps == NULL
 * skips the sample (decoder head: x_sample is computed and never used, simple_fhvae.py:102).
 * h[M,K]; mu, logvar, sample, eps: [M,D] f32 dense.
 * ------------------------------------------------------------------------------------------ */
int fhvae_gauss_head_reparam_fwd(const void* h, int64_t ldh, const void* w_mu, const void* w_lv,
                                 const float* b_mu, const float* b_lv, const float* eps, float* mu,
                                 float* logvar, float* sample, int64_t M, int64_t K, int64_t D,
                                 int dtype, void* stream);
/* mu | logvar of a Gaussian head WITHOUT sampling (the decoder's per-frame head, simple_fhvae.py:98-103, :211-213) as ONE
 * projection over the M = T*B rows: h_lp [M,K] bf16, w_pair_lp = the two bf16 weight matrices stacked [2D,K]; out[M, 2D] f32 (row
 * stride ldo): mu in columns [0,D), logvar in [D,2D). */
int fhvae_gauss_head_pair_fwd(const void* h_lp, int64_t ldh, const void* w_pair_lp, const float* b_mu, const float* b_lv,
                              float* out, int64_t ldo, int64_t M, int64_t K, int64_t D, void* stream);
/* The stacked bf16 operands of a Gaussian head from its f32 master weights w_mu, w_lv [D,K] (nn.Linear layout,
 * simple_fhvae.py:197-198), one launch: wl_pair [2D,K] (forward: fhvae_gauss_head_pair_fwd) and wt_pair [K,ldt] =
 * [w_mu^T | w_lv^T | 0] (backward: fhvae_gauss_head_bwd_pair), ldt >= 2D. */
int fhvae_head_pair_weights(const float* w_mu, const float* w_lv, void* wl_pair, void* wt_pair, int64_t ldt,
                            int64_t D, int64_t K, void* stream);
/* sample[m,c] = out[m,c] + eps[m,c] * exp(0.5 * out[m,D+c]) on the side-by-side (mu | logvar) buffer of
 * fhvae_gauss_head_pair_fwd (simple_fhvae.py:214-216); mu / logvar (may be NULL): contiguous [M,D] copies of the two halves. */
int fhvae_gauss_reparam_pair_fwd(const float* out, int64_t ldo, const float* eps, float* sample, float* mu, float* logvar,
                                 int64_t M, int64_t D, void* stream);
/* g_lp[m, 0..D) = bf16(d_mu + d_sample), [D..2D) = bf16(d_logvar + d_sample * eps * 0.5 * exp(0.5 logvar)), [2D..ldg) = 0:
 * the upstream gradient of both linear layers of a head as one bf16 operand (any of d_mu / d_logvar / d_sample may be NULL;
 * d_sample needs eps and logvar; d_sample has row stride ld_s -- a column slice of the following net's input gradient is taken
 * as it is --, logvar has row stride ld_lv).  db_mu / db_lv [D] (may be NULL): the bias gradients, += the
 * column sums of the two halves of g_lp (nn.Linear's bias backward) from the same launch where a workgroup covers whole rows. */
int fhvae_gauss_reparam_bwd_pair(const float* d_mu, const float* d_logvar, const float* d_sample, int64_t ld_s, const float* eps,
                                 const float* logvar, int64_t ld_lv, void* g_lp, int64_t ldg, float* db_mu, float* db_lv,
                                 int64_t M, int64_t D, void* stream);
/* Backward of both linear layers of a head (nn.Linear backward at simple_fhvae.py:197-198,:210-211) from the bf16 operand
 * g_lp [M,ldg] (fhvae_gauss_reparam_bwd_pair or fhvae_elbo_bwd's d_x_pair_lp): dh[M,K] = g . [W_mu; W_lv] (OVERWRITTEN, may be
 * NULL), dw_mu / dw_lv [D,K] += g^T . h_lp (skipped when both are NULL), db_mu / db_lv [D] += column sums of g (the sum of the
 * col_sum_rows partial rows col_sum[.][2D] when given, else reduced here).  wt_pair [K,ldt] from fhvae_head_pair_weights. */
int fhvae_gauss_head_bwd_pair(const void* h_lp, int64_t ldh, const void* wt_pair, int64_t ldt, const void* g_lp, int64_t ldg,
                              const float* col_sum, int64_t col_sum_rows, float* dh, int64_t lddh, float* dw_mu, float* dw_lv, float* db_mu,
                              float* db_lv, int64_t M, int64_t K, int64_t D, void* stream);

/* Elementwise part of the head's backward: given upstream d_mu, d_logvar, d_sample (any may be
 * NULL = zero) produce the gradients w.r.t. the two linear outputs:
 *   g_mu = d_mu + d_sample ; g_lv = d_logvar + d_sample * eps * 0.5 * exp(0.5*logvar)
 * (the two linear layers' own backward is fhvae_linear_bwd). n = M*D elements. */
int fhvae_gauss_reparam_bwd(const float* d_mu, const float* d_logvar, const float* d_sample,
                            const float* eps, const float* logvar, float* g_mu, float* g_lv,
                            int64_t n, void* stream);
/* The whole backward of fhvae_gauss_head_reparam_fwd (f32 h) in four launches: g_ws[M,2D] = [g_mu | g_lv] (workspace,
 * as fhvae_gauss_reparam_bwd computes them), dh[M,K] = g_mu.W_mu + g_lv.W_lv (one two-segment contraction; NULL to
 * skip), dw_mu/dw_lv[D,K] += g^T.h (one contraction, output split), db_mu/db_lv[D] += column sums of g.
 * Replaces reparam_bwd + 2 x fhvae_linear_bwd (7 launches) -- GaussianLayer backward, simple_fhvae.py:193-216. */
int fhvae_gauss_head_bwd(const float* h, int64_t ldh, const float* w_mu, const float* w_lv,
                         const float* d_mu, const float* d_logvar, const float* d_sample,
                         const float* eps, const float* logvar, float* g_ws, float* dh, int64_t lddh,
                         float* dw_mu, float* dw_lv, float* db_mu, float* db_lv, int64_t M, int64_t K,
                         int64_t D, void* stream);
/* ------------------------------------------------------------------------------------------
 * Multi-layer LSTM over a whole segment (K1), step-fused cells: one launch per wavefront step
 * computes the 4-gate contraction on MFMA and applies sigmoid/tanh + the cell update in the
 * epilogue.  There is NO reference body (fhvae.py:14 raises NotImplementedError); semantics are
 * torch.nn.LSTM(batch_first) CPU: gate order i,f,g,o; gates = W_ih x + b_ih + W_hh h + b_hh.
 * It stands where the FC pre-encoders/decoder stand in simple_fhvae.py:160-164,186-190,240-244.
 *
 * Layer-0 input at step t is [x_t (I cols) || xc (Ic cols)]: x is time-major (T,B,I) (may be
 * NULL with I = 0), xc (B,Ic) is constant over time (may be NULL with Ic = 0); w_ih[0] is
 * [4H, I+Ic].  Layers l >= 1 take h^{l-1}_t (H cols).  All layers share H.
 * ------------------------------------------------------------------------------------------ */
typedef struct fhvae_lstm_desc {
  int32_t dtype;  /* FHVAE_F32 | FHVAE_BF16: MFMA operand type used inside */
  int32_t L;      /* layers, 1..FHVAE_MAX_LAYERS */
  int64_t B, T, I, Ic, H;
  /* inputs and parameters are ALWAYS f32 (master copies) */
  const float* x;   /* (T,B,I) time-major */
  const void* x_lp; /* BF16 mode, optional: the same x already in bf16 (e.g. from fhvae_to_time_major); then the
                       forward does not cast x again (two encoders share one input) */
  const float* xc;  /* (B,Ic) */
  const float* w_ih[FHVAE_MAX_LAYERS]; /* [4H, I+Ic] (l=0) / [4H, H] */
  const float* w_hh[FHVAE_MAX_LAYERS]; /* [4H, H] */
  const float* b_ih[FHVAE_MAX_LAYERS]; /* [4H] */
  const float* b_hh[FHVAE_MAX_LAYERS];
  /* forward outputs, saved for backward */
  void* hs;      /* (L,T,B,H) in the operand dtype (f32 or bf16): h^l_t */
  float* cs;     /* (L,T,B,H) f32: c^l_t */
  void* gates;   /* (L,T,B,4H) in the operand dtype: activated i,f,g,o.  A workspace between a forward and ITS backward: the
                    per-step cells keep column blocks of H per gate, the persistent schedules keep the four gates of a unit
                    quad together (csrc/lstm_cluster.hip, cl_goff); do not read it from outside */
  float* hn;     /* (B, L*H) f32: final hidden state of every layer, concatenated (may be NULL) */
  float* hs_top_f32; /* (T,B,H) f32 copy of the top layer's h_t (BF16 mode, may be NULL; in F32 mode
                        the top layer is hs + (L-1)*T*B*H and this must be NULL) */
  float* pre;    /* workspace (T,B,4H) f32 (I > 0) or (B,4H) (I == 0): layer-0 input projection (the persistent
                    schedules only use its first (B,4H): they multiply x_t by W_ih[0] inside the kernel; the large-tile
                    bf16 step cells of csrc/lstm_cell.hip multiply the whole layer-0 input themselves and leave it unused) */
  void* lp;      /* F32 mode: optional workspace of fhvae_lstm_lp_bytes() bytes (may be NULL): the forward leaves the
                    transposed f32 weights in it and the backward cells then stage both operands by LDS-DMA (64 -> 40 us per
                    launch at B = 2048, H = 256); without it they read the master weights as K-major operands.
                    BF16 mode: workspace of fhvae_lstm_lp_bytes() bytes; the forward fills it with bf16
                    copies of x, xc, the weights and the transposed weights, the backward reuses it.  It also
                    holds the persistent schedules' sync block (first FHVAE_LSTM_SYNC_BYTES) and their exchange
                    buffer (2*L*B*4H bf16): keep it alive and untouched between the forward and its backward */
  void* hn_lp;   /* BF16 mode, optional (may be NULL): (B, L*H) bf16 copy of hn -- the operand of a bf16 Gaussian head
                    (simple_fhvae.py:193-216) straight from the kernel that produced the final states, instead of a cast launch
                    per head and step.  Always filled when set (the persistent kernels store it with hn; the per-step schedules cast hn at the end). */
  /* BF16 mode, optional (head_w_mu == NULL: none): the Gaussian head that consumes this net's states (GaussianLayer,
     simple_fhvae.py:193-216; f32 master weights head_w_mu / head_w_lv [head_D, head_K]).  The forward's operand-cast launch then
     also writes the head's stacked bf16 operands -- head_wl [2 head_D, head_K] = [W_mu; W_lv] and head_wt [head_K, head_ldt] =
     [W_mu^T | W_lv^T | 0] (head_ldt >= 2 head_D), exactly what fhvae_head_pair_weights produces -- instead of one more launch per
     head and step. */
  const float* head_w_mu;
  const float* head_w_lv;
  void* head_wl;
  void* head_wt;
  int64_t head_D, head_K, head_ldt;
  int32_t* sticky_status; /* BF16 mode, optional (may be NULL): int32 device word that the library never clears.  A persistent
                    launch that gives up ORs its status code into it as well as into the workspace's status word (which
                    the next forward on that workspace re-arms): the failure stays visible however late the host looks. */
} fhvae_lstm_desc;

int64_t fhvae_lstm_lp_bytes(const fhvae_lstm_desc* d);
/* Floats the `pre` workspace must hold for this descriptor on the current device (evaluate with `lp` set, as for
   fhvae_lstm_form): (T,B,4H) for the per-step cells of gemm_core.h with a per-frame input, (B,4H) for the persistent
   schedules (they multiply x_t inside the kernel), 1 for the large-tile bf16 cells (csrc/lstm_cell.hip: the whole layer-0
   input projection is theirs; they then REQUIRE 16-byte aligned buffers: the forward returns FHVAE_ERR_ALIGN instead of
   falling back to a schedule that would need the full buffer).  `pre` must still be non-NULL. */
int64_t fhvae_lstm_pre_elems(const fhvae_lstm_desc* d);
/* Identifies the layout of what fhvae_lstm_seq_fwd saves for the backward (gates, schedule workspaces): it follows from the
 * schedule the library picks for this descriptor AND the FHVAE_* environment switches at call time.  A caller that may change
 * either between a forward and its backward keeps the forward's value and checks it before fhvae_lstm_seq_bwd (< 0: bad
 * descriptor; `gates` and `cs` are not looked at). */
int fhvae_lstm_layout_id(const fhvae_lstm_desc* d);

/* Floats fhvae_lstm_bwd_desc.ws_below must hold (0: may be NULL). */
int64_t fhvae_lstm_ws_below_elems(const fhvae_lstm_desc* d);
/* Which schedule fhvae_lstm_seq_fwd/_bwd take for this descriptor on the current device: 0 = one launch per wavefront
   step; 1 = persistent cluster kernel, waves split the batch rows; 2 = persistent cluster kernel, waves split the
   contraction (small batches).  1 and 2 need the GPU to themselves while they run (256 co-resident workgroups);
   FHVAE_NO_CLUSTER=1 in the environment forces 0.  `gates` and `cs` are not looked at (fhvae_lstm_seq_infer takes the same form). */
int fhvae_lstm_form(const fhvae_lstm_desc* d);
int fhvae_lstm_seq_fwd(const fhvae_lstm_desc* d, void* stream);
/* Inference forward: same descriptor as fhvae_lstm_seq_fwd, same schedule choice, same outputs (hs, hn, hn_lp, hs_top_f32,
   head_wl/head_wt), bit-identical values.  `gates` must be NULL (else FHVAE_ERR_SHAPE).  `cs` is a workspace of
   fhvae_lstm_infer_cs_elems(d) floats (may be NULL when that is 0): the per-step schedules keep c^l_{t-1} in a two-slot ring
   (L,2,B,H), the persistent ones keep c in registers / LDS and return 0.  hs stays (L,T,B,H): it is the inter-layer input and the
   persistent kernels' exchange buffer.  F32 mode: `lp` may be NULL and is not filled.  BF16 mode: `lp` is the same workspace (the
   transposed weight copies are not made).  No fhvae_lstm_seq_bwd may follow. */
int64_t fhvae_lstm_infer_cs_elems(const fhvae_lstm_desc* d);
int fhvae_lstm_seq_infer(const fhvae_lstm_desc* d, void* stream);

typedef struct fhvae_lstm_bwd_desc {
  fhvae_lstm_desc f;      /* the forward descriptor (same buffers, already filled by fwd) */
  const float* d_hs_top;  /* (T,B,H) f32 gradient w.r.t. the top layer's h_t (may be NULL) */
  const float* d_hn;      /* (B, L*H) f32 gradient w.r.t. hn (may be NULL) */
  /* workspaces */
  void* dgates;   /* (L,T,B,4H) operand dtype: gradient w.r.t. pre-activation gates */
  float* dgsum;   /* (B,4H) f32: sum_t dgates of layer 0 (required iff Ic > 0) */
  float* dc;      /* (L,B,H) f32: running cell-state gradient */
  /* outputs, f32 (ACCUMULATED: += ; any may be NULL) */
  float* dw_ih[FHVAE_MAX_LAYERS];
  float* dw_hh[FHVAE_MAX_LAYERS];
  float* db_ih[FHVAE_MAX_LAYERS];
  float* db_hh[FHVAE_MAX_LAYERS];
  float* d_xc;    /* (B,Ic) f32, OVERWRITTEN (may be NULL) */
  int32_t phase;  /* 0: everything; 1: the recurrence (dgates, dgsum, d_xc) only; 2: the weight/bias gradient
                     contractions only (reads what phase 1 left in dgates/dgsum) -- lets the host put phase 2 on a
                     second stream, under the next net's latency-bound recurrence */
  float* ws_below; /* (T,B,H) f32 workspace, required when fhvae_lstm_ws_below_elems(&f) > 0 (persistent backward, layer by
                      layer, H != 256: the from-above gradient dg^{l+1}.W_ih^{l+1} reaches the lower layer through it;
                      at H = 256 the lower layer's launch computes that term itself) */
} fhvae_lstm_bwd_desc;

int fhvae_lstm_seq_bwd(const fhvae_lstm_bwd_desc* d, void* stream);
/* Phase 2 of n backward passes at once (their phase 1 must have been enqueued on `stream` before): the weight / bias
 * gradients of several nets.  In BF16 mode the long contractions dW[4H,.] += dgates^T . [x | h] over the T*B rows of ALL the
 * descriptors run as ONE grouped launch (csrc/wgrad.hip); the host defers them to the end of the backward pass, where the
 * three nets of the model together fill the chip with whole tiles and few K slices. */
/* `extra` (may be NULL with n_extra = 0): further contractions C[M,N] += A[K,M]^T . B[K,N] of the same kind (the heads' weight
 * gradients) that ride in the same grouped launch; each must satisfy fhvae_wgrad_desc_ok. */
typedef struct fhvae_wgrad_desc {
  const void* a; int64_t lda;  /* [K, lda] bf16: the contraction index is the ROW */
  int64_t a_col0;              /* `a` points a_col0 columns into the rows of its buffer (a column slice) */
  const void* b; int64_t ldb;  /* [K, ldb] bf16 */
  float* c; int64_t ldc;       /* [M, ldc] f32, accumulated */
  int64_t M, N, K;
} fhvae_wgrad_desc;
int fhvae_wgrad_desc_ok(const fhvae_wgrad_desc* p); /* 1 = the grouped kernel takes it (alignment, ranges), else 0 */
int fhvae_lstm_param_grads_multi(const fhvae_lstm_bwd_desc* const* descs, int n, const fhvae_wgrad_desc* extra, int n_extra,
                                 void* stream);
/* The contraction itself: C[M,N] (f32, ldc) += A[K,M]^T . B[K,N], bf16 operands whose ROW index is the contraction index
 * (lda, ldb in elements, multiples of 8; 16-byte aligned bases; K*ld*2 < 2^30) -- dW += dY^T X of a linear / LSTM layer over
 * K = batch x time rows (autograd of nn.Linear, simple_fhvae.py:127-134; of the LSTM body missing at fhvae.py:14).
 * FHVAE_ERR_ALIGN when the preconditions do not hold. */
int fhvae_wgrad_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, float* c, int64_t ldc, int64_t M,
                     int64_t N, int64_t K, void* stream);
/* The same contraction with f32 operands on exact-f32 MFMA (the parity mode's weight gradients; lda, ldb multiples of 4,
 * K*ld*4 < 2^31). */
int fhvae_wgrad_f32(const float* a, int64_t lda, const float* b, int64_t ldb, float* c, int64_t ldc, int64_t M, int64_t N,
                    int64_t K, void* stream);

/* c[M,N] (f32, ldc) = a[M,K] . b[N,K]^T (+ bias[N], may be NULL): bf16 operands with the contraction index CONTIGUOUS in both
 * (lda, ldb in elements, multiples of 8; K % 64 == 0, N % 4 == 0; 16-byte aligned bases; M*lda*2 < 2^31) -- an activation matrix
 * over M = batch x time rows times a weight matrix as nn.Linear / nn.LSTM store it (y = x W^T, simple_fhvae.py:130; for the LSTM
 * body missing at fhvae.py:14: the from-above term dh^l += dgates^{l+1} . W_ih^{l+1} of the backward, for all time steps at
 * once).  One tile per CU, every row of `a` read once (csrc/proj.hip).  FHVAE_ERR_ALIGN when the preconditions do not hold. */
int fhvae_proj_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, const float* bias, float* c, int64_t ldc,
                    int64_t M, int64_t N, int64_t K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Launch plans of the three matrix-product kernels: what fhvae_proj_bf16, the weight-gradient entries and the generic engine
 * behind the linear layers would launch for the given sizes.  Host only: no stream, nothing is launched, and the pointers of
 * the descriptors are looked at for alignment and equality only (never dereferenced).  Each fills caller-provided plans and
 * returns the number of launches (< 0: the error the entry point would return before its first launch).  These ARE the
 * functions the launchers call (csrc/proj.hip, csrc/wgrad.hip, csrc/gemm.hip), not a description of them.
 * ------------------------------------------------------------------------------------------ */
typedef struct fhvae_proj_plan {
  int32_t BM, BN, tiles; /* proj_kernel<BM, BN> on tiles = ceil(M / BM) * ceil(N / BN) workgroups */
} fhvae_proj_plan;
int fhvae_plan_proj(int64_t M, int64_t N, fhvae_proj_plan* out);

#define FHVAE_WGRAD_MAX_PROBLEMS 16
typedef struct fhvae_wgrad_plan {
  int32_t BN, sk, grid, n; /* wgrad_kernel<., BN> on `grid` workgroups over n problems; sk: the cost model's K slices */
  struct {
    int32_t which; /* index of the problem in the call */
    int32_t m_tiles, n_tiles, ksteps_per, splitk, shared_c;
  } p[FHVAE_WGRAD_MAX_PROBLEMS];
} fhvae_wgrad_plan;
/* the launches of n problems of one dtype in launch order: the problems with N > 128 in chunks of 16, then the others.
 * FHVAE_ERR_ALIGN if a problem is not eligible, FHVAE_ERR_LIMIT beyond 256 problems or `cap` launches. */
int fhvae_plan_wgrad(const fhvae_wgrad_desc* x, int n, int dtype, fhvae_wgrad_plan* out, int cap);

#define FHVAE_GEMM_MAX_GROUP 4
typedef struct fhvae_gemm_desc { /* one problem C[M,N] = sum over two K segments of A . B^T, as the generic engine sees it */
  const void* a[2]; const void* b[2]; int64_t lda[2], ldb[2];
  const void* c; const void* c2; const void* clp; int64_t ldc, ldclp; /* f32 output(s), bf16 copy (any may be NULL) */
  int32_t M, N, K[2], a_kc[2], b_kc[2]; /* K[s] = 0: segment unused; *_kc: 1 = the contraction index is contiguous */
  int32_t splitk, mode;                 /* on entry: K slices (0 = choose, needs mode 1); 0 store, 1 add, 2 atomic add */
} fhvae_gemm_desc;
enum { FHVAE_GEMM_SLOW = 0, FHVAE_GEMM_PLAIN, FHVAE_GEMM_SWAP, FHVAE_GEMM_SWAP_DMA, FHVAE_GEMM_LONGK, FHVAE_GEMM_GROUP,
       FHVAE_GEMM_GROUP_ONCE };
typedef struct fhvae_gemm_plan { /* one launch */
  int32_t first, n; /* problems [first, first + n) of the call; n > 1: one grouped launch */
  int32_t status;   /* != 0: this problem's launch returns that error (the launches before it have gone out) */
  int32_t variant;  /* FHVAE_GEMM_*: scalar fallback; unswapped kernel; swapped epilogue; ... with the LDS-DMA main loop; the
                       long-K 128x64 bf16 tile; grouped; grouped with every output written once (swapped epilogue) */
  int32_t BM, BN, CH, akc, bkc; /* tile, 16-byte chunks per panel row, orientation (0 for the scalar fallback) */
  uint32_t grid[3];
  int32_t splitk[FHVAE_GEMM_MAX_GROUP], mode[FHVAE_GEMM_MAX_GROUP]; /* resolved, per problem of the launch */
} fhvae_gemm_plan;
/* n problems of one call (fhvae_gauss_head_reparam_fwd makes 2): one grouped launch or one launch each; out holds n plans */
int fhvae_plan_gemm(const fhvae_gemm_desc* d, int n, int dtype, fhvae_gemm_plan* out);

/* ------------------------------------------------------------------------------------------
 * mu2 gather (K4): mu2[b,:] = table[idx[b],:]  -- torch.gather, simple_fhvae.py:53.
 * bwd: dtable[idx[b],:] += scale * dmu2[b,:] (float atomics; duplicate indices accumulate; rows
 * outside [0,S) are skipped, which is how a row shard ignores other shards' rows).
 * fwd/bwd take idx RELATIVE to the table passed (a shard passes idx - row0 via `idx_offset`).
 * idx is int64 (DataLoader collate, train_model.py:445); rows outside [0,S) -> error flag:
 * the kernel writes zeros for them and sets *oob_flag (int32 device word, may be NULL).
 * ------------------------------------------------------------------------------------------ */
int fhvae_mu2_gather_fwd(const float* table, const int64_t* idx, int64_t idx_offset, float* mu2,
                         int64_t B, int64_t S, int64_t D, int32_t* oob_flag, void* stream);
int fhvae_mu2_gather_bwd(const float* dmu2, const int64_t* idx, int64_t idx_offset, float* dtable,
                         int64_t B, int64_t S, int64_t D, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused variational lower bound (K3) -- simple_fhvae.py:105-116 with log_gauss :56-60, kld :62-69.
 *   log_pmu2   = sum_d logN(mu2; 0, 1)
 *   neg_kld_z2 = -sum_d KL(N(z2_mu, e^z2_lv) || N(mu2, 0.25))
 *   neg_kld_z1 = -sum_d KL(N(z1_mu, e^z1_lv) || N(0, 1))
 *   log_px_z   = sum_{t,f} logN(x; x_mu, e^x_lv)
 *   lower_bound = log_px_z + neg_kld_z1 + neg_kld_z2 + log_pmu2 / num_segs
 * x, x_mu, x_lv are addressed as base + b*sb + t*st + f (f contiguous) so that both the
 * batch-major (B,T,F) layout of the reference and the time-major (T,B,F) layout of the LSTM
 * decoder are read in place.  num_segs is int64 (B,) or NULL with nsegs_scalar used instead.
 * ------------------------------------------------------------------------------------------ */
typedef struct fhvae_elbo_desc {
  int64_t B, T, F, D1, D2;
  const float* x;    int64_t x_sb, x_st;
  const float* x_mu; const float* x_lv; int64_t xo_sb, xo_st; /* shared strides of x_mu/x_lv */
  const float* z1_mu; const float* z1_lv;  /* (B,D1) */
  const float* z2_mu; const float* z2_lv;  /* (B,D2) */
  const float* mu2;                        /* (B,D2) */
  const int64_t* num_segs; double nsegs_scalar;
  /* outputs (B,) f32 */
  float* lower_bound; float* log_px_z; float* neg_kld_z1; float* neg_kld_z2; float* log_pmu2;
} fhvae_elbo_desc;

int fhvae_elbo_fwd(const fhvae_elbo_desc* d, void* stream);

typedef struct fhvae_elbo_bwd_desc {
  fhvae_elbo_desc f;
  /* upstream gradients, (B,) f32, any may be NULL (= 0): */
  const float* g_lower_bound; const float* g_log_px_z; const float* g_neg_kld_z1;
  const float* g_neg_kld_z2; const float* g_log_pmu2;
  int32_t reference_detach;  /* 1: no gradient into x_mu/x_lv and none from log_pmu2 into mu2
                                (the .detach() calls at simple_fhvae.py:107,114) */
  /* outputs, OVERWRITTEN; same layouts as the forward inputs; d_x_mu/d_x_lv may be NULL */
  float* d_x_mu; float* d_x_lv;
  float* d_z1_mu; float* d_z1_lv; float* d_z2_mu; float* d_z2_lv; float* d_mu2;
  /* optional (NULL = off; needs d_x_mu / d_x_lv, F % 4 == 0, F <= 256, 16-byte aligned buffers and time-major rows
     r = t*B + b): the decoder-output gradients once more as ONE bf16 matrix, the operand of the per-frame head's backward
     contractions (fhvae_gauss_head_bwd_pair): d_x_pair_lp[r*ld_pair + 0..F) = d_x_mu, [F..2F) = d_x_lv, [2F..ld_pair) = 0,
     and partial column sums of them, d_x_colsum[fhvae_elbo_colsum_rows(B)][2F] (OVERWRITTEN; the sum over its rows = the
     head's bias gradients) */
  void* d_x_pair_lp; int64_t ld_pair; float* d_x_colsum;
} fhvae_elbo_bwd_desc;

int fhvae_elbo_bwd(const fhvae_elbo_bwd_desc* d, void* stream);
int64_t fhvae_elbo_colsum_rows(int64_t B);

/* ------------------------------------------------------------------------------------------
 * Discriminative loss (K5): logits[b,s] = -sum_d (q[b,d]-table[s,d])^2 * inv_two_var,
 * log-sum-exp over s, cross-entropy against idx  -- simple_fhvae.py:119-122 (the reference
 * materialises (B,S,D) three times; here the table is streamed once per 256-query tile with an
 * online max-subtracted log-sum-exp and nothing of size B*S is ever written).
 *
 * fwd writes per-query partials so that a row-sharded table can be combined across GPUs:
 *   row_max[b], row_sumexp[b] over THIS table's rows, tgt_logit[b] = logit at row idx[b]-row0
 *   (0 if that row is not in [row0, row0+S)), and, if ce_mean != NULL, the single-shard scalar
 *   ce_mean = ce_scale * mean_b( (row_max - tgt_logit) + log(row_sumexp) )  (ce_scale = 1: the reference's log_qy,
 *   simple_fhvae.py:122; -1: the intended objective's -CE without a negation launch each way).
 * ws: workspace of fhvae_disc_lse_ws_bytes(B,S) bytes.
 * dtype (fwd and bwd; q, table and every output stay f32): FHVAE_F32 = the logits in exact f32 (direct form on the VALU, or
 * the expanded form on exact-f32 MFMA for D = 32 and B*S >= 65536) -- the parity mode; FHVAE_BF16 (D = 32 large problems
 * only, otherwise as F32) = the bf16 compute mode: cross terms on bf16 MFMA with hi/lo-split operands (~2^-16 relative on
 * q.t).  In both MFMA forms the query's own row (idx) is taken in the direct f32 form.
 * ------------------------------------------------------------------------------------------ */
int64_t fhvae_disc_lse_ws_bytes(int64_t B, int64_t S);
int fhvae_disc_lse_fwd(const float* q, const float* table, const int64_t* idx, int64_t row0,
                       float inv_two_var, float* row_max, float* row_sumexp, float* tgt_logit,
                       float* ce_mean, float ce_scale, void* ws, int64_t B, int64_t S, int64_t D, int dtype, void* stream);
/* Helpers of the row-sharded table's exchange (the reference has no distributed code): one launch each.
 * pack / unpack: [q[b, 0..D) | int32 bits of idx[b]] rows of D+1 floats -- queries and row indices travel in one all-gather.
 * merge_partials: the W ranks' K5 partials, parts[w] = [row_max | row_sumexp | tgt_logit] of N queries each, merged into the
 *   global (row_max, row_sumexp, tgt_logit): max, sum of sumexp_w * exp(max_w - max), sum (log-sum-exp of simple_fhvae.py:122).
 * bwd_pack / bwd_unpack: the backward's single all-reduce buffer, N x 2D: [dq_all * dq_scale | dmu2 of the n_own local queries
 *   from row own0 on, zeros elsewhere]; unpack returns the local queries' dq and every query's dmu2 (either may be NULL). */
int fhvae_shard_pack(const float* q, const int64_t* idx, float* out, int64_t B, int64_t D, void* stream);
int fhvae_shard_unpack(const float* packed, float* q, int64_t* idx, int64_t N, int64_t D, void* stream);
int fhvae_disc_merge_partials(const float* parts, float* row_max, float* row_sumexp, float* tgt_logit, int64_t W, int64_t N,
                              void* stream);
int fhvae_shard_bwd_pack(const float* dq_all, float dq_scale, const float* dmu2_local, int64_t own0, int64_t n_own, float* out,
                         int64_t N, int64_t D, void* stream);
int fhvae_shard_bwd_unpack(const float* buf, int64_t own0, int64_t n_own, float* dq_local, float* dmu2_all, int64_t N, int64_t D,
                           void* stream);
int fhvae_disc_ce_mean(const float* row_max, const float* row_sumexp, const float* tgt_logit,
                       float* ce_mean, float ce_scale, int64_t B, void* stream);

/* bwd: given the GLOBAL (all shards combined) row_max[b] and row_sumexp[b] and the scalar scale
 * g = (*g_scale) * g_mul  (= dL/d(ce_mean) / B_total), computes  p[b,s] = exp(logit - row_max[b]) / row_sumexp[b]
 * (kept as max and sum, not as one log-sum-exp: |max| ~ 1e3 would put its ulp into every p),
 * w = g*(p - [s == idx[b]-row0])
 *   dq[b,:]     = sum_s w * (-2 c)(q[b]-t[s])      OVERWRITTEN  (partial over this shard's rows)
 *   dtable[s,:] += sum_b w * (+2 c)(q[b]-t[s])     ACCUMULATED
 * g is read from device memory (g_scale, one f32) so the call stays graph-capturable.
 * ws / ws_bytes: workspace (16-byte aligned) or NULL / 0.  With it (and dq and dtable both wanted) the kernels that have a one-pass
 * form take both gradients from ONE recomputation of the logits; without it, one pass per gradient.  The one-pass form keeps
 * (B/256) x S x (D+1) floats of partial sums: fhvae_disc_lse_bwd_ws_bytes(B,S,D) is the RECOMMENDED size, capped at 1.5 GiB (the
 * partials of B = 16384 queries against 10^6 rows would be 8.4 GB); with fewer bytes than the whole problem needs the queries
 * are processed in groups of as many 256-query tiles as fit (any size from one tile's partials up works; below that the
 * call takes the two-pass form).  0 from the size function = no one-pass form for this shape. */
int64_t fhvae_disc_lse_bwd_ws_bytes(int64_t B, int64_t S, int64_t D);
int fhvae_disc_lse_bwd(const float* q, const float* table, const int64_t* idx, int64_t row0,
                       float inv_two_var, const float* row_max, const float* row_sumexp,
                       const float* g_scale, float g_mul, float* dq, float* dtable, void* ws, int64_t ws_bytes,
                       int64_t B, int64_t S, int64_t D, int dtype, void* stream);

/* The discriminative segment variational lower bound, train_model.py:243-251:
 *   loss = -mean_b(lower_bound[b] + alpha * log_qy) = -(mean(lower_bound) + alpha * log_qy)   (log_qy one f32 on the device)
 * and its backward d_lower_bound[b] = -g/B, d_log_qy = -alpha*g (g = *g_loss, NULL = 1): one launch each instead of the
 * ~10 elementwise/reduction launches of the expression.  nan_flag (optional int32 device word, never cleared here): bit 0 is
 * set when mean(lower_bound) is NaN -- the loop's divergence test `torch.isnan(lower_bound).any()` (train_model.py:464-466)
 * without a host synchronisation per batch; the host reads it once per epoch. */
int fhvae_loss_fwd(const float* lower_bound, const float* log_qy, float alpha, float* loss, int64_t B,
                   int32_t* nan_flag, void* stream);
int fhvae_loss_bwd(const float* g_loss, float alpha, float* d_lower_bound, float* d_log_qy, int64_t B,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Adam (train_model.py:409-411: torch.optim.Adam(lr, betas=(beta_one, beta_two)), eps 1e-8, no
 * weight decay) over one flat f32 buffer; step_count is read from device memory (int32; already
 * incremented by the caller unless FHVAE_ADAM_ADVANCE) so a captured graph advances the bias correction.  p_lp (optional)
 * receives the updated parameters in bf16.  grad_scale multiplies g first (1/world for DP).
 * ------------------------------------------------------------------------------------------ */
int fhvae_adam_step(float* p, float* g, float* m, float* v, void* p_lp, int64_t n, float lr,
                    float beta1, float beta2, float eps, float grad_scale, int flags, int32_t* step_count,
                    void* stream);
#define FHVAE_ADAM_ZERO_GRAD 1 /* g is cleared behind its use: the next backward accumulates into zeros, no memset launch */
#define FHVAE_ADAM_ADVANCE 2   /* the launch counts the step itself: it uses step_count[0] + 1 and stores it; the words behind
                                  it are its arrival counters (one per 128-byte line, zero between launches): step_count is
                                  int32[FHVAE_ADAM_STEP_WORDS], 128-byte aligned -- no increment launch in front of it */
#define FHVAE_ADAM_STEP_WORDS (65 * 32)

/* ------------------------------------------------------------------------------------------
 * Measurement aid (bench.py roofline leg; no reference counterpart): while enabled, every step-cell launch
 * of fhvae_lstm_seq_fwd/bwd is bracketed by two HIP events on its stream and tagged with its kind
 * (0 = forward cell, 1 = backward cell) and its algorithmic FLOPs.  fhvae_trace_collect synchronises on
 * the recorded events, returns the number of records copied (host arrays, any may be NULL) and clears the
 * trace.  Off by default; the only process-global state of the library; not for use under graph capture.
 * ------------------------------------------------------------------------------------------ */
int fhvae_trace_enable(int on);
int64_t fhvae_trace_collect(float* ms, int32_t* kind, double* flops, int64_t cap);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8f "next" #1 -- segment sampler over an utterance pool resident in HBM.
 * pool: (pool_frames, F) f32, all utterances of a split concatenated (288 GB of HBM hold ~900 M frames of
 * 80-bin features); start[b]: absolute first frame of segment b in the pool (= utterance offset + seg.start,
 * datasets.py:155-185).  Writes the (B,T,F) batch-major batch the reference's DataLoader would collate
 * (datasets.py:214-223) and/or its time-major (T,B,F) form, with (x - mean) * inv_std applied per feature
 * when mean/inv_std are given (apply_mvn, datasets.py:100-105).  Frames outside the pool read as 0 and set
 * *oob_flag (int32 device word, may be NULL).
 * ------------------------------------------------------------------------------------------ */
int fhvae_segment_gather(const float* pool, int64_t pool_frames, const int64_t* start, const float* mean,
                         const float* inv_std, float* out_btf, float* out_tbf, int64_t B, int64_t T,
                         int64_t F, int32_t* oob_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * SURVEY 8f "next" #2 -- closed-form mu2 estimate (utils.estimate_mu2_dict, utils.py:45-60):
 *   mu2[y] = sum_{segments n with idx[n] == y} z2_mu[n] / (count[y] + ratio),  ratio = exp(pz2_logvar)/exp(pmu2_logvar)
 * accumulate: zsum[idx[n],:] += z2_mu[n,:], count[idx[n]] += 1 (float atomics; call once per batch, buffers
 * zeroed by the caller); finalize: mu2 = zsum / (count + ratio), 0 for sequences without segments.
 * ------------------------------------------------------------------------------------------ */
int fhvae_mu2_accumulate(const float* z2_mu, const int64_t* idx, float* zsum, float* count, int64_t N,
                         int64_t S, int64_t D, void* stream);
int fhvae_mu2_finalize(const float* zsum, const float* count, float* mu2, int64_t S, int64_t D,
                       float ratio, void* stream);

/* ------------------------------------------------------------------------------------------
 * Hierarchical sampling (Hsu & Glass 2018; csrc/hs.hip): training works through blocks of K sequences whose mu2 rows are
 * set in closed form from the current encoder before the block starts.  Data-dependent errors set bits of the int32 device
 * word `status` (never cleared by the library; the host reads it once per block); host-visible argument errors return
 * FHVAE_ERR_*.
 * select: seq_ptr (S+1) is the CSR over sequences of a segment pool grouped by sequence; block_seqs (K) the block's
 *   sequence ids.  Writes the block's segments in block order, then segment order: seg_ids[o] = seq_ptr[s] + j and
 *   local_idx[o] = position of s in block_seqs, for o < cap; *n_out = the total (also when it exceeds cap).  An id outside
 *   [0, S) counts as 0 segments and sets FHVAE_HS_BAD_SEQ; a total above cap sets FHVAE_HS_CAP.
 * accumulate_sorted: zsum[local_idx[n],:] += z2_mu[n,:], count[local_idx[n]] += 1 for local_idx non-decreasing within the
 *   call, without float atomics: bitwise reproducible for a fixed chunking.  A sequence may continue across calls (its
 *   partial sum is carried in zsum).  An index outside [0, K) sets FHVAE_HS_BAD_IDX, a decreasing one FHVAE_HS_UNSORTED;
 *   either makes the call (and every later call with that status word) add nothing.  D <= 256.
 * load_table: table = zsum / (count + ratio) (0 where count is 0), m_rows = v_rows = 0 (the table's slice of the Adam
 *   moments), then zsum = count = 0; one launch.
 * ------------------------------------------------------------------------------------------ */
#define FHVAE_HS_BAD_SEQ 1
#define FHVAE_HS_CAP 2
#define FHVAE_HS_BAD_IDX 4
#define FHVAE_HS_UNSORTED 8
int fhvae_hs_select(const int64_t* seq_ptr, int64_t S, const int64_t* block_seqs, int64_t K, int64_t* seg_ids,
                    int64_t* local_idx, int64_t* n_out, int64_t cap, int32_t* status, void* stream);
int fhvae_mu2_accumulate_sorted(const float* z2_mu, const int64_t* local_idx, float* zsum, float* count, int64_t N,
                                int64_t K, int64_t D, int32_t* status, void* stream);
int fhvae_mu2_load_table(float* zsum, float* count, float* table, float* m_rows, float* v_rows, int64_t K, int64_t D,
                         float ratio, void* stream);
/* Across W ranks (rank r owns rows [row0, row1) of the K-row table; every rank accumulates part of the block's segments):
 * hs_pack_partials: out (K, D+1) = [zsum | count], then zsum = count = 0; one launch.
 * mu2_merge_load_shard: parts (W, K, D+1) are the W ranks' packed partials in rank order.  For the rows in [row0, row1):
 *   sum = parts[0] + parts[1] + ... + parts[W-1] (added in that order, the count column the same way),
 *   shard[k - row0] = sum / (count + ratio) (0 where count is 0), m_rows = v_rows = 0 (the shard's slice of the Adam moments,
 *   (row1 - row0, D)); one launch, none for an empty shard (row0 == row1).  0 <= row0 <= row1 <= K. */
int fhvae_hs_pack_partials(float* zsum, float* count, float* out, int64_t K, int64_t D, void* stream);
int fhvae_mu2_merge_load_shard(const float* parts, int64_t W, int64_t K, int64_t row0, int64_t row1, float* shard,
                               float* m_rows, float* v_rows, int64_t D, float ratio, void* stream);

/* ------------------------------------------------------------------------------------------
 * Features from audio (csrc/feats.hip): the reference's prepare_numpy_data.generate_feat (prepare_numpy_data.py:14-46) on
 * AudioUtils.stft / rstft / to_melspec (utils.py:155-272, librosa 0.8.0), for a batch of U utterances in one launch.
 *   wave (n_samples) f32: the utterances' samples, concatenated; wave_ptr (U+1) int64 their offsets.
 *   frame_ptr (U+1) int64: output row offsets, frame_ptr[u+1] - frame_ptr[u] = 1 + (L + 2*(n_fft/2) - n_fft) / hop for an
 *     utterance of L >= n_fft/2 + 1 samples; frame_ptr[0] = 0, frame_ptr[U] = n_frames.
 *   Per frame: pre-emphasis y[t] - 0.97 y[t-1] (y[-1] = 0), centre padding of n_fft/2 by reflection (edge not repeated),
 *   S = |DFT(window * frame)| over bins 0 .. n_fft/2; SPEC: out (n_frames, n_fft/2+1) = max(ln S, -50); FBANK: out
 *   (n_frames, n_mels) = max(ln(S . mel^T), -20).
 *   dft_basis (32*G, KP) f32, KP = n_fft rounded up to 16, G = ceil((n_fft/2+1) / 16): row 32g + i holds w[n] cos(2 pi n b / n_fft)
 *     and row 32g + 16 + i holds -w[n] sin(2 pi n b / n_fft) for bin b = 16g + i, n < n_fft (zero for b > n_fft/2 and n >= n_fft).
 *   mel_basis (16*ceil(n_mels/16), 16*G) f32 (FBANK only, NULL for SPEC): row j = mel filter j over the bins, zero-padded.
 *   Both bases 16-byte aligned.  n_fft in [2, FHVAE_FEATS_MAX_NFFT]; FBANK also needs the tile to fit LDS (n_fft <=
 *   FHVAE_FEATS_MAX_NFFT_FBANK) and n_mels in [1, FHVAE_FEATS_MAX_NMELS]; otherwise FHVAE_ERR_LIMIT before any launch.
 *   Pointers that break the framing rule set FHVAE_FEATS_BAD_PTR in the int32 device word `status` (never cleared by the
 *   library; read once per batch) and nothing is written.  Every row is a fixed-order f32 chain over its own samples: the
 *   result of a frame does not depend on the rest of the batch (bitwise).
 * tile_rows: frames per workgroup for (n_fft, ftype); 0 = not supported.
 * ------------------------------------------------------------------------------------------ */
#define FHVAE_FEATS_FBANK 0
#define FHVAE_FEATS_SPEC 1
#define FHVAE_FEATS_MAX_NFFT 2048
#define FHVAE_FEATS_MAX_NFFT_FBANK 1664
#define FHVAE_FEATS_MAX_NMELS 256
#define FHVAE_FEATS_BAD_PTR 1
int fhvae_feats_tile_rows(int64_t n_fft, int ftype);
int fhvae_feats_fwd(const float* wave, int64_t n_samples, const int64_t* wave_ptr, const int64_t* frame_ptr, int64_t U,
                    int64_t n_frames, const float* dft_basis, const float* mel_basis, int64_t n_fft, int64_t hop, int64_t n_mels,
                    int ftype, float* out, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Waveforms from magnitude spectrograms (csrc/synth.hip): Griffin-Lim with librosa 0.8.0's griffinlim / istft semantics
 * (window = periodic Hamming, win_length = n_fft, center = True), for a batch of U utterances per launch.  The framing is
 * the one of fhvae_feats_fwd read backwards: an utterance of F >= 2 frames has hop * (F - 1) samples.
 *   wave_ptr (U+1) int64 sample offsets, frame_ptr (U+1) int64 frame offsets; wave_ptr[0] = frame_ptr[0] = 0, wave_ptr[U] =
 *     n_samples, frame_ptr[U] = n_frames, wave_ptr[u+1] - wave_ptr[u] = hop * (frame_ptr[u+1] - frame_ptr[u] - 1).
 *   Complex arrays are (n_frames, n_fft/2+1, 2) f32 (re, im), 8-byte aligned.
 * istft: wave_out = overlap-add of window * irfft(spec row) at f * hop, divided by the sum of the squared window over the
 *   covering frames where that exceeds tiny(f32), the n_fft/2 centre padding trimmed.  Two launches: the inverse DFT of every
 *   frame into frames_ws (n_frames, KP) f32 (KP = n_fft rounded up to 16; 16-byte aligned), then a gather that sums the
 *   covering frames of every sample in increasing frame order (no atomics).
 *   synth_basis (KP, K2P) f32, K2P = 2 * (n_fft/2+1) rounded up to 16: row n holds at column 2b
 *     window[n] * c_b / n_fft * cos(2 pi b n / n_fft) and at 2b+1 -window[n] * c_b / n_fft * sin(2 pi b n / n_fft), c_b = 1
 *     for bin 0 and (even n_fft) bin n_fft/2, else 2; zero for n >= n_fft and columns >= 2 * (n_fft/2+1).  16-byte aligned.
 *   win_sq (n_fft) f32: the squared window.
 * project: frames of `wave` (centre padding by reflection, numpy "reflect" for any length; frame f reads padded positions
 *   f * hop .. f * hop + n_fft - 1; no pre-emphasis), rebuilt = their DFT (dft_basis as for fhvae_feats_fwd),
 *   a = rebuilt - coef * tprev, next = mag * a / (|a| + 1e-16).  mag (n_frames, n_fft/2+1) f32; tprev NULL = zero; rebuilt
 *   NULL = not stored.  For Griffin-Lim coef = momentum / (1 + momentum).
 * deemph: out[t] = wave[t] + coef * out[t-1] within every utterance (the inverse of the features' pre-emphasis), |coef| < 1;
 *   a blocked scan that restarts W samples before each 256-sample block of the utterance, |coef|^W < 2^-30 (W > 65536:
 *   FHVAE_ERR_LIMIT).  coef = 0 copies.  Only wave_ptr is needed.
 * n_fft in [2, FHVAE_FEATS_MAX_NFFT], 1 <= hop <= n_fft, otherwise FHVAE_ERR_SHAPE / FHVAE_ERR_LIMIT before any launch.
 * Pointers that break the rule above set FHVAE_SYNTH_BAD_PTR in the int32 device word `status` (never cleared by the
 * library) and nothing is written.  Every output is a fixed-order f32 chain over its own utterance: bitwise independent of
 * the batch.
 * tile_rows: frames per workgroup of the two MFMA kernels for n_fft; 0 = not supported.
 * ------------------------------------------------------------------------------------------ */
#define FHVAE_SYNTH_BAD_PTR 1
int fhvae_synth_tile_rows(int64_t n_fft);
int fhvae_synth_istft(const float* spec, int64_t n_frames, const int64_t* wave_ptr, const int64_t* frame_ptr, int64_t U,
                      int64_t n_samples, const float* synth_basis, const float* win_sq, int64_t n_fft, int64_t hop,
                      float* frames_ws, float* wave_out, int32_t* status, void* stream);
int fhvae_synth_project(const float* wave, int64_t n_samples, const int64_t* wave_ptr, const int64_t* frame_ptr, int64_t U,
                        int64_t n_frames, const float* dft_basis, const float* mag, const float* tprev, float coef, int64_t n_fft,
                        int64_t hop, float* rebuilt, float* next, int32_t* status, void* stream);
int fhvae_synth_deemph(const float* wave, const int64_t* wave_ptr, int64_t U, int64_t n_samples, float coef, float* out,
                       int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sample-rate conversion (csrc/resample.hip): librosa.load's resampling (librosa 0.8.0 resample(fix=True, scale=False) on
 * resampy 0.2.2's kaiser_best; the reference's prepare_numpy_data.py:108) for a batch of U utterances per call, as a
 * polyphase FIR whose weights the host computes in float64 (features.ResampleBank) for the reduced ratio L / M = sr_out /
 * sr_in.  An output row is P periods: outputs row * P * L + c, c < P * L, from the window x[row * P * M - WL + k], k < KP
 * (samples outside the utterance count as zero).
 *   wave_in (n_in) f32: the utterances' samples, concatenated; in_ptr (U+1) int64 their offsets (an utterance may be empty).
 *   out_ptr (U+1) int64: output offsets, out_ptr[u+1] - out_ptr[u] = ceil(n * ratio) in double precision for an utterance
 *     of n samples; out_ptr[0] = 0, out_ptr[U] = n_out.  Of those the first (int64)(n * ratio) are computed, the rest are 0
 *     (resampy's length, padded by librosa).
 *   row_ptr (U+1) int64: row offsets, row_ptr[u+1] - row_ptr[u] = ceil(outputs / (P * L)); row_ptr[0] = 0, row_ptr[U] = n_rows.
 *   bank (NCP, KP) f32, NCP = P * L rounded up to 16, KP a multiple of 16, 16-byte aligned: row c = weights of output c of a
 *     row over the window; zero rows past P * L.  chunks (NCP / 16, 2) int32: the range [c0, c1) of 16-sample chunks of the
 *     window in which the 16 columns of a group have weights (only those are multiplied).
 *   exc (n_exc) uint8, alt (alt_taps) f32, alt_wl: output p * L of an utterance with exc[p] != 0 (p < n_exc) is
 *     sum_k alt[k] * x[p * M - 1 - alt_wl + k] instead (resampy's time register, advanced by repeated addition, fell just
 *     below the integer time p * M; computed after the rows by a second launch).  n_exc = 0: none (exc / alt may be NULL).
 *   Limits, otherwise FHVAE_ERR_LIMIT before any launch: L <= FHVAE_RESAMPLE_MAX_L phases; NCP * KP <=
 *   FHVAE_RESAMPLE_MAX_BANK weights (64 MiB); 16 windows of KP + 4 floats within FHVAE_RESAMPLE_LDS_FLOATS (the
 *   160 KiB of a CU's LDS less the 3.25 KiB of per-row bookkeeping), i.e. KP <= 2496.
 *   Pointers that break the rules above set FHVAE_RESAMPLE_BAD_PTR in the int32 device word `status` (never cleared by the
 *   library) and nothing is written.  Every output is a fixed-order f32 chain over its own window: bitwise independent of
 *   the batch and of the utterance's place in it.
 * tile_rows: rows per workgroup for a window of KP samples; 0 = not supported.
 * ------------------------------------------------------------------------------------------ */
#define FHVAE_RESAMPLE_MAX_L 4096
#define FHVAE_RESAMPLE_MAX_BANK (1 << 24)
#define FHVAE_RESAMPLE_LDS_FLOATS 40128
#define FHVAE_RESAMPLE_BAD_PTR 1
int fhvae_resample_tile_rows(int64_t KP);
int fhvae_resample_fwd(const float* wave_in, int64_t n_in, const int64_t* in_ptr, const int64_t* out_ptr,
                       const int64_t* row_ptr, int64_t U, int64_t n_rows, const float* bank, const int32_t* chunks, int64_t L,
                       int64_t M, int64_t P, int64_t KP, int64_t WL, double ratio, const uint8_t* exc, int64_t n_exc,
                       const float* alt, int64_t alt_taps, int64_t alt_wl, float* wave_out, int64_t n_out, int32_t* status,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * Linear magnitudes from mel magnitudes (csrc/melinv.hip): per frame, minimise ||A x - m||^2 over x >= 0 for the mel bank A
 * (n_mels, n_bins) by n_iter accelerated projected-gradient (FISTA) steps from zero, all in one launch:
 *   x = y = 0;  n_iter times { g = A^T (A y - m);  x+ = max(y - inv_l g, 0);  y = x+ + beta[k] (x+ - x);  x = x+ }
 *   mel (n_frames, n_mels) f32: mel magnitudes m, or with FHVAE_MELINV_IN_LOG their natural logarithms (exp on the device).
 *   out (n_frames, n_bins) f32: x, or with FHVAE_MELINV_OUT_LOG max(ln x, -50) as FHVAE_FEATS_SPEC features look.
 *   The bank in band form (a bin lies in at most two adjacent filters, a filter is one contiguous run of bins):
 *     bin_filt (n_bins) int32 in [0, n_mels): the lower filter f of bin b; bin_w (n_bins, 2) f32 = A[f, b], A[f + 1, b] (zero
 *       where there is none).
 *     filt_first (n_mels) int32, filt_off (n_mels + 1) int32, filt_w (nnz) f32: filter j holds A[j, filt_first[j] + k] =
 *       filt_w[filt_off[j] + k] for k < filt_off[j + 1] - filt_off[j]; filt_off[0] = 0, filt_off[n_mels] = nnz <= 2 n_bins.  A
 *       filter without bins is legal.
 *   inv_l f32 = 1 / lambda_max(A A^T), not above it; beta (n_iter) f32 = (t_k - 1) / t_{k+1}, t_0 = 1,
 *     t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2: both computed by the host in double precision.
 *   n_mels in [1, FHVAE_FEATS_MAX_NMELS], n_bins in [2, FHVAE_FEATS_MAX_NFFT / 2 + 1], n_iter >= 1, otherwise
 *   FHVAE_ERR_SHAPE / FHVAE_ERR_LIMIT before any launch.  A band that points outside its arrays sets FHVAE_MELINV_BAD_BAND
 *   in the int32 device word `status` (never cleared by the library) and nothing is written.  Every output is a fixed-order
 *   f32 chain over its own frame: bitwise independent of the batch and of the frame's place in it.
 * tile_rows: frames per workgroup for (n_mels, n_bins); 0 = not supported.
 * ------------------------------------------------------------------------------------------ */
#define FHVAE_MELINV_IN_LOG 1
#define FHVAE_MELINV_OUT_LOG 2
#define FHVAE_MELINV_BAD_BAND 1
int fhvae_mel_invert_tile_rows(int64_t n_mels, int64_t n_bins);
int fhvae_mel_invert(const float* mel, int64_t n_frames, int64_t n_mels, int64_t n_bins, const int32_t* bin_filt,
                     const float* bin_w, const int32_t* filt_first, const int32_t* filt_off, const float* filt_w, int64_t nnz,
                     float inv_l, const float* beta, int64_t n_iter, int flags, float* out, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Kaldi filterbank features (csrc/kaldi_fbank.hip): compute-fbank-feats with snip-edges framing, for a batch of U
 * utterances in one launch.  N = frame_len, S = frame_shift, P = padded_len = the smallest power of two >= N.
 *   wave (n_samples) f32: the utterances' samples on the int16 scale, concatenated; wave_ptr (U+1) int64 their offsets.
 *   frame_ptr (U+1) int64: output row offsets, frame_ptr[u+1] - frame_ptr[u] = 1 + (L - N) / S for an utterance of L >= N
 *     samples; frame_ptr[0] = 0, frame_ptr[U] = n_frames.  Frame f of an utterance is its samples f*S .. f*S + N - 1.
 *   Per frame, in this order: x[i] += dither * g(f, i); x -= mean(x) (FHVAE_KALDI_REMOVE_DC); x[i] -= preemph * x[i-1] for
 *   i = N-1 .. 1, then x[0] -= preemph * x[0]; window and P-point DFT, power re^2 + im^2 of bins 0 .. P/2 - 1 (its square
 *   root without FHVAE_KALDI_USE_POWER); out (n_frames, n_mels) = power . mel^T, with FHVAE_KALDI_USE_LOG
 *   ln(max(., FLT_EPSILON)), the floor being the f32 nearest to ln 2^-23.
 *   dft_basis (32*G, KP) f32, KP = N rounded up to 16, G = ceil((P/2) / 16): row 32g + i holds w[n] cos(2 pi n b / P) and row
 *     32g + 16 + i holds -w[n] sin(2 pi n b / P) for bin b = 16g + i, n < N (zero for b >= P/2 and n >= N); w the window.
 *   mel_basis (16*ceil(n_mels/16), 16*G) f32: row j = mel filter j over bins 0 .. P/2 - 1, zero-padded.  Both 16-byte aligned.
 *   Dither noise g(f, i), only evaluated when dither != 0 (stream_ids may be NULL otherwise): Philox4x32-10 with
 *     key     = (seed & 0xffffffff, seed >> 32)
 *     counter = (f, i / 4, stream_ids[u] & 0xffffffff, stream_ids[u] >> 32)      f = frame index within utterance u
 *     round   : (c0, c1, c2, c3) <- (hi(0xCD9E8D57 * c2) ^ c1 ^ k0, lo(0xCD9E8D57 * c2), hi(0xD2511F53 * c0) ^ c3 ^ k1,
 *               lo(0xD2511F53 * c0)), ten times, the key advancing by (0x9E3779B9, 0xBB67AE85) after each round
 *     uniform : u(r) = (2 * (r >> 9) + 1) * 2^-24, in (0, 1), exact in f32
 *     normals : the output words (r0, r1, r2, r3) give samples 4*(i/4) + 0 .. 3 as
 *               sqrt(-2 ln u(r0)) * cos(2 pi u(r1)), sqrt(-2 ln u(r0)) * sin(2 pi u(r1)),
 *               sqrt(-2 ln u(r2)) * cos(2 pi u(r3)), sqrt(-2 ln u(r2)) * sin(2 pi u(r3))     (f32 on the device)
 *   so the noise of a sample depends on (seed, stream id, f, i) alone: overlapping frames do not share noise, and a
 *   frame's features do not depend on the batch it is computed in.
 *   1 <= S <= N, N >= 2 and P the smallest power of two >= N, otherwise FHVAE_ERR_SHAPE; P <= FHVAE_KALDI_MAX_P,
 *   N <= FHVAE_KALDI_MAX_N (above it a 16-frame tile and its spectrum do not fit the LDS) and n_mels in
 *   [1, FHVAE_FEATS_MAX_NMELS], otherwise FHVAE_ERR_LIMIT; all before any launch.  Pointers that break the framing rule
 *   set FHVAE_KALDI_BAD_PTR in the int32 device word `status` (never cleared by the library) and nothing is written.
 *   Every row is a fixed-order f32 chain over its own samples (bitwise independent of the batch).
 * tile_rows: frames per workgroup for (N, P, n_mels); 0 = not supported.
 * ------------------------------------------------------------------------------------------ */
#define FHVAE_KALDI_REMOVE_DC 1
#define FHVAE_KALDI_USE_LOG 2
#define FHVAE_KALDI_USE_POWER 4
#define FHVAE_KALDI_MAX_P 2048
#define FHVAE_KALDI_MAX_N 1504
#define FHVAE_KALDI_BAD_PTR 1
int fhvae_kaldi_fbank_tile_rows(int64_t frame_len, int64_t padded_len, int64_t n_mels);
int fhvae_kaldi_fbank_fwd(const float* wave, int64_t n_samples, const int64_t* wave_ptr, const int64_t* frame_ptr,
                          const uint64_t* stream_ids, int64_t U, int64_t n_frames, const float* dft_basis,
                          const float* mel_basis, int64_t frame_len, int64_t frame_shift, int64_t padded_len, int64_t n_mels,
                          float preemph, float dither, uint64_t seed, int flags, float* out, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Kaldi compressed matrices (csrc/kaldi_cm.hip): the archive tokens CM, CM2 and CM3 of matrix/compressed-matrix.{h,cc},
 * decoded into and coded from a row-major (n_frames, F) f32 matrix, a batch of U utterances per call (additions of ABI 11).
 *   payload (n_bytes) uint8: the utterances' payloads (what follows the 16-byte header of an archive entry), each at a
 *     byte offset that is a multiple of 4; n_bytes a multiple of 4, the pointer 4-byte aligned.
 *     CM : cols headers of four uint16 (p0, p25, p75, p100), then cols x rows uint8, column-major
 *     CM2: rows x cols uint16 row-major;  CM3: rows x cols uint8 row-major
 *   desc (U): per utterance the token, its size (cols = F), the global header (min_value, range), payload_off, row0 (its
 *     first row in the matrix) and tile0, the number of tiles of FHVAE_KALDI_CM_TILE_ROWS rows of the utterances before it
 *     (n_tiles = the total).  A descriptor that breaks these rules or reaches outside a buffer sets
 *     FHVAE_KALDI_CM_BAD_DESC in the int32 device word `status` (never cleared by the library) and nothing is written.
 * decompress: f32, one rounding per operation, division correctly rounded, no contraction:
 *     u(w) = min_value + (range * w) / 65535;  CM2: u(w);  CM3: min_value + (range * b) / 255;
 *     CM, with P0, P25, P75, P100 = u(p0) .. u(p100) of the column: b <= 64: P0 + ((P25 - P0) * b) / 64; b <= 192:
 *     P25 + ((P75 - P25) * (b - 64)) / 128; else P75 + ((P100 - P75) * (b - 192)) / 63.
 * compress: the token is the caller's choice per utterance; min_value and range are WRITTEN to the descriptors: the
 *     matrix minimum and max - min (1 + |min| for a constant matrix).  q16(v) = trunc(double(f32(clamp((v - min) / range,
 *     0, 1) * 65535)) + 0.499), q8 with 255.  CM2 / CM3 store q16 / q8.  CM: with s the sorted column and q = rows / 4,
 *     p0 = min(q16(s[0]), 65532), p25 = min(max(q16(s[q]), p0 + 1), 65533), p75 = min(max(q16(s[3q]), p25 + 1), 65534),
 *     p100 = max(q16(s[rows-1]), p75 + 1) (the order statistics are exact for any number of rows); with
 *     Pk = min + (range * 1.52590218966964e-05f) * pk a value below P25 is coded clamp(trunc(double(f * 64) + 0.5), 0, 64),
 *     f = (v - P0) / (P25 - P0); below P75 64 + trunc(double((v - P25) / (P75 - P25) * 128) + 0.5) clamped to [64, 192];
 *     else 192 + trunc(double((v - P75) / (P100 - P75) * 63) + 0.5) clamped to [192, 255].
 *     ws: 2 U uint32 of device scratch.  A NaN or Inf in an utterance sets FHVAE_KALDI_CM_NONFINITE in `status`.
 * ------------------------------------------------------------------------------------------ */
#define FHVAE_KALDI_CM 1
#define FHVAE_KALDI_CM2 2
#define FHVAE_KALDI_CM3 3
#define FHVAE_KALDI_CM_TILE_ROWS 128
#define FHVAE_KALDI_CM_BAD_DESC 1
#define FHVAE_KALDI_CM_NONFINITE 2
typedef struct FhvaeKaldiCmDesc {
  int32_t token, rows, cols, tile0;
  float min_value, range;
  int64_t payload_off, row0;
} FhvaeKaldiCmDesc;
int fhvae_kaldi_decompress(const uint8_t* payload, int64_t n_bytes, const FhvaeKaldiCmDesc* desc, int64_t U, int64_t n_tiles,
                           float* out, int64_t n_frames, int64_t F, int32_t* status, void* stream);
int fhvae_kaldi_compress(const float* feats, int64_t n_frames, int64_t F, FhvaeKaldiCmDesc* desc, int64_t U, int64_t n_tiles,
                         uint32_t* ws, uint8_t* payload, int64_t n_bytes, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * FLAC decoding (csrc/flac.hip): the frames of a batch of U files, RFC 9639, up to 24 bits per sample and 8 channels
 * (additions of ABI 11).  The host parses the container (flac_lite.py) and passes what follows each file's metadata.
 *   buf (n_bytes) uint8: the files' frame bytes one after the other.
 *   desc (U): per file its byte range [byte_begin, byte_end) in buf (ascending, not overlapping), STREAMINFO's rate,
 *     channels, bits per sample and minimum block size, and where its samples go: int32 elements
 *     [out_off, out_off + n_samples * channels) of `out`, interleaved (sample, channel).
 * scan:   info[p] for every byte position p: 0, or FHVAE_FLAC_CAND | block size << 8 | header bytes where a frame header
 *     starts that is well formed, agrees with the file's STREAMINFO and carries its CRC-8.
 * decode: one work item per candidate position cand_pos[i] (a header as the scan accepts it).  With out == NULL the frame
 *     is parsed to its end and its CRC-16 verified; with out != NULL it is decoded into its file's part of `out` at its
 *     coded sample position (the CRC-16 is not computed again).  Per candidate: cand_status (FHVAE_OK or a code below),
 *     cand_end (the byte position behind the frame, -1 unless FHVAE_OK) and cand_spos (the coded sample number, or the
 *     coded frame number times min_block).  Which candidates are frames -- the chain from the first byte of a file, each
 *     frame starting where the one before ends -- is for the caller to decide between the two calls.
 *     No read leaves a file's byte range and no write its part of `out`, whatever the bytes say.
 * ------------------------------------------------------------------------------------------ */
#define FHVAE_FLAC_CAND 0x80000000u
#define FHVAE_FLAC_BAD_DESC 1     /* cand_pos in no file, or a descriptor that breaks the rules above */
#define FHVAE_FLAC_BAD_HEADER 2   /* no acceptable frame header at cand_pos */
#define FHVAE_FLAC_BAD_SUBFRAME 3 /* padding bit set, reserved type, wasted bits >= sample size, order > block size */
#define FHVAE_FLAC_BAD_LPC 4      /* coefficient precision code 1111 or a negative shift */
#define FHVAE_FLAC_BAD_RESIDUAL 5 /* reserved coding method, partitions that do not divide the block, residual > 32 bits */
#define FHVAE_FLAC_TRUNCATED 6    /* the frame needs bytes behind the end of its file */
#define FHVAE_FLAC_BAD_PADDING 7  /* non-zero bits before the byte boundary that ends the frame */
#define FHVAE_FLAC_BAD_CRC 8      /* CRC-16 mismatch */
#define FHVAE_FLAC_BAD_RANGE 9    /* the frame's samples do not fit its file's part of out */
typedef struct FhvaeFlacDesc {
  int64_t byte_begin, byte_end, out_off, n_samples;
  int32_t rate, channels, bps, min_block;
} FhvaeFlacDesc;
int fhvae_flac_scan(const uint8_t* buf, int64_t n_bytes, const FhvaeFlacDesc* desc, int64_t U, uint32_t* info, void* stream);
int fhvae_flac_decode(const uint8_t* buf, int64_t n_bytes, const FhvaeFlacDesc* desc, int64_t U, const int64_t* cand_pos,
                      int64_t n_cand, int32_t* cand_status, int64_t* cand_end, int64_t* cand_spos, int32_t* out, int64_t n_out,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * Speaker verification (csrc/sv.hip): the histogram of the cosine scores of all pairs of S embeddings, target and non-target
 * trials apart, with no (S, S) temporary (an addition of ABI 11).
 *   emb (S, D) f32 with leading dimension ld >= D; label (S) int32, -1 = no label: such a row takes part in no trial.
 *   A trial is an unordered pair i < j with both labels >= 0; it is a target iff label[i] == label[j].
 *   score = dot(e_i, e_j) / (n_i * n_j), n = max(sqrt(sum e^2), 1e-30): the dot on exact-f32 MFMA, the sum of squares an f32
 *     fma chain, sqrt and the division correctly rounded; the product n_i * n_j is floored at FLT_MIN (it underflows only
 *     where both rows are below 1e-19, and the dot is 0 there), so a zero row scores 0 against everything.
 *   bin = clamp((int)floorf((score + 1) * (n_bins / 2)), 0, n_bins - 1), in f32.
 *   hist (2, n_bins) uint64 on the device, overwritten: row 0 counts the target trials, row 1 the non-target trials.
 *   The result depends on (emb, label, n_bins) alone: not on the grid, not on S relative to the tiles; score(i, j) equals
 *   score(j, i) bit for bit, so it does not depend on the order of the rows either.  Two calls give equal bits.
 *   ws: fhvae_sv_hist_ws_bytes(S) bytes of device scratch (the rows' norms), 4-byte aligned.
 *   D a multiple of 16 in [16, 128], n_bins a power of two in [64, 8192], S >= 1 (S = 1: all zeros), ld >= D, ws_bytes
 *   large enough, otherwise FHVAE_ERR_SHAPE; ld a multiple of 4 and emb 16-byte aligned, otherwise FHVAE_ERR_ALIGN;
 *   S <= 2^24, otherwise FHVAE_ERR_LIMIT; all before any launch.
 * ------------------------------------------------------------------------------------------ */
int64_t fhvae_sv_hist_ws_bytes(int64_t S);
int fhvae_sv_hist(const float* emb, int64_t ld, const int32_t* label, int64_t S, int64_t D, int64_t n_bins, void* ws,
                  int64_t ws_bytes, uint64_t* hist, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact t-SNE of N embeddings (csrc/tsne.hip) with no (N, N) array: every pass recomputes the squared distances, and the
 * gradient recomputes p_ij, from three numbers per row (an addition of ABI 11).
 *   x (N, D) f32 with leading dimension ld >= D (the caller subtracts the column means).
 *   d2(i, j) = max(n_i + n_j - 2 x_i . x_j, 0): the dot on exact-f32 MFMA, n an f32 fma chain; d2(i, j) == d2(j, i) bit for bit.
 *   j = i takes part in nothing.  m_i = min_j d2(i, j); e_ij = exp(-beta_i (d2(i, j) - m_i)); Z_i = sum_j e_ij;
 *   p_j|i = e_ij / Z_i; p_ij = (p_j|i + p_i|j) / (2 N).
 * fhvae_tsne_affinity: beta_i by bisection on log2 beta over [-60, 60], 48 steps and no exit that depends on the data: a step
 *   moves the lower end up where log Z_i + beta_i sum_j e_ij (d2 - m_i) / Z_i > log(perplexity); beta_i = 2^(the middle of the
 *   last interval).  Writes beta, m, Z (each (N) f32 on the device).  One launch, 50 streaming passes inside it.
 * fhvae_tsne_step: one iteration at y (N, 2), nothing read back:
 *   w_ij = 1 / (1 + |y_i - y_j|^2); F_i = exaggeration sum_j p_ij w_ij (y_i - y_j); R_i = sum_j w_ij^2 (y_i - y_j);
 *   W_i = sum_j w_ij; Zq = sum_i W_i; grad_i = 4 (F_i - R_i / Zq);
 *   inc = v grad < 0; g = inc ? g + 0.2 : 0.8 g; g = max(g, 0.01); v = momentum v - lr g grad; y += v   (y, v, g (N, 2) f32).
 *   kl (device, 1 f32, may be NULL): KL = sum_{i != j} p_ij log(p_ij Zq / w_ij) at the y the call was given, without the
 *   exaggeration (a term with p_ij < 1e-30 counts as 0).
 * fhvae_tsne_grad: the same pass without the update: out (N, 7) f32 = F (2, with the exaggeration), R (2), W, grad (2) per
 *   row, scal (2) f32 = Zq, KL.
 *   The j range is split into chunks; per-row partials per chunk go to the workspace and are added in index order, Zq in a
 *   fixed order in double: no floating-point atomic, two calls give equal bits.
 *   ws: fhvae_tsne_ws_bytes(N, D) bytes of device scratch, 16-byte aligned (0 for an N the entries refuse): the norms, 7 N
 *   floats per chunk, 4 per workgroup; chunks <= max(1, 2048 / ceil(N / 256)) and <= ceil(N / 512): N * chunks <= max(N, 2^19).
 *   8 <= N, D a multiple of 16 in [16, 128], ld >= D, 1 <= perplexity <= (N - 1) / 3, ws_bytes large enough, otherwise
 *   FHVAE_ERR_SHAPE; ld a multiple of 4, x and ws 16-byte, y 8-byte and the rest 4-byte aligned, otherwise FHVAE_ERR_ALIGN;
 *   N <= 2^22, otherwise FHVAE_ERR_LIMIT; all before any launch.
 * ------------------------------------------------------------------------------------------ */
int64_t fhvae_tsne_ws_bytes(int64_t N, int64_t D);
int fhvae_tsne_affinity(const float* x, int64_t ld, int64_t N, int64_t D, float perplexity, float* beta, float* m, float* z,
                        void* ws, int64_t ws_bytes, void* stream);
int fhvae_tsne_step(const float* x, int64_t ld, int64_t N, int64_t D, const float* beta, const float* m, const float* z, float* y,
                    float* v, float* g, float exaggeration, float momentum, float lr, float* kl, void* ws, int64_t ws_bytes,
                    void* stream);
int fhvae_tsne_grad(const float* x, int64_t ld, int64_t N, int64_t D, const float* beta, const float* m, const float* z,
                    const float* y, float exaggeration, float* out, float* scal, void* ws, int64_t ws_bytes, void* stream);

/* small utilities used by the host side */
/* (B,T,F) batch-major f32 -> (T,B,F) time-major in operand dtype `dtype` (and optionally f32) */
int fhvae_to_time_major(const float* x_btf, void* x_tbf, float* x_tbf_f32, int64_t B, int64_t T,
                        int64_t F, int dtype, void* stream);
/* f32 -> bf16 cast, optional transposed copy: src [R,C] -> dst [R,C] and dst_t [C,R] (either NULL) */
int fhvae_cast_bf16(const float* src, void* dst, void* dst_t, int64_t R, int64_t C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FHVAE_HIP_H */
