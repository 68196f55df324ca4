// lstm_cell_fwd_body.h -- the body of cell_fwd_kernel and of its inference twin, included INSIDE both kernels (it is not a header of its
// own): the training kernel then compiles to the very instructions it had as a single function.  `kSave` is a constexpr of
// the including kernel; false = fhvae_lstm_seq_infer: nothing that only the backward reads leaves the kernel.
  constexpr int BK = CellOp<T>::BK, EPC = CellOp<T>::EPC, ES = (int)sizeof(T);
  constexpr int BM = 128, RB = 128, UN = 32;
  constexpr int STAGE = (BM + RB) * 128;
  __shared__ __attribute__((aligned(1024))) char st0[STAGE];
  __shared__ __attribute__((aligned(1024))) char st1[STAGE];
  __shared__ __attribute__((aligned(1024))) char st2[NS > 2 ? STAGE : 16];
  __shared__ __attribute__((aligned(1024))) char st3[NS > 3 ? STAGE : 16];
  const FwdJob<T>& J = jobs.job[blockIdx.z];
  const int H = jobs.H;
  const int m0 = blockIdx.x * BM, u0 = blockIdx.y * UN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int i = lane & 15, gq = lane >> 4;

  // Up to four K segments: h^{l-1}_t . W_ih[l], h^l_{t-1} . W_hh[l], and for layer 0 x_t . W_ih[0][:, :I], xc . W_ih[0][:, I:]
  // (any K that is a multiple of 8: the 16-byte chunks past K are loaded from an out-of-range offset = zeros).  The segment
  // of a k-step is read from the kernel arguments by a dynamic (uniform) index: a select chain over four preloaded descriptors
  // became branches in the loop, and a branch there turns the counted vmcnt waits into vmcnt(0).
  static_assert(offsetof(FwdJob<T>, xseg) == offsetof(FwdJob<T>, seg) + 2 * sizeof(Seg), "seg[] and xseg[] form one array of 4");
  const Seg* segs = &J.seg[0];
  int end0, end1, end2, end3;  // first k-step after each segment
  end0 = (segs[0].K + BK - 1) / BK;
  end1 = end0 + (segs[1].K + BK - 1) / BK;
  end2 = end1 + (segs[2].K + BK - 1) / BK;
  end3 = end2 + (segs[3].K + BK - 1) / BK;
  const int nsteps = end3;
  // image row of this lane's piece q: (wave * 4 + q) * 8 + (lane >> 3); logical chunk c8 lands in physical chunk lane & 7.
  // Weight rows: image row j = wn' * 64 + g * 16 + i'  <->  row g * H + u0 + wn' * 16 + i' of W, i.e. piece q adds
  // (q >> 1) * H + (q & 1) * 8 rows to piece 0's
  const unsigned c8 = (unsigned)((lane & 7) ^ (lane >> 3));
  const unsigned rowa0 = (unsigned)(wave * 32 + (lane >> 3));
  const unsigned rowb0 = (unsigned)((wave & 1) * 2 * H + u0 + (wave >> 1) * 16 + (lane >> 3));

  f32x4 acc[4][4];
#pragma unroll
  for (int tm = 0; tm < 4; ++tm)
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto issue = [&](char* stg, int ks, int part) {
    int s = (ks >= end0) + (ks >= end1) + (ks >= end2);  // uniform
    int start = ks >= end0 ? end0 : 0;
    start = ks >= end1 ? end1 : start;
    start = ks >= end2 ? end2 : start;
    const int kl = ks - start;
    const Seg& S = segs[s];
    const unsigned la = (unsigned)(S.lda * ES), lb = (unsigned)(S.ldb * ES);
    const __amdgpu_buffer_rsrc_t a = __builtin_amdgcn_make_buffer_rsrc((T*)S.A + (int64_t)m0 * S.lda, 0, (int)(BM * la), 0x00020000);
    const __amdgpu_buffer_rsrc_t b = __builtin_amdgcn_make_buffer_rsrc((T*)S.B, 0, (int)(4 * H * lb), 0x00020000);
    // past the segment's K (or past the last step): bit 30 set = beyond num_records, the load returns zeros.  Plain ALU on
    // purpose: selects here came back as exec-masked branches inside the loop
    const int segK = S.K;
    const unsigned oob = (unsigned)((int)(ks >= nsteps) | (int)(kl * BK + (int)c8 * EPC >= segK)) << 30;
    const unsigned kb = ((unsigned)(kl * 128) + c8 * 16u) | oob;
    unsigned xa[4], xb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      xa[q] = (rowa0 + (unsigned)(q * 8)) * la + kb;
      xb[q] = (rowb0 + (unsigned)((q >> 1) * H + (q & 1) * 8)) * lb + kb;
    }
    if (part != 1) cell_issue<4>(stg, a, xa, 0u, wave);
    if (part != 0) cell_issue<4>(stg + BM * 128, b, xb, 0u, wave);
  };
  cell_mainloop<T, BM, RB, NS>(acc, nsteps, issue, st0, st1, st2, st3);

  // Epilogue through LDS: the accumulators (one lane = i,f,g,o of a (row, unit): 16 lanes x 4 B runs) go to an f32 image
  // X[row][gate][32 units] (512 B per row; rows 0..63 in st0, 64..127 in st1), then every lane takes (row, 8 consecutive
  // units) items: 16-byte global loads / stores, whole 64- / 128-byte runs per row (the per-lane form issued 12 two- and
  // four-byte accesses per element).  16-byte slot s of a row sits at s ^ swz(row): conflict-free for the 4-byte writes
  // (the four 4-row groups of a wave land on the four 64-byte quarters) and for the 16-byte reads.
  auto swz = [](int row) { return (row & 1) ^ (((row >> 2) & 1) << 2) ^ ((((row >> 1) ^ (row >> 3)) & 1) << 3); };
  const unsigned uH = (unsigned)H;
  {
    const unsigned unit = u0 + wn * 16 + i;
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    if (J.bias_a) {
#pragma unroll
      for (int g = 0; g < 4; ++g) bsum[g] = J.bias_a[g * uH + unit] + J.bias_b[g * uH + unit];
    }
    __syncthreads();  // every wave has read its last stage
    char* xw = wm ? st1 : st0;
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = tm * 16 + gq * 4 + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int slot = g * 8 + wn * 4 + (i >> 2);
          *(cell_lds_f)(xw + lr * 512 + ((slot ^ swz(lr)) << 4) + (i & 3) * 4) = acc[tm][g][r] + bsum[g];
        }
      }
    __syncthreads();
  }
  const bool has_pre = J.pre != nullptr, has_cp = J.c_prev != nullptr;
  const float* prep = has_pre ? J.pre : J.c_out;  // stand-ins keep the loads unconditional (masked below)
  const unsigned pld = has_pre ? (unsigned)J.pre_ld : uH;
  const float* cprev = has_cp ? J.c_prev : J.c_out;
  const int lr = threadIdx.x >> 2, chunk = threadIdx.x & 3;
  const unsigned u = u0 + chunk * 8;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const char* xr = (k ? st1 : st0) + lr * 512;
    const unsigned row = m0 + k * 64 + lr;
    float x[4][8], pa[4][8], cp[8];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      ld8(prep + row * pld + (has_pre ? g * uH + u : 0u), pa[g]);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const f32x4v v = *(cell_lds_f4)(xr + (((g * 8 + chunk * 2 + hh) ^ swz(lr)) << 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) x[g][hh * 4 + e] = v[e];
      }
    }
    ld8(cprev + row * uH + u, cp);
    float ig[8], fg[8], gg[8], og[8], c[8], h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ig[e] = sigmoidf_(x[0][e] + (has_pre ? pa[0][e] : 0.f));
      fg[e] = sigmoidf_(x[1][e] + (has_pre ? pa[1][e] : 0.f));
      gg[e] = tanhf_(x[2][e] + (has_pre ? pa[2][e] : 0.f));
      og[e] = sigmoidf_(x[3][e] + (has_pre ? pa[3][e] : 0.f));
      c[e] = __builtin_fmaf(fg[e], has_cp ? cp[e] : 0.f, ig[e] * gg[e]);
      h[e] = og[e] * tanhf_(c[e]);
    }
    const unsigned o = row * uH + u;
    st8(J.c_out + o, c);
    st8t(J.h_out + o, h);
    if (J.h_out_f32) st8(J.h_out_f32 + o, h);
    if constexpr (kSave) {
      T* go = J.gates_out + row * 4u * uH + u;
      st8t(go, ig);
      st8t(go + uH, fg);
      st8t(go + 2 * uH, gg);
      st8t(go + 3 * uH, og);
    }
    if (J.hn_out) st8(J.hn_out + row * (unsigned)J.hn_ld + u, h);
  }
