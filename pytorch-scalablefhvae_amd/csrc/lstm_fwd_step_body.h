// lstm_fwd_step_body.h -- the body of lstm_fwd_step_kernel and of its inference twin, included INSIDE both kernels (it is not a header of its
// own): the training kernel then compiles to the very instructions it had as a single function.  `kSave` is a constexpr of
// the including kernel; false = fhvae_lstm_seq_infer: nothing that only the backward reads leaves the kernel.
  using TL = Tile<T, BM, BN, WM, WN, CH>;
  constexpr int TM = TL::TM;
  static_assert(TL::TN == 4, "one wave = one 64-column gate group");
  constexpr bool kPrefetch = TM == 1;
  constexpr int NBUF = CH >= 32 ? 2 : 1;  // wide panels = few large workgroups: double buffer; narrow: occupancy
  using GT = GldsTile<T, BM, BN, WM, WN, CH, NBUF>;
  __shared__ __attribute__((aligned(16))) char smem[TL::SMEM > GT::SMEM ? TL::SMEM : GT::SMEM];
  const FwdJob<T>& J = jobs.job[blockIdx.z];
  const int B = jobs.B, H = jobs.H;
  // blockIdx.x walks the ROW tiles: workgroups are dealt round-robin over the 8 XCDs by linear id, so every XCD
  // (private 4 MB L2) sees 1/8 of the activations and all of the (small) weight slice, instead of all activations
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  f32x4 acc[TM][4];
  zero_acc(acc);
  RowIdent arm{B};
  GateRowMap brm{H};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int unit = (n0 / 64 + wn) * 16 + (lane & 15);
  const bool uok = unit < H;
  auto row_of = [&](int tm, int r) { return m0 + wm * (TM * 16) + tm * 16 + (lane >> 4) * 4 + r; };
  auto fetch_add = [&](int row, int g) -> float {
    float v = 0.f;
    if (J.pre) v = J.pre[(int64_t)row * J.pre_ld + g * H + unit];
    if (J.bias_a) v += J.bias_a[g * H + unit] + J.bias_b[g * H + unit];
    return v;
  };
  // small tile: epilogue operands are fetched BEFORE the contraction so their latency hides under it
  float padd[kPrefetch ? 4 : 1][4], cprev[kPrefetch ? 4 : 1];
  if constexpr (kPrefetch) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row_of(0, r);
      const bool ok = uok && row < B;
#pragma unroll
      for (int g = 0; g < 4; ++g) padd[r][g] = ok ? fetch_add(row, g) : 0.f;
      cprev[r] = (ok && J.c_prev) ? J.c_prev[(int64_t)row * H + unit] : 0.f;
    }
  }
  const int nkb = num_kblocks<T, CH>(J.seg);
  // interior tiles with panel-aligned K take the LDS-DMA path; edges / odd shapes the register-staged one
  const bool dma = jobs.glds && m0 + BM <= B && brm.all_valid(n0, BN) && seg_glds_ok<T>(J.seg[0], TL::BK) &&
                   seg_glds_ok<T>(J.seg[1], TL::BK);
  if (dma)
    mainloop_glds<T, BM, BN, WM, WN, CH, NBUF, false>(acc, J.seg, m0, n0, arm, brm, smem);
  else
    mainloop<T, BM, BN, WM, WN, CH, true, true, false>(acc, J.seg, m0, B, n0, (int)gridDim.y * BN, arm, brm, 0, nkb, smem);

  if (!uok) return;
#pragma unroll
  for (int tm = 0; tm < TM; ++tm)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row_of(tm, r);
      if (row >= B) continue;
      float pa[4], cp;
      if constexpr (kPrefetch) {
#pragma unroll
        for (int g = 0; g < 4; ++g) pa[g] = padd[r][g];
        cp = cprev[r];
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) pa[g] = fetch_add(row, g);
        cp = J.c_prev ? J.c_prev[(int64_t)row * H + unit] : 0.f;
      }
      const float ig = sigmoidf_(acc[tm][0][r] + pa[0]), fg = sigmoidf_(acc[tm][1][r] + pa[1]);
      const float gg = tanhf_(acc[tm][2][r] + pa[2]), og = sigmoidf_(acc[tm][3][r] + pa[3]);
      const float c = __builtin_fmaf(fg, cp, ig * gg);
      const float h = og * tanhf_(c);
      J.c_out[(int64_t)row * H + unit] = c;
      store_h<T>(J.h_out + (int64_t)row * H + unit, h);
      if (J.h_out_f32) J.h_out_f32[(int64_t)row * H + unit] = h;
      if constexpr (kSave) {
        T* go = J.gates_out + (int64_t)row * 4 * H + unit;
        store_h<T>(go, ig);
        store_h<T>(go + H, fg);
        store_h<T>(go + 2 * H, gg);
        store_h<T>(go + 3 * H, og);
      }
      if (J.hn_out) J.hn_out[(int64_t)row * J.hn_ld + unit] = h;
    }
