// lstm_fwd_ksplit_body.h -- the body of lstm_fwd_ksplit_kernel and of its inference twin, included INSIDE both kernels (it is not a header of its
// own): the training kernel then compiles to the very instructions it had as a single function.  `kSave` is a constexpr of
// the including kernel; false = fhvae_lstm_seq_infer: nothing that only the backward reads leaves the kernel.
  constexpr int HC = H / 8, KS = H / 32;
  constexpr int KSP = 64 / RB;    // waves per row tile
  constexpr int KPW = KS / KSP;   // k32-steps of each source per wave
  constexpr int W_BYTES = 64 * HC * 16;
  constexpr int NW = 2 * L - 1;
  static_assert(KSP >= L && KS % KSP == 0, "k split");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Wl = smem;
  char* Part = smem + NW * W_BYTES;             // [wave][L][4] tiles of 1 KB
  int* s_word = (int*)(Part + 4 * L * 4 * 1024);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int rt = wave / KSP, kp = wave % KSP;

  const int joined = cluster_join(p.sync, s_word);
  if (joined < 0) return;
  const int info = joined & 255;                                 // XCD * 32 + slot
  const unsigned ep0 = (unsigned)(joined >> 8) * kSeqEpochs;     // this launch's number on the sync block
  const int NU = p.NU;
  const int cluster = (info >> 5) * (32 / NU) + (info & 31) / NU, me = (info & 31) % NU;
  const int r0 = p.row0 + cluster * p.Mc;
  const int rend = min(p.row0 + p.nrows, r0 + p.Mc);
  if (r0 >= rend) return;
  unsigned* flags = p.sync + kSyncFlags + cluster * 32;
  const int u0 = me * 16, uq = u0 + q * 4;
  const int B = p.B, T = p.T;
  {
    ClGateMap gm{H, u0};
#pragma unroll
    for (int l = 0; l < L; ++l) {
      glds_tile<u16, 64, HC>(Wl + (2 * l) * W_BYTES, p.w_hh[l], H, 0, 0, gm, 0, tid);
      if (l > 0) glds_tile<u16, 64, HC>(Wl + (2 * l - 1) * W_BYTES, p.w_ih[l], H, 0, 0, gm, 0, tid);
    }
  }
  const int row = r0 + rt * 16 + r;
  const int64_t rowc = row < rend ? row : rend - 1;
  const bool epi = kp < L;  // this wave finishes layer kp of its row tile
  f32x4 bias[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    bias[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (epi && (kp > 0 || !p.pre)) bias[g] = *(const f32x4*)(p.b_ih[kp] + g * H + uq) + *(const f32x4*)(p.b_hh[kp] + g * H + uq);
  }
  // the time-constant input's projection (p.xcv): once, by the wave that finishes layer 0, into a constant added to its gates
  f32x4 pxc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) pxc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p.xcv && kp == 0) {
    const int nkc = (p.Ic + 31) / 32, nchc = p.Ic / 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // Ic <= 128
      if (j >= nkc) break;
      const int c = j * 4 + q;
      uint4 xf = uint4{0u, 0u, 0u, 0u};
      if (c < nchc) xf = *(const uint4*)(p.xcv + rowc * p.Ic + c * 8);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint4 wf = uint4{0u, 0u, 0u, 0u};
        if (c < nchc) wf = *(const uint4*)(p.w_ih0 + (int64_t)(g * H + u0 + r) * p.K0 + p.I + c * 8);
        pxc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, xf), pxc[g], 0, 0, 0);
      }
    }
  }
  f32x4 creg = f32x4{0.f, 0.f, 0.f, 0.f};
  auto pack4 = [](const f32x4& v) -> uint2 {
    return uint2{(uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16), (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16)};
  };
  // folded input projection: W_ih[0] fragments of this wave's k-steps (j = kp, kp + KSP, ...) stay in registers
  constexpr int KSXW = (4 + KSP - 1) / KSP;  // up to 128 input features
  const bool fold = p.x != nullptr;
  const int nchx = p.I / 8;
  uint4 wx[4][KSXW];
#pragma unroll
  for (int jj = 0; jj < KSXW; ++jj) {
    const int c = (kp + jj * KSP) * 4 + q;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (fold && c < nchx) v = *(const uint4*)(p.w_ih0 + (int64_t)(g * H + u0 + r) * p.K0 + c * 8);
      wx[g][jj] = v;
    }
  }
  uint4 xn[KSXW];
  auto load_x = [&](int t) {
#pragma unroll
    for (int jj = 0; jj < KSXW; ++jj) {
      const int c = (kp + jj * KSP) * 4 + q;
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (fold && c < nchx) v = *(const uint4*)(p.x + ((int64_t)t * B + rowc) * p.I + c * 8);
      xn[jj] = v;
    }
  };
  load_x(0);
  const __amdgpu_buffer_rsrc_t hs_rs = make_rsrc(p.xch);
  unsigned long long* tl = (p.tlog && cluster == 0 && me == 0) ? p.tlog : nullptr;
  __syncthreads();  // weights have landed

  const int nsteps = T + L - 1;
  for (int s = 0; s < nsteps; ++s) {
    CL_TLOG(s * 8 + 0);
    f32x4 padd[4];
    if (kp == 0 && s < T && p.pre) {
      const float* pp = p.pre + (int64_t)s * p.pre_tstride + rowc * (4 * H) + uq;
#pragma unroll
      for (int g = 0; g < 4; ++g) padd[g] = *(const f32x4*)(pp + g * H);
    }
    uint4 xc[KSXW];  // this wave's k-steps of x_s (folded input projection), fetched during step s-1
#pragma unroll
    for (int jj = 0; jj < KSXW; ++jj) xc[jj] = xn[jj];
    if (s > 0 && !cluster_wait(p.sync, flags, NU, ep0 + (unsigned)s)) return;
    CL_TLOG(s * 8 + 1);

    uint4 a[L][KPW];
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const int tau = s - l - 1;
      if (tau < 0 || tau >= T) continue;
      const int64_t base = (xch_off((s - 1) & 1, l, L, KS, kp * KPW, B, rowc) + q * 8) * 2;
#pragma unroll
      for (int j = 0; j < KPW; ++j) a[l][j] = load_sc1(hs_rs, base + j * (B * 64));
    }
    f32x4 acc[L][4];
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[l][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the weight fragments do not depend on the exchange: all those of a source are requested together while the exchange
    // loads are in flight (a read in front of every MFMA exposed an LDS round trip per MFMA: a wave is alone on its SIMD)
    bf16x8 wh[L][KPW][4], wu[L][KPW][4];
    auto wfrags = [&](int l) {
      const char* Whh = Wl + (2 * l) * W_BYTES;
      const char* Wih = Wl + (2 * l + 1) * W_BYTES;
#pragma unroll
      for (int j = 0; j < KPW; ++j) {
        const int kc = ((kp * KPW + j) << 2) | q;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          wh[l][j][g] = __builtin_bit_cast(bf16x8, *(const uint4*)(Whh + kc_off<HC>(g * 16 + r, kc)));
          if (l + 1 < L) wu[l][j][g] = __builtin_bit_cast(bf16x8, *(const uint4*)(Wih + kc_off<HC>(g * 16 + r, kc)));
        }
      }
    };
    wfrags(0);
    __builtin_amdgcn_sched_barrier(0);
    if (fold && s < T) {
#pragma unroll
      for (int jj = 0; jj < KSXW; ++jj)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          acc[0][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wx[g][jj]), __builtin_bit_cast(bf16x8, xc[jj]), acc[0][g], 0,
                                                              0, 0);
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
      if (l + 1 < L) wfrags(l + 1);  // the next source's fragments fly under this one's MFMAs
      const int tau = s - l - 1;
      if (tau < 0 || tau >= T) continue;
      const bool rec = s - l < T;
#pragma unroll
      for (int j = 0; j < KPW; ++j) {
        const bf16x8 av = __builtin_bit_cast(bf16x8, a[l][j]);
        if (rec) {
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[l][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[l][j][g], av, acc[l][g], 0, 0, 0);
        }
        if (l + 1 < L) {
          constexpr int kTop = L - 1;
          const int lu = l + 1 < L ? l + 1 : kTop;
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[lu][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wu[l][j][g], av, acc[lu][g], 0, 0, 0);
        }
      }
    }
    if (s + 1 < T) load_x(s + 1);  // (HBM: must not sit in front of the next flag poll)
    // partial tiles -> LDS, then wave (rt, l) sums the KSP parts of layer l
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
      for (int g = 0; g < 4; ++g) *(f32x4*)(Part + ((wave * L + l) * 4 + g) * 1024 + lane * 16) = acc[l][g];
    __syncthreads();
    CL_TLOG(s * 8 + 2);
    const int t = s - kp;
    const bool act = epi && t >= 0 && t < T;
    uint2 gpk[4];
    f32x4 hreg;
    if (act) {
      f32x4 gv[4], c;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        gv[g] = ((kp == 0 && p.pre) ? padd[g] : bias[g]) + pxc[g];
#pragma unroll
        for (int k = 0; k < KSP; ++k) gv[g] += *(const f32x4*)(Part + (((rt * KSP + k) * L + kp) * 4 + g) * 1024 + lane * 16);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ig = sigmoidf_(gv[0][i]), fg = sigmoidf_(gv[1][i]), gg = tanhf_(gv[2][i]), og = sigmoidf_(gv[3][i]);
        c[i] = __builtin_fmaf(fg, creg[i], ig * gg);
        hreg[i] = og * tanhf_(c[i]);
        gv[0][i] = ig, gv[1][i] = fg, gv[2][i] = gg, gv[3][i] = og;
      }
      creg = c;
#pragma unroll
      for (int g = 0; g < 4; ++g) gpk[g] = pack4(gv[g]);
      if (row < rend) {
        const uint2 hp = pack4(hreg);
        *(uint2*)(p.xch + xch_off(s & 1, kp, L, KS, uq >> 5, B, row) + (uq & 31)) = hp;  // what the members wait for
        *(uint2*)(p.hs + (((int64_t)kp * T + t) * B + row) * H + uq) = hp;
      }
    }
    CL_TLOG(s * 8 + 3);
    if (s + 1 < nsteps) cluster_publish(flags, me, ep0 + (unsigned)(s + 1));  // (its barrier also frees Part)
    CL_TLOG(s * 8 + 4);
    if (act && row < rend) {
      const int64_t lt = (int64_t)kp * T + t;
      if constexpr (kSave) {
        *(f32x4*)(p.cs + (lt * B + row) * H + uq) = creg;
        cl_store_gates(p.gates + (lt * B + row) * (4 * H), uq, gpk);
      }
      if (kp == L - 1 && p.hs_top_f32) *(f32x4*)(p.hs_top_f32 + ((int64_t)t * B + row) * H + uq) = hreg;
      if (p.hn && t == T - 1) {
        *(f32x4*)(p.hn + (int64_t)row * (L * H) + kp * H + uq) = hreg;
        if (p.hn_lp) *(uint2*)(p.hn_lp + (int64_t)row * (L * H) + kp * H + uq) = pack4(hreg);  // (fhvae_lstm_desc.hn_lp)
      }
    }
  }
