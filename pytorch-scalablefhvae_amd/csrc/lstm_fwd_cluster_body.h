// lstm_fwd_cluster_body.h -- the body of lstm_fwd_cluster_kernel and of its inference twin, included INSIDE both kernels (it is not a header of its
// own): the training kernel then compiles to the very instructions it had as a single function.  `kSave` is a constexpr of
// the including kernel; false = fhvae_lstm_seq_infer: nothing that only the backward reads leaves the kernel.
  using CF = ClFwdCfg<H, L, RB>;
  constexpr int HC = CF::HC, TM = CF::TM, PCH = CF::PCH, NPP = CF::NPP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Wl = smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  char* ring = smem + CF::NW * CF::W_BYTES + wave * (kRing * kPanel);  // this wave's staging ring
  const int r = lane & 15, q = lane >> 4;

  const int joined = cluster_join(p.sync, (int*)(smem + CF::NW * CF::W_BYTES));  // (the rings are idle until step 1)
  if (joined < 0) return;
  const int info = joined & 255;                                 // XCD * 32 + slot
  const unsigned ep0 = (unsigned)(joined >> 8) * kSeqEpochs;     // this launch's number on the sync block
  const int NU = p.NU;
  const int cluster = (info >> 5) * (32 / NU) + (info & 31) / NU, me = (info & 31) % NU;
  const int r0 = p.row0 + cluster * p.Mc;
  const int rend = min(p.row0 + p.nrows, r0 + p.Mc);
  if (r0 >= rend) return;  // the whole cluster leaves: nobody waits for it
  unsigned* flags = p.sync + kSyncFlags + cluster * 32;
  const int u0 = me * 16;
  const int B = p.B, T = p.T;

  // ---- weights of this workgroup's 64 gate columns -> LDS, once
  {
    ClGateMap gm{H, u0};
#pragma unroll
    for (int l = 0; l < L; ++l) {
      glds_tile<u16, 64, HC>(Wl + (2 * l) * CF::W_BYTES, p.w_hh[l], H, 0, 0, gm, 0, tid);
      if (l > 0) glds_tile<u16, 64, HC>(Wl + (2 * l - 1) * CF::W_BYTES, p.w_ih[l], H, 0, 0, gm, 0, tid);
    }
  }
  // MFMA roles: the WEIGHT fragment is the first operand, the h fragment the second, so the 16x16 result has the
  // hidden unit on (lane>>4)*4 + reg and the batch row on lane&15: a lane owns i,f,g,o of FOUR CONSECUTIVE units of one
  // row -> every f32 output leaves as one 16-byte store, every bf16 output as one 8-byte store
  const int uq = u0 + q * 4;  // first of this lane's 4 units
  f32x4 bias[L][4];
#pragma unroll
  for (int l = 0; l < L; ++l)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bias[l][g] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (l > 0) bias[l][g] = *(const f32x4*)(p.b_ih[l] + g * H + uq) + *(const f32x4*)(p.b_hh[l] + g * H + uq);
    }

  if (!p.pre) {  // no time-constant input: layer 0's additive term is its two biases
#pragma unroll
    for (int g = 0; g < 4; ++g) bias[0][g] = *(const f32x4*)(p.b_ih[0] + g * H + uq) + *(const f32x4*)(p.b_hh[0] + g * H + uq);
  }
  const int wrow0 = wave * (TM * 16);       // first cluster row of this wave
  const bool wact = wrow0 < RB;             // waves beyond the tile only help staging
  f32x4 creg[L][TM];
#pragma unroll
  for (int l = 0; l < L; ++l)
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) creg[l][tm] = f32x4{0.f, 0.f, 0.f, 0.f};
  ClRowMap arm{r0, rend - 1};
  auto pack4 = [](const f32x4& v) -> uint2 {
    return uint2{(uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16), (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16)};
  };

  unsigned long long* tl = (p.tlog && cluster == 0 && me == 0) ? p.tlog : nullptr;
  // what only the backward / the caller reads (c, the activated gates, the f32 copy of the top h): stored after the publish.
  // (Deferring these stores into the next step's contraction was measured slower: they queue in front of its operand
  // loads, 246 -> 269 us per net at B = 2048.)
  uint2 gpk[L][TM][4];  // activated gates, packed bf16
  f32x4 hreg[L][TM];
  auto tail_stores = [&](int sp) {
    if (!wact) return;
#pragma unroll
    for (int ll = 0; ll < L; ++ll) {
      const int t = sp - ll;
      if (t < 0 || t >= T) continue;
      const int64_t lt = (int64_t)ll * T + t;
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const int row = r0 + wrow0 + tm * 16 + r;
        if (row >= rend) continue;
        if constexpr (kSave) {
          *(f32x4*)(p.cs + (lt * B + row) * H + uq) = creg[ll][tm];
          cl_store_gates(p.gates + (lt * B + row) * (4 * H), uq, gpk[ll][tm]);
        }
        if (ll == L - 1 && p.hs_top_f32) *(f32x4*)(p.hs_top_f32 + ((int64_t)t * B + row) * H + uq) = hreg[ll][tm];
        if (p.hn && t == T - 1) {
          *(f32x4*)(p.hn + (int64_t)row * (L * H) + ll * H + uq) = hreg[ll][tm];
          if (p.hn_lp) *(uint2*)(p.hn_lp + (int64_t)row * (L * H) + ll * H + uq) = pack4(hreg[ll][tm]);  // (fhvae_lstm_desc.hn_lp)
        }
      }
    }
  };
  f32x4 pnext[TM][4];
  const bool pvar = p.pre && p.pre_tstride != 0;  // a different additive term every step (unfolded input projection)
  auto load_pre = [&](int t) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int row = r0 + wrow0 + tm * 16 + r;
      const float* pp = p.pre + (int64_t)t * p.pre_tstride + (int64_t)(row < rend ? row : rend - 1) * (4 * H) + uq;
#pragma unroll
      for (int g = 0; g < 4; ++g) pnext[tm][g] = (wact && p.pre) ? *(const f32x4*)(pp + g * H) : bias[0][g];
    }
  };
  load_pre(0);
  if (p.xcv) {  // the time-constant input's projection, once: same fragment roles as the folded x projection below
    const int nkc = (p.Ic + 31) / 32, nchc = p.Ic / 8;
    f32x4 accx[TM][4];
    zero_acc(accx);
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // Ic <= 128
      if (j >= nkc) break;
      const int c = j * 4 + q;
      const bool ok = c < nchc;
      uint4 xf[TM];
#pragma unroll
      for (int tm = 0; tm < TM; ++tm) {
        const int row = r0 + wrow0 + tm * 16 + r;
        xf[tm] = uint4{0u, 0u, 0u, 0u};
        if (ok && wact) xf[tm] = *(const uint4*)(p.xcv + (int64_t)(row < rend ? row : rend - 1) * p.Ic + c * 8);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint4 wf = uint4{0u, 0u, 0u, 0u};
        if (ok) wf = *(const uint4*)(p.w_ih0 + (int64_t)(g * H + u0 + r) * p.K0 + p.I + c * 8);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
          accx[tm][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, xf[tm]), accx[tm][g], 0, 0, 0);
      }
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
      for (int g = 0; g < 4; ++g) pnext[tm][g] += accx[tm][g];
  }
  // folded input projection: this member's W_ih[0] fragments (gate g, k-step j) stay in registers for the whole launch;
  // the x fragments of step s+1 are fetched under the epilogue of step s (x comes from HBM, like `pre`)
  constexpr int KSX = 4;  // up to 128 input features
  const bool fold = p.x != nullptr;
  const int nkx = fold ? (p.I + 31) / 32 : 0, nchx = p.I / 8;
  uint4 wx[4][KSX], xn[TM][KSX];
#pragma unroll
  for (int j = 0; j < KSX; ++j) {
    const int c = j * 4 + q;
    const bool ok = fold && c < nchx;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (ok) v = *(const uint4*)(p.w_ih0 + (int64_t)(g * H + u0 + r) * p.K0 + c * 8);
      wx[g][j] = v;
    }
  }
  auto load_x = [&](int t) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
      const int row = r0 + wrow0 + tm * 16 + r;
      const u16* xp = p.x + ((int64_t)t * B + (row < rend ? row : rend - 1)) * p.I;
#pragma unroll
      for (int j = 0; j < KSX; ++j) {
        const int c = j * 4 + q;
        uint4 v = uint4{0u, 0u, 0u, 0u};
        if (fold && wact && c < nchx) v = *(const uint4*)(xp + c * 8);
        xn[tm][j] = v;
      }
    }
  };
  load_x(0);
  const int nsteps = T + L - 1;
  for (int s = 0; s < nsteps; ++s) {
    CL_TLOG(s * 8 + 0);
    // (1) layer 0's additive term for t = s was fetched during step s-1 (it comes from HBM: loads return in order, so
    //     fetching it here would put its latency in front of the flag poll)
    f32x4 padd[TM][4];
    uint4 xc[TM][KSX];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
      for (int g = 0; g < 4; ++g) padd[tm][g] = pnext[tm][g];
#pragma unroll
      for (int j = 0; j < KSX; ++j) xc[tm][j] = xn[tm][j];
    }
    // (2) h of step s-1 from every member
    if (s > 0 && !cluster_wait(p.sync, flags, NU, ep0 + (unsigned)s)) return;

    CL_TLOG(s * 8 + 1);
    // (3) contraction: sources l with tau = s-l-1 in [0,T): h^l_tau feeds layer l (recurrent) and layer l+1 (input)
    f32x4 acc[L][TM][4];
#pragma unroll
    for (int l = 0; l < L; ++l) zero_acc(acc[l]);
    f32x4 g0v[TM][4];   // layer 0's pre-activations, then its activated gates (interleaved form)
    bool did0 = false;  // layer 0's gate math already ran inside the contraction
    const int lo = s - T > 0 ? s - T : 0;
    const int hi = s - 1 < L - 1 ? s - 1 : L - 1;
    const int npan = hi >= lo ? (hi - lo + 1) * NPP : 0;
    auto issue = [&](int n) {
      const int l = lo + n / NPP, pp = n % NPP;
      const u16* src = p.hs + ((int64_t)(l * T + (s - l - 1)) * B) * H;
      glds_wave_panel<CF::WR, PCH>(ring + (n % kRing) * kPanel, src, H, pp * PCH * 8, arm, wrow0, lane);
    };
    if (wact) {
      for (int n = 0; n < kRing - 1 && n < npan; ++n) issue(n);
      if (fold && s < T) {  // layer 0's input projection for t = s, while the first panels are landing
#pragma unroll
        for (int j = 0; j < KSX; ++j) {
          if (j >= nkx) break;
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
              acc[0][tm][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wx[g][j]), __builtin_bit_cast(bf16x8, xc[tm][j]),
                                                                      acc[0][tm][g], 0, 0, 0);
        }
      }
      // L = 2, both sources present (every step from s = 2 on): the h^1 panels are multiplied by an unrolled loop below that
      // carries layer 0's gate math between its MFMAs (layer 0's accumulators are final once the h^0 panels are done)
      const bool two = L == 2 && hi > lo && p.il;
      const int npan_a = two ? NPP : npan;
      for (int n = 0; n < npan_a; ++n) {
        wait_panels(npan - 1 - n < kRing - 2 ? npan - 1 - n : kRing - 2);  // panel n has landed
        if (n + kRing - 1 < npan) issue(n + kRing - 1);  // into the slot consumed one iteration ago
        const int l = lo + n / NPP, pp = n % NPP;
        const char* As = ring + (n % kRing) * kPanel;
        {
          // one panel of source ll: every fragment of a k-step (TM of h, 4 of W_hh[ll], 4 of W_ih[ll+1]) is requested before
          // its MFMAs -- ONE LDS round trip per k-step (a read per MFMA pair costs 8: a wave is alone on its SIMD, nothing
          // hides that latency); REC = layer ll itself is active at this step
          auto panel = [&](auto ll_c, auto rec_c) {
            constexpr int ll = decltype(ll_c)::value;
            constexpr bool REC = decltype(rec_c)::value;
            constexpr bool UP = ll + 1 < L;
            constexpr int lu = UP ? ll + 1 : L - 1;
            const char* Whh = Wl + (2 * ll) * CF::W_BYTES;
            const char* Wih = Wl + (2 * ll + 1) * CF::W_BYTES;  // of layer ll+1 (exists when UP)
            constexpr int NJ = PCH / 4, NB = (REC ? 4 : 0) + (UP ? 4 : 0);
            bf16x8 a[2][TM], bh[2][4], bu[2][4];
            auto frags = [&](int j, int buf) {
              const int kc = pp * PCH + ((j << 2) | q);
#pragma unroll
              for (int tm = 0; tm < TM; ++tm)
                a[buf][tm] = __builtin_bit_cast(bf16x8, *(const uint4*)(As + kc_off<PCH>(tm * 16 + r, (j << 2) | q)));
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                if constexpr (REC) bh[buf][g] = __builtin_bit_cast(bf16x8, *(const uint4*)(Whh + kc_off<HC>(g * 16 + r, kc)));
                if constexpr (UP) bu[buf][g] = __builtin_bit_cast(bf16x8, *(const uint4*)(Wih + kc_off<HC>(g * 16 + r, kc)));
              }
            };
            frags(0, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, TM + NB, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
              if (j + 1 < NJ) frags(j + 1, (j + 1) & 1);  // the next k-step's fragments fly under this one's MFMAs
#pragma unroll
              for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                  if constexpr (REC) acc[ll][tm][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh[j & 1][g], a[j & 1][tm], acc[ll][tm][g], 0, 0, 0);
                  if constexpr (UP) acc[lu][tm][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bu[j & 1][g], a[j & 1][tm], acc[lu][tm][g], 0, 0, 0);
                }
              if (j + 1 < NJ) {
#pragma unroll
                for (int i = 0; i < TM + NB; ++i) {
                  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                  __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, TM * NB - (TM + NB), 0);
              } else {
                __builtin_amdgcn_sched_group_barrier(0x008, TM * NB, 0);
              }
            }
          };
          if (l == 0) {
            if (s < T)
              panel(std::integral_constant<int, 0>{}, std::true_type{});
            else
              panel(std::integral_constant<int, 0>{}, std::false_type{});
          }
          if constexpr (L > 1) {
            if (l == 1) {
              if (s - 1 < T)
                panel(std::integral_constant<int, 1>{}, std::true_type{});
              else
                panel(std::integral_constant<int, 1>{}, std::false_type{});
            }
          }
        }
      }
      if constexpr (L == 2) {
        if (two) {
          if (s < T) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
              for (int g = 0; g < 4; ++g) g0v[tm][g] = acc[0][tm][g] + padd[tm][g];
          }
          // chunk c = (tile c / 4, element c % 4) of layer 0's gate math: 10 transcendentals + the cell update of 1 (row, unit)
          auto g0_chunk = [&](int c) {
            const int tm = c >> 2, i = c & 3;
            const float ig = sigmoidf_(g0v[tm][0][i]), fg = sigmoidf_(g0v[tm][1][i]), gg = tanhf_(g0v[tm][2][i]), og = sigmoidf_(g0v[tm][3][i]);
            const float cn = __builtin_fmaf(fg, creg[0][tm][i], ig * gg);
            creg[0][tm][i] = cn;
            hreg[0][tm][i] = og * tanhf_(cn);
            g0v[tm][0][i] = ig, g0v[tm][1][i] = fg, g0v[tm][2][i] = gg, g0v[tm][3][i] = og;
          };
          auto second = [&](auto with_gates) {
            constexpr bool WG = decltype(with_gates)::value;
            constexpr int KS1 = NPP * (PCH / 4), NCH = TM * 4;  // k-steps of the h^1 source, gate chunks of layer 0
            const char* Whh = Wl + 2 * CF::W_BYTES;
#pragma unroll
            for (int pp = 0; pp < NPP; ++pp) {
              const int n = NPP + pp;
              wait_panels(2 * NPP - 1 - n < kRing - 2 ? 2 * NPP - 1 - n : kRing - 2);
              if (n + kRing - 1 < 2 * NPP) issue(n + kRing - 1);
              const char* As = ring + (n % kRing) * kPanel;
#pragma unroll
              for (int j = 0; j < PCH / 4; ++j) {
                bf16x8 a[TM], b[4];
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
                  a[tm] = __builtin_bit_cast(bf16x8, *(const uint4*)(As + kc_off<PCH>(tm * 16 + r, (j << 2) | q)));
                const int kc = pp * PCH + ((j << 2) | q);
#pragma unroll
                for (int g = 0; g < 4; ++g) b[g] = __builtin_bit_cast(bf16x8, *(const uint4*)(Whh + kc_off<HC>(g * 16 + r, kc)));
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                  for (int tm = 0; tm < TM; ++tm)
                    acc[1][tm][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[g], a[tm], acc[1][tm][g], 0, 0, 0);
                if constexpr (WG) {
                  const int kk = pp * (PCH / 4) + j;
#pragma unroll
                  for (int c = 0; c < NCH; ++c)
                    if (c >= kk * NCH / KS1 && c < (kk + 1) * NCH / KS1) g0_chunk(c);
                }
              }
            }
          };
          if (s < T) {
            second(std::true_type{});
            did0 = true;
          } else {
            second(std::false_type{});
          }
        }
      }
    }

    CL_TLOG(s * 8 + 2);
    if (s + 1 < T) {  // fly under the epilogue
      if (pvar) load_pre(s + 1);
      if (fold) load_x(s + 1);
    }
    // (4) gates + cell update for the active layers; h leaves first (it is what the other members wait for)
    if (wact) {
#pragma unroll
      for (int ll = 0; ll < L; ++ll) {
        const int t = s - ll;
        if (t < 0 || t >= T) continue;
        const int64_t lt = (int64_t)ll * T + t;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
          const int row = r0 + wrow0 + tm * 16 + r;
          if (ll == 0 && did0) {  // computed between the MFMAs of the h^1 panels
#pragma unroll
            for (int g = 0; g < 4; ++g) gpk[0][tm][g] = pack4(g0v[tm][g]);
            if (row < rend) *(uint2*)(p.hs + (lt * B + row) * H + uq) = pack4(hreg[0][tm]);
            continue;
          }
          f32x4 gv[4], c, h;
#pragma unroll
          for (int g = 0; g < 4; ++g) gv[g] = acc[ll][tm][g] + (ll == 0 ? padd[tm][g] : bias[ll][g]);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float ig = sigmoidf_(gv[0][i]), fg = sigmoidf_(gv[1][i]), gg = tanhf_(gv[2][i]), og = sigmoidf_(gv[3][i]);
            c[i] = __builtin_fmaf(fg, creg[ll][tm][i], ig * gg);  // (explicit: see tanhf_)
            h[i] = og * tanhf_(c[i]);
            gv[0][i] = ig, gv[1][i] = fg, gv[2][i] = gg, gv[3][i] = og;
          }
          creg[ll][tm] = c;
          hreg[ll][tm] = h;
#pragma unroll
          for (int g = 0; g < 4; ++g) gpk[ll][tm][g] = pack4(gv[g]);
          if (row < rend) *(uint2*)(p.hs + (lt * B + row) * H + uq) = pack4(h);
        }
      }
    }
    CL_TLOG(s * 8 + 3);
    // (5) publish step s (also the barrier that frees the staging buffers for the next step)
    if (s + 1 < nsteps) cluster_publish(flags, me, ep0 + (unsigned)(s + 1));
    CL_TLOG(s * 8 + 4);
    // (6) what only the backward reads.  Not free: 20 partial-line store instructions per wave and step cost the wave ~130 ns
    // each wherever they are issued -- as this burst (2.6 us before the next flag poll), all behind the next step's first
    // panel issues (228 us per launch against 204), or two or three behind every panel issue of the next step (226): the
    // panels queue behind them; or four behind each of the next step's last three panel waits, i.e. behind its last panel
    // issue and ~1.5 us ahead of the h stores (201 against 190, with the cl_goff layout): a wave whose store queue is full
    // stalls its MFMAs too.  Fewer, fuller stores are what helps (the gate layout, cl_goff).
    tail_stores(s);
  }
