"""The launch decisions of the three matrix-product kernels, mirrored in Python so that a CPU test can prove which compiled
branch a test shape reaches (tests/test_gemm_oracle_cpu.py checks the case tables of tests/test_gemm_oracle_gpu.py with it).
No imports: CPU and GPU tests share it.

These are MIRRORS: they can drift from the C++ they copy.  Each function names the C++ it mirrors, and each mirrored site
carries a comment naming this file; whoever changes one changes the other.  Every floating-point expression keeps the C++
operand order (both sides are IEEE doubles), so the cost models choose the same minimum."""


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# csrc/proj.hip
# ---------------------------------------------------------------------------------------------
PROJ_BMS = (64, 96, 128, 160, 192, 224, 256)  # the explicit instantiations of proj_kernel<BM, BN>, BN in (128, 256)


def proj_plan(M, N):
    """(BM, BN, tiles) of fhvae_proj_bf16 -- launch_proj in csrc/proj.hip: `BN = N > 128 ? 256 : 128`, then the loop
    `for (bm = 64; bm <= 256; bm += 32)` minimising `cdiv(tiles, 256) * (bm + 24)` with a strict `<` (the smallest BM wins a
    tie)."""
    BN = 256 if N > 128 else 128
    ncol = cdiv(N, BN)
    best, best_t = 256, 1e30
    for bm in range(64, 257, 32):
        tiles = cdiv(M, bm) * ncol
        t = float(cdiv(tiles, 256) * (bm + 24))
        if t < best_t:
            best_t, best = t, bm
    return best, BN, cdiv(M, best) * ncol


# ---------------------------------------------------------------------------------------------
# csrc/wgrad.hip
# ---------------------------------------------------------------------------------------------
WG_BM, WG_MAX_PROBLEMS = 256, 16  # kWgBM, kMaxWgProblems


def wgrad_elem(bf16):
    """(BK, rate) of the element traits WgBf16 / WgF32 (csrc/wgrad.hip)."""
    return (64, 1.0e15) if bf16 else (32, 140.0e12)


def wgrad_class_plan(problems, BN, bf16):
    """One launch of launch_class<T, BN> (csrc/wgrad.hip) over at most kMaxWgProblems problems of one tile class.
    problems: (K, M, N) or (K, M, N, c) with c any value naming the output matrix (equal c = the same C: shared_c).
    Returns (BN, sk, grid, per) with per[i] a dict: m_tiles, n_tiles, splitk, ksteps_per, last (k-steps of the last slice),
    ktail (K % BK), ks_total, clipped (the group's sk exceeded ks_total / 2), shared_c, atomic (the epilogue's `splitk == 1 &&
    !shared_c` test fails), remap (the kernel's XCD remap `nb >= 16` applies to this launch)."""
    BK, rate = wgrad_elem(bf16)
    assert 0 < len(problems) <= WG_MAX_PROBLEMS
    tiles, ks_max = 0, 1
    for p in problems:
        K, M, N = p[:3]
        tiles += cdiv(M, WG_BM) * cdiv(N, BN)
        ks_max = max(ks_max, cdiv(K, BK))
    # `t_step = 2.0 * kWgBM * BN * E::BK / (E::kRate / 256), tile_bytes = 4.0 * kWgBM * BN`
    t_step = 2.0 * WG_BM * BN * BK / (rate / 256)
    tile_bytes = 4.0 * WG_BM * BN
    sk, best = 1, 1e30
    c = 1
    while c <= 64 and c * 2 <= ks_max:  # `for (c = 1; c <= 64 && c * 2 <= ks_max; ++c)`
        waves = float(cdiv(tiles * c, 256))
        steps = float(cdiv(ks_max, c)) + 2.0
        t = waves * steps * t_step + ((tiles * c) * tile_bytes / 1.3e12 if c > 1 else 0.0)
        if t < best:
            best, sk = t, c
        c += 1
    per, grid = [], 0
    for p in problems:
        K, M, N = p[:3]
        ks_total = cdiv(K, BK)
        s = sk
        clipped = s > ks_total // 2
        if clipped:
            s = ks_total // 2
        if s < 1:
            s = 1
        ksteps_per = cdiv(ks_total, s)
        splitk = cdiv(ks_total, ksteps_per)
        d = {"m_tiles": cdiv(M, WG_BM), "n_tiles": cdiv(N, BN), "splitk": splitk, "ksteps_per": ksteps_per,
             "last": ks_total - (splitk - 1) * ksteps_per, "ktail": K % BK, "ks_total": ks_total, "clipped": clipped and sk > 1}
        grid += d["m_tiles"] * d["n_tiles"] * splitk
        per.append(d)
    for i, p in enumerate(problems):  # `if (a != b && g.p[a].C == g.p[b].C) g.p[a].shared_c = 1`
        per[i]["shared_c"] = len(p) > 3 and any(j != i and len(q) > 3 and q[3] == p[3] for j, q in enumerate(problems))
        per[i]["atomic"] = not (per[i]["splitk"] == 1 and not per[i]["shared_c"])
    for d in per:
        d["remap"] = grid >= 16
    return BN, sk, grid, per


def wgrad_plan(problems, bf16):
    """Every launch of launch_wgrad (csrc/wgrad.hip) for one call, in launch order: the problems with N > 128 (BN = 256) in
    chunks of kMaxWgProblems, then the others (BN = 128).  A list of (BN, sk, grid, per, which): wgrad_class_plan's tuple plus
    the indices of the chunk's problems in `problems`.  A stand-alone call (fhvae_wgrad_bf16 / fhvae_wgrad_f32) is one problem."""
    wide = [i for i, p in enumerate(problems) if p[2] > 128]
    narrow = [i for i, p in enumerate(problems) if p[2] <= 128]
    out = []
    for BN, idx in ((256, wide), (128, narrow)):
        for at in range(0, len(idx), WG_MAX_PROBLEMS):
            which = idx[at:at + WG_MAX_PROBLEMS]
            out.append(wgrad_class_plan([problems[i] for i in which], BN, bf16) + (which,))
    return out


def wgrad_desc_ok(K, M, N, lda, ldb, ldc, a_col0=0, bf16=True):
    """wgrad_eligible (csrc/wgrad.hip) + wg_from_desc's `ldc >= N` (csrc/lstm.hip), 16-byte aligned bases assumed."""
    es = 2 if bf16 else 4
    max_bytes = (1 << 30) if bf16 else 0x7ffffff0
    if M <= 0 or N <= 0 or K <= 0 or a_col0 < 0:
        return False
    if lda % (16 // es) or ldb % (16 // es) or lda < a_col0 + M or ldb < N:
        return False
    if K * lda * es >= max_bytes or K * ldb * es >= max_bytes:
        return False
    return ldc >= N


# ---------------------------------------------------------------------------------------------
# csrc/gemm.hip (the generic engine of csrc/gemm_core.h)
# ---------------------------------------------------------------------------------------------
def auto_splitk(tiles, panels):
    """auto_splitk in csrc/gemm.hip."""
    if tiles >= 192 or panels < 4:
        return 1
    s = cdiv(512, tiles)
    if s > panels // 2:
        s = panels // 2
    return max(1, min(s, 128))


def gemm_plan(M, N, K, a_kc, b_kc, lda, ldb, auto=False, dtype="f32", ldc=None):
    """launch_gemm + launch_fast (csrc/gemm.hip) for one K segment, 16-byte aligned bases, mode 0 / 1 on entry
    (auto: splitk == 0 with mode 1, the weight gradients).  "slow" (gemm_slow_kernel: seg_fast_ok of csrc/gemm_core.h fails, or
    bf16 with mixed orientations) or a tuple (tile, CH, splitk, tiles, kernel, dma_tiles, vec):
      tile       (BM, BN);  CH: 16-byte chunks per panel row (BK = CH * EPC contraction elements)
      tiles      output tiles (grid.x * grid.y)
      kernel     "swap+dma" (gemm_kernel<..., DMA, SWAP>: `CH == 32 && BM == 64 && splitk == 1 && tiles <= 256`), "swap"
                 (`splitk == 1 && mode != 2`, KC/KC), "plain" (the unswapped kernel: split-K atomics, KM or mixed operands)
      dma_tiles  tiles whose main loop is mainloop_glds (gemm_tile's `dma`: interior tile and K % BK == 0), 0 unless swap+dma
      vec        the swapped epilogue stores 16 bytes (gemm_tile's `vec`: ldc % 4 == 0 && N % 4 == 0); None when not swapped"""
    bf = dtype == "bf16"
    epc = 8 if bf else 4
    ldc = N if ldc is None else ldc
    fast = lda % epc == 0 and ldb % epc == 0 and (K if a_kc else M) % epc == 0 and (K if b_kc else N) % epc == 0
    if bf and bool(a_kc) != bool(b_kc):
        fast = False
    if not fast:
        return "slow"
    if bf and auto and K >= 16384 and M >= 128 and not a_kc and not b_kc:  # the long-K bf16 weight gradient
        tiles = cdiv(M, 128) * cdiv(N, 64)
        sk = max(1, min(cdiv(512, tiles), cdiv(K, 128) // 2))
        return (128, 64), 16, sk, tiles, "plain", 0, None
    big = K > 16 * epc and cdiv(M, 128) * cdiv(N, 128) >= 512
    tb = 128 if big else 64
    ch = 16 if big else (8 if K <= 16 * epc else 32)
    tiles = cdiv(M, tb) * cdiv(N, tb)
    splitk = auto_splitk(tiles, cdiv(K, ch * epc)) if auto else 1
    atomics = splitk > 1  # `if (p.splitk > 1) p.mode = 2`
    kernel, dma_tiles, vec = "plain", 0, None
    if a_kc and b_kc:
        if ch == 32 and tb == 64 and splitk == 1 and tiles <= 256:
            kernel = "swap+dma"
            if K % (ch * epc) == 0:
                dma_tiles = (M // tb) * (N // tb)
        elif splitk == 1 and not atomics:
            kernel = "swap"
        if kernel != "plain":
            vec = ldc % 4 == 0 and N % 4 == 0
    return (tb, tb), ch, splitk, tiles, kernel, dma_tiles, vec


def linear_plans(M, K, N, relu, ldx, ldw, lddy):
    """The three contractions of hip_binding.raw_linear_fwd / raw_linear_bwd (fhvae_linear_fwd / fhvae_linear_bwd in
    csrc/gemm.hip), f32: y[M, N] (KC/KC), dx[M, K] over N (g KC, w KM), dw[N, K] over M (both KM, auto split).  With relu the
    upstream gradient is the masked copy (ld N), else dy itself."""
    ldg = N if relu else lddy
    return {"y": gemm_plan(M, N, K, 1, 1, ldx, ldw), "dx": gemm_plan(M, K, N, 1, 0, ldg, ldw, ldc=K),
            "dw": gemm_plan(N, K, M, 0, 0, ldg, ldx, auto=True, ldc=K)}
