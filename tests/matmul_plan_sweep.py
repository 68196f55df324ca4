"""The launch plans of the three matrix-product kernels, asked from the library (fhvae_plan_proj, fhvae_plan_wgrad,
fhvae_plan_gemm: host-only queries, nothing is launched and no operand is read; the descriptors carry invented, aligned
addresses), in two forms.  Only the two per-tile predicates that the generic kernel evaluates on the device (store_vec,
dma_tiles) are copies kept here:
  * proj_plan / wgrad_plan / gemm_plan / linear_plans / auto_splitk: one call's plan in the shape the oracle tests read
    (tests/test_gemm_oracle_cpu.py, tests/test_gemm_oracle_gpu.py);
  * cases() / rows() / digest(): a sweep with a value on each side of every boundary the C++ names, one canonical line per call,
    one SHA-256 per block.  tests/golden/matmul_plans.json holds the digests of the decisions as they were before the plans
    existed (written from the Python copies of the launch code that the tests used until then); it is never rewritten from the
    library.  tests/test_matmul_plan_cpu.py reproduces it and names the first differing lines of a block that does not."""
import ctypes as C
import functools
import hashlib
import itertools
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "matmul_plans.json")
P = 1 << 20  # a 16-byte aligned address; nothing is dereferenced
PROJ_BMS = (64, 96, 128, 160, 192, 224, 256)  # the explicit instantiations of proj_kernel<BM, BN>, BN in (128, 256)
WG_BM, WG_MAX_PROBLEMS = 256, 16              # kWgBM, kMaxWgProblems of csrc/wgrad.hip
VARIANTS = ("slow", "plain", "swap", "swap+dma", "plain", "group", "group once")  # fhvae_gemm_plan.variant (4: the long-K tile)
ORIENTS = ((1, 1), (0, 0), (1, 0), (0, 1))


@functools.lru_cache(None)
def library():
    import build_ext

    build_ext.build(verbose=False)
    import hip_binding as hb

    return hb.load_library(), hb


def cdiv(a, b):
    return -(-a // b)


def rup(n, m):
    return cdiv(n, m) * m


# ---------------------------------------------------------------------------------------------
# one call's plan
# ---------------------------------------------------------------------------------------------
def proj_plan(M, N):
    """(BM, BN, tiles) of fhvae_proj_bf16."""
    lib, hb = library()
    o = hb.ProjPlan()
    assert lib.fhvae_plan_proj(M, N, C.byref(o)) == 1
    return o.BM, o.BN, o.tiles


def wgrad_elem(bf16):
    """(BK, element size) of the element traits WgBf16 / WgF32."""
    return (64, 2) if bf16 else (32, 4)


def wgrad_descs(problems):
    """problems: (K, M, N) or (K, M, N, c), c any value naming the output matrix (equal c = the same C) -> [hb.WgradDesc] with
    padded leading dimensions (tests/test_gemm_oracle_gpu.py: wgrad_lds) and ldc = N."""
    names = {}
    return [library()[1].WgradDesc(P, rup(M, 8) + 8, 0, P, rup(N, 8) + 16, P * (2 + names.setdefault(c[0] if c else (i,), len(names))), N,
                                   M, N, K) for i, (K, M, N, *c) in enumerate(problems)]


def wgrad_launches(descs, bf16):
    """(return value, [hb.WgradPlan]) of fhvae_plan_wgrad."""
    lib, hb = library()
    out = (hb.WgradPlan * 32)()
    n = lib.fhvae_plan_wgrad((hb.WgradDesc * len(descs))(*descs), len(descs), hb.BF16 if bf16 else hb.F32, out, 32)
    return n, list(out[:max(n, 0)])


def wgrad_plan(problems, bf16):
    """Every launch of one call, in launch order: [(BN, sk, grid, per, which)], which = the indices of the launch's problems, per[i]
    the plan's m_tiles, n_tiles, splitk, ksteps_per, shared_c and what follows from them and K: ks_total, last (k-steps of the last
    slice), ktail (K % BK), clipped (the launch's sk exceeded ks_total / 2), atomic (the epilogue's `splitk == 1 && !shared_c`
    fails), remap (the kernel's XCD remap `nb >= 16` applies)."""
    BK = wgrad_elem(bf16)[0]
    n, launches = wgrad_launches(wgrad_descs(problems), bf16)
    assert n > 0, n
    out = []
    for l in launches:
        per = []
        for q in l.p[:l.n]:
            K = problems[q.which][0]
            d = {k: getattr(q, k) for k in ("m_tiles", "n_tiles", "splitk", "ksteps_per")}
            d.update(shared_c=bool(q.shared_c), ks_total=cdiv(K, BK), ktail=K % BK, remap=l.grid >= 16)
            d.update(last=d["ks_total"] - (q.splitk - 1) * q.ksteps_per, clipped=1 < l.sk > d["ks_total"] // 2,
                     atomic=not (q.splitk == 1 and not q.shared_c))
            per.append(d)
        out.append((l.BN, l.sk, l.grid, per, [q.which for q in l.p[:l.n]]))
    return out


def gemm_problem(M, N, segs, ldc=None, c_off=0, clp=False, splitk=1, mode=0):
    """One problem of fhvae_plan_gemm: segs = [(K, a_kc, b_kc, lda, ldb)] (one or two), c at P + c_off bytes."""
    return dict(M=M, N=N, segs=list(segs), ldc=N if ldc is None else ldc, c_off=c_off, clp=clp, splitk=splitk, mode=mode)


def gemm_launches(problems, dtype):
    """(return value, [hb.GemmPlan]) of fhvae_plan_gemm for one call of 1..kMaxGroup (or more) problems; dtype "f32" / "bf16"."""
    lib, hb = library()
    ds = (hb.GemmDesc * len(problems))()
    for d, p in zip(ds, problems):
        d.M, d.N, d.ldc, d.ldclp, d.splitk, d.mode = p["M"], p["N"], p["ldc"], p["N"], p["splitk"], p["mode"]
        d.c, d.clp = P + p["c_off"], (8 * P if p["clp"] else None)
        for s, (K, a_kc, b_kc, lda, ldb) in enumerate(p["segs"]):
            d.K[s], d.a_kc[s], d.b_kc[s], d.lda[s], d.ldb[s], d.a[s], d.b[s] = K, a_kc, b_kc, lda, ldb, 2 * P, 4 * P
    out = (hb.GemmPlan * len(problems))()
    n = lib.fhvae_plan_gemm(ds, len(problems), hb.BF16 if dtype == "bf16" else hb.F32, out)
    return n, list(out[:max(n, 0)])


def store_vec(p):
    """gemm_tile's `vec` (csrc/gemm.hip; mirrored: change both): the swapped epilogue stores 16 bytes (8 into the bf16 copy)."""
    return p["ldc"] % 4 == 0 and p["N"] % 4 == 0 and (P + p["c_off"]) % 16 == 0 and (not p["clp"] or p["N"] % 4 == 0)  # ldclp = N, clp aligned


def dma_tiles(l, p, dtype):
    """The tiles of a "swap+dma" launch whose gemm_tile `dma` holds (csrc/gemm.hip with seg_glds_ok of csrc/gemm_core.h; mirrored:
    change both): no K split, interior tiles, every live segment whole panels of KC rows with aligned leading dimensions (the
    operand bases of gemm_launches are aligned)."""
    epc = 8 if dtype == "bf16" else 4
    ok = l.splitk[0] == 1 and all(K == 0 or (a and b and K % (l.CH * epc) == 0 and lda % epc == 0 and ldb % epc == 0) for K, a, b, lda, ldb in p["segs"])
    return (p["M"] // l.BM) * (p["N"] // l.BN) if ok else 0


def gemm_plan(M, N, K, a_kc, b_kc, lda, ldb, auto=False, dtype="f32", ldc=None):
    """One problem of one K segment, mode 0 (auto: splitk == 0 with mode 1, the weight gradients).  "slow" (gemm_slow_kernel) or
    (tile, CH, splitk, tiles, kernel, dma_tiles, vec):
      tile       (BM, BN);  CH: 16-byte chunks per panel row;  tiles: output tiles (grid.x * grid.y)
      kernel     "swap+dma" (gemm_kernel<..., DMA, SWAP>), "swap", "plain" (the unswapped kernel)
      dma_tiles  tiles whose main loop is mainloop_glds (gemm_tile's `dma`)
      vec        the swapped epilogue stores 16 bytes (gemm_tile's `vec`); None when not swapped"""
    p = gemm_problem(M, N, [(K, a_kc, b_kc, lda, ldb)], ldc, splitk=0 if auto else 1, mode=int(auto))
    n, (l,) = gemm_launches([p], dtype)
    assert n == 1 and l.status == 0, (n, l.status)
    kernel = VARIANTS[l.variant]
    if kernel == "slow":
        return kernel
    return ((l.BM, l.BN), l.CH, l.splitk[0], l.grid[0] * l.grid[1], kernel, dma_tiles(l, p, dtype) if kernel == "swap+dma" else 0,
            store_vec(p) if kernel != "plain" else None)


def auto_splitk(tiles, panels):
    """The K slices an f32 weight gradient (KM/KM, auto) of `tiles` 64 x 64 tiles and `panels` 128-k panels gets."""
    pl = gemm_plan(64 * tiles, 64, 128 * panels, 0, 0, 64 * tiles, 64, auto=True)
    assert pl[0] == (64, 64) and pl[1] == 32 and pl[3] == tiles
    return pl[2]


def linear_plans(M, K, N, relu, ldx, ldw, lddy):
    """The three contractions of hip_binding.raw_linear_fwd / raw_linear_bwd (fhvae_linear_fwd / fhvae_linear_bwd in
    csrc/gemm.hip), f32: y[M, N] (KC/KC), dx[M, K] over N (g KC, w KM), dw[N, K] over M (both KM, auto split).  With relu the
    upstream gradient is the masked copy (ld N), else dy itself."""
    ldg = N if relu else lddy
    return {"y": gemm_plan(M, N, K, 1, 1, ldx, ldw), "dx": gemm_plan(M, K, N, 1, 0, ldg, ldw, ldc=K),
            "dw": gemm_plan(N, K, M, 0, 0, ldg, ldx, auto=True, ldc=K)}


# ---------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------
SETTINGS = ((1, 0), (1, 1), (1, 2), (0, 1), (0, 0), (4, 2))  # (splitk, mode) on entry: explicit, auto, auto without mode 1 (an error)
GEMM_MN = ((64, 64), (100, 70), (128, 64), (200, 136), (64 * 191, 64), (64 * 192, 64), (64 * 256, 64), (64 * 257, 64),
           (128 * 511, 128), (128 * 512, 128), (1024, 256))
#: (lda pad, ldb pad, ldc pad, byte offset of c, a bf16 copy of the output): tight, padded, each of lda / ldb / ldc / c misaligned
GEMM_LD = ((0, 0, 0, 0, 0), (8, 16, 4, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 4, 0), (0, 0, 0, 0, 1))


def gemm_ks(epc):
    """K at 16 epc and one element group either side, 3 / 4 and 10 / 11 panels of 32 chunks, 16384 -+ 8, clamped at 128 slices."""
    return (epc, 15 * epc, 16 * epc, 17 * epc, 96 * epc, 97 * epc, 320 * epc, 321 * epc, 16376, 16384, 9600 * epc)


def _single(dtype, M, N):
    epc = 8 if dtype == "bf16" else 4
    for K, (a_kc, b_kc), (sk, mode), (pa, pb, pc, off, clp) in itertools.product(gemm_ks(epc), ORIENTS, SETTINGS, GEMM_LD):
        yield dtype, [gemm_problem(M, N, [(K, a_kc, b_kc, (K if a_kc else M) + pa, (K if b_kc else N) + pb)], N + pc, off, bool(clp), sk, mode)]


def _two_segments():
    for dtype, (K0, K1), o0, o1, (sk, mode), (M, N) in itertools.product(("f32", "bf16"), ((64, 64), (256, 128), (0, 256), (256, 0), (132, 260)),
                                                                       ORIENTS, ORIENTS, ((1, 0), (0, 1)), ((128, 128), (64 * 192, 64))):
        yield dtype, [gemm_problem(M, N, [(K, a, b, K if a else M, K if b else N) for K, (a, b) in ((K0, o0), (K1, o1))], splitk=sk, mode=mode)]


def _groups():
    """Groups of 2 and kMaxGroup = 4 members that go out as one launch, and the same with one member, first or last, that forbids
    it for each reason of the loop; 1 and 5 members."""
    for dtype in ("f32", "bf16"):
        epc = 8 if dtype == "bf16" else 4

        def mem(M=256, N=128, K=512, o=(1, 1), pad=0, sk=1, mode=0, K1=0, o1=None):
            segs = [(K, o[0], o[1], (K if o[0] else M) + pad, K if o[1] else N)]
            if K1:
                segs.append((K1, o1[0], o1[1], K1 if o1[0] else M, K1 if o1[1] else N))
            return gemm_problem(M, N, segs, splitk=sk, mode=mode)

        for o in ORIENTS[:2 if dtype == "bf16" else 4]:
            good = [mem(o=o), mem(M=128, N=320, K=16 * epc + epc, o=o), mem(M=64, N=64, K=16384, o=o), mem(M=1024, N=64, K=2048, o=o)]
            auto = [mem(o=o, sk=0, mode=1), mem(M=64, N=64, K=96 * epc, o=o, sk=0, mode=1), mem(M=64, N=64, K=97 * epc, o=o, sk=0, mode=1),
                    mem(M=64, N=64, K=16384, o=o, sk=0, mode=1)]
            yield dtype, good[:1]
            yield dtype, good + good[:1]
            for n in (2, 4):
                yield dtype, good[:n]
                yield dtype, auto[:n]                                      # 768 workgroups over the group's tiles
                yield dtype, auto[1:3] + [mem(M=64 * 190, N=256, o=o)] * (n - 2)  # ... with many tiles: one slice; 3 / 4 panels
                yield dtype, good[:n - 1] + [mem(o=o, sk=2, mode=2)]       # an explicit split: not `once`
                yield dtype, good[:n - 1] + [mem(o=o, mode=2)]             # atomics without a split: not `once` either
                yield dtype, good[:n - 1] + [mem(o=o, sk=-3)]
                other = ORIENTS[1] if o == ORIENTS[0] else ORIENTS[0]
                bad = [mem(o=o, K1=256, o1=other), mem(o=o, pad=1), mem(o=o, K=16 * epc), mem(o=o, sk=0, mode=0), mem(o=o, K=16384 + epc),
                       mem(o=o, K=8192, K1=8192 + epc, o1=o), mem(o=ORIENTS[2]), mem(o=other), mem(M=0)]
                for b in bad:
                    yield dtype, good[:n - 1] + [b]
                    yield dtype, [b] + good[:n - 1]


#: wgrad problems (K, M, N[, c]): N at 128 / 129, ks_max at 1, 2, 128, 129 (of BK = 64 and 32), sk clipped by ks_total / 2
_WG_ONE = [(K, M, N) for N in (8, 128, 129, 256, 260) for M in (40, 256, 257, 1024) for K in (1, 32, 33, 64, 65, 128, 129, 4096, 4097, 8192, 8193, 8256, 40960)]
#: grid at 15 / 16: 15 and 16 tiles of one slice (K < 2 BK)
_WG_CALLS = [[(40, 256 * 15, 256)], [(40, 256 * 16, 256)], [(40, 256 * 15, 128)], [(40, 256 * 16, 128)], [(200, 256 * 5, 768)], [(200, 256 * 4, 1024)]]
_WG_CALLS += [[(300 + 10 * i, 64, 32, i) for i in range(n)] for n in (16, 17, 33)]                    # chunks of 16, 17, 33 problems
_WG_CALLS += [[(300 + 10 * i, 64, 132 if i % 3 else 32, i) for i in range(n)] for n in (17, 33, 40)]  # ... over both tile classes
_WG_CALLS += [[(512, 64, 32, 0 if i in (3, 9) else i) for i in range(20)],    # shared c inside the first chunk
              [(512, 64, 32, 0 if i in (3, 19) else i) for i in range(20)],   # ... across chunks: not shared within either launch
              [(512, 64, 32 if i != 3 else 200, 0 if i in (3, 9) else i) for i in range(20)],  # ... across the tile classes
              [(2048, 512, 256, "a"), (2048, 512, 256, "a"), (2048, 512, 256, "a")], [(4096, 1024, 512), (64, 256, 256), (100, 256, 256)]]


def _wg_eligibility():
    """(K, M, N, lda, ldb, ldc, a_col0, byte offsets of a, b): the boundaries of test_wgrad_desc_ok_at_its_boundaries for both
    element sizes, a NULL or misaligned base."""
    for es in (2, 4):
        e, kmax = 16 // es, ((1 << 30) if es == 2 else 0x7ffffff0)
        k_lim = cdiv(kmax, 512 * es)  # the first K with K * 512 * es >= the element's byte limit
        for K, M, N, lda, ldb in ((k_lim - 1, 256, 8, 512, 8), (k_lim, 256, 8, 512, 8), (k_lim - 1, 8, 256, 8, 512), (k_lim, 8, 256, 8, 512)):
            yield K, M, N, lda, ldb, N, 0, 0, 0
    for lda, col0 in ((80, 40), (72, 40), (79, 40), (80, 0), (84, 0), (80, -8), (76, 0)):
        yield 64, 40, 72, lda, 72, 72, col0, 0, 0
    for ldb, ldc in ((72, 71), (71, 72), (68, 72), (76, 72), (64, 72)):
        yield 64, 40, 72, 80, ldb, ldc, 0, 0, 0
    for a_off, b_off in ((8, 0), (0, 8), (-P, 0), (0, -P)):
        yield 64, 40, 72, 80, 72, 72, 0, a_off, b_off
    for K, M, N in ((0, 40, 72), (64, 0, 72), (64, 40, 0)):
        yield K, M, N, 80, 72, 72, 0, 0, 0


def cases():
    """{block: [case]} in the order of the golden file."""
    import test_gemm_oracle_gpu as G

    wg = [[p] for p in _WG_ONE + [c[:3] for c in G.WGRAD_CASES]] + _WG_CALLS + [list(g) for g in G.GROUPS.values()]
    wg.append([(G.PAIR["K"], G.PAIR["D"], G.PAIR["N"], i) for i in range(2)])
    proj_m = sorted({max(1, bm * 256 * r + d) for bm in PROJ_BMS for r in (1, 2) for d in (-1, 0, 1)} | {1, 63, 64, 65, 70000, 3 * 256 * 256 - 5})
    out = {"proj": [(M, N) for N in (4, 128, 129, 256, 257, 516) for M in proj_m],
           "wgrad bf16": [(c, True) for c in wg], "wgrad f32": [(c, False) for c in wg], "wgrad eligibility": list(_wg_eligibility())}
    out.update(("gemm %s %dx%d" % (dt, M, N), list(_single(dt, M, N))) for dt in ("f32", "bf16") for M, N in GEMM_MN)
    out.update({"gemm two segments": list(_two_segments()), "gemm groups": list(_groups())})
    return out


def _csv(*v):
    return ",".join(str(int(x)) for x in v)


def gemm_row(ret, launches, problems, dtype):
    """The plan's launches, then per problem of a swapped launch whether it stores 16 bytes and the launch's LDS-DMA tiles."""
    return "%d|" % ret + ";".join(_csv(l.first, l.n, l.status, l.variant, l.BM, l.BN, l.CH, l.akc, l.bkc, *l.grid, *l.splitk[:l.n], *l.mode[:l.n],
                                       *(l.variant in (2, 3, 6) and store_vec(p) for p in problems[l.first:l.first + l.n]),
                                       l.variant == 3 and dma_tiles(l, problems[l.first], dtype)) for l in launches)


def wgrad_row(ret, launches):
    return "%d|" % ret + ";".join(_csv(l.BN, l.sk, l.grid, l.n) + ":" + "/".join(
        _csv(q.which, q.m_tiles, q.n_tiles, q.ksteps_per, q.splitk, q.shared_c) for q in l.p[:l.n]) for l in launches)


def rows(block, cs):
    """The canonical lines of a block's cases, from the library."""
    lib, hb = library()
    if block == "proj":
        return [_csv(M, N, *proj_plan(M, N)) for M, N in cs]
    if block.startswith("wgrad b") or block.startswith("wgrad f"):
        return [wgrad_row(*wgrad_launches(wgrad_descs(c), bf16)) for c, bf16 in cs]
    if block == "wgrad eligibility":
        out = []
        for K, M, N, lda, ldb, ldc, col0, a_off, b_off in cs:
            d = hb.WgradDesc(P + a_off, lda, col0, P + b_off, ldb, P, ldc, M, N, K)
            out.append(_csv(lib.fhvae_wgrad_desc_ok(C.byref(d)), wgrad_launches([d], True)[0], wgrad_launches([d], False)[0]))
        return out
    return [gemm_row(*gemm_launches(ps, dtype), ps, dtype) for dtype, ps in cs]


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def load():
    with open(GOLDEN) as f:
        return json.load(f)
