"""Hierarchical sampling on a MI355X: the three kernels of csrc/hs.hip against numpy / float64 oracles and their status words,
encode_z2, one block of HierarchicalTrainer against a hand-written composition of the public pieces, --hip-graph across blocks,
train_model / eval_model end to end, and memory that depends on K, not on S."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_data_ckpt_cpu import corpus  # noqa: F401
from test_ops_gpu import close, hb  # noqa: F401


def _csr(S, seed, p_empty=0.2, hi=40):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, hi, size=S)
    counts[rng.random(S) < p_empty] = 0
    return counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _select(hb, ptr, block, cap):
    dev = torch.device("cuda")
    seg = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    loc = torch.full((cap,), -7, dtype=torch.int64, device=dev)
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    hb.hs_select(torch.from_numpy(ptr).to(dev), torch.as_tensor(block, dtype=torch.int64).to(dev), seg, loc, n, st)
    return seg.cpu().numpy(), loc.cpu().numpy(), int(n.item()), int(st.item())


@pytest.mark.parametrize("K", [1, 257, 5000])
def test_select_against_numpy(hb, K):
    S = 10000
    counts, ptr = _csr(S, K)
    rng = np.random.default_rng(K + 1)
    block = rng.choice(S, size=K, replace=False)  # (sequences with no segments included: they contribute nothing)
    want_seg = np.concatenate([np.arange(ptr[s], ptr[s + 1]) for s in block])
    want_loc = np.concatenate([np.full(counts[s], i) for i, s in enumerate(block)])
    cap = len(want_seg) + 5
    seg, loc, n, st = _select(hb, ptr, block, cap)
    assert st == 0 and n == len(want_seg)
    assert np.array_equal(seg[:n], want_seg) and np.array_equal(loc[:n], want_loc)
    assert (seg[n:] == -7).all() and (loc[n:] == -7).all()
    # a total above cap: the status bit, the true total, nothing written past cap
    cap2 = max(0, len(want_seg) - 3)
    seg2, loc2, n2, st2 = _select(hb, ptr, block, max(cap2, 1))
    if len(want_seg) > 1:
        assert st2 == hb.HS_CAP and n2 == len(want_seg)
        c = max(cap2, 1)
        assert np.array_equal(seg2[:c], want_seg[:c])


def test_select_errors_and_empty(hb):
    counts, ptr = _csr(100, 3)
    block = np.array([5, 100, 7])  # 100 is out of range
    seg, loc, n, st = _select(hb, ptr, block, 200)
    assert st & hb.HS_BAD_SEQ and n == counts[5] + counts[7]
    assert np.array_equal(seg[:n], np.concatenate([np.arange(ptr[5], ptr[6]), np.arange(ptr[7], ptr[8])]))
    _, _, n, st = _select(hb, ptr, np.array([-1]), 4)
    assert st == hb.HS_BAD_SEQ and n == 0
    empty = np.flatnonzero(counts == 0)[:3]
    seg, loc, n, st = _select(hb, ptr, empty, 4)
    assert st == 0 and n == 0 and (seg == -7).all()


def _runs(lengths, D, seed):
    rng = np.random.default_rng(seed)
    idx = np.repeat(np.arange(len(lengths)), lengths).astype(np.int64)
    z = rng.standard_normal((idx.shape[0], D)).astype(np.float32) * 3 + 1
    return idx, z


def _accumulate(hb, idx, z, K, chunks, status=None):
    dev = torch.device("cuda")
    zs = torch.zeros(K, z.shape[1], device=dev)
    cnt = torch.zeros(K, device=dev)
    st = status if status is not None else torch.zeros(1, dtype=torch.int32, device=dev)
    zt, it = torch.from_numpy(z).to(dev), torch.from_numpy(idx).to(dev)
    bounds = [0] + list(chunks) + [len(idx)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b > a:
            hb.mu2_accumulate_sorted(zt[a:b], it[a:b], zs, cnt, st)
    return zs, cnt, int(st.item())


@pytest.mark.parametrize("D", [8, 16, 32, 64])
def test_accumulate_sorted_oracle_and_bitwise(hb, D):
    rng = np.random.default_rng(D)
    lengths = rng.integers(1, 300, size=400)
    lengths[rng.random(400) < 0.1] = 0      # sequences with nothing
    lengths[123] = 100000                   # one sequence far longer than the median
    idx, z = _runs(lengths, D, D)
    K = len(lengths)
    chunks = [1000, 1001, 5000, 40000, 90000]  # cuts inside runs, the long one among them
    zs, cnt, st = _accumulate(hb, idx, z, K, chunks)
    assert st == 0
    want = np.zeros((K, D))
    np.add.at(want, idx, z.astype(np.float64))
    assert np.array_equal(cnt.cpu().numpy(), lengths.astype(np.float32))
    # f32 summation bound: n * eps * sum|z| per row (a loose serial-sum bound; pieces only shorten the chains)
    absum = np.zeros((K, D))
    np.add.at(absum, idx, np.abs(z.astype(np.float64)))
    err = np.abs(zs.cpu().double().numpy() - want)
    bound = (lengths[:, None] + 2) * 2.0 ** -24 * absum + 1e-30
    assert (err <= bound).all(), float((err / bound).max())
    zs2, cnt2, _ = _accumulate(hb, idx, z, K, chunks)
    assert torch.equal(zs, zs2) and torch.equal(cnt, cnt2)  # bitwise, run to run


def test_accumulate_sorted_status(hb):
    idx, z = _runs([3, 4, 5], 16, 0)
    bad = idx.copy()
    bad[5], bad[6] = 2, 0  # decreasing
    zs, cnt, st = _accumulate(hb, bad, z, 3, [])
    assert st & hb.HS_UNSORTED and float(cnt.sum()) == 0 and float(zs.abs().sum()) == 0  # nothing added
    bad2 = idx.copy()
    bad2[-1] = 99
    zs, cnt, st = _accumulate(hb, bad2, z, 3, [])
    assert st & hb.HS_BAD_IDX and float(cnt.sum()) == 0


def test_load_table(hb):
    from fhvae import FHVAE
    from hip_optim import FusedAdam

    K, D = 300, 32
    torch.manual_seed(0)
    m = FHVAE(20 * 8, [16, 16], [16, 16], 8, D, [16, 16], seg_len=20, num_seqs=K).cuda()
    opt = FusedAdam(m.parameters())
    opt.m.normal_()
    opt.v.uniform_()
    slot = [i for i, p in enumerate(opt._params) if p is m.mu2_table][0]
    off = opt.p_arena.offsets[slot]
    zs = torch.randn(K, D, device="cuda")
    cnt = torch.randint(0, 50, (K,), device="cuda").float()
    cnt[::7] = 0
    r = 0.25
    want = torch.where(cnt[:, None] > 0, zs / (cnt[:, None] + r), torch.zeros_like(zs))
    p0, m0, v0 = opt.p_arena.flat.clone(), opt.m.clone(), opt.v.clone()
    hb.mu2_load_table(zs, cnt, m.mu2_table.data, opt.m[off:off + K * D], opt.v[off:off + K * D], r)
    torch.cuda.synchronize()
    assert torch.equal(m.mu2_table.data, want)              # the torch f32 expression, bitwise
    assert (m.mu2_table.data[::7] == 0).all()
    sl = slice(off, off + K * D)
    assert (opt.m[sl] == 0).all() and (opt.v[sl] == 0).all()
    keep = torch.ones_like(p0, dtype=torch.bool)
    keep[sl] = False
    assert torch.equal(opt.p_arena.flat[keep], p0[keep]) and torch.equal(opt.m[keep], m0[keep]) and torch.equal(opt.v[keep], v0[keep])
    assert (zs == 0).all() and (cnt == 0).all()


@pytest.mark.parametrize("kind", ["fhvae_f32", "fhvae_bf16", "simple"])
def test_encode_z2_bitwise(hb, kind):
    from fhvae import FHVAE
    from simple_fhvae import SimpleFHVAE

    torch.manual_seed(1)
    if kind == "simple":
        m = SimpleFHVAE(20 * 16, [64, 64], [64, 64], 16, 16, [64, 64]).cuda()
    else:
        H = 256 if kind == "fhvae_bf16" else 64
        m = FHVAE(20 * 16, [H, H], [H, H], 16, 32, [H, H], seg_len=20, compute_dtype=kind[6:]).cuda()
    x = torch.randn(300, 20, 16, device="cuda")
    assert torch.equal(m.encode_z2(x), m.encode(x)[1])


def _setup(S=60, n=900, T=20, F=16, H=32, D=16, K=8, B=64, seed=0):
    from datasets import SyntheticSegmentPool
    from fhvae import FHVAE
    from hip_optim import FusedAdam
    from train_model import synthetic_split

    x, idx, ns = synthetic_split(n, T, F, S, seed + 1)
    pool = SyntheticSegmentPool(x, idx, ns, S, "cuda")
    torch.manual_seed(seed)
    m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=K, reference_compat=False).cuda()
    opt = FusedAdam(m.parameters())
    return m, opt, pool


def _eager_step(hb, m, opt, K):
    from train_model import loss_function

    def step(li, x, ns):
        opt.zero_grad()
        out = m(x, li, K, ns)
        loss = loss_function(out[0], out[1], 10.0)
        hb.backward(loss)
        opt.step()
        return loss.detach(), out[0].detach()
    return step


def test_block_estimate_matches_estimate_mu2_dict(hb):
    import utils
    from hierarchical import HierarchicalTrainer, plan_epoch

    K = 8
    m, opt, pool = _setup(K=K)
    tr = HierarchicalTrainer(m, opt, pool, K, 64, _eager_step(hb, m, opt, K), log=None)
    block = plan_epoch(tr.eligible, K, 0, 0)[0]
    N = tr.select(block)
    tr.estimate(N)
    tr.load()
    seg, loc = tr.seg_ids[:N], tr.local_idx[:N]

    def loader():
        for c0 in range(0, N, 100):
            yield loc[c0:c0 + 100], pool.features(seg[c0:c0 + 100]), None
    want = utils.estimate_mu2_dict(m, loader(), K)
    assert sorted(want) == list(range(K))
    for i in range(K):
        close(m.mu2_table.data[i], want[i], rtol=1e-6, what="row %d" % i)


def test_trainer_block_equals_hand_composition(hb):
    """One block of HierarchicalTrainer against the same block composed by hand from the public pieces (hs_select, encode_z2,
    mu2_accumulate_sorted, mu2_load_table, randperm with the documented generator, model() + hb.backward + optimizer.step).
    Bitwise: every step's inputs (local indices, features, nsegs) and the loaded table and moment rows.  The parameters after
    the block agree to the tolerance of tests/test_graph_step_gpu.py (f32): the training step itself sums with float atomics
    (split-K GEMMs, the table's gradient scatter), so two runs of the same steps differ in the last bits."""
    from hierarchical import HierarchicalTrainer, mu2_ratio, plan_epoch

    K, B = 8, 64
    runs = []
    for hand in (False, True):
        m, opt, pool = _setup(K=K)
        slot = [i for i, p in enumerate(opt._params) if p is m.mu2_table][0]
        off = opt.p_arena.offsets[slot]
        rows = slice(off, off + K * m.z2_dim)
        inner = _eager_step(hb, m, opt, K)
        rec = []

        def step(li, x, ns):
            if not rec:  # the state the block's first step sees: the loaded table and its cleared moments
                rec.append((m.mu2_table.data.clone(), opt.m[rows].clone(), opt.v[rows].clone()))
            rec.append((li.clone(), x.clone(), ns.clone()))
            return inner(li, x, ns)

        tr = HierarchicalTrainer(m, opt, pool, K, B, step, seed=4, chunk=100, log=None)
        block = plan_epoch(tr.eligible, K, 4, 0)[0]
        torch.manual_seed(11)  # the reparameterisation draws
        if not hand:
            tr.run_block(block)
        else:
            dev = torch.device("cuda")
            cap = tr.seg_ids.shape[0]
            seg = torch.zeros(cap, dtype=torch.int64, device=dev)
            loc = torch.zeros(cap, dtype=torch.int64, device=dev)
            n_out = torch.zeros(1, dtype=torch.int64, device=dev)
            st = torch.zeros(1, dtype=torch.int32, device=dev)
            hb.hs_select(pool.seq_ptr, torch.from_numpy(block).to(dev), seg, loc, n_out, st)
            N = int(n_out.item())
            assert int(st.item()) == 0
            zs = torch.zeros(K, m.z2_dim, device=dev)
            cnt = torch.zeros(K, device=dev)
            for c0 in range(0, N, 100):
                c1 = min(N, c0 + 100)
                hb.mu2_accumulate_sorted(m.encode_z2(pool.features(seg[c0:c1])), loc[c0:c1], zs, cnt, st)
            hb.mu2_load_table(zs, cnt, m.mu2_table.data, opt.m[rows], opt.v[rows], mu2_ratio(m))
            g = torch.Generator(device=dev)
            g.manual_seed(4)
            perm = torch.randperm(N, device=dev, generator=g)
            for s in range(0, N, B):
                sel = perm[s:s + B]
                _, x, ns = pool.batch(seg[sel])
                step(loc[sel], x, ns)
        torch.cuda.synchronize()
        runs.append((rec, opt.p_arena.flat.clone()))
    (rec_t, p_t), (rec_h, p_h) = runs
    assert len(rec_t) == len(rec_h) > 2
    for a, b in zip(rec_t, rec_h):
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    assert (rec_t[0][1] == 0).all() and (rec_t[0][2] == 0).all()
    close(p_t, p_h, rtol=1e-5, what="parameters after the block")


def test_hip_graph_across_blocks(hb):
    """train_model's --hip-graph step (captured in block 1) against eager steps over 3 blocks, with fixed draws."""
    from hierarchical import HierarchicalTrainer
    from train_model import loss_function

    K, B, D = 8, 64, 16
    ge = torch.Generator().manual_seed(5)
    eps = (torch.randn(B, D, generator=ge).cuda(), torch.randn(B, D, generator=ge).cuda())
    results = []
    for use_graph in (False, True):
        m, opt, pool = _setup(K=K, B=B, n=1200)
        losses = []

        def train_step(li, x, ns):
            opt.zero_grad()
            e = eps if x.shape[0] == B else (eps[0][:x.shape[0]], eps[1][:x.shape[0]])
            out = m(x, li, K, ns, eps=e)
            loss = loss_function(out[0], out[1], 10.0)
            hb.backward(loss)
            opt.step()
            return loss.detach(), out[0].detach()

        graph = {}

        def graph_step(li, x, ns):
            if not use_graph or x.shape[0] != B:
                out = train_step(li, x, ns)
            elif not graph:
                st = (li.clone(), x.clone(), ns.clone())
                keep = [t.clone() for t in (opt.p_arena.flat, opt.m, opt.v, opt._step_buf)]
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        train_step(*st)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    outs = train_step(*st)
                for t, k in zip((opt.p_arena.flat, opt.m, opt.v, opt._step_buf), keep):
                    t.copy_(k)
                graph.update(g=g, st=st, outs=outs)
                g.replay()
                out = outs
            else:
                for d, s in zip(graph["st"], (li, x, ns)):
                    d.copy_(s)
                graph["g"].replay()
                out = graph["outs"]
            losses.append(float(out[0]))
            return out

        tr = HierarchicalTrainer(m, opt, pool, K, B, graph_step, seed=2, log=None)
        from hierarchical import plan_epoch

        plan = plan_epoch(tr.eligible, K, 2, 0)
        assert len(plan) >= 2
        firsts = []
        for j, block in enumerate(plan[:3]):
            firsts.append(len(losses))
            tr.run_block(block, j, len(plan))
        torch.cuda.synchronize()
        results.append((opt.p_arena.flat.clone(), losses, firsts))
    (p_e, l_e, f_e), (p_g, l_g, f_g) = results
    assert f_e == f_g and len(l_e) == len(l_g)
    tol = 1e-5
    i2 = f_e[1]  # the first step of block 2: a replay of the graph captured in block 1, on the reloaded table
    assert abs(l_e[i2] - l_g[i2]) <= tol * max(1.0, abs(l_e[i2])), (l_e[i2], l_g[i2])
    for a, b in zip(l_e, l_g):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (l_e, l_g)
    close(p_g, p_e, rtol=tol, what="parameters after 3 blocks, graph vs eager")


@pytest.mark.parametrize("graph", [False, True])
def test_train_and_eval_model_hierarchical(hb, corpus, tmp_path, capsys, graph):
    import eval_model as EM
    import train_model as TM
    import utils as U

    root, _ = corpus
    exp = tmp_path / "exp"
    argv = ["--train-feat-scp", str(root / "feats.scp"), "--train-len-scp", str(root / "len.scp"), "--mvn-path",
            str(root / "mvn.json"), "--z1-hus", "16", "16", "--z2-hus", "16", "16", "--x-hus", "16", "16", "--z1-dim", "8",
            "--z2-dim", "8", "--epochs", "2", "--training-batch-size", "4", "--exp-dir", str(exp),
            "--num-hierarchical-sequences", "2"] + (["--hip-graph"] if graph else [])
    rc = TM.main(argv)
    out = capsys.readouterr().out
    assert rc == 0 and "Training complete!" in out, out
    assert out.count("hs block 1/2: 2 seqs,") == 2 and out.count("hs block 2/2: 2 seqs,") == 2, out
    lb = [float(l.split("lower bound:")[1].split()[0]) for l in out.splitlines() if "Validation set lower bound" in l]
    assert len(lb) == 2 and all(np.isfinite(lb))
    ck = torch.load(exp / "fhvae_run_e1.tar", map_location="cpu", weights_only=False)
    assert ck["hierarchical_sequences"] == 2 and tuple(ck["state_dict"]["mu2_table"].shape) == (2, 8)
    assert U.load_checkpoint_file(exp / "fhvae_run_e1.tar", finetune=True)[0].mu2_table.shape == (2, 8)
    ev = tmp_path / "ev"
    rc = EM.main(["--checkpoint", str(exp / "fhvae_run_e1.tar"), "--out", str(ev), "--feat-scp", str(root / "feats.scp"),
                  "--len-scp", str(root / "len.scp"), "--mvn-path", str(root / "mvn.json"), "--max-recon", "2"])
    assert rc == 0
    summary = json.load(open(ev / "summary.json"))
    assert np.isfinite(summary["lower_bound_per_frame"]) and summary["sequences"] == 3


def test_memory_depends_on_k_not_s(hb):
    """K = 512: the table and its moments are K x D; a block's peak memory at S = 10k and S = 100k differs only by the pool
    and seq_ptr bytes."""
    from datasets import SyntheticSegmentPool
    from fhvae import FHVAE
    from hierarchical import HierarchicalTrainer, plan_epoch
    from hip_optim import FusedAdam

    K, D, T, F, H, B, per = 512, 16, 4, 8, 32, 256, 3
    import gc

    peaks = []
    for S in (2000, 10000, 100000):  # (the first run only creates the library's lazily allocated, persistent workspaces)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base0 = torch.cuda.memory_allocated()
        idx = torch.arange(S).repeat_interleave(per)
        x = torch.randn(S * per, T, F)
        pool = SyntheticSegmentPool(x, idx, torch.full_like(idx, per), S, "cuda")
        pool_bytes = sum(t.numel() * t.element_size() for t in (pool.x, pool.seg_seq, pool.seg_nsegs, pool.seq_ptr))
        torch.manual_seed(0)
        m = FHVAE(T * F, [H, H], [H, H], D, D, [H, H], seg_len=T, num_seqs=K, reference_compat=False).cuda()
        opt = FusedAdam(m.parameters())
        assert tuple(m.mu2_table.shape) == (K, D)
        n_nets = sum(p.numel() for p in m.parameters()) - K * D
        assert opt.m.numel() <= n_nets + K * D + 64 * len(opt._params)  # the moments cover K rows, not S
        tr = HierarchicalTrainer(m, opt, pool, K, B, _eager_step(hb, m, opt, K), seed=0, log=None)
        block = plan_epoch(tr.eligible, K, 0, 0)[0]
        tr.run_block(block)  # warm-up: allocator pools, lazy workspaces (they persist into the second pool's run)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        tr.run_block(plan_epoch(tr.eligible, K, 0, 0)[1])
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base0 - pool_bytes)
        del tr, opt, m, pool
    assert abs(peaks[1] - peaks[2]) <= 1 << 20, peaks


# ---- run lengths on the thresholds of mu2_acc_sorted_kernel (64-row probe, 256-row short / long split, 32-row pieces), at
# ---- D that leave lanes of a workgroup idle (G D < 256) and at D = 256 (G = 1); select tiles with empty sequences at their edges
def _accumulate_guarded(hb, idx, z, K):
    """_accumulate in one call, with zsum / count as sub-ranges of sentinel buffers and z in front of NaN rows"""
    dev, D, N = torch.device("cuda"), z.shape[1], len(idx)
    zfull = torch.full((K + 4, D), -12345.0, device=dev)
    cfull = torch.full((K + 4,), -12345.0, device=dev)
    zs, cnt = zfull[2:K + 2], cfull[2:K + 2]
    zs.zero_()
    cnt.zero_()
    zt = torch.full((N + 3, D), float("nan"), device=dev)
    zt[:N] = torch.from_numpy(z).to(dev)
    it = torch.full((N + 3,), 1 << 62, dtype=torch.int64, device=dev)
    it[:N] = torch.from_numpy(idx).to(dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    hb.mu2_accumulate_sorted(zt[:N], it[:N], zs, cnt, st)
    for full in (zfull, cfull):
        assert (full[:2] == -12345.0).all() and (full[K + 2:] == -12345.0).all()
    return zs.clone(), cnt.clone(), int(st.item())


def _check_sorted(hb, lengths, D, seed):
    idx, z = _runs(lengths, D, seed)
    K = len(lengths)
    zs, cnt, st = _accumulate_guarded(hb, idx, z, K)
    assert st == 0
    want, absum = np.zeros((K, D)), np.zeros((K, D))
    np.add.at(want, idx, z.astype(np.float64))
    np.add.at(absum, idx, np.abs(z.astype(np.float64)))
    assert np.array_equal(cnt.cpu().numpy(), np.asarray(lengths, np.float32))
    err = np.abs(zs.cpu().double().numpy() - want)
    bound = (np.asarray(lengths)[:, None] + 2) * 2.0 ** -24 * absum + 1e-30  # as test_accumulate_sorted_oracle_and_bitwise
    share = float((err / bound).max())
    assert (err <= bound).all(), share
    zs2, cnt2, _ = _accumulate_guarded(hb, idx, z, K)
    assert torch.equal(zs, zs2) and torch.equal(cnt, cnt2)  # bitwise, run to run
    return share


@pytest.mark.parametrize("D", [24, 48, 100, 200, 256])
def test_accumulate_sorted_run_lengths_on_the_thresholds(hb, D):
    from glue_cases import sorted_run_lengths

    lengths = sorted_run_lengths()
    shares = [_check_sorted(hb, lengths, D, D),
              _check_sorted(hb, [1], D, D + 1),      # N = 1
              _check_sorted(hb, [0, 257, 0], D, D + 2)]  # N = 257 rows that all carry one index
    print("measured mu2_accumulate_sorted D=%d: worst share of the bound %.3f" % (D, max(shares)))


@pytest.mark.parametrize("K", [1024, 1025, 2049])
def test_select_empty_sequences_at_tile_edges(hb, K):
    S = 6000
    counts, ptr = _csr(S, K)
    rng = np.random.default_rng(K + 1)
    full, empty = np.flatnonzero(counts > 0), np.flatnonzero(counts == 0)
    block = rng.choice(full, size=K, replace=False)
    edges = sorted({p for p in (0, 1023, 1024, K - 1) if p < K})
    block[edges] = empty[:len(edges)]  # sequences with no segments first and last in a tile of 1024, and in the block
    want_seg = np.concatenate([np.arange(ptr[s], ptr[s + 1]) for s in block])
    want_loc = np.concatenate([np.full(counts[s], i) for i, s in enumerate(block)])
    cap = len(want_seg) + 5
    seg, loc, n, st = _select(hb, ptr, block, cap)
    assert st == 0 and n == len(want_seg)
    assert np.array_equal(seg[:n], want_seg) and np.array_equal(loc[:n], want_loc)
    assert (seg[n:] == -7).all() and (loc[n:] == -7).all()
    assert not np.isin(edges, loc[:n]).any()
